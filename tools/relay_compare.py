#!/usr/bin/env python
"""Plain BP, BP+OSD-E(10) and Relay-BP side by side on one bundled code: failures, non-converged
decodes and shots/s of the data-error shot loop (CodeSimulator_DataError's engine paths).

    python tools/relay_compare.py hgp_34_n225 0.06 250000 --steps 4 --json profiles/relay/n225.json

``p`` is EvalWER's eval_p: Pauli probabilities [p/2]*3, decoder priors p (as bench.py).  Every decoder
runs ``--warmup`` untimed and ``--steps`` timed steps of ``shots`` shots, each step ending in a device
synchronise; shots/s is shots over the median step, with the fastest and slowest step beside it.  All
decoders see the same errors (same seed and shot range).  Non-converged counts decodes (two per shot):
for BP+OSD the decodes handed to OSD, for Relay-BP the chains that found no solution.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(make_sim, run, shots, steps, warmup):
    sim = make_sim()
    for _ in range(warmup):
        run(sim, shots)
    times, fails, nonconv, iters = [], 0, 0, 0
    sim._shot_offset = 0  # every decoder's timed steps cover the same shots
    for _ in range(steps):
        t0 = time.perf_counter()
        f, nc, it = run(sim, shots)  # ends in a device synchronise
        times.append(time.perf_counter() - t0)
        fails, nonconv, iters = fails + f, nonconv + nc, iters + it
    med = statistics.median(times)
    total = shots * steps
    return {"shots": total, "failures": fails, "nonconverged_decodes": nonconv,
            "mean_iterations": iters / (2 * total) if iters else None,
            "shots_per_s": shots / med, "shots_per_s_min": shots / max(times), "shots_per_s_max": shots / min(times),
            "step_seconds": times}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("code")
    ap.add_argument("p", type=float)
    ap.add_argument("shots", type=int, help="shots per step")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--precision", type=int, default=64, choices=(32, 64))
    ap.add_argument("--max-iter-ratio", type=float, default=10, help="plain BP and BP+OSD: max_iter = N / ratio")
    ap.add_argument("--pre-iter", type=int, default=60)
    ap.add_argument("--pre-gamma", type=float, default=0.125)
    ap.add_argument("--leg-iter", type=int, default=40)
    ap.add_argument("--gamma-lo", type=float, default=-0.24)
    ap.add_argument("--gamma-hi", type=float, default=0.66)
    ap.add_argument("--gamma-seed", type=int, default=7)
    ap.add_argument("--relay", default="5,1;20,1;20,3", help="num_legs,stop_nconv settings, ';'-separated")
    ap.add_argument("--seed", type=int, default=20251020)
    ap.add_argument("--json", default=None, help="also write the results to this file")
    a = ap.parse_args()

    from qldpc_fault_tolerance_amd import codes
    from qldpc_fault_tolerance_amd.decoders import BP_Decoder_Class, BPOSD_Decoder_Class, RelayBPDecoder
    from qldpc_fault_tolerance_amd.simulators import CodeSimulator_DataError

    code = codes.get_code(a.code)
    pauli = [a.p / 2] * 3

    def sim_of(dx, dz):
        return CodeSimulator_DataError(code, dx, dz, pauli, "Total", seed=a.seed)

    def from_class(cls):
        return lambda: sim_of(cls.GetDecoder({"h": code.hz, "p_data": a.p}), cls.GetDecoder({"h": code.hx, "p_data": a.p}))

    def fused(sim, shots):
        r = sim.fused_counts(shots)
        return r.failures, int(sum(r.sector_nonconv)), int(sum(r.sector_iters))

    def bposd(sim, shots):
        f, _, osd_n = sim.bposd_counts(shots)
        return f, osd_n, 0

    mi = int(code.N / a.max_iter_ratio)
    rows = [(f"plain BP({mi})", from_class(BP_Decoder_Class(a.max_iter_ratio, "minimum_sum", 0.625, a.precision)), fused),
            (f"BP({mi})+OSD-E(10)", from_class(BPOSD_Decoder_Class(a.max_iter_ratio, "minimum_sum", 0.625, "osd_e", 10,
                                                                  a.precision)), bposd)]
    geometry = {}
    for setting in a.relay.split(";"):
        legs, stop = (int(v) for v in setting.split(","))

        def make(legs=legs, stop=stop):
            kw = dict(pre_iter=a.pre_iter, pre_gamma=a.pre_gamma, num_legs=legs, leg_iter=a.leg_iter,
                      gamma_interval=(a.gamma_lo, a.gamma_hi), stop_nconv=stop, gamma_seed=a.gamma_seed,
                      ms_scaling_factor=0.625, precision=a.precision)
            dx = RelayBPDecoder(code.hz, a.p, **kw)
            dz = RelayBPDecoder(code.hx, a.p, **kw)
            g = dx.decoder.geometry()
            geometry.update({k: g[k] for k in ("threads", "lds_bytes", "blocks_per_cu")})
            return sim_of(dx, dz)

        rows.append((f"Relay-BP T0={a.pre_iter} R={legs} Tr={a.leg_iter} S={stop}", make, fused))

    out = {"code": a.code, "eval_p": a.p, "precision": a.precision, "shots_per_step": a.shots, "steps": a.steps,
           "warmup": a.warmup, "relay_gamma": [a.pre_gamma, a.gamma_lo, a.gamma_hi, a.gamma_seed], "decoders": {}}
    print(f"{a.code} eval_p={a.p} fp{a.precision}: {a.steps} steps of {a.shots} shots (+{a.warmup} warm-up)")
    print(f"{'decoder':<34}{'failures':>10}{'non-conv':>10}{'mean it':>9}{'shots/s':>12}   (slowest .. fastest step)")
    for name, make, run in rows:
        r = measure(make, run, a.shots, a.steps, a.warmup)
        out["decoders"][name] = r
        it = f"{r['mean_iterations']:.1f}" if r["mean_iterations"] else "n/a"
        print(f"{name:<34}{r['failures']:>10}{r['nonconverged_decodes']:>10}{it:>9}{r['shots_per_s']:>12.0f}"
              f"   ({r['shots_per_s_min']:.0f} .. {r['shots_per_s_max']:.0f})")
    out["relay_geometry"] = geometry
    print("relay kernel geometry (hz sector):", geometry)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

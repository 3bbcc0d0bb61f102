#!/usr/bin/env python
"""The flooding and the serial BP schedule side by side on one bundled code, as plain BP and as
BP+OSD-E(10): failures, non-converged decodes, mean iterations and shots/s of the data-error shot loop
(CodeSimulator_DataError's engine paths).

    python tools/schedule_compare.py hgp_34_n225 0.06 250000 --steps 4 --json profiles/serial/n225_p006.json

``p`` is EvalWER's eval_p: Pauli probabilities [p/2]*3, decoder priors p (as bench.py).  Three
configurations per decoder: flooding at max_iter = N / ratio, serial at max_iter and serial at
max_iter // 2.  Every configuration runs ``--warmup`` untimed and ``--steps`` timed steps of ``shots``
shots, each step ending in a device synchronise; shots/s is shots over the median step, with the
slowest and fastest step beside it.  All configurations see the same errors (same seed and shot
range).  Non-converged counts decodes (two per shot): for BP+OSD the decodes handed to OSD.  Flooding
BP runs the fused engine-3 loop and flooding BP+OSD the device-resident loop; serial BP runs the
staged pipeline and serial BP+OSD the host-assisted loop.
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
    sim.rewind_shots()  # every configuration's timed steps cover the same shots
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
    ap.add_argument("--max-iter-ratio", type=float, default=10, help="max_iter = N / ratio")
    ap.add_argument("--only", default="bp,bposd", help="which decoders to run: bp, bposd or both")
    ap.add_argument("--seed", type=int, default=20251020)
    ap.add_argument("--json", default=None, help="also write the results to this file")
    a = ap.parse_args()

    from qldpc_fault_tolerance_amd import codes
    from qldpc_fault_tolerance_amd.decoders import BPDecoder, BPOSD_Decoder
    from qldpc_fault_tolerance_amd.simulators import CodeSimulator_DataError

    code = codes.get_code(a.code)
    import numpy as np

    pauli = [a.p / 2] * 3
    probs = a.p * np.ones(code.N)
    mi = int(code.N / a.max_iter_ratio)
    geometry = {}

    def bp_sim(schedule, max_iter):
        def make():
            dx, dz = (BPDecoder(h, probs, max_iter, "minimum_sum", 0.625, precision=a.precision, schedule=schedule)
                      for h in (code.hz, code.hx))
            if schedule == "serial":
                g = dx.decoder.geometry()
                geometry.update({k: g[k] for k in ("threads", "lds_bytes", "blocks_per_cu")})
            return CodeSimulator_DataError(code, dx, dz, pauli, "Total", seed=a.seed)
        return make

    def bposd_sim(schedule, max_iter):
        def make():
            dx, dz = (BPOSD_Decoder(h, probs, max_iter, "minimum_sum", 0.625, "osd_e", 10, precision=a.precision,
                                    schedule=schedule) for h in (code.hz, code.hx))
            return CodeSimulator_DataError(code, dx, dz, pauli, "Total", seed=a.seed)
        return make

    def fused(sim, shots):
        r = sim.fused_counts(shots)
        return r.failures, int(sum(r.sector_nonconv)), int(sum(r.sector_iters))

    def bposd(sim, shots):
        f, _, osd_n = sim.bposd_counts(shots)
        return f, osd_n, 0

    configs = [("flooding", "parallel", mi), ("serial", "serial", mi), ("serial", "serial", max(1, mi // 2))]
    rows = []
    if "bp" in a.only.split(","):
        rows += [(f"BP {name}({it})", bp_sim(sched, it), fused) for name, sched, it in configs]
    if "bposd" in a.only.split(","):
        rows += [(f"BP {name}({it})+OSD-E(10)", bposd_sim(sched, it), bposd) for name, sched, it in configs]

    out = {"code": a.code, "eval_p": a.p, "precision": a.precision, "shots_per_step": a.shots, "steps": a.steps,
           "warmup": a.warmup, "edges": [int(code.csr("hz").nnz), int(code.csr("hx").nnz)], "decoders": {}}
    print(f"{a.code} eval_p={a.p} fp{a.precision}: {a.steps} steps of {a.shots} shots (+{a.warmup} warm-up)")
    print(f"{'decoder':<30}{'failures':>10}{'non-conv':>10}{'mean it':>9}{'shots/s':>12}   (slowest .. fastest step)")
    for name, make, run in rows:
        r = measure(make, run, a.shots, a.steps, a.warmup)
        out["decoders"][name] = r
        it = f"{r['mean_iterations']:.1f}" if r["mean_iterations"] else "n/a"
        print(f"{name:<30}{r['failures']:>10}{r['nonconverged_decodes']:>10}{it:>9}{r['shots_per_s']:>12.0f}"
              f"   ({r['shots_per_s_min']:.0f} .. {r['shots_per_s_max']:.0f})", flush=True)
    out["serial_geometry"] = geometry
    out["serial_env"] = {k: v for k, v in os.environ.items() if k.startswith("QLDPC_SERIAL")}
    print("serial kernel geometry (hz sector):", geometry)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

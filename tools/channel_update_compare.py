#!/usr/bin/env python
"""Independent sectors and X/Z-correlated decoding (``channel_update``) side by side on one bundled
code, on the same Philox errors: failures, non-converged decodes and mean iterations per sector, and
shots/s of the data-error shot loop (CodeSimulator_DataError's engine paths).

    python tools/channel_update_compare.py hgp_34_n225 0.06 250000 --steps 4 --json profiles/side/n225_p006.json

``p`` is EvalWER's eval_p: Pauli probabilities [p/2]*3, decoder priors p (as bench.py and
tools/schedule_compare.py).  Five configurations, flooding min-sum at max_iter = N / ratio unless said:
independent sectors on the fused engine-3 loop; independent sectors on engine 7 without memory or legs
through the staged pipeline (the same law: its failure count must equal the engine-3 line's, asserted);
``x->z`` and ``z->x`` on engine 7 (the first sector as in the independent line, the second with the
conditional priors as side tables); ``x->z`` with the serial schedule (engine 8).  Every configuration
runs ``--warmup`` untimed and ``--steps`` timed steps of ``shots`` shots, each step ending in a device
synchronise; shots/s is shots over the median step, with the slowest and fastest step beside it.  One
JSON line per configuration goes to stdout.

Four BP+OSD lines follow on the same errors (OSD-E(10) behind the same flooding min-sum; ``--no-bposd``
leaves them out): independent sectors on the fused engine-3 BP+OSD loop (``qldpc_mc_set_osd``);
independent sectors on engine 7 through the staged loop with the GPU OSD behind each sector's soft BP
(``qldpc_mc_set_staged_osd``; the same law: its failure count must equal the fused line's, asserted);
``x->z`` and ``z->x`` BP+OSD (the second sector's BP and OSD under the conditional priors).  Their
``nonconverged_decodes`` are the decodes handed to OSD per sector.

Two more lines give the cost of the side selection alone, per engine: one handle decodes the X-sector
syndromes of 65,536 sampled shots plainly and as a side decode with ``p0 = p1`` = its own prior under
random side bytes, so both run the same iterations bit for bit (asserted) and differ only in the
per-syndrome side read and the two-row table; the two alternate ``--steps`` times after ``--warmup``.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(sim, shots, steps, warmup, run=None):
    """``run(shots)``: one step's MCResult (default: ``sim.fused_counts``)."""
    run = run or sim.fused_counts
    for _ in range(warmup):
        run(shots)
    sim.rewind_shots()  # every configuration's timed steps cover the same shots
    times, fails, nonconv, iters, decodes = [], 0, [0, 0], [0, 0], [0, 0]
    for _ in range(steps):
        t0 = time.perf_counter()
        r = run(shots)  # ends in a device synchronise
        times.append(time.perf_counter() - t0)
        fails += r.failures
        for q in range(2):
            nonconv[q] += int(r.sector_nonconv[q])
            iters[q] += int(r.sector_iters[q])
            decodes[q] += int(r.sector_decodes[q])
    med = statistics.median(times)
    return {"shots": shots * steps, "failures": fails, "nonconverged_decodes": nonconv,
            "mean_iterations": [iters[q] / decodes[q] if decodes[q] else None for q in range(2)],
            "shots_per_s": shots / med, "shots_per_s_min": shots / max(times), "shots_per_s_max": shots / min(times),
            "step_seconds": times}


def side_decode_cost(code, probs, pauli, mi, precision, seed, steps, warmup, serial):
    """Median seconds of a plain decode and of the bit-identical side decode of the same syndromes."""
    import numpy as np

    from qldpc_fault_tolerance_amd.engine import DeviceBP, RelayParams, _torch, sample_errors
    from qldpc_fault_tolerance_amd.simulators import gf2_rows

    torch = _torch()
    H = code.csr("hz")
    B = 65536
    err = sample_errors(code.N, *pauli, seed, 0, B).cpu().numpy()
    kw = dict(max_iter=mi, schedule="serial") if serial else dict(relay=RelayParams(pre_iter=mi, pre_gamma=0.0, num_legs=0))
    dec = DeviceBP(H, probs, ms_scaling_factor=0.625, precision=precision, **kw)
    dec.set_side_probs(probs, probs)
    dev = torch.device("cuda", dec.graph.device)
    synd = torch.from_numpy(gf2_rows(H, err & 1)).to(dev)
    side = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (B, H.n)).astype(np.uint8)).to(dev)
    out = [torch.empty((B, H.n), dtype=torch.uint8, device=dev) for _ in range(2)]
    iters = [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2)]
    times = ([], [])
    for step in range(warmup + steps):
        for k, sb in enumerate((None, side)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            dec.decode_batch_device(synd, out[k], iters[k], None, side=sb)
            torch.cuda.synchronize(dev)
            if step >= warmup:
                times[k].append(time.perf_counter() - t0)
    assert torch.equal(out[0], out[1]) and torch.equal(iters[0], iters[1]), "p0 = p1: the two decodes must agree"
    plain, sided = statistics.median(times[0]), statistics.median(times[1])
    return {"syndromes": B, "mean_iterations": float(iters[0].double().mean()), "plain_seconds": plain,
            "side_seconds": sided, "side_over_plain": sided / plain, "plain_step_seconds": times[0],
            "side_step_seconds": times[1]}


def bposd_lines(a, code, pauli, probs, mi, out, BPOSD_Decoder, CodeSimulator_DataError, channel_update_probs,
                DeviceBP, DeviceMC, DeviceOSD, RelayParams):
    """The four BP+OSD configurations, on the Philox errors of the BP lines."""
    def bposd(h, side_probs=None):
        return BPOSD_Decoder(h, probs, mi, "minimum_sum", 0.625, "osd_e", a.osd_order, precision=a.precision,
                             side_probs=side_probs)

    def emit(name, r):
        out["configurations"][name] = r
        print(json.dumps({"configuration": name, "code": a.code, "eval_p": a.p, **r}), flush=True)

    # independent, fused engine-3 loop (bposd_counts' device path; its counters stay in last_result)
    sim = CodeSimulator_DataError(code, bposd(code.hz), bposd(code.hx), pauli, "Total", seed=a.seed)

    def fused(shots):
        sim.bposd_counts(shots)
        return sim.last_result

    emit("independent BP+OSD engine 3 (fused)", measure(sim, a.shots, a.steps, a.warmup, fused))
    # independent, staged loop: engine 7 without memory or legs, the GPU OSD behind each sector
    relay = RelayParams(pre_iter=mi, pre_gamma=0.0, num_legs=0)
    dx = DeviceBP(code.csr("hz"), probs, ms_scaling_factor=0.625, precision=a.precision, relay=relay)
    dz = DeviceBP(code.csr("hx"), probs, ms_scaling_factor=0.625, precision=a.precision, relay=relay)
    mc = DeviceMC(code, dx, dz, staged=True)
    mc.set_staged_osd(DeviceOSD(dx.graph, probs, "osd_e", a.osd_order), DeviceOSD(dz.graph, probs, "osd_e", a.osd_order))
    sim = CodeSimulator_DataError(code, bposd(code.hz), bposd(code.hx), pauli, "Total", seed=a.seed)

    def staged(shots):
        return sim._fused_run(lambda: mc, shots, lambda loop, b, c, cnt: loop.launch(*pauli, sim.seed, b, c, "Total", cnt))

    emit("independent BP+OSD engine 7 (staged)", measure(sim, a.shots, a.steps, a.warmup, staged))
    f3, f7 = (out["configurations"][k]["failures"] for k in ("independent BP+OSD engine 3 (fused)",
                                                              "independent BP+OSD engine 7 (staged)"))
    assert f3 == f7, f"same errors, same law: the fused BP+OSD loop counted {f3} failures, the staged one {f7}"
    for direction in ("x->z", "z->x"):
        _, p0, p1 = channel_update_probs(*pauli, direction)
        x_first = direction == "x->z"
        sim = CodeSimulator_DataError(code, bposd(code.hz, None if x_first else (p0, p1)),
                                      bposd(code.hx, (p0, p1) if x_first else None), pauli, "Total", seed=a.seed,
                                      channel_update=direction)
        emit(f"{direction} BP+OSD engine 7", measure(sim, a.shots, a.steps, a.warmup))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("code")
    ap.add_argument("p", type=float)
    ap.add_argument("shots", type=int, help="shots per step")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--precision", type=int, default=64, choices=(32, 64))
    ap.add_argument("--max-iter-ratio", type=float, default=10, help="max_iter = N / ratio")
    ap.add_argument("--seed", type=int, default=20251021)
    ap.add_argument("--osd-order", type=int, default=10, help="order of the BP+OSD lines' OSD-E")
    ap.add_argument("--no-bposd", action="store_true", help="leave the BP+OSD lines out")
    ap.add_argument("--json", default=None, help="also write the results to this file")
    a = ap.parse_args()

    import numpy as np

    from qldpc_fault_tolerance_amd import codes
    from qldpc_fault_tolerance_amd.decoders import BPDecoder, BPOSD_Decoder, RelayBPDecoder, channel_update_probs
    from qldpc_fault_tolerance_amd.engine import DeviceBP, DeviceMC, DeviceOSD, RelayParams
    from qldpc_fault_tolerance_amd.simulators import CodeSimulator_DataError

    code = codes.get_code(a.code)
    pauli = [a.p / 2] * 3
    probs = a.p * np.ones(code.N)
    mi = int(code.N / a.max_iter_ratio)

    def flooding(h):
        return BPDecoder(h, probs, mi, "minimum_sum", 0.625, precision=a.precision)

    def engine7(h):  # plain min-sum on the relay engine: no memory, no legs
        return RelayBPDecoder(h, probs, mi, pre_gamma=0.0, num_legs=0, ms_scaling_factor=0.625, precision=a.precision)

    def serial(h):
        return BPDecoder(h, probs, mi, "minimum_sum", 0.625, precision=a.precision, schedule="serial")

    configs = [("independent engine 3 (fused)", flooding, None), ("independent engine 7 (staged)", engine7, None),
               ("x->z engine 7", engine7, "x->z"), ("z->x engine 7", engine7, "z->x"),
               ("x->z serial (engine 8)", serial, "x->z")]
    out = {"code": a.code, "eval_p": a.p, "precision": a.precision, "max_iter": mi, "shots_per_step": a.shots,
           "steps": a.steps, "warmup": a.warmup, "configurations": {}}
    for name, make, direction in configs:
        sim = CodeSimulator_DataError(code, make(code.hz), make(code.hx), pauli, "Total", seed=a.seed,
                                      channel_update=direction)
        r = measure(sim, a.shots, a.steps, a.warmup)
        out["configurations"][name] = r
        print(json.dumps({"configuration": name, "code": a.code, "eval_p": a.p, **r}), flush=True)
    e3, e7 = (out["configurations"][k]["failures"] for k in ("independent engine 3 (fused)",
                                                              "independent engine 7 (staged)"))
    assert e3 == e7, f"same errors, same law: engine 3 counted {e3} failures, engine 7 {e7}"
    if not a.no_bposd:
        bposd_lines(a, code, pauli, probs, mi, out, BPOSD_Decoder, CodeSimulator_DataError, channel_update_probs,
                    DeviceBP, DeviceMC, DeviceOSD, RelayParams)
    out["side_decode_cost"] = {}
    for name, is_serial in (("engine 7", False), ("engine 8", True)):
        r = side_decode_cost(code, probs, pauli, mi, a.precision, a.seed, a.steps, a.warmup, is_serial)
        out["side_decode_cost"][name] = r
        print(json.dumps({"configuration": f"side decode cost, {name}", "code": a.code, "eval_p": a.p, **r}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Failure spectrum of a bundled code: failures at fixed error weight, and the weight-stratified
logical / word error rate beside a direct Monte Carlo estimate.

    python tools/failure_spectrum.py --code hgp_34_n225 --p 0.06 --shots-per-weight 4096

``--p`` is the total Pauli error rate px + py + pz (px = py = pz = p / 3); the decoders are min-sum
BP with priors 2p/3 and max_iter = n / 10, as CodeFamily.EvalWER builds them.  ``--weights a,b,...``
replaces the default window (all weights that leave at most ``--tail`` of the binomial weight
distribution uncovered).  The direct side runs ``--direct-shots`` i.i.d. shots through the same staged
pipeline (``DeviceMC(..., staged=True).run``), so one kernel trace of this tool,

    rocprofv3 --kernel-trace --stats -- python tools/failure_spectrum.py ...

holds both samplers: ``wt_sample`` (fixed weight) and ``ph_sample`` (i.i.d.).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from qldpc_fault_tolerance_amd import codes, decoders, simulators  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--code", default="hgp_34_n225")
    ap.add_argument("--p", type=float, required=True, help="total Pauli error rate px + py + pz")
    ap.add_argument("--shots-per-weight", type=int, required=True)
    ap.add_argument("--weights", default="", help="comma-separated weights (default: the --tail window)")
    ap.add_argument("--tail", type=float, default=1e-12)
    ap.add_argument("--direct-shots", type=int, default=-1, help="i.i.d. shots (default: as many as the spectrum)")
    ap.add_argument("--eval-logical-type", default="Total", choices=["X", "Z", "Total"])
    ap.add_argument("--precision", type=int, default=64, choices=[32, 64])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=1,
                    help="timed repetitions of both sides, alternating, on fresh shot ranges (rates: the median)")
    ap.add_argument("--json", default="", help="also write the numbers to this file")
    a = ap.parse_args()

    import torch

    code = codes.get_code(a.code)
    n, K = code.N, code.K
    probs = [a.p / 3] * 3
    cls = decoders.BP_Decoder_Class(10, "minimum_sum", 0.625, precision=a.precision)
    dx = cls.GetDecoder({"h": code.hz, "p_data": 2 * a.p / 3})
    dz = cls.GetDecoder({"h": code.hx, "p_data": 2 * a.p / 3})
    sim = simulators.CodeSimulator_DataError(code, dx, dz, probs, a.eval_logical_type, seed=a.seed)
    if a.weights:
        weights = [int(w) for w in a.weights.split(",")]
    else:
        lo, hi = simulators.stratified_window(n, a.p, a.tail)
        weights = list(range(lo, hi + 1))
    S = a.shots_per_weight

    nd = a.direct_shots if a.direct_shots >= 0 else S * len(weights)
    sim.FailureSpectrum(weights[:1], min(S, 64))  # warm-up: handle, buffers, kernels loaded
    mc = sim._mc_staged
    if nd > 0:
        mc.run(*probs, seed=a.seed, shot_begin=1 << 48, shot_count=64, logical_mode=a.eval_logical_type)
    torch.cuda.synchronize()
    tw, td = [], []
    fails = shots = r = None
    for i in range(max(1, a.repeats)):  # the first repetition's counts are the ones reported
        t0 = time.perf_counter()
        f_i, s_i = sim.FailureSpectrum(weights, S)  # (synchronizes)
        tw.append(time.perf_counter() - t0)
        if fails is None:
            fails, shots = f_i, s_i
        if nd > 0:
            t0 = time.perf_counter()
            r_i = mc.run(*probs, seed=a.seed, shot_begin=(1 << 50) + i * nd, shot_count=nd,
                         logical_mode=a.eval_logical_type)
            td.append(time.perf_counter() - t0)
            r = r or r_i
    t_w = float(np.median(tw))
    d = simulators.stratified_word_error_rate(a.p, n, K, weights, fails, shots)

    direct = None
    if nd > 0:
        t_d = float(np.median(td))
        ler = r.failures / r.shots
        wer, wer_eb = simulators.word_error_rate(r.failures, r.shots, K)
        direct = {"shots": r.shots, "failures": r.failures, "ler": ler,
                  "ler_eb": float(np.sqrt(ler * (1 - ler) / r.shots)), "wer": float(wer), "wer_eb": float(wer_eb),
                  "seconds": t_d, "shots_per_s": r.shots / t_d, "seconds_all": td}

    print(f"{a.code}: n = {n}, K = {K}, p_tot = {a.p}, fp{a.precision}, {a.eval_logical_type}")
    print(f"{'w':>6} {'Binom(w)':>12} {'fails':>10} {'shots':>10} {'f(w)':>10}")
    for w, B, f, s in zip(d["weights"], d["pmf"], d["fails"], d["shots"]):
        print(f"{w:6d} {B:12.4e} {f:10d} {s:10d} {f / s:10.3e}")
    print(f"stratified: LER = {d['ler']:.6e} +- {d['ler_eb']:.2e}  (uncovered {d['uncovered']:.2e}, "
          f"upper {d['ler_upper']:.6e})  WER = {d['wer']:.6e} +- {d['wer_eb']:.2e}")
    print(f"            lowest failing weight: {d['min_failing_weight']}")
    tot = int(np.sum(shots))
    print(f"            {tot} shots in {t_w:.3f} s = {tot / t_w:.4g} shots/s"
          + (f"  (median of {len(tw)}: {min(tw):.3f} .. {max(tw):.3f} s)" if len(tw) > 1 else ""))
    if direct:
        print(f"direct:     LER = {direct['ler']:.6e} +- {direct['ler_eb']:.2e}  WER = {direct['wer']:.6e} +- "
              f"{direct['wer_eb']:.2e}")
        print(f"            {direct['failures']} failures in {direct['shots']} shots, {direct['seconds']:.3f} s = "
              f"{direct['shots_per_s']:.4g} shots/s"
              + (f"  (median of {len(td)}: {min(td):.3f} .. {max(td):.3f} s)" if len(td) > 1 else ""))
    if a.json:
        out = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
        out.update(code=a.code, precision=a.precision, seconds=t_w, shots_per_s=tot / t_w, seconds_all=tw,
                   direct=direct)
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()

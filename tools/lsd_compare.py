#!/usr/bin/env python
"""Plain BP, BP+OSD-0, BP+OSD-E(10), BP+OSD-CS(10), BP+LSD of order 0 (bits_per_step 1, 2, 3) and of higher
order (bits_per_step 1 with lsd_e 2, lsd_e 4, lsd_cs 4, lsd_cs 8) side by side on one bundled code:
failures, decodes handed to the second stage and shots/s of the data-error shot loop, plus a probe of
the second stage alone (its kernel time on one batch, and for LSD the mean rounds and active columns
and the decodes that outgrew the LDS image and ran again on the HBM slice).

    python tools/lsd_compare.py hgp_34_n1600 0.04 250000 --steps 4 --json profiles/lsd/lsd_n1600_p004.json

The protocol is tools/relay_compare.py's: ``p`` is EvalWER's eval_p (Pauli probabilities [p/2]*3, decoder
priors p), every decoder runs ``--warmup`` untimed and ``--steps`` timed steps of ``shots`` shots, each
step ending in a device synchronise; shots/s is shots over the median step.  All decoders see the same
errors.  The probe decodes the X sector of the first ``--probe`` shots: soft BP once, then the stage's
launch over the whole batch timed with device events (one warm-up, median of 5); the time is for the
batch's handed decodes together, one persistent launch.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from relay_compare import measure  # noqa: E402  (the shared timing protocol)


def probe(code, dec, pauli, seed, count):
    """Second-stage kernel time and statistics of decoder ``dec`` (on hz) over ``count`` sampled shots."""
    import numpy as np
    import torch

    from qldpc_fault_tolerance_amd import engine
    from qldpc_fault_tolerance_amd.simulators import gf2_rows

    err = engine.sample_errors(code.N, *pauli, seed, 0, count).cpu().numpy()
    synd = gf2_rows(code.csr("hz"), (err & 1).astype(np.uint8))
    _, dev, sd, corr, iters, conv = engine._decode_buffers(dec.decoder.graph, synd)
    st = engine._stream_handle(torch, dev)
    post = dec.decoder._decode_soft_device(sd, corr, iters, conv, st)
    o0, ow = torch.empty_like(corr), torch.empty_like(corr)
    times = []
    for _ in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dec.gpu_osd.decode_device(sd, post, conv, corr, o0, ow, st)
        b.record()
        torch.cuda.synchronize(dev)
        times.append(a.elapsed_time(b))
    handed = int((conv == 0).sum().item())
    out = {"probe_shots": count, "probe_handed": handed, "stage_ms": statistics.median(times[1:]),
           "stage_us_per_handed_decode": 1e3 * statistics.median(times[1:]) / max(handed, 1),
           "geometry": dec.gpu_osd.geometry()}
    if hasattr(dec.gpu_osd, "decode_device_stats"):
        stats = torch.zeros((count, 4), dtype=torch.int32, device=dev)
        dec.gpu_osd.retries()  # clear: the count below is of one launch
        dec.gpu_osd.decode_device_stats(sd, post, conv, corr, ow, stats, st)
        torch.cuda.synchronize(dev)
        s = stats.cpu().numpy()[conv.cpu().numpy() == 0]
        out.update(mean_rounds=float(s[:, 1].mean()), mean_active_columns=float(s[:, 2].mean()),
                   max_active_columns=int(s[:, 2].max()), mean_clusters=float(s[:, 3].mean()),
                   retried_on_hbm=dec.gpu_osd.retries())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("code")
    ap.add_argument("p", type=float)
    ap.add_argument("shots", type=int, help="shots per step")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--precision", type=int, default=64, choices=(32, 64))
    ap.add_argument("--max-iter-ratio", type=float, default=10, help="max_iter = N / ratio")
    ap.add_argument("--probe", type=int, default=16384, help="shots of the second-stage probe")
    ap.add_argument("--seed", type=int, default=20251020)
    ap.add_argument("--json", default=None, help="also write the results to this file")
    a = ap.parse_args()

    from qldpc_fault_tolerance_amd import codes
    from qldpc_fault_tolerance_amd.decoders import BP_Decoder_Class, BPLSD_Decoder_Class, BPOSD_Decoder_Class
    from qldpc_fault_tolerance_amd.simulators import CodeSimulator_DataError

    code = codes.get_code(a.code)
    pauli = [a.p / 2] * 3
    made = {}

    def from_class(name, cls):
        def make():
            dx, dz = cls.GetDecoder({"h": code.hz, "p_data": a.p}), cls.GetDecoder({"h": code.hx, "p_data": a.p})
            made[name] = dx
            return CodeSimulator_DataError(code, dx, dz, pauli, "Total", seed=a.seed)
        return make

    def fused(sim, shots):
        r = sim.fused_counts(shots)
        return r.failures, int(sum(r.sector_nonconv)), int(sum(r.sector_iters))

    def second(sim, shots):
        f, _, handed = sim.bposd_counts(shots)
        return f, handed, 0

    mi = int(code.N / a.max_iter_ratio)
    r, ms, al, pr = a.max_iter_ratio, "minimum_sum", 0.625, a.precision
    rows = [(f"plain BP({mi})", BP_Decoder_Class(r, ms, al, pr), fused),
            (f"BP({mi})+OSD-0", BPOSD_Decoder_Class(r, ms, al, "osd_0", 0, pr), second),
            (f"BP({mi})+OSD-E(10)", BPOSD_Decoder_Class(r, ms, al, "osd_e", 10, pr), second),
            (f"BP({mi})+OSD-CS(10)", BPOSD_Decoder_Class(r, ms, al, "osd_cs", 10, pr), second)]
    rows += [(f"BP({mi})+LSD k={k}", BPLSD_Decoder_Class(r, ms, al, k, pr), second) for k in (1, 2, 3)]
    rows += [(f"BP({mi})+LSD k=1 {meth} {w}",
              BPLSD_Decoder_Class(r, ms, al, 1, pr, lsd_method=meth, lsd_order=w), second)
             for meth, w in (("lsd_e", 2), ("lsd_e", 4), ("lsd_cs", 4), ("lsd_cs", 8))]
    out = {"code": a.code, "eval_p": a.p, "precision": a.precision, "shots_per_step": a.shots, "steps": a.steps,
           "warmup": a.warmup, "decoders": {}}
    print(f"{a.code} eval_p={a.p} fp{a.precision}: {a.steps} steps of {a.shots} shots (+{a.warmup} warm-up); "
          f"stage probe on {a.probe} shots (X sector)")
    print(f"{'decoder':<26}{'failures':>9}{'handed':>9}{'shots/s':>11}  {'(slowest .. fastest)':<22}"
          f"{'stage ms':>9}{'us/decode':>10}{'rounds':>8}{'|A|':>8}{'retried':>9}")
    for name, cls, run in rows:
        res = measure(from_class(name, cls), run, a.shots, a.steps, a.warmup)
        if run is second:
            res["stage"] = probe(code, made[name], pauli, a.seed, a.probe)
        out["decoders"][name] = res
        s = res.get("stage", {})
        fmt = lambda v, f: format(v, f) if v is not None else "n/a"  # noqa: E731
        print(f"{name:<26}{res['failures']:>9}{res['nonconverged_decodes']:>9}{res['shots_per_s']:>11.0f}  "
              f"({res['shots_per_s_min']:.0f} .. {res['shots_per_s_max']:.0f})".ljust(79) +
              f"{fmt(s.get('stage_ms'), '9.3f'):>9}{fmt(s.get('stage_us_per_handed_decode'), '10.2f'):>10}"
              f"{fmt(s.get('mean_rounds'), '8.1f'):>8}{fmt(s.get('mean_active_columns'), '8.1f'):>8}"
              f"{fmt(s.get('retried_on_hbm'), 'd'):>9}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

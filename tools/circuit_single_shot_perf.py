"""Throughput of the single-shot circuit loop (CodeSimulator_Circuit.WordErrorRate) in the Threshold
notebook's HGP circuit-threshold configuration, on one GPU.

    python tools/circuit_single_shot_perf.py [--codes hgp_34_n225,hgp_34_n625] [--cycles 3,21] [--p 2e-3]
        [--samples 1048576] [--repeats 5] [--loop single_shot|space_time] [--dem-only] [--out FILE]

CX noise only (p_CX = p), coloration schedule; decoder1 = min-sum BP (alpha 0.625, max_iter N/30) on
[hx | I] with the notebook's priors p_data = 3 * 6 * (8/15) p, p_synd = 7 * (8/15) p; decoder2 =
BP + OSD-E(10), max_iter N/10, prior p.  Per (code, num_cycles): the host-side circuit + DEM build
time, one warm-up run of the same size, then ``--repeats`` timed ``WordErrorRate(samples)`` calls (each
ends in a device synchronise; the loop runs the samples in batches of 65536); one JSON line with the
median, the spread and the counters.

``--loop space_time`` runs ``CodeSimulator_Circuit_SpaceTime`` (num_rep 1) on the same code and noise
with decoders on its fault hypergraphs: the loop whose cs_unpack + cs_apply the step kernel replaces,
for the kernel-trace comparison.  The bundled HGP codes' fault hypergraphs have column degrees past
what the BP engines take (QLDPC_ENOTSUP), so that comparison runs on ``toric_d3`` (hgp(ring 3, ring 3)).
``--dem-only`` stops after the DEM build (needs no GPU).

Kernel split: run it with ``--repeats 1`` under ``rocprofv3 --kernel-trace --stats`` (a run of its
own, no counters) and summarise with tools/rocpd_stats.py.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qldpc_fault_tolerance_amd import codes  # noqa: E402

ALPHA = 0.625


def _ring(d):
    h = np.zeros((d, d), np.uint8)
    for i in range(d):
        h[i, i] = h[i, (i + 1) % d] = 1
    return h


def build(name, cycles, p, loop):
    from qldpc_fault_tolerance_amd import simulators as S

    code = codes.hgp(_ring(3), _ring(3)) if name == "toric_d3" else codes.get_code(name)
    ep = {"p_i": 0.0, "p_state_p": 0.0, "p_m": 0.0, "p_CX": p, "p_idling_gate": 0.0}
    t0 = time.perf_counter()
    if loop == "single_shot":
        sim = S.CodeSimulator_Circuit(code=code, p=p, num_cycles=cycles, error_params=ep, seed=1)
        sim._generate_circuit()
    else:
        sim = S.CodeSimulator_Circuit_SpaceTime(code=code, p=p, num_cycles=cycles, num_rep=1, error_params=ep, seed=1)
        sim._generate_circuit()
        sim._generate_circuit_graph()
    return code, sim, time.perf_counter() - t0


def decoders(code, sim, p, loop):
    from qldpc_fault_tolerance_amd import _native
    from qldpc_fault_tolerance_amd import decoders as D

    n = code.N
    if loop == "single_shot":
        hx = sim.eval_code.hx
        m = hx.shape[0]
        p1 = np.hstack([3 * 6 * (8 / 15) * p * np.ones(n), 7 * (8 / 15) * p * np.ones(m)])
        sim.decoder1_z = D.BPDecoder(sim.hx_ext, p1, n / 30, "minimum_sum", ALPHA)
        sim.decoder2_z = D.BPOSD_Decoder(hx, p * np.ones(n), n / 10, "minimum_sum", ALPHA, "osd_e", 10)
    else:
        g = sim.circuit_graph
        sim.decoder1_z = D.ST_BP_Decoder_Circuit(g["h1"], g["channel_ps1"], int(n / 30), "minimum_sum", ALPHA)
        try:
            sim.decoder2_z = D.ST_BPOSD_Decoder_Circuit(g["h2"], g["channel_ps2"], n / 10, "minimum_sum", ALPHA, "osd_e",
                                                        10)
        except _native.QldpcError as e:  # soft BP does not take h2's column degrees: plain BP, said in the record
            if e.rc != _native.ENOTSUP:
                raise
            sim.decoder2_z = D.ST_BP_Decoder_Circuit(g["h2"], g["channel_ps2"], int(n / 10), "minimum_sum", ALPHA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codes", default="hgp_34_n225,hgp_34_n625")
    ap.add_argument("--cycles", default="3,21")
    ap.add_argument("--p", type=float, default=2e-3)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop", default="single_shot", choices=["single_shot", "space_time"])
    ap.add_argument("--dem-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    for name in a.codes.split(","):
        for cycles in (int(c) for c in a.cycles.split(",")):
            code, sim, t_dem = build(name, cycles, a.p, a.loop)
            rec = {"loop": a.loop, "code": name, "n": code.N, "m": int(sim.eval_code.hx.shape[0]), "num_cycles": cycles,
                   "p": a.p, "dem_mechanisms": sim.dem.num_errors, "dem_detectors": sim.dem.num_detectors,
                   "circuit_and_dem_build_s": round(t_dem, 3)}
            if not a.dem_only:
                decoders(code, sim, a.p, a.loop)
                assert sim._engine_parts() is not None
                sim.WordErrorRate(a.samples)  # warm-up: the timed shapes, code objects, route tables
                times = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    wer, _ = sim.WordErrorRate(a.samples)  # ends in a device synchronise
                    times.append(time.perf_counter() - t0)
                r = sim.last_result
                med = statistics.median(times)
                rec.update({"samples": a.samples, "repeats": a.repeats, "seconds_median": med, "seconds_min": min(times),
                            "seconds_max": max(times), "samples_per_s": a.samples / med, "wer_last": wer,
                            "failures_last": r.failures, "decoder1_mean_iters": r.sector_iters[0] / r.sector_decodes[0],
                            "decoder1_nonconv_frac": r.sector_nonconv[0] / r.sector_decodes[0],
                            "decoder2_nonconv_frac": r.sector_nonconv[1] / r.sector_decodes[1],
                            "decoder1_engine": sim.decoder1_z.decoder.geometry().get("engine"),
                            "decoder2": type(sim.decoder2_z).__name__})
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()

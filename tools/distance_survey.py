"""Distance survey of the bundled codes: random information-set search, both sectors, on the GPU.

    python tools/distance_survey.py --trials 65536 [--trial-begin B] [--codes a,b] [--out FILE]
    python tools/distance_survey.py --throughput [--trials 16384] [--out FILE]

One JSON line per code and sector: weight (upper bound on the distance), hits, trials, seconds (of
the search calls, without the host-side generator-matrix set-up, but with each call's output-buffer
allocation and, on a process's first call, the code-object load: for the small codes the survey's
trials_per_s is a lower bound on the kernel's rate, not its throughput; use --throughput for that),
trials_per_s and, for HGP codes, the exact D of the distance theorem.  ``--trial-begin`` shards a
search: ranges of one seed combine by the minimum of (weight, trial).  ``--throughput`` times the
kernel (one warm-up, three timed repeats) beside the single-core host path on the same inputs.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from qldpc_fault_tolerance_amd import codes  # noqa: E402

THROUGHPUT_CODES = ["hgp_34_n1600", "LP_Matg8_L30_Dmin20", "GenBicycleA4"]
CHUNK = 1 << 16  # trials per call (bounds the per-trial output buffer)


def search(H, L, trials, seed, begin, backend):
    """Chunked distance_search; returns (weight, trial, hits, seconds)."""
    best, hits, dt = None, {}, 0.0
    for b in range(0, trials, CHUNK):
        r = codes.distance_search(H, L, trials=min(CHUNK, trials - b), seed=seed, trial_begin=begin + b, backend=backend)
        dt += r.seconds
        if r.weight is None:
            continue
        hits[r.weight] = hits.get(r.weight, 0) + r.hits
        if best is None or (r.weight, r.trial) < best:
            best = (r.weight, r.trial)
    return (best[0], best[1], hits[best[0]], dt) if best else (None, None, 0, dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=65536)
    ap.add_argument("--trial-begin", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--codes", default="")
    ap.add_argument("--backend", default="gpu")
    ap.add_argument("--throughput", action="store_true")
    ap.add_argument("--host-trials", type=int, default=32)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout

    def emit(rec):
        out.write(json.dumps(rec) + "\n")
        out.flush()

    names = [n for n in a.codes.split(",") if n] or (THROUGHPUT_CODES if a.throughput else codes.bundled_codes())
    for name in names:
        c = codes.get_code(name)
        D = codes.hgp(c.h1, c.h2, compute_distance=True).D if c.h1 is not None and not a.throughput else None
        for kind in ("X", "Z"):
            H, L = (c.hx, c.lx) if kind == "Z" else (c.hz, c.lz)
            rec = {"code": name, "N": c.N, "K": c.K, "sector": kind, "seed": a.seed, "trial_begin": a.trial_begin}
            if a.throughput:
                search(H, L, min(a.trials, 4096), a.seed, a.trial_begin, a.backend)  # warm-up
                reps = [search(H, L, a.trials, a.seed, a.trial_begin, a.backend) for _ in range(3)]
                secs = sorted(r[3] for r in reps)
                hw, _, _, hdt = search(H, L, a.host_trials, a.seed, a.trial_begin, "host")
                rec.update(weight=reps[0][0], hits=reps[0][2], trials=a.trials, seconds=secs, trials_per_s=a.trials / secs[1],
                           host_trials=a.host_trials, host_seconds=hdt, host_trials_per_s=a.host_trials / hdt)
            else:
                w, t, h, dt = search(H, L, a.trials, a.seed, a.trial_begin, a.backend)
                rec.update(weight=w, trial=t, hits=h, trials=a.trials, seconds=dt, trials_per_s=a.trials / dt)
                if D is not None:
                    rec["D"] = D
            emit(rec)


if __name__ == "__main__":
    main()

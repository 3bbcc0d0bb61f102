"""NumPy restatement of the random information-set distance search (the contract of
``qldpc_dist_*``), on dense 0/1 matrices with no word packing, for the CPU tests.

Trial ``t``: ``key[c]`` = first word of Philox4x32-10 at counter ``(c, t_lo, t_hi, 0x51D50005)``
and key ``(seed_lo, seed_hi)`` (drawn from the oracle's generator); columns are visited in
ascending ``(key[c], c)``; a column is a pivot when a row without a pivot has its bit set, that
row takes it and every other row with the bit has it xored in (pairing bits ride along);
candidates are the rows that hold a pivot and (with a pairing) pair non-trivially; the trial
reports min ``(weight, pivot position)``, a range min ``(weight, trial)``.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

STREAM_DISTANCE = 0x51D50005
NO_CANDIDATE = 0x7FFFFFFF


def column_order(oracle, n, seed, t):
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    keys = [oracle.philox4x32_10((c, t & 0xFFFFFFFF, (t >> 32) & 0xFFFFFFFF, STREAM_DISTANCE), key)[0]
            for c in range(n)]
    return sorted(range(n), key=lambda c: (keys[c], c))


@dataclass
class Trial:
    """What one trial did.  ``pivot_rows`` and ``filtered_rows`` name rows of the input matrix and so
    depend on the free choice of the row that takes a pivot; the other fields do not."""
    weight: int                  # NO_CANDIDATE if the trial has no candidate
    pos: int                     # pivot position of the winner (-1 if none)
    row: np.ndarray | None       # the winner's reduced row, n bits
    npiv: int                    # pivots taken (the rank, unless the trial stopped at ``rows``)
    last_pivot: int              # position of the last pivot (-1 if none)
    skipped_before_last: int     # visited columns before ``last_pivot`` that no row could take
    pivot_rows: list             # the row that took each pivot, in pivot order
    filtered_rows: list          # pivot rows the pairing filter removed (zero pairing)


def trial_facts(oracle, G, P, seed, t) -> Trial:
    rows, n = G.shape
    M = np.hstack([G, P]).astype(np.uint8) if P is not None else G.astype(np.uint8).copy()
    piv = np.full(rows, -1, dtype=np.int64)
    npiv, skipped, skipped_before_last, last, pivot_rows = 0, 0, 0, -1, []
    for j, c in enumerate(column_order(oracle, n, seed, t)):
        if npiv == rows:
            break
        elig = np.flatnonzero((M[:, c] == 1) & (piv < 0))
        if elig.size == 0:
            skipped += 1
            continue
        r = int(elig[-1])  # any eligible row: the contract leaves the choice free
        piv[r] = j
        npiv += 1
        last, skipped_before_last = j, skipped
        pivot_rows.append(r)
        others = np.flatnonzero(M[:, c])
        others = others[others != r]
        M[others] ^= M[r]
    best = (NO_CANDIDATE, -1, None)
    filtered = []
    for r in range(rows):
        if piv[r] < 0:
            continue
        if P is not None and not M[r, n:].any():
            filtered.append(r)
            continue
        cand = (int(M[r, :n].sum()), int(piv[r]))
        if cand < best[:2]:
            best = (cand[0], cand[1], M[r, :n].copy())
    return Trial(best[0], best[1], best[2], npiv, last, skipped_before_last, pivot_rows, filtered)


def trial(oracle, G, P, seed, t):
    """``(weight, pivot position, reduced row)`` of trial ``t``; weight NO_CANDIDATE if none."""
    f = trial_facts(oracle, G, P, seed, t)
    return f.weight, f.pos, f.row


def search(oracle, G, P, seed, trial_begin, trials, facts=None):
    """``(weight, trial, witness, trial_min)`` over ``[trial_begin, trial_begin + trials)``; a list
    passed as ``facts`` receives each trial's ``Trial``."""
    n = G.shape[1]
    tmin = np.full(trials, NO_CANDIDATE, dtype=np.int32)
    bw, bt, wit = NO_CANDIDATE, 0, np.zeros(n, np.uint8)
    for i in range(trials):
        f = trial_facts(oracle, G, P, seed, trial_begin + i)
        if facts is not None:
            facts.append(f)
        tmin[i] = f.weight
        if f.weight < bw:
            bw, bt, wit = f.weight, trial_begin + i, f.row
    return bw, bt, wit, tmin

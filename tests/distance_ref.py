"""NumPy restatement of the random information-set distance search (the contract of
``qldpc_dist_*``), on dense 0/1 matrices with no word packing, for the CPU tests.

Trial ``t``: ``key[c]`` = first word of Philox4x32-10 at counter ``(c, t_lo, t_hi, 0x51D50005)``
and key ``(seed_lo, seed_hi)`` (drawn from the oracle's generator); columns are visited in
ascending ``(key[c], c)``; a column is a pivot when a row without a pivot has its bit set, that
row takes it and every other row with the bit has it xored in (pairing bits ride along);
candidates are the rows that hold a pivot and (with a pairing) pair non-trivially; the trial
reports min ``(weight, pivot position)``, a range min ``(weight, trial)``.
"""
import numpy as np

STREAM_DISTANCE = 0x51D50005
NO_CANDIDATE = 0x7FFFFFFF


def column_order(oracle, n, seed, t):
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    keys = [oracle.philox4x32_10((c, t & 0xFFFFFFFF, (t >> 32) & 0xFFFFFFFF, STREAM_DISTANCE), key)[0]
            for c in range(n)]
    return sorted(range(n), key=lambda c: (keys[c], c))


def trial(oracle, G, P, seed, t):
    """``(weight, pivot position, reduced row)`` of trial ``t``; weight NO_CANDIDATE if none."""
    rows, n = G.shape
    M = np.hstack([G, P]).astype(np.uint8) if P is not None else G.astype(np.uint8).copy()
    piv = np.full(rows, -1, dtype=np.int64)
    npiv = 0
    for j, c in enumerate(column_order(oracle, n, seed, t)):
        if npiv == rows:
            break
        elig = np.flatnonzero((M[:, c] == 1) & (piv < 0))
        if elig.size == 0:
            continue
        r = int(elig[-1])  # any eligible row: the contract leaves the choice free
        piv[r] = j
        npiv += 1
        others = np.flatnonzero(M[:, c])
        others = others[others != r]
        M[others] ^= M[r]
    best = (NO_CANDIDATE, -1, None)
    for r in range(rows):
        if piv[r] < 0:
            continue
        if P is not None and not M[r, n:].any():
            continue
        cand = (int(M[r, :n].sum()), int(piv[r]))
        if cand < best[:2]:
            best = (cand[0], cand[1], M[r, :n].copy())
    return best


def search(oracle, G, P, seed, trial_begin, trials):
    """``(weight, trial, witness, trial_min)`` over ``[trial_begin, trial_begin + trials)``."""
    n = G.shape[1]
    tmin = np.full(trials, NO_CANDIDATE, dtype=np.int32)
    bw, bt, wit = NO_CANDIDATE, 0, np.zeros(n, np.uint8)
    for i in range(trials):
        w, _, row = trial(oracle, G, P, seed, trial_begin + i)
        tmin[i] = w
        if w < bw:
            bw, bt, wit = w, trial_begin + i, row
    return bw, bt, wit, tmin

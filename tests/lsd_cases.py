"""Shared inputs of the BP+LSD case tests (tests/test_lsd_cases_cpu.py, tests/test_gpu_lsd_cases.py).

Plain numpy, deterministic, no GPU.  One table of graphs: the OSD and BP shape tables' edge graphs
(tests/osd_cases.py, tests/bp_cases.py), hgp_34_n225's hz under the oracle's BP posteriors, and two graphs cut from the cluster kernel's own LDS accounting
(``expected``, the restatement of ``lsd_layout`` / ``lsd_gpu_from_host`` in csrc/lsd.hip): ``fit_exact``
has as many rows as the LDS image holds at its width, ``fit_over`` one more, so that a syndrome whose
cluster swallows the graph outgrows the LDS image there and is decoded on the HBM slice.

Per case a frozen batch: consistent syndromes at ``P_ERR``, the all-zero syndrome, and on the
rank-deficient graphs inconsistent ones (a set bit on an all-zero row of H; two copies of a row that
disagree), under crafted posteriors (mass ties, both zeros, both infinities, a constant row, an ascending
and a descending ramp).  No NaN: the law leaves it unspecified.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import bp_cases
import osd_cases

P_ERR = osd_cases.P_ERR
KS = (1, 2, 3, 64)
THREADS = 256
LDS_MAX = 160 * 1024
FIT_N = 600


def _al16(x):
    return (x + 15) & ~15


def _img_bytes(cap):
    return _al16(cap * 6) + cap * (cap // 64) * 16


def expected(m: int, n: int) -> dict:
    """The geometry ``DeviceLSD(graph).geometry()`` must report for an m x n graph (no QLDPC_LSD_WS)."""
    NP = 1
    while NP < n:
        NP <<= 1
    RWh = max(1, (m + 63) // 64)
    o = _al16(2 * n)
    sort_end = o + 12 * NP
    for b in (4 * m, 4 * m, 2 * m, 2 * m, 2 * n):
        o = _al16(o + b)
    nb, mb = (n + 31) // 32 * 4, (m + 31) // 32 * 4
    for b in (nb, nb, nb, mb, mb, THREADS * 4, RWh * 16, RWh * 16, 64):
        o = _al16(o + b)

    def total(cap):
        return max(sort_end, o + (_img_bytes(cap) if cap else 0))

    def fit(budget):
        for cap in range((m + 63) // 64 * 64, 63, -64):
            if total(cap) <= budget:
                return cap
        return 0

    cap = fit(64 * 1024) if m > 0 else 0
    if m > 0 and cap < 128 and cap < (m + 63) // 64 * 64:
        cap = min(fit(LDS_MAX), 128)
    # every workgroup owns an HBM slice of capacity m (the overflow route); the slices bound the grid to 256 MiB
    grid_bound = max(1, (256 << 20) // _img_bytes(max(64, (m + 63) // 64 * 64)))
    return {"row_words": 0, "window_words": 0, "threads": THREADS, "lds_rows": cap, "lds_bytes": total(cap),
            "grid_bound": grid_bound}


@lru_cache(maxsize=None)
def fit_rows() -> int:
    """The largest m at which an m x FIT_N graph's LDS image holds every row."""
    m = max(m for m in range(64, 2049, 64) if expected(m, FIT_N)["lds_rows"] >= m)
    assert expected(m + 1, FIT_N)["lds_rows"] == m, "one more row must not fit"
    return m


@dataclass(frozen=True)
class Case:
    id: str
    src: str            # "osd", "bp" (the table the graph comes from) or "fit"
    seed: int
    big: bool = False   # the Python law decodes the inconsistent syndromes at k = 64 alone (its round count);
                        # host stage against kernel runs them at every k


_CASES = (
    [Case(i, "osd", 300 + t, big=i in ("lds_maxn", "lds_m2049"))
     for t, i in enumerate(("rr2_tail", "rr2_exact", "k0", "small_k", "rank0", "tall", "lds_maxn", "lds_m2049"))] +
    [Case(i, "bp", 320 + t) for t, i in enumerate(("col1to8", "row33", "row64", "holes", "one_row", "one_col"))] +
    [Case("fit_exact", "fit", 341, big=True), Case("fit_over", "fit", 342, big=True),
     Case("n225_bp", "lib", 343)]  # hgp_34_n225 hz under the oracle's own BP posteriors
)
CASES = {c.id: c for c in _CASES}
CASE_IDS = [c.id for c in _CASES]


def _ro(a):
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def graph(case_id: str) -> np.ndarray:
    c = CASES[case_id]
    if c.src == "osd":
        return osd_cases.graph(case_id)
    if c.src == "bp":
        return bp_cases.graph(case_id)
    if c.src == "lib":
        from qldpc_fault_tolerance_amd import codes

        return _ro(np.ascontiguousarray(codes.get_code("hgp_34_n225").hz.astype(np.uint8)))
    m = fit_rows() + (1 if case_id == "fit_over" else 0)
    H = bp_cases.balanced(m, FIT_N, np.full(FIT_N, 3), c.seed).copy()  # no empty row: every row can turn active
    H[m - 1] = H[0]  # two copies of a row: a syndrome on which they disagree is inconsistent
    return _ro(H)


def crafted_posteriors(n: int, B: int, seed) -> np.ndarray:
    """The posterior kinds of tests/osd_cases.py on n columns: mass ties, +-0, +-inf; row 1 constant,
    row 2 ascending, row 3 descending."""
    rng = np.random.default_rng(seed)
    post = np.round(rng.normal(size=(B, n)) * 2.0) / 2.0
    post[:, ::11] = 0.0
    post[:, 5::17] = -0.0
    post[:, 3::29] = np.inf
    post[:, 7::31] = -np.inf
    ramp = (np.arange(n, dtype=np.float64) - n // 3) * 0.25
    if B > 1:
        post[1] = 1.5
    if B > 2:
        post[2] = ramp
    if B > 3:
        post[3] = -ramp
    return post


def _inconsistent_rows(case_id: str):
    """(all-zero row or None, (row, its copy) or None) of a case's graph."""
    H = graph(case_id)
    zero = np.flatnonzero(H.sum(axis=1) == 0)
    seen, dup = {}, None
    for i in range(H.shape[0]):
        key = H[i].tobytes()
        if H[i].any() and key in seen:
            dup = (seen[key], i)
            break
        seen.setdefault(key, i)
    return (int(zero[0]) if zero.size else None), dup


@lru_cache(maxsize=None)
def inputs(case_id: str):
    """(syndromes [B, m] uint8, posteriors [B, n] float64, inconsistent [B] bool), read-only: 6 consistent
    syndromes, the all-zero one, then the inconsistent ones the graph allows."""
    c = CASES[case_id]
    H = graph(case_id)
    m, n = H.shape
    rng = np.random.default_rng([c.seed, 1])
    if c.src == "lib":  # BP's own posteriors (oracle min-sum, 22 iterations) at p = 0.06: 6 non-converged decodes
        import oracle

        oracle.build()
        e = (rng.random((64, n)) < 0.06).astype(np.int64)
        S = np.concatenate([(e @ H.T.astype(np.int64) % 2).astype(np.uint8), np.zeros((1, m), np.uint8)])
        _, _, conv, post = oracle.bp_decode_batch_soft(H, 0.06, 22, 0.625, S)
        keep = np.concatenate([np.flatnonzero(~np.asarray(conv, bool))[:6], [64]])
        assert keep.size == 7
        return _ro(S[keep].copy()), _ro(np.ascontiguousarray(post[keep], dtype=np.float64)), _ro(np.zeros(7, bool))
    e = (rng.random((6, n)) < P_ERR).astype(np.int64)
    e[0, rng.integers(0, n)] = 1  # never an all-zero error in row 0
    S = [(e @ H.T.astype(np.int64) % 2).astype(np.uint8), np.zeros((1, m), np.uint8)]
    zero, dup = _inconsistent_rows(case_id)
    bad = []
    if zero is not None:
        s = S[0][1].copy()
        s[zero] = 1
        bad.append(s)
    if dup is not None:
        s = S[0][2].copy()
        s[dup[1]] = 1 - s[dup[0]]
        bad.append(s)
        s = np.zeros(m, np.uint8)  # nothing but the disagreement
        s[dup[1]] = 1
        bad.append(s)
    if bad:
        S.append(np.array(bad, np.uint8))
    S = np.concatenate(S)
    inc = np.zeros(S.shape[0], bool)
    inc[7:] = True
    return _ro(S), _ro(crafted_posteriors(n, S.shape[0], [c.seed, 3])), _ro(inc)


def ks_of(case_id: str, inconsistent: bool):
    """The bits_per_step values a syndrome of a case is decoded at."""
    return (64,) if (CASES[case_id].big and inconsistent) else KS

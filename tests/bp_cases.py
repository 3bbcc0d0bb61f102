"""Shared inputs of the irregular-graph BP tests (tests/test_bp_cases_cpu.py, tests/test_gpu_bp_cases.py).

Plain numpy, deterministic, no GPU.  One table of Tanner graphs that no bundled code resembles:
column degrees 1..12, row degrees 1..64, empty rows and columns, degree-1 columns, and the sizes on
either side of the switches between the general-purpose kernels.  Each case records the route
``plan_bp`` gives it per precision, (engine, kernel_id, row_chunks), frozen here:

* column degree 9..12 selects engine 6 (HBM-resident messages) on its own;
* column degree 7..8 selects engine 2's 8-slot kernels;
* wide rows stay on engine 3 (the register engine) with 7 to 32 row chunks;
* m = 64 / 65 are the two sides of the thread-per-syndrome one-iteration kernel (firstmin.hip),
  n + m = 2048 / 2049 those of engine 6's LDS-ballot switch.

Graph rule (``balanced``): every column takes its ``d_j`` distinct rows by ascending current row
degree, ties broken by a seeded generator, which balances the rows.

Every case has a list of prior levels p.  Priors at a level: ``uniform`` (p), ``nonuniform``
(linspace(0.5 p, 2 p), every fourth prior tied to the second) and ``half`` (the non-uniform ones with
three priors of exactly 0.5: zero LLRs).

Syndromes at a level: H e of N_PER_LEVEL i.i.d. errors at rate p, the all-zero syndrome and, where
the graph has an empty row, one syndrome with that row's bit set (unsatisfiable), shuffled once.
``mixed`` stacks the levels and shuffles again: early-converging, late-converging and
non-converging decodes in every slice.  The tiny graphs take all 2^m syndromes instead.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

P0 = 0.05            # the uniform prior of the recorded routes
MAX_ITER = 20
ALPHA = 0.625
N_PER_LEVEL = 100
LEVELS = (0.01, 0.03, 0.08, 0.15)
PRIORS = ("uniform", "nonuniform", "half")
HBM_MAX_DEG = 12     # engine 6 takes row and column degrees up to this
SOFT_MAX_COL = 8     # engine 1 (soft output) takes column degrees up to this


@dataclass(frozen=True)
class Case:
    id: str
    m: int
    n: int
    col: tuple              # (lo, hi): column j has degree lo + j % (hi - lo + 1)
    seed: int
    route64: tuple          # plan_bp at fp64, uniform priors: (engine, kernel_id, row_chunks)
    route32: tuple
    kind: str = "balanced"  # "holes": a row and two columns emptied; "ai": [A | I]; "all": every syndrome
    levels: tuple = LEVELS
    route64_nonuniform: tuple | None = None  # where non-uniform priors take another fp64 kernel
    # decode classes the syndrome set must hold under the oracle (tests/test_bp_cases_cpu.py):
    # "fail" >= 5 decodes that do not converge, "late" >= 5 that converge after the first
    # iteration, "first" >= 1 that converges in it
    classes: tuple = ("fail", "late", "first")

    def route(self, precision: int, kind: str = "uniform") -> tuple:
        if int(precision) == 32:
            return self.route32
        return self.route64 if kind == "uniform" or self.route64_nonuniform is None else self.route64_nonuniform


LOW_LEVELS = (0.002, 0.005) + LEVELS  # wide rows: product-sum converges late at the lowest levels only

_CASES = [
    # ---- column degree 7..8: engine 2's 8-slot kernels
    Case("col7", 48, 96, (7, 7), 201, (2, 2, 7), (2, 2, 4)),
    Case("col8", 64, 64, (8, 8), 202, (2, 2, 4), (2, 2, 2)),
    Case("col1to8", 80, 120, (1, 8), 203, (2, 2, 4), (2, 2, 2)),
    Case("col5", 48, 96, (5, 5), 204, (2, 2, 5), (3, 3, 3)),
    # ---- column degree 9..12: engine 6 without being asked
    Case("col9", 96, 96, (9, 9), 205, (6, 6, 0), (6, 6, 0)),
    Case("col12", 120, 120, (12, 12), 206, (6, 6, 0), (6, 6, 0)),
    Case("col1to12", 128, 128, (1, 12), 207, (6, 6, 0), (6, 6, 0)),
    # ---- wide rows on engine 3 (column degree 3): row_chunks 7, 8, 16, 17, 32 in fp64
    Case("row13", 12, 52, (3, 3), 208, (3, 3, 7), (3, 3, 4)),
    Case("row16", 12, 64, (3, 3), 209, (3, 3, 8), (3, 3, 4)),
    Case("row32", 12, 128, (3, 3), 210, (3, 3, 16), (3, 3, 8), levels=LOW_LEVELS),
    Case("row33", 12, 132, (3, 3), 211, (3, 3, 17), (3, 3, 9), levels=LOW_LEVELS),
    Case("row64", 12, 256, (3, 3), 212, (3, 3, 32), (3, 3, 16), levels=LOW_LEVELS),
    # ---- two variables per thread on engine 2
    Case("col7_vpl2", 130, 257, (7, 7), 213, (2, 2, 7), (2, 2, 4)),
    # ---- degree-0 and degree-1 nodes
    Case("holes", 48, 96, (3, 3), 214, (3, 3, 3), (3, 3, 2), kind="holes"),
    Case("a_i", 30, 90, (3, 3), 215, (3, 3, 4), (3, 3, 2), kind="ai"),
    # a single check / a single variable: 2 and 32 syndromes in all, every one of them decoded.  One
    # check of five variables converges at once or never; one variable under five degree-1 checks
    # gets the same five messages in every iteration (each holds its own syndrome bit alone), so its
    # decision never changes after the first: no late convergence exists on either graph
    Case("one_row", 1, 5, (1, 1), 216, (3, 3, 3), (3, 3, 2), kind="all", classes=("first",)),
    Case("one_col", 5, 1, (5, 5), 217, (2, 2, 1), (3, 3, 1), kind="all", classes=("fail", "first")),
    # ---- m = 64 | 65: the thread-per-syndrome one-iteration kernel and the wave kernel
    Case("m64", 64, 200, (3, 3), 218, (3, 3, 5), (3, 3, 3)),
    Case("m65", 65, 200, (3, 3), 219, (3, 3, 5), (3, 3, 3)),
    # ---- n + m = 2048 | 2049: engine 6's decisions in LDS ballot words, or in HBM (their own fp64
    # route is the one-word family under uniform priors, the two-word kernel otherwise)
    Case("xlds_2048", 682, 1366, (3, 3), 220, (3, 11103, 3), (3, 3, 2), route64_nonuniform=(3, 103, 4)),
    Case("xlds_2049", 682, 1367, (3, 3), 221, (3, 11103, 3), (3, 3, 2), route64_nonuniform=(3, 103, 4)),
]
CASES = {c.id: c for c in _CASES}
CASE_IDS = [c.id for c in _CASES]
# the Python restatements (tests/relay_ref.py, ps_ref below) are slow: the graphs they run on
SMALL_IDS = [c.id for c in _CASES if c.n <= 132]

# graphs the plan and creation refuse alike (QLDPC_ENOTSUP, "HBM engine: row or column degree above
# 12"): column degree 13; column degree 12 with rows of 13; column degree 9 whose rows come out at 18
OVER_DEGREE = {"col13": (48, 96, 13, 231), "col12_row13": (120, 130, 12, 232), "col9_row18": (48, 96, 9, 233)}


def _ro(a):
    a.setflags(write=False)
    return a


def balanced(m: int, n: int, degrees, seed: int) -> np.ndarray:
    """H [m, n] uint8: column j on ``degrees[j]`` distinct rows, the least loaded ones first."""
    rng = np.random.default_rng(seed)
    H = np.zeros((m, n), np.uint8)
    load = np.zeros(m, np.int64)
    for j in range(n):
        rows = np.lexsort((rng.random(m), load))[:int(degrees[j])]
        H[rows, j] = 1
        load[rows] += 1
    return H


def column_degrees(c: Case, n: int | None = None) -> np.ndarray:
    lo, hi = c.col
    return lo + np.arange(c.n if n is None else n) % (hi - lo + 1)


@lru_cache(maxsize=None)
def graph(case_id: str) -> np.ndarray:
    """The parity-check matrix of a case, uint8 [m, n], read-only."""
    c = CASES[case_id]
    if c.kind == "ai":
        na = c.n - c.m
        H = np.hstack([balanced(c.m, na, column_degrees(c, na), c.seed), np.eye(c.m, dtype=np.uint8)])
    else:
        H = balanced(c.m, c.n, column_degrees(c), c.seed)
    if c.kind == "holes":
        H[c.m // 2] = 0
        H[:, [c.n // 2, c.n - 1]] = 0
    assert H.shape == (c.m, c.n)
    return _ro(H)


@lru_cache(maxsize=None)
def over_degree_graph(name: str) -> np.ndarray:
    m, n, d, seed = OVER_DEGREE[name]
    return _ro(balanced(m, n, np.full(n, d), seed))


def empty_rows(case_id: str) -> np.ndarray:
    return np.flatnonzero(graph(case_id).sum(axis=1) == 0)


@lru_cache(maxsize=None)
def priors(case_id: str, kind: str, level: float = P0) -> np.ndarray:
    """Channel probabilities float64 [n] at prior level ``level``, read-only."""
    return priors_of(CASES[case_id].n, kind, level)


def priors_of(n: int, kind: str, level: float) -> np.ndarray:
    """The prior rule of the module docstring on ``n`` variables (tests/firstmin_cases.py shares it)."""
    if kind == "uniform":
        return _ro(np.full(n, level))
    p = np.linspace(0.5 * level, 2.0 * level, n)
    p[1::4] = p[min(1, n - 1)]
    if kind == "half":
        p[sorted({min(2, n - 1), n // 2, n - 1})] = 0.5
    elif kind != "nonuniform":
        raise ValueError(kind)
    return _ro(p)


@lru_cache(maxsize=None)
def syndromes(case_id: str, level: float) -> np.ndarray:
    """The syndromes of a case at one level, uint8 [B, m], read-only (see the module docstring)."""
    c = CASES[case_id]
    if c.kind == "all":
        return _ro(((np.arange(1 << c.m)[:, None] >> np.arange(c.m)) & 1).astype(np.uint8))
    return syndromes_of(graph(case_id), c.seed, c.levels.index(level), level)


def syndromes_of(H: np.ndarray, seed: int, level_index: int, level: float) -> np.ndarray:
    """The syndrome rule of the module docstring on a graph (tests/firstmin_cases.py shares it)."""
    m, n = H.shape
    rng = np.random.default_rng([seed, 1, level_index])
    # H e in float32: the counts are integers below 2^24, so the product is exact (and fast at n ~ 5000)
    assert n < 1 << 24
    e = (rng.random((N_PER_LEVEL, n)) < level).astype(np.float32)
    parts = [((e @ H.T.astype(np.float32)).astype(np.int64) % 2).astype(np.uint8), np.zeros((1, m), np.uint8)]
    hole = np.flatnonzero(H.sum(axis=1) == 0)
    if hole.size:
        s = parts[0][:1].copy()
        s[0, hole[0]] = 1
        parts.append(s)
    S = np.vstack(parts)
    return _ro(np.ascontiguousarray(S[rng.permutation(len(S))]))


@lru_cache(maxsize=None)
def mixed(case_id: str, B: int) -> np.ndarray:
    """``B`` syndromes drawn from all levels of a case (cycled when B exceeds them), shuffled."""
    c = CASES[case_id]
    return mixed_of([syndromes(case_id, lv) for lv in c.levels], c.seed, B)


def mixed_of(per_level: list, seed: int, B: int) -> np.ndarray:
    """The ``mixed`` rule on the syndromes of each level (tests/firstmin_cases.py shares it)."""
    S = np.vstack(per_level)
    rng = np.random.default_rng([seed, 2, B])
    S = S[rng.permutation(len(S))]
    return _ro(np.ascontiguousarray(S[np.arange(B) % len(S)]))


def classes_of(iters, conv) -> dict:
    """Decodes per class of a decoded syndrome set (see ``Case.classes``)."""
    iters, conv = np.asarray(iters), np.asarray(conv).astype(bool)
    return {"fail": int((~conv).sum()), "late": int((conv & (iters > 1)).sum()), "first": int((conv & (iters == 1)).sum())}


NEEDED = {"fail": 5, "late": 5, "first": 1}


def ps_ref(csr, channel_probs, max_iter, precision, synd):
    """The oracle's product-sum law (``bp_ps_*``, oracle/qldpc_oracle.c; ldpc's
    ``bp_decode_prob_ratios``) restated in sequential Python with scalars of the decoder's number
    type: ordered forward / backward products per row and per column, NaN -> 1 in the column
    products, decision ``ratio >= 1``.  [B, m] syndromes -> (corr [B, n] uint8, iters, conv)."""
    T = np.float64 if int(precision) == 64 else np.float32  # numpy scalars: x / 0 = inf as in C
    one, two = T(1.0), T(2.0)
    m, n = csr.m, csr.n
    rp = [int(v) for v in csr.row_ptr]
    ci = [int(v) for v in csr.col_idx]
    col_edges = [[] for _ in range(n)]
    for i in range(m):
        for e in range(rp[i], rp[i + 1]):
            col_edges[ci[e]].append(e)
    ratio = [T(float(p) / (1.0 - float(p))) for p in np.broadcast_to(np.asarray(channel_probs, np.float64), (n,))]

    def decode(s):
        b2c, c2b = [one] * rp[m], [one] * rp[m]
        for j in range(n):
            for e in col_edges[j]:
                b2c[e] = ratio[j]
        dec = [0] * n
        for it in range(1, max_iter + 1):
            for i in range(m):
                temp = T(-1.0) if s[i] else one
                for e in range(rp[i], rp[i + 1]):
                    c2b[e] = temp
                    temp = temp * (two / (one + b2c[e]) - one)
                temp = one
                for e in range(rp[i + 1] - 1, rp[i] - 1, -1):
                    c2b[e] = c2b[e] * temp
                    c2b[e] = (one - c2b[e]) / (one + c2b[e])
                    temp = temp * (two / (one + b2c[e]) - one)
            for j in range(n):
                temp = ratio[j]
                for e in col_edges[j]:
                    b2c[e] = temp
                    temp = temp * c2b[e]
                    if temp != temp:
                        temp = one
                dec[j] = 1 if temp >= one else 0
                temp = one
                for e in reversed(col_edges[j]):
                    b2c[e] = b2c[e] * temp
                    temp = temp * c2b[e]
                    if temp != temp:
                        temp = one
            if all((sum(dec[ci[e]] for e in range(rp[i], rp[i + 1])) & 1) == s[i] for i in range(m)):
                return dec, it, 1
        return dec, max_iter, 0

    with np.errstate(all="ignore"):
        out = [decode([int(v) & 1 for v in s]) for s in np.atleast_2d(np.asarray(synd))]
    return (np.array([o[0] for o in out], np.uint8).reshape(len(out), n), np.array([o[1] for o in out], np.int32),
            np.array([o[2] for o in out], bool))

"""Shared inputs of the higher-order BP+LSD tests (tests/test_lsd_order_cpu.py, tests/test_gpu_lsd_order.py):
a table cut from tests/lsd_cases.py (imported, not edited), two prior vectors per graph, the settings, and the
Python law (tests/lsd_order_ref.py) computed once per (case, priors, k, setting).

Plain numpy, deterministic, no GPU.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import lsd_cases
import lsd_order_ref

CASE_IDS = ("small_k", "rank0", "col1to8", "row33", "row64", "holes", "one_row", "one_col", "rr2_tail", "n225_bp")
KS = (1, 2)
SETTINGS = (("lsd_e", 1), ("lsd_e", 4), ("lsd_cs", 4), ("lsd_cs", 8))
PRIORS = ("uniform", "mixed")
EXTRA = "tie_pair"  # a crafted graph (below), beside the table
# more candidates per cluster than the kernel's 256 threads: on graphs of 12 and 48 rows whose clusters reach the
# order in free columns (row33 / row64: 12 rows under 132 / 256 columns), lsd_e 8 and 12 give 255 and 4,095
# candidates, lsd_cs 64 up to |F| + 2,016; uniform priors make most of them as heavy as another
BIG_CASE_IDS = ("row33", "row64", "holes")
BIG_SETTINGS = (("lsd_e", 8), ("lsd_e", 12), ("lsd_cs", 64))


@lru_cache(maxsize=None)
def graph(case_id: str) -> np.ndarray:
    if case_id != EXTRA:
        return lsd_cases.graph(case_id)
    # one seed row with four columns that meet again in pairs: growth to two free columns gives candidates as
    # heavy as the incumbent under uniform priors, and lighter ones with more columns under the mixed ones
    H = np.zeros((5, 8), np.uint8)
    H[0, :4] = 1
    H[1, [0, 1, 4]] = 1
    H[2, [2, 3, 5]] = 1
    H[3, [4, 5, 6]] = 1
    H[4, [6, 7]] = 1
    H.setflags(write=False)
    return H


@lru_cache(maxsize=None)
def inputs(case_id: str):
    """(syndromes [B, m], posteriors [B, n]) of a case, read-only: the frozen batch of tests/lsd_cases.py
    (consistent, all-zero and inconsistent syndromes under the crafted posteriors; BP's own on n225_bp)."""
    if case_id != EXTRA:
        S, P, _ = lsd_cases.inputs(case_id)
        return S, P
    H = graph(case_id)
    rng = np.random.default_rng(77)
    e = (rng.random((6, H.shape[1])) < 0.3).astype(np.int64)
    e[0, 0] = 1
    S = (e @ H.T.astype(np.int64) % 2).astype(np.uint8)
    P = lsd_cases.crafted_posteriors(H.shape[1], 6, [77, 3])
    for a in (S, P):
        a.setflags(write=False)
    return S, P


@lru_cache(maxsize=None)
def priors(case_id: str, kind: str) -> np.ndarray:
    """uniform: 0.05 everywhere.  mixed: drawn from (0.01, 0.3), every fourth column tied at 0.07."""
    n = graph(case_id).shape[1]
    if kind == "uniform":
        p = np.full(n, 0.05)
    else:
        p = np.random.default_rng([n, 5]).uniform(0.01, 0.3, n)
        p[::4] = 0.07
    p.setflags(write=False)
    return p


_LAW = {}


def law(case_id, kind, k, method, w, wq):
    """(x0, xw, stats, events) of a case under the Python law with the handle's integer weights."""
    key = (case_id, kind, k, method, w)
    if key not in _LAW:
        S, P = inputs(case_id)
        _LAW[key] = lsd_order_ref.decode_batch(graph(case_id), S, P, k, method, w, wq)
    return _LAW[key]

"""Shared inputs of the first-min tests (tests/test_firstmin_cases_cpu.py, tests/test_gpu_firstmin.py).

Plain numpy, deterministic, no GPU.  The loop kernels of csrc/firstmin.hip on graphs no bundled code
resembles.  Graphs, priors (``nonuniform``, ``half``) and syndromes are those of tests/bp_cases.py, by
its own rules; this table adds what first-min needs on top:

* the two graphs on either side of the natural kernel switch (one wave per syndrome while four
  syndromes' arrays fit 64 KiB of LDS, m + n <= 8192; one workgroup per syndrome past it), made by
  ``bp_cases.balanced`` with column degree 3;
* the CSR graphs at the edge of the creation envelope (2 (m + n) + 16 bytes of LDS <= 64 KiB), never
  dense;
* per case, the prior levels the decoder is built at, chosen on the CPU oracle so that the ``mixed``
  syndromes hold, over those levels, every decode class of ``firstmin_ref.classes_of`` the graph
  admits (tests/test_firstmin_cases_cpu.py), and a one-line reason for each class it cannot hold.

The decoder's priors sit at one level at a time while the syndromes mix all error rates of the
bp_cases levels.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import bp_cases as bc
from qldpc_fault_tolerance_amd.codes import CSR

MAX_ITERS = (0, 1, 12)
MAX_ITER = 12                 # the classes are counted at this one
ALPHAS = (0.625, 0.0)
ALPHA_DEG1 = 0.9              # added where a column meets several degree-1 rows (SENTINEL * alpha sums)
PRECISIONS = (64, 32)
PRIORS = ("nonuniform", "half")
B_MIXED = 301                 # ragged against the 4 waves of a workgroup
NEEDED = 5                    # decodes per class; 1 on the all-syndrome graphs
LDS_LIMIT = 64 * 1024
WG_STATIC_LDS = 16            # the workgroup kernel's own words (.group_segment_fixed_size)


def takes_wave(m: int, n: int) -> bool:
    """One wave per syndrome: four syndromes' arrays, each rounded up to 16 bytes, fit 64 KiB."""
    return 4 * ((2 * (m + n) + 15) // 16 * 16) <= LDS_LIMIT


def admitted(m: int, n: int) -> bool:
    """``qldpc_firstmin_create`` takes the graph: the workgroup kernel's arrays and its own words fit."""
    return 2 * (m + n) + WG_STATIC_LDS <= LDS_LIMIT


@dataclass(frozen=True)
class Case:
    id: str
    levels: tuple = (0.03, 0.3)  # prior levels the decoder is built at
    source: str | None = None  # the bp_cases case it takes graph, priors and syndromes from
    shape: tuple | None = None  # (m, n, seed) of a graph of its own (bp_cases.balanced, column degree 3)
    deg1_rows: bool = False    # alpha 0.9 joins the alphas
    # class -> why the graph cannot hold it at these levels (it must hold every other class of
    # firstmin_ref.CLASSES[:4], and none of these); absent64: in fp64 only
    absent: dict = field(default_factory=dict)
    absent64: dict = field(default_factory=dict)
    toggling: bool = False     # under ``half`` priors an empty column has p = 0.5: BP1(0) decides it

    @property
    def all_syndromes(self) -> bool:
        return self.source is not None and bc.CASES[self.source].kind == "all"

    @property
    def alphas(self) -> tuple:
        return ALPHAS + ((ALPHA_DEG1,) if self.deg1_rows else ())


_ONE_ROW = {  # positive priors at both levels: BP1(0) = 0 and the syndrome weight is at most 1
    "rejected": "one check: no decision takes the weight above 1",
    "stopped": "one check: once cleared nothing is decided, and a weight of 1 is never exceeded",
}
_ONE_COL = {
    "stopped": "a flip complements the syndrome and is accepted from weight >= 3 only; the complement never flips back",
}
_ONE_COL_64 = {  # (fp32 sums overflow after the first two messages, which alone then decide: weight 2 -> 3)
    "rejected": "fp64 at alpha 0.625 decides by the majority of the five messages: a flip never raises the weight",
}

# Two prior levels by default.  At 0.03 every prior is below 0.5: light syndromes clear, most others
# run to max_iter on a weight that no longer falls.  At 0.3 the non-uniform priors reach 0.6: negative
# LLRs (the tables' prior-sign parities), BP1(0) decides something, and decodes are rejected or stop.
_CASES = [
    Case("holes", source="holes", toggling=True),
    Case("a_i", source="a_i"),
    Case("col1to8", source="col1to8"),
    Case("col1to12", source="col1to12"),
    Case("row64", source="row64"),
    # at 0.03 the least reliable variable keeps its sign (exhausted), at 0.2 it alone flips (cleared)
    Case("one_row", (0.03, 0.2), source="one_row", absent=_ONE_ROW),
    Case("one_col", (0.03,), source="one_col", deg1_rows=True, absent=_ONE_COL, absent64=_ONE_COL_64),
    Case("col7_vpl2", source="col7_vpl2"),
    Case("xlds_2048", source="xlds_2048"),
]
CASES = {c.id: c for c in _CASES}
CASE_IDS = [c.id for c in _CASES]

# the natural kernel switch: m + n = 8192 takes the wave kernel with exactly 64 KiB of LDS, 8193 the
# workgroup kernel
SWITCH = {"lds_8192": Case("lds_8192", shape=(2731, 5461, 241)),
          "lds_8193": Case("lds_8193", shape=(2731, 5462, 242))}
B_SWITCH = 24

# the creation envelope: m + n = 32760 is the largest graph admitted, 32768 the largest the dynamic
# LDS alone would admit
ENVELOPE = {"env_32760": (10914, 21846), "env_32768": (10914, 21854)}  # m = 6 * 17 * 107: coprime to 7 and 13
ENVELOPE_P = 0.01
ENVELOPE_MAX_ITER = 3


def case(case_id: str) -> Case:
    return CASES[case_id] if case_id in CASES else SWITCH[case_id]


@lru_cache(maxsize=None)
def graph(case_id: str) -> np.ndarray:
    c = case(case_id)
    if c.source is not None:
        return bc.graph(c.source)
    m, n, seed = c.shape
    H = bc.balanced(m, n, np.full(n, 3), seed)
    H.setflags(write=False)
    return H


@lru_cache(maxsize=None)
def priors(case_id: str, kind: str, level: float) -> np.ndarray:
    assert level in case(case_id).levels
    return bc.priors_of(graph(case_id).shape[1], kind, level)


@lru_cache(maxsize=None)
def mixed(case_id: str, B: int = B_MIXED) -> np.ndarray:
    """``B`` syndromes of all bp_cases levels, shuffled (``bp_cases.mixed``), uint8 [B, m], read-only."""
    c = case(case_id)
    if c.source is not None:
        return bc.mixed(c.source, B)
    _, _, seed = c.shape
    return bc.mixed_of([bc.syndromes_of(graph(case_id), seed, i, lv) for i, lv in enumerate(bc.LEVELS)], seed, B)


@lru_cache(maxsize=None)
def reuse_batch(case_id: str, B: int) -> np.ndarray:
    """``B`` syndromes for the reuse tests: the mixed set cycled, then shuffled once, so that the
    syndromes one wave or workgroup takes in turn are of every class."""
    S = mixed(case_id, B_MIXED)
    c = case(case_id)
    rng = np.random.default_rng([bc.CASES[c.source].seed if c.source is not None else c.shape[2], 3, B])
    out = np.ascontiguousarray(S[np.arange(B) % len(S)][rng.permutation(B)])
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def envelope_graph(name: str) -> CSR:
    """Column j on rows j % m, (7 j + 1) % m and (13 j + 5) % m, as a CSR (no dense matrix)."""
    m, n = ENVELOPE[name]
    j = np.arange(n, dtype=np.int64)
    r = np.stack([j % m, (7 * j + 1) % m, (13 * j + 5) % m])
    assert (r[0] != r[1]).all() and (r[0] != r[2]).all() and (r[1] != r[2]).all()  # three distinct rows
    rows, cols = r.ravel(), np.tile(j, 3)
    order = np.lexsort((cols, rows))  # row-major, columns ascending within a row
    row_ptr = np.zeros(m + 1, np.int64)
    np.add.at(row_ptr, rows + 1, 1)
    return CSR(m, n, np.cumsum(row_ptr).astype(np.int32), cols[order].astype(np.int32))


@lru_cache(maxsize=None)
def envelope_syndromes(name: str, B: int = 3) -> np.ndarray:
    csr = envelope_graph(name)
    rng = np.random.default_rng([csr.m, csr.n, 11])
    S = csr.matvec((rng.random((B, csr.n)) < 0.004).astype(np.uint8))
    S.setflags(write=False)
    return S

"""Shared inputs of the distance-search case tests (tests/test_distance_cases_cpu.py,
tests/test_gpu_distance_cases.py).

Plain numpy, deterministic, no GPU.  One table of raw ``(G, P)`` pairs for ``qldpc_dist_create``
(not check matrices: zero, repeated and dependent generator rows are legal inputs), chosen to sit
on the edges of ``dist_kernel<WT>`` (csrc/distance.hip), with the geometry each device handle must
report written out, not computed from the library:

* ``threads``: rows rounded up to whole waves; ``row_words`` = ceil(n / 64); ``pair_words`` =
  ceil(k / 64); ``tpl``: the first compiled width in ``WIDTHS`` that holds code + pairing words;
  LDS = 16400 + 256 * tpl bytes (the 16 KiB sort, two parities of sixteen wave slots of ``tpl``
  words, 16 bytes of scalars).

Every pairing is ``P = G L^T`` for an ``L`` the case keeps, so that the pairing is a function of
the code vector (with dependent rows a free ``P`` would make the outputs depend on which row takes
a pivot, which the contract leaves open) and a witness can be checked by ``L w != 0``.  On a
full-rank ``[I | A]`` any ``P`` is such a product: ``lift`` puts row r's pairing on its identity
column.

Added to the cases the issue lists: ``w26_full`` (the table had no exactly-full case of width 26),
``lower_tri_wide`` (a square invertible G reduces to the identity in every trial, so
``lower_tri_dense`` can neither skip a column nor change its minimum; the wide one can), and
``pair_k1`` beside ``w4_pad``, and ``all_ones_1792`` (weight 1792, the largest the kernel's
(weight, position) key has to pack).  The exactly-full width cases that end in a pairing word pair
in the last bit of that word only, so that the candidate filter hangs on the row's last word.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

WIDTHS = (2, 4, 8, 12, 16, 20, 24, 26, 28)   # the compiled dist_kernel<WT>
NO_CANDIDATE = 0x7FFFFFFF
SEED = (0x5EED << 32) | 0xD157               # a high word, so Philox key word 1 is not zero
TRIAL_BEGIN = 5


@dataclass(frozen=True)
class Case:
    id: str
    rows: int
    n: int
    k: int
    threads: int            # qldpc_dist_geometry of a device handle
    row_words: int
    pair_words: int
    tpl: int                # the template width that runs it
    kind: str               # constructor (``_generator``)
    seed: int
    full: bool | None = True   # rank == rows (True), rank < rows (False); asserted on the CPU
    trials: int = 8
    pairing: str = "rand"   # how L is made when k > 0 (``_pairing``)
    rank: int = 0           # ``span``: the rank of the row space
    candidate: bool = True  # False: built to have no candidate in any trial

    @property
    def lds_bytes(self) -> int:
        return 16400 + 256 * self.tpl


def _w(cid, n, k, rw, pw, tpl, seed, **kw):
    """A width case: about 70 rows (two waves, the second partial)."""
    kw.setdefault("kind", "ia_dense")
    return Case(cid, 70, n, k, 128, rw, pw, tpl, seed=seed, **kw)


def _p(cid, k, pw, seed, **kw):
    """A pairing case on w4_pad's shape: 70 x 128, 2 code words, template 4."""
    kw.setdefault("kind", "ia_dense")
    return Case(cid, 70, 128, k, 128, 2, pw, 4, seed=seed, **kw)


_CASES = [
    # ---- width edges: every compiled width exactly full and, where a smaller count maps to it, padded
    _w("w2_full", 64, 64, 1, 1, 2, 201, kind="span", rank=48, full=False),   # rows > n
    _w("w2_pad", 40, 0, 1, 0, 2, 202, kind="span", rank=28, full=False),
    _w("w4_full", 192, 64, 3, 1, 4, 203, pairing="last_row"),
    _w("w4_pad", 128, 1, 2, 1, 4, 204),
    _w("w8_full", 448, 64, 7, 1, 8, 205, pairing="last_row"),
    _w("w8_pad", 257, 0, 5, 0, 8, 206),
    _w("w12_full", 640, 128, 10, 2, 12, 207, pairing="last_row"),
    _w("w12_pad", 513, 0, 9, 0, 12, 208),
    _w("w16_full", 1024, 0, 16, 0, 16, 209),            # np = n: no sort padding
    _w("w16_pad", 769, 65, 13, 2, 16, 210),
    _w("w20_full", 1216, 64, 19, 1, 20, 211, pairing="last_row"),
    _w("w20_pad", 1025, 1, 17, 1, 20, 212),             # n = 2^10 + 1: 1023 pad keys
    _w("w24_full", 1408, 128, 22, 2, 24, 213, pairing="last_row"),
    _w("w24_pad", 1281, 0, 21, 0, 24, 214),
    _w("w26_full", 1600, 64, 25, 1, 26, 215, pairing="last_row"),
    _w("w26_pad", 1600, 0, 25, 0, 26, 216),
    _w("w28_full", 1792, 0, 28, 0, 28, 217),
    _w("w28_pair", 1664, 65, 26, 2, 28, 218, pairing="last_row"),
    _w("w28_pad", 1700, 0, 27, 0, 28, 219),
    # ---- row-count edges: n = 96, k = 0 (rows > 96 is rank-deficient by construction)
    Case("rows_1", 1, 96, 0, 64, 2, 0, 2, "sparse", 231),
    Case("rows_63", 63, 96, 0, 64, 2, 0, 2, "ia_dense", 232),
    Case("rows_64", 64, 96, 0, 64, 2, 0, 2, "ia_dense", 233),
    Case("rows_65", 65, 96, 0, 128, 2, 0, 2, "ia_dense", 234),
    Case("rows_128", 128, 96, 0, 128, 2, 0, 2, "span", 235, rank=60, full=False),
    Case("rows_1023", 1023, 96, 0, 1024, 2, 0, 2, "span", 236, rank=60, full=False),
    Case("rows_1024", 1024, 96, 0, 1024, 2, 0, 2, "span", 237, rank=60, full=False),
    # the far corner of the envelope
    Case("corner_1024x28", 1024, 1792, 0, 1024, 28, 0, 28, "ia_mid", 238, trials=2),
    # ---- column-count edges
    Case("n1", 1, 1, 0, 64, 1, 0, 2, "n1", 241),                    # np = 2, one pad key
    Case("n2", 2, 2, 0, 64, 1, 0, 2, "n2", 242),
    Case("one_row_1792", 1, 1792, 0, 64, 28, 0, 28, "sparse", 243),  # 64 threads sort 2048 keys
    Case("all_ones_1792", 1, 1792, 0, 64, 28, 0, 28, "ones", 246),   # the largest weight the key packs
    Case("n64_lastword", 40, 64, 0, 64, 1, 0, 2, "ia_fill", 244),    # bit 63 of the last word in use
    Case("n128_lastword", 70, 128, 0, 128, 2, 0, 2, "ia_fill", 245),
    # ---- rank and structure edges
    Case("all_zero", 150, 200, 0, 192, 4, 0, 4, "all_zero", 251, full=False, candidate=False),
    Case("zero_rows", 150, 200, 0, 192, 4, 0, 4, "zero_rows", 252, full=False),
    Case("dup_rows", 150, 200, 0, 192, 4, 0, 4, "dup_rows", 253, full=False),
    Case("rank1", 130, 200, 0, 192, 4, 0, 4, "rank1", 254, full=False),
    Case("identity", 100, 100, 0, 128, 2, 0, 2, "identity", 255),
    Case("lower_tri_dense", 128, 128, 0, 128, 2, 0, 2, "lower_tri", 256),
    Case("lower_tri_wide", 128, 160, 0, 128, 3, 0, 4, "lower_tri", 257),
    Case("last_wave_only", 1000, 96, 0, 1024, 2, 0, 2, "last_wave", 258, full=False),
    Case("dense_row", 150, 200, 0, 192, 4, 0, 4, "dense_row", 259, full=None),   # rank not declared
    # ---- pairing edges
    _p("pair_k1", 1, 1, 261),
    _p("pair_k63", 63, 1, 262),
    _p("pair_k64", 64, 1, 263),
    _p("pair_k65", 65, 2, 264),
    _p("pair_k128", 128, 2, 265),
    _p("pair_last_bit", 128, 2, 266, pairing="last_bit"),
    _p("pair_zero", 64, 1, 267, pairing="zero", candidate=False),
    _p("pair_heavy_only", 64, 1, 268, kind="ia_heavy", pairing="heavy"),
    _p("pair_dense", 128, 2, 272, kind="ia_light", pairing="ones"),
    # ---- ties: every trial of the identity reaches weight 1, each with another witness
    Case("ties", 100, 100, 0, 128, 2, 0, 2, "identity", 271, trials=24),
]
CASES = {c.id: c for c in _CASES}
CASE_IDS = [c.id for c in _CASES]
assert len(CASES) == len(_CASES)

HEAVY_ROWS = (5, 20, 37, 50, 64, 69)   # ia_heavy / dense_row: rows of weight about n / 2
LAST_WAVE_FIRST_ROW = 960
# one minimum and no skipped column are all these can show: rows = 1 (the reduced row is the row),
# a square invertible G (it reduces to the identity) or a rank-1 row space
TRIVIAL = ("identity", "ties", "rank1", "all_zero", "n1", "n2", "rows_1", "one_row_1792", "all_ones_1792",
           "lower_tri_dense")

# (rows, n, k): a device handle answers QLDPC_ENOTSUP, a host handle runs them
UNSUPPORTED = [(1025, 96, 0), (0, 96, 0), (1, 1793, 0), (1, 1728, 65)]


def _ro(a):
    if a is not None:
        a.setflags(write=False)
    return a


def sparse_rows(rows: int, n: int, rng, wlo: int = 3, whi: int = 8) -> np.ndarray:
    """Random rows of weight wlo..whi (at most n)."""
    G = np.zeros((rows, n), np.uint8)
    for r in range(rows):
        w = min(n, int(rng.integers(wlo, whi + 1)))
        G[r, rng.choice(n, size=w, replace=False)] = 1
    return G


def identity_plus(rows: int, n: int, rng, wlo: int = 3, whi: int = 8):
    """``[I | A]`` under a fixed column permutation: full rank, row weight wlo..whi (one entry on the
    row's identity column, the rest among the n - rows others).  Returns (G, identity columns)."""
    assert rows <= n
    perm = rng.permutation(n)
    idc, rest = perm[:rows], perm[rows:]
    G = np.zeros((rows, n), np.uint8)
    G[np.arange(rows), idc] = 1
    for r in range(rows):
        w = min(rest.size, int(rng.integers(wlo, whi + 1)) - 1)
        if w > 0:
            G[r, rng.choice(rest, size=w, replace=False)] = 1
    return G, idc


def span_rows(rows: int, n: int, rank: int, rng) -> np.ndarray:
    """``rows`` > rank rows of a rank-``rank`` space: an ``[I | A]`` basis and sums of two of
    its rows, in a random row order."""
    B, _ = identity_plus(rank, n, rng, *_dense_weights(n))
    G = np.zeros((rows, n), np.uint8)
    G[:rank] = B
    for r in range(rank, rows):
        i, j = rng.choice(rank, size=2, replace=False)
        G[r] = B[i] ^ B[j]
    return G[rng.permutation(rows)]


def lift(P: np.ndarray, idc: np.ndarray, n: int) -> np.ndarray:
    """L [k, n] with ``G L^T = P`` for ``G = [I | A]`` whose identity columns are ``idc``."""
    L = np.zeros((P.shape[1], n), np.uint8)
    L[:, idc] = P.T
    return L


def _dense_weights(n):
    return max(3, n // 12), max(8, n // 8)


def _generator(c: Case, rng):
    """(G, identity columns or None)."""
    rows, n = c.rows, c.n
    if c.kind == "ia":
        return identity_plus(rows, n, rng)
    if c.kind == "ia_dense":      # rows meet in most columns: an xor at nearly every step
        return identity_plus(rows, n, rng, *_dense_weights(n))
    if c.kind == "ia_mid":        # the corner: about twenty rows meet in a column, 96 columns are empty
        G, idc = identity_plus(rows, n, rng, 12, 20)
        G[:, np.setdiff1d(np.arange(n), idc)[::8]] = 0
        return G, idc
    if c.kind == "ia_light":      # lighter rows: a reduced row that sums few of them is usually the minimum
        return identity_plus(rows, n, rng, 5, 6)
    if c.kind == "ia_fill":       # every column in use, bit 63 of the last word among them
        G, idc = identity_plus(rows, n, rng, *_dense_weights(n))
        for col in np.flatnonzero(~G.any(axis=0)):
            G[col % rows, col] = 1
        return G, idc
    if c.kind == "ia_heavy":      # six rows dense on the non-identity columns: still [I | A]
        G, idc = identity_plus(rows, n, rng)
        rest = np.setdiff1d(np.arange(n), idc)
        for r in HEAVY_ROWS:
            G[r, rest] = rng.random(rest.size) < 0.5
        return G, idc
    if c.kind == "dense_row":     # three rows of weight about n / 2 over all columns
        G, idc = identity_plus(rows, n, rng)
        for r in HEAVY_ROWS[:3]:
            G[r] = rng.random(n) < 0.5
            G[r, idc[r]] = 1
        return G, None
    if c.kind == "sparse":
        return sparse_rows(rows, n, rng, 8, 8), None
    if c.kind == "span":
        return span_rows(rows, n, c.rank, rng), None
    if c.kind == "ones":
        return np.ones((rows, n), np.uint8), None
    if c.kind == "n1":
        return np.ones((1, 1), np.uint8), None
    if c.kind == "n2":
        return np.array([[1, 1], [0, 1]], np.uint8), None
    if c.kind == "all_zero":
        return np.zeros((rows, n), np.uint8), None
    if c.kind == "zero_rows":
        G, _ = identity_plus(rows, n, rng)
        G[[0, 63, 64, rows - 1]] = 0
        return G, None
    if c.kind == "dup_rows":
        G, _ = identity_plus(rows, n, rng)
        G[rows - 5:] = G[:5]
        G[70] = G[10] ^ G[11]
        return G, None
    if c.kind == "rank1":
        return np.repeat(sparse_rows(1, n, rng), rows, axis=0), None
    if c.kind == "identity":
        return np.eye(rows, n, dtype=np.uint8), None
    if c.kind == "lower_tri":     # dense below a unit diagonal; columns past ``rows`` dense random
        G = (rng.random((rows, n)) < 0.5).astype(np.uint8)
        G[:, :rows] = np.tril(G[:, :rows])
        G[np.arange(rows), np.arange(rows)] = 1
        return G, None
    if c.kind == "last_wave":     # rows below 960 zero: every winner comes from wave 15
        G = np.zeros((rows, n), np.uint8)
        G[LAST_WAVE_FIRST_ROW:], _ = identity_plus(rows - LAST_WAVE_FIRST_ROW, n, rng, *_dense_weights(n))
        return G, None
    raise ValueError(c.kind)


def _pairing(c: Case, G, idc, rng):
    """L [k, n]."""
    rows, n, k = c.rows, c.n, c.k
    if c.pairing == "rand":       # density 1/2, so G L^T is too
        return (rng.random((k, n)) < 0.5).astype(np.uint8)
    if c.pairing == "last_row":   # only the last bit of the last pairing word, on about half of the rows:
        L = np.zeros((k, n), np.uint8)   # the filter hangs on the last word of a row that fills its template
        L[k - 1] = rng.random(n) < 0.5
        return L
    assert idc is not None
    P = np.zeros((rows, k), np.uint8)
    if c.pairing == "last_bit":   # only the last bit of the last pairing word, on a third of the rows
        P[::3, k - 1] = 1
    elif c.pairing == "heavy":    # only the rows built to be heavy pair at all
        P[list(HEAVY_ROWS)] = rng.random((len(HEAVY_ROWS), k)) < 0.5
        P[list(HEAVY_ROWS), 0] = 1
    elif c.pairing == "ones":     # weights must not count these 128 bits
        P[:] = 1
    elif c.pairing != "zero":
        raise ValueError(c.pairing)
    return lift(P, idc, n)


@lru_cache(maxsize=None)
def matrices(case_id: str):
    """``(G, P, L)`` of a case: uint8 [rows, n], [rows, k], [k, n]; P and L are None when k = 0.
    Read-only."""
    c = CASES[case_id]
    rng = np.random.default_rng(c.seed)
    G, idc = _generator(c, rng)
    G = np.ascontiguousarray(G, dtype=np.uint8)
    assert G.shape == (c.rows, c.n), (case_id, G.shape)
    if c.k == 0:
        return _ro(G), None, None
    L = _pairing(c, G, idc, rng)
    P = (G.astype(np.int64) @ L.T.astype(np.int64) % 2).astype(np.uint8)
    assert P.shape == (c.rows, c.k)
    return _ro(G), _ro(P), _ro(L)


def unsupported_matrices(rows: int, n: int, k: int):
    """A sparse (G, P) of a shape outside the device envelope."""
    rng = np.random.default_rng([rows, n, k])
    G = sparse_rows(rows, n, rng)
    P = (rng.random((rows, k)) < 0.5).astype(np.uint8) if k else None
    return G, P


# ------------------------------------------------------------------ the C API on raw (G, P)
class Handle:
    """A ``qldpc_dist`` handle on an explicit generator (rows may be dependent or zero):
    ``device = -1`` is a host handle, which ``run`` serves by ``qldpc_dist_run_host``."""

    def __init__(self, G, P=None, device: int = -1):
        from qldpc_fault_tolerance_amd import _native, codes

        self._native, self._codes = _native, codes
        self.lib = _native.lib()
        self.device, (self.rows, self.n) = device, G.shape
        self.k = 0 if P is None else P.shape[1]
        vp = ctypes.c_void_p
        Gw = codes._pack_rows(G)
        Pw = codes._pack_rows(P) if self.k else None
        self.words = Gw.shape[1]
        self.h = vp()
        rc = self.lib.qldpc_dist_create(device, self.rows, self.n, self.k, Gw.ctypes.data_as(vp),
                                        Pw.ctypes.data_as(vp) if self.k else None, ctypes.byref(self.h))
        _native.check(rc, "qldpc_dist_create")

    def geometry(self):
        """[threads, row_words, pair_words, lds_bytes]"""
        geo = [ctypes.c_int32(-1) for _ in range(4)]
        assert self.lib.qldpc_dist_geometry(self.h, *[ctypes.byref(g) for g in geo]) == 0
        return [g.value for g in geo]

    def run(self, trials, seed=0, trial_begin=0, workgroups=0, stream=None, want_trial_min=True):
        """(weight, trial, witness uint8 [n], trial_min int32 [trials] or None)"""
        vp = ctypes.c_void_p
        # a value the call must overwrite (a trial's minimum is never negative)
        tmin = np.full(trials, -7, np.int32) if want_trial_min else None
        tp = tmin.ctypes.data_as(vp) if want_trial_min else None
        bw, bt = ctypes.c_int32(-7), ctypes.c_uint64(0xDEAD)
        wit = np.full(self.words, 0xA5A5A5A5A5A5A5A5, "<u8")
        if self.device >= 0:
            rc = self.lib.qldpc_dist_run(self.h, seed, trial_begin, trials, workgroups, tp, ctypes.byref(bw),
                                         ctypes.byref(bt), wit.ctypes.data_as(vp), stream)
            self._native.check(rc, "qldpc_dist_run")
        else:
            rc = self.lib.qldpc_dist_run_host(self.h, seed, trial_begin, trials, tp, ctypes.byref(bw),
                                              ctypes.byref(bt), wit.ctypes.data_as(vp))
            self._native.check(rc, "qldpc_dist_run_host")
        assert not (wit[-1] >> np.uint64(1) >> np.uint64((self.n - 1) % 64)), "witness bits past column n"
        return bw.value, bt.value, self._codes._unpack_row(wit, self.n), tmin

    def close(self):
        if self.h:
            self.lib.qldpc_dist_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def run_raw(G, P, trials, seed=0, trial_begin=0, device=-1, workgroups=0):
    """One handle, one run: (weight, trial, trial_min, witness, geometry)."""
    with Handle(G, P, device) as h:
        bw, bt, wit, tmin = h.run(trials, seed, trial_begin, workgroups)
        return bw, bt, tmin, wit, h.geometry()

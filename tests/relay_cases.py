"""Shared inputs of the Relay-BP pinning tests (tests/test_relay_cases_cpu.py, tests/test_gpu_relay_cases.py).

Plain numpy, deterministic, no GPU.  Engine 7 (csrc/relay.hip) on what no bundled code gives it:

* **irregular graphs**: the tests/bp_cases.py graphs (column degrees 1..12, rows of 13..64, empty rows
  and columns, ``[A | I]``, one row, one column), their syndromes (``bp_cases.mixed``) and their prior
  kinds, plus ``flipped``: the non-uniform priors with 0.7 where ``half`` has 0.5, which gives negative
  L0 and negative integer solution weights;
* **the solution-choice set**: frozen syndromes on which the chain, under the Python law
  (tests/relay_ref.py), replaces an earlier solution by a lighter one, keeps it on a tie between
  different decision vectors, or keeps it against a heavier one (``solution_classes``);
* **geometry cases**: graphs at the edges of every decision ``qldpc_bp_create_relay`` takes on its own
  (messages in LDS or in the HBM workspace, the 16-bit index copy or the global walk, 256 / 512 / 1024
  threads, the creation envelope), with the expectation computed here by ``relay_lds`` /
  ``relay_threads`` / ``expected``, restated from the comments of relay.hip and not taken from the
  library.

In ``expected`` the library's ``E, n, m <= 0xffff`` terms of the index decision do not appear: they are
implied by the LDS fit (a 16-bit copy of 65,536 edges alone is 256 KiB, 65,536 variables hold 640 KiB
of state, 65,536 checks 192 KiB), so no graph can separate them.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import bp_cases as bc
from qldpc_fault_tolerance_amd.codes import CSR

SEED = 0x9E3779B97F4A7C15
PRECISIONS = (64, 32)
PRIORS = bc.PRIORS + ("flipped",)
LEVEL = 0.05                  # the prior level of every decoder here
FLIPPED_P = 0.7

# ---------------------------------------------------------------------------------- relay settings
# (pre_iter, pre_gamma, num_legs, leg_iter, stop_nconv): chains of at most 36 iterations, gammas from
# [-0.24, 0.66] by SEED
SETTINGS = {
    "s1": (4, 0.125, 3, 4, 1),
    "s2": (4, 0.125, 4, 4, 2),
    "s8": (4, 0.125, 8, 4, 8),
}
# (setting, ms_scaling_factor) pairs every irregular case is decoded under: both alpha schedules
PAIRS = (("s1", 0.0), ("s2", 0.625), ("s8", 0.625), ("s8", 0.0))
PAIR_IDS = [f"{s}-a{a}" for s, a in PAIRS]
GAMMA_LO, GAMMA_HI = -0.24, 0.66


def relay_kwargs(setting: str) -> dict:
    t0, g0, legs, tr, stop = SETTINGS[setting]
    return dict(pre_iter=t0, pre_gamma=g0, num_legs=legs, leg_iter=tr, gamma_lo=GAMMA_LO, gamma_hi=GAMMA_HI,
                stop_nconv=stop, gamma_seed=SEED)


# ---------------------------------------------------------------------------------- irregular cases
IRREGULAR_IDS = ("col1to8", "col1to12", "row13", "row33", "row64", "holes", "a_i", "one_row", "one_col", "m65")
LAW_IDS = tuple(c for c in IRREGULAR_IDS if bc.CASES[c].n <= 132)  # the Python law is slow past that
B_IRREGULAR = 96              # syndromes of ``bp_cases.mixed`` per case (the tiny graphs: all of them, cycled)
# decode classes of the B_IRREGULAR syndromes under CLASS_PAIR (stop_nconv 1: the chain ends at its
# first solution), counted over the four prior kinds together: "first" converges in the first leg,
# "later" in a later one, "unsolved" never.  Every case holds IRREGULAR_NEEDED of each, except
# (one_row holds all three: a later leg's unequal gammas part its five tied variables)
CLASS_PAIR = ("s1", 0.0)
ABSENT = {
    "one_col": {"later": "one variable under five degree-1 checks gets the same five sentinel-sized messages "
                         "in every iteration of every leg: no bias outweighs them, its decision never changes"},
}
IRREGULAR_NEEDED = 3


def priors_of(n: int, kind: str, level: float = LEVEL) -> np.ndarray:
    """``bp_cases.priors_of`` with the kind ``flipped``: the non-uniform priors with three priors of
    0.7, at the positions where ``half`` has its 0.5."""
    if kind != "flipped":
        return bc.priors_of(n, kind, level)
    p = np.array(bc.priors_of(n, "nonuniform", level))
    p[special_positions(n)] = FLIPPED_P
    p.setflags(write=False)
    return p


def special_positions(n: int) -> list:
    """Where ``half`` puts 0.5 and ``flipped`` 0.7 (the rule of ``bp_cases.priors_of``)."""
    return sorted({min(2, n - 1), n // 2, n - 1})


@lru_cache(maxsize=None)
def dense(case_id: str) -> np.ndarray:
    """The parity-check matrix of a bp_cases graph or of one of OWN, uint8 [m, n], read-only."""
    if case_id == HGP:
        from qldpc_fault_tolerance_amd import codes

        H = np.ascontiguousarray(np.asarray(codes.get_code(HGP).hz, dtype=np.uint8))
    else:
        return bc.graph(case_id)
    H.setflags(write=False)
    return H


@lru_cache(maxsize=None)
def graph(case_id: str) -> CSR:
    return CSR.from_dense(dense(case_id))


@lru_cache(maxsize=None)
def priors(case_id: str, kind: str) -> np.ndarray:
    return priors_of(graph(case_id).n, kind)


@lru_cache(maxsize=None)
def mixed(case_id: str, B: int) -> np.ndarray:
    """``bp_cases.mixed`` of a bp_cases graph; on the graphs of OWN the same rule (``syndromes_of`` at the
    bp_cases levels with the graph's own seed, then ``mixed_of``)."""
    if case_id not in OWN:
        return bc.mixed(case_id, B)
    seed = OWN[case_id]
    return bc.mixed_of([bc.syndromes_of(dense(case_id), seed, i, lv) for i, lv in enumerate(bc.LEVELS)], seed, B)


def irregular_classes(iters, conv, pre_iter: int) -> dict:
    iters, conv = np.asarray(iters), np.asarray(conv).astype(bool)
    return {"first": int((conv & (iters <= pre_iter)).sum()), "later": int((conv & (iters > pre_iter)).sum()),
            "unsolved": int((~conv).sum())}


# ---------------------------------------------------------------------------------- solution choice
HGP = "hgp_34_n225"
OWN = {HGP: 225}              # graphs with syndromes of their own: the seed of ``mixed``
CHOICE_SETTING = "s8"         # T0 = 4, 8 legs of 4, stop_nconv 8
CHOICE_ALPHA = 0.625
POOL = 300                    # the search pool: the first POOL of ``mixed(case, POOL)``
POOL_GRAPHS = ("row13", "row33", "row64", HGP)
CLASSES = ("replaced", "tie_kept", "heavier_kept")
CHOICE_NEEDED = 3


def solution_classes(trace) -> set:
    """The decisions the chain took among its solutions ``trace`` ((leg, weight, decisions) per
    solution, ``relay_ref.decode_one``): ``replaced`` a lighter solution took the place of an earlier
    one, ``tie_kept`` the earlier one stayed against a different decision vector of equal weight,
    ``heavier_kept`` it stayed against a heavier one.  A repeat of the kept vector is no decision."""
    out = set()
    best = None
    for _, w, dec in trace:
        if best is None:
            best = (w, dec)
        elif w < best[0]:
            out.add("replaced")
            best = (w, dec)
        elif w == best[0] and dec != best[1]:
            out.add("tie_kept")
        elif w > best[0]:
            out.add("heavier_kept")
    return out


def law_traces(oracle, case_id: str, kind: str, precision: int, synd, setting=CHOICE_SETTING, alpha=CHOICE_ALPHA):
    """The Python law on ``synd`` -> ((corr, iters, conv, nsol) arrays, the trace of every decode)."""
    import relay_ref

    H = graph(case_id)
    t0, g0, legs, tr, stop = SETTINGS[setting]
    l0, wq = relay_ref.priors(priors(case_id, kind), precision)
    gam = relay_ref.gammas(oracle, H.n, g0, legs, GAMMA_LO, GAMMA_HI, SEED, precision)
    traces, out = [], []
    for s in np.atleast_2d(synd):
        tr_ = []
        out.append(relay_ref.decode_one(H, l0, wq, gam, t0, legs, tr, stop, float(alpha), int(precision), s, trace=tr_))
        traces.append(tr_)
    res = (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32),
           np.array([o[2] for o in out], bool), np.array([o[3] for o in out], np.int32))
    return res, traces


# The frozen set: (graph, prior kind, indices into ``mixed(graph, POOL)``), found by ``law_traces`` over
# the pool (every POOL_GRAPHS graph under every prior kind, both precisions) and kept where a decode
# is of the same class in both precisions.  tests/test_relay_cases_cpu.py recounts the classes.
#
# No decode of the pool is a ``tie_kept`` under ``half``: its three zero weights sit on columns 2, n // 2
# and n - 1, and two solutions tie through them only if some of these columns sum to zero, which they
# do on no bp_cases graph and not on hgp_34_n225 (on one_row columns 2 and 4 are equal, get equal
# messages and decide alike).  Counted with this setting under both alpha schedules, POOL syndromes
# each, fp64: 0 ties under ``half`` on the 19 bp_cases graphs with n <= 260 and on hgp_34_n225.  The ties of the set
# are those of equal weights: all of them (``uniform``) or the tied fourth of the non-uniform priors
# (``nonuniform``, ``flipped``).
CHOICE = (
    ("row33", "uniform", (7, 11, 22, 76, 128)),
    ("row33", "nonuniform", (3, 7, 22, 27, 29, 55, 68, 152, 206, 233)),
    ("row33", "flipped", (13, 41, 46, 63)),
    ("row13", "half", (7, 16, 28)),
    ("row64", "flipped", (6, 118, 246)),
    ("row64", "nonuniform", (31,)),
    (HGP, "flipped", (29, 81, 155)),
    (HGP, "uniform", (4, 116)),
)
CHOICE_IDS = [f"{c}-{k}" for c, k, _ in CHOICE]
# indices of row33 / nonuniform with no solution at all: they join the reuse batch of the GPU test
CHOICE_UNSOLVED = ("row33", "nonuniform", (2, 8, 10, 14))


def choice_syndromes(entry) -> np.ndarray:
    case_id, _, idx = entry
    return np.ascontiguousarray(mixed(case_id, POOL)[list(idx)])


# ---------------------------------------------------------------------------------- geometry cases
LDS_MAX = 160 * 1024
GEO_RELAY = dict(pre_iter=4, pre_gamma=0.125, num_legs=2, leg_iter=4, gamma_lo=GAMMA_LO, gamma_hi=GAMMA_HI,
                 stop_nconv=2, gamma_seed=SEED)
GEO_B = 16
GEO_P = 0.02
BALANCED_MAX = 1 << 23        # m n up to which a geometry graph is made dense by ``bp_cases.balanced``


def relay_lds(precision: int, m: int, n: int, E: int, lds_messages: bool, lds_index: bool) -> int:
    """The dynamic LDS of a relay workgroup: [b2c, c2b: 2E values when in LDS][M: n values, rounded up
    to 8 bytes][weight word: 8][flags: 2 x 4][dec: n][best: n][syndrome: m], then, when the indices are
    staged, from the next even address [rp: m + 1][cp: n + 1][ci: E][ce: E] as 16-bit words; the part
    after the messages is rounded up to 16 bytes."""
    ts = 4 if int(precision) == 32 else 8
    tail = ((n * ts + 7) & ~7) + 16 + 2 * n + m
    if lds_index:
        tail = ((tail + 1) & ~1) + 2 * ((m + 1) + (n + 1) + 2 * E)
    return (2 * E * ts if lds_messages else 0) + (tail + 15) // 16 * 16


def resident(lds_bytes: int) -> int:
    """Workgroups LDS leaves resident on a CU, of the 8 that 256-thread workgroups can reach."""
    return max(1, min(8, LDS_MAX // max(1, lds_bytes)))


def relay_threads(lds_bytes: int, m: int, n: int) -> int:
    """256 threads, doubled up to 1024 while the resident workgroups stay within the CU's 32 waves and
    there are rows or columns left for the new threads."""
    tb = 256
    while tb < 1024 and resident(lds_bytes) * (2 * tb // 64) <= 32 and tb < max(m, n):
        tb *= 2
    return tb


def expected(precision: int, m: int, n: int, E: int):
    """(messages in LDS, indices in LDS, threads, lds_bytes) of ``qldpc_bp_create_relay`` with no
    environment switch set, or None where creation answers QLDPC_ENOTSUP."""
    msgs = relay_lds(precision, m, n, E, True, False) <= LDS_MAX
    lds = relay_lds(precision, m, n, E, msgs, False)
    if lds > LDS_MAX:
        return None
    lds_idx = relay_lds(precision, m, n, E, msgs, True)
    idx = lds_idx <= LDS_MAX and resident(lds_idx) == resident(lds)
    if idx:
        lds = lds_idx
    return msgs, idx, relay_threads(lds, m, n), lds


@dataclass(frozen=True)
class Geo:
    id: str
    m: int
    n: int
    degrees: tuple            # ((degree, columns), ..): the column degrees in runs, in this order
    seed: int
    note: str

    @property
    def E(self) -> int:
        return sum(d * c for d, c in self.degrees)

    def expected(self, precision: int):
        return expected(precision, self.m, self.n, self.E)


_GEO = [
    Geo("w256", 100, 200, ((3, 200),), 301, "small image: 8 resident workgroups, 256 threads"),
    Geo("narrow256", 256, 256, ((12, 256),), 302, "3 (fp64) resident: max(m, n) = 256 stops the doubling at 256"),
    Geo("narrow512", 200, 400, ((8, 400),), 303, "2 (fp64) resident: max(m, n) = 400 stops the doubling at 512"),
    Geo("idx_kept", 540, 1080, ((3, 1080),), 304, "fp64: 2 resident with and without the index copy: staged"),
    Geo("idx_dropped", 690, 1380, ((3, 1380),), 305, "fp64: the index copy would leave 1 of 2 resident: global walk"),
    Geo("auto_ws", 1600, 3200, ((3, 3200),), 306, "fp64 image 187,216 bytes: the workspace without the switch"),
    Geo("auto_ws32", 3200, 6400, ((3, 6400),), 307, "fp32 image 195,216 bytes: the fp32 workspace"),
    Geo("image_at_limit", 1024, 3000, ((2, 700), (3, 2300)), 308, "fp64 image = 163,840 exactly: LDS, 1024 threads"),
    Geo("image_over", 1025, 3000, ((2, 700), (3, 2300)), 309, "one more row: fp64 image 163,856, the workspace"),
    Geo("image32_at_limit", 1024, 3000, ((6, 2900), (7, 100)), 310, "fp32 image = 163,840 exactly"),
    Geo("image32_over", 1025, 3000, ((6, 2900), (7, 100)), 311, "one more row: fp32 image 163,856, the workspace"),
    Geo("state_at_limit", 3824, 16000, ((1, 16000),), 312, "fp64 state 10 n + 16 + m = 163,840: admitted"),
    Geo("state_over", 3825, 16000, ((1, 16000),), 313, "fp64 state 163,841: QLDPC_ENOTSUP"),
    Geo("state32_at_limit", 1824, 27000, ((1, 27000),), 314, "fp32 state 6 n + 16 + m = 163,840: admitted"),
    Geo("state32_over", 1825, 27000, ((1, 27000),), 315, "fp32 state 163,841: QLDPC_ENOTSUP (fp64 too)"),
    Geo("ws_idx", 3000, 9000, ((1, 9000),), 316, "fp64: workspace, and the index copy beside the state keeps 1 resident"),
    Geo("ws_idx32", 6, 13650, ((1, 13650),), 317, "fp32: workspace, state + index copy = 163,838, rounded 163,840"),
    Geo("big", 6000, 12000, ((6, 12000),), 318, "E = 72,000 past the 16-bit range: workspace, global walk, 1024 threads"),
]
GEO = {g.id: g for g in _GEO}
GEO_IDS = [g.id for g in _GEO]
GEO_SIDE_IDS = ("auto_ws", "idx_dropped", "image_at_limit")  # the side decode's geometry cases (the last: 1024 threads)

# column j of a large geometry graph sits on rows (a_k j + b_k) % m, k < degree (the rule of
# firstmin_cases.envelope_graph: a CSR, never dense)
_MULT = (1, 7, 13, 29, 37, 43)
_OFFS = (0, 1, 5, 11, 17, 23)


@lru_cache(maxsize=None)
def geo_graph(geo_id: str) -> CSR:
    g = GEO[geo_id]
    deg = np.concatenate([np.full(c, d, np.int64) for d, c in g.degrees])
    assert deg.shape == (g.n,)
    if g.m * g.n <= BALANCED_MAX:
        csr = CSR.from_dense(bc.balanced(g.m, g.n, deg, g.seed))
    else:
        j = np.arange(g.n, dtype=np.int64)
        K = int(deg.max())
        r = np.stack([(_MULT[k] * j + _OFFS[k]) % g.m for k in range(K)])      # [K, n]
        keep = np.arange(K)[:, None] < deg[None, :]
        for b in range(1, K):  # distinct rows per column: a slot that meets an earlier one moves on by one row
            while True:
                clash = (r[:b] == r[b]).any(axis=0)
                if not clash.any():
                    break
                r[b, clash] = (r[b, clash] + 1) % g.m
        rows, cols = r[keep], np.broadcast_to(j, r.shape)[keep]
        order = np.lexsort((cols, rows))
        row_ptr = np.zeros(g.m + 1, np.int64)
        np.add.at(row_ptr, rows + 1, 1)
        csr = CSR(g.m, g.n, np.cumsum(row_ptr).astype(np.int32), cols[order].astype(np.int32))
    assert int(csr.row_ptr[-1]) == g.E
    return csr


@lru_cache(maxsize=None)
def geo_syndromes(geo_id: str, B: int = GEO_B) -> np.ndarray:
    """``B`` syndromes of i.i.d. errors, a quarter each at a mean weight of 1, 3, 8 and 24, the first
    the zero syndrome."""
    csr = geo_graph(geo_id)
    rng = np.random.default_rng([GEO[geo_id].seed, 4, B])
    rate = np.array([1.0, 3.0, 8.0, 24.0])[np.arange(B) % 4] / csr.n
    e = (rng.random((B, csr.n)) < rate[:, None]).astype(np.uint8)
    e[0] = 0
    S = np.ascontiguousarray(csr.matvec(e).astype(np.uint8))
    S.setflags(write=False)
    return S


def geo_priors(geo_id: str, kind: str = "nonuniform") -> np.ndarray:
    return priors_of(GEO[geo_id].n, kind, GEO_P)


def side_bytes(seed, B: int, n: int, density: float = 0.3) -> np.ndarray:
    """Seeded side bytes [B, n]: bit 0 set at ``density``, noise in the bits the decoders must ignore."""
    rng = np.random.default_rng(seed)
    return (((rng.random((B, n)) < density).astype(np.uint8)) | (rng.integers(0, 128, (B, n)).astype(np.uint8) << 1)).astype(np.uint8)


# ---------------------------------------------------------------------------------- side decodes
# the second prior table of a side decode on a solution-choice entry: another kind than the entry's own
SIDE_P1 = {"uniform": "flipped", "nonuniform": "flipped", "flipped": "uniform", "half": "flipped"}
SIDE_DENSITY = 0.3


def side_case(entry):
    """(graph, p0, p1, syndromes, side bytes) of a side decode on a solution-choice entry."""
    case_id, kind, idx = entry
    H = graph(case_id)
    side = side_bytes([OWN.get(case_id) or bc.CASES[case_id].seed, 5, len(idx)], len(idx), H.n, SIDE_DENSITY)
    return H, priors(case_id, kind), priors(case_id, SIDE_P1[kind]), choice_syndromes(entry), side


def kept_of(trace, weight=None):
    """The decision vector the chain keeps among the solutions of ``trace`` (strictly lighter replaces),
    by the recorded weights or by ``weight(decisions)``; None without a solution."""
    best = None
    for _, w, dec in trace:
        if weight is not None:
            w = weight(dec)
        if best is None or w < best[0]:
            best = (w, dec)
    return None if best is None else best[1]


def side_weight_decides(oracle, entry, precision: int) -> list:
    """Positions of the entry's syndromes whose side decode, under the Python law, keeps another
    solution than the same chain judged by row 0's weights alone (a kernel that read every weight
    from row 0 of its table would keep that one)."""
    import relay_ref
    import side_ref

    H, p0, p1, synd, side = side_case(entry)
    t0, g0, legs, tr, stop = SETTINGS[CHOICE_SETTING]
    l0a, wqa = relay_ref.priors(p0, precision)
    l0b, wqb = relay_ref.priors(p1, precision)
    gam = relay_ref.gammas(oracle, H.n, g0, legs, GAMMA_LO, GAMMA_HI, SEED, precision)
    out = []
    for b, (s, sb) in enumerate(zip(synd, side)):
        trace = []
        relay_ref.decode_one(H, side_ref.select(l0a, l0b, sb), side_ref.select(wqa, wqb, sb), gam, t0, legs, tr, stop,
                             CHOICE_ALPHA, int(precision), s, trace=trace)
        if trace and kept_of(trace) != kept_of(trace, lambda dec: sum(w for w, d in zip(wqa, dec) if d)):
            out.append(b)
    return out

"""CSS codes whose X and Z sectors differ, for the shot loops (tests/test_css_cases_cpu.py on the
CPU, tests/test_gpu_css_cases.py on the GPU).  Plain numpy: nothing here needs the library or a GPU.

Every bundled code but one has hx.shape == hz.shape and equal degrees, so a sector reading the
other's row count, slot count, logical mask or trace offset passes any test on it.  The codes here
have m_x != m_z (two of them also sectors whose engine-3 slot maps differ: ``slot_order``), and
every one runs in both orientations: "swapped" is
``CSSCode.from_checks(hz, hx, lx=lz, lz=lx)``, so that the larger sector is decoder X (the hz
decoder) in one orientation and decoder Z in the other.

Per case the table freezes what the host decides for it (checked against ``plan_bp`` and against
the conditions of ``qldpc_mc_create`` by test_css_cases_cpu.py) and the error rates at which the
oracle's decodes are neither all trivial nor all failures (checked there too).
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from qldpc_fault_tolerance_amd import codes
from qldpc_fault_tolerance_amd.codes import CSSCode

MAX_ITER = 20
# the shot ranges of the GPU tests; the rates below are chosen, and checked, on exactly these
MC_SEED, MC_SHOT0, MC_SHOTS = 0xC55, 0, 600
PHEN_SEED, PHEN_SHOT0, PHEN_SHOTS, PHEN_ROUNDS, PHEN_REPS = 7, 0, 333, 3, (2, 3)
PRECISIONS = (64, 32)
ORIENTATIONS = (False, True)  # swapped?
PLAN_KEYS = ("engine", "kernel_id", "row_chunks", "threads", "vars_per_thread", "degree3_slots")


def ring(n):
    """The n x n cyclic repetition-code checks: row i on columns i and i + 1 (mod n)."""
    H = np.zeros((n, n), np.uint8)
    for i in range(n):
        H[i, i] = H[i, (i + 1) % n] = 1
    return H


def _biregular(m, n, dc, dv, seed):
    """A random (dv, dc)-regular m x n parity-check matrix (configuration model, no double edges)."""
    rng = np.random.default_rng(seed)
    while True:
        stubs = np.repeat(np.arange(n), dv)
        rng.shuffle(stubs)
        H = np.zeros((m, n), np.uint8)
        ok = True
        for i in range(m):
            for j in stubs[i * dc:(i + 1) * dc]:
                ok = ok and not H[i, j]
                H[i, j] = 1
        if ok:
            return H


def asymmetric_hgp():
    """HGP of a (3,4)-regular 6x8 h1 and a rank-deficient (3,3)-regular 8x8 h2: hx is all
    degree 3 (rows of 7), hz has 64 degree-3 and 48 degree-4 columns (rows of 6).  With 4 variables per
    thread (64 lanes) both sectors qualify for the one-word fp64 families, with different degree-3
    slot counts (hx 4, hz 1)."""
    from qldpc_fault_tolerance_amd import gf2

    h2 = next(h for h in (_biregular(8, 8, 3, 3, 100 + s) for s in range(64)) if gf2.rank(h) < 8)
    return codes.hgp(_biregular(6, 8, 4, 3, 7), h2, name="hgp_asym_112")


@dataclass(frozen=True)
class Case:
    """One code.  ``hx`` / ``hz``: the sector shapes.  ``p``, ``split``: the data-error loop's channel
    is (px, py, pz) = p * split (swapped orientation: px and pz change places, so each sector keeps
    its own rate); the decoders' priors are px + py (hz decoder) and pz + py (hx decoder), as
    ``oracle.mc_run`` takes them.  ``phen``: (p, q) of the phenomenological loop, channel p * split,
    syndrome flips q, decoder priors p_data = p, p_synd = q.  ``plans[precision]``: the ``plan_bp``
    tuples (PLAN_KEYS) of the hz and the hx decoder.  ``path[precision,
    swapped]``: what ``qldpc_mc_create`` makes of that pair in that orientation."""

    hx: tuple
    hz: tuple
    NK: tuple
    p: float
    split: tuple
    phen: tuple
    plans: dict
    path: dict


def _paths(p64, p32):
    return {(64, False): p64, (64, True): p64, (32, False): p32, (32, True): p32}


HALF = (0.5, 0.5, 0.5)  # the reference's EvalWER data branch: px = py = pz = p / 2

CASES = {
    # smaller than one wave, 1 variable per thread; fp64 rows of 3 and 4 edges both take 2 chunks
    "asym15": Case(hx=(9, 15), hz=(6, 15), NK=(15, 1), p=0.05, split=HALF, phen=(0.03, 0.03),
                   plans={64: ((3, 3, 2, 64, 1, 0), (3, 3, 2, 64, 1, 0)), 32: ((3, 3, 1, 64, 1, 1), (3, 3, 1, 64, 1, 1))},
                   path=_paths("fused", "fused")),
    # fp64: row_chunks 3 vs 4 at equal 64 x 2 geometry (run-time nch); fp32: degree3_slots 1 vs 2 (min)
    "asym112": Case(hx=(48, 112), hz=(64, 112), NK=(112, 6), p=0.015, split=HALF, phen=(0.006, 0.006),
                    plans={64: ((3, 3, 3, 64, 2, 0), (3, 3, 4, 64, 2, 0)), 32: ((3, 3, 2, 64, 2, 1), (3, 3, 2, 64, 2, 2))},
                    path=_paths("fused", "fused")),
    # degree-1 and degree-2 columns; degree3_slots 2 vs 4 in both precisions (fp64: the 103 family)
    "asym230": Case(hx=(105, 230), hz=(120, 230), NK=(230, 6), p=0.02, split=HALF, phen=(0.008, 0.008),
                    plans={64: ((3, 103, 3, 64, 4, 2), (3, 103, 3, 64, 4, 4)),
                           32: ((3, 3, 2, 64, 4, 2), (3, 3, 2, 64, 4, 4))},
                    path=_paths("fused", "fused")),
    # asym112 and asym230 with their columns permuted.  Every product above lists its columns of degree
    # <= 3 first in both sectors, so the engine-3 slot maps (degree <= 3 variables first, stably) of hx
    # and hz are both the identity there; here hz's map is a permutation and hx's is not, and whatever a
    # fused kernel keys by (thread, variable slot) means different variables in the two sectors.
    "asym112p": Case(hx=(48, 112), hz=(64, 112), NK=(112, 6), p=0.015, split=HALF, phen=(0.006, 0.006),
                     plans={64: ((3, 3, 3, 64, 2, 0), (3, 3, 4, 64, 2, 0)), 32: ((3, 3, 2, 64, 2, 1), (3, 3, 2, 64, 2, 2))},
                     path=_paths("fused", "fused")),
    "asym230p": Case(hx=(105, 230), hz=(120, 230), NK=(230, 6), p=0.02, split=HALF, phen=(0.008, 0.008),
                     plans={64: ((3, 103, 3, 64, 4, 2), (3, 103, 3, 64, 4, 4)),
                            32: ((3, 3, 2, 64, 4, 2), (3, 3, 2, 64, 4, 4))},
                     path=_paths("fused", "fused")),
    # sectors on different geometries (fp32: 64 x 6 vs 128 x 3) and engines (fp64: 3 vs 2).  hz has 180
    # degree-1 columns and fails on nearly every X error while hx seldom fails: only a Z-biased
    # channel leaves shots where the hx sector alone fails.
    "tanner_code1": Case(hx=(240, 360), hz=(120, 360), NK=(360, 8), p=0.03, split=(0.07, 0.02, 1.0),
                         phen=(0.01, 0.01),
                         plans={64: ((3, 103, 3, 64, 6, 6), (2, 2, 4, 256, 2, 0)),
                                32: ((3, 3, 2, 64, 6, 6), (3, 3, 2, 128, 3, 1))},
                         path=_paths("staged", "staged")),
}
CASE_IDS = list(CASES)
FUSED_IDS = [c for c in CASE_IDS if set(CASES[c].path.values()) == {"fused"}]


def _build(case_id) -> CSSCode:
    if case_id == "asym15":
        return codes.hgp(ring(3), np.array([[1, 1, 0], [0, 1, 1]], np.uint8), name="asym15")
    if case_id == "asym112":
        return asymmetric_hgp()
    if case_id == "asym230":
        return codes.hgp(_biregular(15, 20, 4, 3, 9), ring(7)[:-1], name="asym230")
    if case_id in ("asym112p", "asym230p"):
        c = _build(case_id[:-1])
        perm = np.random.default_rng(c.N).permutation(c.N)
        return CSSCode.from_checks(c.hx[:, perm], c.hz[:, perm], name=case_id, lx=c.lx[:, perm], lz=c.lz[:, perm])
    return codes.get_code(case_id)


@lru_cache(maxsize=None)
def code(case_id, swapped=False) -> CSSCode:
    """The case's code; ``swapped``: hx and hz (and lx and lz) exchanged."""
    c = _build(case_id)
    if swapped:
        c = CSSCode.from_checks(c.hz, c.hx, name=c.name + "_swapped", lx=c.lz, lz=c.lx)
    for a in (c.hx, c.hz, c.lx, c.lz):
        a.setflags(write=False)
    return c


def pauli(case_id, swapped=False, phen=False):
    """(px, py, pz) of the case's data-error loop (``phen``: of its phenomenological loop)."""
    c = CASES[case_id]
    p = c.phen[0] if phen else c.p
    fx, fy, fz = c.split[::-1] if swapped else c.split
    return p * fx, p * fy, p * fz


def plans(case_id, precision, swapped=False):
    """(plan of decoder X = the hz decoder, plan of decoder Z = the hx decoder) in that orientation."""
    pz_, px_ = CASES[case_id].plans[precision]
    return (px_, pz_) if swapped else (pz_, px_)


def split_trace(trace, num_rounds, num_rep, m_x, m_z):
    """A phenomenological trace [S, trace_len] as (Z-sector detector histories [S, R - 1, num_rep, m_x],
    X-sector histories [S, R - 1, num_rep, m_z], final Z-sector syndromes [S, m_x], final X-sector
    syndromes [S, m_z]): per noisy round the Z block (hx rows) comes before the X block (hz rows)."""
    trace = np.asarray(trace)
    S, R1 = trace.shape[0], num_rounds - 1
    wz, wx = num_rep * m_x, num_rep * m_z
    assert trace.shape[1] == R1 * (wz + wx) + m_x + m_z, (trace.shape, num_rounds, num_rep, m_x, m_z)
    body = trace[:, :R1 * (wz + wx)].reshape(S, R1, wz + wx)
    fin = trace[:, R1 * (wz + wx):]
    return (body[:, :, :wz].reshape(S, R1, num_rep, m_x), body[:, :, wz:].reshape(S, R1, num_rep, m_z),
            fin[:, :m_x], fin[:, m_x:])


def slot_order(H):
    """The variable order of an engine-3 decoder's slots on ``H`` (``degree_sorted(g, {3})`` of
    csrc/qldpc_hip.hip): columns of degree <= 3 first, then the others, each in column order."""
    return np.argsort(np.asarray(H).sum(0) > 3, kind="stable")


def mc_path(plan_x, plan_z, colmax_x, colmax_z, precision):
    """``"fused"`` or ``"staged"``: the conditions of ``qldpc_mc_create`` (csrc/qldpc_hip.hip) on the
    PLAN_KEYS tuples of the two sector decoders and their graphs' largest column degrees, for the
    kernel ids this table reaches: 2 (engine 2) and the plain engine-3 layout (3; 103 is its fp64
    variant with a compile-time row width), which carries none of the layout flags (tail, one-slot,
    byte F, packed) that send a pair to the staged pipeline.  One fused kernel then serves a pair on
    the same engine, threads, vars per thread and degree class (4 slots for column degree <= 4;
    engine 3 has its own for 5, and 6 in fp32; 8 otherwise).  Row counts, row_chunks and degree-3 slot counts may differ:
    the kernel takes the larger image, the run-time row width and the smaller slot count."""
    def dmax(colmax, engine):
        if colmax <= 4:
            return 4
        return colmax if engine == 3 and (colmax == 5 or (precision == 32 and colmax == 6)) else 8

    (ex, kx, _, tx, vx, _), (ez, kz, _, tz, vz, _) = plan_x, plan_z
    if not {kx, kz} <= {2, 3, 103}:
        raise NotImplementedError(f"kernel ids {kx}, {kz}: restate their conditions of qldpc_mc_create here")
    same = (ex, tx, vx, dmax(colmax_x, ex)) == (ez, tz, vz, dmax(colmax_z, ez))
    return "fused" if same else "staged"


def phen_noisy_round(code, U, px, py, pz, q, num_rep):
    """One noisy round of ``CodeSimulator_Phenon_SpaceTime._single_run`` (the reference's
    src/Simulators_SpaceTime.py:405-481) from external uniforms, in plain numpy, written from that
    file alone: ``U`` [S, >= num_rep * (N + m_x + m_z)], one block of N + m_x + m_z uniforms per
    repetition.  A block's first N uniforms split the data qubits (u < pz: Z; pz <= u < pz + px: X;
    pz + px <= u < pz + px + py: Y), the next m_x flip the hx-row measurements (u < q), the last m_z
    the hz-row measurements.  Data errors accumulate over the repetitions, measurement flips do
    not.  Returns (Z-sector detectors [S, num_rep, m_x]: each repetition's hx syndrome XOR the one
    before it, the first one raw; X-sector histories [S, num_rep, m_z]: the raw hz syndromes, which
    the reference does not difference).  The reference itself allocates the Z history with hz's row
    count (:455) and so raises on m_x != m_z; the width here is that of the syndrome it stores there."""
    U = np.asarray(U, np.float64)
    S, n = U.shape[0], code.N
    hx, hz = code.hx.astype(np.int64), code.hz.astype(np.int64)
    m_x, m_z = hx.shape[0], hz.shape[0]
    ex, ez = np.zeros((S, n), np.int64), np.zeros((S, n), np.int64)
    synd_z, synd_x = np.zeros((S, num_rep, m_x), np.int64), np.zeros((S, num_rep, m_z), np.int64)
    for j in range(num_rep):
        blk = U[:, j * (n + m_x + m_z):(j + 1) * (n + m_x + m_z)]
        u = blk[:, :n]
        new_z = (u < pz) | ((pz + px <= u) & (u < pz + px + py))
        new_x = ((pz <= u) & (u < pz + px)) | ((pz + px <= u) & (u < pz + px + py))
        ez, ex = (ez + new_z) % 2, (ex + new_x) % 2
        synd_z[:, j] = (ez @ hx.T + (blk[:, n:n + m_x] < q)) % 2
        synd_x[:, j] = (ex @ hz.T + (blk[:, n + m_x:] < q)) % 2
    det_z = synd_z.copy()
    det_z[:, 1:] = (synd_z[:, 1:] + synd_z[:, :-1]) % 2
    return det_z.astype(np.uint8), synd_x.astype(np.uint8)

"""CPU tests of the random information-set distance search: the host path of ``qldpc_dist_*``
against the NumPy restatement (``distance_ref.py``), known distances, witnesses, trial ranges,
and the ``codes`` surface built on it (``classical_distance``, ``hgp(compute_distance=True)``,
``random_biregular_check_matrix(min_distance=...)``)."""
import ctypes
import itertools

import numpy as np
import pytest

import distance_ref as ref
from distance_cases import run_raw
from qldpc_fault_tolerance_amd import _native, codes, gf2

SYNTH_SEED = 0x51D5EED0  # tools/synth_hgp_codes.py
SYNTH_JOBS = [("hgp_34_n625", 5), ("hgp_34_n1225_q3", 7), ("hgp_34_n1600", 8)]


def ring(d):
    """Cyclic repetition-code checks: hgp(ring(d), ring(d)) is the distance-d toric code."""
    I = np.eye(d, dtype=np.uint8)
    return (I + np.roll(I, 1, axis=1)) % 2


_CODES = {}


def get(name):
    if name not in _CODES:
        if name.startswith("toric"):
            d = int(name[5:])
            _CODES[name] = codes.hgp(ring(d), ring(d), name=name)
        elif name == "planar3":
            _CODES[name] = codes.hgp(ring(3)[:-1], ring(3)[:-1], name=name)
        else:
            _CODES[name] = codes.get_code(name)
    return _CODES[name]


def sector(name, kind):
    c = get(name)
    if kind == "C":  # the classical seed of an HGP code
        return c.h1, None
    return (c.hx, c.lx) if kind == "Z" else (c.hz, c.lz)


def brute_force_distance(H):
    """Minimum weight over all non-zero vectors of ker(H) (None if there is none)."""
    G = gf2.nullspace(H).astype(np.int64)
    k = G.shape[0]
    if k == 0:
        return None
    best = None
    for bits in itertools.product((0, 1), repeat=k):
        if any(bits):
            w = int(((np.array(bits) @ G) % 2).sum())
            best = w if best is None else min(best, w)
    return best


def hgp_theorem_distance(c):
    ds = [brute_force_distance(h) for h in (c.h1, c.h2, c.h1.T, c.h2.T)]
    return min(d for d in ds if d is not None)


# ------------------------------------------------- host path == restatement, bit for bit
CASES = [
    ("toric3", "X", 64), ("toric3", "Z", 64), ("toric5", "X", 64), ("toric5", "Z", 64),
    ("GenBicycleA1", "Z", 64), ("hgp_34_n225", "Z", 64),
    ("tanner_code1", "X", 64), ("tanner_code1", "Z", 64),
    ("LP_Matg8_L16_Dmin12", "Z", 4), ("hgp_34_n625", "C", 64),
]


@pytest.mark.parametrize("name,kind,trials", CASES)
def test_host_path_matches_restatement(oracle, name, kind, trials):
    H, L = sector(name, kind)
    G = gf2.nullspace(H)
    P = gf2.matmul(G, L.T) if L is not None else None
    bw, bt, wit, tmin = ref.search(oracle, G, P, seed=0, trial_begin=0, trials=trials)
    r = codes.distance_search(H, L, trials=trials, seed=0, backend="host")
    assert np.array_equal(r.trial_min, tmin)
    assert (r.weight, r.trial) == (bw, bt)
    assert np.array_equal(r.witness, wit)
    assert r.hits == int((tmin == bw).sum()) and r.trials == trials


def test_rank_deficient_and_unequal_sectors_are_what_the_cases_claim():
    c = get("hgp_34_n225")
    assert c.hx.shape[0] == 108 and gf2.rank(c.hx) == 104
    t = get("tanner_code1")
    assert sorted((gf2.nullspace(t.hx).shape[0], gf2.nullspace(t.hz).shape[0])) == [127, 241]
    assert get("LP_Matg8_L16_Dmin12").K == 80


# ------------------------------------------------------------------- known answers
@pytest.mark.parametrize("name,d", [("toric3", 3), ("toric5", 5), ("planar3", 3)])
def test_known_distance_small_codes(name, d):
    assert get(name).distance_bound(trials=64, seed=0, backend="host") == (d, d)


@pytest.mark.parametrize("name", ["hgp_34_n225", "hgp_34_n625"])
def test_known_distance_hgp_by_the_distance_theorem(name):
    c = get(name)
    d = hgp_theorem_distance(c)
    dx, dz = c.distance_bound(trials=64, seed=0, backend="host")
    assert min(dx, dz) == d and dx >= d and dz >= d
    assert codes.hgp(c.h1, c.h2, compute_distance=True).D == d
    assert codes.hgp(c.h1, c.h2).D is None  # the default leaves the code as it was


@pytest.mark.parametrize("name,kind", [("toric5", "X"), ("toric5", "Z"), ("GenBicycleA1", "X"), ("hgp_34_n225", "Z"),
                                       ("hgp_34_n625", "X"), ("hgp_34_n625", "C")])
def test_witness_is_a_logical_operator_of_the_reported_weight(name, kind):
    H, L = sector(name, kind)
    r = codes.distance_search(H, L, trials=16, seed=3, backend="host")
    assert r.weight is not None and int(r.witness.sum()) == r.weight
    assert not gf2.matmul(H, r.witness[:, None]).any()
    if L is not None:
        assert gf2.matmul(L, r.witness[:, None]).any()
    assert r.trial_min[r.trial] == r.weight and r.trial_min.min() == r.weight
    assert r.trial == int(np.flatnonzero(r.trial_min == r.weight)[0])


# -------------------------------------------------------------------- trial ranges
def test_split_range_concatenates():
    H, L = sector("hgp_34_n225", "X")
    full = codes.distance_search(H, L, trials=64, seed=7, backend="host")
    a = codes.distance_search(H, L, trials=32, seed=7, trial_begin=0, backend="host")
    b = codes.distance_search(H, L, trials=32, seed=7, trial_begin=32, backend="host")
    assert np.array_equal(np.concatenate([a.trial_min, b.trial_min]), full.trial_min)
    best = min((a, b), key=lambda r: (r.weight, r.trial))
    assert (best.weight, best.trial) == (full.weight, full.trial)
    assert np.array_equal(best.witness, full.witness)
    assert b.trial >= 32


def test_trial_begin_above_2_to_32(oracle):
    H, L = sector("toric3", "Z")
    G = gf2.nullspace(H)
    t0 = (1 << 32) + 5
    bw, bt, wit, tmin = ref.search(oracle, G, gf2.matmul(G, L.T), seed=(9 << 32) | 1, trial_begin=t0, trials=8)
    r = codes.distance_search(H, L, trials=8, seed=(9 << 32) | 1, trial_begin=t0, backend="host")
    assert np.array_equal(r.trial_min, tmin) and (r.weight, r.trial) == (bw, bt) and np.array_equal(r.witness, wit)


def test_dependent_and_zero_generator_rows_never_give_weight_zero(oracle):
    c = get("toric3")
    G0 = gf2.nullspace(c.hx)
    G = np.vstack([G0, np.zeros((2, c.N), np.uint8), G0[0] ^ G0[1], G0[:3]])  # zero, dependent and repeated rows
    P = gf2.matmul(G, c.lx.T)
    bw, _, tmin, wit, geo = run_raw(G, P, 32)
    assert tmin.min() >= 1 and bw == 3 and int(wit.sum()) == 3
    assert geo == [0, 1, 1, 0]  # host handle: no threads, no LDS; one code word, one pairing word
    # the extra rows change nothing: same pivots, same reduced rows
    plain = codes.distance_search(c.hx, c.lx, trials=32, seed=0, backend="host")
    assert np.array_equal(tmin, plain.trial_min) and np.array_equal(wit, plain.witness)
    # classical on the same generator: every pivot row counts, still none of weight 0
    bw2, _, tmin2, _, _ = run_raw(G, None, 32)
    assert tmin2.min() >= 1 and bw2 <= 3
    r = ref.search(oracle, G, None, 0, 0, 32)
    assert np.array_equal(r[3], tmin2)


def test_no_candidate_gives_none():
    r = codes.distance_search(np.eye(5, dtype=np.uint8), trials=4, backend="host")  # k' = 0
    assert r.weight is None and r.hits == 0 and not r.witness.any()
    assert (r.trial_min == ref.NO_CANDIDATE).all() and r.trial_min.dtype == np.int32
    c = get("toric3")
    # pairing that is identically zero (L inside the stabiliser group): pivots, but no candidate
    r = codes.distance_search(c.hx, c.hx[:2], trials=4, backend="host")
    assert r.weight is None and (r.trial_min == ref.NO_CANDIDATE).all()
    assert codes.classical_distance(np.eye(5, dtype=np.uint8)) is None


# --------------------------------------------------------------- the codes surface
@pytest.mark.parametrize("name", ["hgp_34_n225", "hgp_34_n625", "hgp_34_n1600"])
def test_classical_distance_enumeration_agrees_with_search(name):
    h = get(name).h1
    exact = codes.classical_distance(h)
    assert exact == brute_force_distance(h)  # k = 3, 5, 8
    assert codes.classical_distance(h, exact_max_k=0, trials=64, seed=0, backend="host") == exact
    assert codes.classical_distance(codes.CSR.from_dense(h)) == exact
    assert codes.classical_distance(h.T) == brute_force_distance(h.T)


def test_distance_search_takes_csr_and_validates():
    c = get("toric3")
    a = codes.distance_search(codes.CSR.from_dense(c.hx), codes.CSR.from_dense(c.lx), trials=8, backend="host")
    b = c.distance_search("Z", trials=8, backend="host")
    assert np.array_equal(a.trial_min, b.trial_min) and a.weight == b.weight
    with pytest.raises(ValueError):
        c.distance_search("Y")
    with pytest.raises(ValueError):
        codes.distance_search(c.hx, c.lx[:, :-1], backend="host")
    with pytest.raises(ValueError):
        codes.distance_search(c.hx, c.lx, backend="cpu")


@pytest.mark.parametrize("name,n0", SYNTH_JOBS)
def test_min_distance_default_keeps_the_committed_seeds(name, n0):
    """``min_distance=None`` draws the stream it always drew: the three synth_hgp_codes.py jobs
    still give the committed check matrices, byte for byte."""
    h = codes.random_biregular_check_matrix(n0, 4, 3, seed=SYNTH_SEED + n0, min_girth=6)
    want = get(name).h1
    assert h.dtype == want.dtype and h.tobytes() == want.tobytes()


def test_min_distance_rejects_instances_below_the_bound():
    """The filter on a 12 x 16 graph (girth 4, so a try is cheap): the default call succeeds, a
    reachable bound above the default instance's distance gives another instance that meets it,
    and a bound no 16-bit code can meet (17) turns every try down."""
    kw = dict(seed=13, min_girth=4, max_tries=50)
    h = codes.random_biregular_check_matrix(4, 4, 3, **kw)
    d = brute_force_distance(h)
    assert d is not None and d >= 1
    assert np.array_equal(codes.random_biregular_check_matrix(4, 4, 3, min_distance=d, **kw), h)  # already met
    h2 = codes.random_biregular_check_matrix(4, 4, 3, min_distance=d + 1, **kw)
    assert brute_force_distance(h2) >= d + 1 and not np.array_equal(h2, h)
    assert h2.shape == h.shape and set(h2.sum(0)) == {3} and set(h2.sum(1)) == {4}
    with pytest.raises(RuntimeError):
        codes.random_biregular_check_matrix(4, 4, 3, min_distance=17, **kw)


# ---------------------------------------------------------------------- bad shapes
def test_create_rejects_bad_shapes():
    L = _native.lib()
    vp = ctypes.c_void_p
    G = np.array([[3]], dtype="<u8")  # one row, columns 0 and 1
    h = vp()

    def create(dev, rows, n, k, g, p):
        return L.qldpc_dist_create(dev, rows, n, k, g.ctypes.data_as(vp) if g is not None else None,
                                   p.ctypes.data_as(vp) if p is not None else None, ctypes.byref(h))

    assert create(-1, 1, 2, 0, G, None) == 0
    L.qldpc_dist_destroy(h)
    for args in [(-1, 1, 0, 0, G, None), (-1, -1, 2, 0, G, None), (-1, 1, 2, -1, G, None), (-2, 1, 2, 0, G, None),
                 (-1, 1, 2, 0, None, None),   # no generator
                 (-1, 1, 2, 1, G, None),      # k > 0 without a pairing
                 (-1, 1, 2, 0, G, G),         # a pairing without k
                 (-1, 1, 1, 0, G, None),      # a bit past column n
                 (-1, 1, 2, 1, G, G)]:        # a pairing bit past k
        assert create(*args) == -1, args  # QLDPC_EINVAL
        assert b"qldpc_dist_create" in L.qldpc_last_error()
    assert L.qldpc_dist_create(-1, 1, 2, 0, G.ctypes.data_as(vp), None, None) == -1
    assert L.qldpc_dist_run_host(None, 0, 0, 1, None, None, None, None) == -1

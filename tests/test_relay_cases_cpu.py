"""The Relay-BP pinning inputs (tests/relay_cases.py) without a GPU: the host law
(``qldpc_relay_decode_host``, the checker of tests/test_gpu_relay_cases.py) equals the Python law
(tests/relay_ref.py) bit for bit on the irregular graphs and on the solution-choice set, the frozen sets
hold the decode classes they are there for, the geometry table's arithmetic hits its limits, and the
host side law is the plain host law on per-syndrome selected priors.
"""
import numpy as np
import pytest

import relay_cases as rc
import relay_ref
from qldpc_fault_tolerance_amd.engine import RelayParams, relay_decode_host, relay_decode_host_side

LAW_PER_PAIR = 6  # syndromes the Python law decodes per (setting, alpha) pair, consecutive slices of ``mixed``

_cache = {}


def _law(oracle, entry, precision):
    """The Python law with its trace on a solution-choice entry, once per (entry, precision)."""
    key = (entry, precision)
    if key not in _cache:
        _cache[key] = rc.law_traces(oracle, entry[0], entry[1], precision, rc.choice_syndromes(entry))
    return _cache[key]


def _equal(got, ref):
    assert np.array_equal(got[0], ref[0])
    assert np.array_equal(got[1], ref[1])
    assert np.array_equal(got[2], np.asarray(ref[2]).astype(bool))
    assert np.array_equal(got[3], ref[3])


# ------------------------------------------------------------------ host law == Python law
@pytest.mark.parametrize("precision", rc.PRECISIONS)
@pytest.mark.parametrize("kind", rc.PRIORS)
@pytest.mark.parametrize("case_id", rc.LAW_IDS)
def test_host_law_equals_the_python_law_on_irregular_graphs(oracle, case_id, kind, precision):
    H, probs = rc.graph(case_id), rc.priors(case_id, kind)
    S = rc.mixed(case_id, rc.B_IRREGULAR)
    for k, (setting, alpha) in enumerate(rc.PAIRS):
        synd = S[k * LAW_PER_PAIR:(k + 1) * LAW_PER_PAIR]
        t0, g0, legs, tr, stop = rc.SETTINGS[setting]
        got = relay_decode_host(H, probs, RelayParams(**rc.relay_kwargs(setting)), synd, ms_scaling_factor=alpha,
                                precision=precision, threads=2)
        with np.errstate(all="ignore"):  # (one_col in fp32: sums of sentinel-sized messages overflow, as in C)
            ref = relay_ref.decode_batch(oracle, H, probs, t0, g0, legs, tr, rc.GAMMA_LO, rc.GAMMA_HI, stop, rc.SEED,
                                         alpha, precision, synd)
        _equal(got, ref)
        assert (got[1] <= t0 + legs * tr).all() and (got[3] <= stop).all()


@pytest.mark.parametrize("precision", rc.PRECISIONS)
@pytest.mark.parametrize("entry", rc.CHOICE, ids=rc.CHOICE_IDS)
def test_host_law_equals_the_python_law_on_the_solution_choice_set(oracle, entry, precision):
    ref, _ = _law(oracle, entry, precision)
    got = relay_decode_host(rc.graph(entry[0]), rc.priors(entry[0], entry[1]),
                            RelayParams(**rc.relay_kwargs(rc.CHOICE_SETTING)), rc.choice_syndromes(entry),
                            ms_scaling_factor=rc.CHOICE_ALPHA, precision=precision)
    _equal(got, ref)


def test_the_trace_changes_no_result(oracle):
    entry = rc.CHOICE[0]
    H, probs = rc.graph(entry[0]), rc.priors(entry[0], entry[1])
    t0, g0, legs, tr, stop = rc.SETTINGS[rc.CHOICE_SETTING]
    plain = relay_ref.decode_batch(oracle, H, probs, t0, g0, legs, tr, rc.GAMMA_LO, rc.GAMMA_HI, stop, rc.SEED,
                                   rc.CHOICE_ALPHA, 64, rc.choice_syndromes(entry))
    traced, traces = _law(oracle, entry, 64)
    _equal([np.asarray(x) for x in traced], plain)
    assert [len(t) for t in traces] == plain[3].tolist()
    assert all(np.array_equal(np.array(rc.kept_of(t), np.uint8), c) for t, c in zip(traces, plain[0]) if t)


# ------------------------------------------------------------------ the frozen sets hold their classes
@pytest.mark.parametrize("precision", rc.PRECISIONS)
def test_solution_choice_set_holds_its_classes(oracle, precision):
    """At least CHOICE_NEEDED decodes of each class; a ``replaced`` and a ``heavier_kept`` under ``flipped``
    priors (negative weights); a ``tie_kept`` under priors that are not all equal.  (A ``tie_kept`` under
    ``half`` exists on none of the graphs: tests/relay_cases.py, above CHOICE.)"""
    count = {c: 0 for c in rc.CLASSES}
    by_kind = {}
    for entry in rc.CHOICE:
        _, traces = _law(oracle, entry, precision)
        for t in traces:
            cls = rc.solution_classes(t)
            assert cls, (entry[0], entry[1], "a decode of the set takes no decision among its solutions")
            for c in cls:
                count[c] += 1
                by_kind.setdefault((entry[1], c), 0)
                by_kind[(entry[1], c)] += 1
    print(precision, count, by_kind)
    assert all(count[c] >= rc.CHOICE_NEEDED for c in rc.CLASSES), count
    assert by_kind.get(("flipped", "replaced"), 0) >= 1 and by_kind.get(("flipped", "heavier_kept"), 0) >= 1
    assert by_kind.get(("nonuniform", "tie_kept"), 0) + by_kind.get(("flipped", "tie_kept"), 0) >= 1
    # the weights of the flipped decodes really are negative somewhere: a solution uses a p = 0.7 variable
    neg = 0
    for entry in rc.CHOICE:
        if entry[1] == "flipped":
            sp = rc.special_positions(rc.graph(entry[0]).n)
            neg += sum(1 for t in _law(oracle, entry, precision)[1] for _, _, dec in t if any(dec[j] for j in sp))
    assert neg >= 3
    # and the unsolved syndromes of the reuse batch have no solution
    case_id, kind, idx = rc.CHOICE_UNSOLVED
    res, _ = rc.law_traces(oracle, case_id, kind, precision, rc.choice_syndromes(rc.CHOICE_UNSOLVED))
    assert not res[2].any()


@pytest.mark.parametrize("precision", rc.PRECISIONS)
@pytest.mark.parametrize("case_id", rc.IRREGULAR_IDS)
def test_irregular_syndromes_hold_first_later_and_unsolved(case_id, precision):
    setting, alpha = rc.CLASS_PAIR
    total = {"first": 0, "later": 0, "unsolved": 0}
    for kind in rc.PRIORS:
        _, it, conv, nsol = relay_decode_host(rc.graph(case_id), rc.priors(case_id, kind),
                                              RelayParams(**rc.relay_kwargs(setting)),
                                              rc.mixed(case_id, rc.B_IRREGULAR), ms_scaling_factor=alpha,
                                              precision=precision)
        for k, v in rc.irregular_classes(it, conv, rc.SETTINGS[setting][0]).items():
            total[k] += v
    print(case_id, precision, total)
    absent = rc.ABSENT.get(case_id, {})
    for k, v in total.items():
        if k in absent:
            assert v == 0, (k, absent[k])
        else:
            assert v >= rc.IRREGULAR_NEEDED, (k, total)


def test_stop_settings_collect_their_solutions():
    """stop_nconv 2 and 8 are reached on the irregular graphs (chains that go on after a solution)."""
    for setting in ("s2", "s8"):
        stop = rc.SETTINGS[setting][4]
        for case_id in ("col1to12", "row33", "holes"):
            nsol = relay_decode_host(rc.graph(case_id), rc.priors(case_id, "flipped"),
                                     RelayParams(**rc.relay_kwargs(setting)), rc.mixed(case_id, rc.B_IRREGULAR))[3]
            assert nsol.max() == stop and nsol.min() == 0


def test_flipped_priors():
    for n in (1, 5, 52, 132):
        p, h, f = rc.priors_of(n, "nonuniform"), rc.priors_of(n, "half"), rc.priors_of(n, "flipped")
        sp = rc.special_positions(n)
        assert np.array_equal(np.flatnonzero(h == 0.5), sp) and np.array_equal(np.flatnonzero(f == rc.FLIPPED_P), sp)
        rest = np.setdiff1d(np.arange(n), sp)
        assert np.array_equal(f[rest], p[rest]) and np.array_equal(h[rest], p[rest])
        l0, wq = relay_ref.priors(f, 64)
        assert all(l0[j] < 0 and wq[j] < 0 for j in sp) and all(wq[j] > 0 for j in rest)


# ------------------------------------------------------------------ the geometry table
def test_geometry_table_arithmetic():
    G, L = rc.GEO, rc.LDS_MAX
    ex = {(g, p): G[g].expected(p) for g in rc.GEO_IDS for p in rc.PRECISIONS}
    # the limits, hit exactly, and the cases one step past them
    for at, over, p in (("image_at_limit", "image_over", 64), ("image32_at_limit", "image32_over", 32)):
        a, o = G[at], G[over]
        assert rc.relay_lds(p, a.m, a.n, a.E, True, False) == L and ex[(at, p)] == (True, False, 1024, L)
        assert (o.m, o.n, o.E) == (a.m + 1, a.n, a.E)
        assert rc.relay_lds(p, o.m, o.n, o.E, True, False) == L + 16 and ex[(over, p)][0] is False
    for at, over, p in (("state_at_limit", "state_over", 64), ("state32_at_limit", "state32_over", 32)):
        a, o = G[at], G[over]
        ts = p // 8
        assert (ts + 2) * a.n + 16 + a.m == L and ex[(at, p)] == (False, False, 1024, L)
        assert (o.m, o.n, o.E) == (a.m + 1, a.n, a.E) and ex[(over, p)] is None
    assert ex[("state32_over", 64)] is None and ex[("state32_at_limit", 64)] is None
    assert ex[("ws_idx32", 32)] == (False, True, 1024, L)  # the index copy beside the state fills LDS
    # the workspace without the switch, the index decision without the switch
    a = G["auto_ws"]
    assert rc.relay_lds(64, a.m, a.n, a.E, True, False) == 187216 and ex[("auto_ws", 64)][0] is False
    assert rc.relay_lds(32, a.m, a.n, a.E, True, False) == 97616 and ex[("auto_ws", 32)][0] is True
    assert ex[("auto_ws32", 32)][0] is False
    k, d = G["idx_kept"], G["idx_dropped"]
    assert ex[("idx_kept", 64)][:2] == (True, True) and ex[("idx_dropped", 64)][:2] == (True, False)
    assert rc.resident(rc.relay_lds(64, k.m, k.n, k.E, True, False)) == rc.resident(rc.relay_lds(64, k.m, k.n, k.E, True, True)) == 2
    assert rc.resident(rc.relay_lds(64, d.m, d.n, d.E, True, False)) == 2
    assert rc.resident(rc.relay_lds(64, d.m, d.n, d.E, True, True)) == 1 and rc.relay_lds(64, d.m, d.n, d.E, True, True) <= L
    b = G["big"]
    assert b.E > 0xffff and ex[("big", 64)][:3] == ex[("big", 32)][:3] == (False, False, 1024)
    # max(m, n) stops the doubling where the resident workgroups would allow another
    for g, p, tb in (("narrow256", 64, 256), ("narrow512", 64, 512)):
        e = ex[(g, p)]
        assert e[2] == tb and rc.resident(e[3]) * (2 * tb // 64) <= 32 and tb >= max(G[g].m, G[g].n)
    # all four (messages, index) combinations and all three widths, in each precision
    for p in rc.PRECISIONS:
        have = [e for (g, q), e in ex.items() if q == p and e is not None]
        assert {e[:2] for e in have} == {(True, True), (True, False), (False, True), (False, False)}
        assert {e[2] for e in have} == {256, 512, 1024}
        for e in have:  # 5 or more resident: 256 threads; 512 needs 4 or fewer, 1024 needs 2 or fewer
            r = rc.resident(e[3])
            assert e[3] <= L and (r < 5 or e[2] == 256) and (e[2] < 512 or r <= 4) and (e[2] < 1024 or r <= 2)
        wide = [rc.resident(e[3]) for e in have if e[2] == 1024]
        assert 1 in wide and 2 in wide and {rc.resident(e[3]) for e in have if e[2] == 512} & {3, 4}
    for g in rc.GEO_SIDE_IDS:
        assert all(ex[(g, p)] is not None for p in rc.PRECISIONS)
    assert ex[("image_at_limit", 64)][2] == ex[("image_at_limit", 32)][2] == 1024


@pytest.mark.parametrize("geo_id", rc.GEO_IDS)
def test_geometry_graphs(geo_id):
    g, csr = rc.GEO[geo_id], rc.geo_graph(geo_id)
    assert (csr.m, csr.n, csr.nnz) == (g.m, g.n, g.E)
    deg = np.concatenate([np.full(c, d) for d, c in g.degrees])
    assert np.array_equal(csr.col_degrees(), deg)
    assert all((np.diff(csr.col_idx[csr.row_ptr[i]:csr.row_ptr[i + 1]]) > 0).all() for i in range(0, g.m, max(1, g.m // 50)))
    S = rc.geo_syndromes(geo_id)
    assert S.shape == (rc.GEO_B, g.m) and not S[0].any() and S.any()


# ------------------------------------------------------------------ the host side law
@pytest.mark.parametrize("precision", rc.PRECISIONS)
def test_host_side_law_is_the_host_law_on_selected_priors(oracle, precision):
    relay = RelayParams(**rc.relay_kwargs(rc.CHOICE_SETTING))
    decided = 0
    for entry in rc.CHOICE:
        H, p0, p1, synd, side = rc.side_case(entry)
        assert (side & 1).any() and not (side & 1).all() and (side >> 1).any()
        got = relay_decode_host_side(H, p0, p1, relay, synd, side, ms_scaling_factor=rc.CHOICE_ALPHA, precision=precision)
        for b in range(len(synd)):
            sel = np.where(side[b] & 1, p1, p0)
            ref = relay_decode_host(H, sel, relay, synd[b:b + 1], ms_scaling_factor=rc.CHOICE_ALPHA, precision=precision)
            _equal([x[b:b + 1] for x in got], ref)
        decided += len(rc.side_weight_decides(oracle, entry, precision))
    # found under the Python law: 3 in fp64 and 3 in fp32 (row33 / uniform twice, hgp_34_n225 / flipped once)
    print(precision, "decodes whose kept solution row 0's weights alone would not keep:", decided)
    assert decided >= 3

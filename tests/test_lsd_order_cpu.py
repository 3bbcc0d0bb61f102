"""BP+LSD of higher order without a GPU: the host stage (qldpc_osd_create_lsd_order, plain C++ in
csrc/lsd.hip) against the Python restatement of the law (tests/lsd_order_ref.py) on the oracle's BP
posteriors and on a table cut from tests/lsd_cases.py, order 0 through the new create call against
qldpc_osd_create_lsd, the integer weights, the argument checks, and the quality conditions against the
oracle's OSD-E(10).
"""
import ctypes
import math

import numpy as np
import pytest

import lsd_order_cases as cases
import lsd_order_ref
from qldpc_fault_tolerance_amd import _native, codes, decoders
from qldpc_fault_tolerance_amd.engine import HostLSD, lsd_method_code
from qldpc_fault_tolerance_amd.simulators import gf2_rows

KS = cases.KS
SETTINGS = cases.SETTINGS


@pytest.fixture(scope="module")
def code():
    return codes.get_code("hgp_34_n225")


@pytest.fixture(scope="module")
def n225(oracle, code):
    """The 96 syndromes of tests/test_lsd_cpu.py: hz at p = 0.06 with the oracle's min-sum posteriors."""
    H = code.hz.astype(np.uint8)
    rng = np.random.default_rng(21)
    e = (rng.random((96, H.shape[1])) < 0.06).astype(np.uint8)
    synd = gf2_rows(code.csr("hz"), e)
    corr, _, conv, post = oracle.bp_decode_batch_soft(H, 0.06, 22, 0.625, synd)
    assert 8 <= (~conv).sum() and conv.sum() >= 1
    return H, synd, corr.astype(np.uint8), conv, post


_N225_LAW = {}


@pytest.mark.parametrize("threads", [1, 2])
@pytest.mark.parametrize("method,w", SETTINGS)
@pytest.mark.parametrize("k", KS)
def test_host_stage_equals_the_law(n225, k, method, w, threads):
    H, synd, corr, conv, post = n225
    lsd = HostLSD(H, k, 0.06, method, w)
    if (k, method, w) not in _N225_LAW:
        _N225_LAW[k, method, w] = lsd_order_ref.decode_batch(H, synd, post, k, method, w, lsd.weights())
    X0, XW, T, _ = _N225_LAW[k, method, w]
    o0, ow = lsd.decode_batch(synd, post, threads=threads)
    assert np.array_equal(o0, X0) and np.array_equal(ow, XW)
    x, st = lsd.decode_batch_stats(synd, post, threads=threads)
    assert np.array_equal(x, XW) and np.array_equal(st, T)
    assert (st[:, 0] == 1).all(), "hz has full row rank: no cluster is unsolvable"
    for out in (o0, ow):
        assert np.array_equal(gf2_rows(codes.CSR.from_dense(H), out), synd)
    for b in (0, 5):  # B = 1
        a0, aw = lsd.decode_batch(synd[b:b + 1], post[b:b + 1], threads=threads)
        assert np.array_equal(a0[0], X0[b]) and np.array_equal(aw[0], XW[b])
    # converged shots copy BP's correction into both outputs
    c0, cw = lsd.decode_batch(synd, post, conv, corr, threads=threads)
    assert np.array_equal(c0[conv], corr[conv]) and np.array_equal(cw[conv], corr[conv])
    assert np.array_equal(c0[~conv], X0[~conv]) and np.array_equal(cw[~conv], XW[~conv])


@pytest.mark.parametrize("kind", cases.PRIORS)
@pytest.mark.parametrize("case_id", cases.CASE_IDS + (cases.EXTRA,))
def test_host_stage_equals_the_law_on_the_table(case_id, kind):
    H = cases.graph(case_id)
    S, P = cases.inputs(case_id)
    pri = cases.priors(case_id, kind)
    for k in KS:
        for method, w in SETTINGS:
            lsd = HostLSD(H, k, pri, method, w)
            X0, XW, T, _ = cases.law(case_id, kind, k, method, w, lsd.weights())
            for threads in (1, 2):
                o0, ow = lsd.decode_batch(S, P, threads=threads)
                x, st = lsd.decode_batch_stats(S, P, threads=threads)
                assert np.array_equal(o0, X0) and np.array_equal(ow, XW), (k, method, w, threads)
                assert np.array_equal(x, XW) and np.array_equal(st, T), (k, method, w, threads)
            zero = ~S.any(1)
            assert (st[zero] == (1, 0, 0, 0)).all() and not ow[zero].any() and not o0[zero].any()


def test_every_event_kind_occurs():
    tot = dict.fromkeys(lsd_order_ref.EVENTS, 0)
    for case_id in cases.CASE_IDS + (cases.EXTRA,):
        for kind in cases.PRIORS:
            for k in KS:
                for method, w in SETTINGS:
                    wq = HostLSD(cases.graph(case_id), k, cases.priors(case_id, kind), method, w).weights()
                    ev = cases.law(case_id, kind, k, method, w, wq)[3]
                    for e in lsd_order_ref.EVENTS:
                        tot[e] += ev[e]
    print("events over the table:", tot)
    for e in lsd_order_ref.EVENTS:
        assert tot[e] >= 1, e


@pytest.mark.parametrize("method,w", cases.BIG_SETTINGS)
@pytest.mark.parametrize("kind", cases.PRIORS)
@pytest.mark.parametrize("case_id", cases.BIG_CASE_IDS)
def test_host_stage_equals_the_law_with_many_candidates(case_id, kind, method, w):
    """The orders at which a cluster has more candidates than the kernel has threads (the GPU file runs the
    same cases against the host stage): host stage = law, and the law meets such a cluster."""
    H = cases.graph(case_id)
    S, P = cases.inputs(case_id)
    lsd = HostLSD(H, 2, cases.priors(case_id, kind), method, w)
    X0, XW, T, ev = cases.law(case_id, kind, 2, method, w, lsd.weights())
    for threads in (1, 2):
        o0, ow = lsd.decode_batch(S, P, threads=threads)
        x, st = lsd.decode_batch_stats(S, P, threads=threads)
        assert np.array_equal(o0, X0) and np.array_equal(ow, XW) and np.array_equal(x, XW) and np.array_equal(st, T)
    if (method, w) != ("lsd_e", 8):
        assert ev["max_candidates"] > 256, ev
    else:
        assert ev["max_candidates"] == 255, ev
    if kind == "uniform":
        assert ev["tie_kept"] >= 1 and ev["replaced"] >= 1, ev


@pytest.mark.parametrize("k", [1, 3])
def test_order_0_through_the_new_call_equals_create_lsd(n225, k):
    H, synd, corr, conv, post = n225
    want = HostLSD(H, k).decode_batch_stats(synd, post, conv, corr)
    for method, w, probs in (("lsd_0", 0, None), ("lsd_0", 7, 0.06), ("lsd_e", 0, 0.06), ("lsd_cs", 0, None)):
        lsd = HostLSD(H, k, probs, method, w)
        got = lsd.decode_batch_stats(synd, post, conv, corr)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        o0, ow = lsd.decode_batch(synd, post, conv, corr)
        assert np.array_equal(o0, want[0]) and np.array_equal(ow, want[0])
        lsd.set_side_probs(0.01, 0.3)  # order-0 handles keep their side decode
        a = lsd.decode_batch(synd, post, conv, corr, side=np.ones((96, H.shape[1]), np.uint8))
        assert np.array_equal(a[1], want[0])


def test_weights(n225):
    H = n225[0]
    n = H.shape[1]
    p = np.random.default_rng(9).uniform(1e-6, 0.999, n)
    p[::3] = 0.0123
    p[1], p[2] = 1e-300, 1.0 - 2.0 ** -53
    wq = HostLSD(H, 1, p, "lsd_e", 2).weights()
    assert wq.dtype == np.int64
    for j in range(n):
        assert abs(int(wq[j]) - math.floor(math.log(1 / p[j]) * 2 ** 32 + 0.5)) <= 1, j
    assert (wq[::3] == wq[0]).all(), "equal priors have equal weights"
    assert (HostLSD(H, 1, 0.05, "lsd_0", 0).weights() == math.floor(math.log(1 / 0.05) * 2 ** 32 + 0.5)).all()
    with pytest.raises(_native.QldpcError):
        HostLSD(H, 1).weights()  # created without priors


def test_argument_checks(n225, code):
    H = n225[0]
    n = H.shape[1]
    for kw in (dict(lsd_method="lsd_e", lsd_order=13), dict(lsd_method="lsd_cs", lsd_order=65),
               dict(lsd_method="lsd_e", lsd_order=-1), dict(lsd_method="lsd_0", lsd_order=-1),
               dict(lsd_method=3, lsd_order=1), dict(lsd_method=-1, lsd_order=0)):
        with pytest.raises(_native.QldpcError) as e:
            HostLSD(H, 1, 0.05, **kw)
        assert e.value.rc == _native.EINVAL, kw
    HostLSD(H, 1, 0.05, "lsd_e", 12)
    HostLSD(H, 1, 0.05, "lsd_cs", 64)
    for bad in (0.0, 1.0):
        p = np.full(n, 0.05)
        p[n // 2] = bad
        with pytest.raises(_native.QldpcError) as e:
            HostLSD(H, 1, p, "lsd_e", 1)
        assert e.value.rc == _native.EINVAL
        HostLSD(H, 1, p, "lsd_e", 0)  # no order in force: the priors are not read
    with pytest.raises(_native.QldpcError) as e:
        HostLSD(H, 1, None, "lsd_cs", 2)  # an order above 0 needs priors
    assert e.value.rc == _native.EINVAL
    with pytest.raises(ValueError):
        HostLSD(H, 1, np.full(n - 1, 0.05), "lsd_e", 2)  # a prior vector of the wrong length never reaches C
    with pytest.raises(ValueError):
        lsd_method_code("lsd_x")
    assert [lsd_method_code(v) for v in ("lsd_0", "LSD_E", "lsd_cs", 2)] == [0, 1, 2, 2]
    c = codes.CSR.from_dense(H)
    rp, ci = np.ascontiguousarray(c.row_ptr, np.int32), np.ascontiguousarray(c.col_idx, np.int32)
    pr = np.full(n, 0.05)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    h = ctypes.c_void_p()
    f = _native.lib().qldpc_osd_create_lsd_order
    assert f(c.m, c.n, None, vp(ci), vp(pr), 1, 1, 2, ctypes.byref(h)) == _native.EINVAL
    assert f(c.m, c.n, vp(rp), vp(ci), vp(pr), 0, 1, 2, ctypes.byref(h)) == _native.EINVAL
    assert f(c.m, c.n, vp(rp), vp(ci), vp(pr), 1, 1, 2, None) == _native.EINVAL
    lsd = HostLSD(H, 1, 0.05, "lsd_e", 4)
    assert _native.lib().qldpc_lsd_weights(lsd.handle, None) == _native.EINVAL
    with pytest.raises(_native.QldpcError) as e:
        lsd.set_side_probs(0.01, 0.3)
    assert e.value.rc == _native.ENOTSUP
    with pytest.raises(ValueError):
        decoders.BPLSD_Decoder(code.hz, 0.05 * np.ones(n), 22, "minimum_sum", 0.625, bits_per_step=1,
                               lsd_method="lsd_e", lsd_order=2, side_probs=(0.01, 0.3), use_gpu_osd=False)


def test_quality_against_the_oracle_osd_e10(oracle, code):
    """hgp_34_n225, p = 0.03, max_iter 22, the 3000 shots of default_rng(11) (the draws of
    tests/test_lsd_cpu.py's quality test): among the non-converged decodes the host stage at k = 1 fails at
    most as often as the oracle's BP+OSD-E(10), with lsd_e 4 and with lsd_cs 8 (the Python law gives 269 and
    266 against 300), and out_osd0 always solves the syndrome."""
    H = code.hz.astype(np.uint8)
    n, p = H.shape[1], 0.03
    rng = np.random.default_rng(11)
    e = (rng.random((3000, n)) < p).astype(np.uint8)
    synd = gf2_rows(code.csr("hz"), e)
    corr, _, conv, post = oracle.bp_decode_batch_soft(H, p, 22, 0.625, synd)
    nc = np.flatnonzero(~conv)
    osde = oracle.osd_decode_batch(H, p * np.ones(n), synd[nc], post[nc], "osd_e", 10)[1]

    def failures(x):
        r = (e[nc] ^ x).astype(np.uint8)
        return int((gf2_rows(code.csr("hz"), r).any(1) | gf2_rows(code.csr("lz"), r).any(1)).sum())

    fe = failures(osde)
    out = {}
    for method, w in (("lsd_e", 4), ("lsd_cs", 8)):
        lsd = HostLSD(H, 1, p, method, w)
        o0, ow = lsd.decode_batch(synd[nc], post[nc])
        st = lsd.decode_batch_stats(synd[nc], post[nc])[1]
        assert (st[:, 0] == 1).all()
        assert np.array_equal(gf2_rows(code.csr("hz"), o0), synd[nc]), "out_osd0 solves the syndrome"
        assert np.array_equal(gf2_rows(code.csr("hz"), ow), synd[nc])
        out[method, w] = (failures(ow), failures(o0), st[:, 1].mean(), st[:, 2].mean())
    print(f"non-converged {nc.size}, OSD-E(10) failures {fe}; (method, w): (failures, failures of out_osd0, "
          f"mean rounds, mean |A|) = {out}")
    assert out["lsd_e", 4][0] <= fe
    assert out["lsd_cs", 8][0] <= fe

"""Serial-schedule min-sum BP without a GPU: the layer rule (qldpc_serial_layers) and the host law
(qldpc_serial_decode_host, plain C++) against the Python restatement of the law (tests/serial_ref.py),
the anchor to the oracle's flooding BP where the two schedules coincide, the effect of the schedule
on hgp_34_n225, and the argument checks.
"""
import ctypes
import os

import numpy as np
import pytest

import bp_cases
import serial_cases
import serial_ref
from qldpc_fault_tolerance_amd import _native, codes
from qldpc_fault_tolerance_amd.codes import CSR
from qldpc_fault_tolerance_amd.engine import serial_decode_host, serial_layers


@pytest.fixture(scope="module")
def hz():
    return codes.get_code("hgp_34_n225").csr("hz")


def _graphs(hz):
    out = {"n225_hz": hz, "ring5": serial_cases.ring5(), "irregular": serial_cases.irregular(),
           "chain257": serial_cases.chain(257)}
    for cid in ("col1to12", "holes", "one_col", "row33"):
        out["bp_cases_" + cid] = CSR.from_dense(bp_cases.graph(cid))
    return out


def test_layers_are_independent_and_first_fit(hz):
    for name, H in _graphs(hz).items():
        layer, num = serial_layers(H)
        assert layer.shape == (H.n,) and num == int(layer.max()) + 1, name
        assert np.array_equal(layer, serial_ref.layers(H)), name  # the definition, variable by variable
        D = H.to_dense().astype(np.int64)
        share = (D.T @ D) > 0
        np.fill_diagonal(share, False)
        same = layer[:, None] == layer[None, :]
        assert not (share & same).any(), name  # no two variables of a layer share a check
    assert serial_layers(hz)[1] >= 2


def test_layers_of_a_graph_without_shared_checks():
    layer, num = serial_layers(serial_cases.identity(8))
    assert num == 1 and (layer == 0).all()
    layer, num = serial_layers(serial_cases.chain(257))
    assert num == 2 and np.array_equal(layer, np.arange(257) % 2)


def _law_cases(hz):
    """name -> (graph, priors, max_iter, syndromes)."""
    rng = np.random.default_rng(7)
    irr = serial_cases.irregular()
    ring = serial_cases.ring5()
    out = {
        "n225": (hz, 0.05, 10, serial_cases.syndromes(hz, 0.05, 20, rng)),
        "ring5": (ring, 0.1, 6, np.array([[(v >> i) & 1 for i in range(5)] for v in range(0, 32, 2)], np.uint8)),
        "irregular": (irr, 0.06, 12, serial_cases.syndromes(irr, 0.08, 20, rng)),
        "irregular_nonuniform": (irr, serial_cases.irregular_priors(irr.n), 12,
                                 serial_cases.syndromes(irr, 0.08, 20, rng)),
    }
    # an unsatisfiable bit on the degree-1 row's neighbourhood: decodes that reach max_iter
    out["irregular"][3][1, :] ^= 1
    return out


@pytest.fixture(scope="module")
def law_cases(hz):
    return _law_cases(hz)


@pytest.fixture(scope="module")
def law_reference(law_cases):
    """The Python law, computed once per (case, precision, alpha)."""
    cache = {}

    def get(name, precision, alpha):
        key = (name, precision, alpha)
        if key not in cache:
            H, probs, max_iter, synd = law_cases[name]
            cache[key] = serial_ref.decode_batch(H, probs, max_iter, alpha, precision, synd)
        return cache[key]

    return get


@pytest.mark.parametrize("alpha", [0.625, 0.0])
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", ["n225", "ring5", "irregular", "irregular_nonuniform"])
def test_host_decode_equals_the_law(law_cases, law_reference, name, precision, alpha):
    H, probs, max_iter, synd = law_cases[name]
    ref = law_reference(name, precision, alpha)
    got = serial_decode_host(H, probs, max_iter, synd, ms_scaling_factor=alpha, precision=precision, threads=2)
    print(name, precision, alpha, "iters", ref[1].tolist(), "conv", ref[2].tolist())
    assert np.array_equal(got[0], ref[0])
    assert np.array_equal(got[1], ref[1])
    assert np.array_equal(got[2], ref[2].astype(bool))
    assert np.array_equal(got[3], ref[3])  # posteriors, bit for bit
    if precision == 32:
        assert np.array_equal(got[3], got[3].astype(np.float32).astype(np.float64))
    assert (got[1] >= 1).all() and (got[1] <= max_iter).all()
    assert np.array_equal(got[2] | (got[1] == max_iter), np.ones(len(synd), bool))
    ok = (H.matvec(got[0].astype(np.uint8)) == synd).all(axis=1)
    assert np.array_equal(ok, got[2])
    assert np.array_equal(got[0], (got[3] <= 0).astype(np.int64))


def test_law_cases_hold_both_outcomes(law_cases, law_reference):
    """The n225 syndromes are a mix of converged and non-converged decodes, zero syndrome included."""
    _, _, _, synd = law_cases["n225"]
    assert not synd[0].any()
    conv = law_reference("n225", 64, 0.625)[2]
    assert conv[0] == 1 and 0 < conv.sum() < len(conv)


def test_the_order_matters(law_cases, law_reference):
    """The natural order is another decoder: the law's order pi is part of the contract."""
    H, probs, max_iter, synd = law_cases["n225"]
    ref = law_reference("n225", 64, 0.625)
    nat = serial_ref.decode_batch(H, probs, max_iter, 0.625, 64, synd[:6], pi=range(H.n))
    assert not np.array_equal(nat[3], ref[3][:6])


@pytest.mark.parametrize("alpha", [0.625, 0.0])
@pytest.mark.parametrize("precision", [64, 32])
def test_identity_graph_equals_the_oracle(oracle, precision, alpha):
    """One layer, no shared check: a serial sweep is a flooding iteration, so iteration counting and
    the convergence test are the oracle's."""
    H = serial_cases.identity(8)
    probs = np.linspace(0.05, 0.6, 8)  # priors above 1/2: negative LLRs
    synd = np.array([[(v >> i) & 1 for i in range(8)] for v in range(0, 256, 5)], np.uint8)
    for max_iter in (1, 4):
        got = serial_decode_host(H, probs, max_iter, synd, ms_scaling_factor=alpha, precision=precision)
        ref = oracle.bp_decode_batch(H, probs, max_iter, "minimum_sum", alpha, synd, precision)
        assert np.array_equal(got[0], ref[0])
        assert np.array_equal(got[1], ref[1])
        assert np.array_equal(got[2], ref[2].astype(bool))


@pytest.mark.parametrize("precision", [64, 32])
def test_host_decode_equals_the_recorded_law(hz, precision):
    """tests/golden/serial_n225.npz (tests/golden/make_golden_serial.py)."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "serial_n225.npz"))
    got = serial_decode_host(hz, float(g["p_prior"]), int(g["max_iter"]), g["synd"],
                             ms_scaling_factor=float(g["alpha"]), precision=precision)
    assert np.array_equal(got[0], g[f"corr{precision}"])
    assert np.array_equal(got[1], g[f"iters{precision}"])
    assert np.array_equal(got[2], g[f"conv{precision}"].astype(bool))
    assert np.array_equal(got[3], g[f"post{precision}"])


def test_serial_leaves_fewer_non_converged_decodes(oracle, hz):
    """2000 syndromes of hgp_34_n225 hz at p = 0.02: at the same cap the serial schedule leaves
    strictly fewer non-converged decodes than flooding, and at half the cap no more."""
    rng = np.random.default_rng(20260101)
    synd = serial_cases.syndromes(hz, 0.02, 2000, rng, zero=False)
    flood = oracle.bp_decode_batch(hz, 0.02, 22, "minimum_sum", 0.625, synd, 64)
    full = serial_decode_host(hz, 0.02, 22, synd)
    half = serial_decode_host(hz, 0.02, 11, synd)
    nf, ns, nh = int((flood[2] == 0).sum()), int((~full[2]).sum()), int((~half[2]).sum())
    print("non-converged of 2000: flooding(22)", nf, "serial(22)", ns, "serial(11)", nh,
          "mean iterations", float(flood[1].mean()), float(full[1].mean()), float(half[1].mean()))
    assert ns < nf
    assert nh <= nf


def test_argument_errors(hz):
    L = _native.lib()
    rp = np.ascontiguousarray(hz.row_ptr, dtype=np.int32)
    ci = np.ascontiguousarray(hz.col_idx, dtype=np.int32)
    probs = np.full(hz.n, 0.05)
    synd = np.zeros((1, hz.m), np.uint8)
    corr = np.zeros((1, hz.n), np.uint8)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def host(max_iter, precision):
        return L.qldpc_serial_decode_host(hz.m, hz.n, vp(rp), vp(ci), vp(probs), max_iter, 0.625, precision, vp(synd),
                                          vp(corr), None, None, None, 1, 1)

    assert host(5, 64) == 0  # iters, conv and post may each be NULL
    assert host(0, 64) == _native.EINVAL
    assert host(-3, 32) == _native.EINVAL
    assert host(5, 16) == _native.EINVAL
    with pytest.raises(_native.QldpcError) as e:
        serial_decode_host(hz, 0.05, 0, synd)
    assert e.value.rc == _native.EINVAL
    bad = ci.copy()
    bad[0] = hz.n
    assert L.qldpc_serial_layers(hz.m, hz.n, vp(rp), vp(bad), vp(np.zeros(hz.n, np.int32)), None) == _native.EINVAL


def test_schedule_argument_errors(hz):
    """Raised before any device call: product-sum, relay legs and unknown names have no serial schedule."""
    from qldpc_fault_tolerance_amd.decoders import BPDecoder
    from qldpc_fault_tolerance_amd.engine import DeviceBP, RelayParams

    with pytest.raises(ValueError):
        DeviceBP(hz, 0.05, max_iter=5, bp_method="product_sum", schedule="serial")
    with pytest.raises(ValueError):
        DeviceBP(hz, 0.05, max_iter=5, schedule="serial", relay=RelayParams(pre_iter=5))
    with pytest.raises(ValueError):
        DeviceBP(hz, 0.05, max_iter=5, schedule="layered")
    with pytest.raises(ValueError):
        BPDecoder(hz, 0.05 * np.ones(hz.n), 5, "product_sum", 0.625, schedule="serial")

"""Side-prior decoding without a GPU: the host side laws (qldpc_relay_decode_host_side,
qldpc_serial_decode_host_side, plain C++) against the Python restatement (tests/side_ref.py), the
anchors to the plain host laws and to the oracle's min-sum BP, the quality condition of X/Z-correlated
decoding, channel_update_probs, and the argument checks.
"""
import os

import numpy as np
import pytest

import side_ref
from qldpc_fault_tolerance_amd import codes, decoders, simulators
from qldpc_fault_tolerance_amd._native import QldpcError
from qldpc_fault_tolerance_amd.engine import (RelayParams, relay_decode_host, relay_decode_host_side,
                                              serial_decode_host, serial_decode_host_side)

SEED = 0x9E3779B97F4A7C15
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "side_n225.npz")


@pytest.fixture(scope="module")
def code():
    return codes.get_code("hgp_34_n225")


@pytest.fixture(scope="module")
def hz(code):
    return code.csr("hz")


def _syndromes(H, p, count, rng):
    e = (rng.random((count, H.n)) < p).astype(np.uint8)
    return e, H.matvec(e).astype(np.uint8)


@pytest.fixture(scope="module")
def law_syndromes(hz):
    rng = np.random.default_rng(5)
    parts = [_syndromes(hz, p, 3, rng)[1] for p in (0.01, 0.03, 0.05, 0.08)]
    return np.concatenate(parts)  # 12 syndromes, easy to hopeless (as test_relay_cpu.py draws them)


@pytest.fixture(scope="module")
def tables(hz):
    return side_ref.nonuniform_tables(hz.n)


def _law_side(hz, density):
    """12 rows of side bytes at ``density`` with noise in the high bits, plus the two named bytes."""
    rng = np.random.default_rng(int(density * 100) + 1)
    side = side_ref.side_bytes(rng, 12, hz.n, density)
    if 0 < density < 1:
        side[0, :8] = 0xFE  # counts as 0
        side[1, :8] = 0x03  # counts as 1
    return side


# ------------------------------------------------------------------ quality (run first)
def _quality(code, direction, shots=2000):
    """Failures and non-converged second-sector decodes of independent and of `direction` decoding of
    the same errors, host law only: flooding min-sum(22), alpha 0.625, fp64, px = py = pz = 0.04 / 3."""
    p = 0.04
    probs = (p / 3, p / 3, p / 3)
    rng = np.random.default_rng(1)
    ex, ez = simulators.pauli_split(rng.random((shots, code.N)), probs)
    err = (ex | (ez << 1)).astype(np.uint8)
    r = RelayParams(pre_iter=22, **side_ref.PLAIN)
    p_first, p0, p1 = decoders.channel_update_probs(*probs, direction)

    def first(H, synd):
        return relay_decode_host(H, p_first, r, synd)[:3]

    def second(H, synd, side):
        return relay_decode_host_side(H, p0, p1, r, synd, side)[:3]

    def independent(H, synd, side):
        return relay_decode_host(H, p_first, r, synd)[:3]

    q2 = 1 if direction == "x->z" else 0  # the second sector's column
    upd = side_ref.compose(code, err, direction, first, second)
    ind = side_ref.compose(code, err, direction, first, independent)
    out = {}
    for name, res in (("independent", ind), ("update", upd)):
        out[name] = (int((res["fail"][:, 0] | res["fail"][:, 1]).sum()), int((~res["conv"][:, q2]).sum()))
    return out


@pytest.mark.parametrize("direction", ["x->z", "z->x"])
def test_channel_update_cuts_failures_by_a_tenth(code, direction):
    """hgp_34_n225, px = py = pz = 0.04 / 3, 2,000 errors from default_rng(1): the update leaves at most
    0.9 x the failures of independent decoding and strictly fewer non-converged second-sector decodes."""
    q = _quality(code, direction)
    (f_ind, nc_ind), (f_upd, nc_upd) = q["independent"], q["update"]
    print(f"{direction}: failures {f_ind} -> {f_upd} ({f_upd / max(1, f_ind):.3f}), "
          f"non-converged second sector {nc_ind} -> {nc_upd}")
    assert f_ind > 0
    assert f_upd <= 0.9 * f_ind
    assert nc_upd < nc_ind


# ------------------------------------------------------------------ host law == restatement
SETTINGS = {
    "plain": (8, 0.0, 0, 0, 1),
    "memory": (8, 0.125, 0, 0, 1),
    "relay_s3": (6, 0.125, 3, 6, 3),
}


@pytest.mark.parametrize("alpha", [0.625, 0.0])
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("density", [0.0, 0.03, 0.5, 1.0])
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_relay_host_side_equals_the_law(oracle, hz, law_syndromes, tables, setting, density, precision, alpha):
    t0, g0, legs, tr, stop = SETTINGS[setting]
    p0, p1 = tables
    side = _law_side(hz, density)
    r = RelayParams(pre_iter=t0, pre_gamma=g0, num_legs=legs, leg_iter=tr, gamma_lo=-0.24, gamma_hi=0.66,
                    stop_nconv=stop, gamma_seed=SEED)
    got = relay_decode_host_side(hz, p0, p1, r, law_syndromes, side, ms_scaling_factor=alpha, precision=precision,
                                 threads=2)
    ref = side_ref.relay_decode_batch(oracle, hz, p0, p1, side, t0, g0, legs, tr, -0.24, 0.66, stop, SEED, alpha,
                                      precision, law_syndromes)
    assert np.array_equal(got[0], ref[0])
    assert np.array_equal(got[1], ref[1])
    assert np.array_equal(got[2], ref[2].astype(bool))
    assert np.array_equal(got[3], ref[3])


@pytest.mark.parametrize("alpha", [0.625, 0.0])
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("density", [0.0, 0.03, 0.5, 1.0])
def test_serial_host_side_equals_the_law(hz, law_syndromes, tables, density, precision, alpha):
    p0, p1 = tables
    side = _law_side(hz, density)
    got = serial_decode_host_side(hz, p0, p1, 8, law_syndromes, side, ms_scaling_factor=alpha, precision=precision,
                                  threads=2)
    ref = side_ref.serial_decode_batch(hz, p0, p1, side, 8, alpha, precision, law_syndromes)
    assert np.array_equal(got[0], ref[0])
    assert np.array_equal(got[1], ref[1])
    assert np.array_equal(got[2], ref[2].astype(bool))


def test_the_side_bytes_change_the_decode(hz, law_syndromes, tables):
    """The law cases are not vacuous: the densities give different corrections, on both engines."""
    p0, p1 = tables
    r = RelayParams(pre_iter=8, **side_ref.PLAIN)
    a = relay_decode_host_side(hz, p0, p1, r, law_syndromes, _law_side(hz, 0.0))
    b = relay_decode_host_side(hz, p0, p1, r, law_syndromes, _law_side(hz, 0.5))
    assert not np.array_equal(a[0], b[0])
    a = serial_decode_host_side(hz, p0, p1, 8, law_syndromes, _law_side(hz, 0.0))
    b = serial_decode_host_side(hz, p0, p1, 8, law_syndromes, _law_side(hz, 0.5))
    assert not np.array_equal(a[0], b[0])


# ------------------------------------------------------------------ anchors
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_relay_anchors(hz, law_syndromes, tables, setting, precision):
    t0, g0, legs, tr, stop = SETTINGS[setting]
    p0, p1 = tables
    r = RelayParams(pre_iter=t0, pre_gamma=g0, num_legs=legs, leg_iter=tr, stop_nconv=stop, gamma_seed=SEED)
    B = len(law_syndromes)
    zeros = np.full((B, hz.n), 0xFE, np.uint8)  # bit 0 clear
    ones = np.full((B, hz.n), 0x03, np.uint8)
    for side, p in ((zeros, p0), (ones, p1)):
        got = relay_decode_host_side(hz, p0, p1, r, law_syndromes, side, precision=precision)
        ref = relay_decode_host(hz, p, r, law_syndromes, precision=precision)
        assert all(np.array_equal(x, y) for x, y in zip(got, ref))


@pytest.mark.parametrize("precision", [64, 32])
def test_serial_anchors(hz, law_syndromes, tables, precision):
    p0, p1 = tables
    B = len(law_syndromes)
    for side, p in ((np.zeros((B, hz.n), np.uint8), p0), (np.ones((B, hz.n), np.uint8), p1)):
        got = serial_decode_host_side(hz, p0, p1, 8, law_syndromes, side, precision=precision)
        ref = serial_decode_host(hz, p, 8, law_syndromes, precision=precision)[:3]
        assert all(np.array_equal(x, y) for x, y in zip(got, ref))


@pytest.mark.parametrize("alpha", [0.625, 0.0])
@pytest.mark.parametrize("precision", [64, 32])
def test_no_legs_no_memory_is_the_oracles_min_sum_per_syndrome(oracle, hz, law_syndromes, tables, precision, alpha):
    """Engine 7 with zero legs and zero memory under side priors = the oracle's bp_decode_batch run
    syndrome by syndrome with that syndrome's prior vector."""
    p0, p1 = tables
    side = _law_side(hz, 0.5)
    r = RelayParams(pre_iter=22, **side_ref.PLAIN)
    corr, it, conv, nsol = relay_decode_host_side(hz, p0, p1, r, law_syndromes, side, ms_scaling_factor=alpha,
                                                  precision=precision)
    for b, s in enumerate(law_syndromes):
        probs = np.where(side[b] & 1, p1, p0)
        oc, oi, ov = oracle.bp_decode_batch(hz, probs, 22, "minimum_sum", alpha, synd=s[None], precision=precision)
        assert np.array_equal(corr[b], oc[0]) and it[b] == oi[0] and conv[b] == ov[0] and nsol[b] == int(ov[0])
    assert conv.any() and (~conv).any()


# ------------------------------------------------------------------ further checks
def test_channel_update_probs_equals_the_formulas():
    px, py, pz = 0.01, 0.002, 0.03
    assert decoders.channel_update_probs(px, py, pz, "x->z") == (px + py, pz / (1 - px - py), py / (px + py))
    assert decoders.channel_update_probs(px, py, pz, "z->x") == (pz + py, px / (1 - pz - py), py / (pz + py))
    with pytest.raises(ValueError, match="p1"):
        decoders.channel_update_probs(0.01, 0.0, 0.01, "x->z")
    with pytest.raises(ValueError, match="p1"):
        decoders.channel_update_probs(0.01, 0.0, 0.01, "z->x")
    with pytest.raises(ValueError, match="p0"):
        decoders.channel_update_probs(0.01, 0.01, 0.0, "x->z")
    with pytest.raises(ValueError):
        decoders.channel_update_probs(0.01, 0.01, 0.01, "y->x")


def test_host_side_law_is_independent_of_the_thread_count(hz, law_syndromes, tables):
    p0, p1 = tables
    side = _law_side(hz, 0.5)
    r = RelayParams(pre_iter=6, num_legs=3, leg_iter=6, stop_nconv=2, gamma_seed=3)
    a = relay_decode_host_side(hz, p0, p1, r, law_syndromes, side, threads=1)
    b = relay_decode_host_side(hz, p0, p1, r, law_syndromes, side, threads=5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    a = serial_decode_host_side(hz, p0, p1, 8, law_syndromes, side, threads=1)
    b = serial_decode_host_side(hz, p0, p1, 8, law_syndromes, side, threads=5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("precision", [64, 32])
def test_host_side_law_equals_the_recorded_law(hz, precision):
    """tests/golden/side_n225.npz (tests/golden/make_golden_side.py): what the GPU test pins the kernels to."""
    g = np.load(GOLDEN)
    r = RelayParams(pre_iter=int(g["pre_iter"]), pre_gamma=float(g["pre_gamma"]), num_legs=int(g["num_legs"]),
                    leg_iter=int(g["leg_iter"]), gamma_lo=float(g["gamma_lo"]), gamma_hi=float(g["gamma_hi"]),
                    stop_nconv=int(g["stop_nconv"]), gamma_seed=int(g["gamma_seed"]))
    corr, it, conv, nsol = relay_decode_host_side(hz, g["p0"], g["p1"], r, g["synd"], g["side"],
                                                  ms_scaling_factor=float(g["alpha"]), precision=precision)
    assert np.array_equal(corr, g[f"relay_corr{precision}"]) and np.array_equal(it, g[f"relay_iters{precision}"])
    assert np.array_equal(conv, g[f"relay_conv{precision}"].astype(bool))
    assert np.array_equal(nsol, g[f"relay_nsol{precision}"])
    corr, it, conv = serial_decode_host_side(hz, g["p0"], g["p1"], int(g["serial_iter"]), g["synd"], g["side"],
                                             ms_scaling_factor=float(g["alpha"]), precision=precision)
    assert np.array_equal(corr, g[f"serial_corr{precision}"]) and np.array_equal(it, g[f"serial_iters{precision}"])
    assert np.array_equal(conv, g[f"serial_conv{precision}"].astype(bool))
    assert conv.any() and (~conv).any()


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")])
@pytest.mark.parametrize("which", [0, 1])
def test_a_side_prior_outside_the_open_interval_is_einval(hz, bad, which):
    p = [np.full(hz.n, 0.03), np.full(hz.n, 0.2)]
    p[which][hz.n // 2] = bad
    synd = np.zeros((1, hz.m), np.uint8)
    side = np.zeros((1, hz.n), np.uint8)
    for call in (lambda: relay_decode_host_side(hz, p[0], p[1], RelayParams(pre_iter=4), synd, side),
                 lambda: serial_decode_host_side(hz, p[0], p[1], 4, synd, side)):
        with pytest.raises(QldpcError) as ei:
            call()
        assert ei.value.rc == -1  # QLDPC_EINVAL


def test_bad_engine_parameters_are_einval(hz):
    synd = np.zeros((1, hz.m), np.uint8)
    side = np.zeros((1, hz.n), np.uint8)
    for call in (lambda: relay_decode_host_side(hz, 0.03, 0.2, RelayParams(pre_iter=0), synd, side),
                 lambda: relay_decode_host_side(hz, 0.03, 0.2, RelayParams(pre_iter=4), synd, side, precision=16),
                 lambda: serial_decode_host_side(hz, 0.03, 0.2, 0, synd, side)):
        with pytest.raises(QldpcError) as ei:
            call()
        assert ei.value.rc == -1
    with pytest.raises(ValueError):  # side bytes of the wrong shape never reach the library
        relay_decode_host_side(hz, 0.03, 0.2, RelayParams(pre_iter=4), synd, side[:, :-1])


def test_the_side_entry_points_are_exported():
    from qldpc_fault_tolerance_amd import _native

    for name in ("qldpc_bp_set_side_probs", "qldpc_bp_decode_batch_side", "qldpc_relay_decode_host_side",
                 "qldpc_serial_decode_host_side", "qldpc_mc_set_channel_update"):
        assert name in _native.EXPORTED and hasattr(_native.lib(), name)
    assert _native.lib().qldpc_abi_version() == 1


def test_simulator_and_decoder_refusals_without_a_gpu(code):
    with pytest.raises(ValueError):
        simulators.CodeSimulator_DataError(code=code, channel_update="x<-z")
    with pytest.raises(ValueError):
        simulators.CodeFamily([code], None, None).EvalWER("phenl", "Total", [0.01], 10, channel_update="x->z")

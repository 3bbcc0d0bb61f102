"""OSD under per-shot priors without a GPU: the host stage's side decode (qldpc_osd_decode_batch_side)
against the per-syndrome oracle (tests/side_osd_ref.py), its two anchors to the plain decode, the
condition that the side bytes change decodes, the quality of BP+OSD channel-update decoding judged by
the oracle alone, and the argument checks.
"""
import ctypes

import numpy as np
import pytest

import osd_cases as oc
import side_osd_ref
import side_ref
from qldpc_fault_tolerance_amd import _native, codes, decoders, simulators
from qldpc_fault_tolerance_amd._native import EINVAL, QldpcError
from qldpc_fault_tolerance_amd.engine import HostOSD

B = 8
CASES = ["rr2_tail", "rr8_pad", "small_k", "rank0", "k0"]
DENSITIES = [0.0, 0.03, 0.5, 1.0]
TABLES = ["uniform", "nonuniform"]


def tables(case_id, kind):
    """(p0, p1) of a case: ``uniform`` = priors(uniform) with p1 = 0.4 everywhere; ``nonuniform`` =
    priors(nonuniform) with a salted non-uniform p1."""
    n = oc.CASES[case_id].n
    if kind == "uniform":
        return oc.priors(case_id, "uniform"), np.full(n, 0.4)
    p1 = np.random.default_rng([oc.CASES[case_id].seed, 9]).uniform(0.05, 0.45, n)
    p1[::5] = p1[2]
    return oc.priors(case_id, "nonuniform"), p1


def side_bytes(case_id, density, nb=B, seed=5):
    """Side bytes [nb, n] at ``density`` with random high bits (only bit 0 counts)."""
    rng = np.random.default_rng([seed, int(density * 100), oc.CASES[case_id].seed])
    return side_ref.side_bytes(rng, nb, oc.CASES[case_id].n, density)


def inputs(case_id, kind):
    c = oc.CASES[case_id]
    if kind == "consistent":
        return oc.consistent_syndromes(case_id, B), oc.posteriors(case_id, B)
    assert c.rank_deficient
    return oc.inconsistent_syndromes(case_id, B), oc.posteriors(case_id, B, 1)


def host_osd(case_id, probs, method, order, side_tables=None):
    osd = HostOSD(oc.graph(case_id), probs, method, order)
    if side_tables is not None:
        osd.set_side_probs(*side_tables)
    return osd


# ------------------------------------------------------------------ quality (the oracle alone)
def _quality(oracle, code, direction, shots=2000):
    """Failures and non-converged second-sector decodes of independent and of ``direction`` BP+OSD
    decoding of the same errors: flooding min-sum(22), alpha 0.625, OSD-E(10), fp64, px = py = pz =
    0.04 / 3, errors from default_rng(1)."""
    p = 0.04
    probs = (p / 3, p / 3, p / 3)
    ex, ez = simulators.pauli_split(np.random.default_rng(1).random((shots, code.N)), probs)
    err = (ex | (ez << 1)).astype(np.uint8)
    p_first, p0, p1 = decoders.channel_update_probs(*probs, direction)
    bp = side_osd_ref.flooding_soft(oracle, 22)
    q2 = 1 if direction == "x->z" else 0
    out = {}
    for name, update in (("independent", False), ("update", True)):
        res = side_osd_ref.compose(oracle, code, err, direction, bp, p_first, p0, p1, "osd_e", 10, update=update)
        out[name] = (int((res["fail"][:, 0] | res["fail"][:, 1]).sum()), int((~res["conv"][:, q2]).sum()))
    return out


@pytest.mark.parametrize("direction", ["x->z", "z->x"])
def test_channel_update_bposd_cuts_failures(oracle, direction):
    """hgp_34_n225, px = py = pz = 0.04 / 3, 2,000 errors: update BP+OSD leaves at most 0.85 x the
    failures of independent BP+OSD (the oracle gives 0.70 and 0.67) and strictly fewer non-converged
    second-sector decodes."""
    q = _quality(oracle, codes.get_code("hgp_34_n225"), direction)
    (f_ind, nc_ind), (f_upd, nc_upd) = q["independent"], q["update"]
    print(f"{direction}: BP+OSD failures {f_ind} -> {f_upd} ({f_upd / max(1, f_ind):.3f}), "
          f"non-converged second sector {nc_ind} -> {nc_upd}")
    assert f_ind > 0
    assert f_upd <= 0.85 * f_ind
    assert nc_upd < nc_ind


# ------------------------------------------------------------------ host stage == the law
@pytest.mark.parametrize("kind", TABLES)
@pytest.mark.parametrize("method,order", oc.METHODS)
@pytest.mark.parametrize("case_id", CASES)
def test_host_side_decode_equals_the_law(oracle, case_id, method, order, kind):
    p0, p1 = tables(case_id, kind)
    osd = host_osd(case_id, p0, method, order, (p0, p1))
    H = oc.graph(case_id)
    conv = np.zeros(B, np.uint8)
    conv[5] = 1
    bpc = ((np.arange(B)[:, None] + np.arange(H.shape[1])[None, :]) % 3 == 0).astype(np.uint8)
    for synd_kind in ("consistent", "inconsistent"):
        if synd_kind == "inconsistent" and not oc.CASES[case_id].rank_deficient:
            continue
        synd, post = inputs(case_id, synd_kind)
        for density in DENSITIES:
            side = side_bytes(case_id, density)
            r0, rw = side_osd_ref.osd_side_batch(oracle, H, p0, p1, synd, post, side, method, order, conv, bpc)
            o0, ow = osd.decode_batch(synd, post, conv, bpc, threads=2, side=side)
            assert np.array_equal(o0, r0) and np.array_equal(ow, rw), (case_id, method, kind, synd_kind, density)


@pytest.mark.parametrize("kind", TABLES)
@pytest.mark.parametrize("method,order", oc.METHODS)
@pytest.mark.parametrize("case_id", CASES)
def test_host_side_anchors(case_id, method, order, kind):
    """side = 0 everywhere is the plain decode of the same handle (a uniform handle's popcount path
    included); side = 1 everywhere is the plain decode of a handle built on p1.  High bits are noise."""
    p0, p1 = tables(case_id, kind)
    osd = host_osd(case_id, p0, method, order, (p0, p1))
    on_p1 = host_osd(case_id, p1, method, order)
    n = oc.CASES[case_id].n
    synd, post = inputs(case_id, "consistent")
    zero = np.full((B, n), 0xFE, np.uint8)
    one = np.full((B, n), 0x03, np.uint8)
    a0, aw = osd.decode_batch(synd, post, side=zero)
    b0, bw = osd.decode_batch(synd, post)
    assert np.array_equal(a0, b0) and np.array_equal(aw, bw)
    c0, cw = osd.decode_batch(synd, post, side=one)
    d0, dw = on_p1.decode_batch(synd, post)
    assert np.array_equal(c0, d0) and np.array_equal(cw, dw)


@pytest.mark.parametrize("method,order", [m for m in oc.METHODS if m[0] != "osd_0"])
@pytest.mark.parametrize("case_id", [c for c in CASES if c not in oc.NO_IMPROVEMENT_NEEDED])
def test_the_side_bytes_change_decodes(case_id, method, order):
    """At least one of the 16 decodes at densities 0.03 and 0.5 differs from the plain p0 decode."""
    p0, p1 = tables(case_id, "nonuniform")
    osd = host_osd(case_id, p0, method, order, (p0, p1))
    synd, post = inputs(case_id, "consistent")
    _, plain = osd.decode_batch(synd, post)
    changed = 0
    for density in (0.03, 0.5):
        _, ow = osd.decode_batch(synd, post, side=side_bytes(case_id, density))
        changed += int((ow != plain).any(axis=1).sum())
    print(f"{case_id} {method}: {changed} of 16 decodes changed by the side bytes")
    assert changed >= 1


# ------------------------------------------------------------------ argument checks and symbols
@pytest.mark.parametrize("bad", [0.0, 1.0, float("nan")])
def test_bad_side_tables_are_refused(bad):
    case_id = "rr2_tail"
    n = oc.CASES[case_id].n
    osd = host_osd(case_id, oc.P_ERR, "osd_e", 4)
    good = np.full(n, 0.1)
    broken = good.copy()
    broken[n // 2] = bad
    for pair in ((broken, good), (good, broken)):
        with pytest.raises(QldpcError) as ei:
            osd.set_side_probs(*pair)
        assert ei.value.rc == EINVAL


def test_side_decode_without_tables_is_refused():
    case_id = "rr2_tail"
    osd = host_osd(case_id, oc.P_ERR, "osd_e", 4)
    synd, post = inputs(case_id, "consistent")
    with pytest.raises(QldpcError) as ei:
        osd.decode_batch(synd, post, side=side_bytes(case_id, 0.5))
    assert ei.value.rc == EINVAL


def test_new_symbols_and_abi_version():
    L = _native.lib()
    for name in ("qldpc_bp_decode_batch_side_soft", "qldpc_osd_set_side_probs", "qldpc_osd_decode_batch_side",
                 "qldpc_osd_gpu_set_side_probs", "qldpc_osd_gpu_decode_side", "qldpc_mc_set_staged_osd"):
        assert name in _native.EXPORTED
        assert isinstance(getattr(L, name), ctypes._CFuncPtr)
    assert L.qldpc_abi_version() == 1

"""GPU tests of the Relay-BP engine (csrc/relay.hip, engine 7).

The checker is the host law (``qldpc_relay_decode_host``, plain C++), which tests/test_relay_cpu.py
pins to the Python restatement of the law and to the oracle's min-sum BP; the kernel must equal it
bit for bit in corrections, iteration counts and convergence flags, with its state in LDS and with
the messages in the HBM workspace (``QLDPC_RELAY_WS=1``), and so must every loop that decodes
through the handle.
"""
import os

import numpy as np
import pytest

from qldpc_fault_tolerance_amd import _native, codes, decoders, simulators
from qldpc_fault_tolerance_amd.codes import CSR
from qldpc_fault_tolerance_amd.engine import (DeviceBP, DeviceMC, DeviceOSD, RelayParams, relay_decode_host,
                                              sample_errors, sample_errors_weight)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relay_n225.npz")
SEED = 0x9E3779B97F4A7C15
ENOTSUP = -4
RELAY = RelayParams(pre_iter=6, pre_gamma=0.125, num_legs=3, leg_iter=6, gamma_lo=-0.24, gamma_hi=0.66,
                    stop_nconv=2, gamma_seed=SEED)
MODES = [(64, False), (64, True), (32, False), (32, True)]  # (precision, messages in the HBM workspace)
MODE_IDS = ["f64-lds", "f64-ws", "f32-lds", "f32-ws"]

_cache = {}


def _code(name="hgp_34_n225"):
    if name not in _cache:
        _cache[name] = codes.get_code(name)
    return _cache[name]


def _syndromes(H, ps, per_p, seed):
    """per_p syndromes of i.i.d. errors at each rate of ps: easy to hopeless."""
    key = ("synd", id(H), tuple(ps), per_p, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        e = np.concatenate([(rng.random((per_p, H.n)) < p).astype(np.uint8) for p in ps])
        _cache[key] = H.matvec(e).astype(np.uint8)
    return _cache[key]


def _host(H, prior, relay, synd, alpha, precision):
    """The host law's (corr, iters, conv, nsol), computed once per argument set."""
    key = ("host", id(H), float(np.sum(prior)), relay, synd.tobytes(), alpha, precision)
    if key not in _cache:
        _cache[key] = relay_decode_host(H, prior, relay, synd, ms_scaling_factor=alpha, precision=precision)
    return _cache[key]


def _check(H, prior, relay, synd, precision, ws, monkeypatch, alpha=0.625, idx=True):
    monkeypatch.setenv("QLDPC_RELAY_WS", "1" if ws else "0")
    monkeypatch.setenv("QLDPC_RELAY_IDX", "1" if idx else "0")
    dec = DeviceBP(H, prior, ms_scaling_factor=alpha, precision=precision, relay=relay)
    geo = dec.geometry()
    assert geo["engine"] == 7 and geo["threads"] in (256, 512, 1024) and geo["blocks_per_cu"] >= 1
    assert 0 < geo["lds_bytes"] <= 160 * 1024
    corr, it, conv = dec.decode_batch(synd)
    hc, hi, hv, _ = _host(H, prior, relay, synd, alpha, precision)
    assert np.array_equal(corr, hc)
    assert np.array_equal(it, hi)
    assert np.array_equal(conv, hv)
    return dec, geo, (hc, hi, hv)


@pytest.mark.parametrize("precision,ws", MODES, ids=MODE_IDS)
def test_n225_equals_host_law(gpu, monkeypatch, precision, ws):
    H = _code().csr("hz")
    synd = _syndromes(H, (0.01, 0.03, 0.05, 0.08), 64, 1)
    synd = np.concatenate([synd, synd[:1]])  # B = 257
    _, geo, (_, it, conv) = _check(H, 0.03, RELAY, synd, precision, ws, monkeypatch)
    assert (conv & (it <= 6)).any() and (conv & (it > 6)).any() and (~conv).any()
    _check(H, 0.03, RELAY, synd[37:38], precision, ws, monkeypatch)  # B = 1
    # the other alpha schedule, one solution
    one = RelayParams(pre_iter=6, num_legs=3, leg_iter=6, stop_nconv=1, gamma_seed=SEED)
    _check(H, 0.03, one, synd[:64:3], precision, ws, monkeypatch, alpha=0.0)
    assert geo["threads"] == 256  # eight workgroups per CU fit: no widening
    if ws:  # the workspace holds the messages: LDS keeps M and the byte state only
        assert geo["lds_bytes"] < 2 * H.row_ptr[-1] * (precision // 8)


@pytest.mark.parametrize("precision,ws", MODES, ids=MODE_IDS)
def test_global_index_walk_equals_host_law(gpu, monkeypatch, precision, ws):
    """QLDPC_RELAY_IDX=0: the CSR / CSC read from global memory instead of the 16-bit copy in LDS (the
    path of graphs with more than 65,535 edges, or whose copy would cost a resident workgroup)."""
    H = _code().csr("hz")
    synd = _syndromes(H, (0.01, 0.03, 0.05, 0.08), 64, 1)[::3]
    _, staged, _ = _check(H, 0.03, RELAY, synd, precision, ws, monkeypatch)
    _, walked, _ = _check(H, 0.03, RELAY, synd, precision, ws, monkeypatch, idx=False)
    edges = int(H.row_ptr[-1])
    assert staged["lds_bytes"] - walked["lds_bytes"] >= 2 * (2 * edges + H.m + H.n + 2) - 16
    T = _code("tanner_code1").csr("hx")
    _check(T, 0.02, RELAY, _syndromes(T, (0.005, 0.02, 0.04), 20, 4), precision, ws, monkeypatch, idx=False)


@pytest.mark.parametrize("precision,ws", MODES, ids=MODE_IDS)
def test_state_is_reset_between_syndromes_of_a_workgroup(gpu, monkeypatch, precision, ws):
    """More syndromes than the persistent grid has workgroups: every workgroup decodes several, easy,
    multi-leg and never-converging ones in turn."""
    import torch

    H = _code().csr("hz")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_p = (10 * cus) // 3 + 1  # the wave cap is 8 workgroups of 256 threads per CU
    synd = _syndromes(H, (0.01, 0.05, 0.09), per_p, 2)
    rng = np.random.default_rng(3)
    synd = synd[rng.permutation(synd.shape[0])]
    relay = RelayParams(pre_iter=4, pre_gamma=0.125, num_legs=2, leg_iter=4, stop_nconv=2, gamma_seed=SEED)
    _, geo, (_, it, conv) = _check(H, 0.03, relay, synd, precision, ws, monkeypatch)
    assert synd.shape[0] > geo["blocks_per_cu"] * cus
    assert conv.any() and (~conv).any() and (conv & (it > 4)).any()


@pytest.mark.parametrize("precision,ws", MODES, ids=MODE_IDS)
def test_tanner_code_with_unequal_sector_degrees(gpu, monkeypatch, precision, ws):
    code = _code("tanner_code1")
    hz, hx = code.csr("hz"), code.csr("hx")
    assert (hz.row_degrees().max(), hz.col_degrees().max()) != (hx.row_degrees().max(), hx.col_degrees().max())
    for H in (hz, hx):
        _check(H, 0.02, RELAY, _syndromes(H, (0.005, 0.02, 0.04), 20, 4), precision, ws, monkeypatch)


@pytest.mark.parametrize("precision,ws", MODES, ids=MODE_IDS)
def test_tiny_graph_with_empty_row_and_column(gpu, monkeypatch, precision, ws):
    """5 x 9, row 2 and column 7 empty, every one of the 32 syndromes (row 2's bit can never be met).
    max_iter = 1 in all must still run the relay law, not the one-iteration first-min shortcut."""
    rows = [[0, 1, 2], [2, 3, 4, 5], [], [5, 6], [0, 6, 8]]
    D = np.zeros((5, 9), np.uint8)
    for i, r in enumerate(rows):
        D[i, r] = 1
    H = CSR.from_dense(D)
    synd = ((np.arange(32)[:, None] >> np.arange(5)) & 1).astype(np.uint8)
    prior = np.linspace(0.02, 0.2, 9)
    for relay in (RELAY, RelayParams(pre_iter=1, pre_gamma=0.3, num_legs=0),
                  RelayParams(pre_iter=1, pre_gamma=0.3, num_legs=2, leg_iter=1, stop_nconv=3, gamma_seed=5)):
        dec, _, (_, it, conv) = _check(H, prior, relay, synd, precision, ws, monkeypatch)
        assert not conv[synd[:, 2] == 1].any() and conv[0] and it[0] == min(relay.stop_nconv, 1 + relay.num_legs)
        assert dec.max_iter == relay.max_iter


@pytest.mark.parametrize("precision,ws", MODES, ids=MODE_IDS)
def test_n1600_equals_host_law(gpu, monkeypatch, precision, ws):
    H = _code("hgp_34_n1600").csr("hz")
    relay = RelayParams(pre_iter=12, pre_gamma=0.125, num_legs=2, leg_iter=10, stop_nconv=1, gamma_seed=SEED)
    synd = _syndromes(H, (0.01, 0.04, 0.06, 0.09), 16, 5)  # B = 64
    _, geo, (_, it, conv) = _check(H, 0.04, relay, synd, precision, ws, monkeypatch)
    assert conv.any() and (~conv).any()
    if not ws:  # LDS leaves one (fp64) or three (fp32) workgroups per CU: widened towards the CU's 32 waves
        resident = min(8, 160 * 1024 // geo["lds_bytes"])
        assert resident == (1 if precision == 64 else 3) and geo["threads"] > 256
        assert resident * geo["threads"] // 64 <= 32
        assert geo["threads"] == 1024 or resident * 2 * geo["threads"] // 64 > 32


@pytest.mark.parametrize("precision", [64, 32])
def test_kernel_equals_the_recorded_python_law(gpu, precision):
    g = np.load(GOLDEN)
    H = _code().csr("hz")
    relay = RelayParams(**{k: (float(g[k]) if "gamma" in k and k != "gamma_seed" else int(g[k]))
                           for k in ("pre_iter", "pre_gamma", "num_legs", "leg_iter", "gamma_lo", "gamma_hi",
                                     "stop_nconv", "gamma_seed")})
    dec = DeviceBP(H, float(g["p_prior"]), ms_scaling_factor=float(g["alpha"]), precision=precision, relay=relay)
    corr, it, conv = dec.decode_batch(g["synd"])
    assert np.array_equal(corr, g[f"corr{precision}"])
    assert np.array_equal(it, g[f"iters{precision}"])
    assert np.array_equal(conv, g[f"conv{precision}"].astype(bool))


@pytest.mark.parametrize("precision", [64, 32])
def test_no_legs_no_memory_is_plain_min_sum(gpu, precision):
    H = _code().csr("hz")
    synd = _syndromes(H, (0.01, 0.03, 0.05, 0.08), 64, 1)
    plain = DeviceBP(H, 0.04, max_iter=22, bp_method="minimum_sum", ms_scaling_factor=0.625, precision=precision)
    relay = DeviceBP(H, 0.04, ms_scaling_factor=0.625, precision=precision,
                     relay=RelayParams(pre_iter=22, pre_gamma=0.0, num_legs=0))
    a, b = plain.decode_batch(synd), relay.decode_batch(synd)
    assert plain.geometry()["engine"] != 7
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert b[2].any() and (~b[2]).any()


def test_set_channel_probs_rebuilds_priors_and_weights(gpu):
    H = _code().csr("hz")
    synd = _syndromes(H, (0.01, 0.03, 0.05, 0.08), 16, 6)
    p0 = 0.03 * np.ones(H.n)
    p1 = np.linspace(0.005, 0.12, H.n)
    dec = DeviceBP(H, p0, precision=64, relay=RELAY)
    first = dec.decode_batch(synd)
    dec.set_channel_probs(p1)
    second = dec.decode_batch(synd)
    for probs, got in ((p0, first), (p1, second)):
        ref = _host(H, probs, RELAY, synd, 0.625, 64)
        assert all(np.array_equal(x, y) for x, y in zip(got, ref[:3]))
    assert not np.array_equal(first[0], second[0])


# ------------------------------------------------------------------ shot loops
PX = PY = PZ = 0.02
PRIOR = 0.04
LOOP = dict(pre_iter=8, pre_gamma=0.125, num_legs=3, leg_iter=8, gamma_interval=(-0.24, 0.66), stop_nconv=2,
            gamma_seed=7)


def _sim(seed):
    code = _code()
    ones = PRIOR * np.ones(code.N)
    dx = decoders.RelayBPDecoder(code.hz, ones, **LOOP)
    dz = decoders.RelayBPDecoder(code.hx, ones, **LOOP)
    return simulators.CodeSimulator_DataError(code, dx, dz, [PX, PY, PZ], "Total", seed=seed), dx, dz


def _replay(err, relay):
    """The test's own pipeline on sampled errors [S, n] (bit0 x, bit1 z): syndromes, the host relay
    law, residuals, the [H; L] check -> (fail flags [S] bit0 X / bit1 Z, nonconv [2], iters [2])."""
    code = _code()
    fail = np.zeros(err.shape[0], np.uint8)
    nonconv, iters = [], []
    for q, (h, l) in enumerate((("hz", "lz"), ("hx", "lx"))):
        H, L = code.csr(h), code.csr(l)
        e = ((err >> q) & 1).astype(np.uint8)
        synd = H.matvec(e).astype(np.uint8)
        corr, it, conv, _ = relay_decode_host(H, PRIOR, relay, synd)
        r = e ^ corr.astype(np.uint8)
        fail |= ((H.matvec(r).any(axis=1) | L.matvec(r).any(axis=1)).astype(np.uint8) << q)
        nonconv.append(int((~conv).sum()))
        iters.append(int(it.sum()))
    return fail, nonconv, iters


def test_data_error_shot_loop_through_the_staged_pipeline(gpu):
    sim, dx, dz = _sim(seed=31)
    assert simulators._engine_bp(dx) is dx.decoder and dx.decoder.geometry()["engine"] == 7
    S = 2048
    res = sim.fused_counts(S)
    err = sample_errors(sim.N, PX, PY, PZ, 31, 0, S).cpu().numpy()
    fail, nonconv, iters = _replay(err, dx.relay)
    assert res.shots == S and res.failures == int((fail != 0).sum())
    assert res.sector_nonconv == nonconv and res.sector_iters == iters
    assert 0 < res.failures < S and min(nonconv) > 0
    mc = sim._mc
    whole = mc.run(PX, PY, PZ, 31, 0, S, "Total", per_shot=True)
    assert np.array_equal(whole.err, err) and np.array_equal(whole.fail, fail)
    a = mc.run(PX, PY, PZ, 31, 0, S // 2, "Total", per_shot=True)
    b = mc.run(PX, PY, PZ, 31, S // 2, S // 2, "Total", per_shot=True)
    assert np.array_equal(np.concatenate([a.fail, b.fail]), fail)
    both = a.merge(b)
    for k in ("shots", "failures", "sector_decodes", "sector_iters", "sector_nonconv", "sector_fail"):
        assert getattr(both, k) == getattr(whole, k) == getattr(res, k), k
    assert np.array_equal(both.iter_hist, res.iter_hist)
    # the reference-shaped entry points take the decoder like a BPDecoder
    wer, wer_eb = sim.WordErrorRate(256)
    assert 0.0 <= wer < 1.0


def test_launch_weight_accepts_a_relay_handle(gpu):
    sim, dx, dz = _sim(seed=5)
    mc = DeviceMC(_code(), dx.decoder, dz.decoder, staged=True)
    S, w = 512, 10
    res = mc.run_weight(w, PX, PY, PZ, seed=5, shot_begin=4096, shot_count=S, logical_mode="Total", per_shot=True)
    err = sample_errors_weight(sim.N, w, PX, PY, PZ, 5, 4096, S).cpu().numpy()
    fail, nonconv, iters = _replay(err, dx.relay)
    assert np.array_equal(res.err, err) and np.array_equal(res.fail, fail)
    assert res.failures == int((fail != 0).sum())
    assert res.sector_nonconv == nonconv and res.sector_iters == iters
    fails, shots = sim.FailureSpectrum([4, 10], 128)
    assert list(shots) == [128, 128] and all(0 <= f <= 128 for f in fails)


def test_phenomenological_final_round_takes_a_relay_handle(gpu):
    """decoder2 of the phenomenological loop as a relay handle: with no legs and no memory the run equals
    the plain-BP run in every counter and flag; with legs it decodes the same sampled histories."""
    from qldpc_fault_tolerance_amd.engine import DevicePhenl

    code = _code()
    m, n = code.hz.shape
    p, mi, S = 0.02, 22, 512
    st = [DeviceBP(codes.space_time_csr(h, 3), np.hstack([p * np.ones(n), p * np.ones(m)] * 3), max_iter=mi)
          for h in (code.hz, code.hx)]

    def run(make):
        d2 = [make(code.csr(k)) for k in ("hz", "hx")]
        return DevicePhenl(code, st[0], st[1], d2[0], d2[1], num_rep=3).run(p / 2, p / 2, p / 2, p, 3, 0, S, 3, "Total",
                                                                             per_shot=True)

    plain = run(lambda H: DeviceBP(H, p * np.ones(n), max_iter=mi))
    anchor = run(lambda H: DeviceBP(H, p * np.ones(n), relay=RelayParams(pre_iter=mi, pre_gamma=0.0, num_legs=0)))
    assert np.array_equal(anchor.fail, plain.fail) and np.array_equal(anchor.trace, plain.trace)
    for k in ("shots", "failures", "sector_decodes", "sector_iters", "sector_nonconv", "sector_fail"):
        assert getattr(anchor, k) == getattr(plain, k), k
    legs = run(lambda H: DeviceBP(H, p * np.ones(n), relay=RelayParams(pre_iter=mi, num_legs=4, leg_iter=mi, gamma_seed=2)))
    assert legs.shots == S and np.array_equal(legs.trace, plain.trace)
    assert legs.sector_decodes == plain.sector_decodes


def test_relay_decoder_classes(gpu):
    code = _code()
    cls = decoders.RelayBP_Decoder_Class(pre_iter_ratio=20, leg_iter_ratio=30, num_legs=2, stop_nconv=1, gamma_seed=3)
    d = cls.GetDecoder({"h": code.hz, "p_data": 0.03})
    assert (d.relay.pre_iter, d.relay.leg_iter, d.relay.num_legs) == (11, 7, 2) and d.max_iter == 25
    H = code.csr("hz")
    synd = _syndromes(H, (0.01, 0.03, 0.05, 0.08), 4, 8)
    corr, it, conv = d.decode_batch(synd)
    ref = _host(H, 0.03, d.relay, synd, 0.625, 64)
    assert all(np.array_equal(x, y) for x, y in zip((corr, it, conv), ref[:3]))
    one = d.decode(synd[0])
    assert np.array_equal(one, corr[0]) and d.iter == it[0] and d.converge == int(conv[0])
    st = cls.GetDecoder({"h": np.hstack([code.hz, np.eye(code.hz.shape[0], dtype=code.hz.dtype)]), "p_data": 0.03,
                         "p_syndrome": 0.02})
    assert st.num_qubits == code.N + code.hz.shape[0] and st.relay.pre_iter == 11


def test_no_soft_output_and_no_osd(gpu):
    code = _code()
    H = code.csr("hz")
    dec = DeviceBP(H, 0.03, relay=RELAY)
    assert dec.geometry()["engine"] == 7 and dec.geometry()["kernel_id"] == 7
    with pytest.raises(_native.QldpcError) as ei:
        dec.decode_batch_soft(np.zeros((2, H.m), np.uint8))
    assert ei.value.rc == ENOTSUP
    dz = DeviceBP(code.csr("hx"), 0.03, relay=RELAY)
    mc = DeviceMC(code, dec, dz)
    with pytest.raises(_native.QldpcError) as ei:
        mc.set_osd(DeviceOSD(dec.graph, 0.03 * np.ones(H.n), "osd_e", 4), None)
    assert ei.value.rc == ENOTSUP
    with pytest.raises(NotImplementedError):
        DeviceBP(H, 0.03, bp_method="product_sum", relay=RELAY)
    with pytest.raises(_native.QldpcError) as ei:
        DeviceBP(H, 0.03, relay=RelayParams(pre_iter=0))
    assert ei.value.rc == -1

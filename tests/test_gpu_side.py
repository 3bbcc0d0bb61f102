"""GPU tests of side-prior decoding (qldpc_bp_decode_batch_side on engines 7 and 8) and of X/Z-correlated
decoding in the staged data-error pipeline (qldpc_mc_set_channel_update).

The checker is the host side law (``qldpc_relay_decode_host_side`` / ``qldpc_serial_decode_host_side``,
plain C++), which tests/test_side_cpu.py pins to the Python restatement and to the oracle's min-sum BP;
the kernels must equal it bit for bit in corrections, iteration counts and convergence flags in every
mode, and the pipeline must equal the composition first sector -> side decode of the second -> check.
"""
import os
import random

import numpy as np
import pytest

import side_ref
from qldpc_fault_tolerance_amd import _native, codes, decoders, simulators
from qldpc_fault_tolerance_amd.engine import (DeviceBP, DeviceMC, DeviceOSD, RelayParams, relay_decode_host,
                                              relay_decode_host_side, sample_errors, sample_errors_weight,
                                              serial_decode_host, serial_decode_host_side)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "side_n225.npz")
SEED = 0x9E3779B97F4A7C15
EINVAL, ENOTSUP = -1, -4
RELAY = RelayParams(pre_iter=6, pre_gamma=0.125, num_legs=3, leg_iter=6, gamma_lo=-0.24, gamma_hi=0.66,
                    stop_nconv=2, gamma_seed=SEED)
SERIAL_ITER = 8
# (precision, messages in the HBM workspace, indices staged in LDS)
MODES = [(p, ws, idx) for p in (64, 32) for ws in (False, True) for idx in (True, False)]
MODE_IDS = [f"f{p}-{'ws' if ws else 'lds'}-{'idx' if idx else 'walk'}" for p, ws, idx in MODES]

_cache = {}


def _code(name="hgp_34_n225"):
    if name not in _cache:
        _cache[name] = codes.get_code(name)
    return _cache[name]


def _case(name, sector, per_p, seed, density=0.5):
    """(H, p0, p1, syndromes easy to hopeless, mixed side bytes with noise in the high bits)."""
    key = ("case", name, sector, per_p, seed, density)
    if key not in _cache:
        H = _code(name).csr(sector)
        rng = np.random.default_rng(seed)
        e = np.concatenate([(rng.random((per_p, H.n)) < p).astype(np.uint8) for p in (0.01, 0.03, 0.05, 0.08)])
        synd = H.matvec(e).astype(np.uint8)
        synd = np.concatenate([synd, synd[:1]])
        p0, p1 = side_ref.nonuniform_tables(H.n)
        side = side_ref.side_bytes(np.random.default_rng(9), synd.shape[0], H.n, density)
        _cache[key] = (H, p0, p1, synd, side)
    return _cache[key]


def _host_relay(H, p0, p1, relay, synd, side, alpha, precision):
    key = ("hr", id(H), relay, synd.tobytes(), side.tobytes(), alpha, precision)
    if key not in _cache:
        _cache[key] = relay_decode_host_side(H, p0, p1, relay, synd, side, ms_scaling_factor=alpha,
                                             precision=precision)[:3]
    return _cache[key]


def _host_serial(H, p0, p1, synd, side, alpha, precision):
    key = ("hs", id(H), synd.tobytes(), side.tobytes(), alpha, precision)
    if key not in _cache:
        _cache[key] = serial_decode_host_side(H, p0, p1, SERIAL_ITER, synd, side, ms_scaling_factor=alpha,
                                              precision=precision)
    return _cache[key]


def _equal(got, ref):
    assert np.array_equal(got[0], ref[0])
    assert np.array_equal(got[1], ref[1])
    assert np.array_equal(got[2], ref[2])


def _relay_dec(H, p0, p1, precision, ws, idx, monkeypatch, relay=RELAY, alpha=0.625):
    monkeypatch.setenv("QLDPC_RELAY_WS", "1" if ws else "0")
    monkeypatch.setenv("QLDPC_RELAY_IDX", "1" if idx else "0")
    dec = DeviceBP(H, p0, ms_scaling_factor=alpha, precision=precision, relay=relay)
    dec.set_side_probs(p0, p1)
    assert dec.geometry()["engine"] == 7
    return dec


def _serial_dec(H, p0, p1, precision, ws, idx, monkeypatch, tb=0, alpha=0.625):
    monkeypatch.setenv("QLDPC_SERIAL_WS", "1" if ws else "0")
    monkeypatch.setenv("QLDPC_SERIAL_IDX", "1" if idx else "0")
    monkeypatch.setenv("QLDPC_SERIAL_TB", str(tb))
    dec = DeviceBP(H, p0, max_iter=SERIAL_ITER, ms_scaling_factor=alpha, precision=precision, schedule="serial")
    dec.set_side_probs(p0, p1)
    geo = dec.geometry()
    assert geo["engine"] == 8 and (tb == 0 or geo["threads"] == tb)
    return dec


# ------------------------------------------------------------------ kernel == host side law
@pytest.mark.parametrize("precision,ws,idx", MODES, ids=MODE_IDS)
def test_relay_kernel_equals_host_side_law(gpu, monkeypatch, precision, ws, idx):
    H, p0, p1, synd, side = _case("hgp_34_n225", "hz", 64, 1)  # B = 257
    dec = _relay_dec(H, p0, p1, precision, ws, idx, monkeypatch)
    ref = _host_relay(H, p0, p1, RELAY, synd, side, 0.625, precision)
    _equal(dec.decode_batch(synd, side), ref)
    assert ref[2].any() and (~ref[2]).any() and (ref[2] & (ref[1] > 6)).any()
    _equal(dec.decode_batch(synd[37:38], side[37:38]), [r[37:38] for r in ref])  # B = 1
    # stop_nconv = 2: the per-shot weights decide which solution is kept
    key = ("hits", precision)
    if key not in _cache:
        _cache[key] = side_ref.second_solution_kept_by_side_weights(H, p0, p1, RELAY, synd, side, precision)
    assert len(_cache[key]) >= 1
    # the other alpha schedule
    dec0 = _relay_dec(H, p0, p1, precision, ws, idx, monkeypatch, alpha=0.0)
    _equal(dec0.decode_batch(synd[::5], side[::5]), _host_relay(H, p0, p1, RELAY, synd[::5], side[::5], 0.0, precision))


@pytest.mark.parametrize("precision,ws,idx", MODES, ids=MODE_IDS)
def test_relay_kernel_on_unequal_sector_degrees(gpu, monkeypatch, precision, ws, idx):
    for sector in ("hz", "hx"):
        H, p0, p1, synd, side = _case("tanner_code1", sector, 5, 4)  # B = 21
        dec = _relay_dec(H, p0, p1, precision, ws, idx, monkeypatch)
        _equal(dec.decode_batch(synd, side), _host_relay(H, p0, p1, RELAY, synd, side, 0.625, precision))


@pytest.mark.parametrize("precision,ws,idx", MODES, ids=MODE_IDS)
def test_serial_kernel_equals_host_side_law(gpu, monkeypatch, precision, ws, idx):
    H, p0, p1, synd, side = _case("hgp_34_n225", "hz", 64, 1)  # B = 257
    dec = _serial_dec(H, p0, p1, precision, ws, idx, monkeypatch)
    ref = _host_serial(H, p0, p1, synd, side, 0.625, precision)
    _equal(dec.decode_batch(synd, side), ref)
    assert ref[2].any() and (~ref[2]).any()
    _equal(dec.decode_batch(synd[37:38], side[37:38]), [r[37:38] for r in ref])  # B = 1
    dec0 = _serial_dec(H, p0, p1, precision, ws, idx, monkeypatch, alpha=0.0)
    _equal(dec0.decode_batch(synd[::5], side[::5]), _host_serial(H, p0, p1, synd[::5], side[::5], 0.0, precision))
    for sector in ("hz", "hx"):
        T, q0, q1, ts, tside = _case("tanner_code1", sector, 5, 4)
        _equal(_serial_dec(T, q0, q1, precision, ws, idx, monkeypatch).decode_batch(ts, tside),
               _host_serial(T, q0, q1, ts, tside, 0.625, precision))


@pytest.mark.parametrize("tb", [64, 256])
@pytest.mark.parametrize("precision,ws", [(64, False), (64, True), (32, False), (32, True)],
                         ids=["f64-lds", "f64-ws", "f32-lds", "f32-ws"])
def test_serial_kernel_widths(gpu, monkeypatch, precision, ws, tb):
    H, p0, p1, synd, side = _case("hgp_34_n225", "hz", 64, 1)
    dec = _serial_dec(H, p0, p1, precision, ws, True, monkeypatch, tb=tb)
    _equal(dec.decode_batch(synd, side), _host_serial(H, p0, p1, synd, side, 0.625, precision))
    T, q0, q1, ts, tside = _case("tanner_code1", "hx", 5, 4)
    _equal(_serial_dec(T, q0, q1, precision, ws, True, monkeypatch, tb=tb).decode_batch(ts, tside),
           _host_serial(T, q0, q1, ts, tside, 0.625, precision))


@pytest.mark.parametrize("precision", [64, 32])
def test_kernels_equal_the_recorded_law(gpu, precision):
    g = np.load(GOLDEN)
    H = _code().csr("hz")
    relay = RelayParams(**{k: (float(g[k]) if "gamma" in k and k != "gamma_seed" else int(g[k]))
                           for k in ("pre_iter", "pre_gamma", "num_legs", "leg_iter", "gamma_lo", "gamma_hi",
                                     "stop_nconv", "gamma_seed")})
    dec = DeviceBP(H, g["p0"], ms_scaling_factor=float(g["alpha"]), precision=precision, relay=relay)
    dec.set_side_probs(g["p0"], g["p1"])
    corr, it, conv = dec.decode_batch(g["synd"], g["side"])
    assert np.array_equal(corr, g[f"relay_corr{precision}"]) and np.array_equal(it, g[f"relay_iters{precision}"])
    assert np.array_equal(conv, g[f"relay_conv{precision}"].astype(bool))
    dec = DeviceBP(H, g["p0"], max_iter=int(g["serial_iter"]), ms_scaling_factor=float(g["alpha"]),
                   precision=precision, schedule="serial")
    dec.set_side_probs(g["p0"], g["p1"])
    corr, it, conv = dec.decode_batch(g["synd"], g["side"])
    assert np.array_equal(corr, g[f"serial_corr{precision}"]) and np.array_equal(it, g[f"serial_iters{precision}"])
    assert np.array_equal(conv, g[f"serial_conv{precision}"].astype(bool))


@pytest.mark.parametrize("engine", ["relay", "serial"])
@pytest.mark.parametrize("precision", [64, 32])
def test_anchors_against_the_plain_decode(gpu, precision, engine):
    """side = 0 with p0 = channel_probs is the handle's plain decode; side = 1 is the plain decode of a
    handle built on p1; replacing the tables takes effect; the plain decode never changes."""
    H, p0, p1, synd, _ = _case("hgp_34_n225", "hz", 16, 6)
    kw = dict(relay=RELAY) if engine == "relay" else dict(max_iter=SERIAL_ITER, schedule="serial")
    dec = DeviceBP(H, p0, precision=precision, **kw)
    plain0 = dec.decode_batch(synd)
    dec.set_side_probs(p0, p1)
    B = synd.shape[0]
    _equal(dec.decode_batch(synd, np.full((B, H.n), 0xFE, np.uint8)), plain0)
    on_p1 = DeviceBP(H, p1, precision=precision, **kw).decode_batch(synd)
    _equal(dec.decode_batch(synd, np.full((B, H.n), 0x03, np.uint8)), on_p1)
    assert not np.array_equal(plain0[0], on_p1[0])
    _equal(dec.decode_batch(synd), plain0)
    dec.set_side_probs(p1, p0)  # replaced: bit 0 now selects p0
    _equal(dec.decode_batch(synd, np.ones((B, H.n), np.uint8)), plain0)
    _equal(dec.decode_batch(synd), plain0)


@pytest.mark.parametrize("engine", ["relay", "serial"])
@pytest.mark.parametrize("precision,ws", [(64, False), (64, True), (32, False), (32, True)],
                         ids=["f64-lds", "f64-ws", "f32-lds", "f32-ws"])
def test_side_state_is_reset_between_syndromes_of_a_workgroup(gpu, monkeypatch, precision, ws, engine):
    """More syndromes than the persistent grid has workgroups, shuffled, the side density alternating
    between 0 and 0.5 from one syndrome to the next: a prior left over from the previous syndrome of a
    workgroup would show."""
    import torch

    H = _code().csr("hz")
    p0, p1 = side_ref.nonuniform_tables(H.n)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    relay = RelayParams(pre_iter=4, pre_gamma=0.125, num_legs=2, leg_iter=4, stop_nconv=2, gamma_seed=SEED)
    if engine == "relay":
        dec = _relay_dec(H, p0, p1, precision, ws, True, monkeypatch, relay=relay)
    else:
        dec = _serial_dec(H, p0, p1, precision, ws, True, monkeypatch)
    count = dec.geometry()["blocks_per_cu"] * cus + 37  # (one-wave serial workgroups: up to 24 per CU)
    key = ("reset", count)
    if key not in _cache:
        per_p = count // 3 + 1
        rng = np.random.default_rng(2)
        e = np.concatenate([(rng.random((per_p, H.n)) < p).astype(np.uint8) for p in (0.01, 0.05, 0.09)])
        synd = H.matvec(e).astype(np.uint8)
        synd = synd[rng.permutation(synd.shape[0])]
        side = side_ref.side_bytes(rng, synd.shape[0], H.n, 0.5)
        side[0::2] &= 0xFE  # density 0 on every other syndrome
        _cache[key] = (synd, side)
    synd, side = _cache[key]
    if engine == "relay":
        ref = _host_relay(H, p0, p1, relay, synd, side, 0.625, precision)
    else:
        ref = _host_serial(H, p0, p1, synd, side, 0.625, precision)
    assert synd.shape[0] > dec.geometry()["blocks_per_cu"] * cus
    _equal(dec.decode_batch(synd, side), ref)
    assert ref[2].any() and (~ref[2]).any()


@pytest.mark.parametrize("engine", ["relay", "serial"])
@pytest.mark.parametrize("precision", [64, 32])
def test_a_handle_without_side_tables_is_the_handle_of_today(gpu, precision, engine):
    """Side tables change neither the geometry nor the plain decode; without them a side decode is EINVAL."""
    H, p0, p1, synd, side = _case("hgp_34_n225", "hz", 16, 6)
    kw = dict(relay=RELAY) if engine == "relay" else dict(max_iter=SERIAL_ITER, schedule="serial")
    bare = DeviceBP(H, p0, precision=precision, **kw)
    with_side = DeviceBP(H, p0, precision=precision, **kw)
    geo = with_side.geometry()
    with_side.set_side_probs(p0, p1)
    assert bare.geometry() == geo == with_side.geometry()
    _equal(bare.decode_batch(synd), with_side.decode_batch(synd))
    host = (relay_decode_host(H, p0, RELAY, synd, precision=precision)[:3] if engine == "relay"
            else serial_decode_host(H, p0, SERIAL_ITER, synd, precision=precision)[:3])
    _equal(bare.decode_batch(synd), host)
    with pytest.raises(_native.QldpcError) as ei:
        bare.decode_batch(synd, side)
    assert ei.value.rc == EINVAL


# ------------------------------------------------------------------ staged pipeline
PROBS = (0.012, 0.01, 0.016)  # px, py, pz: a biased channel, so the two directions differ
MAX_ITER = 22
PLAIN22 = RelayParams(pre_iter=MAX_ITER, **side_ref.PLAIN)


def _pipeline(name, direction, second="relay"):
    """(mc, first_decode, second_decode) of a channel-update pipeline on code `name`: the first sector
    on engine 7 without legs, the second on engine 7 (or 8) with the conditional priors as side tables."""
    key = ("pipe", name, direction, second)
    if key not in _cache:
        code = _code(name)
        p_first, p0, p1 = decoders.channel_update_probs(*PROBS, direction)
        x_first = direction == "x->z"
        h1, h2 = (code.csr("hz"), code.csr("hx")) if x_first else (code.csr("hx"), code.csr("hz"))
        p_second = (PROBS[2] if x_first else PROBS[0]) + PROBS[1]  # the handle's ordinary prior: not used
        d1 = DeviceBP(h1, p_first, relay=PLAIN22)
        if second == "relay":
            d2 = DeviceBP(h2, p_second, relay=PLAIN22)
        else:
            d2 = DeviceBP(h2, p_second, max_iter=MAX_ITER, schedule="serial")
        d2.set_side_probs(p0, p1)
        mc = DeviceMC(code, d1 if x_first else d2, d2 if x_first else d1, staged=True)
        mc.set_channel_update(direction)

        def first(H, synd):
            return relay_decode_host(H, p_first, PLAIN22, synd)[:3]

        def second_fn(H, synd, side):
            if second == "relay":
                return relay_decode_host_side(H, p0, p1, PLAIN22, synd, side)[:3]
            return serial_decode_host_side(H, p0, p1, MAX_ITER, synd, side)

        _cache[key] = (mc, first, second_fn)
    return _cache[key]


def _check_result(res, comp, mode, S):
    bits = comp["fail"].astype(np.uint8)
    want_bits = (bits[:, 0] if mode != "Z" else 0) | ((bits[:, 1] << 1) if mode != "X" else 0)
    assert np.array_equal(res.corr, comp["corr"]) and np.array_equal(res.iters, comp["iters"])
    assert np.array_equal(res.fail, want_bits)
    assert res.shots == S and res.failures == int(side_ref.mode_failures(comp["fail"], mode).sum())
    assert res.sector_decodes == [S, S]
    assert res.sector_iters == comp["iters"].sum(0).tolist()
    assert res.sector_nonconv == (~comp["conv"]).sum(0).tolist()
    assert res.sector_fail == [int(bits[:, 0].sum()) if mode != "Z" else 0, int(bits[:, 1].sum()) if mode != "X" else 0]


@pytest.mark.parametrize("direction", ["x->z", "z->x"])
@pytest.mark.parametrize("name", ["hgp_34_n225", "tanner_code1"])
def test_staged_pipeline_equals_the_composition(gpu, name, direction):
    code = _code(name)
    mc, first, second = _pipeline(name, direction)
    S, seed = 4096 + 1, 31
    err = sample_errors(code.N, *PROBS, seed, 0, S).cpu().numpy()
    comp = side_ref.compose(code, err, direction, first, second)
    whole = mc.run(*PROBS, seed, 0, S, "Total", per_shot=True)
    assert np.array_equal(whole.err, err)
    _check_result(whole, comp, "Total", S)
    assert 0 < whole.failures < S and min(whole.sector_nonconv) > 0
    # the side decode is not the independent decode of the same syndromes
    ind = side_ref.compose(code, err, direction, first, lambda H, s, side: first(H, s))
    q2 = 1 if direction == "x->z" else 0
    assert not np.array_equal(ind["corr"][:, q2], comp["corr"][:, q2])
    # two launches over the split range
    cut = 1500
    a = mc.run(*PROBS, seed, 0, cut, "Total", per_shot=True)
    b = mc.run(*PROBS, seed, cut, S - cut, "Total", per_shot=True)
    assert np.array_equal(np.concatenate([a.fail, b.fail]), whole.fail)
    both = a.merge(b)
    for k in ("shots", "failures", "sector_decodes", "sector_iters", "sector_nonconv", "sector_fail"):
        assert getattr(both, k) == getattr(whole, k), k
    assert np.array_equal(both.iter_hist, whole.iter_hist)
    # qldpc_mc_run (counters only)
    import ctypes

    out = _native.Counters()
    _native.check(_native.lib().qldpc_mc_run(mc.handle, *PROBS, seed, 0, S, 2, ctypes.byref(out), None), "qldpc_mc_run")
    assert (out.shots, out.failures) == (S, whole.failures) and list(out.sector_iters) == whole.sector_iters


@pytest.mark.parametrize("mode", ["X", "Z"])
@pytest.mark.parametrize("direction", ["x->z", "z->x"])
def test_staged_pipeline_logical_modes(gpu, direction, mode):
    """Both sectors are decoded and tallied whatever the mode; the failure tally follows the mode."""
    code = _code()
    mc, first, second = _pipeline("hgp_34_n225", direction)
    S, seed = 1024 + 1, 32
    err = sample_errors(code.N, *PROBS, seed, 0, S).cpu().numpy()
    comp = side_ref.compose(code, err, direction, first, second)
    _check_result(mc.run(*PROBS, seed, 0, S, mode, per_shot=True), comp, mode, S)


@pytest.mark.parametrize("direction", ["x->z", "z->x"])
def test_staged_pipeline_at_fixed_weight_and_with_a_serial_second_sector(gpu, direction):
    code = _code()
    S, seed, w = 1024 + 1, 33, 12
    err = sample_errors_weight(code.N, w, *PROBS, seed, 4096, S).cpu().numpy()
    for second_engine in ("relay", "serial"):
        mc, first, second = _pipeline("hgp_34_n225", direction, second_engine)
        comp = side_ref.compose(code, err, direction, first, second)
        res = mc.run_weight(w, *PROBS, seed, 4096, S, "Total", per_shot=True)
        assert np.array_equal(res.err, err)
        _check_result(res, comp, "Total", S)


# ------------------------------------------------------------------ simulators
def _sim(direction, seed, schedule="parallel", mode="Total"):
    code = _code()
    px, py, pz = PROBS
    dx = decoders.BPDecoder(code.hz, (px + py) * np.ones(code.N), MAX_ITER, "minimum_sum", 0.625, schedule=schedule)
    dz = decoders.BPDecoder(code.hx, (pz + py) * np.ones(code.N), MAX_ITER, "minimum_sum", 0.625, schedule=schedule)
    return simulators.CodeSimulator_DataError(code, dx, dz, list(PROBS), mode, seed=seed, channel_update=direction)


def _sim_composition(direction, err, schedule="parallel"):
    """The composition with the first sector's prior as the user's decoder holds it (px + py or pz + py)."""
    code = _code()
    px, py, pz = PROBS
    _, p0, p1 = decoders.channel_update_probs(px, py, pz, direction)
    p_first = (px + py) if direction == "x->z" else (pz + py)
    if schedule == "serial":
        return side_ref.compose(code, err, direction,
                                lambda H, s: serial_decode_host(H, p_first, MAX_ITER, s)[:3],
                                lambda H, s, side: serial_decode_host_side(H, p0, p1, MAX_ITER, s, side))
    return side_ref.compose(code, err, direction,
                            lambda H, s: relay_decode_host(H, p_first, PLAIN22, s)[:3],
                            lambda H, s, side: relay_decode_host_side(H, p0, p1, PLAIN22, s, side)[:3])


@pytest.mark.parametrize("schedule", ["parallel", "serial"])
def test_simulator_fused_counts_and_spectrum_equal_the_composition(gpu, schedule):
    code = _code()
    S, seed = 2048 + 1, 41
    sim = _sim("x->z", seed, schedule)
    res = sim.fused_counts(S)
    err = sample_errors(code.N, *PROBS, seed, 0, S).cpu().numpy()
    comp = _sim_composition("x->z", err, schedule)
    assert res.shots == S and res.failures == int(side_ref.mode_failures(comp["fail"], "Total").sum())
    assert res.sector_iters == comp["iters"].sum(0).tolist() and res.sector_nonconv == (~comp["conv"]).sum(0).tolist()
    assert sim._mc_cu.dec_z.geometry()["engine"] == (8 if schedule == "serial" else 7)
    # the fixed-weight strata run on the same handle, after the shots fused_counts took
    weights, per = [6, 14], 257
    fails, shots = sim.FailureSpectrum(weights, per)
    assert list(shots) == [per, per]
    for i, w in enumerate(weights):
        e = sample_errors_weight(code.N, w, *PROBS, seed, S + i * per, per).cpu().numpy()
        c = _sim_composition("x->z", e, schedule)
        assert fails[i] == int(side_ref.mode_failures(c["fail"], "Total").sum())
    wer, _ = sim.WordErrorRate(256)
    assert 0.0 <= wer < 1.0
    wer, total = sim.WordErrorRate_TargetFailure(1, 128, 2)
    assert total in (128, 256)


def test_code_family_passes_channel_update_through(gpu):
    fam = simulators.CodeFamily([_code()], None, decoders.BP_Decoder_Class(10, "minimum_sum", 0.625))
    seen = []
    make = fam._data_simulator

    def spy(*args):
        seen.append(make(*args))
        return seen[-1]

    fam._data_simulator = spy
    w = fam.EvalWER("data", "Total", [0.04], 512, if_plot=False, channel_update="x->z")
    assert w.shape == (1, 1) and 0.0 <= w[0, 0] < 1.0
    s = fam.EvalWER_Stratified("Total", [0.04], 32, tail=1e-3, channel_update="z->x")
    assert s.shape == (1, 1) and 0.0 <= s[0, 0] < 1.0
    assert [x.channel_update for x in seen] == ["x->z", "z->x"]
    assert all(x._mc_cu is not None and x._mc_cu.channel_update == x.channel_update for x in seen)
    assert seen[0].last_result.sector_decodes == [512, 512]
    fam._data_simulator = make
    assert fam.EvalWER("data", "Total", [0.04], 64, if_plot=False).shape == (1, 1)


def test_simulator_single_run_equals_the_composition_per_shot(gpu):
    code = _code()
    px, py, pz = PROBS
    for direction in ("x->z", "z->x"):
        _, p0, p1 = decoders.channel_update_probs(px, py, pz, direction)
        x_first = direction == "x->z"
        side_kw = dict(side_probs=(p0, p1))
        dx = decoders.BPDecoder(code.hz, (px + py) * np.ones(code.N), MAX_ITER, "minimum_sum", 0.625,
                                **({} if x_first else side_kw))
        dz = decoders.BPDecoder(code.hx, (pz + py) * np.ones(code.N), MAX_ITER, "minimum_sum", 0.625,
                                **(side_kw if x_first else {}))
        sim = simulators.CodeSimulator_DataError(code, dx, dz, list(PROBS), "Total", channel_update=direction)
        random.seed(2024)
        got = [sim._single_run() for _ in range(24)]
        random.seed(2024)
        u = np.array([[random.random() for _ in range(code.N)] for _ in range(24)])
        ex, ez = simulators.pauli_split(u, PROBS)
        comp = _sim_composition(direction, (ex | (ez << 1)).astype(np.uint8))
        assert got == side_ref.mode_failures(comp["fail"], "Total").astype(int).tolist()
        # without side_probs on the second sector's decoder the per-shot run refuses
        plain = decoders.BPDecoder(code.hx if x_first else code.hz, 0.02 * np.ones(code.N), MAX_ITER, "minimum_sum", 0.625)
        bad = simulators.CodeSimulator_DataError(code, dx if x_first else plain, plain if x_first else dz, list(PROBS),
                                                 "Total", channel_update=direction)
        with pytest.raises(TypeError):
            bad._single_run()


def test_decoder_classes_with_side_probs(gpu):
    H, p0, p1, synd, side = _case("hgp_34_n225", "hz", 4, 8)
    d = decoders.BPDecoder(H, p0, MAX_ITER, "minimum_sum", 0.625, side_probs=(p0, p1))
    assert d.decoder.geometry()["engine"] == 7 and d.decoder.relay == PLAIN22
    _equal(d.decode_batch(synd, side), relay_decode_host_side(H, p0, p1, PLAIN22, synd, side)[:3])
    _equal(d.decode_batch(synd), relay_decode_host(H, p0, PLAIN22, synd)[:3])
    one = d.decode(synd[3], side=side[3])
    assert np.array_equal(one, d.decode_batch(synd, side)[0][3])
    s = decoders.BPDecoder(H, p0, SERIAL_ITER, "minimum_sum", 0.625, schedule="serial", side_probs=(p0, p1))
    assert s.decoder.geometry()["engine"] == 8
    _equal(s.decode_batch(synd, side), _host_serial(H, p0, p1, synd, side, 0.625, 64))
    r = decoders.RelayBPDecoder(H, p0, 6, num_legs=3, leg_iter=6, stop_nconv=2, gamma_seed=SEED, side_probs=(0.03, 0.3))
    assert r.relay == RELAY
    _equal(r.decode_batch(synd, side), relay_decode_host_side(H, 0.03, 0.3, RELAY, synd, side)[:3])
    with pytest.raises(ValueError):
        decoders.BPDecoder(H, p0, MAX_ITER, "product_sum", 0.625, side_probs=(p0, p1))


def test_refusals(gpu):
    code = _code()
    H = code.csr("hz")
    ones = 0.03 * np.ones(code.N)
    # an engine-3 handle, a product-sum handle and a soft engine-1 handle take no side tables
    for kw in (dict(), dict(bp_method="product_sum"), dict(soft=True)):
        dec = DeviceBP(H, ones, max_iter=MAX_ITER, **kw)
        assert dec.geometry()["engine"] not in (7, 8)
        with pytest.raises(_native.QldpcError) as ei:
            dec.set_side_probs(0.03, 0.3)
        assert ei.value.rc == ENOTSUP
        with pytest.raises(_native.QldpcError) as ei:
            dec.decode_batch(np.zeros((1, H.m), np.uint8), np.zeros((1, H.n), np.uint8))
        assert ei.value.rc == ENOTSUP
    relay = DeviceBP(H, ones, relay=PLAIN22)
    for bad in (0.0, 1.0, float("nan")):
        with pytest.raises(_native.QldpcError) as ei:
            relay.set_side_probs(0.03, bad)
        assert ei.value.rc == EINVAL
    dz = DeviceBP(code.csr("hx"), ones, relay=PLAIN22)
    # not staged: ENOTSUP; staged without side tables on the second sector, or without it: EINVAL
    fused = DeviceMC(code, DeviceBP(H, ones, max_iter=MAX_ITER), DeviceBP(code.csr("hx"), ones, max_iter=MAX_ITER))
    with pytest.raises(_native.QldpcError) as ei:
        fused.set_channel_update("x->z")
    assert ei.value.rc == ENOTSUP
    mc = DeviceMC(code, relay, dz, staged=True)
    with pytest.raises(_native.QldpcError) as ei:
        mc.set_channel_update("x->z")
    assert ei.value.rc == EINVAL
    with pytest.raises(_native.QldpcError) as ei:
        DeviceMC(code, relay, None, staged=True).set_channel_update("z->x")
    assert ei.value.rc == EINVAL
    with pytest.raises(ValueError):
        mc.set_channel_update("x<-z")
    dz.set_side_probs(0.02, 0.4)
    mc.set_channel_update("x->z")
    with pytest.raises(_native.QldpcError) as ei:  # z->x needs the tables on the X sector's decoder
        mc.set_channel_update("z->x")
    assert ei.value.rc == EINVAL
    with pytest.raises(_native.QldpcError) as ei:
        mc.set_osd(DeviceOSD(relay.graph, ones, "osd_e", 4), None)
    assert ei.value.rc == ENOTSUP
    mc.set_channel_update(None)  # off again: the independent pipeline
    res = mc.run(0.01, 0.01, 0.01, 1, 0, 64, "X")
    assert res.sector_decodes == [64, 0]
    # simulators: BP+OSD and product-sum sectors
    bposd = [decoders.BPOSD_Decoder(h, ones, MAX_ITER, "minimum_sum", 0.625, "osd_e", 4) for h in (code.hz, code.hx)]
    sim = simulators.CodeSimulator_DataError(code, bposd[0], bposd[1], [0.01] * 3, "Total", channel_update="x->z")
    for call in (lambda: sim.fused_counts(64), lambda: sim.WordErrorRate(64), lambda: sim.FailureSpectrum([4], 64),
                 sim._single_run):
        with pytest.raises(TypeError):
            call()
    ps = [decoders.BPDecoder(h, ones, MAX_ITER, "product_sum", 0.625) for h in (code.hz, code.hx)]
    sim = simulators.CodeSimulator_DataError(code, ps[0], ps[1], [0.01] * 3, "Total", channel_update="x->z")
    with pytest.raises(ValueError):
        sim.fused_counts(64)

"""GPU tests of BP+OSD under per-shot priors: the soft output of a side decode
(qldpc_bp_decode_batch_side_soft, engines 7 and 8), the GPU OSD's side decode
(qldpc_osd_gpu_decode_side, every layout), the BP+OSD stage of the staged shot loop with and without a
channel-update direction (qldpc_mc_set_staged_osd), and the Python surface on top.

Checkers: the host OSD stage's side decode (pinned to the per-syndrome oracle in
tests/test_side_osd_cpu.py), the oracle's soft min-sum BP and the serial law's host form under the
selected priors, the fused engine-3 BP+OSD loop, and the composition of tests/side_osd_ref.py.
Everything compared is bytes, integers or bit patterns of doubles: equality, no tolerance.
"""
import random

import numpy as np
import pytest

import bp_cases as bc
import bposd_ref
import css_cases
import osd_cases as oc
import side_osd_ref
import side_ref
from qldpc_fault_tolerance_amd import _native, codes, decoders, simulators
from qldpc_fault_tolerance_amd.engine import (DeviceBP, DeviceGraph, DeviceMC, DeviceOSD, HostOSD, RelayParams,
                                              sample_errors, sample_errors_weight, serial_decode_host)

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -1, -4
MAX_ITER = 22
PLAIN22 = RelayParams(pre_iter=MAX_ITER, **side_ref.PLAIN)
B = 8
SENTINEL = 0xA5
_cache = {}


def _code(name="hgp_34_n225"):
    if name not in _cache:
        _cache[name] = css_cases.code(name) if name in css_cases.CASES else codes.get_code(name)
    return _cache[name]


# ================================================================== 1. soft output of a side decode
SOFT_GRAPHS = ["n225_hz", "col1to8", "row33"]


def _soft_case(gid):
    """(H dense, syndromes [96, m] easy to hopeless, p0, p1, side bytes [96, n])."""
    if ("soft", gid) not in _cache:
        if gid == "n225_hz":
            H = np.ascontiguousarray(_code().hz.astype(np.uint8))
            rng = np.random.default_rng(11)
            e = np.concatenate([(rng.random((24, H.shape[1])) < p).astype(np.int64) for p in (0.01, 0.03, 0.05, 0.08)])
            synd = (e @ H.T.astype(np.int64) % 2).astype(np.uint8)
        else:
            H = bc.graph(gid)
            synd = np.array(bc.mixed(gid, 96))
        n = H.shape[1]
        p0, p1 = side_ref.nonuniform_tables(n)
        side = side_ref.side_bytes(np.random.default_rng(13), 96, n, 0.5)
        side[0::4] &= 0xFE  # every fourth syndrome at density 0
        _cache[("soft", gid)] = (H, synd, p0, p1, side)
    return _cache[("soft", gid)]


def _soft_dec(engine, H, probs, precision):
    if engine == 7:
        dec = DeviceBP(H, probs, precision=precision, relay=PLAIN22)
    else:
        dec = DeviceBP(H, probs, max_iter=MAX_ITER, precision=precision, schedule="serial", soft=True)
    assert dec.geometry()["engine"] == engine
    return dec


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _law_soft(oracle, engine, H, probs_rows, synd, precision):
    """Per-syndrome law: soft BP of syndrome b under the probability vector ``probs_rows[b]``."""
    bp = (side_osd_ref.flooding_soft(oracle, MAX_ITER, precision=precision) if engine == 7
          else side_osd_ref.serial_soft(MAX_ITER, precision=precision))
    out = [bp(H, pr, s[None]) for s, pr in zip(synd, probs_rows)]
    return (np.concatenate([o[0] for o in out]).astype(np.int64), np.concatenate([o[1] for o in out]),
            np.concatenate([np.asarray(o[2], bool) for o in out]), np.concatenate([o[3] for o in out]))


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("engine", [7, 8])
@pytest.mark.parametrize("gid", SOFT_GRAPHS)
def test_soft_side_decode(gpu, oracle, gid, engine, precision):
    H, synd, p0, p1, side = _soft_case(gid)
    dec = _soft_dec(engine, H, p0, precision)
    geo = dec.geometry()
    dec.set_side_probs(p0, p1)
    assert dec.geometry() == geo
    # plain: corr / iters / conv of decode_batch, posteriors of the engine's own law
    corr, it, conv, post = dec.decode_batch_soft(synd)
    c0, i0, v0 = dec.decode_batch(synd)
    assert np.array_equal(corr, c0) and np.array_equal(it, i0) and np.array_equal(conv, v0)
    assert conv.any() and (~conv).any()
    if engine == 7:  # pre_gamma = 0: engine 1's log_prob_ratios bit for bit
        e1 = DeviceBP(H, p0, max_iter=MAX_ITER, precision=precision, soft=True)
        assert e1.geometry()["engine"] == 1
        r = e1.decode_batch_soft(synd)
        assert np.array_equal(corr, r[0]) and np.array_equal(it, r[1]) and np.array_equal(conv, r[2])
        assert _same_bits(post, r[3])
    else:
        r = serial_decode_host(H, p0, MAX_ITER, synd, precision=precision)
        assert np.array_equal(corr, r[0]) and np.array_equal(it, r[1]) and np.array_equal(conv, r[2])
        assert _same_bits(post, r[3])
    # side decode: the same three outputs as decode_batch(synd, side), posteriors of the law under the
    # selected priors
    corr, it, conv, post = dec.decode_batch_soft(synd, side)
    c1, i1, v1 = dec.decode_batch(synd, side)
    assert np.array_equal(corr, c1) and np.array_equal(it, i1) and np.array_equal(conv, v1)
    key = ("law", gid, engine, precision)
    if key not in _cache:
        _cache[key] = _law_soft(oracle, engine, H, [side_osd_ref.selected(p0, p1, sb) for sb in side], synd, precision)
    law = _cache[key]
    assert np.array_equal(corr, law[0]) and np.array_equal(it, law[1]) and np.array_equal(conv, law[2])
    assert _same_bits(post, law[3])
    assert not _same_bits(post, dec.decode_batch_soft(synd)[3])
    # B = 1
    one = dec.decode_batch_soft(synd[37:38], side[37:38])
    assert np.array_equal(one[0], corr[37:38]) and one[1][0] == it[37] and _same_bits(one[3], post[37:38])


def test_soft_side_decode_refusals(gpu):
    H, synd, p0, p1, side = _soft_case("n225_hz")
    chain = DeviceBP(H, p0, relay=RelayParams(pre_iter=6, pre_gamma=0.125, num_legs=2, leg_iter=6))
    with pytest.raises(_native.QldpcError) as ei:  # a chain has no single posterior
        chain.decode_batch_soft(synd[:4])
    assert ei.value.rc == ENOTSUP
    hard = DeviceBP(H, p0, max_iter=MAX_ITER, schedule="serial")  # engine 8 without soft
    with pytest.raises(_native.QldpcError) as ei:
        hard.decode_batch_soft(synd[:4])
    assert ei.value.rc == ENOTSUP
    plain = DeviceBP(H, p0, relay=PLAIN22)  # no side tables
    with pytest.raises(_native.QldpcError) as ei:
        plain.decode_batch_soft(synd[:4], side[:4])
    assert ei.value.rc == EINVAL
    # qldpc_bp_decode_batch_soft keeps refusing engine 7
    import torch

    dev = torch.device("cuda", plain.graph.device)
    sd = torch.zeros((1, plain.m), dtype=torch.uint8, device=dev)
    corr = torch.zeros((1, plain.n), dtype=torch.uint8, device=dev)
    post = torch.zeros((1, plain.n), dtype=torch.float64, device=dev)
    rc = _native.lib().qldpc_bp_decode_batch_soft(plain.handle, sd.data_ptr(), corr.data_ptr(), None, None,
                                                  post.data_ptr(), 1, None)
    assert rc == ENOTSUP


# ================================================================== 2. GPU OSD side decode
OSD_CASES = ["rr2_tail", "rr8_pad", "rr20_pad", "lds_w27", "hbm_m830", "small_k", "rank0", "k0"]
DENSITIES = [0.0, 0.03, 0.5, 1.0]


def _tables(case_id, kind):
    n = oc.CASES[case_id].n
    if kind == "uniform":
        return oc.priors(case_id, "uniform"), np.full(n, 0.4)
    p1 = np.random.default_rng([oc.CASES[case_id].seed, 9]).uniform(0.05, 0.45, n)
    p1[::5] = p1[2]
    return oc.priors(case_id, "nonuniform"), p1


def _side_bytes(case_id, density, nb=B):
    rng = np.random.default_rng([5, int(density * 100), oc.CASES[case_id].seed])
    return side_ref.side_bytes(rng, nb, oc.CASES[case_id].n, density)


def _graph(case_id):
    if ("g", case_id) not in _cache:
        _cache[("g", case_id)] = DeviceGraph(oc.graph(case_id))
    return _cache[("g", case_id)]


def _device_osd(case_id, probs, method, order, side_tables=None):
    c = oc.CASES[case_id]
    osd = DeviceOSD(_graph(case_id), probs, method, order)
    geo = osd.geometry()
    assert (geo["row_words"], geo["threads"]) == (c.row_words, c.threads), (case_id, geo)
    if side_tables is not None:
        osd.set_side_probs(*side_tables)
        assert osd.geometry() == geo  # side tables change no layout
    return osd


def _bp_corr(nb, n):
    b, j = np.arange(nb)[:, None], np.arange(n)[None, :]
    return ((7 * j + 3 * b) % 5 == 0).astype(np.uint8)


def _gpu_decode(osd, synd, post, conv, corr, side=None):
    import torch

    dev = torch.device("cuda", osd.graph.device)
    nb, n = synd.shape[0], osd.graph.n
    up = lambda a: torch.from_numpy(np.array(a, order="C")).to(dev)  # noqa: E731
    o0 = torch.full((nb, n), SENTINEL, dtype=torch.uint8, device=dev)
    ow = torch.full((nb, n), SENTINEL, dtype=torch.uint8, device=dev)
    osd.decode_device(up(synd), up(post), up(conv), up(corr), o0, ow, side_dev=None if side is None else up(side))
    torch.cuda.synchronize(dev)
    return o0.cpu().numpy(), ow.cpu().numpy()


@pytest.mark.parametrize("kind", ["uniform", "nonuniform"])
@pytest.mark.parametrize("method,order", oc.METHODS)
@pytest.mark.parametrize("case_id", OSD_CASES)
def test_gpu_osd_side_decode_equals_the_host_stage(gpu, case_id, method, order, kind):
    c = oc.CASES[case_id]
    p0, p1 = _tables(case_id, kind)
    osd = _device_osd(case_id, p0, method, order, (p0, p1))
    host = HostOSD(oc.graph(case_id), p0, method, order)
    host.set_side_probs(p0, p1)
    conv = np.zeros(B, np.uint8)
    conv[5] = 1
    corr = _bp_corr(B, c.n)
    kinds = ["consistent"] + (["inconsistent"] if c.rank_deficient else [])
    for synd_kind in kinds:
        if synd_kind == "consistent":
            synd, post = oc.consistent_syndromes(case_id, B), oc.posteriors(case_id, B)
        else:
            synd, post = oc.inconsistent_syndromes(case_id, B), oc.posteriors(case_id, B, 1)
        for density in DENSITIES:
            side = _side_bytes(case_id, density)
            r0, rw = host.decode_batch(synd, post, conv, corr, side=side)
            o0, ow = _gpu_decode(osd, synd, post, conv, corr, side)
            assert np.array_equal(o0, r0) and np.array_equal(ow, rw), (case_id, method, kind, synd_kind, density)
    # anchors: side = 0 is the plain decode of this handle (a uniform handle's popcount path included),
    # side = 1 the plain decode of a handle built on p1; the plain decode itself is untouched
    synd, post = oc.consistent_syndromes(case_id, B), oc.posteriors(case_id, B)
    plain = _gpu_decode(osd, synd, post, conv, corr)
    bare = _gpu_decode(_device_osd(case_id, p0, method, order), synd, post, conv, corr)
    assert np.array_equal(plain[0], bare[0]) and np.array_equal(plain[1], bare[1])
    zero = _gpu_decode(osd, synd, post, conv, corr, np.full((B, c.n), 0xFE, np.uint8))
    assert np.array_equal(zero[0], plain[0]) and np.array_equal(zero[1], plain[1])
    one = _gpu_decode(osd, synd, post, conv, corr, np.full((B, c.n), 0x03, np.uint8))
    on_p1 = _gpu_decode(_device_osd(case_id, p1, method, order), synd, post, conv, corr)
    assert np.array_equal(one[0], on_p1[0]) and np.array_equal(one[1], on_p1[1])


def test_gpu_osd_side_weights_do_not_survive_into_the_next_syndrome(gpu):
    """A batch of four times the persistent grid on rr2_tail, the side bytes alternating between
    all-0 and all-1 rows: a weight staged for a workgroup's previous syndrome would show."""
    case_id, method, order, period = "rr2_tail", "osd_e", 4, 13
    c = oc.CASES[case_id]
    p0, p1 = _tables(case_id, "nonuniform")
    osd = _device_osd(case_id, p0, method, order, (p0, p1))
    wg = osd.geometry()["workgroups"]
    nb = 4 * wg
    idx = np.arange(nb) % period
    synd, post = oc.consistent_syndromes(case_id, period, salt=2), oc.posteriors(case_id, period, salt=2)
    host = HostOSD(oc.graph(case_id), p0, method, order)
    host.set_side_probs(p0, p1)
    ref = [host.decode_batch(synd, post, side=np.full((period, c.n), v, np.uint8)) for v in (0, 1)]
    assert not np.array_equal(ref[0][1], ref[1][1])  # the two tables decode differently
    which = (np.arange(nb) + np.arange(nb) // wg) % 2  # alternates along a workgroup's syndromes too
    side = np.repeat(which[:, None].astype(np.uint8), c.n, axis=1)
    conv = np.zeros(nb, np.uint8)
    o0, ow = _gpu_decode(osd, synd[idx], post[idx], conv, _bp_corr(nb, c.n), side)
    want0 = np.where(which[:, None] == 1, ref[1][0][idx], ref[0][0][idx])
    wantw = np.where(which[:, None] == 1, ref[1][1][idx], ref[0][1][idx])
    assert np.array_equal(o0, want0) and np.array_equal(ow, wantw)


def test_gpu_osd_side_refusals(gpu):
    case_id = "rr2_tail"
    c = oc.CASES[case_id]
    osd = _device_osd(case_id, oc.P_ERR, "osd_e", 4)
    synd, post = oc.consistent_syndromes(case_id, B), oc.posteriors(case_id, B)
    with pytest.raises(_native.QldpcError) as ei:  # no tables
        _gpu_decode(osd, synd, post, np.zeros(B, np.uint8), _bp_corr(B, c.n), _side_bytes(case_id, 0.5))
    assert ei.value.rc == EINVAL
    good = np.full(c.n, 0.1)
    for bad in (0.0, 1.0, float("nan")):
        broken = good.copy()
        broken[c.n // 2] = bad
        with pytest.raises(_native.QldpcError) as ei:
            osd.set_side_probs(good, broken)
        assert ei.value.rc == EINVAL


# ================================================================== 3. staged pipeline
PROBS = (0.016, 0.012, 0.014)  # px, py, pz
ORDER = 10


def _launch(mc, seed, S, mode, corr=False, weight=None, probs=None):
    """One launch with per-shot fail bits and errors (and corrections / iterations on request)."""
    import torch

    probs = PROBS if probs is None else probs
    dev = torch.device("cuda", mc.device)
    cnt = mc.new_counters()
    f = torch.zeros(S, dtype=torch.uint8, device=dev)
    e = torch.zeros((S, mc.code.N), dtype=torch.uint8, device=dev)
    c = torch.zeros((S, 2, mc.code.N), dtype=torch.uint8, device=dev) if corr else None
    it = torch.zeros((S, 2), dtype=torch.int32, device=dev) if corr else None
    if weight is None:
        mc.launch(*probs, seed, 0, S, mode, cnt, None, f, e, c, it)
    else:
        mc.launch_weight(weight, *probs, seed, 0, S, mode, cnt, f, e, c, it)
    torch.cuda.synchronize(dev)
    from qldpc_fault_tolerance_amd.engine import MCResult

    res = MCResult.from_words(cnt.cpu().numpy())
    res.fail, res.err = f.cpu().numpy(), e.cpu().numpy()
    if corr:
        res.corr, res.iters = c.cpu().numpy(), it.cpu().numpy()
    return res


def _priors():
    px, py, pz = PROBS
    return px + py, pz + py  # hz decoder (X sector), hx decoder (Z sector)


def _staged_bposd(engine, name="hgp_34_n225"):
    """A staged handle with BP+OSD in both sectors, no direction."""
    code = _code(name)
    pxs, pzs = _priors()
    if engine == 7:
        dx, dz = DeviceBP(code.csr("hz"), pxs, relay=PLAIN22), DeviceBP(code.csr("hx"), pzs, relay=PLAIN22)
    else:
        dx = DeviceBP(code.csr("hz"), pxs, max_iter=MAX_ITER, schedule="serial", soft=True)
        dz = DeviceBP(code.csr("hx"), pzs, max_iter=MAX_ITER, schedule="serial", soft=True)
    mc = DeviceMC(code, dx, dz, staged=True)
    mc.set_staged_osd(DeviceOSD(dx.graph, pxs, "osd_e", ORDER), DeviceOSD(dz.graph, pzs, "osd_e", ORDER))
    return mc


@pytest.mark.parametrize("mode", ["X", "Z", "Total"])
def test_staged_bposd_equals_the_fused_loop(gpu, monkeypatch, mode):
    """Engine 7 + set_staged_osd against the fused engine-3 qldpc_mc_set_osd loop, same seed."""
    code = _code()
    S, seed = 512, 51
    pxs, pzs = _priors()
    bx, bz = DeviceBP(code.csr("hz"), pxs, max_iter=MAX_ITER), DeviceBP(code.csr("hx"), pzs, max_iter=MAX_ITER)
    assert bx.geometry()["engine"] == 3
    fused = DeviceMC(code, bx, bz)
    fused.set_osd(DeviceOSD(bx.graph, pxs, "osd_e", ORDER), DeviceOSD(bz.graph, pzs, "osd_e", ORDER))
    want = _launch(fused, seed, S, mode)
    got = _launch(_staged_bposd(7), seed, S, mode)
    assert np.array_equal(got.err, want.err) and np.array_equal(got.fail, want.fail)
    assert got.failures == want.failures and got.sector_nonconv == want.sector_nonconv
    assert got.sector_fail == want.sector_fail and got.shots == S
    assert sum(got.sector_nonconv) > 0 and 0 < got.failures < S
    # a posterior buffer bounded to one batch of 64 shots: the same counters and verdicts
    monkeypatch.setenv("QLDPC_OSD_CAPTURE_MB", "0.11")  # 115343 bytes / (225 * 8) -> 64 shots
    small = _launch(_staged_bposd(7), seed, S, mode)
    assert np.array_equal(small.fail, got.fail) and np.array_equal(small.err, got.err)
    for k in ("failures", "sector_nonconv", "sector_fail", "sector_iters", "sector_decodes"):
        assert getattr(small, k) == getattr(got, k), k


class _SerialLaw:
    """``oracle`` for bposd_ref.oracle_sector_fails with the serial law's host form as its BP."""

    def __init__(self, oracle):
        self.osd_decode_batch = oracle.osd_decode_batch

    @staticmethod
    def bp_decode_batch_soft(H, p, mi, alpha, synd, precision):
        c, it, cv, post = serial_decode_host(H, p, mi, synd, ms_scaling_factor=alpha, precision=precision)
        return c.astype(np.uint8), it, cv, post


@pytest.mark.parametrize("mode", ["X", "Z", "Total"])
def test_staged_bposd_on_the_serial_engine_equals_the_oracle(gpu, oracle, mode):
    code = _code()
    S, seed = 512, 52
    got = _launch(_staged_bposd(8), seed, S, mode)
    err = sample_errors(code.N, *PROBS, seed, 0, S).cpu().numpy()
    assert np.array_equal(got.err, err)
    if "serial_fails" not in _cache:
        _cache["serial_fails"] = bposd_ref.oracle_sector_fails(_SerialLaw(oracle), code, err, _priors(), MAX_ITER, ORDER)
    sf = _cache["serial_fails"].astype(np.uint8)
    bits = (sf[:, 0] if mode != "Z" else 0) | ((sf[:, 1] << 1) if mode != "X" else 0)
    assert np.array_equal(got.fail, bits)
    assert got.failures == int(side_ref.mode_failures(sf.astype(bool), mode).sum())


def _cu_pipeline(name, direction, probs=PROBS):
    """(mc, composition inputs) of a BP+OSD channel-update pipeline on engine 7."""
    key = ("cu", name, direction, probs)
    if key not in _cache:
        code = _code(name)
        p_first, p0, p1 = decoders.channel_update_probs(*probs, direction)
        x_first = direction == "x->z"
        h1, h2 = (code.csr("hz"), code.csr("hx")) if x_first else (code.csr("hx"), code.csr("hz"))
        d1 = DeviceBP(h1, p_first, relay=PLAIN22)
        d2 = DeviceBP(h2, p_first, relay=PLAIN22)  # the handle's ordinary prior: not used
        d2.set_side_probs(p0, p1)
        o1 = DeviceOSD(d1.graph, p_first, "osd_e", ORDER)
        o2 = DeviceOSD(d2.graph, p_first, "osd_e", ORDER)
        o2.set_side_probs(p0, p1)
        mc = DeviceMC(code, d1 if x_first else d2, d2 if x_first else d1, staged=True)
        mc.set_staged_osd(o1 if x_first else o2, o2 if x_first else o1)
        mc.set_channel_update(direction)
        _cache[key] = (mc, p_first, p0, p1)
    return _cache[key]


def _check_cu(res, comp, S):
    bits = comp["fail"].astype(np.uint8)
    assert np.array_equal(res.corr, comp["corr"]) and np.array_equal(res.iters, comp["iters"])
    assert np.array_equal(res.fail, bits[:, 0] | (bits[:, 1] << 1))
    assert res.shots == S and res.failures == int((comp["fail"][:, 0] | comp["fail"][:, 1]).sum())
    assert res.sector_decodes == [S, S]
    assert res.sector_iters == comp["iters"].sum(0).tolist()
    assert res.sector_nonconv == (~comp["conv"]).sum(0).tolist()


@pytest.mark.parametrize("direction", ["x->z", "z->x"])
@pytest.mark.parametrize("name,S,probs", [("hgp_34_n225", 512, PROBS), ("asym112", 256, (0.03, 0.025, 0.035))])
def test_staged_bposd_channel_update_equals_the_composition(gpu, oracle, name, S, probs, direction):
    code = _code(name)
    seed = 53
    mc, p_first, p0, p1 = _cu_pipeline(name, direction, probs)
    res = _launch(mc, seed, S, "Total", corr=True, probs=probs)
    err = sample_errors(code.N, *probs, seed, 0, S).cpu().numpy()
    assert np.array_equal(res.err, err)
    bp = side_osd_ref.flooding_soft(oracle, MAX_ITER)
    comp = side_osd_ref.compose(oracle, code, err, direction, bp, p_first, p0, p1, "osd_e", ORDER)
    _check_cu(res, comp, S)
    # the second sector's OSD correction is not the independent one's on every shot
    ind = side_osd_ref.compose(oracle, code, err, direction, bp, p_first, p0, p1, "osd_e", ORDER, update=False)
    q2 = 1 if direction == "x->z" else 0
    handed = ~comp["conv"][:, q2] & ~ind["conv"][:, q2]
    differs = (comp["corr"][:, q2] != ind["corr"][:, q2]).any(axis=1)
    print(f"{name} {direction}: {int((handed & differs).sum())} second-sector OSD corrections differ "
          f"from the independent ones ({int(handed.sum())} handed to OSD in both)")
    assert (handed & differs).any()
    if name == "hgp_34_n225":  # one fixed weight through qldpc_mc_launch_weight
        w = 14
        rw = _launch(mc, seed, 257, "Total", corr=True, weight=w, probs=probs)
        ew = sample_errors_weight(code.N, w, *probs, seed, 0, 257).cpu().numpy()
        assert np.array_equal(rw.err, ew)
        _check_cu(rw, side_osd_ref.compose(oracle, code, ew, direction, bp, p_first, p0, p1, "osd_e", ORDER), 257)


def test_staged_bposd_refusals(gpu):
    code = _code()
    pxs, pzs = _priors()
    H = code.csr("hz")
    # a fused handle takes no staged stage
    bx, bz = DeviceBP(H, pxs, max_iter=MAX_ITER), DeviceBP(code.csr("hx"), pzs, max_iter=MAX_ITER)
    fused = DeviceMC(code, bx, bz)
    with pytest.raises(_native.QldpcError) as ei:
        fused.set_staged_osd(DeviceOSD(bx.graph, pxs, "osd_e", 4), None)
    assert ei.value.rc == ENOTSUP
    # a sector decoder without soft output: a relay chain, an engine-3 decoder in the staged loop
    chain = DeviceBP(H, pxs, relay=RelayParams(pre_iter=6, pre_gamma=0.125, num_legs=2, leg_iter=6))
    dz = DeviceBP(code.csr("hx"), pzs, relay=PLAIN22)
    for dx in (chain, bx):
        mc = DeviceMC(code, dx, dz if dx is chain else bz, staged=True)
        with pytest.raises(_native.QldpcError) as ei:
            mc.set_staged_osd(DeviceOSD(dx.graph, pxs, "osd_e", 4), None)
        assert ei.value.rc == ENOTSUP
    # an OSD handle of another graph
    dx = DeviceBP(H, pxs, relay=PLAIN22)
    mc = DeviceMC(code, dx, dz, staged=True)
    with pytest.raises(_native.QldpcError) as ei:
        mc.set_staged_osd(DeviceOSD(dz.graph, pzs, "osd_e", 4), None)
    assert ei.value.rc == EINVAL
    # qldpc_mc_set_osd keeps refusing staged handles
    with pytest.raises(_native.QldpcError) as ei:
        mc.set_osd(DeviceOSD(dx.graph, pxs, "osd_e", 4), None)
    assert ei.value.rc == ENOTSUP
    # a direction needs side tables on the second sector's OSD handle, whichever call comes second
    dz.set_side_probs(0.02, 0.4)
    ox, oz = DeviceOSD(dx.graph, pxs, "osd_e", 4), DeviceOSD(dz.graph, pzs, "osd_e", 4)
    mc.set_staged_osd(ox, oz)
    with pytest.raises(_native.QldpcError) as ei:
        mc.set_channel_update("x->z")
    assert ei.value.rc == EINVAL
    mc.set_staged_osd(None, None)
    mc.set_channel_update("x->z")
    with pytest.raises(_native.QldpcError) as ei:
        mc.set_staged_osd(ox, oz)
    assert ei.value.rc == EINVAL
    oz.set_side_probs(0.02, 0.4)
    mc.set_staged_osd(ox, oz)
    res = mc.run(*PROBS, 1, 0, 64, "Total")
    assert res.sector_decodes == [64, 64]


# ================================================================== 4. Python surface
def _bposd_pair(direction, schedule="parallel", side=True):
    code = _code()
    px, py, pz = PROBS
    _, p0, p1 = decoders.channel_update_probs(px, py, pz, direction)
    x_first = direction == "x->z"
    kw = dict(side_probs=(p0, p1)) if side else {}
    dx = decoders.BPOSD_Decoder(code.hz, (px + py) * np.ones(code.N), MAX_ITER, "minimum_sum", 0.625, "osd_e", ORDER,
                                schedule=schedule, **({} if x_first else kw))
    dz = decoders.BPOSD_Decoder(code.hx, (pz + py) * np.ones(code.N), MAX_ITER, "minimum_sum", 0.625, "osd_e", ORDER,
                                schedule=schedule, **(kw if x_first else {}))
    return dx, dz, p0, p1


def _sim_composition(oracle, direction, err, schedule="parallel"):
    px, py, pz = PROBS
    _, p0, p1 = decoders.channel_update_probs(px, py, pz, direction)
    p_first = (px + py) if direction == "x->z" else (pz + py)
    bp = side_osd_ref.flooding_soft(oracle, MAX_ITER) if schedule == "parallel" else side_osd_ref.serial_soft(MAX_ITER)
    return side_osd_ref.compose(oracle, _code(), err, direction, bp, p_first, p0, p1, "osd_e", ORDER)


@pytest.mark.parametrize("schedule", ["parallel", "serial"])
def test_bposd_decoder_with_side_probs(gpu, oracle, schedule):
    code = _code()
    H = code.csr("hx")
    dx, dz, p0, p1 = _bposd_pair("x->z", schedule)
    assert dz.decoder.geometry()["engine"] == (7 if schedule == "parallel" else 8)
    assert dx.decoder.geometry()["engine"] == (1 if schedule == "parallel" else 8)  # without side_probs: as before
    rng = np.random.default_rng(3)
    e = (rng.random((24, code.N)) < 0.04).astype(np.uint8)
    synd = H.matvec(e).astype(np.uint8)
    side = side_ref.side_bytes(rng, 24, code.N, 0.05)
    bp = side_osd_ref.flooding_soft(oracle, MAX_ITER) if schedule == "parallel" else side_osd_ref.serial_soft(MAX_ITER)
    want, it, conv = side_osd_ref.bposd_side(oracle, bp, H, p0, p1, synd, side, "osd_e", ORDER)
    assert (~conv).any()
    got = dz.decode_batch(synd, side)
    assert np.array_equal(got, want) and np.array_equal(dz.iters_batch, it) and np.array_equal(dz.conv_batch, conv)
    assert np.array_equal(dz.decode(synd[3], side=side[3]), want[3])
    pz_prior = (PROBS[2] + PROBS[1]) * np.ones(code.N)
    plain = side_osd_ref.bposd(oracle, bp, H, pz_prior, synd, "osd_e", ORDER)[0]
    assert np.array_equal(dz.decode_batch(synd), plain)
    # the host OSD stage carries the same tables
    host = decoders.BPOSD_Decoder(code.hx, pz_prior, MAX_ITER, "minimum_sum", 0.625, "osd_e", ORDER, schedule=schedule,
                                  side_probs=(p0, p1), use_gpu_osd=False)
    assert host.gpu_osd is None and np.array_equal(host.decode_batch(synd, side), want)
    with pytest.raises(TypeError):
        dx.decode_batch(synd[:, :dx.num_checks], side)  # built without side_probs
    with pytest.raises(ValueError):
        decoders.BPOSD_Decoder(code.hx, pz_prior, MAX_ITER, "product_sum", 0.625, "osd_e", ORDER, side_probs=(p0, p1))
    fac = decoders.BPOSD_Decoder_Class(10, "minimum_sum", 0.625, "osd_e", ORDER, schedule=schedule)
    made = fac.GetDecoder({"h": code.hx, "p_data": 0.03, "side_probs": (p0, p1)})
    assert made.side_probs is not None and made.decoder.geometry()["engine"] == (7 if schedule == "parallel" else 8)
    assert fac.GetDecoder({"h": code.hx, "p_data": 0.03}).side_probs is None


@pytest.mark.parametrize("direction", ["x->z", "z->x"])
def test_simulator_bposd_channel_update(gpu, oracle, direction):
    code = _code()
    dx, dz, _, _ = _bposd_pair(direction)
    S, seed = 384, 61
    sim = simulators.CodeSimulator_DataError(code, dx, dz, list(PROBS), "Total", seed=seed, channel_update=direction)
    res = sim.fused_counts(S)
    err = sample_errors(code.N, *PROBS, seed, 0, S).cpu().numpy()
    comp = _sim_composition(oracle, direction, err)
    assert res.shots == S and res.failures == int((comp["fail"][:, 0] | comp["fail"][:, 1]).sum())
    assert res.sector_iters == comp["iters"].sum(0).tolist() and res.sector_nonconv == (~comp["conv"]).sum(0).tolist()
    # _single_run equals the fused path per shot on replayed uniforms
    random.seed(2025)
    got = [sim._single_run() for _ in range(24)]
    random.seed(2025)
    u = np.array([[random.random() for _ in range(code.N)] for _ in range(24)])
    mc = sim._mc_cu
    per = mc.run(*PROBS, 0, 0, 24, "Total", uniforms=u, per_shot=True)
    assert got == (per.fail != 0).astype(int).tolist()
    ex, ez = simulators.pauli_split(u, PROBS)
    c = _sim_composition(oracle, direction, (ex | (ez << 1)).astype(np.uint8))
    assert got == (c["fail"][:, 0] | c["fail"][:, 1]).astype(int).tolist()
    # the other entry points run
    f, shots, osd_n = sim.bposd_counts(128)
    assert shots == 128 and 0 <= f <= 128 and osd_n >= 0
    wer, _ = sim.WordErrorRate(128)
    assert 0.0 <= wer < 1.0
    fails, shots = sim.FailureSpectrum([6, 14], 65)
    assert list(shots) == [65, 65]


def test_simulator_refusals_and_code_family(gpu):
    code = _code()
    dx, dz, p0, p1 = _bposd_pair("x->z")
    # mixed BP / BP+OSD sectors
    bp = decoders.BPDecoder(code.hz, 0.03 * np.ones(code.N), MAX_ITER, "minimum_sum", 0.625)
    sim = simulators.CodeSimulator_DataError(code, bp, dz, list(PROBS), "Total", channel_update="x->z")
    for call in (lambda: sim.fused_counts(64), lambda: sim.WordErrorRate(64), sim._single_run):
        with pytest.raises(TypeError):
            call()
    # BP+OSD sectors without side_probs keep refusing
    ax, az, _, _ = _bposd_pair("x->z", side=False)
    sim = simulators.CodeSimulator_DataError(code, ax, az, list(PROBS), "Total", channel_update="x->z")
    for call in (lambda: sim.fused_counts(64), lambda: sim.WordErrorRate(64), lambda: sim.FailureSpectrum([4], 64),
                 lambda: sim.bposd_counts(64), sim._single_run):
        with pytest.raises(TypeError):
            call()
    # CodeFamily hands side_probs to the second sector's factory call
    fam = simulators.CodeFamily([code], None, decoders.BPOSD_Decoder_Class(10, "minimum_sum", 0.625, "osd_e", ORDER))
    seen = []
    make = fam._data_simulator

    def spy(*args):
        seen.append(make(*args))
        return seen[-1]

    fam._data_simulator = spy
    w = fam.EvalWER("data", "Total", [0.04], 256, if_plot=False, channel_update="x->z")
    assert w.shape == (1, 1) and 0.0 <= w[0, 0] < 1.0
    w = fam.EvalWER("data", "Total", [0.04], 256, if_plot=False, channel_update="z->x")
    assert w.shape == (1, 1) and 0.0 <= w[0, 0] < 1.0
    assert [x.channel_update for x in seen] == ["x->z", "z->x"]
    assert seen[0].decoder_z.side_probs is not None and seen[0].decoder_x.side_probs is None
    assert seen[1].decoder_x.side_probs is not None and seen[1].decoder_z.side_probs is None
    assert all(x._mc_cu is not None and x.last_result.sector_decodes == [256, 256] for x in seen)
    fam._data_simulator = make
    assert fam.EvalWER("data", "Total", [0.04], 64, if_plot=False).shape == (1, 1)

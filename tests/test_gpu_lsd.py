"""BP+LSD on the GPU above the kernel: BPLSD_Decoder against oracle BP followed by the Python law, the
fused and the staged data-error shot loops with DeviceLSD handles against the host pipeline (oracle BP +
host law + failure check), X/Z-correlated decoding (channel_update) with two BPLSD_Decoders against its
host restatement, and the phenomenological simulator with a BPLSD_Decoder as decoder2.
"""
import numpy as np
import pytest

import lsd_ref
import side_osd_ref
import side_ref
from qldpc_fault_tolerance_amd import codes, decoders, simulators
from qldpc_fault_tolerance_amd.engine import (DeviceBP, DeviceLSD, DeviceMC, HostLSD, MCResult, RelayParams,
                                              sample_errors)
from qldpc_fault_tolerance_amd.simulators import gf2_rows

pytestmark = pytest.mark.gpu

MAX_ITER = 22
PROBS = (0.016, 0.012, 0.014)  # px, py, pz
PLAIN22 = RelayParams(pre_iter=MAX_ITER, **side_ref.PLAIN)


@pytest.fixture(scope="module")
def code():
    return codes.get_code("hgp_34_n225")


def _host_lsd(k):
    """``second(H, synd, post, conv, corr) -> x``: BP's correction where it converged, else the host law."""
    def stage(H, synd, post, conv, corr):
        x = np.asarray(corr, np.uint8).copy()
        nc = np.flatnonzero(~np.asarray(conv, bool))
        if nc.size:
            x[nc] = HostLSD(H, k).decode_batch_stats(synd[nc], post[nc])[0]
        return x
    return stage


@pytest.mark.parametrize("k", [1, 3])
def test_bplsd_decoder_equals_oracle_bp_then_the_law(gpu, oracle, code, k):
    H = code.hz.astype(np.uint8)
    p = 0.06
    rng = np.random.default_rng(31)
    e = (rng.random((64, code.N)) < p).astype(np.uint8)
    synd = gf2_rows(code.csr("hz"), e)
    corr, iters, conv, post = oracle.bp_decode_batch_soft(H, p, MAX_ITER, 0.625, synd)
    assert (~conv).sum() >= 8 and conv.any()
    want = corr.astype(np.uint8).copy()
    stats = np.tile(np.array([1, 0, 0, 0], np.int32), (64, 1))
    g = lsd_ref.Graph(H)
    for b in np.flatnonzero(~conv):
        want[b], stats[b], _ = lsd_ref.decode(g, synd[b], post[b], k)
    dec = decoders.BPLSD_Decoder(code.hz, p * np.ones(code.N), MAX_ITER, "minimum_sum", 0.625, bits_per_step=k)
    assert isinstance(dec, decoders.BPOSD_Decoder) and isinstance(dec.gpu_osd, DeviceLSD)
    got = dec.decode_batch(synd)
    assert np.array_equal(got, want) and np.array_equal(dec.osd0_batch, want)
    assert np.array_equal(dec.conv_batch, conv) and np.array_equal(dec.iters_batch, iters)
    x, st = dec.lsd_stats_batch(synd)
    assert np.array_equal(x, want) and np.array_equal(st, stats)
    b = int(np.flatnonzero(~conv)[0])
    assert np.array_equal(dec.decode(synd[b]), want[b]) and np.array_equal(dec.osd0_decoding, dec.osdw_decoding)
    host = decoders.BPLSD_Decoder(code.hz, p * np.ones(code.N), MAX_ITER, "minimum_sum", 0.625, bits_per_step=k,
                                  use_gpu_osd=False)
    assert host.gpu_osd is None and np.array_equal(host.decode_batch(synd), want)
    made = decoders.BPLSD_Decoder_Class(10, "minimum_sum", 0.625, bits_per_step=k).GetDecoder(
        {"h": code.hz, "p_data": p})
    assert made.bits_per_step == k and np.array_equal(made.decode_batch(synd), want)


def _launch(mc, seed, S, mode):
    import torch

    dev = torch.device("cuda", mc.device)
    cnt = mc.new_counters()
    f = torch.zeros(S, dtype=torch.uint8, device=dev)
    e = torch.zeros((S, mc.code.N), dtype=torch.uint8, device=dev)
    mc.launch(*PROBS, seed, 0, S, mode, cnt, None, f, e, None, None)
    torch.cuda.synchronize(dev)
    res = MCResult.from_words(cnt.cpu().numpy())
    res.fail, res.err = f.cpu().numpy(), e.cpu().numpy()
    return res


def _host_pipeline(oracle, code, err, k):
    """Per shot and sector: (fail [S, 2], conv [S, 2]) of oracle BP, the host law where BP did not
    converge, and the failure check (the shape of bposd_ref.oracle_sector_fails)."""
    px, py, pz = PROBS
    fail = np.zeros((err.shape[0], 2), bool)
    conv = np.zeros((err.shape[0], 2), bool)
    stage = _host_lsd(k)
    for q, name, lname, pq in ((0, "hz", "lz", px + py), (1, "hx", "lx", pz + py)):
        H = getattr(code, name).astype(np.uint8)
        e = ((err >> q) & 1).astype(np.uint8)
        synd = gf2_rows(code.csr(name), e)
        c, _, cv, post = oracle.bp_decode_batch_soft(H, pq, MAX_ITER, 0.625, synd)
        r = e ^ stage(H, synd, post, cv, c)
        fail[:, q] = gf2_rows(code.csr(name), r).any(1) | gf2_rows(code.csr(lname), r).any(1)
        conv[:, q] = cv
    return fail, conv


@pytest.mark.parametrize("staged", [False, True], ids=["fused", "staged"])
@pytest.mark.parametrize("k", [1, 2])
def test_shot_loops_with_lsd_handles_equal_the_host_pipeline(gpu, oracle, code, k, staged):
    S, seed = 512, 71
    px, py, pz = PROBS
    if staged:
        dx, dz = DeviceBP(code.csr("hz"), px + py, relay=PLAIN22), DeviceBP(code.csr("hx"), pz + py, relay=PLAIN22)
        mc = DeviceMC(code, dx, dz, staged=True)
        mc.set_staged_osd(DeviceLSD(dx.graph, k), DeviceLSD(dz.graph, k))
    else:
        dx, dz = DeviceBP(code.csr("hz"), px + py, max_iter=MAX_ITER), DeviceBP(code.csr("hx"), pz + py, max_iter=MAX_ITER)
        mc = DeviceMC(code, dx, dz)
        mc.set_osd(DeviceLSD(dx.graph, k), DeviceLSD(dz.graph, k))
    res = _launch(mc, seed, S, "Total")
    assert np.array_equal(res.err, sample_errors(code.N, *PROBS, seed, 0, S).cpu().numpy())
    fail, conv = _host_pipeline(oracle, code, res.err, k)
    assert np.array_equal(res.fail, fail[:, 0].astype(np.uint8) | (fail[:, 1].astype(np.uint8) << 1))
    assert res.shots == S and res.failures == int((fail[:, 0] | fail[:, 1]).sum())
    assert res.sector_fail == fail.sum(0).tolist() and res.sector_nonconv == (~conv).sum(0).tolist()
    assert sum(res.sector_nonconv) > 0 and 0 < res.failures < S


@pytest.mark.parametrize("direction", ["x->z", "z->x"])
def test_channel_update_with_two_bplsd_decoders(gpu, oracle, code, direction):
    k, S, seed = 2, 384, 61
    px, py, pz = PROBS
    p_first, p0, p1 = decoders.channel_update_probs(px, py, pz, direction)
    x_first = direction == "x->z"
    mk = lambda h, p, **kw: decoders.BPLSD_Decoder(h, p * np.ones(code.N), MAX_ITER, "minimum_sum", 0.625,  # noqa: E731
                                                   bits_per_step=k, **kw)
    side = dict(side_probs=(p0, p1))
    dx = mk(code.hz, px + py, **({} if x_first else side))
    dz = mk(code.hx, pz + py, **(side if x_first else {}))
    sim = simulators.CodeSimulator_DataError(code, dx, dz, list(PROBS), "Total", seed=seed, channel_update=direction)
    res = sim.fused_counts(S)
    err = sample_errors(code.N, *PROBS, seed, 0, S).cpu().numpy()
    bp = side_osd_ref.flooding_soft(oracle, MAX_ITER)
    stage = _host_lsd(k)

    def first(H, synd):
        Hd = H.to_dense().astype(np.uint8)
        c, it, cv, post = bp(Hd, p_first, synd)
        return stage(Hd, synd, post, cv, c), it, np.asarray(cv, bool)

    def second(H, synd, sb):
        Hd = H.to_dense().astype(np.uint8)
        c, it, cv, post = side_osd_ref.bp_side_soft(bp, Hd, p0, p1, synd, sb)
        return stage(Hd, synd, post, cv, c), it, cv

    comp = side_ref.compose(code, err, direction, first, second)
    assert res.shots == S and res.failures == int((comp["fail"][:, 0] | comp["fail"][:, 1]).sum())
    assert res.sector_iters == comp["iters"].sum(0).tolist() and res.sector_nonconv == (~comp["conv"]).sum(0).tolist()
    assert min(res.sector_nonconv) > 0
    f, shots, handed = sim.bposd_counts(128)
    assert shots == 128 and 0 <= f <= 128 and handed >= 0
    wer, _ = sim.WordErrorRate(128)
    assert 0.0 <= wer < 1.0


def test_phenon_with_a_bplsd_decoder2_runs_on_the_device_path(gpu, code):
    from qldpc_fault_tolerance_amd.decoders import BP_Decoder_Class, BPLSD_Decoder_Class
    from qldpc_fault_tolerance_amd.simulators import CodeSimulator_Phenon

    p, rounds, S = 0.02, 3, 600
    ext = lambda h: np.hstack([h, np.identity(h.shape[0])])  # noqa: E731
    b1 = BP_Decoder_Class(10, "minimum_sum", 0.625)
    d1 = {"p_data": p, "p_syndrome": p}

    def sim(dec2_cls):
        return CodeSimulator_Phenon(code, b1.GetDecoder({**d1, "h": ext(code.hz)}), b1.GetDecoder({**d1, "h": ext(code.hx)}),
                                    dec2_cls.GetDecoder({"h": code.hz, "p_data": p}),
                                    dec2_cls.GetDecoder({"h": code.hx, "p_data": p}), pauli_error_probs=[p / 2] * 3,
                                    q=p, eval_logical_type="Total", seed=31)

    s_lsd = sim(BPLSD_Decoder_Class(10, "minimum_sum", 0.625, bits_per_step=1))
    assert s_lsd._engine_parts() is not None
    assert all(isinstance(o, DeviceLSD) for o in s_lsd._final_osd())
    lsd, bp = s_lsd.fused_counts(rounds, S), sim(b1).fused_counts(rounds, S)
    assert lsd.shots == bp.shots == S and 0 <= lsd.failures <= bp.failures

"""The serial-schedule min-sum engine (engine 8, csrc/serial.hip) on the GPU: the kernel against the host
law (qldpc_serial_decode_host, pinned to the Python law by tests/test_serial_cpu.py) bit for bit, on
every path the kernel takes (messages in LDS or in the HBM workspace, 16-bit staged or global indices,
layers narrower and wider than the workgroup, columns kept in registers and past them), and the
loops that decode through a serial handle.
"""
import random

import numpy as np
import pytest

import serial_cases
from qldpc_fault_tolerance_amd import _native, codes, decoders, simulators
from qldpc_fault_tolerance_amd.codes import CSR
from qldpc_fault_tolerance_amd.engine import DeviceBP, DeviceMC, DeviceOSD, serial_decode_host

pytestmark = pytest.mark.gpu


def _code(name="hgp_34_n225"):
    return codes.get_code(name)


def _check(H, probs, max_iter, synd, precision, alpha=0.625):
    """A soft serial handle against the host law: corr, iters, conv through decode_batch, and the
    posteriors through decode_batch_soft."""
    dec = DeviceBP(H, probs, max_iter=max_iter, ms_scaling_factor=alpha, precision=precision, soft=True,
                   schedule="serial")
    geo = dec.geometry()
    assert geo["engine"] == 8 and dec.schedule == "serial"
    ref = serial_decode_host(H, probs, max_iter, synd, ms_scaling_factor=alpha, precision=precision)
    got = dec.decode_batch(synd)
    for k, (x, y) in enumerate(zip(got, ref[:3])):
        assert np.array_equal(x, y), ("corr", "iters", "conv")[k]
    soft = dec.decode_batch_soft(synd)
    for k, (x, y) in enumerate(zip(soft, ref)):
        assert np.array_equal(x, y), ("corr", "iters", "conv", "post")[k]
    return dec, geo, ref


def _staged(geo, H, precision):
    """Whether a soft handle's kernel is the variant with the index arrays in LDS, read off its LDS
    size: without them the image is the messages, the posteriors, two flags and the decision and
    syndrome bytes (plus alignment); the 16-bit copy adds more than 6 bytes per edge."""
    ts = precision // 8
    plain = H.nnz * ts + H.n * ts + 8 + H.n + H.m + 32
    assert geo["lds_bytes"] <= plain or geo["lds_bytes"] > plain + 4 * H.nnz
    return geo["lds_bytes"] > plain


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("max_iter", [1, 22])
@pytest.mark.parametrize("B", [1, 3, 700])
def test_n225_equals_host_law(gpu, B, max_iter, precision):
    H = _code().csr("hz")
    synd = serial_cases.syndromes(H, 0.05, B, np.random.default_rng(B), zero=B > 1)
    _, geo, ref = _check(H, 0.05, max_iter, synd, precision)
    # messages in LDS; at one wave per decode the 16-bit index copy would cost resident workgroups, so
    # this graph walks its indices in global memory (the small graphs below take the staged variant)
    assert geo["lds_bytes"] < 64 * 1024 and geo["threads"] == 64 and not _staged(geo, H, precision)
    if B == 700 and max_iter == 22:
        assert ref[2].any() and (~ref[2]).any()


@pytest.mark.parametrize("alpha", [0.625, 0.0])
@pytest.mark.parametrize("precision", [64, 32])
def test_irregular_graph_equals_host_law(gpu, precision, alpha):
    """Degree-1 row (sentinel), degree-12 row, degree-0 column, a degree-8 column (registers) and a
    degree-10 column (the recomputing path), non-uniform priors."""
    H = serial_cases.irregular()
    synd = serial_cases.syndromes(H, 0.08, 40, np.random.default_rng(3))
    synd[1, :] ^= 1
    _, geo, _ = _check(H, serial_cases.irregular_priors(H.n), 12, synd, precision, alpha)
    assert _staged(geo, H, precision)  # serial_kernel<T, uint16_t>


@pytest.mark.parametrize("precision", [64, 32])
def test_layers_wider_than_the_workgroup(gpu, precision):
    """H = I_300 (one layer of 300 > 256 threads) and a 257-variable chain (layers of 129 and 128)."""
    H = serial_cases.identity(300)
    synd = (np.random.default_rng(4).random((5, 300)) < 0.3).astype(np.uint8)
    _, geo, _ = _check(H, np.linspace(0.02, 0.6, 300), 3, synd, precision)
    assert geo["threads"] == 256 and _staged(geo, H, precision)
    H = serial_cases.chain(257)
    synd = serial_cases.syndromes(H, 0.1, 9, np.random.default_rng(5))
    _, geo, _ = _check(H, 0.08, 15, synd, precision)
    assert geo["threads"] == 256


@pytest.mark.parametrize("precision", [64, 32])
def test_space_time_graph_equals_host_law(gpu, precision):
    code = _code()
    H = codes.space_time_csr(code.hz, 2)
    m, n = code.hz.shape
    probs = np.hstack([0.02 * np.ones(n), 0.03 * np.ones(m)] * 2)
    synd = serial_cases.syndromes(H, 0.03, 48, np.random.default_rng(6))
    _, _, ref = _check(H, probs, 22, synd, precision)
    assert ref[2].any()


@pytest.mark.parametrize("precision", [64, 32])
def test_messages_in_the_hbm_workspace(gpu, monkeypatch, precision):
    H = _code().csr("hz")
    synd = serial_cases.syndromes(H, 0.05, 700, np.random.default_rng(8))
    lds = DeviceBP(H, 0.05, max_iter=22, precision=precision, soft=True, schedule="serial").geometry()["lds_bytes"]
    monkeypatch.setenv("QLDPC_SERIAL_WS", "1")
    _, geo, _ = _check(H, 0.05, 22, synd, precision)
    assert geo["lds_bytes"] <= lds - H.nnz * (precision // 8) + 16  # the E messages left LDS


@pytest.mark.parametrize("precision", [64, 32])
def test_indices_walked_in_global_memory(gpu, monkeypatch, precision):
    """A graph that stages its indices by default, with the switch that keeps them in global memory."""
    H = serial_cases.irregular()
    synd = serial_cases.syndromes(H, 0.08, 40, np.random.default_rng(9))
    monkeypatch.setenv("QLDPC_SERIAL_IDX", "0")
    _, geo, _ = _check(H, serial_cases.irregular_priors(H.n), 12, synd, precision)
    assert not _staged(geo, H, precision)  # serial_kernel<T, int32_t>


@pytest.mark.parametrize("precision", [64, 32])
def test_graph_past_the_16_bit_index_range(gpu, precision):
    """n = 70,000, one or two checks per variable, 87,500 edges: 32-bit indices in global memory, the
    messages in the workspace."""
    n, m = 70000, 35000
    j = np.arange(n)
    rows = np.concatenate([j // 2, (j[::4] // 2 + 1) % m])
    cols = np.concatenate([j, j[::4]])
    order = np.lexsort((cols, rows))
    rp = np.zeros(m + 1, np.int64)
    np.add.at(rp, rows + 1, 1)
    H = CSR(m=m, n=n, row_ptr=np.cumsum(rp).astype(np.int32), col_idx=cols[order].astype(np.int32))
    assert H.nnz == 87500 and H.nnz > 0xffff
    synd = serial_cases.syndromes(H, 0.03, 2, np.random.default_rng(10), zero=False)
    dec = DeviceBP(H, 0.03, max_iter=6, precision=precision, schedule="serial")
    ref = serial_decode_host(H, 0.03, 6, synd, precision=precision)
    got = dec.decode_batch(synd)
    assert all(np.array_equal(x, y) for x, y in zip(got, ref[:3]))


def test_set_channel_probs_rebuilds_the_priors(gpu):
    H = _code().csr("hz")
    synd = serial_cases.syndromes(H, 0.05, 32, np.random.default_rng(12))
    p0 = 0.03 * np.ones(H.n)
    p1 = np.linspace(0.005, 0.12, H.n)
    dec = DeviceBP(H, p0, max_iter=22, schedule="serial")
    first = dec.decode_batch(synd)
    dec.set_channel_probs(p1)
    second = dec.decode_batch(synd)
    fresh = DeviceBP(H, p1, max_iter=22, schedule="serial").decode_batch(synd)
    assert all(np.array_equal(x, y) for x, y in zip(second, fresh))
    assert all(np.array_equal(x, y) for x, y in zip(second, serial_decode_host(H, p1, 22, synd)[:3]))
    assert not np.array_equal(first[0], second[0])


def test_no_soft_output_without_the_flag_and_no_osd(gpu):
    code = _code()
    H = code.csr("hz")
    dec = DeviceBP(H, 0.03, max_iter=22, schedule="serial")
    with pytest.raises(_native.QldpcError) as ei:
        dec.decode_batch_soft(np.zeros((2, H.m), np.uint8))
    assert ei.value.rc == _native.ENOTSUP
    dz = DeviceBP(code.csr("hx"), 0.03, max_iter=22, schedule="serial")
    mc = DeviceMC(code, dec, dz)
    with pytest.raises(_native.QldpcError) as ei:
        mc.set_osd(DeviceOSD(dec.graph, 0.03 * np.ones(H.n), "osd_e", 4), None)
    assert ei.value.rc == _native.ENOTSUP


# ------------------------------------------------------------------ shot loops
PX = PY = PZ = 0.04 / 3
PRIOR = 2 * 0.04 / 3


def _fail_flags(code, err, decode):
    """[H; L] check of sampled errors [S, n] (bit0 x, bit1 z) under ``decode(q, H, synd) -> corr``."""
    fail = np.zeros(err.shape[0], np.uint8)
    for q, (h, l) in enumerate((("hz", "lz"), ("hx", "lx"))):
        H, L = code.csr(h), code.csr(l)
        e = ((err >> q) & 1).astype(np.uint8)
        r = e ^ decode(q, H, H.matvec(e).astype(np.uint8)).astype(np.uint8)
        fail |= ((H.matvec(r).any(axis=1) | L.matvec(r).any(axis=1)).astype(np.uint8) << q)
    return fail


def test_data_error_shot_loop_takes_the_staged_route(gpu):
    code = _code()
    ones = PRIOR * np.ones(code.N)
    dx = decoders.BPDecoder(code.hz, ones, 22, "minimum_sum", 0.625, schedule="serial")
    dz = decoders.BPDecoder(code.hx, ones, 22, "minimum_sum", 0.625, schedule="serial")
    assert dx.schedule == "serial" and dx.decoder.geometry()["engine"] == 8
    sim = simulators.CodeSimulator_DataError(code, dx, dz, [PX, PY, PZ], "Total", seed=17)
    ok, bx, bz = sim._engine_ready()
    assert ok and bx is dx.decoder
    S = 300
    res = sim._device_mc(bx, bz).run(PX, PY, PZ, 17, 0, S, "Total", per_shot=True)
    fail = _fail_flags(code, res.err, lambda q, H, synd: serial_decode_host(H, PRIOR, 22, synd)[0])
    assert np.array_equal(res.fail, fail) and res.failures == int((fail != 0).sum())
    assert 0 < res.failures < S
    # the staged pipeline: the only one qldpc_mc_launch_weight runs on
    w = sim._mc.run_weight(9, PX, PY, PZ, 17, 1000, 64, "Total", per_shot=True)
    assert np.array_equal(w.fail, _fail_flags(code, w.err,
                                              lambda q, H, synd: serial_decode_host(H, PRIOR, 22, synd)[0]))
    wer, _ = sim.WordErrorRate(128)
    assert 0.0 <= wer < 1.0


def test_bposd_decode_batch_on_the_serial_schedule(gpu, oracle):
    code = _code()
    H = code.csr("hz")
    probs = 0.06 * np.ones(H.n)
    synd = serial_cases.syndromes(H, 0.06, 64, np.random.default_rng(13))
    ref = serial_decode_host(H, probs, 22, synd)
    want = ref[0].copy()
    bad = np.flatnonzero(~ref[2])
    assert 0 < bad.size < 64
    # oracle.osd_decode_batch is oracle.osd_decode step for step in C; the numpy original takes ~1.6 s
    # per syndrome, so it decodes the first three and the C restatement all of them
    want[bad] = oracle.osd_decode_batch(H, probs, synd[bad], ref[3][bad], "osd_e", 10)[1]
    for b in bad[:3]:
        assert np.array_equal(want[b], oracle.osd_decode(code.hz, probs, synd[b], ref[3][b], "osd_e", 10)[1])
    for use_gpu_osd in (True, False):
        d = decoders.BPOSD_Decoder(code.hz, probs, 22, "minimum_sum", 0.625, "osd_e", 10, use_gpu_osd=use_gpu_osd,
                                   schedule="serial")
        assert d.schedule == "serial" and d.decoder.geometry()["engine"] == 8
        out = d.decode_batch(synd)
        assert np.array_equal(d.bp_batch, ref[0])
        assert np.array_equal(d.conv_batch, ref[2]) and np.array_equal(d.iters_batch, ref[1])
        assert np.array_equal(out, want)


def test_serial_bposd_simulator_keeps_the_host_assisted_loop(gpu, oracle):
    code = _code()
    ones = PRIOR * np.ones(code.N)
    mk = lambda h: decoders.BPOSD_Decoder(h, ones, 22, "minimum_sum", 0.625, "osd_e", 10, schedule="serial")  # noqa: E731
    sim = simulators.CodeSimulator_DataError(code, mk(code.hz), mk(code.hx), [PX, PY, PZ], "Total", seed=23)
    assert sim._bposd_device_mc(True, True) is None
    fails, shots, osd_n = sim.bposd_counts(256, keep_shots=True)
    err, sf = sim.last_shots
    n_osd = [0]

    def decode(q, H, synd):
        corr, _, conv, post = serial_decode_host(H, PRIOR, 22, synd)
        bad = np.flatnonzero(~conv)
        if bad.size:  # (oracle.osd_decode in C: see test_bposd_decode_batch_on_the_serial_schedule)
            corr[bad] = oracle.osd_decode_batch(H, ones, synd[bad], post[bad], "osd_e", 10)[1]
        n_osd[0] += int(bad.size)
        return corr

    fail = _fail_flags(code, err, decode)
    assert shots == 256 and fails == int((fail != 0).sum()) and osd_n == n_osd[0] > 0
    assert np.array_equal(sf[:, 0], (fail & 1) != 0) and np.array_equal(sf[:, 1], (fail & 2) != 0)
    # the flooding pair still gets the device-resident loop
    flood = lambda h: decoders.BPOSD_Decoder(h, ones, 22, "minimum_sum", 0.625, "osd_e", 10)  # noqa: E731
    sim2 = simulators.CodeSimulator_DataError(code, flood(code.hz), flood(code.hx), [PX, PY, PZ], "Total", seed=23)
    assert sim2._bposd_device_mc(True, True) is not None


class _HostST:
    """ST_BP_Decoder_syndrome's contract on the host law; keeps the histories it was handed."""

    def __init__(self, h, p_data, p_synd, max_iter, num_rep):
        self.m, self.n = h.shape
        self.num_rep = num_rep
        self.H = codes.space_time_csr(h, num_rep)
        self.probs = np.hstack([p_data * np.ones(self.n), p_synd * np.ones(self.m)] * num_rep)
        self.max_iter = max_iter
        self.seen = []

    def decode(self, hist):
        hist = np.asarray(hist).astype(np.uint8)
        self.seen.append(hist.copy())
        corr = serial_decode_host(self.H, self.probs, self.max_iter, hist.reshape(1, -1))[0]
        return decoders.fold_space_time_correction(corr[0], self.n, self.m, self.num_rep)


class _HostFlood:
    """BPDecoder's contract on the oracle's flooding BP."""

    def __init__(self, oracle, H, p, max_iter):
        self.oracle, self.H, self.p, self.max_iter = oracle, H, p, max_iter
        self.seen = []

    def decode(self, synd):
        s = np.asarray(synd).astype(np.uint8).reshape(1, -1)
        self.seen.append(s[0].copy())
        return self.oracle.bp_decode_batch(self.H, self.p, self.max_iter, "minimum_sum", 0.625, s, 64)[0][0].astype(int)


def test_space_time_simulator_with_serial_round_decoders(gpu, oracle, monkeypatch):
    """decoder1 = ST_BP_Decoder_syndrome(schedule="serial") in the phenomenological space-time loop, fed
    external uniforms; the host replays the same draws through the simulator's own per-sample loop
    with the host law as decoder1.  Round r + 1's detector history holds round r's correction, so
    equal histories are equal corrections; the failure flags are compared the same way."""
    code = _code()
    p, rep, rounds, S, mi = 0.005, 2, 3, 64, 22  # (at p = 0.02 nearly every sample fails: no mix of flags)
    hz, hx = code.csr("hz"), code.csr("hx")
    st = lambda h: decoders.ST_BP_Decoder_syndrome(h, p, p, mi, "minimum_sum", 0.625, rep, schedule="serial")  # noqa: E731
    d2 = lambda h: decoders.BPDecoder(h, p * np.ones(code.N), mi, "minimum_sum", 0.625)  # noqa: E731
    sim = simulators.CodeSimulator_Phenon_SpaceTime(code, st(code.hz), st(code.hx), d2(code.hz), d2(code.hx),
                                                     [p / 2, p / 2, p / 2], p, "Total", num_rep=rep, seed=1)
    assert sim.decoder1_x.schedule == "serial" and sim.decoder1_x.space_decoder.geometry()["engine"] == 8
    parts = sim._engine_parts()
    assert parts is not None and parts[0] is sim.decoder1_x.space_decoder
    ph = sim._device_phenl(parts)
    U = np.random.default_rng(14).random((S, ph.uniforms_per_sample(rounds)))
    res = ph.run(p / 2, p / 2, p / 2, p, 0, 0, S, rounds, "Total", uniforms=U, per_shot=True)

    hx_host, hz_host = _HostST(code.hz, p, p, mi, rep), _HostST(code.hx, p, p, mi, rep)
    fx_host, fz_host = _HostFlood(oracle, hz, p, mi), _HostFlood(oracle, hx, p, mi)
    host = simulators.CodeSimulator_Phenon_SpaceTime(code, hx_host, hz_host, fx_host, fz_host, [p / 2, p / 2, p / 2], p,
                                                      "Total", num_rep=rep, seed=1)
    fails = []
    for s in range(S):
        draws = iter(U[s].tolist())
        monkeypatch.setattr(random, "random", lambda: next(draws))
        fails.append(int(host._single_run(rounds)))
    monkeypatch.undo()
    R1, mx, mz = rounds - 1, hx.m, hz.m
    assert mx == mz
    body = res.trace[:, :R1 * 2 * rep * mx].reshape(S, R1, 2, rep, mx)
    assert np.array_equal(body[:, :, 0].reshape(S * R1, rep, mx), np.stack(hz_host.seen))  # Z sector (hx)
    assert np.array_equal(body[:, :, 1].reshape(S * R1, rep, mz), np.stack(hx_host.seen))
    fin = res.trace[:, R1 * 2 * rep * mx:].reshape(S, 2, mx)
    assert np.array_equal(fin[:, 0], np.stack(fz_host.seen)) and np.array_equal(fin[:, 1], np.stack(fx_host.seen))
    assert np.array_equal((res.fail != 0).astype(int), np.array(fails))
    assert np.stack(hz_host.seen)[1::R1].any() and 0 < sum(fails) < S  # second-round histories are not all quiet

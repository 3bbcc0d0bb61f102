"""The single-shot circuit loop on the GPU (``qldpc_circ_create_single_shot``, csrc/circuit.hip;
``CodeSimulator_Circuit``, src/Simulators.py:386-671).  All bit-exact.

* Per sample: failure flags, sampled detector / observable bits and the decode counters == the NumPy
  restatement of ``_decoding_samples`` on the CPU oracle's decoders (``circuit_single_shot_ref``);
  the fixture tags also == the flags the REFERENCE's own ``_decoding_samples`` recorded
  (``tests/golden/reference_circuit_single_shot.npz``).  S = 1500 from sample 4242: a 28-sample tail
  word and a start that is no multiple of 64.  Every case is informative: both outcomes occur and at
  least 5 % of the samples carry a non-zero residual into some cycle.
* Batch and shard invariance; the per-sample plugin path == the fused path on the same draws;
  ``CodeFamily.EvalWER('circuit', ..)`` with the X, Z, X, .. alternation of the in-place swap; argument
  errors.
"""
import random

import numpy as np
import pytest

import circuit_single_shot_ref as ref

pytestmark = pytest.mark.gpu

S, B0 = ref.SAMPLES, ref.SHOT_BEGIN


def _sim(name, logical, ncyc, scales, p, osd=True, firstmin=False, max_iter=(6, 6), seed=ref.SEED, max_batch=0):
    from qldpc_fault_tolerance_amd.decoders import BPDecoder, BPOSD_Decoder, FirstMinBPDecoder
    from qldpc_fault_tolerance_amd.simulators import CodeSimulator_Circuit

    sim = CodeSimulator_Circuit(code=ref.make_code(name), p=p, num_cycles=ncyc, error_params=ref.error_params(scales, p),
                                eval_logical_type=logical, circuit_type="coloration", seed=seed, max_batch=max_batch)
    sim._generate_circuit()
    hx = sim.eval_code.hx
    m, n = hx.shape
    d1 = (FirstMinBPDecoder if firstmin else BPDecoder)(ref.ext(hx), ref.priors1(n, m, p), max_iter[0], "minimum_sum",
                                                        ref.ALPHA)
    if osd:
        d2 = BPOSD_Decoder(hx, p * np.ones(n), max_iter[1], "minimum_sum", ref.ALPHA, "osd_e", 10)
    else:
        d2 = BPDecoder(hx, p * np.ones(n), max_iter[1], "minimum_sum", ref.ALPHA)
    sim.decoder1_z, sim.decoder2_z = d1, d2
    return sim


def _restatement(sim, p, osd, firstmin=False, max_iter=(6, 6), shot_count=S, key=None):
    hx, lx = sim.eval_code.hx, sim.eval_code.lx
    m, n = hx.shape
    fn = lambda: ref.run(sim.dem, hx, lx, ref.priors1(n, m, p), p * np.ones(n), max_iter[0], max_iter[1],  # noqa: E731
                         sim.num_cycles, seed=sim.seed, shot_begin=B0, shot_count=shot_count, final_osd=osd,
                         firstmin=firstmin)
    return ref.cached_run(key, fn) if key is not None else fn()


def _check(res, want, sim, shots):
    D = sim.dem.num_detectors
    assert np.array_equal(res.detobs[:, :D], want["det"]) and np.array_equal(res.detobs[:, D:], want["logical"])
    assert np.array_equal(res.fail, want["fail"]), (int(res.fail.sum()), want["failures"])
    assert res.shots == shots and res.failures == want["failures"]
    assert res.sector_decodes == want["sector_decodes"]
    assert res.sector_iters == want["sector_iters"]
    assert res.sector_nonconv == want["sector_nonconv"]
    assert res.sector_fail[1] == want["failures"]
    # informative: both outcomes, and a carried residual in at least 5 % of the samples
    assert 0 < want["failures"] < shots and want["carried"] >= 0.05 * shots, (want["failures"], want["carried"])


# (id, code, logical, cycles, noise, OSD final, first-min decoder1, fixture tag)
CASES = [
    ("tor5_osd", "tor", "Z", 5, ref.ALL_NOISE, True, False, "tor_z5"),
    ("tor3_bp", "tor", "Z", 3, ref.ALL_NOISE, False, False, None),
    ("tor2_bp", "tor", "Z", 2, ref.ALL_NOISE, False, False, None),
    ("tor2_bp_cx", "tor", "Z", 2, ref.CX_ONLY, False, False, "tor_z2cx"),
    ("tor5_osd_cx", "tor", "Z", 5, ref.CX_ONLY, True, False, None),
    ("asym_x5_osd", "asym", "X", 5, ref.ALL_NOISE, True, False, "asym_x5"),
    ("asym_z5_osd", "asym", "Z", 5, ref.ALL_NOISE, True, False, None),
    ("tor5_firstmin", "tor", "Z", 5, ref.ALL_NOISE, True, True, None),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fused_loop_matches_restatement_per_sample(gpu, case):
    cid, name, logical, ncyc, scales, osd, fm, tag = case
    p = 3e-3
    sim = _sim(name, logical, ncyc, scales, p, osd=osd, firstmin=fm)
    assert sim._engine_parts() is not None
    if logical == "X":  # 6 check rows, 15 + 6 variables: the swapped sector
        assert sim.eval_code.hx.shape == (6, 15) and sim.decoder1_z.decoder.n == 21
    res = sim._device().run(sim.seed, B0, S, per_shot=True)
    want = _restatement(sim, p, osd, firstmin=fm, key=cid)
    _check(res, want, sim, S)
    if tag is not None:  # the reference's own _decoding_samples on the same draws
        z = np.load(ref.GOLDEN)
        D, K = sim.dem.num_detectors, sim.dem.num_observables
        assert np.array_equal(np.unpackbits(z[f"{tag}_samples"], axis=1)[:, :D + K], res.detobs)
        assert np.array_equal(z[f"{tag}_fail"], res.fail)


def test_fused_loop_n225_more_than_one_row_tile(gpu):
    """hgp_34_n225: m = 108 check rows (two row tiles of the step kernel, the second one partial, its
    logical rows behind the syndrome rows), 3 cycles, p = 2e-3, S = 320."""
    p, mi, n_s = 2e-3, (225 // 30, 225 // 10), 320
    sim = _sim("hgp_34_n225", "Z", 3, ref.ALL_NOISE, p, osd=True, max_iter=mi)
    assert sim.eval_code.hx.shape[0] == 108
    res = sim._device().run(sim.seed, B0, n_s, per_shot=True)
    want = _restatement(sim, p, True, max_iter=mi, shot_count=n_s)
    _check(res, want, sim, n_s)


def test_batch_and_shard_invariance(gpu):
    """One launch == 64-sample batches (max_batch = 64) == two launches split at an unaligned sample."""
    p = 3e-3
    one = _sim("tor", "Z", 5, ref.ALL_NOISE, p)._device().run(ref.SEED, B0, S, per_shot=True)
    small = _sim("tor", "Z", 5, ref.ALL_NOISE, p, max_batch=64)._device().run(ref.SEED, B0, S, per_shot=True)
    dev = _sim("tor", "Z", 5, ref.ALL_NOISE, p)._device()
    a, b = dev.run(ref.SEED, B0, 201, per_shot=True), dev.run(ref.SEED, B0 + 201, S - 201, per_shot=True)
    ab = a.merge(b)
    want = _restatement(_sim("tor", "Z", 5, ref.ALL_NOISE, p), p, True, key="tor5_osd")
    assert np.array_equal(one.fail, want["fail"])
    for got, fail in ((small, small.fail), (ab, np.concatenate([a.fail, b.fail]))):
        assert np.array_equal(fail, one.fail)
        assert (got.shots, got.failures) == (one.shots, one.failures)
        assert got.sector_decodes == one.sector_decodes and got.sector_iters == one.sector_iters
        assert got.sector_nonconv == one.sector_nonconv and got.sector_fail == one.sector_fail
        assert np.array_equal(got.iter_hist, one.iter_hist)
    assert np.array_equal(np.vstack([a.detobs, b.detobs]), one.detobs) and np.array_equal(small.detobs, one.detobs)


def test_plugin_path_equals_fused_path(gpu):
    """Foreign decoders (objects with ``.decode`` and ``.h``: the reference's plugin contract) run
    ``_decoding_samples`` per sample on GPU-sampled detectors: the same failures as the fused launch
    on the same draws.  A ``BPOSD_Decoder`` as decoder1 goes the plugin way too."""
    import oracle
    from qldpc_fault_tolerance_amd.decoders import BPOSD_Decoder

    p, n_s = 3e-3, 400
    sim = _sim("tor", "Z", 3, ref.ALL_NOISE, p, osd=False)
    hx = sim.eval_code.hx
    m, n = hx.shape
    fused = sim.fused_counts(n_s).failures

    class OracleBP:
        def __init__(self, h, probs):
            self.h, self.p = np.asarray(h, np.uint8), np.asarray(probs)

        def decode(self, synd):
            c, _, _ = oracle.bp_decode_batch(self.h, self.p, 6, "minimum_sum", ref.ALPHA,
                                             np.asarray(synd).reshape(1, -1).astype(np.uint8), 64)
            return c[0].astype(np.int64)

    d2 = sim.decoder2_z
    sim._shot_offset = 0  # the same draws again
    sim.decoder1_z, sim.decoder2_z = OracleBP(ref.ext(hx), ref.priors1(n, m, p)), OracleBP(hx, p * np.ones(n))
    assert sim._engine_parts() is None
    assert sim._batch_failures(n_s) == fused
    assert 0 < fused < n_s
    sim.decoder1_z = BPOSD_Decoder(ref.ext(hx), ref.priors1(n, m, p), 6, "minimum_sum", ref.ALPHA, "osd_e", 10)
    sim.decoder2_z = d2
    assert sim._engine_parts() is None


def _family(ratio):
    from qldpc_fault_tolerance_amd.decoders import BP_Decoder_Class, BPOSD_Decoder_Class

    return (BP_Decoder_Class(ratio, "minimum_sum", ref.ALPHA),
            BPOSD_Decoder_Class(ratio, "minimum_sum", ref.ALPHA, "osd_e", 10))


def _expected_failures(code, logical, p, ncyc, ratio, dsr, scales, seed, n_s):
    """The restatement's failure count of one CodeSimulator_Circuit run as EvalWER sets it up, on
    `code` as the previous run left it (the X run swaps it in place)."""
    from qldpc_fault_tolerance_amd.simulators import CodeSimulator_Circuit

    sim = CodeSimulator_Circuit(code=code, p=p, num_cycles=ncyc, error_params=ref.error_params(scales, p),
                                eval_logical_type=logical)
    sim._generate_circuit()
    hx, lx = sim.eval_code.hx, sim.eval_code.lx
    m, n = hx.shape
    mi = int(n / ratio)
    p1 = np.hstack([dsr * p * np.ones(n), p * np.ones(m)])
    out = ref.run(sim.dem, hx, lx, p1, p * np.ones(n), mi, mi, ncyc, seed=seed, shot_begin=0, shot_count=n_s)
    return out["failures"]


def test_codefamily_evalwer_circuit(gpu):
    """``CodeFamily.EvalWER('circuit', ..)`` (src/Simulators.py:815-870): 'Z' and 'Total' == the WER
    formula on the restatement's counts; 'X' with two points on `asym` evaluates X, then Z (the
    constructor swaps the passed code in place).  Each simulator draws its seed from ``random``."""
    from qldpc_fault_tolerance_amd.simulators import CodeFamily, word_error_rate_phenl

    ncyc, ratio, dsr, n_s = 3, 3, 2.0, 600
    scales = dict(ref.ALL_NOISE)

    def seeds(k):
        random.seed(2024)
        s = [random.getrandbits(64) for _ in range(k)]
        random.seed(2024)
        return s

    d1c, d2c = _family(ratio)
    # 'Z' on tor, two points
    ps = [3e-3, 4e-3]
    sd = seeds(2)
    got = CodeFamily([ref.make_code("tor")], d1c, d2c).EvalWER("circuit", "Z", ps, n_s, num_cycles=ncyc,
                                                              data_synd_noise_ratio=dsr, circuit_error_params=scales,
                                                              if_plot=False)
    tor = ref.make_code("tor")
    fails = [_expected_failures(tor, "Z", p, ncyc, ratio, dsr, scales, s, n_s) for p, s in zip(ps, sd)]
    assert all(0 < f < n_s for f in fails)
    assert got.shape == (1, 2)
    assert list(got[0]) == [word_error_rate_phenl(f, n_s, 2, ncyc) for f in fails]
    # 'Total' on asym: the Z run, then the X run
    sd = seeds(2)
    got = CodeFamily([ref.make_code("asym")], d1c, d2c).EvalWER("circuit", "Total", [3e-3], n_s, num_cycles=ncyc,
                                                               data_synd_noise_ratio=dsr, circuit_error_params=scales,
                                                               if_plot=False)
    asym = ref.make_code("asym")
    fz = _expected_failures(asym, "Z", 3e-3, ncyc, ratio, dsr, scales, sd[0], n_s)
    fx = _expected_failures(asym, "X", 3e-3, ncyc, ratio, dsr, scales, sd[1], n_s)
    assert 0 < fz < n_s and 0 < fx < n_s and fz != fx
    assert got[0, 0] == word_error_rate_phenl(fz, n_s, 1, ncyc) + word_error_rate_phenl(fx, n_s, 1, ncyc)
    # 'X' on asym, two points: X, then (swapped back) Z
    sd = seeds(2)
    code = ref.make_code("asym")
    hx0 = code.hx.copy()
    got = CodeFamily([code], d1c, d2c).EvalWER("circuit", "X", ps, n_s, num_cycles=ncyc, data_synd_noise_ratio=dsr,
                                               circuit_error_params=scales, if_plot=False)
    assert np.array_equal(code.hx, hx0)  # swapped twice
    asym = ref.make_code("asym")
    f0 = _expected_failures(asym, "X", ps[0], ncyc, ratio, dsr, scales, sd[0], n_s)
    assert asym.hx.shape == (6, 15)
    f1 = _expected_failures(asym, "X", ps[1], ncyc, ratio, dsr, scales, sd[1], n_s)  # swaps back: the Z sector
    assert asym.hx.shape == (9, 15)
    assert list(got[0]) == [word_error_rate_phenl(f0, n_s, 1, ncyc), word_error_rate_phenl(f1, n_s, 1, ncyc)]
    # and that second point is NOT what an X evaluation at ps[1] gives
    fx1 = _expected_failures(ref.make_code("asym"), "X", ps[1], ncyc, ratio, dsr, scales, sd[1], n_s)
    assert fx1 != f1


def test_argument_errors(gpu):
    from qldpc_fault_tolerance_amd import _native
    from qldpc_fault_tolerance_amd.engine import DeviceCircuit, DeviceCircuitSingleShot, DeviceFirstMin

    p = 3e-3
    sim = _sim("tor", "Z", 3, ref.ALL_NOISE, p, osd=False)
    hx, lx = sim.eval_code.hx, sim.eval_code.lx
    m, n = hx.shape
    b1, b2 = sim.decoder1_z.decoder, sim.decoder2_z.decoder
    with pytest.raises(_native.QldpcError) as e:  # 3 * m detectors, 4 cycles asked
        DeviceCircuitSingleShot(sim.dem, b1, hx, lx, b2, 4)
    assert e.value.rc == -1
    with pytest.raises(_native.QldpcError) as e:
        DeviceCircuitSingleShot(sim.dem, b1, hx, lx, b2, 1)
    assert e.value.rc == -1
    with pytest.raises(_native.QldpcError) as e:  # decoder1 on hx instead of [hx | I]
        DeviceCircuitSingleShot(sim.dem, b2, hx, lx, b2, 3)
    assert e.value.rc == -1
    fm = DeviceFirstMin(ref.ext(hx), ref.priors1(n, m, p), 6)
    # first-min rounds on a space-time handle
    pad = np.zeros((m, m), np.uint8)
    st = DeviceCircuit(sim.dem, b1, np.hstack([hx, pad]), np.hstack([lx, pad[:lx.shape[0]]]), b2, lx, num_rounds=2,
                       num_rep=1)
    assert _native.lib().qldpc_circ_set_round_firstmin(st.handle, fm.handle) == -1
    assert st.run(ref.SEED, 0, 64).shots == 64  # the space-time handle itself is fine
    # a first-min handle on another graph than decoder1's; no decoder1 and no first-min handle
    dev = DeviceCircuitSingleShot(sim.dem, None, hx, lx, b2, 3)
    cnt = dev.new_counters()
    with pytest.raises(_native.QldpcError) as e:
        dev.launch(ref.SEED, 0, 64, cnt)
    assert e.value.rc == -1
    other = DeviceFirstMin(np.hstack([np.identity(m, dtype=np.uint8), hx]), ref.priors1(n, m, p)[::-1].copy(), 6)
    with pytest.raises(_native.QldpcError) as e:
        dev.set_round_firstmin(other)
    assert e.value.rc == -1
    dev.set_round_firstmin(fm)
    assert dev.run(ref.SEED, 0, 64).shots == 64

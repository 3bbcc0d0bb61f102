"""GPU tests of fixed-weight error sampling (csrc/weight.hip) and the pipeline behind it.

The per-shot oracle of a fixed-weight batch: the sampling law in Python (tests/weight_ref.py), encoded
as uniforms of the reference's three-way split, through ``oracle.mc_run(uniforms=...)`` with the
decoders' priors.  ``qldpc_mc_launch_weight`` must equal it in errors, corrections, iteration counts,
failure flags and every counter.
"""
import numpy as np
import pytest

import weight_ref
from qldpc_fault_tolerance_amd import _native, codes, decoders, simulators
from qldpc_fault_tolerance_amd.engine import DeviceBP, DeviceMC, sample_errors_weight

pytestmark = pytest.mark.gpu

SHAPES = [(1, 0), (1, 1), (63, 63), (64, 1), (65, 64), (225, 0), (225, 1), (225, 60), (225, 224), (225, 225),
          (1600, 16)]
RATIOS = [(1.0, 1.0, 1.0), (1.0, 0.0, 0.0), (0.01, 0.002, 0.03)]
S0 = 2 ** 32 - 64
PX = PY = PZ = 0.02
PRIOR = 0.04  # px + py = pz + py
EINVAL, ENOTSUP = -1, -4

_cache = {}


def _code(name="hgp_34_n225"):
    if name not in _cache:
        _cache[name] = codes.get_code(name)
    return _cache[name]


def _ref(oracle, w, seed, begin, S, mode="Total", precision=64, method="minimum_sum", max_iter=22,
         name="hgp_34_n225"):
    """(errors, uniforms, oracle result) of a fixed-weight batch, computed once per argument set."""
    key = (w, seed, begin, S, mode, precision, method, max_iter, name)
    if key not in _cache:
        code = _code(name)
        e = weight_ref.ref_errors(oracle, code.N, w, PX, PY, PZ, seed, begin, S)
        U = weight_ref.to_uniforms(e, PX, PY, PZ)
        r = oracle.mc_run(code, PX, PY, PZ, seed=0, shot_begin=0, shot_count=S, logical_mode=mode, max_iter=max_iter,
                          bp_method=method, precision=precision, probs_x=PRIOR, probs_z=PRIOR, uniforms=U,
                          per_shot=True)
        for a in (e, *[v for v in r.values() if isinstance(v, np.ndarray)]):  # (torch wants U writable)
            a.setflags(write=False)
        _cache[key] = (e, U, r)
    return _cache[key]


def _decoders(precision=64, method="minimum_sum", max_iter=22, name="hgp_34_n225", sectors="xz"):
    code = _code(name)
    ones = PRIOR * np.ones(code.N)
    dx = DeviceBP(code.hz, ones, max_iter=max_iter, bp_method=method, precision=precision) if "x" in sectors else None
    dz = DeviceBP(code.hx, ones, max_iter=max_iter, bp_method=method, precision=precision) if "z" in sectors else None
    return code, dx, dz


def _same(res, e, ref, mode="Total"):
    need = {"Total": [0, 1], "X": [0], "Z": [1]}[mode]
    assert np.array_equal(res.err, e)
    assert np.array_equal(res.err, ref["err"])  # the uniforms encode the law's errors
    assert np.array_equal(res.fail, ref["fail"])
    hb = _native.HIST_BINS
    for q in (0, 1):
        if q in need:
            assert np.array_equal(res.corr[:, q], ref["corr"][:, q])
            assert np.array_equal(res.iters[:, q], ref["iters"][:, q])
            hist = np.bincount(np.minimum(ref["iters"][:, q], hb - 1), minlength=hb)
        else:
            hist = np.zeros(hb, np.int64)
        assert np.array_equal(res.iter_hist[q], hist)
    assert res.shots == ref["shots"] and res.failures == ref["failures"]
    for k in ("sector_decodes", "sector_iters", "sector_nonconv", "sector_fail"):
        assert getattr(res, k) == ref[k], k


@pytest.mark.parametrize("ratio", RATIOS)
def test_device_sampler_equals_host(gpu, ratio):
    px, py, pz = ratio
    for n, w in SHAPES + [(4096, 5)]:  # 4096: the kernel's cap (64 KiB of LDS)
        S = 130 if n < 4096 else 70
        host = sample_errors_weight(n, w, px, py, pz, seed=77, shot_begin=S0, shot_count=S, host=True)
        dev = sample_errors_weight(n, w, px, py, pz, seed=77, shot_begin=S0, shot_count=S).cpu().numpy()
        assert np.array_equal(dev, host), (n, w)
        assert ((dev != 0).sum(axis=1) == w).all()


@pytest.mark.parametrize("precision", [64, 32])
def test_per_shot_parity_with_oracle(gpu, oracle, precision):
    code, dx, dz = _decoders(precision)
    mc = DeviceMC(code, dx, dz, staged=True)
    for w in (0, 1, 4, 8, 12, 30):
        e, _, ref = _ref(oracle, w, 7, 5000, 200, precision=precision)
        if w == 8:
            f = ref["fail"] != 0
            assert f.any() and not f.all()
        res = mc.run_weight(w, PX, PY, PZ, seed=7, shot_begin=5000, shot_count=200, logical_mode="Total",
                            per_shot=True)
        _same(res, e, ref)
        plain = mc.run_weight(w, PX, PY, PZ, seed=7, shot_begin=5000, shot_count=200, logical_mode="Total")
        assert plain.failures == ref["failures"] and plain.fail is None


@pytest.mark.parametrize("mode", ["X", "Z"])
def test_single_sector_handles(gpu, oracle, mode):
    code, dx, dz = _decoders(sectors=mode.lower())
    mc = DeviceMC(code, dx, dz, staged=True)
    e, _, ref = _ref(oracle, 8, 7, 5000, 200, mode=mode)
    res = mc.run_weight(8, PX, PY, PZ, seed=7, shot_begin=5000, shot_count=200, logical_mode=mode, per_shot=True)
    _same(res, e, ref, mode)
    with pytest.raises(_native.QldpcError) as ei:  # the other sector has no decoder
        mc.run_weight(8, PX, PY, PZ, 7, 0, 10, "Total")
    assert ei.value.rc == EINVAL


def test_batching_and_split_invariance(gpu, oracle, monkeypatch):
    monkeypatch.setenv("QLDPC_STAGED_BATCH", "128")
    code, dx, dz = _decoders()
    mc = DeviceMC(code, dx, dz, staged=True)
    e, _, ref = _ref(oracle, 8, 9, 1000, 300)
    one = mc.run_weight(8, PX, PY, PZ, seed=9, shot_begin=1000, shot_count=300, logical_mode="Total", per_shot=True)
    _same(one, e, ref)
    a = mc.run_weight(8, PX, PY, PZ, seed=9, shot_begin=1000, shot_count=100, logical_mode="Total", per_shot=True)
    b = mc.run_weight(8, PX, PY, PZ, seed=9, shot_begin=1100, shot_count=200, logical_mode="Total", per_shot=True)
    for k in ("err", "fail", "corr", "iters"):
        assert np.array_equal(np.concatenate([getattr(a, k), getattr(b, k)]), getattr(one, k)), k
    both = a.merge(b)
    assert both.shots == one.shots and both.failures == one.failures
    for k in ("sector_decodes", "sector_iters", "sector_nonconv", "sector_fail"):
        assert getattr(both, k) == getattr(one, k)
    assert np.array_equal(both.iter_hist, one.iter_hist)


def test_product_sum_pair(gpu, oracle):
    code, dx, dz = _decoders(method="product_sum")
    mc = DeviceMC(code, dx, dz, staged=True)
    e, _, ref = _ref(oracle, 8, 3, 0, 128, method="product_sum")
    res = mc.run_weight(8, PX, PY, PZ, seed=3, shot_begin=0, shot_count=128, logical_mode="Total", per_shot=True)
    _same(res, e, ref)


def test_n1600(gpu, oracle):
    code, dx, dz = _decoders(max_iter=30, name="hgp_34_n1600")
    mc = DeviceMC(code, dx, dz, staged=True)
    for w in (16, 40):
        e, _, ref = _ref(oracle, w, 5, 2 ** 40, 128, max_iter=30, name="hgp_34_n1600")
        res = mc.run_weight(w, PX, PY, PZ, seed=5, shot_begin=2 ** 40, shot_count=128, logical_mode="Total",
                            per_shot=True)
        _same(res, e, ref)


def test_fused_path_agrees_on_the_same_errors(gpu, oracle):
    """The untouched fused kernels on the same errors (as uniforms) give the same verdicts."""
    code, dx, dz = _decoders()
    e, U, ref = _ref(oracle, 8, 7, 5000, 200)
    staged = DeviceMC(code, dx, dz, staged=True)
    fused = DeviceMC(code, dx, dz)
    with pytest.raises(_native.QldpcError) as ei:
        fused.run_weight(8, PX, PY, PZ, 7, 5000, 200, "Total")
    assert ei.value.rc == ENOTSUP
    a = staged.run_weight(8, PX, PY, PZ, seed=7, shot_begin=5000, shot_count=200, logical_mode="Total", per_shot=True)
    b = fused.run(PX, PY, PZ, seed=0, shot_begin=0, shot_count=200, logical_mode="Total", uniforms=U, per_shot=True)
    assert np.array_equal(a.err, b.err)
    assert np.array_equal(a.fail, b.fail) and np.array_equal(a.corr, b.corr)
    # a staged handle still runs the i.i.d. channel like any other handle
    c = staged.run(PX, PY, PZ, seed=0, shot_begin=0, shot_count=200, logical_mode="Total", uniforms=U, per_shot=True)
    assert np.array_equal(c.fail, b.fail) and np.array_equal(c.corr, b.corr) and np.array_equal(c.iters, b.iters)


def _sim(seed=21, cls=decoders.BPDecoder, extra=()):
    code = _code()
    ones = PRIOR * np.ones(code.N)
    dx = cls(code.hz, ones, 22, "minimum_sum", 0.625, *extra)
    dz = cls(code.hx, ones, 22, "minimum_sum", 0.625, *extra)
    return simulators.CodeSimulator_DataError(code, dx, dz, [PX, PY, PZ], "Total", seed=seed)


def test_failure_spectrum_and_stratified_wer(gpu, oracle):
    sim = _sim()
    weights = [2, 8, 12]
    fails, shots = sim.FailureSpectrum(weights, 256)
    assert list(shots) == [256] * 3
    assert list(fails) == [_ref(oracle, w, 21, i * 256, 256)[2]["failures"] for i, w in enumerate(weights)]
    assert sim._shot_offset == 3 * 256 and sim._mc is None
    wer, wer_eb = sim.WordErrorRate_Stratified(64, tail=1e-2)
    d = sim.last_spectrum
    code_n = sim.N
    lo, hi = simulators.stratified_window(code_n, 3 * PX, 1e-2)
    assert list(d["weights"]) == list(range(lo, hi + 1)) and list(d["shots"]) == [64] * (hi - lo + 1)
    assert sim._shot_offset == 3 * 256 + 64 * (hi - lo + 1)
    again = simulators.stratified_word_error_rate(3 * PX, code_n, sim.K, d["weights"], d["fails"], d["shots"])
    assert (wer, wer_eb) == (again["wer"], again["wer_eb"]) and 0.0 < wer < 1.0
    assert d["uncovered"] <= 1e-2
    # the first stratum of that run, against the oracle over the range the method documents
    assert d["fails"][0] == _ref(oracle, lo, 21, 3 * 256, 64)[2]["failures"]


def test_eval_wer_stratified(gpu):
    fam = simulators.CodeFamily([_code()], None, decoders.BP_Decoder_Class(10, "minimum_sum", 0.625))
    out = fam.EvalWER_Stratified("Total", [0.02, 0.04], 32, tail=1e-2)
    assert out.shape == (1, 2) and np.isfinite(out).all() and (out >= 0).all() and (out < 1).all()
    assert out[0, 0] < out[0, 1]


def test_error_paths(gpu):
    code, dx, dz = _decoders()
    mc = DeviceMC(code, dx, dz, staged=True)
    for args in ((-1, PX, PY, PZ), (code.N + 1, PX, PY, PZ), (3, 0.0, 0.0, 0.0), (3, -0.1, PY, PZ)):
        with pytest.raises(_native.QldpcError) as ei:
            mc.run_weight(*args, seed=1, shot_begin=0, shot_count=64, logical_mode="Total")
        assert ei.value.rc == EINVAL, args
    assert mc.run_weight(0, 0.0, 0.0, 0.0, seed=1, shot_begin=0, shot_count=64, logical_mode="Total").shots == 64
    with pytest.raises(_native.QldpcError) as ei:
        DeviceMC(code, dx, dz).run_weight(3, PX, PY, PZ, seed=1, shot_begin=0, shot_count=64, logical_mode="Total")
    assert ei.value.rc == ENOTSUP
    with pytest.raises(_native.QldpcError) as ei:  # past the sampler's cap
        sample_errors_weight(4097, 3, PX, PY, PZ, seed=1, shot_begin=0, shot_count=64)
    assert ei.value.rc == ENOTSUP
    with pytest.raises(TypeError):
        _sim(cls=decoders.BPOSD_Decoder, extra=("osd_e", 4)).FailureSpectrum([2], 64)

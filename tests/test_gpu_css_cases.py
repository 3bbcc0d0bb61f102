"""Every shot loop on CSS codes whose X and Z sectors differ (tests/css_cases.py), in both
orientations, bit for bit against the oracle on the same Philox stream: no tolerances anywhere.

What only unequal sectors reach: in ``qldpc_mc_create`` the common LDS image (larger m, larger V
slot count), the run-time row width when the sectors' row_chunks differ, the smaller degree-3 slot
count, the rows a smaller sector leaves unused, the per-shot class cache written in one sector's
pass and read in the other's (keyed by thread and variable slot: it serves asym15, asym112 and
asym230, whose sectors' slot maps are both the identity, and must stay off on the column-permuted
asym112p and asym230p, whose maps differ); in the phenomenological loop the m_x hx-row flips before the m_z
hz-row flips, the Z block before the X block in the trace, the shared syndrome buffer; the
per-sector capture buffers of the BP+OSD stages.  The path every pair takes (one fused kernel or
the staged pipeline) is asserted per case: sectors that plan onto different geometries or engines
(tanner_code1) run staged instead of being refused.
"""
import numpy as np
import pytest

import css_cases as cc
import weight_ref
from bposd_ref import oracle_sector_fails
from qldpc_fault_tolerance_amd import _native, codes, decoders, simulators
from qldpc_fault_tolerance_amd.engine import DeviceBP, DeviceFirstMin, DeviceMC, DeviceOSD, DevicePhenl

pytestmark = pytest.mark.gpu

ENOTSUP = -4  # QLDPC_ENOTSUP (include/qldpc_hip.h)
MI = cc.MAX_ITER
S = cc.MC_SHOTS
COUNTERS = ("shots", "failures", "sector_decodes", "sector_iters", "sector_nonconv", "sector_fail")
ORIENT = pytest.mark.parametrize("swapped", cc.ORIENTATIONS, ids=["asis", "swapped"])
PREC = pytest.mark.parametrize("precision", cc.PRECISIONS)

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cache():
    """The handles and oracle results the tests share live as long as this file's tests run."""
    yield
    _cache.clear()


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _priors(case_id, swapped):
    """(prior of the hz decoder, prior of the hx decoder) of the case's data-error channel."""
    px, py, pz = cc.pauli(case_id, swapped)
    return px + py, pz + py


def _decoders(case_id, swapped, precision, max_iter=MI):
    code = cc.code(case_id, swapped)
    qx, qz = _priors(case_id, swapped)
    return (DeviceBP(code.hz, qx, max_iter=max_iter, precision=precision),
            DeviceBP(code.hx, qz, max_iter=max_iter, precision=precision))


def _default_mc(case_id, swapped, precision):
    """The case's DeviceMC on default decoders (no vars_per_thread, no switches), built once."""
    def make():
        dx, dz = _decoders(case_id, swapped, precision)
        return DeviceMC(cc.code(case_id, swapped), dx, dz), dx, dz

    return _memo(("mc", case_id, swapped, precision), make)


def _mc_ref(oracle, case_id, swapped, precision, mode="Total", begin=cc.MC_SHOT0, shots=S, uniforms=None):
    """The oracle's per-shot run of the case, computed once per argument set (``uniforms``: a seed)."""
    def make():
        U = None if uniforms is None else _uniforms(uniforms, shots, cc.code(case_id, swapped).N)
        return _frozen(oracle.mc_run(cc.code(case_id, swapped), *cc.pauli(case_id, swapped), cc.MC_SEED, begin, shots,
                                     mode, max_iter=MI, precision=precision, uniforms=U, per_shot=True))

    return _memo(("ref", case_id, swapped, precision, mode, begin, shots, uniforms), make)


def _uniforms(seed, shots, width):
    return np.random.default_rng(seed).random((shots, width))


def _run(mc, case_id, swapped, mode="Total", begin=cc.MC_SHOT0, shots=S, uniforms=None):
    return mc.run(*cc.pauli(case_id, swapped), cc.MC_SEED, begin, shots, mode, uniforms=uniforms, per_shot=True)


def _path(mc):
    """``"staged"`` or ``"fused"``: switching channel update off succeeds on a staged handle only."""
    try:
        mc.set_channel_update(None)
    except _native.QldpcError as e:
        assert e.rc == ENOTSUP, e
        return "fused"
    return "staged"


def _same(res, ref, mode="Total"):
    """Per-shot arrays, counters and the iteration histogram of a DeviceMC run == the oracle's."""
    need = {"Total": [0, 1], "X": [0], "Z": [1]}[mode]
    assert np.array_equal(res.err, ref["err"])
    assert np.array_equal(res.fail, ref["fail"])
    for q in need:
        assert np.array_equal(res.corr[:, q], ref["corr"][:, q]), q
        assert np.array_equal(res.iters[:, q], ref["iters"][:, q]), q
    for k in COUNTERS:
        assert getattr(res, k) == ref[k], k
    for q in (0, 1):
        assert int(res.iter_hist[q].sum()) == res.sector_decodes[q] == (res.shots if q in need else 0)
        hb = _native.HIST_BINS
        hist = np.bincount(np.minimum(ref["iters"][:, q], hb - 1), minlength=hb) if q in need else np.zeros(hb, int)
        assert np.array_equal(res.iter_hist[q], hist), q


def _same_runs(a, b):
    for k in ("err", "fail", "corr", "iters"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for k in COUNTERS:
        assert getattr(a, k) == getattr(b, k), k
    assert np.array_equal(a.iter_hist, b.iter_hist)


# ------------------------------------------------------------------ 1. default decoders, every case
@ORIENT
@PREC
@pytest.mark.parametrize("case_id", cc.CASE_IDS)
def test_default_decoders_match_oracle_on_the_frozen_path(gpu, oracle, case_id, precision, swapped):
    mc, dx, dz = _default_mc(case_id, swapped, precision)
    for dec, plan in zip((dx, dz), cc.plans(case_id, precision, swapped)):
        g = dec.geometry()
        assert tuple(g[k] for k in cc.PLAN_KEYS) == plan, g
    assert _path(mc) == cc.CASES[case_id].path[precision, swapped]
    for mode in ("Total", "X", "Z"):
        _same(_run(mc, case_id, swapped, mode), _mc_ref(oracle, case_id, swapped, precision, mode), mode)


def test_fused_cases_are_the_ones_the_table_promises(gpu):
    """At least three fused cases whose sectors differ in m, one in row_chunks, one in degree3_slots,
    read off the handles the first test ran."""
    seen = {"m": set(), "row_chunks": set(), "degree3_slots": set()}
    for cid in cc.FUSED_IDS:
        for precision in cc.PRECISIONS:
            mc, dx, dz = _default_mc(cid, False, precision)
            assert _path(mc) == "fused"
            gx, gz = dx.geometry(), dz.geometry()
            if dx.m != dz.m:
                seen["m"].add(cid)
            for k in ("row_chunks", "degree3_slots"):
                if gx[k] != gz[k]:
                    seen[k].add((cid, precision))
    assert len(seen["m"]) >= 3 and seen["row_chunks"] and seen["degree3_slots"], seen


# ------------------------------------------------- 2. stream and sharding invariants, fused cases
@ORIENT
@PREC
@pytest.mark.parametrize("case_id", cc.FUSED_IDS)
def test_fused_stream_and_sharding_invariants(gpu, oracle, case_id, precision, swapped):
    """Shots across the 2^32 boundary of the Philox counter (the high word, and the class cache
    across it), the same range as two launches cut at an unaligned shot, and external uniforms."""
    mc, _, _ = _default_mc(case_id, swapped, precision)
    assert _path(mc) == "fused"
    begin, cut = 2 ** 32 - 100, 217
    ref = _mc_ref(oracle, case_id, swapped, precision, begin=begin)
    assert not np.array_equal(ref["err"], _mc_ref(oracle, case_id, swapped, precision)["err"])
    one = _run(mc, case_id, swapped, begin=begin)
    _same(one, ref)
    a = _run(mc, case_id, swapped, begin=begin, shots=cut)
    b = _run(mc, case_id, swapped, begin=begin + cut, shots=S - cut)
    for k in ("err", "fail", "corr", "iters"):
        assert np.array_equal(np.concatenate([getattr(a, k), getattr(b, k)]), getattr(one, k)), k
    both = a.merge(b)
    for k in COUNTERS:
        assert getattr(both, k) == getattr(one, k), k
    assert np.array_equal(both.iter_hist, one.iter_hist)
    seed = 1000 + swapped
    U = _uniforms(seed, S, cc.code(case_id, swapped).N)
    _same(_run(mc, case_id, swapped, uniforms=U), _mc_ref(oracle, case_id, swapped, precision, uniforms=seed))


# -------------------------------------------------------- 3. forced engines and the staged pipeline
@pytest.mark.parametrize("env,engine,path", [("QLDPC_ENGINE=1", 1, "fused"), ("QLDPC_ENGINE=2", 2, "fused"),
                                             ("QLDPC_MC_STAGED=1", 3, "staged")])
@ORIENT
@PREC
@pytest.mark.parametrize("case_id", ["asym112", "asym230"])
def test_forced_engines_and_staged_pipeline_match_oracle_and_default(gpu, oracle, monkeypatch, case_id, precision,
                                                                     swapped, env, engine, path):
    default = _run(_default_mc(case_id, swapped, precision)[0], case_id, swapped)
    monkeypatch.setenv(*env.split("="))
    dx, dz = _decoders(case_id, swapped, precision)
    assert dx.geometry()["engine"] == dz.geometry()["engine"] == engine
    mc = DeviceMC(cc.code(case_id, swapped), dx, dz)
    assert _path(mc) == path
    res = _run(mc, case_id, swapped)
    _same(res, _mc_ref(oracle, case_id, swapped, precision))
    _same_runs(res, default)


@ORIENT
def test_staged_pipeline_in_chunks_copies_per_shot_outputs(gpu, oracle, monkeypatch, swapped):
    """600 shots in staged batches of 128: corr and iters of chunks that do not start at shot 0."""
    monkeypatch.setenv("QLDPC_STAGED_BATCH", "128")
    monkeypatch.setenv("QLDPC_MC_STAGED", "1")
    dx, dz = _decoders("asym230", swapped, 64)
    mc = DeviceMC(cc.code("asym230", swapped), dx, dz)
    assert _path(mc) == "staged"
    _same(_run(mc, "asym230", swapped), _mc_ref(oracle, "asym230", swapped, 64))


# ------------------------------------------------------------------------- 4. fixed-weight loop
WEIGHTS = {"asym230": 6, "tanner_code1": 9}
W_SEED, W_BEGIN, W_SHOTS = 7, 5000, 200


def _weight_ref(oracle, case_id, swapped, mode, precision=64):
    """(errors of the sampling law in Python, the oracle's decode of them) of a fixed-weight batch."""
    def make():
        code = cc.code(case_id, swapped)
        px, py, pz = cc.pauli(case_id, swapped)
        qx, qz = _priors(case_id, swapped)
        e = _memo(("werr", case_id, swapped), lambda: weight_ref.ref_errors(
            oracle, code.N, WEIGHTS[case_id], px, py, pz, W_SEED, W_BEGIN, W_SHOTS))
        r = oracle.mc_run(code, px, py, pz, seed=0, shot_begin=0, shot_count=W_SHOTS, logical_mode=mode, max_iter=MI,
                          precision=precision, probs_x=qx, probs_z=qz, uniforms=weight_ref.to_uniforms(e, px, py, pz),
                          per_shot=True)
        return e, _frozen(r)

    return _memo(("wref", case_id, swapped, mode, precision), make)


@ORIENT
@pytest.mark.parametrize("case_id", list(WEIGHTS))
def test_fixed_weight_loop_matches_sampler_and_oracle(gpu, oracle, case_id, swapped):
    dx, dz = _decoders(case_id, swapped, 64)
    mc = DeviceMC(cc.code(case_id, swapped), dx, dz, staged=True)
    px, py, pz = cc.pauli(case_id, swapped)
    for mode in ("Total", "X", "Z"):
        e, ref = _weight_ref(oracle, case_id, swapped, mode)
        if mode == "Total":
            assert ((e != 0).sum(1) == WEIGHTS[case_id]).all()
            for bit in (1, 2):  # each sector fails on some shots and not on others
                f = (ref["fail"] & bit) != 0
                assert f.any() and not f.all(), bit
        res = mc.run_weight(WEIGHTS[case_id], px, py, pz, W_SEED, W_BEGIN, W_SHOTS, mode, per_shot=True)
        assert np.array_equal(res.err, e)
        _same(res, ref, mode)


# ------------------------------------------------------------------------- 5. BP+OSD device loop
def _bposd_sim(case_id, swapped, precision, order=4, seed=160):
    code = cc.code(case_id, swapped)
    qx, qz = _priors(case_id, swapped)
    dx = decoders.BPOSD_Decoder(code.hz, qx * np.ones(code.N), MI, "minimum_sum", 0.625, "osd_e", order, precision=precision)
    dz = decoders.BPOSD_Decoder(code.hx, qz * np.ones(code.N), MI, "minimum_sum", 0.625, "osd_e", order, precision=precision)
    return simulators.CodeSimulator_DataError(code, dx, dz, list(cc.pauli(case_id, swapped)), "Total", seed=seed)


@ORIENT
@pytest.mark.parametrize("case_id", ["asym112", "asym230", "asym112p", "asym230p"])
def test_bposd_device_loop_matches_oracle_per_shot(gpu, oracle, case_id, swapped):
    code = cc.code(case_id, swapped)
    sim = _bposd_sim(case_id, swapped, 64)
    fails, shots, osd_n = sim.bposd_counts(160, keep_shots=True)
    assert {pl[0] for pl in cc.plans(case_id, 64, swapped)} == {3}
    assert sim._bposd_dev, "both sectors plan on engine 3: the device-resident loop must serve the pair"
    assert _path(sim._bposd_dev) == "fused"
    assert shots == 160 and osd_n >= 5
    err, sf = sim.last_shots
    ref = oracle_sector_fails(oracle, code, err, cc.CASES[case_id].p, MI, 4)  # px + py = pz + py = p
    # each sector sends decodes to its own OSD stage (which mends nearly all of the smaller sector's)
    assert min(sim.last_result.sector_nonconv) >= 3 and ref.any() and not ref.all()
    assert np.array_equal(sf, ref)
    assert fails == int((ref[:, 0] | ref[:, 1]).sum())
    # the capture buffers are per sector: the counters tell the sectors apart
    assert sim.last_result.sector_fail == [int(ref[:, 0].sum()), int(ref[:, 1].sum())]


def test_bposd_on_a_staged_pair_takes_the_host_assisted_loop(gpu, oracle):
    """tanner_code1 swapped, fp32: both sectors on engine 3 with the same threads and vars per thread
    but degree classes 6 and 4.  ``qldpc_mc_create`` hands the pair to the staged pipeline,
    ``qldpc_mc_set_osd`` refuses that handle, and ``bposd_counts`` keeps the host-assisted loop, with
    the oracle's verdicts."""
    code = cc.code("tanner_code1", True)
    sim = _bposd_sim("tanner_code1", True, 32)
    fails, shots, osd_n = sim.bposd_counts(160, batch=64, keep_shots=True)
    assert sim._bposd_dev is False
    assert shots == 160 and osd_n > 0
    # the pair that loop tried first: the Z sector on the X sector's vars per thread
    qx, qz = _priors("tanner_code1", True)
    dx = DeviceBP(code.hz, qx, max_iter=MI, precision=32)
    dz = DeviceBP(code.hx, qz, max_iter=MI, precision=32, vars_per_thread=dx.geometry()["vars_per_thread"])
    mc = DeviceMC(code, dx, dz)
    gx, gz = dx.geometry(), dz.geometry()
    assert (gx["engine"], gx["threads"], gx["vars_per_thread"]) == (gz["engine"], gz["threads"], gz["vars_per_thread"])
    assert _path(mc) == "staged"
    with pytest.raises(_native.QldpcError) as ei:
        mc.set_osd(sim.decoder_x.gpu_osd, sim.decoder_z.gpu_osd)
    assert ei.value.rc == ENOTSUP
    err, sf = sim.last_shots
    ref = oracle_sector_fails(oracle, code, err, _priors("tanner_code1", True), MI, 4, precision=32)
    assert np.array_equal(sf, ref)
    assert fails == int((ref[:, 0] | ref[:, 1]).sum())


# ------------------------------------------------------------------- 6. phenomenological loop
def _phenl(case_id, swapped, num_rep, precision, max_batch=0, soft2=False):
    code = cc.code(case_id, swapped)
    p, q = cc.CASES[case_id].phen
    n = code.N
    st = [DeviceBP(codes.space_time_csr(h, num_rep), np.hstack([p * np.ones(n), q * np.ones(h.shape[0])] * num_rep),
                   max_iter=MI, precision=precision) for h in (code.hz, code.hx)]
    d2 = [DeviceBP(h, p, max_iter=MI, precision=precision, soft=soft2) for h in (code.hz, code.hx)]
    return DevicePhenl(code, st[0], st[1], d2[0], d2[1], num_rep=num_rep, max_batch=max_batch)


def _phen_args(case_id, swapped, shots=cc.PHEN_SHOTS, rounds=cc.PHEN_ROUNDS):
    return (*cc.pauli(case_id, swapped, phen=True), cc.CASES[case_id].phen[1], cc.PHEN_SEED, cc.PHEN_SHOT0, shots, rounds)


def _phen_ref(oracle, case_id, swapped, num_rep, precision, mode="Total", **kw):
    p, q = cc.CASES[case_id].phen
    a = _phen_args(case_id, swapped)
    return oracle.phenl_run(cc.code(case_id, swapped), *a, num_rep, mode, p_data=p, p_synd=q, max_iter_st=MI,
                            max_iter_2=MI, precision=precision, per_shot=True, **kw)


def _same_phen(res, ref):
    assert np.array_equal(res.trace, ref["trace"])
    assert np.array_equal(res.fail, ref["fail"])
    for k in COUNTERS:
        assert getattr(res, k) == ref[k], k


@pytest.mark.parametrize("num_rep", cc.PHEN_REPS)
@ORIENT
@PREC
@pytest.mark.parametrize("case_id", cc.CASE_IDS)
def test_phenl_matches_oracle_with_both_trace_widths(gpu, oracle, case_id, precision, swapped, num_rep):
    code = cc.code(case_id, swapped)
    m_x, m_z = code.hx.shape[0], code.hz.shape[0]
    R = cc.PHEN_ROUNDS
    ph = _phenl(case_id, swapped, num_rep, precision)
    assert ph.trace_len(R) == (R - 1) * num_rep * (m_x + m_z) + m_x + m_z
    assert ph.uniforms_per_sample(R) == ((R - 1) * num_rep + 1) * (code.N + m_x + m_z)
    for mode in ("Total", "X", "Z"):
        res = ph.run(*_phen_args(case_id, swapped), mode, per_shot=True)
        ref = _phen_ref(oracle, case_id, swapped, num_rep, precision, mode)
        _same_phen(res, ref)
        if mode == "Total":
            total = res
            hz_, hx_, fz, fx = cc.split_trace(res.trace, R, num_rep, m_x, m_z)
            rz, rx, rfz, rfx = cc.split_trace(ref["trace"], R, num_rep, m_x, m_z)
            assert hz_.shape[2:] == (num_rep, m_x) and hx_.shape[2:] == (num_rep, m_z)  # Z block: hx rows
            assert hz_[:, 0].reshape(len(hz_), -1).shape[1] == num_rep * m_x
            assert hx_[:, 0].reshape(len(hx_), -1).shape[1] == num_rep * m_z
            for a, b in ((hz_, rz), (hx_, rx), (fz, rfz), (fx, rfx)):
                assert a.any() and np.array_equal(a, b)
    # the same run in chunks of 64 samples: identical per-sample outputs and counters
    chunked = _phenl(case_id, swapped, num_rep, precision, max_batch=64).run(*_phen_args(case_id, swapped), "Total",
                                                                            per_shot=True)
    assert np.array_equal(chunked.trace, total.trace) and np.array_equal(chunked.fail, total.fail)
    for k in COUNTERS:
        assert getattr(chunked, k) == getattr(total, k), k


@pytest.mark.parametrize("num_rep", [1, 2, 3])
@ORIENT
@pytest.mark.parametrize("case_id", ["asym15", "asym112"])
def test_phenl_first_round_equals_numpy_statement_of_the_reference(gpu, oracle, case_id, swapped, num_rep):
    """External uniforms, num_rounds = 2: the first num_rep * (m_x + m_z) trace bytes equal the numpy
    statement of the reference's noisy round (tests/css_cases.py), the whole run the oracle's."""
    code = cc.code(case_id, swapped)
    m_x, m_z, n = code.hx.shape[0], code.hz.shape[0], code.N
    shots, px, py, pz, q = 40, 0.05, 0.03, 0.08, 0.11
    U = _uniforms(100 * num_rep + swapped, shots, (num_rep + 1) * (n + m_x + m_z))
    st = [DeviceBP(codes.space_time_csr(h, num_rep), np.hstack([0.1 * np.ones(n), q * np.ones(h.shape[0])] * num_rep),
                   max_iter=3) for h in (code.hz, code.hx)]
    d2 = [DeviceBP(h, 0.1, max_iter=3) for h in (code.hz, code.hx)]
    ph = DevicePhenl(code, st[0], st[1], d2[0], d2[1], num_rep=num_rep)
    res = ph.run(px, py, pz, q, 0, 0, shots, 2, "Total", uniforms=U, per_shot=True)
    det_z, hist_x = cc.phen_noisy_round(code, U, px, py, pz, q, num_rep)
    assert np.array_equal(res.trace[:, :num_rep * (m_x + m_z)],
                          np.hstack([det_z.reshape(shots, -1), hist_x.reshape(shots, -1)]))
    ref = oracle.phenl_run(code, px, py, pz, q, 0, 0, shots, 2, num_rep, "Total", p_data=0.1, p_synd=q, max_iter_st=3,
                           max_iter_2=3, uniforms=U, per_shot=True)
    _same_phen(res, ref)


@ORIENT
def test_phenl_final_osd_per_sector(gpu, oracle, swapped):
    """``qldpc_phenl_set_final_osd`` with sectors of different sizes: per-sector capture buffers."""
    code = cc.code("asym112", swapped)
    p = cc.CASES["asym112"].phen[0]
    ph = _phenl("asym112", swapped, 2, 64, soft2=True)
    d2x, d2z = ph.decoders[2:]
    ph.set_final_osd(DeviceOSD(d2x.graph, np.full(code.N, p), "osd_e", 4),
                     DeviceOSD(d2z.graph, np.full(code.N, p), "osd_e", 4))
    res = ph.run(*_phen_args("asym112", swapped), "Total", per_shot=True)
    ref = _phen_ref(oracle, "asym112", swapped, 2, 64, osd_method="osd_e", osd_order=4)
    bp = _phen_ref(oracle, "asym112", swapped, 2, 64)
    assert ref["sector_fail"] != bp["sector_fail"]  # the OSD stage changes verdicts
    assert np.array_equal(res.trace, ref["trace"]) and np.array_equal(res.fail, ref["fail"])
    assert res.failures == ref["failures"] and res.sector_fail == ref["sector_fail"]


@ORIENT
def test_phenl_round_firstmin_per_sector(gpu, oracle, swapped):
    """``qldpc_phenl_set_round_firstmin`` with sectors of different sizes (num_rep = 1, [h | I])."""
    code = cc.code("asym112", swapped)
    p, q = cc.CASES["asym112"].phen
    n = code.N
    ext = [codes.space_time_csr(h, 1) for h in (code.hz, code.hx)]
    pri = [np.hstack([p * np.ones(n), q * np.ones(h.shape[0])]) for h in (code.hz, code.hx)]
    st = [DeviceBP(e, pr, max_iter=MI) for e, pr in zip(ext, pri)]
    fm = [DeviceFirstMin(e, pr, MI) for e, pr in zip(ext, pri)]
    d2 = [DeviceBP(h, p, max_iter=MI) for h in (code.hz, code.hx)]
    ph = DevicePhenl(code, st[0], st[1], d2[0], d2[1], num_rep=1)
    ph.set_round_firstmin(fm[0], fm[1])
    res = ph.run(*_phen_args("asym112", swapped), "Total", per_shot=True)
    ref = _phen_ref(oracle, "asym112", swapped, 1, 64, firstmin_max_iter=MI)
    bp = _phen_ref(oracle, "asym112", swapped, 1, 64)
    assert not np.array_equal(ref["trace"], bp["trace"])  # first-min corrects the rounds differently
    assert 0 < ref["sector_fail"][0] < cc.PHEN_SHOTS and 0 < ref["sector_fail"][1] < cc.PHEN_SHOTS
    assert np.array_equal(res.trace, ref["trace"]) and np.array_equal(res.fail, ref["fail"])
    for k in ("failures", "sector_fail", "sector_iters", "sector_nonconv"):
        assert list(np.atleast_1d(getattr(res, k))) == list(np.atleast_1d(ref[k])), k


@ORIENT
def test_phen_single_shot_simulator_on_unequal_sectors(gpu, oracle, swapped):
    """num_rep = 1 through ``CodeSimulator_Phenon`` (decoder1 on [h | I]) on asym112."""
    code = cc.code("asym112", swapped)
    p, q = cc.CASES["asym112"].phen
    cls = decoders.BP_Decoder_Class(max_iter_ratio=10, bp_method="minimum_sum", ms_scaling_factor=0.625)
    ext = lambda h: np.hstack([h, np.identity(h.shape[0])])  # noqa: E731
    sim = simulators.CodeSimulator_Phenon(
        code=code, decoder1_x=cls.GetDecoder({"h": ext(code.hz), "p_data": p, "p_syndrome": q}),
        decoder1_z=cls.GetDecoder({"h": ext(code.hx), "p_data": p, "p_syndrome": q}),
        decoder2_x=cls.GetDecoder({"h": code.hz, "p_data": p}), decoder2_z=cls.GetDecoder({"h": code.hx, "p_data": p}),
        pauli_error_probs=list(cc.pauli("asym112", swapped, phen=True)), q=q, eval_logical_type="Total", seed=2024)
    wer, none = sim.WordErrorRate(5, 700)
    ref = oracle.phenl_run(code, *cc.pauli("asym112", swapped, phen=True), q, 2024, 0, 700, 5, 1, "Total", p_data=p,
                           p_synd=q)
    assert none is None and 0 < ref["failures"] < 700
    assert wer == simulators.word_error_rate_phenl(ref["failures"], 700, code.K, 5)
    for k in ("sector_iters", "sector_nonconv", "sector_fail"):
        assert getattr(sim.last_result, k) == ref[k], k


# ----------------------------------------------------------------------------------- 7. drop-ins
DROPINS = [("tanner_code1", False, 32), ("tanner_code1", False, 64), ("asym230", True, 64)]


@pytest.mark.parametrize("case_id,swapped,precision", DROPINS)
def test_data_error_simulator_dropin(gpu, oracle, case_id, swapped, precision):
    """``CodeSimulator_DataError.WordErrorRate`` on default decoder classes == ``word_error_rate`` on
    the oracle's count (tanner_code1: sector decoders of different geometries and engines)."""
    code = cc.code(case_id, swapped)
    qx, qz = _priors(case_id, swapped)
    cls = decoders.BP_Decoder_Class(10, "minimum_sum", 0.625, precision=precision)
    sim = simulators.CodeSimulator_DataError(code, cls.GetDecoder({"h": code.hz, "p_data": qx}),
                                             cls.GetDecoder({"h": code.hx, "p_data": qz}),
                                             list(cc.pauli(case_id, swapped)), "Total", seed=99)
    wer = sim.WordErrorRate(2000)
    ref = oracle.mc_run(code, *cc.pauli(case_id, swapped), 99, 0, 2000, "Total", precision=precision)
    assert 0 < ref["failures"] < 2000
    assert wer == simulators.word_error_rate(ref["failures"], 2000, code.K)
    for k in COUNTERS:
        assert getattr(sim.last_result, k) == ref[k], k


@pytest.mark.parametrize("case_id,swapped,precision", DROPINS)
def test_space_time_simulator_dropin(gpu, oracle, case_id, swapped, precision):
    """``CodeSimulator_Phenon_SpaceTime.WordErrorRate`` == the per-cycle formula on the oracle's count."""
    code = cc.code(case_id, swapped)
    p, q = cc.CASES[case_id].phen
    c1 = decoders.ST_BP_Decoder_Class(10, "minimum_sum", 0.625, precision=precision)
    c2 = decoders.BP_Decoder_Class(10, "minimum_sum", 0.625, precision=precision)
    d1 = {"p_data": p, "p_syndrome": q, "num_rep": 3}
    sim = simulators.CodeSimulator_Phenon_SpaceTime(
        code=code, decoder1_x=c1.GetDecoder({**d1, "h": code.hz}), decoder1_z=c1.GetDecoder({**d1, "h": code.hx}),
        decoder2_x=c2.GetDecoder({"h": code.hz, "p_data": p}), decoder2_z=c2.GetDecoder({"h": code.hx, "p_data": p}),
        pauli_error_probs=list(cc.pauli(case_id, swapped, phen=True)), q=q, eval_logical_type="Total", num_rep=3,
        seed=99)
    wer, none = sim.WordErrorRate(num_cycles=7, num_samples=500)  # num_rounds = 3
    ref = oracle.phenl_run(code, *cc.pauli(case_id, swapped, phen=True), q, 99, 0, 500, 3, 3, "Total", p_data=p,
                           p_synd=p, precision=precision)  # (the factory's p_synd = p_data)
    assert none is None and 0 < ref["failures"] < 500
    assert wer == simulators.word_error_rate_per_cycle(ref["failures"], 500, code.K, 7)
    for k in COUNTERS:
        assert getattr(sim.last_result, k) == ref[k], k

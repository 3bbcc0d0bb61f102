"""The first-min loop kernels (csrc/firstmin.hip: one wave or one workgroup per syndrome) against the
reference loop (tests/firstmin_ref.py over the CPU oracle's one-iteration BP), bit for bit in
corrections and accepted steps, on the case table of tests/firstmin_cases.py: irregular graphs, empty
rows and columns, priors of exactly 0.5 and above it, sums that overflow, several syndromes per wave
and per workgroup in one launch, both sides of the natural kernel switch and of the creation envelope,
and the table's ``holes`` graph inside the single-shot circuit loop.

Which kernel ran is asserted through ``DeviceFirstMin.geometry()``, never assumed."""
from functools import lru_cache

import numpy as np
import pytest

import bp_cases as bc
import firstmin_cases as fc
import firstmin_ref
from qldpc_fault_tolerance_amd import _native
from qldpc_fault_tolerance_amd.engine import DeviceBP, DeviceFirstMin, plan_bp

pytestmark = pytest.mark.gpu

KERNELS = ("wave", "wg")


def _pick(monkeypatch, kernel):
    """The kernel a decode takes: ``wave`` is the default within m + n <= 8192, ``wg`` the hook."""
    monkeypatch.delenv("QLDPC_FM_WAVE", raising=False)
    if kernel == "wg":
        monkeypatch.setenv("QLDPC_FM_WAVE", "0")


@lru_cache(maxsize=None)
def _trace(case_id, kind, level, max_iter, alpha, precision, B):
    """The reference's trace on the case's mixed syndromes: computed once, shared by both kernels,
    never written to."""
    t = firstmin_ref.trace(fc.graph(case_id), fc.priors(case_id, kind, level), max_iter, alpha, precision,
                           fc.mixed(case_id, B))
    for a in t.values():
        a.setflags(write=False)
    return t


def _reference(*key):
    t = _trace(*key)
    return t["corr"], t["steps"]


def _assert_equal(fm, S, want, what):
    corr, steps = fm.decode_batch(S)
    bad = np.flatnonzero((corr != want[0]).any(axis=1) | (steps != want[1]))
    assert bad.size == 0, (what, bad[:8], steps[bad[:8]], want[1][bad[:8]])


# ------------------------------------------------------------------ every case x precision x kernel
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("precision", fc.PRECISIONS)
@pytest.mark.parametrize("case_id", fc.CASE_IDS)
def test_loop_kernels_match_reference_on_the_table(gpu, oracle, monkeypatch, case_id, precision, kernel):
    """301 mixed syndromes (ragged against the 4 waves of a workgroup), max_iter 0 / 1 / 12,
    ``nonuniform`` and ``half`` priors at every prior level of the case, alpha 0.625 and ldpc's 0
    schedule, and alpha 0.9 where degree-1 rows send SENTINEL * alpha."""
    c = fc.CASES[case_id]
    _pick(monkeypatch, kernel)
    H, S = fc.graph(case_id), fc.mixed(case_id)
    for level in c.levels:
        for kind in fc.PRIORS:
            for alpha in c.alphas:
                for mi in fc.MAX_ITERS:
                    fm = DeviceFirstMin(H, fc.priors(case_id, kind, level), mi, alpha, precision=precision)
                    g = fm.geometry()
                    assert g["wave"] == (kernel == "wave") and g["threads"] == 256 and g["grid"] >= 1
                    _assert_equal(fm, S, _reference(case_id, kind, level, mi, alpha, precision, fc.B_MIXED),
                                  (level, kind, alpha, mi))


@pytest.mark.parametrize("kernel", KERNELS)
def test_single_syndrome(gpu, oracle, monkeypatch, kernel):
    """B = 1: one workgroup whose other three waves have no syndrome."""
    _pick(monkeypatch, kernel)
    for case_id, kind, level in (("col1to12", "half", 0.3), ("holes", "half", 0.03)):
        want = _reference(case_id, kind, level, fc.MAX_ITER, 0.625, 64, fc.B_MIXED)
        pick = [int(np.flatnonzero(want[1] == v)[0]) for v in sorted(set(want[1].tolist()))]  # one of each step count
        fm = DeviceFirstMin(fc.graph(case_id), fc.priors(case_id, kind, level), fc.MAX_ITER, 0.625, precision=64)
        assert fm.geometry()["wave"] == (kernel == "wave")
        for b in pick:
            corr, steps = fm.decode_batch(fc.mixed(case_id)[b:b + 1])
            assert np.array_equal(corr[0], want[0][b]) and steps[0] == want[1][b], (case_id, b)


# -------------------------------------------------- several syndromes per wave / workgroup in a launch
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("precision", fc.PRECISIONS)
@pytest.mark.parametrize("case_id,classes", [("a_i", ("rejected", "stopped", "exhausted", "cleared")),
                                             ("holes", ("toggling", "exhausted"))])
def test_reuse_across_the_syndromes_of_one_launch(gpu, oracle, monkeypatch, case_id, classes, precision, kernel):
    """The workgroup kernel keeps ``grid`` workgroups resident and the wave kernel 16 ``grid`` waves:
    with B = 2 grid + 1 and B = 32 grid + 3 every workgroup / wave decodes a second syndrome (some a
    third) on the LDS arrays, correction and flags its first one left behind.  The syndromes cycle
    through the mixed set, shuffled, so rejected, stopped, exhausted and cleared decodes (``a_i``
    holds all four under ``half`` priors at 0.03; on ``holes``: toggling ones) follow each other."""
    _pick(monkeypatch, kernel)
    kind, level = "half", 0.03
    key = (case_id, kind, level, fc.MAX_ITER, 0.625, precision, fc.B_MIXED)
    held = firstmin_ref.classes_of(_trace(*key), fc.mixed(case_id), fc.MAX_ITER)
    assert all(held[k] >= fc.NEEDED for k in classes), held
    fm = DeviceFirstMin(fc.graph(case_id), fc.priors(case_id, kind, level), fc.MAX_ITER, 0.625, precision=precision)
    g = fm.geometry()
    assert g["wave"] == (kernel == "wave")
    B = 32 * g["grid"] + 3 if kernel == "wave" else 2 * g["grid"] + 1
    launched = min((B + 3) // 4, 4 * g["grid"]) * 4 if kernel == "wave" else min(B, g["grid"])
    assert B > 2 * launched  # every wave / workgroup takes a second syndrome, some a third
    print(f"{case_id} fp{precision} {kernel}: grid {g['grid']}, B {B}")
    S = fc.reuse_batch(case_id, B)
    # the loop is a function of the syndrome: the reference decodes the 301 distinct ones
    want = _reference(*key)
    index = {s.tobytes(): i for i, s in enumerate(fc.mixed(case_id))}
    src = np.array([index[s.tobytes()] for s in S])
    corr, steps = fm.decode_batch(S)
    bad = np.flatnonzero((corr != want[0][src]).any(axis=1) | (steps != want[1][src]))
    assert bad.size == 0, (bad[:8], steps[bad[:8]], want[1][src][bad[:8]])


# -------------------------------------------------------------------------- the natural kernel switch
@pytest.mark.parametrize("precision", fc.PRECISIONS)
@pytest.mark.parametrize("name", list(fc.SWITCH))
def test_natural_kernel_switch(gpu, oracle, monkeypatch, name, precision):
    """m + n = 8192: the wave kernel with exactly 64 KiB of LDS per workgroup; 8193: the workgroup
    kernel, with no environment hook set."""
    monkeypatch.delenv("QLDPC_FM_WAVE", raising=False)
    H = fc.graph(name)
    m, n = H.shape
    S = fc.mixed(name, fc.B_SWITCH)
    for kind, level in (("nonuniform", 0.03), ("half", 0.3)):
        fm = DeviceFirstMin(H, fc.priors(name, kind, level), fc.MAX_ITER, 0.625, precision=precision)
        g = fm.geometry()
        if name == "lds_8192":
            assert g["wave"] == 1 and g["lds_bytes"] == 64 * 1024
        else:
            assert g["wave"] == 0 and g["lds_bytes"] == 2 * (m + n) + fc.WG_STATIC_LDS
        assert g["wave"] == fc.takes_wave(m, n)
        _assert_equal(fm, S, _reference(name, kind, level, fc.MAX_ITER, 0.625, precision, fc.B_SWITCH), (kind, level))


# ------------------------------------------------------------------------------ the creation envelope
def test_largest_admitted_graph_decodes(gpu, oracle, monkeypatch):
    """m + n = 32760: 2 (m + n) + 16 bytes = 64 KiB exactly, the workgroup kernel's whole LDS."""
    monkeypatch.delenv("QLDPC_FM_WAVE", raising=False)
    csr = fc.envelope_graph("env_32760")
    assert fc.admitted(csr.m, csr.n) and not fc.admitted(csr.m, csr.n + 1)
    probs = np.full(csr.n, fc.ENVELOPE_P)
    fm = DeviceFirstMin(csr, probs, fc.ENVELOPE_MAX_ITER, 0.625)
    g = fm.geometry()
    assert g["wave"] == 0 and g["lds_bytes"] == 64 * 1024 and g["grid"] >= 1
    S = fc.envelope_syndromes("env_32760")
    want = firstmin_ref.decode(csr, probs, fc.ENVELOPE_MAX_ITER, 0.625, 64, S)
    assert want[0].any()
    _assert_equal(fm, S, want, "env_32760")


@pytest.mark.parametrize("precision", fc.PRECISIONS)
def test_past_the_envelope_creation_refuses(gpu, precision):
    """m + n = 32768: the arrays alone fit 64 KiB, the kernel's own 16 bytes do not."""
    csr = fc.envelope_graph("env_32768")
    assert 2 * (csr.m + csr.n) == fc.LDS_LIMIT and not fc.admitted(csr.m, csr.n)
    with pytest.raises(_native.QldpcError, match="first-min decoder") as e:
        DeviceFirstMin(csr, np.full(csr.n, fc.ENVELOPE_P), fc.ENVELOPE_MAX_ITER, 0.625, precision=precision)
    assert e.value.rc == _native.ENOTSUP


def test_one_iteration_bp_past_the_envelope_keeps_its_engine(gpu, oracle):
    """A ``max_iter = 1`` min-sum handle hands its decodes to the first-min one-iteration kernel where
    that can be built; at m + n = 32768 it cannot, and the handle decodes on the engine of its plan."""
    csr = fc.envelope_graph("env_32768")
    probs = np.full(csr.n, fc.ENVELOPE_P)
    dec = DeviceBP(csr, probs, max_iter=1)
    plan = plan_bp(csr, probs)
    assert dec.geometry()["engine"] == plan["engine"] and dec.geometry()["kernel_id"] == plan["kernel_id"]
    S = fc.envelope_syndromes("env_32768")
    c, i, v = dec.decode_batch(S)
    oc, oi, ov = oracle.bp_decode_batch(csr, probs, 1, "minimum_sum", 0.625, S, 64)
    assert oc.any()
    assert np.array_equal(c, oc.astype(np.int64)) and np.array_equal(i, oi) and np.array_equal(v, ov)


# -------------------------------------------------------------------------------- a consumer of the loop
def _holes_dem(hx, lx, cycles, p_data, p_check):
    """A synthetic single-shot DEM: per cycle, one mechanism per data bit (its column of hx in that
    cycle's detectors, its column of lx in the observables) and one per check (that cycle's detector
    and the next one's: a measurement error)."""
    from qldpc_fault_tolerance_amd.circuit import DetectorErrorModel

    m, n = hx.shape
    dem = DetectorErrorModel(num_detectors=cycles * m, num_observables=lx.shape[0])
    for c in range(cycles):
        for j in range(n):
            dem.probs.append(p_data)
            dem.dets.append([c * m + int(i) for i in np.flatnonzero(hx[:, j])])
            dem.obs.append([int(k) for k in np.flatnonzero(lx[:, j])])
        for i in range(m):
            dem.probs.append(p_check)
            dem.dets.append([c * m + i] + ([(c + 1) * m + i] if c + 1 < cycles else []))
            dem.obs.append([])
    return dem


def test_single_shot_circuit_loop_on_the_holes_graph(gpu, oracle):
    """The single-shot circuit loop with no decoder1 and a first-min handle on [hx | I], hx = the
    ``holes`` graph with its empty row and columns kept (the empty columns on the logical operators,
    column n - 1 at a prior of exactly 0.5), decoder1's priors at the table's upper level (0.15 to
    0.6: steps are rejected, stop early or run to max_iter): failure flags, sampled bits and the
    accepted steps counted as iterations equal the loop's restatement
    (tests/circuit_single_shot_ref.py), which takes any hx and lx: nothing in it needs a CSS pair."""
    import circuit_single_shot_ref as ref
    from qldpc_fault_tolerance_amd.engine import DeviceCircuitSingleShot

    hx = np.array(fc.graph("holes"))
    m, n = hx.shape
    assert not hx[m // 2].any() and not hx[:, [n // 2, n - 1]].any()
    lx = (np.random.default_rng(31).random((2, n)) < 0.1).astype(np.uint8)
    lx[0, n // 2] = lx[1, n - 1] = 1  # the empty columns are on the logical operators
    cycles, shots, begin, mi1, mi2 = 3, 200, 4243, 5, 8
    dem = _holes_dem(hx, lx, cycles, 0.02, 0.02)
    assert all(len(d) or len(o) for d, o in zip(dem.dets, dem.obs))  # no mechanism without an effect
    p1 = np.array(bc.priors_of(n + m, "nonuniform", 0.3))
    p1[n - 1] = 0.5
    p2 = np.full(n, 0.04)
    fm = DeviceFirstMin(ref.ext(hx), p1, mi1, ref.ALPHA)
    dec2 = DeviceBP(hx, p2, max_iter=mi2)
    dev = DeviceCircuitSingleShot(dem, None, hx, lx, dec2, cycles, firstmin=fm)
    res = dev.run(ref.SEED, begin, shots, per_shot=True)
    want = ref.run(dem, hx, lx, p1, p2, mi1, mi2, cycles, seed=ref.SEED, shot_begin=begin, shot_count=shots,
                   final_osd=False, firstmin=True)
    D = dem.num_detectors
    assert np.array_equal(res.detobs[:, :D], want["det"]) and np.array_equal(res.detobs[:, D:], want["logical"])
    assert np.array_equal(res.fail, want["fail"]), (int(res.fail.sum()), want["failures"])
    assert res.sector_iters == want["sector_iters"] and res.sector_decodes == want["sector_decodes"]
    assert res.sector_nonconv == want["sector_nonconv"]
    # informative: both outcomes, residuals carried, and decoder1 accepted steps but not always all of them
    assert 0 < want["failures"] < shots and want["carried"] >= 0.05 * shots
    assert 0 < want["sector_iters"][0] < mi1 * shots * (cycles - 1)

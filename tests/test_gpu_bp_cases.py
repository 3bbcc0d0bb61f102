"""Every general-purpose BP path on the irregular graphs of tests/bp_cases.py, bit-exact against the
oracle: corrections, iteration counts and convergence flags (and engine 1's posteriors) with
``np.array_equal``; product-sum posteriors under the <= 1 ulp rule of test_gpu_product_sum.py.

* the default route of every case (asserted first: ``geometry()`` equals the recorded route), which
  is the first time engine 6 is selected by column degree 9..12, engine 2's 8-slot kernels see real
  degree-7 / 8 columns, and engine 3's run-time-width check phase runs rows of 7, 8, 16, 17 and 32
  chunks;
* engine 6 forced onto every graph it takes, on both sides of its LDS-ballot switch;
* engine 1 (soft output) and engine 5 (product-sum, with soft output);
* max_iter = 1 on the first-min kernels, both sides of m = 64;
* batch edges and persistence: B = 1 / 65 / 333, lanes of engine 6 and workgroups of engines 5, 2
  and 3 that decode several syndromes in a row, new priors on a live handle.

Decoder handles and oracle results are cached per module and shared by the checks of a case.
"""
import numpy as np
import pytest

import bp_cases as bc
from qldpc_fault_tolerance_amd import _native

pytestmark = pytest.mark.gpu

PRECISIONS = [64, 32]
HBM_IDS = [c for c in bc.CASE_IDS if max(bc.graph(c).sum(axis=0).max(), bc.graph(c).sum(axis=1).max()) <= bc.HBM_MAX_DEG]
SOFT_IDS = [c for c in bc.CASE_IDS if bc.graph(c).sum(axis=0).max() <= bc.SOFT_MAX_COL]
NO_SOFT_IDS = [c for c in bc.CASE_IDS if c not in SOFT_IDS]

_DEC, _ORA = {}, {}


def _mid(case_id):
    lv = bc.CASES[case_id].levels
    return lv[len(lv) // 2 - 1]


def _decoder(case_id, precision, kind, level, alpha, max_iter=bc.MAX_ITER, **kw):
    from qldpc_fault_tolerance_amd.engine import DeviceBP

    key = (case_id, precision, kind, level, alpha, max_iter, tuple(sorted(kw.items())))
    if key not in _DEC:
        # the annealed V-slot placement of the fp64 engine-3 families is host work that only moves
        # bank conflicts (seconds on the 682-row graphs): the greedy placement decodes identically
        anneal = 0 if bc.CASES[case_id].n > 1000 else None
        _DEC[key] = DeviceBP(bc.graph(case_id), bc.priors(case_id, kind, level), max_iter=max_iter,
                             ms_scaling_factor=alpha, precision=precision, anneal_iters=anneal, **kw)
    return _DEC[key]


def _synd(case_id, what):
    return bc.syndromes(case_id, what[1]) if what[0] == "level" else bc.mixed(case_id, what[1])


def _oracle(oracle, case_id, precision, kind, level, alpha, what, method="minimum_sum", max_iter=bc.MAX_ITER):
    """(corr, iters, conv, post) of the oracle for the syndromes ``what`` = ("level", p) | ("mixed", B)."""
    key = (case_id, precision, kind, level, alpha, what, method, max_iter)
    if key not in _ORA:
        _ORA[key] = oracle.bp_decode_batch_soft(bc.graph(case_id), bc.priors(case_id, kind, level), max_iter, alpha,
                                                _synd(case_id, what), precision, bp_method=method)
    return _ORA[key]


def _same(got, want, ctx):
    corr, iters, conv = got[:3]
    assert np.array_equal(iters, want[1]), ctx
    assert np.array_equal(conv, want[2]), ctx
    assert np.array_equal(corr, want[0].astype(np.int64)), ctx


def _route(dec):
    g = dec.geometry()
    return g["engine"], g["kernel_id"], g["row_chunks"]


# ------------------------------------------------------------------------------- the default route
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case_id", bc.CASE_IDS)
def test_default_route_matches_oracle(gpu, oracle, case_id, precision):
    c = bc.CASES[case_id]
    runs = [(kind, _mid(case_id), alpha) for kind in bc.PRIORS for alpha in (bc.ALPHA, 0.0)]
    runs += [("nonuniform", lv, (bc.ALPHA, 0.0)[i % 2]) for i, lv in enumerate(c.levels) if lv != _mid(case_id)]
    for kind, level, alpha in runs:
        dec = _decoder(case_id, precision, kind, level, alpha)
        assert _route(dec) == c.route(precision, kind), (kind, level)
        what = ("level", level)
        _same(dec.decode_batch(_synd(case_id, what)), _oracle(oracle, case_id, precision, kind, level, alpha, what),
              (kind, level, alpha))


@pytest.mark.parametrize("name", list(bc.OVER_DEGREE))
def test_creation_refuses_what_the_plan_refuses(gpu, name):
    from qldpc_fault_tolerance_amd.engine import DeviceBP

    for kw in ({}, {"hbm": True}):
        with pytest.raises(_native.QldpcError, match="HBM engine: row or column degree above 12") as e:
            DeviceBP(bc.over_degree_graph(name), bc.P0, max_iter=5, **kw)
        assert e.value.rc == _native.ENOTSUP


# ---------------------------------------------------------------------------------- engine 6, forced
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case_id", HBM_IDS)
def test_forced_hbm_matches_oracle(gpu, oracle, case_id, precision):
    level = _mid(case_id)
    what = ("level", level)
    for kind, alpha in (("nonuniform", bc.ALPHA), ("half", 0.0), ("uniform", bc.ALPHA)):
        dec = _decoder(case_id, precision, kind, level, alpha, hbm=True)
        assert _route(dec)[0] == 6
        _same(dec.decode_batch(_synd(case_id, what)), _oracle(oracle, case_id, precision, kind, level, alpha, what),
              (kind, alpha))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_hbm_lds_ballot_switch(gpu, oracle, monkeypatch, precision):
    """682 x 1366 keeps its decisions and syndromes in LDS ballot words (n + m = 2048), 682 x 1367
    in HBM; the smaller one again with the ballot words switched off."""
    lo, hi = bc.CASES["xlds_2048"], bc.CASES["xlds_2049"]
    assert lo.n + lo.m == 2048 and hi.n + hi.m == 2049
    level = _mid("xlds_2048")
    what = ("level", level)
    dec = _decoder("xlds_2048", precision, "nonuniform", level, bc.ALPHA, hbm=True)
    want = _oracle(oracle, "xlds_2048", precision, "nonuniform", level, bc.ALPHA, what)
    monkeypatch.setenv("QLDPC_HBM_XLDS", "0")
    _same(dec.decode_batch(_synd("xlds_2048", what)), want, "XLDS=0")


@pytest.mark.parametrize("xlds", ["1", "0"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_hbm_edgeless_graph(gpu, oracle, monkeypatch, precision, xlds):
    """H = 0 (3 x 4) on engine 6: no message, one workspace line; every index of the kernel stays in
    its tables (rows and columns of degree 0).  The zero syndrome converges in the first iteration,
    every other one runs to max_iter; the decisions are the priors' (1 where p = 0.5)."""
    from qldpc_fault_tolerance_amd.engine import DeviceBP

    monkeypatch.setenv("QLDPC_HBM_XLDS", xlds)
    H = np.zeros((3, 4), np.uint8)
    probs = np.array([0.05, 0.5, 0.2, 0.01])
    S = ((np.arange(8)[:, None] >> np.arange(3)) & 1).astype(np.uint8)
    dec = DeviceBP(H, probs, max_iter=4, precision=precision, hbm=True)
    corr, iters, conv = dec.decode_batch(S)
    oc, oi, ov = oracle.bp_decode_batch(H, probs, 4, "minimum_sum", bc.ALPHA, S, precision)
    assert np.array_equal(corr, oc) and np.array_equal(iters, oi) and np.array_equal(conv, ov)
    assert conv.tolist() == [True] + [False] * 7 and iters.tolist() == [1] + [4] * 7


# ------------------------------------------------------------------------------ engine 1, soft output
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case_id", SOFT_IDS)
def test_soft_output_matches_oracle(gpu, oracle, case_id, precision):
    level = _mid(case_id)
    what = ("level", level)
    for kind, alpha in (("nonuniform", bc.ALPHA), ("half", 0.0)):
        dec = _decoder(case_id, precision, kind, level, alpha, soft=True)
        assert _route(dec)[0] == 1
        got = dec.decode_batch_soft(_synd(case_id, what))
        want = _oracle(oracle, case_id, precision, kind, level, alpha, what)
        _same(got, want, (kind, alpha))
        assert np.array_equal(got[3].view(np.int64), want[3].view(np.int64)), (kind, alpha)  # posteriors, bit for bit


@pytest.mark.parametrize("case_id", NO_SOFT_IDS)
def test_soft_output_refuses_column_degree_above_8(gpu, case_id):
    from qldpc_fault_tolerance_amd.engine import DeviceBP

    with pytest.raises(_native.QldpcError) as e:
        DeviceBP(bc.graph(case_id), bc.P0, max_iter=5, soft=True)
    assert e.value.rc == _native.ENOTSUP


# -------------------------------------------------------------------------------- engine 5, product-sum
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case_id", bc.CASE_IDS)
def test_product_sum_matches_oracle(gpu, oracle, case_id, precision):
    c = bc.CASES[case_id]
    for kind, level in [("nonuniform", lv) for lv in c.levels[:3]] + [("half", _mid(case_id)), ("uniform", _mid(case_id))]:
        what = ("level", level)
        dec = _decoder(case_id, precision, kind, level, 0.0, bp_method="product_sum")
        assert _route(dec)[0] == 5
        _same(dec.decode_batch(_synd(case_id, what)),
              _oracle(oracle, case_id, precision, kind, level, 0.0, what, method="product_sum"), (kind, level))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case_id", bc.CASE_IDS)
def test_product_sum_soft_output_matches_oracle(gpu, oracle, case_id, precision):
    level = _mid(case_id)
    what = ("level", level)
    dec = _decoder(case_id, precision, "nonuniform", level, 0.0, bp_method="product_sum", soft=True)
    assert _route(dec)[0] == 5
    got = dec.decode_batch_soft(_synd(case_id, what))
    want = _oracle(oracle, case_id, precision, "nonuniform", level, 0.0, what, method="product_sum")
    _same(got, want, case_id)
    post, op = got[3], want[3]
    fin = np.isfinite(op)
    assert np.array_equal(np.isfinite(post), fin)
    assert np.array_equal(post[~fin].view(np.int64), op[~fin].view(np.int64))
    ulp = np.abs(post[fin].view(np.int64) - op[fin].view(np.int64))
    assert ulp.size == 0 or ulp.max() <= 1, int(ulp.max())


# ---------------------------------------------------------------------------------------- max_iter = 1
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case_id", bc.CASE_IDS)
def test_one_iteration_matches_oracle_and_engine(gpu, oracle, monkeypatch, case_id, precision):
    """B = 300: the last 256-wide block of the thread-per-syndrome kernel (m <= 64) is ragged.  64 x 200
    runs it without LDS staging (256 (m + n) bytes > 64 KiB), 40 x 120 of test_gpu_parity.py with;
    65 x 200 is the first graph of the wave kernel."""
    from qldpc_fault_tolerance_amd.engine import DeviceBP

    c = bc.CASES[case_id]
    if case_id == "m64":
        assert c.m <= 64 and 256 * (c.m + c.n) > 64 * 1024
    if case_id == "m65":
        assert c.m > 64
    level = _mid(case_id)
    what = ("mixed", 300)
    S = _synd(case_id, what)
    for kind, alpha in (("nonuniform", bc.ALPHA), ("half", 0.0)):
        got = _decoder(case_id, precision, kind, level, alpha, max_iter=1).decode_batch(S)
        _same(got, _oracle(oracle, case_id, precision, kind, level, alpha, what, max_iter=1), (kind, alpha))
        monkeypatch.setenv("QLDPC_BP1", "0")  # read at creation: the engine's own kernels
        own = DeviceBP(bc.graph(case_id), bc.priors(case_id, kind, level), max_iter=1, ms_scaling_factor=alpha,
                       precision=precision, anneal_iters=0).decode_batch(S)
        monkeypatch.delenv("QLDPC_BP1")
        _same(own, (got[0], got[1], got[2]), (kind, alpha, "QLDPC_BP1=0"))


# ------------------------------------------------------------------------- batch and persistence edges


@pytest.mark.parametrize("B", [1, 65, 333])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("mode", ["engine2", "engine3", "engine6", "engine1", "engine5"])
def test_batch_edges(gpu, oracle, mode, precision, B):
    case_id, kw, method, alpha = {"engine2": ("col8", {}, "minimum_sum", bc.ALPHA),
                                  "engine3": ("row13", {}, "minimum_sum", bc.ALPHA),
                                  "engine6": ("col9", {}, "minimum_sum", bc.ALPHA),
                                  "engine1": ("col8", {"soft": True}, "minimum_sum", bc.ALPHA),
                                  "engine5": ("row13", {"bp_method": "product_sum"}, "product_sum", 0.0)}[mode]
    level = _mid(case_id)
    dec = _decoder(case_id, precision, "nonuniform", level, alpha, **kw)
    assert _route(dec)[0] == int(mode[-1])
    what = ("mixed", B)
    _same(dec.decode_batch(_synd(case_id, what)),
          _oracle(oracle, case_id, precision, "nonuniform", level, alpha, what, method=method), (mode, B))


@pytest.mark.parametrize("xlds", ["1", "0"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_hbm_lanes_decode_several_syndromes(gpu, oracle, monkeypatch, precision, xlds):
    """A workspace budget of one wave (QLDPC_HBM_WS_GB) leaves one workgroup of 256 lanes for 700
    syndromes: every lane takes its next syndrome from the device queue when its decode ends, after
    1 to 20 iterations, next to lanes that are still decoding."""
    case_id, level, what = "col9", _mid("col9"), ("mixed", 700)
    want = _oracle(oracle, case_id, precision, "nonuniform", level, bc.ALPHA, what)
    assert bc.classes_of(want[1], want[2])["fail"] >= 5 and bc.classes_of(want[1], want[2])["late"] >= 5
    dec = _decoder(case_id, precision, "nonuniform", level, bc.ALPHA)
    assert _route(dec)[0] == 6
    monkeypatch.setenv("QLDPC_HBM_WS_GB", "1e-9")
    monkeypatch.setenv("QLDPC_HBM_XLDS", xlds)
    _same(dec.decode_batch(_synd(case_id, what)), want, xlds)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("mode", ["engine2", "engine3", "engine5"])
def test_workgroups_decode_several_syndromes(gpu, oracle, mode, precision):
    """B = 2 x blocks_per_cu x CUs + 1: every workgroup of the persistent grid decodes more than one
    syndrome (engine 2: its one slot is refilled from a chunk of 3; engine 3: chunks of 1 from the
    queue; engine 5: the state reset and the double-buffered flag across syndromes)."""
    import torch

    case_id, kw, method, alpha = {"engine2": ("col8", {}, "minimum_sum", bc.ALPHA),
                                  "engine3": ("row13", {}, "minimum_sum", bc.ALPHA),
                                  "engine5": ("row13", {"bp_method": "product_sum"}, "product_sum", 0.0)}[mode]
    level = _mid(case_id)
    dec = _decoder(case_id, precision, "nonuniform", level, alpha, **kw)
    g = dec.geometry()
    assert g["engine"] == int(mode[-1])
    cap = g["blocks_per_cu"] * torch.cuda.get_device_properties(dec.graph.device).multi_processor_count
    B = 2 * cap + 1
    what = ("mixed", B)
    want = _oracle(oracle, case_id, precision, "nonuniform", level, alpha, what, method=method)
    cl = bc.classes_of(want[1], want[2])
    assert min(cl.values()) >= 5, cl
    _same(dec.decode_batch(_synd(case_id, what)), want, (mode, B))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case_id", ["col8", "col9"])
def test_set_channel_probs_equals_fresh_decoder(gpu, oracle, case_id, precision):
    from qldpc_fault_tolerance_amd.engine import DeviceBP

    lv = bc.CASES[case_id].levels
    dec = DeviceBP(bc.graph(case_id), bc.priors(case_id, "uniform", lv[0]), max_iter=bc.MAX_ITER,
                   ms_scaling_factor=bc.ALPHA, precision=precision)
    assert _route(dec)[0] == {"col8": 2, "col9": 6}[case_id]
    what = ("level", lv[0])
    _same(dec.decode_batch(_synd(case_id, what)), _oracle(oracle, case_id, precision, "uniform", lv[0], bc.ALPHA, what), "before")
    for kind, level in (("nonuniform", lv[2]), ("half", lv[1])):
        dec.set_channel_probs(bc.priors(case_id, kind, level))
        what = ("level", level)
        got = dec.decode_batch(_synd(case_id, what))
        _same(got, _oracle(oracle, case_id, precision, kind, level, bc.ALPHA, what), (kind, level))
        _same(_decoder(case_id, precision, kind, level, bc.ALPHA).decode_batch(_synd(case_id, what)), got, "fresh")

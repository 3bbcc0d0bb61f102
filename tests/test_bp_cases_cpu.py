"""The irregular-graph BP case table (tests/bp_cases.py) on the CPU alone: the routes it records, the
graphs the plan must refuse, non-vacuity of every case under the oracle, and two independent
restatements of the oracle's decoding laws on graphs no bundled code resembles.  No GPU needed."""
import numpy as np
import pytest

import bp_cases as bc
import relay_ref
from qldpc_fault_tolerance_amd import _native
from qldpc_fault_tolerance_amd.codes import CSR
from qldpc_fault_tolerance_amd.engine import DeviceBP, DeviceGraph, plan_bp

EINVAL = -1  # QLDPC_EINVAL (include/qldpc_hip.h)
METHODS = ("minimum_sum", "product_sum")


# ------------------------------------------------------------------------------- the table itself
@pytest.mark.parametrize("case_id", bc.CASE_IDS)
def test_graph_has_the_degrees_its_case_names(case_id):
    c, H = bc.CASES[case_id], bc.graph(case_id)
    rows, cols = H.sum(axis=1), H.sum(axis=0)
    if c.kind == "holes":
        assert rows[c.m // 2] == 0 and cols[c.n // 2] == 0 and cols[-1] == 0 and cols.max() == 3
    elif c.kind == "ai":
        assert np.array_equal(H[:, -c.m:], np.eye(c.m, dtype=np.uint8)) and cols[:-c.m].max() == 3
    else:
        assert np.array_equal(cols, bc.column_degrees(c))
        assert rows.max() - rows.min() <= 1  # the builder balances the rows
    assert H.flags.writeable is False


def test_wide_rows_have_the_widths_their_names_say():
    for case_id, width in (("row13", 13), ("row16", 16), ("row32", 32), ("row33", 33), ("row64", 64)):
        assert set(bc.graph(case_id).sum(axis=1)) == {width}


# --------------------------------------------------------------------------------- route agreement
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("case_id", bc.CASE_IDS)
def test_plan_equals_recorded_route(case_id, precision):
    c, H = bc.CASES[case_id], bc.graph(case_id)
    for kind in bc.PRIORS:
        plan = plan_bp(H, bc.priors(case_id, kind), precision=precision)
        assert (plan["engine"], plan["kernel_id"], plan["row_chunks"]) == c.route(precision, kind), kind


def test_recorded_routes_reach_the_paths_the_table_is_for():
    r64 = {cid: bc.CASES[cid].route64 for cid in bc.CASE_IDS}
    assert {r64[c][0] for c in ("col9", "col12", "col1to12")} == {6}            # engine 6 unasked
    assert {r64[c][0] for c in ("col7", "col8", "col1to8", "col7_vpl2")} == {2}  # the 8-slot kernels
    assert [r64[c][2] for c in ("row13", "row16", "row32", "row33", "row64")] == [7, 8, 16, 17, 32]
    assert {r64[c][0] for c in ("row13", "row16", "row32", "row33", "row64")} == {3}
    assert plan_bp(bc.graph("col7_vpl2"), bc.P0)["vars_per_thread"] == 2
    for c in bc.CASE_IDS:  # engine 6's LDS-ballot switch
        assert (bc.CASES[c].m + bc.CASES[c].n <= 2048) == (c != "xlds_2049")


# ------------------------------------------------------------- the plan refuses what creation refuses
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", list(bc.OVER_DEGREE))
def test_plan_refuses_degrees_past_engine_6(name, precision):
    H = bc.over_degree_graph(name)
    assert max(H.sum(axis=0).max(), H.sum(axis=1).max()) > bc.HBM_MAX_DEG and H.sum(axis=0).max() > 8
    with pytest.raises(_native.QldpcError, match="HBM engine: row or column degree above 12") as e:
        plan_bp(H, bc.P0, precision=precision)
    assert e.value.rc == _native.ENOTSUP


def test_plan_takes_degree_12_in_both_directions():
    assert plan_bp(bc.graph("col12"), bc.P0)["engine"] == 6


@pytest.mark.parametrize("shape", [(0, 5), (3, 0), (0, 0)])
def test_plan_and_creation_refuse_empty_shapes_alike(shape):
    """m = 0 or n = 0: QLDPC_EINVAL from the plan and from every creation entry point, before either
    touches a device (the kernels read the first row and column unconditionally)."""
    H = np.zeros(shape, np.uint8)
    probs = np.full(max(shape[1], 1), bc.P0)[:shape[1]]
    calls = [lambda: plan_bp(H, probs)]
    for kw in ({}, {"soft": True}, {"hbm": True}, {"bp_method": "product_sum"},
               {"relay": {"pre_iter": 4}}):
        calls.append(lambda kw=kw: DeviceBP(H, probs, max_iter=3, device=0, **kw))
    for call in calls:
        with pytest.raises(_native.QldpcError) as e:
            call()
        assert e.value.rc == EINVAL


def test_a_graph_without_checks_is_still_a_graph():
    assert DeviceGraph(np.zeros((0, 5), np.uint8), device=0).info()["m"] == 0  # logical operators of K = 0


# ------------------------------------------------------------------------------------ non-vacuity
@pytest.fixture(scope="module")
def decoded(oracle):
    """(case, method, level) -> (corr, iters, conv) of the oracle, fp64, non-uniform priors."""
    memo = {}

    def get(case_id, method, level):
        key = (case_id, method, level)
        if key not in memo:
            memo[key] = oracle.bp_decode_batch(bc.graph(case_id), bc.priors(case_id, "nonuniform", level), bc.MAX_ITER,
                                               method, bc.ALPHA, bc.syndromes(case_id, level), 64)
        return memo[key]

    return get


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case_id", bc.CASE_IDS)
def test_every_case_holds_every_decode_class(decoded, case_id, method):
    """The syndromes the GPU tests decode contain non-converging, late-converging and
    first-iteration decodes under the oracle alone (max_iter 20, alpha 0.625, fp64, non-uniform
    priors), so a kernel that is wrong only after the first iteration, or only when it runs to
    max_iter, cannot pass them."""
    c = bc.CASES[case_id]
    total = {k: 0 for k in bc.NEEDED}
    for level in c.levels:
        _, iters, conv = decoded(case_id, method, level)
        for k, v in bc.classes_of(iters, conv).items():
            total[k] += v
    print(case_id, method, total)
    for k in c.classes:
        assert total[k] >= bc.NEEDED[k], (k, total)
    mixed = bc.mixed(case_id, 333)
    assert len(mixed) == 333


@pytest.mark.parametrize("case_id", ["holes"])
def test_empty_row_syndrome_is_unsatisfiable(decoded, case_id):
    hole = bc.empty_rows(case_id)
    assert hole.size == 1
    for level in bc.CASES[case_id].levels:
        S = bc.syndromes(case_id, level)
        bad = np.flatnonzero(S[:, hole[0]])
        assert bad.size == 1
        assert not decoded(case_id, "minimum_sum", level)[2][bad[0]]
        assert not S[np.flatnonzero(~S.any(axis=1))].any() and (~S.any(axis=1)).sum() >= 1  # the zero syndrome


# -------------------------------------------------------------- independent restatements of the oracle
def _picked(oracle, case_id, method, level):
    """A few syndromes of each decode class at one level (the Python restatements are slow)."""
    S = bc.syndromes(case_id, level)
    _, iters, conv = oracle.bp_decode_batch(bc.graph(case_id), bc.priors(case_id, "nonuniform", level), bc.MAX_ITER,
                                            method, bc.ALPHA, S, 64)
    idx = np.concatenate([np.flatnonzero(~conv)[:1], np.flatnonzero(conv & (iters > 1))[:2],
                          np.flatnonzero(conv & (iters == 1))[:1]])
    return np.ascontiguousarray(S[idx])


@pytest.mark.parametrize("precision,alpha", [(64, bc.ALPHA), (32, 0.0), (64, 0.0), (32, bc.ALPHA)])
@pytest.mark.parametrize("case_id", bc.SMALL_IDS)
def test_oracle_min_sum_equals_relay_restatement(oracle, case_id, precision, alpha):
    """tests/relay_ref.py with no legs and pre_gamma = 0 is plain min-sum in the oracle's operation
    order, written independently: corrections, iteration counts and flags bit for bit."""
    c = bc.CASES[case_id]
    csr = CSR.from_dense(bc.graph(case_id))
    level = c.levels[len(c.levels) // 2 - 1]
    kind = "half" if precision == 64 else "nonuniform"
    probs = bc.priors(case_id, kind, level)
    S = _picked(oracle, case_id, "minimum_sum", level)
    oc, oi, ov = oracle.bp_decode_batch(csr, probs, bc.MAX_ITER, "minimum_sum", alpha, S, precision)
    with np.errstate(all="ignore"):  # one_col in fp32: five messages of alpha * FLT_MAX overflow, as in C
        rc, ri, rv, _ = relay_ref.decode_batch(oracle, csr, probs, bc.MAX_ITER, 0.0, 0, 0, 0.0, 0.0, 1, 0, alpha, precision, S)
    assert np.array_equal(ri, oi) and np.array_equal(rv.astype(bool), ov) and np.array_equal(rc, oc)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("case_id", bc.SMALL_IDS)
def test_oracle_product_sum_equals_python_restatement(oracle, case_id, precision):
    """bc.ps_ref: ordered forward / backward products, NaN -> 1, decision ratio >= 1, in numpy
    scalars of the decoder's type."""
    c = bc.CASES[case_id]
    csr = CSR.from_dense(bc.graph(case_id))
    level = c.levels[len(c.levels) // 2 - 1]
    probs = bc.priors(case_id, "half" if precision == 32 else "nonuniform", level)
    S = _picked(oracle, case_id, "product_sum", level)
    oc, oi, ov = oracle.bp_decode_batch(csr, probs, bc.MAX_ITER, "product_sum", 0.0, S, precision)
    rc, ri, rv = bc.ps_ref(csr, probs, bc.MAX_ITER, precision, S)
    assert np.array_equal(ri, oi) and np.array_equal(rv, ov) and np.array_equal(rc, oc)


# --------------------------------------------------------------------------------------- CSR.matvec
@pytest.mark.parametrize("H", [
    np.array([[1, 1, 0, 1], [0, 0, 0, 0], [0, 1, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]], np.uint8),  # trailing empty rows
    np.zeros((3, 4), np.uint8),                                                               # no edges at all
    np.array([[0, 0, 0], [1, 0, 1]], np.uint8),                                               # leading empty row
    np.zeros((0, 4), np.uint8),
], ids=["trailing", "edgeless", "leading", "no_rows"])
def test_csr_matvec_with_empty_rows(H):
    csr = CSR.from_dense(H)
    rng = np.random.default_rng(5)
    V = rng.integers(0, 2, size=(7, H.shape[1])).astype(np.uint8)
    want = (V.astype(np.int64) @ H.T.astype(np.int64) % 2).astype(np.uint8)
    got = csr.matvec(V)
    assert got.shape == want.shape and np.array_equal(got, want)
    for b in range(len(V)):
        one = csr.matvec(V[b])
        assert one.shape == (H.shape[0],) and np.array_equal(one, want[b])


def test_csr_matvec_on_the_table(oracle):
    for case_id in ("holes", "a_i", "one_col"):
        H = bc.graph(case_id)
        V = np.random.default_rng(6).integers(0, 2, size=(5, H.shape[1])).astype(np.uint8)
        assert np.array_equal(CSR.from_dense(H).matvec(V), V.astype(np.int64) @ H.T.astype(np.int64) % 2)

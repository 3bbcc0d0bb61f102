"""The route plan (``plan_bp`` / ``qldpc_bp_plan``: host only) against the routes recorded on an MI355X
for every bundled graph (tests/golden/routes_fp{64,32}.jsonl: hz, its space-time graphs over 2-5
rounds and [hz | I] of every bundled code, plus the hgp codes' hz with QLDPC_M2S=0), and the
switch cases the GPU suites pin.  No GPU needed."""
import numpy as np
import pytest

import route_fixtures as rf
from qldpc_fault_tolerance_amd import _native, codes
from qldpc_fault_tolerance_amd.engine import plan_bp

LINES = rf.load(64) + rf.load(32)


def _plan(code, tag, precision, **env):
    H = rf.graph(code, tag)
    with rf.switches(env):
        return plan_bp(H, rf.PROB * np.ones(H.n), precision=precision)


def test_fixtures_cover_every_bundled_graph():
    for prec in (64, 32):
        have = {(r["code"], r["graph"]) for r in rf.load(prec) if "QLDPC_M2S" not in r["env"]}
        assert have == {(c, t) for c in codes.bundled_codes() for t in rf.GRAPH_TAGS}
    assert all("error" not in r for r in LINES)


@pytest.mark.parametrize("rec", LINES, ids=rf.line_id)
def test_plan_equals_recorded_route(rec):
    H = rf.graph(rec["code"], rec["graph"])
    assert (H.m, H.n, len(H.col_idx)) == (rec["m"], rec["n"], rec["nnz"])
    with rf.switches(rec["env"]):
        plan = plan_bp(H, rf.PROB * np.ones(H.n), precision=rec["precision"])
    assert {k: plan[k] for k in rf.PLANNED} == {k: rec[k] for k in rf.PLANNED}


def test_m2s_switch_plans_the_two_word_family():
    assert _plan("hgp_34_n1600", "hz", 64)["kernel_id"] == 11103
    assert _plan("hgp_34_n1600", "hz", 64, QLDPC_M2S="0")["kernel_id"] == 103


def test_small_hgp_graph_stays_off_the_m2s_family():
    assert _plan("hgp_34_n225", "hz", 64)["kernel_id"] != 11103


def test_config5_space_time_graph_plans_the_one_word_tail_family():
    H = rf.graph("hgp_34_n1225_q3", "st3")
    assert (H.m, H.n) == (1764, 5439)
    plan = plan_bp(H, rf.PROB * np.ones(H.n), precision=64)
    assert (plan["engine"], plan["kernel_id"], plan["threads"], plan["vars_per_thread"]) == (3, 111313, 1024, 6)
    assert plan["degree2_slots"] >= 1
    # non-uniform priors are outside the family (one prior in SGPRs): the two-word tail family
    pr = np.hstack([0.02 * np.ones(1225), 0.01 * np.ones(588)] * 3)
    assert plan_bp(H, pr, precision=64)["kernel_id"] == 101013


@pytest.mark.parametrize("name,tb", [("LP_Matg8_L16_Dmin12", 128), ("LP_Matg8_L21_Dmin16", 192)])
def test_small_lp_codes_plan_the_m2s8_geometry(name, tb):
    plan = _plan(name, "hz", 64)
    assert (plan["engine"], plan["kernel_id"], plan["row_chunks"], plan["threads"], plan["vars_per_thread"]) == \
        (3, 10203, 4, tb, 5)
    assert _plan(name, "hz", 64, QLDPC_M2S8_SMALL="0")["engine"] == 2


def test_hbm_fallback_switch_turns_the_fallback_into_enotsup():
    assert _plan("GenBicycleA4", "st5", 32)["engine"] == 6
    with pytest.raises(_native.QldpcError) as e:
        _plan("GenBicycleA4", "st5", 32, QLDPC_HBM_FALLBACK="0")
    assert e.value.rc == _native.ENOTSUP


def _removed_family_graphs():
    code = codes.get_code("hgp_34_n1600")
    return {
        "n1600-hz": lambda: codes.CSR.from_dense(code.hz),
        "n1600-hx": lambda: codes.CSR.from_dense(code.hx),
        # 512 threads x 4 variables on the plain fp64 kernels: the geometry the removed 257-512-thread
        # family took
        "n1225-hI-512-threads": lambda: rf.graph("hgp_34_n1225_q3", "hI"),
    }


@pytest.mark.parametrize("name", list(_removed_family_graphs()))
def test_switches_of_the_removed_families_move_no_plan(name):
    """QLDPC_C2S / QLDPC_M2V / QLDPC_M2V_PERM / QLDPC_F64X selected kernel families that were measured,
    not kept and removed: the plan is the one with none of them set."""
    H = _removed_family_graphs()[name]()
    pr = rf.PROB * np.ones(H.n)
    plain = plan_bp(H, pr, precision=64)
    if name.startswith("n1225"):
        assert 256 < plain["threads"] <= 512 and plain["engine"] == 3, plain
    with rf.switches({"QLDPC_C2S": "1", "QLDPC_M2V": "1", "QLDPC_M2V_PERM": "1", "QLDPC_F64X": "1"}):
        assert plan_bp(H, pr, precision=64) == plain


def test_engine_4_is_not_supported():
    with pytest.raises(_native.QldpcError) as e:
        _plan("hgp_34_n225", "hz", 64, QLDPC_ENGINE="4")
    assert e.value.rc == _native.ENOTSUP


def test_product_sum_has_no_host_plan():
    H = rf.graph("hgp_34_n225", "hz")
    with pytest.raises(_native.QldpcError) as e:
        plan_bp(H, 0.05, bp_method="product_sum")
    assert e.value.rc == _native.ENOTSUP

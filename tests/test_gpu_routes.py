"""Decoders built on the GPU against the host route plan and the routes recorded on an MI355X
(tests/golden/routes_fp{64,32}.jsonl), for the smallest graph of every distinct (precision,
kernel id) there.  ``lds_model`` and the bank-stats pair are functions of the built edge tables and
check labels, so their equality with the recorded values pins the tables as well as the route."""
import numpy as np
import pytest

import route_fixtures as rf
from qldpc_fault_tolerance_amd.engine import DeviceBP, plan_bp

pytestmark = pytest.mark.gpu


def _smallest_per_kernel():
    best = {}
    for rec in rf.load(64) + rf.load(32):
        key = (rec["precision"], rec["kernel_id"])
        if key not in best or rec["nnz"] < best[key]["nnz"]:
            best[key] = rec
    return [best[k] for k in sorted(best)]


@pytest.mark.parametrize("rec", _smallest_per_kernel(), ids=rf.line_id)
def test_built_decoder_equals_plan_and_recorded_route(gpu, rec):
    H = rf.graph(rec["code"], rec["graph"])
    probs = rf.PROB * np.ones(H.n)
    with rf.switches(rec["env"]):
        plan = plan_bp(H, probs, precision=rec["precision"])
        geo = DeviceBP(H, probs, max_iter=10, precision=rec["precision"]).geometry()
    geo["gather_conflicts"] = list(geo["gather_conflicts"])
    assert {k: geo[k] for k in rf.PLANNED} == {k: plan[k] for k in rf.PLANNED}
    assert geo == {k: rec[k] for k in geo}

"""The BP+LSD case table (tests/lsd_cases.py) without a GPU: the host stage equals the Python law bit
for bit on every graph, posterior kind and syndrome kind; the table exercises every event kind of the
law; the outputs satisfy what the law promises; the two ``fit`` graphs sit on the edge of the kernel's
LDS accounting.
"""
import numpy as np
import pytest

import lsd_cases
import lsd_ref
from qldpc_fault_tolerance_amd.engine import HostLSD

_LAW = {}


def law(case_id, k):
    """(selected batch rows, x, stats, events) of a case at k under the Python law, computed once."""
    if (case_id, k) not in _LAW:
        S, P, inc = lsd_cases.inputs(case_id)
        sel = np.flatnonzero([k in lsd_cases.ks_of(case_id, bool(i)) for i in inc])
        _LAW[case_id, k] = (sel,) + lsd_ref.decode_batch(lsd_cases.graph(case_id), S[sel], P[sel], k)
    return _LAW[case_id, k]


@pytest.mark.parametrize("k", lsd_cases.KS)
@pytest.mark.parametrize("case_id", lsd_cases.CASE_IDS)
def test_host_stage_equals_the_law_on_the_table(case_id, k):
    H = lsd_cases.graph(case_id)
    S, P, inc = lsd_cases.inputs(case_id)
    sel, X, T, _ = law(case_id, k)
    lsd = HostLSD(H, k)
    x, st = lsd.decode_batch_stats(S[sel], P[sel], threads=1)
    assert np.array_equal(x, X) and np.array_equal(st, T)
    # B = 96 on two threads, B = 1
    rep = np.resize(np.arange(sel.size), 96)
    x96, st96 = lsd.decode_batch_stats(S[sel][rep], P[sel][rep], threads=2)
    assert np.array_equal(x96, X[rep]) and np.array_equal(st96, T[rep])
    x1, st1 = lsd.decode_batch_stats(S[sel][:1], P[sel][:1], threads=2)
    assert np.array_equal(x1, X[:1]) and np.array_equal(st1, T[:1])
    # what the law promises
    Hx = (x.astype(np.int64) @ H.T.astype(np.int64) % 2).astype(np.uint8)
    ok = st[:, 0] == 1
    assert np.array_equal(Hx[ok], S[sel][ok])
    assert np.array_equal(ok, ~inc[sel]), "exactly the inconsistent syndromes have an unsolvable cluster"
    zero = ~S[sel].any(1)
    assert (st[zero] == (1, 0, 0, 0)).all() and not x[zero].any()
    # (valid = 0: H x = s on the rows of the valid clusters is asserted inside lsd_ref.decode)


def test_every_event_kind_occurs():
    tot = dict.fromkeys(lsd_ref.EVENTS, 0)
    for case_id in lsd_cases.CASE_IDS:
        for k in lsd_cases.KS:
            for e, c in law(case_id, k)[3].items():
                tot[e] += c
    print("events over the table:", tot)
    for e in lsd_ref.EVENTS:
        assert tot[e] >= 1, e


def test_inconsistent_syndromes_where_the_graph_allows_them():
    with_zero_row = 0
    for case_id in lsd_cases.CASE_IDS:
        H = lsd_cases.graph(case_id)
        S, _, inc = lsd_cases.inputs(case_id)
        assert not S[6].any() and (S[:6].any() or not H.any())
        with_zero_row += int(any(S[b][H.sum(1) == 0].any() for b in np.flatnonzero(inc)))
    assert with_zero_row >= 3, "a set row of an all-zero row of H"


def test_fit_graphs_sit_on_the_edge_of_the_lds_accounting():
    m = lsd_cases.fit_rows()
    assert lsd_cases.graph("fit_exact").shape == (m, lsd_cases.FIT_N)
    assert lsd_cases.graph("fit_over").shape == (m + 1, lsd_cases.FIT_N)
    assert lsd_cases.expected(m, lsd_cases.FIT_N)["lds_rows"] == m
    assert lsd_cases.expected(m + 1, lsd_cases.FIT_N)["lds_rows"] == m
    assert lsd_cases.expected(m, lsd_cases.FIT_N)["lds_bytes"] <= 64 * 1024
    # the swallowing syndromes reach every row of the graph's one large component: more than the image holds
    for case_id in ("fit_exact", "fit_over"):
        sel, X, T, _ = law(case_id, 64)
        assert T[:, 2].max() == lsd_cases.FIT_N
        assert lsd_cases.graph(case_id).any(1).all(), "every row is adjacent to a column, so every row turns active"
    e = lsd_cases.expected(8192, 8192)
    assert e["lds_bytes"] <= lsd_cases.LDS_MAX and e["lds_rows"] >= 64

"""The host law of the distance search (``qldpc_dist_run_host``) against the NumPy restatement
(tests/distance_ref.py) on every case of tests/distance_cases.py, bit for bit; the witness checked
without either implementation; and the conditions that keep the table from being vacuous, each
decided by the restatement alone.  tests/test_gpu_distance_cases.py then pins the kernel to the
host law on the same cases, seed and trial range."""
import numpy as np
import pytest

import distance_cases as dc
import distance_ref as ref
from qldpc_fault_tolerance_amd import _native, gf2

_RUNS = {}


def _reference(oracle, case_id, paired=True):
    """(weight, trial, witness, trial_min, facts) of the restatement, computed once per case."""
    key = (case_id, paired)
    if key not in _RUNS:
        c = dc.CASES[case_id]
        G, P, _ = dc.matrices(case_id)
        facts = []
        bw, bt, wit, tmin = ref.search(oracle, G, P if paired else None, dc.SEED, dc.TRIAL_BEGIN, c.trials, facts)
        tmin.setflags(write=False)
        _RUNS[key] = (bw, bt, wit, tmin, facts)
    return _RUNS[key]


# ------------------------------------------------------------------ the table itself
def test_table_restates_the_selector():
    for c in dc.CASES.values():
        rw, pw = -(-c.n // 64), -(-c.k // 64)
        assert (c.row_words, c.pair_words) == (rw, pw), c.id
        assert c.tpl == next(w for w in dc.WIDTHS if w >= rw + pw), c.id
        assert c.threads == -(-c.rows // 64) * 64 and 64 <= c.threads <= 1024, c.id
        assert c.lds_bytes == 16400 + 256 * c.tpl
        assert c.trials <= (2 if c.rows * c.n > 500_000 else 24), c.id
        G, P, L = dc.matrices(c.id)
        assert G.shape == (c.rows, c.n) and (P is None) == (c.k == 0), c.id
        if P is not None:
            assert P.shape == (c.rows, c.k) and np.array_equal(P, gf2.matmul(G, L.T)), c.id


def test_every_width_runs_exactly_full_and_padded():
    full = {c.tpl for c in dc.CASES.values() if c.row_words + c.pair_words == c.tpl}
    padded = {c.tpl for c in dc.CASES.values() if c.row_words + c.pair_words < c.tpl}
    assert full == set(dc.WIDTHS) and padded == set(dc.WIDTHS)
    assert {c.rows for c in dc.CASES.values()} >= {1, 63, 64, 65, 128, 1023, 1024}
    assert {c.k for c in dc.CASES.values()} >= {0, 1, 63, 64, 65, 128}


@pytest.mark.parametrize("case_id", dc.CASE_IDS)
def test_rank_is_what_the_case_declares(case_id):
    c = dc.CASES[case_id]
    G, _, _ = dc.matrices(case_id)
    rank = gf2.rank(G) if G.any() else 0
    if c.full is True:
        assert rank == c.rows
    elif c.full is False:
        assert rank < c.rows
    if c.kind == "span":
        assert rank == c.rank < min(c.rows, c.n)   # rank = n would reduce every trial to the identity


def test_structure_of_the_special_cases():
    G, _, _ = dc.matrices("zero_rows")
    assert not G[[0, 63, 64, 149]].any() and G[1:63].any(axis=1).all()
    G, _, _ = dc.matrices("dup_rows")
    assert np.array_equal(G[-5:], G[:5]) and np.array_equal(G[70], G[10] ^ G[11])
    G, _, _ = dc.matrices("rank1")
    assert G[0].any() and (G == G[0]).all()
    G, _, _ = dc.matrices("last_wave_only")
    assert not G[:dc.LAST_WAVE_FIRST_ROW].any() and G[dc.LAST_WAVE_FIRST_ROW:].any(axis=1).all()
    G, _, _ = dc.matrices("dense_row")
    assert sorted(G.sum(axis=1))[-3] > 80
    G, _, _ = dc.matrices("lower_tri_dense")
    assert not np.triu(G, 1).any() and G.diagonal().all() and G.sum() > 128 * 128 // 5
    for cid in ("n64_lastword", "n128_lastword"):
        G, _, _ = dc.matrices(cid)
        assert G.any(axis=0)[-64:].all(), cid
    G, P, _ = dc.matrices("pair_last_bit")
    assert not P[:, :127].any() and 20 <= P[:, 127].sum() <= 30
    assert dc.matrices("pair_dense")[1].all() and not dc.matrices("pair_zero")[1].any()
    G, P, _ = dc.matrices("pair_heavy_only")
    heavy = list(dc.HEAVY_ROWS)
    assert np.flatnonzero(P.any(axis=1)).tolist() == heavy
    assert G[heavy].sum(axis=1).min() > 2 * np.delete(G, heavy, axis=0).sum(axis=1).max()


# ------------------------------------------------------------------ host law == restatement
@pytest.mark.parametrize("case_id", dc.CASE_IDS)
def test_host_law_matches_restatement(oracle, case_id):
    c = dc.CASES[case_id]
    G, P, L = dc.matrices(case_id)
    bw, bt, wit, tmin, facts = _reference(oracle, case_id)
    hw, ht, htmin, hwit, geo = dc.run_raw(G, P, c.trials, dc.SEED, dc.TRIAL_BEGIN)
    assert geo == [0, c.row_words, c.pair_words, 0]   # host handle: no threads, no LDS
    assert np.array_equal(htmin, tmin)
    assert (hw, ht) == (bw, bt)
    assert np.array_equal(hwit, wit)

    # independent of both: the witness is a vector of the row space with the reported weight that
    # pairs non-trivially
    if not c.candidate:
        assert bw == ref.NO_CANDIDATE and bt == 0 and not wit.any() and (tmin == ref.NO_CANDIDATE).all()
        return
    assert (tmin != ref.NO_CANDIDATE).all(), "a trial without a candidate"
    assert 1 <= bw == int(hwit.sum()) == tmin.min()
    assert ht == dc.TRIAL_BEGIN + int(np.flatnonzero(tmin == bw)[0])
    assert gf2.rank(np.vstack([G, hwit[None, :]])) == gf2.rank(G)
    if L is not None:
        assert gf2.matmul(L, hwit[:, None]).any()

    # not vacuous: the minimum moves between trials, and some trial passes over a column that no
    # row can take before it has all its pivots
    if case_id not in dc.TRIVIAL:
        assert len(set(tmin.tolist())) >= 2, tmin
        assert any(f.skipped_before_last > 0 for f in facts)
    if c.full is True:
        assert all(f.npiv == c.rows for f in facts)


def test_trivial_cases_are_trivial_for_the_stated_reason(oracle):
    """The cases left out of the two conditions above cannot meet them: one row, a rank-1 space, or
    a square invertible G (every column pivots and the reduced matrix is the identity)."""
    for cid in dc.TRIVIAL:
        c = dc.CASES[cid]
        G, _, _ = dc.matrices(cid)
        rank = gf2.rank(G) if G.any() else 0
        assert rank <= 1 or rank == c.rows == c.n, cid
    _, _, _, tmin, facts = _reference(oracle, "lower_tri_dense")
    assert (tmin == 1).all() and all(f.skipped_before_last == 0 and f.last_pivot == 127 for f in facts)
    _, _, _, tmin, facts = _reference(oracle, "lower_tri_wide")   # its wide twin does move
    assert len(set(tmin.tolist())) >= 2


# ------------------------------------------------------------------ what single cases are there for
def test_all_zero_takes_no_pivot(oracle):
    _, _, _, _, facts = _reference(oracle, "all_zero")
    assert all(f.npiv == 0 and f.last_pivot == -1 for f in facts)


def test_identity_witness_is_the_first_column(oracle):
    for cid in ("identity", "ties"):
        bw, bt, wit, tmin, facts = _reference(oracle, cid)
        assert (tmin == 1).all() and bt == dc.TRIAL_BEGIN
        first = ref.column_order(oracle, 100, dc.SEED, dc.TRIAL_BEGIN)[0]
        assert np.flatnonzero(wit).tolist() == [first]
        assert all(f.pos == 0 and f.npiv == 100 for f in facts)


def test_ties_spread_over_grids_of_2_3_and_7(oracle):
    bw, _, _, tmin, facts = _reference(oracle, "ties")
    at_min = np.flatnonzero(tmin == bw)   # offsets in the range: what the grid stride distributes
    assert at_min.size >= 4
    assert len(set(at_min % 2)) == 2 and len(set(at_min % 3)) >= 2 and len(set(at_min % 7)) >= 2
    # the tied trials hold different witnesses, so returning a later one shows
    assert len({tuple(f.row) for f in facts}) >= 4


def test_last_wave_only_pivots_in_wave_15(oracle):
    _, _, _, _, facts = _reference(oracle, "last_wave_only")
    for f in facts:
        assert f.npiv == 40 and min(f.pivot_rows) >= dc.LAST_WAVE_FIRST_ROW


def test_rank_deficient_cases_visit_every_column(oracle):
    for cid in ("w2_full", "zero_rows", "dup_rows", "rows_1024"):
        c = dc.CASES[cid]
        G, _, _ = dc.matrices(cid)
        rank = gf2.rank(G)
        _, _, _, _, facts = _reference(oracle, cid)
        assert all(f.npiv == rank < c.rows for f in facts), cid
        assert any(c.n - 1 - f.last_pivot > 0 for f in facts), cid   # columns walked after the last pivot


def test_pair_heavy_only_filter_changes_the_answer(oracle):
    _, _, _, paired, facts = _reference(oracle, "pair_heavy_only")
    _, _, _, classical, _ = _reference(oracle, "pair_heavy_only", paired=False)
    assert (classical <= paired).all() and (classical < paired).any()
    assert all(len(f.filtered_rows) > 0 for f in facts)


def test_pair_last_bit_candidates_pair_in_bit_127_only(oracle):
    G, P, L = dc.matrices("pair_last_bit")
    _, _, _, tmin, facts = _reference(oracle, "pair_last_bit")
    for f in facts:
        pairing = gf2.matmul(L, f.row[:, None])[:, 0]
        assert not pairing[:64].any() and not pairing[64:127].any() and pairing[127] == 1
    assert any(len(f.filtered_rows) > 0 for f in facts)


def test_last_row_pairings_filter_rows_in_every_trial(oracle):
    ids = [c.id for c in dc.CASES.values() if c.pairing == "last_row"]
    assert len(ids) >= 7 and {dc.CASES[i].tpl for i in ids} >= {4, 8, 12, 20, 24, 26, 28}
    for cid in ids:
        c = dc.CASES[cid]
        assert c.row_words + c.pair_words == c.tpl, cid   # the pairing word closes an exactly full row
        _, P, _ = dc.matrices(cid)
        assert not P[:, :-1].any() and 15 <= P[:, -1].sum() <= 55, cid
        _, _, _, _, facts = _reference(oracle, cid)
        assert all(0 < len(f.filtered_rows) < c.rows for f in facts), cid


def test_pair_zero_filters_every_pivot_row(oracle):
    _, _, _, tmin, facts = _reference(oracle, "pair_zero")
    assert all(f.npiv == 70 and len(f.filtered_rows) == 70 for f in facts)


def test_pair_dense_weights_do_not_count_pairing_words(oracle):
    _, _, _, paired, _ = _reference(oracle, "pair_dense")
    _, _, _, classical, _ = _reference(oracle, "pair_dense", paired=False)
    assert np.array_equal(paired, classical) and paired.max() < 128


# ------------------------------------------------------------------ shapes outside the device envelope
@pytest.mark.parametrize("rows,n,k", dc.UNSUPPORTED)
def test_host_handle_runs_shapes_outside_the_device_envelope(oracle, rows, n, k):
    G, P = dc.unsupported_matrices(rows, n, k)
    assert rows > 1024 or rows == 0 or -(-n // 64) + -(-k // 64) > 28
    hw, ht, htmin, hwit, _ = dc.run_raw(G, P, 2, dc.SEED, dc.TRIAL_BEGIN)
    if rows == 0:
        assert hw == ref.NO_CANDIDATE and (htmin == ref.NO_CANDIDATE).all() and not hwit.any()
    elif rows == 1:   # the reduced row is the row
        assert hw == int(G.sum()) and np.array_equal(hwit, G[0]) and (htmin == hw).all()
    else:
        bw, bt, wit, tmin = ref.search(oracle, G, P, dc.SEED, dc.TRIAL_BEGIN, 2)
        assert (hw, ht) == (bw, bt) and np.array_equal(htmin, tmin) and np.array_equal(hwit, wit)


def test_enotsup_is_the_code_the_gpu_file_expects():
    assert _native.ENOTSUP == -4

"""The distance-search kernel (``dist_kernel<WT>``, csrc/distance.hip) at every row width, row
count and rank edge, and the whole surface of ``qldpc_dist_run``.

Each case of tests/distance_cases.py goes through ``qldpc_dist_create`` as a raw ``(G, P)`` pair;
the device handle's geometry is asserted against the table before anything runs (so a case cannot
run another template than it names), then the kernel is compared with ``qldpc_dist_run_host`` on a
host handle: per-trial minima, weight, trial and witness bytes.  The host law is pinned to the
NumPy restatement on the same cases, seed and trial range by tests/test_distance_cases_cpu.py.
Nothing here is floating-point: equality, no tolerance.
"""
import numpy as np
import pytest

import distance_cases as dc

pytestmark = pytest.mark.gpu

DEV = 0
SURFACE = ["w4_pad", "dup_rows", "ties"]   # pairing + full rank, dependent rows, every trial tied
_HOST = {}                                 # host-law results, computed once per input and shared


def _host(case_id, trials, seed=dc.SEED, begin=dc.TRIAL_BEGIN):
    """(weight, trial, witness, trial_min) of ``qldpc_dist_run_host``."""
    key = (case_id, trials, seed, begin)
    if key not in _HOST:
        G, P, _ = dc.matrices(case_id)
        with dc.Handle(G, P) as h:
            w, t, wit, tmin = h.run(trials, seed, begin)
        wit.setflags(write=False)
        tmin.setflags(write=False)
        _HOST[key] = (w, t, wit, tmin)
    return _HOST[key]


def _device(case_id):
    """A device handle of the case, its geometry asserted against the table."""
    c = dc.CASES[case_id]
    G, P, _ = dc.matrices(case_id)
    h = dc.Handle(G, P, device=DEV)
    assert h.geometry() == [c.threads, c.row_words, c.pair_words, c.lds_bytes], case_id
    return h


def _same(got, want, what):
    w, t, wit, tmin = got
    hw, ht, hwit, htmin = want
    if tmin is not None:
        assert np.array_equal(tmin, htmin), (what, tmin.tolist(), htmin.tolist())
    assert (w, t) == (hw, ht), what
    assert np.array_equal(wit, hwit), what


def _default_grid(case_id):
    """workgroups = 0: compute units x (1024 / threads), as include/qldpc_hip.h documents."""
    import torch

    return torch.cuda.get_device_properties(DEV).multi_processor_count * (1024 // dc.CASES[case_id].threads)


# ------------------------------------------------------------------ every case, three grids
@pytest.mark.parametrize("case_id", dc.CASE_IDS)
def test_kernel_matches_host_law(gpu, case_id):
    c = dc.CASES[case_id]
    want = _host(case_id, c.trials)
    assert (want[0] != dc.NO_CANDIDATE) == c.candidate
    with _device(case_id) as h:
        for wg in (1, 2, 0):
            _same(h.run(c.trials, dc.SEED, dc.TRIAL_BEGIN, wg), want, (case_id, wg))


# ------------------------------------------------------------------ the run surface
@pytest.mark.parametrize("wg", [3, 7])
def test_earliest_tied_trial_wins(gpu, wg):
    c = dc.CASES["ties"]
    want = _host("ties", c.trials)
    assert (want[3] == want[0]).sum() >= 4 and want[1] == dc.TRIAL_BEGIN
    with _device("ties") as h:
        _same(h.run(c.trials, dc.SEED, dc.TRIAL_BEGIN, wg), want, wg)


@pytest.mark.parametrize("case_id", SURFACE)
def test_two_rounds_and_one_trial_more(gpu, case_id):
    """trials = 2 * grid + 1: the first workgroup runs three trials, the others two."""
    with _device(case_id) as h:
        for wg, grid in ((2, 2), (0, _default_grid(case_id))):
            trials = 2 * grid + 1
            _same(h.run(trials, dc.SEED, dc.TRIAL_BEGIN, wg), _host(case_id, trials), (case_id, wg, trials))


@pytest.mark.parametrize("case_id", SURFACE)
def test_few_trials(gpu, case_id):
    with _device(case_id) as h:
        _same(h.run(3, dc.SEED, dc.TRIAL_BEGIN, 64), _host(case_id, 3), "more workgroups than trials")
        for wg in (0, 1, 5):
            _same(h.run(1, dc.SEED, dc.TRIAL_BEGIN, wg), _host(case_id, 1), ("one trial", wg))
        for wg in (0, 3):
            w, t, wit, tmin = h.run(0, dc.SEED, dc.TRIAL_BEGIN, wg)   # QLDPC_OK, or run() raises
            assert (w, t) == (dc.NO_CANDIDATE, 0) and not wit.any() and tmin.size == 0


@pytest.mark.parametrize("case_id", SURFACE)
def test_trial_min_may_be_null(gpu, case_id):
    trials = 2 * dc.CASES[case_id].trials
    want = _host(case_id, trials)
    with _device(case_id) as h:
        for wg in (0, 3):
            got = h.run(trials, dc.SEED, dc.TRIAL_BEGIN, wg, want_trial_min=False)
            assert got[3] is None
            _same(got, want, (case_id, wg))


@pytest.mark.parametrize("case_id", SURFACE)
def test_one_handle_run_four_times(gpu, case_id):
    """The per-trial, per-workgroup and witness buffers grow and are then reused: every run of the
    one handle equals a fresh handle's (and the host law)."""
    runs = [(4, 1), (40, 8), (8, 2), (40, 0)]
    with _device(case_id) as h:
        for i, (trials, wg) in enumerate(runs):
            begin = dc.TRIAL_BEGIN + 11 * i   # another range each time: a stale buffer would show
            got = h.run(trials, dc.SEED, begin, wg)
            with _device(case_id) as fresh:
                _same(got, fresh.run(trials, dc.SEED, begin, wg), (case_id, "fresh", trials, wg))
            _same(got, _host(case_id, trials, begin=begin), (case_id, trials, wg))


@pytest.mark.parametrize("case_id", SURFACE)
def test_trial_counter_crosses_2_to_32(gpu, case_id):
    seed, begin = (9 << 32) | 1, (1 << 32) - 3
    want = _host(case_id, 8, seed, begin)
    # the high counter word matters: the same low words under other high words give another answer
    other = _host(case_id, 8, seed, begin + (1 << 32))
    assert not (np.array_equal(other[2], want[2]) and np.array_equal(other[3], want[3]))
    with _device(case_id) as h:
        for wg in (0, 1, 3):
            _same(h.run(8, seed, begin, wg), want, (case_id, wg))


@pytest.mark.parametrize("case_id", SURFACE)
def test_split_range_concatenates(gpu, case_id):
    full = _host(case_id, 32)
    with _device(case_id) as h:
        a = h.run(13, dc.SEED, dc.TRIAL_BEGIN, 4)
        b = h.run(19, dc.SEED, dc.TRIAL_BEGIN + 13, 0)
    assert np.array_equal(np.concatenate([a[3], b[3]]), full[3])
    best = min((a, b), key=lambda r: (r[0], r[1]))
    assert (best[0], best[1]) == (full[0], full[1]) and np.array_equal(best[2], full[2])
    assert b[1] >= dc.TRIAL_BEGIN + 13 or b[0] == dc.NO_CANDIDATE


@pytest.mark.parametrize("case_id", SURFACE)
def test_non_default_stream(gpu, case_id):
    import torch

    c = dc.CASES[case_id]
    want = _host(case_id, c.trials)
    stream = torch.cuda.Stream(device=DEV)
    assert stream.cuda_stream != 0
    with _device(case_id) as h:
        for wg in (0, 2):
            _same(h.run(c.trials, dc.SEED, dc.TRIAL_BEGIN, wg, stream=stream.cuda_stream), want, (case_id, wg))
        _same(h.run(c.trials, dc.SEED, dc.TRIAL_BEGIN, 0), want, (case_id, "default stream after"))


# ------------------------------------------------------------------ the envelope
@pytest.mark.parametrize("rows,n,k", dc.UNSUPPORTED)
def test_shapes_outside_the_envelope_are_refused(gpu, rows, n, k):
    G, P = dc.unsupported_matrices(rows, n, k)
    with pytest.raises(gpu.QldpcError) as e:
        dc.Handle(G, P, device=DEV)
    assert e.value.rc == gpu.ENOTSUP
    with dc.Handle(G, P) as h:   # a host handle takes them
        w, t, wit, tmin = h.run(2, dc.SEED, dc.TRIAL_BEGIN)
    if rows == 0:
        assert w == dc.NO_CANDIDATE and not wit.any()
    else:
        assert 1 <= w == int(wit.sum()) == tmin.min()


def test_no_candidate_through_the_python_surface(gpu):
    from qldpc_fault_tolerance_amd import codes

    I = np.eye(3, dtype=np.uint8)
    ring = (I + np.roll(I, 1, axis=1)) % 2
    c = codes.hgp(ring, ring)
    # a pairing that is identically zero (L inside the stabiliser group): pivots, but no candidate
    r = codes.distance_search(c.hx, c.hx[:2], trials=4, backend="gpu")
    assert r.weight is None and r.hits == 0 and not r.witness.any()
    assert (r.trial_min == dc.NO_CANDIDATE).all()

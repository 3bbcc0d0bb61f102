"""The first-min case table (tests/firstmin_cases.py) and its reference (tests/firstmin_ref.py) on the
CPU alone: the reference replays the reference class's recorded output, every case holds the decode
classes it declares under the reference, the overflowing sums are really in the table, and the LDS
envelope arithmetic of csrc/firstmin.hip.  No GPU needed."""
import os

import numpy as np
import pytest

import bp_cases as bc
import firstmin_cases as fc
import firstmin_ref
from qldpc_fault_tolerance_amd import codes

PHEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_harness_phen_n225.npz")


def test_reference_replays_the_reference_class_fixture(oracle):
    """``firstmin_synd`` -> ``firstmin_corr`` of the phenomenological fixture is FirstMinBPDecoder's own
    output on [hz | I] of hgp_34_n225 (p = 0.02, max_iter 20, alpha 0.625)."""
    g = np.load(PHEN)
    code = codes.get_code("hgp_34_n225")
    mz = code.hz.shape[0]
    h = np.hstack([code.hz, np.identity(mz, dtype=np.uint8)]).astype(np.uint8)
    corr, steps = firstmin_ref.decode(h, np.full(code.N + mz, 0.02), 20, 0.625, 64, g["firstmin_synd"])
    assert np.array_equal(corr, g["firstmin_corr"])
    assert steps.shape == (len(corr),) and steps.max() <= 20


def test_reference_equals_the_scalar_loop(oracle):
    """The vectorised loop against the reference's loop written per syndrome (src/Decoders.py:60-74)."""
    H, S = fc.graph("col1to8"), fc.mixed("col1to8")[:40]
    probs = fc.priors("col1to8", "half", 0.3)
    corr, steps = firstmin_ref.decode(H, probs, 5, 0.625, 64, S)
    Hl = H.astype(np.int64)
    bp1 = firstmin_ref.oracle_bp1(H, probs, 0.625, 64)
    for b in range(len(S)):
        c, cur, k = np.zeros(H.shape[1], np.int64), S[b].astype(np.int64), 0
        nc = bp1(cur[None].astype(np.uint8))[0].astype(np.int64)
        ns = (Hl @ nc + cur) % 2
        while ns.sum() <= cur.sum() and k < 5:
            cur, c, k = ns, (c + nc) % 2, k + 1
            nc = bp1(cur[None].astype(np.uint8))[0].astype(np.int64)
            ns = (Hl @ nc + cur) % 2
        assert np.array_equal(corr[b], c) and steps[b] == k, b


# ------------------------------------------------------------------------------------ non-vacuity
@pytest.mark.parametrize("precision", fc.PRECISIONS)
@pytest.mark.parametrize("case_id", fc.CASE_IDS)
def test_every_case_holds_its_decode_classes(oracle, case_id, precision):
    """The 301 mixed syndromes the GPU tests decode hold rejected, stopped, exhausted and cleared
    decodes under the reference alone (max_iter 12, alpha 0.625, non-uniform priors, over the case's
    prior levels), except the classes the table declares impossible, which it must not hold."""
    c = fc.CASES[case_id]
    S = fc.mixed(case_id)
    assert S.shape == (fc.B_MIXED, fc.graph(case_id).shape[0])
    total = dict.fromkeys(firstmin_ref.CLASSES, 0)
    for level in c.levels:
        t = firstmin_ref.trace(fc.graph(case_id), fc.priors(case_id, "nonuniform", level), fc.MAX_ITER, 0.625,
                               precision, S)
        for k, v in firstmin_ref.classes_of(t, S, fc.MAX_ITER).items():
            total[k] += v
    print(case_id, precision, total)
    absent = dict(c.absent, **(c.absent64 if precision == 64 else {}))
    assert set(absent) <= set(firstmin_ref.CLASSES[:4]) and all(len(r) > 20 for r in absent.values())
    for k in firstmin_ref.CLASSES[:4]:
        if k in absent:
            assert total[k] == 0, (k, total)
        else:
            assert total[k] >= (1 if c.all_syndromes else fc.NEEDED), (k, total)


@pytest.mark.parametrize("precision", fc.PRECISIONS)
def test_holes_under_half_priors_toggles(oracle, precision):
    """Column n - 1 of ``holes`` is empty and has p = 0.5 under ``half`` priors: its LLR is 0, its
    posterior 0 <= 0, so BP1 decides it at every step.  With every other prior below 0.5 that is all
    BP1(0) decides: H dec = 0, every step is accepted, and the bit ends as the parity of max_iter."""
    H, S = fc.graph("holes"), fc.mixed("holes")
    n = H.shape[1]
    probs = fc.priors("holes", "half", 0.03)
    assert fc.CASES["holes"].toggling and [c for c in fc.CASE_IDS if fc.CASES[c].toggling] == ["holes"]
    assert probs[n - 1] == 0.5 and probs[n // 2] == 0.5 and not H[:, [n // 2, n - 1]].any()
    t = firstmin_ref.trace(H, probs, fc.MAX_ITER, 0.625, precision, S)
    k = firstmin_ref.classes_of(t, S, fc.MAX_ITER)
    print(k)
    assert k["toggling"] >= fc.NEEDED and k["cleared"] == 0
    zero = np.flatnonzero(~S.any(axis=1))
    assert zero.size >= 1
    for mi in fc.MAX_ITERS:
        corr, steps = firstmin_ref.decode(H, probs, mi, 0.625, precision, S[zero])
        assert (steps == mi).all() and (corr[:, n - 1] == mi % 2).all() and (corr[:, n // 2] == mi % 2).all()


@pytest.mark.parametrize("precision,alpha", [(64, fc.ALPHA_DEG1), (32, 0.625)])
def test_one_col_sums_overflow(oracle, precision, alpha):
    """Five degree-1 checks on one variable: each sends SENTINEL * alpha, and the variable's sum
    leaves the number format (0.9e308 twice in fp64, 0.625 FLT_MAX twice in fp32).  The posterior
    the oracle's one-iteration BP reports is non-finite at some step of the reference loop."""
    import oracle as orc

    c = fc.CASES["one_col"]
    H, S = fc.graph("one_col"), fc.mixed("one_col")
    assert c.deg1_rows and (H.sum(axis=1) == 1).all() and H.shape == (5, 1) and alpha in c.alphas
    probs = fc.priors("one_col", "nonuniform", c.levels[0])
    seen = []

    def bp1(s):
        corr, _, _, post = orc.bp_decode_batch_soft(H, probs, 1, alpha, s, precision)
        assert np.array_equal(corr, orc.bp_decode_batch(H, probs, 1, "minimum_sum", alpha, s, precision)[0])
        seen.append(post)
        return corr

    corr, steps = firstmin_ref.decode(H, probs, fc.MAX_ITER, alpha, precision, S, bp1)
    assert not np.isfinite(np.concatenate(seen)).all()
    ref = firstmin_ref.decode(H, probs, fc.MAX_ITER, alpha, precision, S)
    assert np.array_equal(corr, ref[0]) and np.array_equal(steps, ref[1])


# ------------------------------------------------------------------------------------- the graphs
def test_switch_graphs_sit_on_either_side_of_the_wave_kernel():
    for name, total in (("lds_8192", 8192), ("lds_8193", 8193)):
        m, n, _ = fc.SWITCH[name].shape
        assert m + n == total
    assert fc.takes_wave(*fc.SWITCH["lds_8192"].shape[:2]) and not fc.takes_wave(*fc.SWITCH["lds_8193"].shape[:2])
    assert fc.CASES["xlds_2048"].source == "xlds_2048" and fc.graph("xlds_2048").shape[0] > 256  # two trips of the row loops
    assert fc.graph("col7_vpl2").shape[1] == 257


def test_switch_graph_is_balanced_with_column_degree_3():
    H = fc.graph("lds_8192")
    assert H.shape == (2731, 5461) and (H.sum(axis=0) == 3).all()
    rows = H.sum(axis=1)
    assert rows.max() - rows.min() <= 1
    S = fc.mixed("lds_8192", fc.B_SWITCH)
    assert S.shape == (fc.B_SWITCH, 2731) and S.any()


@pytest.mark.parametrize("name", list(fc.ENVELOPE))
def test_envelope_graphs_are_csr_with_three_distinct_rows_per_column(name):
    csr = fc.envelope_graph(name)
    m, n = fc.ENVELOPE[name]
    assert (csr.m, csr.n, csr.nnz) == (m, n, 3 * n) and m + n == int(name.split("_")[1])
    assert (csr.col_degrees() == 3).all()
    rows = np.repeat(np.arange(m), csr.row_degrees())
    assert len(set(zip(rows.tolist(), csr.col_idx.tolist()))) == 3 * n  # no edge twice: the rows are distinct
    for i in (0, 1, m - 1):
        r = csr.col_idx[csr.row_ptr[i]:csr.row_ptr[i + 1]]
        assert (np.diff(r) > 0).all()
    j = n - 1
    assert {int(i) for i in rows[csr.col_idx == j]} == {j % m, (7 * j + 1) % m, (13 * j + 5) % m}
    S = fc.envelope_syndromes(name)
    assert S.shape == (3, m) and S.any(axis=1).all()


def test_reuse_batch_cycles_and_shuffles_the_mixed_set():
    S, R = fc.mixed("a_i"), fc.reuse_batch("a_i", 2 * fc.B_MIXED + 3)
    key = lambda A: sorted(map(bytes, A))  # noqa: E731
    assert key(R) == key(np.vstack([S, S, S[:3]]))
    assert not np.array_equal(R[:fc.B_MIXED], S)


# --------------------------------------------------------------------------- the envelope arithmetic
def test_envelope_arithmetic():
    """wave <=> m + n <= 8192 (four syndromes' 2 (m + n) bytes, each rounded up to 16, in 64 KiB);
    admitted <=> 2 (m + n) + 16 <= 65536 (the workgroup kernel's arrays and its 16 static bytes)."""
    for t in list(range(1, 40)) + list(range(8150, 8240)) + list(range(32700, 32800)):
        for m in {1, t // 3, t - 1} - {0}:
            n = t - m
            if n < 1:
                continue
            assert fc.takes_wave(m, n) == (t <= 8192), t
            assert fc.admitted(m, n) == (2 * t + 16 <= 65536) == (t <= 32760), t
    assert fc.admitted(*fc.ENVELOPE["env_32760"]) and not fc.admitted(*fc.ENVELOPE["env_32768"])
    assert 2 * sum(fc.ENVELOPE["env_32768"]) == fc.LDS_LIMIT  # the dynamic LDS alone would still fit
    assert not fc.takes_wave(*fc.ENVELOPE["env_32760"])
    for c in fc.CASE_IDS:  # every table case is within the wave kernel's reach
        assert fc.takes_wave(*fc.graph(c).shape)

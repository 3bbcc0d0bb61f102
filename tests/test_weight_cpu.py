"""Fixed-weight error sampling and the stratified WER estimator, without a GPU.

* ``sample_errors_weight(host=True)`` (qldpc_sample_errors_weight_host, plain C++) against the law
  written in Python integers (tests/weight_ref.py), bit for bit;
* the law draws uniform subsets and classes in the requested ratio (chi-square);
* ``stratified_word_error_rate`` against exact rational arithmetic, and the window rule;
* the stratified estimate against direct sampling, both on the CPU oracle.
"""
import math
from fractions import Fraction
from itertools import combinations

import numpy as np
import pytest

import weight_ref
from qldpc_fault_tolerance_amd import codes, simulators
from qldpc_fault_tolerance_amd.engine import sample_errors_weight

SHAPES = [(1, 0), (1, 1), (63, 63), (64, 1), (65, 64), (225, 0), (225, 1), (225, 60), (225, 224), (225, 225),
          (1600, 16)]
RATIOS = [(1.0, 1.0, 1.0), (1.0, 0.0, 0.0), (0.01, 0.002, 0.03)]
S0 = 2 ** 32 - 64  # s_hi changes inside a 130-shot range


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("n,w", SHAPES)
def test_host_sampler_equals_the_law(oracle, n, w, ratio):
    px, py, pz = ratio
    S = 130
    got = sample_errors_weight(n, w, px, py, pz, seed=0x1234567ABCDEF01, shot_begin=S0, shot_count=S, host=True)
    ref = weight_ref.ref_errors(oracle, n, w, px, py, pz, 0x1234567ABCDEF01, S0, S)
    assert got.shape == (S, n) and got.dtype == np.uint8
    assert np.array_equal(got, ref)
    assert ((got != 0).sum(axis=1) == w).all()
    if ratio == (1.0, 0.0, 0.0):
        assert set(np.unique(got)) <= {0, 1}


def test_host_sampler_is_keyed_by_the_global_shot():
    a = sample_errors_weight(225, 12, 1, 1, 1, seed=5, shot_begin=1000, shot_count=300, host=True)
    b = sample_errors_weight(225, 12, 1, 1, 1, seed=5, shot_begin=1100, shot_count=200, host=True)
    assert np.array_equal(a[100:], b)
    c = sample_errors_weight(225, 12, 2, 2, 2, seed=5, shot_begin=1000, shot_count=300, host=True)
    assert np.array_equal(a, c)  # only the ratios matter
    d = sample_errors_weight(225, 12, 1, 1, 1, seed=6, shot_begin=1000, shot_count=300, host=True)
    assert not np.array_equal(a, d)


def test_host_sampler_rejects_bad_arguments():
    from qldpc_fault_tolerance_amd._native import QldpcError

    for kw in (dict(weight=-1), dict(weight=226), dict(px=0.0, py=0.0, pz=0.0), dict(px=-1.0)):
        args = dict(n=225, weight=3, px=1.0, py=1.0, pz=1.0, seed=1, shot_begin=0, shot_count=4, host=True)
        args.update(kw)
        with pytest.raises(QldpcError) as ei:
            sample_errors_weight(**args)
        assert ei.value.rc == -1  # QLDPC_EINVAL
    # weight 0 draws nothing, so all-zero probabilities are fine there
    z = sample_errors_weight(225, 0, 0.0, 0.0, 0.0, seed=1, shot_begin=0, shot_count=4, host=True)
    assert not z.any()


def test_law_is_uniform_over_subsets_and_classes():
    """n = 6, w = 3, 20,000 shots: chi-square over the 20 subsets < 43.82 (0.999 quantile, 19 dof)
    and over the three classes < 13.82 (0.999 quantile, 2 dof)."""
    px, py, pz = 0.01, 0.002, 0.03
    S = 20000
    e = sample_errors_weight(6, 3, px, py, pz, seed=1, shot_begin=0, shot_count=S, host=True)
    index = {c: i for i, c in enumerate(combinations(range(6), 3))}
    counts = np.zeros(20)
    for row in e:
        counts[index[tuple(np.flatnonzero(row))]] += 1
    chi_subsets = float(((counts - S / 20) ** 2 / (S / 20)).sum())
    T = px + py + pz
    cls = np.array([(e == 1).sum(), (e == 2).sum(), (e == 3).sum()], dtype=float)
    exp = 3 * S * np.array([px, pz, py]) / T
    chi_classes = float(((cls - exp) ** 2 / exp).sum())
    print(f"chi2 subsets {chi_subsets:.2f} classes {chi_classes:.2f}")
    assert chi_subsets < 43.82
    assert chi_classes < 13.82


# ------------------------------------------------------------------ estimator


class _Over:
    """Exact rationals over one fixed denominator (Fraction's gcds on 10^5-bit terms are slow)."""

    def __init__(self, nums, den):
        self.nums, self.den = nums, den

    def __getitem__(self, i):
        v = self.nums[i]
        return [Fraction(x, self.den) for x in v] if isinstance(i, slice) else Fraction(v, self.den)

    def sum(self, lo=0, hi=None):
        return Fraction(sum(self.nums[lo:hi]), self.den)


def _exact_pmf(n, p):
    """Binom(w; n, p) for the double p, exactly: numerators over the denominator b^n, p = a / b."""
    a, b = Fraction(p).as_integer_ratio()
    return _Over([math.comb(n, w) * a ** w * (b - a) ** (n - w) for w in range(n + 1)], b ** n)


def test_stratified_estimator_matches_exact_arithmetic():
    n, K, p = 225, 9, 0.06
    rng = np.random.default_rng(3)
    weights = np.arange(2, 41)
    shots = rng.integers(100, 4000, size=weights.size)
    fails = (shots * np.clip((weights - 1) / 30.0, 0, 1) * rng.random(weights.size)).astype(np.int64)
    fails[0] = 0
    d = simulators.stratified_word_error_rate(p, n, K, weights, fails, shots)
    B = _exact_pmf(n, p)
    f = [Fraction(int(a), int(b)) for a, b in zip(fails, shots)]
    ler = sum(B[w] * fw for w, fw in zip(weights, f))
    var = sum(B[w] ** 2 * fw * (1 - fw) / int(s) for w, fw, s in zip(weights, f, shots))
    unc = 1 - sum(B[w] for w in weights)
    assert d["ler"] == pytest.approx(float(ler), rel=1e-12)
    assert d["ler_eb"] == pytest.approx(math.sqrt(float(var)), rel=1e-12)
    assert d["uncovered"] == pytest.approx(float(unc), rel=1e-12)
    assert d["ler_upper"] == pytest.approx(float(ler + unc), rel=1e-12)
    assert d["wer"] == pytest.approx(1.0 - (1.0 - float(ler)) ** (1 / K), rel=1e-10)
    eb = math.sqrt(float(var))
    assert d["wer_eb"] == pytest.approx(eb * (1 - eb) ** (1 / K - 1) / K, rel=1e-12)
    assert d["min_failing_weight"] == int(weights[np.flatnonzero(fails > 0)[0]])
    # the same arithmetic as word_error_rate when one stratum carries all the mass
    one = simulators.stratified_word_error_rate(1.0, 4, 2, [4], [30], [100])
    wer, wer_eb = simulators.word_error_rate(30, 100, 2)
    assert one["wer"] == pytest.approx(wer, rel=1e-14) and one["wer_eb"] == pytest.approx(wer_eb, rel=1e-14)
    assert one["uncovered"] == 0.0
    none = simulators.stratified_word_error_rate(0.06, 225, 9, [3, 4], [0, 0], [10, 0])
    assert none["min_failing_weight"] is None and list(none["weights"]) == [3] and none["ler"] == 0.0


def test_stratified_estimator_is_finite_at_n1600():
    n, K, p = 1600, 64, 0.001
    B = simulators.binomial_pmf(n, p)
    assert np.isfinite(B).all() and (B >= 0).all()
    assert math.fsum(B) == pytest.approx(1.0, rel=1e-10)
    exact = _exact_pmf(n, p)
    for w in (0, 1, 2, 10, 40):
        assert B[w] == pytest.approx(float(exact[w]), rel=1e-11)
    prev = -1.0
    for top in (0, 1, 2, 4, 8, 16, 64, 400, 1600):  # f_w = 1 up to `top`: ler grows with the window
        w = np.arange(0, top + 1)
        d = simulators.stratified_word_error_rate(p, n, K, w, np.full(w.size, 10), np.full(w.size, 10))
        assert all(math.isfinite(d[k]) for k in ("ler", "ler_eb", "uncovered", "ler_upper", "wer", "wer_eb"))
        assert d["ler"] >= prev and 0.0 <= d["ler"] <= 1.0 + 1e-12
        prev = d["ler"]
    assert prev == pytest.approx(1.0, rel=1e-10)


@pytest.mark.parametrize("n,p,tail", [(225, 0.06, 1e-9), (225, 0.06, 1e-12), (1600, 0.001, 1e-12),
                                      (1600, 0.09, 1e-6), (12, 0.5, 1e-2), (5, 0.3, 1e-30)])
def test_window_rule_leaves_at_most_tail(n, p, tail):
    lo, hi = simulators.stratified_window(n, p, tail)
    assert 0 <= lo <= n * p <= hi <= n
    B = _exact_pmf(n, p)
    below, above = B.sum(0, lo), B.sum(hi + 1)
    slack = Fraction(1 + 1e-9)  # the pmf's own rounding
    assert below <= Fraction(tail) / 2 * slack and above <= Fraction(tail) / 2 * slack
    w = np.arange(lo, hi + 1)
    d = simulators.stratified_word_error_rate(p, n, 1, w, np.zeros(w.size, int), np.ones(w.size, int))
    assert d["uncovered"] <= tail * (1 + 1e-9)
    assert d["uncovered"] == pytest.approx(float(below + above), rel=1e-9, abs=1e-300)
    # not wider than needed: one weight less on either side breaks the bound
    if lo > 0:
        assert B.sum(0, lo + 1) > Fraction(tail) / 2 * (2 - slack)
    if hi < n:
        assert B.sum(hi) > Fraction(tail) / 2 * (2 - slack)


def test_window_of_the_issue():
    assert simulators.stratified_window(225, 0.06, 1e-9) == (0, 40)


def test_stratified_estimate_agrees_with_direct_sampling(oracle):
    """hgp_34_n225, p_tot = 0.06, decoder priors fixed: 1,500 fixed-weight reference shots per weight of
    the window 0 .. 40 (seed 11, shot index (w << 32) + s) against 40,000 direct shots (seed 99), both
    decoded by the CPU oracle.  The two LERs differ by at most 4.5 combined standard errors."""
    code = codes.get_code("hgp_34_n225")
    n, K = code.N, code.K
    px = py = pz = 0.02
    p_tot = px + py + pz
    lo, hi = simulators.stratified_window(n, p_tot, 1e-9)
    assert (lo, hi) == (0, 40)
    S = 1500
    weights = list(range(lo, hi + 1))
    fails = []
    for w in weights:
        e = weight_ref.ref_errors(oracle, n, w, px, py, pz, 11, w << 32, S)
        U = weight_ref.to_uniforms(e, px, py, pz)
        r = oracle.mc_run(code, px, py, pz, seed=0, shot_begin=0, shot_count=S, logical_mode="Total", max_iter=22,
                          probs_x=px + py, probs_z=pz + py, uniforms=U)
        fails.append(r["failures"])
    d = simulators.stratified_word_error_rate(p_tot, n, K, weights, fails, [S] * len(weights))
    direct = oracle.mc_run(code, px, py, pz, seed=99, shot_begin=0, shot_count=40000, logical_mode="Total",
                           max_iter=22, probs_x=px + py, probs_z=pz + py)
    ler = direct["failures"] / 40000
    eb = math.sqrt(ler * (1 - ler) / 40000)
    sigma = abs(d["ler"] - ler) / math.hypot(eb, d["ler_eb"])
    print(f"stratified {d['ler']:.5f} +- {d['ler_eb']:.5f}  direct {ler:.5f} +- {eb:.5f}  {sigma:.2f} sigma")
    assert d["uncovered"] <= 1e-9
    assert sigma <= 4.5

"""Characterisation of the host-side shot-loop plumbing of the simulators, without a GPU.

A stub device loop stands in for the HIP launch (the pattern of ``test_distributed_cpu.py``, in one
process): it records the non-tensor arguments of every launch and credits the launched shot range
with deterministic counts.  What is pinned: the seed and the shot ranges two consecutive
``fused_counts`` calls hand to the launch, the running ``_shot_offset``, ``last_result``, the lazy
64-bit seed, and where the adaptive ``WordErrorRate_TargetFailure`` loops stop and what they return.
"""
import itertools

import numpy as np
import pytest

from qldpc_fault_tolerance_amd import _native, codes, engine, simulators

PROBS = [0.01, 0.02, 0.03]
Q = 0.04


def _stub_counts(b, c):
    """Deterministic counters of the global shots [b, b + c): (shots, failures, iterations)."""
    idx = np.arange(b, b + c, dtype=np.int64)
    return c, int(np.sum(idx % 7 == 3)), int(np.sum(idx % 11))


class _StubLoop:
    """Stands in for engine.DevicePhenl / DeviceCircuit: counters on the CPU, every launch recorded."""

    device = 0

    def __init__(self):
        self.launched = []

    def new_counters(self):
        import torch

        return torch.zeros(_native.COUNTER_WORDS, dtype=torch.int64)

    def launch(self, *args):
        import torch

        plain = tuple(a for a in args if not isinstance(a, torch.Tensor))
        (counters,) = [a for a in args if isinstance(a, torch.Tensor)]
        self.launched.append(plain)
        # (seed, b, c) | (px, py, pz, seed, b, c, mode) | (px, py, pz, q, seed, b, c, num_rounds, mode)
        b, c = {3: plain[1:3], 7: plain[4:6], 9: plain[5:7]}[len(plain)]
        s, f, it = _stub_counts(b, c)
        counters[0] += s
        counters[1] += f
        counters[2] += s
        counters[4] += it


@pytest.fixture
def code():
    return codes.get_code("hgp_34_n225")


@pytest.fixture
def stub_torch(monkeypatch):
    class _T:
        cuda = type("C", (), {"synchronize": staticmethod(lambda *a, **k: None)})

    monkeypatch.setattr(engine, "_torch", lambda: _T)  # the stub counters live on the CPU


def _phenon(code, seed=5):
    return simulators.CodeSimulator_Phenon(code=code, pauli_error_probs=PROBS, q=Q, eval_logical_type="Total",
                                           seed=seed)


def _phenon_st(code, seed=5):
    return simulators.CodeSimulator_Phenon_SpaceTime(code=code, pauli_error_probs=PROBS, q=Q, eval_logical_type="Z",
                                                     num_rep=2, seed=seed)


def _circuit(code, seed=5):
    return simulators.CodeSimulator_Circuit(code=code, p=0.001, num_cycles=3, eval_logical_type="Z", seed=seed)


def _circuit_st(code, seed=5):
    return simulators.CodeSimulator_Circuit_SpaceTime(code=code, p=0.001, num_cycles=3, num_rep=1,
                                                      eval_logical_type="Z", seed=seed)


def _stubbed(make, code, seed=5):
    """(simulator with a stub device loop, the stub, the leading arguments of its fused_counts)."""
    sim = make(code, seed)
    stub = _StubLoop()
    sim._engine_parts = lambda: (object(), object(), object(), object())
    if make in (_phenon, _phenon_st):
        sim._ph = stub
        return sim, stub, (3,)  # num_rounds
    sim._device = lambda: stub
    return sim, stub, ()


def _check_result(res, b, c):
    s, f, it = _stub_counts(b, c)
    assert isinstance(res, engine.MCResult)
    assert (res.shots, res.failures, res.sector_decodes[0], res.sector_iters[0]) == (s, f, s, it)


@pytest.mark.parametrize("make", [_phenon, _phenon_st, _circuit, _circuit_st])
def test_fused_counts_launches_consecutive_shot_ranges(make, code, stub_torch):
    sim, stub, lead = _stubbed(make, code)
    r1 = sim.fused_counts(*lead, 100)
    assert sim.last_result is r1
    r2 = sim.fused_counts(*lead, 50)
    assert sim.last_result is r2
    if lead:
        px, py, pz = PROBS
        assert stub.launched == [(px, py, pz, Q, 5, 0, 100, 3, sim.eval_logical_type),
                                 (px, py, pz, Q, 5, 100, 50, 3, sim.eval_logical_type)]
    else:
        assert stub.launched == [(5, 0, 100), (5, 100, 50)]
    assert sim._shot_offset == 150
    _check_result(r1, 0, 100)
    _check_result(r2, 100, 50)


@pytest.mark.parametrize("make", [_phenon, _phenon_st, _circuit, _circuit_st])
def test_fused_counts_needs_engine_decoders(make, code, stub_torch):
    sim, stub, lead = _stubbed(make, code)
    sim._engine_parts = lambda: None
    with pytest.raises(TypeError, match="fused path needs engine"):
        sim.fused_counts(*lead, 10)
    assert stub.launched == [] and sim._shot_offset == 0 and sim.last_result is None


@pytest.mark.parametrize("make", [_phenon, _phenon_st, _circuit, _circuit_st])
def test_batch_failures_goes_through_the_fused_path(make, code, stub_torch):
    sim, stub, lead = _stubbed(make, code)
    if make is _phenon:  # the single-shot simulator keeps its own name for the same step
        assert sim.WordErrorProbability(3, 100) == simulators.word_error_rate(_stub_counts(0, 100)[1], 100, sim.K)
    else:
        assert sim._batch_failures(*lead, 100) == _stub_counts(0, 100)[1]
    assert sim._shot_offset == 100


@pytest.mark.parametrize("make", [_phenon_st, _circuit_st])
def test_lazy_seed_is_drawn_once(make, code, stub_torch):
    sim, stub, lead = _stubbed(make, code, seed=None)
    assert sim.seed is None
    sim.fused_counts(*lead, 10)
    seed = sim.seed
    assert isinstance(seed, int) and 0 <= seed < 2 ** 64
    sim.fused_counts(*lead, 10)
    assert sim.seed == seed
    assert [a[4 if lead else 0] for a in stub.launched] == [seed, seed]
    assert sim._shot_offset == 20


def test_lazy_seed_comes_from_python_random(code, stub_torch):
    import random

    sim = simulators.CodeSimulator_DataError(code=code, pauli_error_probs=PROBS, eval_logical_type="Total")
    stub = _StubLoop()
    sim._engine_ready = lambda: (True, object(), object())
    sim._mc = stub
    state = random.getstate()
    try:
        random.seed(1234)
        want = random.getrandbits(64)
        random.seed(1234)
        sim.fused_counts(10)
    finally:
        random.setstate(state)
    assert sim.seed == want
    assert stub.launched == [(*PROBS, want, 0, 10, "Total")]


# ------------------------------------------------------------------------------- adaptive loop


def _data_error(code):
    return simulators.CodeSimulator_DataError(code=code, pauli_error_probs=PROBS, eval_logical_type="Total", seed=5)


def _feed(sim, fails, lead=0):
    """Replace ``_batch_failures`` by a stub that hands out ``fails`` in turn and records its arguments."""
    calls = []
    it = iter(fails)

    def batch_failures(*args):
        assert len(args) == lead + 1
        calls.append(args)
        return next(it)

    sim._batch_failures = batch_failures
    return calls


SEQ = [1, 0, 2, 4, 9, 9]


@pytest.mark.parametrize("target, max_batches, batches", [(3, 6, 3), (7, 6, 4), (1, 6, 1), (100, 5, 5), (2, 2, 2)])
def test_target_failure_data_error(code, target, max_batches, batches):
    sim = _data_error(code)
    calls = _feed(sim, SEQ)
    wer, total = sim.WordErrorRate_TargetFailure(target_failures=target, batch_size=40, max_batches=max_batches)
    assert calls == [(40,)] * batches
    assert total == 40 * batches
    assert wer == simulators.word_error_rate(sum(SEQ[:batches]), total, sim.K)[0]


@pytest.mark.parametrize("target, max_batches, batches", [(3, 6, 3), (7, 6, 4), (100, 5, 5)])
def test_target_failure_phenon_spacetime(code, target, max_batches, batches):
    sim = _phenon_st(code)
    calls = _feed(sim, SEQ, lead=1)
    wer, total = sim.WordErrorRate_TargetFailure(num_cycles=5, target_failures=target, batch_size=40,
                                                 max_batches=max_batches)
    assert calls == [(3, 40)] * batches  # num_rounds = (5 - 1) / num_rep + 1
    assert total == 40 * batches
    assert wer == simulators.word_error_rate_per_cycle(sum(SEQ[:batches]), total, sim.K, 5)


@pytest.mark.parametrize("target, max_batches, batches", [(3, 6, 3), (7, 6, 4), (100, 5, 5)])
def test_target_failure_circuit_spacetime(code, capsys, target, max_batches, batches):
    sim = _circuit_st(code)
    calls = _feed(sim, SEQ)
    wer, total = sim.WordErrorRate_TargetFailure(target_failures=target, batch_size=40, max_batches=max_batches)
    assert calls == [(40,)] * batches
    assert total == 40 * batches
    assert wer == simulators.word_error_rate_per_cycle(sum(SEQ[:batches]), total, sim.K, sim.num_cycles)
    assert capsys.readouterr().out == f"failures: {sum(SEQ[:batches])}\n"


def test_target_failure_circuit_spacetime_needs_odd_cycles(code):
    sim = simulators.CodeSimulator_Circuit_SpaceTime(code=code, p=0.001, num_cycles=4, num_rep=1, seed=5)
    calls = _feed(sim, itertools.repeat(1))
    with pytest.raises(AssertionError):
        sim.WordErrorRate_TargetFailure(target_failures=1, batch_size=10, max_batches=2)
    assert calls == []

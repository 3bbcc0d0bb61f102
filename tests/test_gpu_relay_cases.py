"""GPU tests of the Relay-BP kernel (csrc/relay.hip, engine 7) on the pinning inputs of
tests/relay_cases.py: irregular graphs under priors on both sides of 0.5, the frozen syndromes whose
chains choose among several solutions, and the graphs at the edges of every geometry decision
``qldpc_bp_create_relay`` takes on its own.

The checker is the host law (``qldpc_relay_decode_host`` / ``qldpc_relay_decode_host_side``, plain C++),
which tests/test_relay_cases_cpu.py pins to the Python law on these inputs; the kernel must equal it bit
for bit in corrections, iteration counts and convergence flags.
"""
import numpy as np
import pytest

import relay_cases as rc
from qldpc_fault_tolerance_amd import _native
from qldpc_fault_tolerance_amd.engine import DeviceBP, RelayParams, relay_decode_host, relay_decode_host_side

pytestmark = pytest.mark.gpu

ENOTSUP = -4
# (precision, messages forced into the HBM workspace, indices staged in LDS where the handle would)
MODES = [(p, ws, idx) for p in (64, 32) for ws in (False, True) for idx in (True, False)]
MODE_IDS = [f"f{p}-{'ws' if ws else 'lds'}-{'idx' if idx else 'walk'}" for p, ws, idx in MODES]
CHOICE_RELAY = RelayParams(**rc.relay_kwargs(rc.CHOICE_SETTING))
GEO_RELAY = RelayParams(**rc.GEO_RELAY)

_cache = {}


def _host(key, H, probs, relay, synd, alpha, precision):
    """The host law's (corr, iters, conv), once per ``key``."""
    key = ("host", key, relay, alpha, precision)
    if key not in _cache:
        _cache[key] = relay_decode_host(H, probs, relay, synd, ms_scaling_factor=alpha, precision=precision)[:3]
    return _cache[key]


def _host_side(key, H, p0, p1, relay, synd, side, alpha, precision):
    key = ("side", key, relay, alpha, precision)
    if key not in _cache:
        _cache[key] = relay_decode_host_side(H, p0, p1, relay, synd, side, ms_scaling_factor=alpha,
                                             precision=precision)[:3]
    return _cache[key]


def _equal(got, ref):
    assert np.array_equal(got[0], ref[0])
    assert np.array_equal(got[1], ref[1])
    assert np.array_equal(got[2], ref[2])


def _decoder(H, probs, relay, precision, ws, idx, monkeypatch, alpha=0.625):
    monkeypatch.setenv("QLDPC_RELAY_WS", "1" if ws else "0")
    monkeypatch.setenv("QLDPC_RELAY_IDX", "1" if idx else "0")
    dec = DeviceBP(H, probs, ms_scaling_factor=alpha, precision=precision, relay=relay)
    geo = dec.geometry()
    assert geo["engine"] == 7 and geo["threads"] in (256, 512, 1024) and geo["blocks_per_cu"] >= 1
    assert 0 < geo["lds_bytes"] <= rc.LDS_MAX
    return dec


# ------------------------------------------------------------------ irregular graphs
@pytest.mark.parametrize("precision,ws,idx", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case_id", rc.IRREGULAR_IDS)
def test_irregular_graphs_equal_host_law(gpu, monkeypatch, case_id, precision, ws, idx):
    """Every prior kind (``flipped``: negative L0 and weights) under every (setting, alpha) pair:
    stop_nconv 1, 2 and 8, both alpha schedules; B = 96 and B = 1."""
    H = rc.graph(case_id)
    synd = rc.mixed(case_id, rc.B_IRREGULAR)
    for kind in rc.PRIORS:
        probs = rc.priors(case_id, kind)
        for setting, alpha in rc.PAIRS:
            relay = RelayParams(**rc.relay_kwargs(setting))
            dec = _decoder(H, probs, relay, precision, ws, idx, monkeypatch, alpha)
            ref = _host((case_id, kind), H, probs, relay, synd, alpha, precision)
            _equal(dec.decode_batch(synd), ref)
            _equal(dec.decode_batch(synd[5:6]), [r[5:6] for r in ref])


# ------------------------------------------------------------------ the choice among several solutions
@pytest.mark.parametrize("precision,ws,idx", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("entry", rc.CHOICE, ids=rc.CHOICE_IDS)
def test_solution_choice_set_equals_host_law(gpu, monkeypatch, entry, precision, ws, idx):
    """Chains that replace a solution by a lighter one, keep the earlier one on a tie and keep it against
    a heavier one (tests/test_relay_cases_cpu.py counts them under the Python law)."""
    case_id, kind, _ = entry
    H, probs, synd = rc.graph(case_id), rc.priors(case_id, kind), rc.choice_syndromes(entry)
    dec = _decoder(H, probs, CHOICE_RELAY, precision, ws, idx, monkeypatch, rc.CHOICE_ALPHA)
    ref = _host(("choice", case_id, kind), H, probs, CHOICE_RELAY, synd, rc.CHOICE_ALPHA, precision)
    _equal(dec.decode_batch(synd), ref)
    for b in range(len(synd)):  # B = 1
        _equal(dec.decode_batch(synd[b:b + 1]), [r[b:b + 1] for r in ref])


@pytest.mark.parametrize("precision,ws", [(64, False), (64, True), (32, False), (32, True)],
                         ids=["f64-lds", "f64-ws", "f32-lds", "f32-ws"])
def test_a_workgroup_decodes_replaced_tied_and_unsolved_in_turn(gpu, monkeypatch, precision, ws):
    """More syndromes than the persistent grid has workgroups, on row33 / nonuniform: the frozen
    ``replaced`` / ``tie_kept`` / ``heavier_kept`` syndromes and unsolved ones, cycled with a period
    coprime to the grid, so that each workgroup meets all of them and a weight word, a best vector or
    a solution count left over from the previous syndrome shows."""
    import torch

    entry = next(e for e in rc.CHOICE if e[:2] == rc.CHOICE_UNSOLVED[:2])
    case_id, kind, _ = entry
    H, probs = rc.graph(case_id), rc.priors(case_id, kind)
    base = np.concatenate([rc.choice_syndromes(entry), rc.choice_syndromes(rc.CHOICE_UNSOLVED)])[:13]
    assert len(base) == 13 and len(entry[2]) < 13  # 13: coprime to a grid of (a small factor) x (the CUs)
    dec = _decoder(H, probs, CHOICE_RELAY, precision, ws, True, monkeypatch, rc.CHOICE_ALPHA)
    grid = dec.geometry()["blocks_per_cu"] * torch.cuda.get_device_properties(0).multi_processor_count
    assert grid % 13 != 0
    B = 3 * grid + 7
    ref13 = _host(("reuse", case_id, kind), H, probs, CHOICE_RELAY, base, rc.CHOICE_ALPHA, precision)
    assert ref13[2].any() and (~ref13[2]).any()
    pick = np.arange(B) % 13
    got = dec.decode_batch(np.ascontiguousarray(base[pick]))
    _equal(got, [r[pick] for r in ref13])


def test_set_channel_probs_from_uniform_to_flipped(gpu, monkeypatch):
    case_id = "row33"
    H, synd = rc.graph(case_id), rc.mixed(case_id, rc.B_IRREGULAR)
    for precision in rc.PRECISIONS:
        dec = _decoder(H, rc.priors(case_id, "uniform"), CHOICE_RELAY, precision, False, True, monkeypatch)
        first = dec.decode_batch(synd)
        dec.set_channel_probs(rc.priors(case_id, "flipped"))
        second = dec.decode_batch(synd)
        fresh = _decoder(H, rc.priors(case_id, "flipped"), CHOICE_RELAY, precision, False, True, monkeypatch)
        _equal(second, fresh.decode_batch(synd))
        _equal(second, _host((case_id, "flipped", "set"), H, rc.priors(case_id, "flipped"), CHOICE_RELAY, synd, 0.625,
                             precision))
        assert not np.array_equal(first[0], second[0])


# ------------------------------------------------------------------ geometry decisions, no switch set
@pytest.mark.parametrize("precision", rc.PRECISIONS)
@pytest.mark.parametrize("geo_id", rc.GEO_IDS)
def test_geometry_cases_without_a_switch(gpu, monkeypatch, geo_id, precision):
    """What the handle decides on its own equals the table; every admitted graph launches (with up to
    160 KiB of dynamic LDS and 1024 threads) and equals the host law; one step past the envelope is
    QLDPC_ENOTSUP at creation."""
    monkeypatch.delenv("QLDPC_RELAY_WS", raising=False)
    monkeypatch.delenv("QLDPC_RELAY_IDX", raising=False)
    g, H = rc.GEO[geo_id], rc.geo_graph(geo_id)
    probs, synd = rc.geo_priors(geo_id), rc.geo_syndromes(geo_id)
    want = g.expected(precision)
    if want is None:
        with pytest.raises(_native.QldpcError) as ei:
            DeviceBP(H, probs, precision=precision, relay=GEO_RELAY)
        assert ei.value.rc == ENOTSUP and "graph too large" in str(ei.value)
        return
    dec = DeviceBP(H, probs, precision=precision, relay=GEO_RELAY)
    geo = dec.geometry()
    assert geo["engine"] == 7
    assert (geo["threads"], geo["lds_bytes"]) == want[2:] and geo["blocks_per_cu"] >= 1
    assert geo["vars_per_thread"] == -(-g.n // want[2])
    got = dec.decode_batch(synd)
    ref = _host(("geo", geo_id), H, probs, GEO_RELAY, synd, 0.625, precision)
    _equal(got, ref)
    assert ref[2][0] and ref[2].any()
    _equal(dec.decode_batch(synd[3:4]), [r[3:4] for r in ref])


# ------------------------------------------------------------------ side decodes
@pytest.mark.parametrize("precision,ws,idx", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("entry", rc.CHOICE, ids=rc.CHOICE_IDS)
def test_side_decode_of_the_solution_choice_set(gpu, monkeypatch, entry, precision, ws, idx):
    """Per-syndrome priors and weights from two tables of different kinds; three of these decodes keep a
    solution that row 0's weights alone would not keep (tests/test_relay_cases_cpu.py)."""
    H, p0, p1, synd, side = rc.side_case(entry)
    dec = _decoder(H, p0, CHOICE_RELAY, precision, ws, idx, monkeypatch, rc.CHOICE_ALPHA)
    dec.set_side_probs(p0, p1)
    ref = _host_side(entry[:2], H, p0, p1, CHOICE_RELAY, synd, side, rc.CHOICE_ALPHA, precision)
    _equal(dec.decode_batch(synd, side), ref)
    _equal(dec.decode_batch(synd[-1:], side[-1:]), [r[-1:] for r in ref])
    # the plain decode of the same handle is untouched
    _equal(dec.decode_batch(synd), _host(("choice", entry[0], entry[1]), H, p0, CHOICE_RELAY, synd, rc.CHOICE_ALPHA,
                                         precision))


@pytest.mark.parametrize("precision", rc.PRECISIONS)
@pytest.mark.parametrize("geo_id", rc.GEO_SIDE_IDS)
def test_side_decode_on_geometry_cases(gpu, monkeypatch, geo_id, precision):
    monkeypatch.delenv("QLDPC_RELAY_WS", raising=False)
    monkeypatch.delenv("QLDPC_RELAY_IDX", raising=False)
    g, H = rc.GEO[geo_id], rc.geo_graph(geo_id)
    p0, p1, synd = rc.geo_priors(geo_id), rc.geo_priors(geo_id, "flipped"), rc.geo_syndromes(geo_id)
    side = rc.side_bytes([g.seed, 6], len(synd), g.n, 0.05)
    dec = DeviceBP(H, p0, precision=precision, relay=GEO_RELAY)
    dec.set_side_probs(p0, p1)
    want = g.expected(precision)
    geo = dec.geometry()
    assert (geo["threads"], geo["lds_bytes"]) == want[2:]
    _equal(dec.decode_batch(synd, side), _host_side(("geo", geo_id), H, p0, p1, GEO_RELAY, synd, side, 0.625, precision))

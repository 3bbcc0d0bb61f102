"""The BP+LSD case table (tests/lsd_cases.py) on the GPU: the cluster kernel (csrc/lsd.hip) equals the
host stage bit for bit, for x and the statistics, on every graph, posterior kind and syndrome kind, with
the active image in LDS and forced to the HBM slice, at B = 1, B = 96 and a batch larger than the
persistent grid in which each workgroup meets solvable, unsolvable, all-zero and converged entries in
turn.  The geometry of each case is asserted against the restated accounting (lsd_cases.expected).
"""
import numpy as np
import pytest

import lsd_cases
from qldpc_fault_tolerance_amd.engine import DeviceGraph, DeviceLSD, HostLSD

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
_HOST = {}


def host(case_id, k):
    """(x, stats) of the host stage on every syndrome of a case, once per case and k."""
    if (case_id, k) not in _HOST:
        S, P, _ = lsd_cases.inputs(case_id)
        _HOST[case_id, k] = HostLSD(lsd_cases.graph(case_id), k).decode_batch_stats(S, P)
    return _HOST[case_id, k]


def device(monkeypatch, case_id, k, ws):
    """The GPU handle of a case with its geometry asserted against the restated accounting."""
    m, n = lsd_cases.graph(case_id).shape
    if ws:
        monkeypatch.setenv("QLDPC_LSD_WS", "1")
    lsd = DeviceLSD(DeviceGraph(lsd_cases.graph(case_id)), k)
    geo = lsd.geometry()
    want = dict(lsd_cases.expected(m, n))
    if ws:
        want["lds_rows"] = 0  # no image in LDS: the tables (and the sort under them) alone
    assert 1 <= geo["workgroups"] <= want["grid_bound"]
    for key in ("row_words", "window_words", "threads", "lds_rows"):
        assert geo[key] == want[key], (key, geo)
    if not ws:
        assert geo["lds_bytes"] == want["lds_bytes"] <= lsd_cases.LDS_MAX
    return lsd, geo


@pytest.mark.parametrize("ws", [False, True], ids=["lds", "ws"])
@pytest.mark.parametrize("k", lsd_cases.KS)
@pytest.mark.parametrize("case_id", lsd_cases.CASE_IDS)
def test_kernel_equals_the_host_stage(gpu, monkeypatch, case_id, k, ws):
    n = lsd_cases.graph(case_id).shape[1]
    S, P, inc = lsd_cases.inputs(case_id)
    X, T = host(case_id, k)
    lsd, _ = device(monkeypatch, case_id, k, ws)
    # B = whole batch (every syndrome, the inconsistent ones at every k), B = 1
    x, st = lsd.decode_batch_stats(S, P)
    assert np.array_equal(st, T) and np.array_equal(x, X)
    assert np.array_equal(st[:, 0] == 0, inc)
    x1, st1 = lsd.decode_batch_stats(S[:1], P[:1])
    assert np.array_equal(x1, X[:1]) and np.array_equal(st1, T[:1])
    # B = 96 with converged entries
    rep = np.resize(np.arange(S.shape[0]), 96)
    conv = (np.arange(96) % 5 == 3).astype(np.uint8)
    bp = np.full((96, n), 1, np.uint8)
    x96, st96 = lsd.decode_batch_stats(S[rep], P[rep], conv, bp)
    c = conv.astype(bool)
    assert np.array_equal(x96[~c], X[rep][~c]) and np.array_equal(st96[~c], T[rep][~c])
    assert (x96[c] == 1).all() and (st96[c] == (1, 0, 0, 0)).all()
    if case_id == "fit_over" and not ws:
        # the swallowing syndromes outgrew the LDS image and ran again on the HBM slice
        lsd.retries()
        lsd.decode_batch_stats(S, P)
        assert lsd.retries() >= int(inc.sum()) >= 1
    if case_id == "fit_exact" and not ws:
        lsd.retries()
        lsd.decode_batch_stats(S, P)
        assert lsd.retries() == 0, "the image holds every row"


@pytest.mark.parametrize("ws", [False, True], ids=["lds", "ws"])
@pytest.mark.parametrize("k", lsd_cases.KS)
@pytest.mark.parametrize("case_id", lsd_cases.CASE_IDS)
def test_batch_larger_than_the_grid(gpu, monkeypatch, case_id, k, ws):
    """Every workgroup of the persistent grid meets every kind of entry in turn and re-initialises its
    state, LDS image or HBM slice: the batch cycles through the case's syndromes (solvable, all-zero,
    unsolvable where the graph has them) and converged entries, with a stride coprime to the cycle."""
    import torch

    n = lsd_cases.graph(case_id).shape[1]
    S, P, inc = lsd_cases.inputs(case_id)
    X, T = host(case_id, k)
    lsd, geo = device(monkeypatch, case_id, k, ws)
    grid = geo["workgroups"]
    B = grid + grid // 2 + 37
    nb = S.shape[0]
    idx = (np.arange(B) * 7) % nb if nb % 7 else (np.arange(B) * 5) % nb
    conv = ((np.arange(B) + np.arange(B) // grid) % 4 == 1).astype(np.uint8)
    bp = ((np.arange(B)[:, None] + np.arange(n)[None, :]) % 3 == 0).astype(np.uint8)
    dev = torch.device("cuda", lsd.graph.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out0 = torch.full((B, n), SENTINEL, dtype=torch.uint8, device=dev)
    outw = torch.full((B, n), SENTINEL, dtype=torch.uint8, device=dev)
    lsd.decode_device(up(S[idx]), up(P[idx]), up(conv), up(bp), out0, outw)  # qldpc_osd_gpu_decode
    torch.cuda.synchronize(dev)
    c = conv.astype(bool)
    want = np.where(c[:, None], bp, X[idx])
    assert np.array_equal(outw.cpu().numpy(), want) and np.array_equal(out0.cpu().numpy(), want)
    kinds = {(bool(T[i, 0]), bool(S[i].any())) for i in idx[~c]}
    need = {(True, False)} | ({(True, True)} if S[~inc].any() else set()) | ({(False, True)} if inc.any() else set())
    assert need <= kinds and c.any()


def test_envelope(gpu):
    from qldpc_fault_tolerance_amd import _native

    wide = np.zeros((1, 8193), np.uint8)
    wide[0, 0] = 1
    for H in (wide, np.ascontiguousarray(wide.T)):  # n > 8192, m > 8192
        with pytest.raises(_native.QldpcError) as e:
            DeviceLSD(DeviceGraph(H), 1)
        assert e.value.rc == _native.ENOTSUP
    with pytest.raises(_native.QldpcError) as e:
        DeviceLSD(DeviceGraph(np.ones((2, 2), np.uint8)), 0)
    assert e.value.rc == _native.EINVAL

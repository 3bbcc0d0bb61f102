"""NumPy restatement of the single-shot circuit loop (TEST INFRASTRUCTURE ONLY).

``CodeSimulator_Circuit._decoding_samples`` (``src/Simulators.py:612-644``) for a batch of samples, on
the CPU oracle's decoders (``oracle.bp_decode_batch`` / ``bp_decode_batch_soft`` / ``osd_decode_batch``)
and the oracle's DEM sampler (``circuit_oracle.sample_mechanisms``)::

    corr = 0; res = 0
    for j in 0 .. num_cycles-2:
        s  = hist[j] ^ res
        c  = decoder1.decode(s)            # on [hx | I], n + m variables
        corr ^= c[:n]
        res = s ^ hx c[:n]                 # identity part NOT applied
    s_f = hist[-1] ^ res
    c2  = decoder2.decode(s_f)
    fail = (s_f ^ hx c2).any() or (obs ^ lx (corr ^ c2)).any()

It also returns what the device loop counts (decodes, iterations, non-converged decodes per decoder)
and how many samples carried a non-zero residual into some cycle: a test whose carry is always zero
would not see a wrong carry.  The codes, noise settings and priors of the tests live here too, shared
by the fixture generator (``tests/golden/make_golden_circuit_single_shot.py``) and both test files.
"""
from __future__ import annotations

import os

import numpy as np

import circuit_oracle
import oracle

from qldpc_fault_tolerance_amd import codes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_circuit_single_shot.npz")
ALPHA = 0.625
SEED, SHOT_BEGIN, SAMPLES = 7, 4242, 1500
ALL_NOISE = {"p_i": 1.0, "p_state_p": 1.0, "p_m": 1.0, "p_CX": 1.0, "p_idling_gate": 1.0}
CX_ONLY = {"p_i": 0.0, "p_state_p": 0.0, "p_m": 0.0, "p_CX": 1.0, "p_idling_gate": 0.0}
# (tag, code name, eval_logical_type, num_cycles, noise scales, p) of the golden fixture
GOLDEN_CASES = [
    ("tor_z5", "tor", "Z", 5, ALL_NOISE, 3e-3),
    ("asym_x5", "asym", "X", 5, ALL_NOISE, 3e-3),
    ("tor_z2cx", "tor", "Z", 2, CX_ONLY, 3e-3),
]


def ring(d):
    h = np.zeros((d, d), np.uint8)
    for i in range(d):
        h[i, i] = h[i, (i + 1) % d] = 1
    return h


def make_code(name):
    """``tor``: hgp(ring3, ring3), 18 qubits, 9 + 9 checks, K = 2.  ``asym``: hgp(ring3, [[1,1,0],[0,1,1]]),
    15 qubits, hx 9 x 15, hz 6 x 15, K = 1 (two sectors of different shapes)."""
    if name == "tor":
        return codes.hgp(ring(3), ring(3))
    if name == "asym":
        return codes.hgp(ring(3), np.array([[1, 1, 0], [0, 1, 1]], np.uint8))
    return codes.get_code(name)


def error_params(scales, p):
    return {k: v * p for k, v in scales.items()}


def priors1(n, m, p):
    """The Threshold notebook's decoder1 priors on [h | I]: p_data = 3 * 6 * (8/15) p on the n data
    columns, p_synd = 7 * (8/15) p on the m identity columns."""
    return np.hstack([3 * 6 * (8 / 15) * p * np.ones(n), 7 * (8 / 15) * p * np.ones(m)])


def ext(h):
    h = np.asarray(h, np.uint8) % 2
    return np.hstack([h, np.identity(h.shape[0], dtype=np.uint8)])


def firstmin_batch(h, probs, max_iter, synd):
    """``FirstMinBPDecoder.decode`` (``src/Decoders.py:60-74``) for a batch: one-iteration min-sum BP
    repeated on the running syndrome while its weight does not grow, at most ``max_iter`` accepted
    steps.  -> (corrections, accepted steps)."""
    h = np.asarray(h, np.uint8)
    hi = h.astype(np.int64)
    cur = np.asarray(synd, np.uint8).copy()
    B = cur.shape[0]
    corr = np.zeros((B, h.shape[1]), np.int64)
    steps = np.zeros(B, np.int64)
    active = np.ones(B, bool)
    new = np.zeros((B, h.shape[1]), np.int64)
    nsyn = np.zeros_like(cur)
    while active.any():
        idx = np.flatnonzero(active)
        c, _, _ = oracle.bp_decode_batch(h, probs, 1, "minimum_sum", ALPHA, cur[idx], 64)
        new[idx] = c
        nsyn[idx] = ((c.astype(np.int64) @ hi.T + cur[idx]) % 2).astype(np.uint8)
        ok = active & (nsyn.sum(1) <= cur.sum(1)) & (steps < max_iter)
        cur[ok] = nsyn[ok]
        corr[ok] = (corr[ok] + new[ok]) % 2
        steps[ok] += 1
        active = ok
    return corr, steps


def decode_samples(det, logical, hx, lx, p1, p2, max_iter1, max_iter2, num_cycles, final_osd=True, firstmin=False,
                   osd_method="osd_e", osd_order=10):
    """The loop of the module docstring on sampled detector / observable bits [S, num_cycles * m] /
    [S, K].  ``firstmin``: decoder1 is ``FirstMinBPDecoder`` (accepted steps count as iterations,
    nothing as non-converged: the device loop's convention)."""
    hx = np.asarray(hx, np.uint8) % 2
    lx = np.asarray(lx, np.int64) % 2
    hxi = hx.astype(np.int64)
    m, n = hx.shape
    h1 = ext(hx)
    det = np.asarray(det, np.int64)
    S = det.shape[0]
    assert det.shape[1] == num_cycles * m
    corr = np.zeros((S, n), np.int64)
    res = np.zeros((S, m), np.int64)
    carried = np.zeros(S, bool)
    it1 = nc1 = 0
    for j in range(num_cycles - 1):
        carried |= res.any(axis=1)
        s = (det[:, j * m:(j + 1) * m] + res) % 2
        if firstmin:
            c, it = firstmin_batch(h1, p1, max_iter1, s.astype(np.uint8))
        else:
            c, it, cv = oracle.bp_decode_batch(h1, np.asarray(p1), max_iter1, "minimum_sum", ALPHA, s.astype(np.uint8), 64)
            nc1 += int((~cv).sum())
        it1 += int(np.asarray(it, np.int64).sum())
        c = c.astype(np.int64)[:, :n]
        corr = (corr + c) % 2
        res = (s + c @ hxi.T) % 2
    carried |= res.any(axis=1)
    sf = ((det[:, (num_cycles - 1) * m:] + res) % 2).astype(np.uint8)
    if final_osd:
        bp, it2, cv2, post = oracle.bp_decode_batch_soft(hx, np.asarray(p2), max_iter2, ALPHA, sf, 64)
        _, osdw = oracle.osd_decode_batch(hx, np.asarray(p2), sf, post, osd_method, osd_order)
        c2 = np.where(cv2[:, None].astype(bool), bp, osdw).astype(np.int64)
    else:
        c2, it2, cv2 = oracle.bp_decode_batch(hx, np.asarray(p2), max_iter2, "minimum_sum", ALPHA, sf, 64)
        c2 = c2.astype(np.int64)
    res_syn = (sf + c2 @ hxi.T) % 2
    res_log = (np.asarray(logical, np.int64) + (corr + c2) @ lx.T) % 2
    fail = (res_syn.any(axis=1) | res_log.any(axis=1)).astype(np.uint8)
    return {"fail": fail, "failures": int(fail.sum()), "carried": int(carried.sum()),
            "sector_decodes": [S * (num_cycles - 1), S],
            "sector_iters": [it1, int(np.asarray(it2, np.int64).sum())],
            "sector_nonconv": [nc1, int((~np.asarray(cv2, bool)).sum())]}


def sample(dem, seed, shot_begin, shot_count):
    """(detector bits [S, D], observable bits [S, K]) of the oracle's geometric-skip sampler."""
    e = circuit_oracle.sample_mechanisms(dem.probs, seed, shot_begin, shot_count).astype(np.int64)
    det = (e @ dem.check_matrix().T.astype(np.int64)) % 2
    obs = (e @ dem.observable_matrix().T.astype(np.int64)) % 2
    return det.astype(np.uint8), obs.astype(np.uint8)


def run(dem, hx, lx, p1, p2, max_iter1, max_iter2, num_cycles, seed=SEED, shot_begin=SHOT_BEGIN, shot_count=SAMPLES,
        **kw):
    det, obs = sample(dem, seed, shot_begin, shot_count)
    out = decode_samples(det, obs, hx, lx, p1, p2, max_iter1, max_iter2, num_cycles, **kw)
    out["det"], out["logical"] = det, obs
    return out


_CACHE = {}


def cached_run(key, fn):
    """One restatement per configuration and test session, shared (and left unchanged) by the tests."""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def golden_ops(z, tag):
    """[(gate, argument or nan, targets)] of a fixture tag."""
    names, args = z[f"{tag}_names"], z[f"{tag}_args"]
    offs, tg = z[f"{tag}_offs"], z[f"{tag}_targets"]
    return [(str(names[i]), float(args[i]), [int(t) for t in tg[offs[i]:offs[i + 1]]]) for i in range(len(names))]

"""Reference for the fixed-weight error sampler (helper, not a test).

``ref_errors`` is the sampling law of ``qldpc_mc_launch_weight`` (csrc/weight.hip, include/qldpc_hip.h)
written in Python integers over the oracle's Philox4x32-10.  ``to_uniforms`` encodes an error as
uniforms of the reference's three-way split, so ``oracle.mc_run(..., uniforms=U, probs_x=...,
probs_z=..., per_shot=True)`` is the per-shot oracle of any fixed-weight batch.
"""
import math

import numpy as np

STREAM_WEIGHT = 0x51D50006


def thresholds(px, py, pz):
    """(K1, K2) = (ceil(2^53 pz / T), ceil(2^53 (pz + px) / T)), T = (pz + px) + py, in doubles."""
    px, py, pz = float(px), float(py), float(pz)
    T = (pz + px) + py

    def ceil53(t):
        if not t > 0.0:
            return 0
        if t >= 1.0:
            return 1 << 53
        return int(math.ceil(math.ldexp(t, 53)))

    return ceil53(pz / T), ceil53((pz + px) / T)


def ref_shot(oracle, n, w, K1, K2, seed, shot):
    """One shot's error classes [n] (0 none, 1 X, 2 Z, 3 Y)."""
    e = np.zeros(n, np.uint8)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    for i in range(w):
        t = n - w + i
        o0, o1, o2, o3 = oracle.philox4x32_10((i, shot & 0xFFFFFFFF, (shot >> 32) & 0xFFFFFFFF, STREAM_WEIGHT), key)
        r = (((o1 << 32) | o0) * (t + 1)) >> 64
        q = t if e[r] else r
        k = ((o2 >> 5) << 26) | (o3 >> 6)
        e[q] = 2 if k < K1 else 1 if k < K2 else 3
    return e


def ref_errors(oracle, n, w, px, py, pz, seed, shot_begin, shot_count):
    """[S, n] uint8 classes (bit0 x, bit1 z) of shots shot_begin .. shot_begin + S - 1."""
    K1, K2 = thresholds(px, py, pz) if w > 0 else (0, 0)
    out = np.zeros((int(shot_count), int(n)), np.uint8)
    for s in range(int(shot_count)):
        out[s] = ref_shot(oracle, int(n), int(w), K1, K2, int(seed), int(shot_begin) + s)
    return out


def to_uniforms(err, px, py, pz):
    """Uniforms that make the reference's split (Z on [0, pz), X on [pz, pz+px), Y on
    [pz+px, pz+px+py)) reproduce ``err``: the midpoint of the class's interval, and 1 - 2^-53
    (the largest uniform) for no error."""
    px, py, pz = float(px), float(py), float(pz)
    t1, t2, t3 = pz, pz + px, (pz + px) + py
    assert t3 < 1.0
    table = np.array([1.0 - 2.0 ** -53, (t1 + t2) / 2, t1 / 2, (t2 + t3) / 2])
    err = np.asarray(err)
    for c, (lo, hi) in ((1, (t1, t2)), (2, (0.0, t1)), (3, (t2, t3))):
        assert not (err == c).any() or lo < table[c] < hi, "class with an empty interval"
    return table[err]

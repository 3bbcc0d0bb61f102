"""Reference for the serial-schedule min-sum decoder (helper, not a test).

The decoding law of ``qldpc_bp_create_serial`` / ``qldpc_serial_decode_host`` (include/qldpc_hip.h,
csrc/serial.hip) restated in slow, sequential Python: scalars of the decoder's number type (Python
floats are IEEE doubles; ``numpy.float32`` scalars round every operation to float), the sweep taken
variable by variable in an explicit order ``pi`` (``sweep_order`` gives the law's; ``range(n)`` is the
natural order).
"""
import math

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def _number_type(precision):
    return float if int(precision) == 64 else np.float32


def layers(csr):
    """layer(j) of every variable: first-fit in ascending variable index, straight from the definition."""
    rp = [int(v) for v in csr.row_ptr]
    ci = [int(v) for v in csr.col_idx]
    checks = [set() for _ in range(csr.n)]
    for i in range(csr.m):
        for e in range(rp[i], rp[i + 1]):
            checks[ci[e]].add(i)
    layer = []
    for j in range(csr.n):
        taken = {layer[k] for k in range(j) if checks[k] & checks[j]}
        l = 0
        while l in taken:
            l += 1
        layer.append(l)
    return np.array(layer, np.int32)


def sweep_order(csr):
    """pi: the variables sorted by (layer, index)."""
    lay = layers(csr)
    return sorted(range(csr.n), key=lambda j: (int(lay[j]), j))


def priors(channel_probs, precision):
    T = _number_type(precision)
    return [T(math.log((1.0 - float(p)) / float(p))) for p in channel_probs]


def decode_one(csr, l0, pi, max_iter, alpha, precision, synd):
    """One syndrome -> (corr [n] uint8, iters, conv, post [n] float64)."""
    T = _number_type(precision)
    m, n = csr.m, csr.n
    rp = [int(v) for v in csr.row_ptr]
    ci = [int(v) for v in csr.col_idx]
    col_edges = [[] for _ in range(n)]  # (edge id, row) of a column, rows ascending
    for i in range(m):
        for e in range(rp[i], rp[i + 1]):
            col_edges[ci[e]].append((e, i))
    sentinel = T(1e308) if precision == 64 else T(FLT_MAX)
    zero = T(0.0)
    synd = [int(s) & 1 for s in synd]
    b2c = [l0[ci[e]] for e in range(rp[m])]
    dec = [0] * n
    post = [zero] * n
    iters, conv = 0, 0
    for t in range(1, max_iter + 1):
        a_t = T(1.0 - math.ldexp(1.0, -t)) if alpha == 0.0 else T(alpha)
        for j in pi:
            c2b = []
            for e, i in col_edges[j]:
                mag, s = sentinel, synd[i]
                for x in range(rp[i], rp[i + 1]):
                    if x == e:
                        continue
                    a = abs(b2c[x])
                    if a < mag:
                        mag = a
                    if b2c[x] <= 0:
                        s += 1
                c2b.append(T(mag * (-a_t if s & 1 else a_t)))
            temp = l0[j]
            for (e, _), c in zip(col_edges[j], c2b):
                b2c[e] = temp
                temp = T(temp + c)
            post[j] = temp
            dec[j] = 1 if temp <= 0 else 0
            temp = zero
            for (e, _), c in zip(reversed(col_edges[j]), reversed(c2b)):
                b2c[e] = T(b2c[e] + temp)
                temp = T(temp + c)
        iters = t
        ok = True
        for i in range(m):
            a = synd[i]
            for e in range(rp[i], rp[i + 1]):
                a ^= dec[ci[e]]
            if a:
                ok = False
                break
        if ok:
            conv = 1
            break
    return np.array(dec, np.uint8), iters, conv, np.array([float(v) for v in post], np.float64)


def decode_batch(csr, channel_probs, max_iter, alpha, precision, synd, pi=None):
    """[B, m] syndromes -> (corr [B, n] uint8, iters [B] int32, conv [B] uint8, post [B, n] float64)."""
    probs = np.broadcast_to(np.asarray(channel_probs, np.float64), (csr.n,))
    l0 = priors(probs, precision)
    if pi is None:
        pi = sweep_order(csr)
    synd = np.atleast_2d(np.asarray(synd))
    out = [decode_one(csr, l0, list(pi), int(max_iter), float(alpha), int(precision), s) for s in synd]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32),
            np.array([o[2] for o in out], np.uint8), np.stack([o[3] for o in out]))

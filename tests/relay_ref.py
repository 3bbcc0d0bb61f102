"""Reference for the Relay-BP decoder (helper, not a test).

The decoding law of ``qldpc_bp_create_relay`` / ``qldpc_relay_decode_host`` (include/qldpc_hip.h,
csrc/relay.hip) restated in slow, sequential Python: the loops of ``bp_ms_*`` in
oracle/qldpc_oracle.c, scalars of the decoder's number type (Python floats are IEEE doubles;
``numpy.float32`` scalars round every operation to float), the gamma table from the oracle's
Philox4x32-10.
"""
import math

import numpy as np

STREAM_RELAY = 0x51D50007
FLT_MAX = float(np.finfo(np.float32).max)


def _number_type(precision):
    return float if int(precision) == 64 else np.float32


def gammas(oracle, n, pre_gamma, num_legs, gamma_lo, gamma_hi, seed, precision):
    """[num_legs + 1][n] memory strengths in the decoder's type, widened to float64."""
    T = _number_type(precision)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = np.zeros((num_legs + 1, n), np.float64)
    out[0, :] = float(T(float(pre_gamma)))
    for r in range(1, num_legs + 1):
        for j in range(n):
            o0, o1, _, _ = oracle.philox4x32_10((j, r, 0, STREAM_RELAY), key)
            u = float(((o0 >> 5) << 26) | (o1 >> 6)) / 9007199254740992.0
            out[r, j] = float(T(float(gamma_lo) + (float(gamma_hi) - float(gamma_lo)) * u))
    return out


def priors(channel_probs, precision):
    """(L0 [n] in the decoder's type, integer solution weights [n])."""
    T = _number_type(precision)
    l64 = [math.log((1.0 - float(p)) / float(p)) for p in channel_probs]
    return [T(v) for v in l64], [int(math.floor(v * 4294967296.0 + 0.5)) for v in l64]


def decode_one(csr, l0, wq, gam, pre_iter, num_legs, leg_iter, stop_nconv, alpha, precision, synd, trace=None):
    """One syndrome -> (corr [n] uint8, iters, conv, nsol).  ``trace``: a list that receives, per
    solution of the chain in order, (leg, integer weight, decision vector as a tuple)."""
    T = _number_type(precision)
    m, n = csr.m, csr.n
    rp = [int(v) for v in csr.row_ptr]
    ci = [int(v) for v in csr.col_idx]
    col_edges = [[] for _ in range(n)]  # edge ids of a column, rows ascending
    for i in range(m):
        for e in range(rp[i], rp[i + 1]):
            col_edges[ci[e]].append(e)
    E = rp[m]
    sentinel = T(1e308) if precision == 64 else T(FLT_MAX)
    one, zero = T(1.0), T(0.0)
    synd = [int(s) & 1 for s in synd]
    M = list(l0)
    b2c = [zero] * E
    c2b = [zero] * E
    sgn = [0] * E
    dec = [0] * n
    best = None
    best_w = None
    nsol = iters = 0

    def bias(g, j):
        a = T((one - g) * l0[j])  # two rounded products, one rounded sum
        b = T(g * M[j])
        return T(a + b)

    for r in range(num_legs + 1):
        t_r = pre_iter if r == 0 else leg_iter
        g = [T(v) for v in gam[r]]
        for j in range(n):
            bj = bias(g[j], j)
            for e in col_edges[j]:
                b2c[e] = bj
        converged = False
        for t in range(1, t_r + 1):
            a_t = T(1.0 - math.ldexp(1.0, -t)) if alpha == 0.0 else T(alpha)
            for i in range(m):
                temp, s = sentinel, synd[i]
                for e in range(rp[i], rp[i + 1]):
                    c2b[e] = temp
                    sgn[e] = s
                    a = abs(b2c[e])
                    if a < temp:
                        temp = a
                    if b2c[e] <= 0:
                        s += 1
                temp, s = sentinel, 0
                for e in range(rp[i + 1] - 1, rp[i] - 1, -1):
                    if temp < c2b[e]:
                        c2b[e] = temp
                    sgn[e] += s
                    c2b[e] = T(c2b[e] * (-a_t if sgn[e] & 1 else a_t))
                    a = abs(b2c[e])
                    if a < temp:
                        temp = a
                    if b2c[e] <= 0:
                        s += 1
            for j in range(n):
                temp = bias(g[j], j)
                for e in col_edges[j]:
                    b2c[e] = temp
                    temp = T(temp + c2b[e])
                M[j] = temp
                dec[j] = 1 if temp <= 0 else 0
                temp = zero
                for e in reversed(col_edges[j]):
                    b2c[e] = T(b2c[e] + temp)
                    temp = T(temp + c2b[e])
            iters += 1
            ok = True
            for i in range(m):
                a = synd[i]
                for e in range(rp[i], rp[i + 1]):
                    a ^= dec[ci[e]]
                if a:
                    ok = False
                    break
            if ok:
                converged = True
                break
        if not converged:
            continue
        nsol += 1
        w = sum(wq[j] for j in range(n) if dec[j])
        if trace is not None:
            trace.append((r, w, tuple(dec)))
        if best_w is None or w < best_w:
            best_w, best = w, list(dec)
        if nsol >= stop_nconv:
            break
    return np.array(best if nsol > 0 else dec, np.uint8), iters, int(nsol > 0), nsol


def decode_batch(oracle, csr, channel_probs, pre_iter, pre_gamma, num_legs, leg_iter, gamma_lo, gamma_hi,
                 stop_nconv, gamma_seed, alpha, precision, synd):
    """[B, m] syndromes -> (corr [B, n] uint8, iters [B] int32, conv [B] uint8, nsol [B] int32)."""
    probs = np.broadcast_to(np.asarray(channel_probs, np.float64), (csr.n,))
    l0, wq = priors(probs, precision)
    gam = gammas(oracle, csr.n, pre_gamma, num_legs, gamma_lo, gamma_hi, gamma_seed, precision)
    synd = np.atleast_2d(np.asarray(synd))
    out = [decode_one(csr, l0, wq, gam, pre_iter, num_legs, leg_iter, stop_nconv, float(alpha), int(precision), s)
           for s in synd]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32),
            np.array([o[2] for o in out], np.uint8), np.array([o[3] for o in out], np.int32))

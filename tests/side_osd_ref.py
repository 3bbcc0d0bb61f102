"""Reference for OSD under per-shot priors and for BP+OSD channel-update decoding (helper, not a test).

The side law of ``qldpc_osd_decode_batch_side`` / ``qldpc_osd_gpu_decode_side`` (include/qldpc_hip.h)
restated in Python: per syndrome, ``oracle.osd_decode_batch`` with the probability vector the side
bytes select (entry j from ``p1`` where bit 0 of the byte is set, from ``p0`` otherwise).  Everything
else is the oracle's OSD, taken unchanged.

Also the two-sector composition the staged BP+OSD loop and the simulators are checked against, on
top of ``side_ref.compose``: each sector is soft BP, then OSD where BP did not converge, the second
sector's BP and OSD both under the priors the first sector's correction selects.
"""
import numpy as np

import side_ref


def selected(p0, p1, side_row):
    """The probability vector of one syndrome: ``p1[j]`` where bit 0 of ``side_row[j]`` is set, else ``p0[j]``."""
    n = len(side_row)
    a = np.broadcast_to(np.asarray(p0, np.float64), (n,))
    b = np.broadcast_to(np.asarray(p1, np.float64), (n,))
    return np.where((np.asarray(side_row).astype(np.uint8) & 1) != 0, b, a)


def osd_side_batch(oracle, H, p0, p1, synd, post, side, osd_method, osd_order, conv=None, bp_corr=None):
    """(osd0, osdw) uint8 [B, n] of the side law; rows with ``conv`` set copy ``bp_corr``."""
    synd = np.atleast_2d(np.asarray(synd))
    post = np.atleast_2d(np.asarray(post, np.float64))
    side = np.atleast_2d(np.asarray(side))
    B, n = post.shape
    o0 = np.zeros((B, n), np.uint8)
    ow = np.zeros((B, n), np.uint8)
    for b in range(B):
        if conv is not None and conv[b]:
            o0[b] = ow[b] = np.asarray(bp_corr[b], np.uint8)
            continue
        a, w = oracle.osd_decode_batch(H, selected(p0, p1, side[b]), synd[b:b + 1], post[b:b + 1], osd_method,
                                       osd_order)
        o0[b], ow[b] = a[0], w[0]
    return o0, ow


# ------------------------------------------------------------------ soft BP under selected priors
def flooding_soft(oracle, max_iter, alpha=0.625, precision=64):
    """``bp(H, probs [n] or scalar, synd [B, m]) -> (corr, iters, conv, post)``: the oracle's flooding
    min-sum with soft output."""
    def bp(Hq, probs, synd):
        return oracle.bp_decode_batch_soft(Hq, probs, max_iter, alpha, synd, precision)
    return bp


def serial_soft(max_iter, alpha=0.625, precision=64):
    """The same signature over the serial law's host form (``qldpc_serial_decode_host``)."""
    from qldpc_fault_tolerance_amd.engine import serial_decode_host

    def bp(Hq, probs, synd):
        c, it, cv, post = serial_decode_host(Hq, probs, max_iter, synd, ms_scaling_factor=alpha, precision=precision)
        return c.astype(np.uint8), it, cv, post
    return bp


def bp_side_soft(bp, H, p0, p1, synd, side):
    """Soft BP of every syndrome under its own selected priors -> (corr, iters, conv, post)."""
    out = [bp(H, selected(p0, p1, sb), s[None]) for s, sb in zip(np.atleast_2d(synd), np.atleast_2d(side))]
    return (np.concatenate([o[0] for o in out]).astype(np.uint8), np.concatenate([o[1] for o in out]),
            np.concatenate([np.asarray(o[2], bool) for o in out]), np.concatenate([o[3] for o in out]))


def bposd(oracle, bp, H, probs, synd, osd_method, osd_order):
    """Plain BP+OSD of a sector -> (osdw, iters, conv): BP's correction where it converged."""
    c, it, cv, post = bp(H, probs, synd)
    x = np.asarray(c, np.uint8).copy()
    nc = np.flatnonzero(~np.asarray(cv, bool))
    if nc.size:
        n = x.shape[1]
        x[nc] = oracle.osd_decode_batch(H, np.broadcast_to(np.asarray(probs, np.float64), (n,)), synd[nc], post[nc],
                                        osd_method, osd_order)[1]
    return x, it, np.asarray(cv, bool)


def bposd_side(oracle, bp, H, p0, p1, synd, side, osd_method, osd_order):
    """BP+OSD of a sector under the side law, both stages -> (osdw, iters, conv)."""
    c, it, cv, post = bp_side_soft(bp, H, p0, p1, synd, side)
    _, ow = osd_side_batch(oracle, H, p0, p1, synd, post, side, osd_method, osd_order, conv=cv, bp_corr=c)
    return ow, it, cv


def compose(oracle, code, err, direction, bp, p_first, p0, p1, osd_method="osd_e", osd_order=10, update=True):
    """``side_ref.compose`` with BP+OSD sectors: the first sector at the prior ``p_first``, the second
    under ``(p0, p1)`` selected by the first sector's OSD correction.  ``update=False``: the second
    sector is decoded independently at ``p_first`` (its own marginal prior in a symmetric channel)."""
    def first(H, synd):
        return bposd(oracle, bp, H, p_first, synd, osd_method, osd_order)

    def second(H, synd, side):
        if not update:
            return first(H, synd)
        return bposd_side(oracle, bp, H, p0, p1, synd, side, osd_method, osd_order)

    return side_ref.compose(code, err, direction, first, second)

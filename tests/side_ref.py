"""Reference for side-prior decoding (helper, not a test).

The side law of ``qldpc_bp_decode_batch_side`` / ``qldpc_relay_decode_host_side`` /
``qldpc_serial_decode_host_side`` (include/qldpc_hip.h) restated in Python: per syndrome, the prior
(and, for Relay-BP, the integer solution weight) of variable j comes from ``p1`` when bit 0 of its side
byte is set and from ``p0`` otherwise; everything else is the engine's own law, taken unchanged from
tests/relay_ref.py and tests/serial_ref.py (their ``decode_one`` already take the tables as arguments).

Also the composition the staged pipeline and the simulators are checked against: first sector by the
plain host law, second sector by the host side law on the first sector's corrections.
"""
import numpy as np

import relay_ref
import serial_ref


def select(table0, table1, side_row):
    """Entry j of ``table1`` where bit 0 of ``side_row[j]`` is set, else of ``table0``."""
    return [table1[j] if (int(b) & 1) else table0[j] for j, b in enumerate(side_row)]


def _tables(p, n):
    return np.broadcast_to(np.asarray(p, np.float64), (n,))


def relay_decode_batch(oracle, csr, p0, p1, side, pre_iter, pre_gamma, num_legs, leg_iter, gamma_lo, gamma_hi,
                       stop_nconv, gamma_seed, alpha, precision, synd):
    """[B, m] syndromes, [B, n] side bytes -> (corr [B, n] uint8, iters [B], conv [B], nsol [B])."""
    l0a, wqa = relay_ref.priors(_tables(p0, csr.n), precision)
    l0b, wqb = relay_ref.priors(_tables(p1, csr.n), precision)
    gam = relay_ref.gammas(oracle, csr.n, pre_gamma, num_legs, gamma_lo, gamma_hi, gamma_seed, precision)
    synd = np.atleast_2d(np.asarray(synd))
    side = np.atleast_2d(np.asarray(side))
    out = [relay_ref.decode_one(csr, select(l0a, l0b, sb), select(wqa, wqb, sb), gam, pre_iter, num_legs, leg_iter,
                                stop_nconv, float(alpha), int(precision), s) for s, sb in zip(synd, side)]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32),
            np.array([o[2] for o in out], np.uint8), np.array([o[3] for o in out], np.int32))


def serial_decode_batch(csr, p0, p1, side, max_iter, alpha, precision, synd):
    """[B, m] syndromes, [B, n] side bytes -> (corr [B, n] uint8, iters [B], conv [B])."""
    l0a = serial_ref.priors(_tables(p0, csr.n), precision)
    l0b = serial_ref.priors(_tables(p1, csr.n), precision)
    pi = serial_ref.sweep_order(csr)
    synd = np.atleast_2d(np.asarray(synd))
    side = np.atleast_2d(np.asarray(side))
    out = [serial_ref.decode_one(csr, select(l0a, l0b, sb), list(pi), int(max_iter), float(alpha), int(precision), s)
           for s, sb in zip(synd, side)]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32),
            np.array([o[2] for o in out], np.uint8))


# ------------------------------------------------------------------ the channel-update composition
PLAIN = dict(pre_gamma=0.0, num_legs=0)  # engine 7 without memory and legs: plain min-sum


def nonuniform_tables(n, seed=3):
    """Two non-uniform prior tables for the law tests: entries equal to 0.5, entries with p1 < p0."""
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(0.01, 0.08, n)
    p1 = rng.uniform(0.05, 0.6, n)
    p0[::17] = 0.5
    p1[5::19] = 0.5
    p1[3::11] = p0[3::11] * 0.25  # p1 < p0
    return p0, p1


def side_bytes(rng, B, n, density, high_bits=True):
    """Random side bytes at ``density``; with ``high_bits``, bits 1-7 are noise (0xFE counts as 0)."""
    bit = (rng.random((B, n)) < density).astype(np.uint8)
    if not high_bits:
        return bit
    return (bit | (rng.integers(0, 128, (B, n)).astype(np.uint8) << 1)).astype(np.uint8)


def compose(code, err, direction, first_decode, second_decode):
    """The two-stage decode of errors ``err`` [S, n] (bit 0 = x, bit 1 = z): ``first_decode(H, synd)``
    and ``second_decode(H, synd, side)`` return (corr, iters, conv).  -> dict of corr [S, 2, n], iters
    [S, 2], conv [S, 2], fail [S, 2] (sector order X, Z)."""
    from qldpc_fault_tolerance_amd.simulators import gf2_rows

    S, n = err.shape
    ex, ez = (err & 1).astype(np.uint8), ((err >> 1) & 1).astype(np.uint8)
    hz, hx = code.csr("hz"), code.csr("hx")
    sx, sz = gf2_rows(hz, ex), gf2_rows(hx, ez)
    if direction == "x->z":
        cx, ix, vx = first_decode(hz, sx)
        cz, iz, vz = second_decode(hx, sz, cx.astype(np.uint8))
    else:
        cz, iz, vz = first_decode(hx, sz)
        cx, ix, vx = second_decode(hz, sx, cz.astype(np.uint8))
    rx, rz = ex ^ cx.astype(np.uint8), ez ^ cz.astype(np.uint8)
    fx = gf2_rows(hz, rx).any(1) | gf2_rows(code.csr("lz"), rx).any(1)
    fz = gf2_rows(hx, rz).any(1) | gf2_rows(code.csr("lx"), rz).any(1)
    return dict(corr=np.stack([cx, cz], 1).astype(np.uint8), iters=np.stack([ix, iz], 1).astype(np.int32),
                conv=np.stack([vx, vz], 1).astype(bool), fail=np.stack([fx, fz], 1))


def mode_failures(fail, mode):
    """Per-shot failure under ``logical_mode`` from the sector flags [S, 2]."""
    return fail[:, 0] if mode == "X" else fail[:, 1] if mode == "Z" else (fail[:, 0] | fail[:, 1])


def second_solution_kept_by_side_weights(H, p0, p1, relay_two, synd, side, precision, alpha=0.625):
    """Syndromes of a ``stop_nconv = 2`` chain whose kept solution the per-shot weights decide
    differently from ``p0``'s weights, judged by the host law: the chain found two solutions and kept
    the second (it differs from what the same chain stopped at one solution returns), while under
    ``p0``'s integer weights the second is not strictly lighter, so the first would have stayed."""
    import dataclasses
    import math

    from qldpc_fault_tolerance_amd.engine import relay_decode_host_side

    assert relay_two.stop_nconv == 2
    one = dataclasses.replace(relay_two, stop_nconv=1)
    kept = relay_decode_host_side(H, p0, p1, relay_two, synd, side, ms_scaling_factor=alpha, precision=precision)
    first = relay_decode_host_side(H, p0, p1, one, synd, side, ms_scaling_factor=alpha, precision=precision)
    w0 = [int(math.floor(math.log((1.0 - float(p)) / float(p)) * 4294967296.0 + 0.5))
          for p in np.broadcast_to(np.asarray(p0, np.float64), (H.n,))]

    def weight(c):
        return sum(w0[j] for j in np.flatnonzero(c))

    return [b for b in range(len(synd)) if kept[3][b] == 2 and not np.array_equal(kept[0][b], first[0][b])
            and weight(kept[0][b]) >= weight(first[0][b])]

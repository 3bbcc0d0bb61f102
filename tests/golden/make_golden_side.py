"""Writes tests/golden/side_n225.npz: eight syndromes of hgp_34_n225 hz with mixed side bytes and
non-uniform side priors, and what the host side laws (qldpc_relay_decode_host_side,
qldpc_serial_decode_host_side; tests/test_side_cpu.py holds them to the Python restatement) decode
them to, in both precisions.

    python tests/golden/make_golden_side.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import side_ref  # noqa: E402
from qldpc_fault_tolerance_amd import codes  # noqa: E402
from qldpc_fault_tolerance_amd.engine import RelayParams, relay_decode_host_side, serial_decode_host_side  # noqa: E402

PARAMS = dict(pre_iter=6, pre_gamma=0.125, num_legs=3, leg_iter=6, gamma_lo=-0.24, gamma_hi=0.66, stop_nconv=2,
              gamma_seed=0x9E3779B97F4A7C15)
ALPHA, SERIAL_ITER = 0.625, 8


def main():
    hz = codes.get_code("hgp_34_n225").csr("hz")
    rng = np.random.default_rng(2026)
    err = np.concatenate([(rng.random((2, hz.n)) < p).astype(np.uint8) for p in (0.01, 0.03, 0.05, 0.08)])
    synd = hz.matvec(err).astype(np.uint8)
    p0, p1 = side_ref.nonuniform_tables(hz.n, seed=7)
    side = np.concatenate([side_ref.side_bytes(rng, 2, hz.n, d) for d in (0.0, 0.03, 0.5, 1.0)])
    out = dict(synd=synd, side=side, p0=p0, p1=p1, alpha=ALPHA, serial_iter=SERIAL_ITER,
               **{k: np.asarray(v) for k, v in PARAMS.items()})
    r = RelayParams(**PARAMS)
    for prec in (64, 32):
        corr, iters, conv, nsol = relay_decode_host_side(hz, p0, p1, r, synd, side, ms_scaling_factor=ALPHA,
                                                         precision=prec)
        out.update({f"relay_corr{prec}": corr.astype(np.uint8), f"relay_iters{prec}": iters,
                    f"relay_conv{prec}": conv.astype(np.uint8), f"relay_nsol{prec}": nsol})
        print(prec, "relay iters", iters.tolist(), "nsol", nsol.tolist())
        corr, iters, conv = serial_decode_host_side(hz, p0, p1, SERIAL_ITER, synd, side, ms_scaling_factor=ALPHA,
                                                    precision=prec)
        out.update({f"serial_corr{prec}": corr.astype(np.uint8), f"serial_iters{prec}": iters,
                    f"serial_conv{prec}": conv.astype(np.uint8)})
        print(prec, "serial iters", iters.tolist(), "conv", conv.astype(int).tolist())
    np.savez_compressed(os.path.join(HERE, "side_n225.npz"), **out)


if __name__ == "__main__":
    main()

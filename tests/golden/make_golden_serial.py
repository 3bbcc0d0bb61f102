"""Writes tests/golden/serial_n225.npz: eight syndromes of hgp_34_n225 hz and what the Python
restatement of the serial-schedule min-sum law (tests/serial_ref.py) decodes them to, in both
precisions.

    python tests/golden/make_golden_serial.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import serial_ref  # noqa: E402
from qldpc_fault_tolerance_amd import codes  # noqa: E402

P_PRIOR, ALPHA, MAX_ITER = 0.03, 0.625, 8


def main():
    hz = codes.get_code("hgp_34_n225").csr("hz")
    rng = np.random.default_rng(2026)
    err = np.concatenate([(rng.random((2, hz.n)) < p).astype(np.uint8) for p in (0.01, 0.03, 0.05, 0.08)])
    synd = hz.matvec(err).astype(np.uint8)
    out = dict(synd=synd, p_prior=P_PRIOR, alpha=ALPHA, max_iter=MAX_ITER)
    for prec in (64, 32):
        corr, iters, conv, post = serial_ref.decode_batch(hz, P_PRIOR, MAX_ITER, ALPHA, prec, synd)
        out.update({f"corr{prec}": corr, f"iters{prec}": iters, f"conv{prec}": conv, f"post{prec}": post})
        print(prec, "iters", iters.tolist(), "conv", conv.tolist())
    np.savez_compressed(os.path.join(HERE, "serial_n225.npz"), **out)


if __name__ == "__main__":
    main()

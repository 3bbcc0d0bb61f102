"""Shared inputs of the serial-schedule BP tests (tests/test_serial_cpu.py, tests/test_gpu_serial.py).

Plain numpy, deterministic, no GPU.
"""
import numpy as np

from qldpc_fault_tolerance_amd.codes import CSR


def ring5():
    """Five variables on a ring of five degree-2 checks."""
    H = np.zeros((5, 5), np.uint8)
    for i in range(5):
        H[i, i] = H[i, (i + 1) % 5] = 1
    return CSR.from_dense(H)


def irregular():
    """14 x 40: row 0 has degree 1 (the sentinel), row 1 degree 12, column 39 degree 0, column 3
    degree 8 (the widest column the kernel keeps in registers), column 5 degree 10 (past it), the rest
    of degree 1..3, seeded."""
    rng = np.random.default_rng(11)
    m, n = 14, 40
    H = np.zeros((m, n), np.uint8)
    H[0, 0] = 1
    H[1, 1:13] = 1
    H[2:9, 3] = 1
    H[2:11, 5] = 1
    for j in range(13, n - 1):
        H[rng.choice(np.arange(2, m), size=1 + j % 3, replace=False), j] = 1
    assert H[0].sum() == 1 and H[1].sum() == 12 and H[:, n - 1].sum() == 0
    assert H[:, 3].sum() == 8 and H[:, 5].sum() == 10  # (rows 2..8 / 2..10, and row 1)
    return CSR.from_dense(H)


def irregular_priors(n):
    """Non-uniform priors, every fourth tied to the second."""
    p = np.linspace(0.02, 0.12, n)
    p[::4] = p[1]
    return p


def identity(k):
    return CSR(m=k, n=k, row_ptr=np.arange(k + 1, dtype=np.int64), col_idx=np.arange(k, dtype=np.int64))


def chain(n):
    """n variables, n - 1 checks, check i on variables i and i + 1: two layers, for any n."""
    m = n - 1
    rp = 2 * np.arange(m + 1, dtype=np.int64)
    ci = np.stack([np.arange(m), np.arange(m) + 1], axis=1).reshape(-1).astype(np.int64)
    return CSR(m=m, n=n, row_ptr=rp, col_idx=ci)


def syndromes(H, p, count, rng, zero=True):
    """H e of ``count`` i.i.d. errors at rate p (the first replaced by the zero syndrome)."""
    e = (rng.random((count, H.n)) < p).astype(np.uint8)
    if zero:
        e[0] = 0
    return H.matvec(e).astype(np.uint8)

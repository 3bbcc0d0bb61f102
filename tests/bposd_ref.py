"""Per-shot BP+OSD verdicts of the data-error loop under the oracle (helper, not a test)."""
import numpy as np


def oracle_sector_fails(oracle, code, err, p, mi, order, method="osd_e", precision=64):
    """Per shot and sector: the reference's BPOSD verdict on the engine's sampled errors —
    oracle BP (soft), then the C OSD restatement where BP did not converge, then the
    _single_run failure check (src/Simulators.py:135-160).  ``p``: the decoders' prior, or the pair
    (prior of the hz decoder, prior of the hx decoder)."""
    from qldpc_fault_tolerance_amd.simulators import gf2_rows

    priors = np.broadcast_to(np.asarray(p, dtype=np.float64), (2,))
    out = np.zeros((err.shape[0], 2), dtype=bool)
    for q, H, k in ((0, code.hz, "hz"), (1, code.hx, "hx")):
        pq = float(priors[q])
        e = ((err >> q) & 1).astype(np.uint8)
        synd = gf2_rows(code.csr(k), e)
        oc, _, ov, op = oracle.bp_decode_batch_soft(H, pq, mi, 0.625, synd, precision)
        x = oc.copy()
        nc = np.flatnonzero(~ov)
        if nc.size:
            x[nc] = oracle.osd_decode_batch(H, pq * np.ones(code.N), synd[nc], op[nc], method, order)[1]
        r = (e ^ x).astype(np.uint8)
        out[:, q] = gf2_rows(code.csr(k), r).any(1) | gf2_rows(code.csr("lz" if q == 0 else "lx"), r).any(1)
    return out

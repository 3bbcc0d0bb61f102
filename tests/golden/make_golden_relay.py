"""Writes tests/golden/relay_n225.npz: eight syndromes of hgp_34_n225 hz and what the Python
restatement of the Relay-BP law (tests/relay_ref.py) decodes them to, in both precisions.

    python tests/golden/make_golden_relay.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import oracle  # noqa: E402
import relay_ref  # noqa: E402
from qldpc_fault_tolerance_amd import codes  # noqa: E402

PARAMS = dict(pre_iter=6, pre_gamma=0.125, num_legs=3, leg_iter=6, gamma_lo=-0.24, gamma_hi=0.66, stop_nconv=2,
              gamma_seed=0x9E3779B97F4A7C15)
P_PRIOR, ALPHA = 0.03, 0.625


def main():
    oracle.build()
    hz = codes.get_code("hgp_34_n225").csr("hz")
    rng = np.random.default_rng(2025)
    err = np.concatenate([(rng.random((2, hz.n)) < p).astype(np.uint8) for p in (0.01, 0.03, 0.05, 0.08)])
    synd = hz.matvec(err).astype(np.uint8)
    out = dict(synd=synd, p_prior=P_PRIOR, alpha=ALPHA, **{k: np.asarray(v) for k, v in PARAMS.items()})
    for prec in (64, 32):
        corr, iters, conv, nsol = relay_ref.decode_batch(
            oracle, hz, P_PRIOR, PARAMS["pre_iter"], PARAMS["pre_gamma"], PARAMS["num_legs"], PARAMS["leg_iter"],
            PARAMS["gamma_lo"], PARAMS["gamma_hi"], PARAMS["stop_nconv"], PARAMS["gamma_seed"], ALPHA, prec, synd)
        out.update({f"corr{prec}": corr, f"iters{prec}": iters, f"conv{prec}": conv, f"nsol{prec}": nsol})
        print(prec, "iters", iters.tolist(), "nsol", nsol.tolist())
    np.savez_compressed(os.path.join(HERE, "relay_n225.npz"), **out)


if __name__ == "__main__":
    main()

"""The recorded routes of every bundled graph (tests/golden/routes_fp{64,32}.jsonl) and the graphs
they name, shared by test_routes_cpu.py and test_gpu_routes.py.

One JSON line per decoder: ``code`` / ``graph`` name the parity-check matrix (hz itself, its
space-time graphs over 2-5 rounds, [hz | I]), ``env`` the QLDPC_* switches set while it was built
(QLDPC_M2S_ANNEAL=0 everywhere: the placement search moves no route), the rest is the decoder's
``geometry()`` as recorded on an MI355X.
"""
import json
import os

import numpy as np

from qldpc_fault_tolerance_amd import codes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# what plan_bp (no device) must reproduce of a recorded line
PLANNED = ("engine", "kernel_id", "row_chunks", "threads", "vars_per_thread", "lds_bytes", "degree3_slots")
GRAPH_TAGS = ("hz", "st2", "st3", "st4", "st5", "hI")
PROB = 0.01


def graph(code_name, tag):
    hz = codes.get_code(code_name).hz
    if tag == "hz":
        return codes.CSR.from_dense(hz)
    if tag == "hI":
        return codes.CSR.from_dense(np.hstack([hz, np.eye(hz.shape[0], dtype=np.uint8)]))
    return codes.space_time_csr(hz, int(tag[2:]))


def load(precision):
    with open(os.path.join(GOLDEN, f"routes_fp{precision}.jsonl")) as f:
        return [json.loads(line) for line in f if line.strip()]


def line_id(rec):
    env = ",".join(f"{k}={v}" for k, v in sorted(rec["env"].items()) if k != "QLDPC_M2S_ANNEAL")
    return f"fp{rec['precision']}-{rec['code']}-{rec['graph']}" + (f"-{env}" if env else "")


class switches:
    """Set the QLDPC_* switches of a fixture line for the duration of one create / plan call."""

    def __init__(self, env):
        self.env = dict(env)

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

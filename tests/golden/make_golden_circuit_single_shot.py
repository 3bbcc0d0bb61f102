"""Golden vectors of the single-shot circuit simulator, from the reference's own Python.

    python tests/golden/make_golden_circuit_single_shot.py   # reference_circuit_single_shot.npz

It needs the reference checkout that ``make_golden.py`` reads, so it never runs with the GPU tests.
With the stubs of ``make_golden.py`` (``install_stubs``, ``RecordingCircuit`` as ``stim.Circuit``) the reference's
``CodeSimulator_Circuit._generate_circuit`` and ``AddCXError`` (``src/Simulators.py:438-609``,
``src/ErrorPlugin.py:11-25``) run unchanged; the recorded op list is stored.  The samples are drawn
with the oracle's sampler (``circuit_oracle.sample_mechanisms``: seed 7, shot_begin 4242, 1500
samples) on the engine's DEM of the RECORDED circuit, and the reference's own ``_decoding_samples``
(``:612-644``) decodes them with decoder stubs that wrap the CPU oracle and carry ``.h``
(decoder1: min-sum BP on [hx | I]; decoder2: BP + OSD-E(10), or plain BP for the two-cycle tag).

Per tag (``circuit_single_shot_ref.GOLDEN_CASES``): ``names / args / offs / targets`` (the op list),
``samples`` ([S, ceil((D + K) / 8)] bit-packed detector + observable bits), ``fail`` ([S] the
reference's failure flags), ``params``.  Data only.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import RecordingCircuit, _pack_ops, _RecTarget, install_stubs  # noqa: E402

import circuit_single_shot_ref as ref  # noqa: E402
import oracle  # noqa: E402


class _Circuit(RecordingCircuit):
    """``append("DETECTOR", stim.target_rec(k))``: the single-shot builder passes ONE target, not a list."""

    def append(self, name, targets=(), arg=None):
        if isinstance(targets, _RecTarget):
            targets = [targets]
        return super().append(name, targets, arg)


class _BP:
    def __init__(self, h, probs, max_iter):
        self.h = np.asarray(h, np.uint8)
        self.probs, self.max_iter = np.asarray(probs, np.float64), int(max_iter)

    def decode(self, synd):
        c, _, _ = oracle.bp_decode_batch(self.h, self.probs, self.max_iter, "minimum_sum", ref.ALPHA,
                                         np.asarray(synd).reshape(1, -1).astype(np.uint8), 64, nthreads=1)
        return c[0].astype(np.int64)


class _BPOSD(_BP):
    def decode(self, synd):
        s = np.asarray(synd).reshape(1, -1).astype(np.uint8)
        bp, _, conv, post = oracle.bp_decode_batch_soft(self.h, self.probs, self.max_iter, ref.ALPHA, s, 64, nthreads=1)
        _, osdw = oracle.osd_decode_batch(self.h, self.probs, s, post, "osd_e", 10)
        return (bp if conv[0] else osdw)[0].astype(np.int64)


def main():
    install_stubs()
    stim = sys.modules["stim"]
    stim.Circuit = _Circuit
    stim.target_rec = _RecTarget
    import Simulators as SIM

    out = {}
    for tag, name, logical, ncyc, scales, p in ref.GOLDEN_CASES:
        code = ref.make_code(name)
        n = code.N
        final_osd = ncyc > 2
        mk2 = _BPOSD if final_osd else _BP
        # built before the constructor swaps the sectors of `code` (eval_logical_type 'X')
        d1z = _BP(ref.ext(code.hx), ref.priors1(n, code.hx.shape[0], p), 6)
        d1x = _BP(ref.ext(code.hz), ref.priors1(n, code.hz.shape[0], p), 6)
        d2z, d2x = mk2(code.hx, p * np.ones(n), 6), mk2(code.hz, p * np.ones(n), 6)
        sim = SIM.CodeSimulator_Circuit(code=code, decoder1_z=d1z, decoder1_x=d1x, decoder2_z=d2z, decoder2_x=d2x,
                                        p=p, num_cycles=ncyc, error_params=ref.error_params(scales, p),
                                        eval_logical_type=logical, circuit_type="coloration")
        sim._generate_circuit()
        names, args, offs, tg = _pack_ops(sim.circuit.ops)
        out[f"{tag}_names"], out[f"{tag}_args"], out[f"{tag}_offs"], out[f"{tag}_targets"] = names, args, offs, tg
        dem = sim.circuit.engine_circuit().detector_error_model()
        det, obs = ref.sample(dem, ref.SEED, ref.SHOT_BEGIN, ref.SAMPLES)
        samples = np.hstack([det, obs])
        fail = np.asarray(sim._decoding_samples([list(r) for r in samples]), dtype=np.uint8)
        out[f"{tag}_samples"] = np.packbits(samples, axis=1)
        out[f"{tag}_fail"] = fail
        out[f"{tag}_params"] = np.array([p, ncyc, logical == "X", final_osd, dem.num_detectors, dem.num_observables,
                                         ref.SEED, ref.SHOT_BEGIN, ref.SAMPLES], dtype=np.float64)
        print(tag, "ops", len(names), "detectors", dem.num_detectors, "mechanisms", dem.num_errors, "failures",
              int(fail.sum()), flush=True)
    path = os.path.join(HERE, "reference_circuit_single_shot.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

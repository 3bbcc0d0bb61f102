"""Device-side objects of the engine: Tanner graphs, BP decoders, fused MC runs.

Thin owners of the C-ABI handles in ``libqldpc_hip.so``.  PyTorch-ROCm is used
only for device buffers and the current HIP stream; every computation runs in
the hand-written kernels.  No CPU fallback exists (``_native`` raises).
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

from . import _native
from .codes import CSR, CSSCode

METHODS = {"product_sum": 0, "prod_sum": 0, "ps": 0, "minimum_sum": 1, "min_sum": 1, "ms": 1}
LOGICAL_MODES = {"X": 0, "Z": 1, "Total": 2}
OSD_METHODS = {"osd_0": 0, "osd0": 0, "osd_e": 1, "osde": 1, "exhaustive": 1, "osd_cs": 2, "osdcs": 2,
               "combination_sweep": 2}


def _torch():
    import torch

    if not torch.cuda.is_available():
        raise _native.NativeUnavailable("torch reports no HIP device; the engine needs an MI355X (no CPU fallback)")
    return torch


def _stream_handle(torch, device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _stream(stream, device):
    """``stream`` as given, or the current HIP stream of ``device``."""
    torch = _torch()
    return stream if stream is not None else _stream_handle(torch, device)


def _ptr(t):
    """Device address of a tensor as ``c_void_p``; None stays None (an optional ABI buffer)."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _handle(obj):
    """The C handle of an optional engine object."""
    return obj.handle if obj is not None else None


def _seed64(seed) -> int:
    return int(seed) & (2**64 - 1)


def _logical_mode(logical_mode) -> int:
    return LOGICAL_MODES[logical_mode] if isinstance(logical_mode, str) else int(logical_mode)


def _device_index(device):
    """``device``, or this rank's GPU (LOCAL_RANK under torch.distributed.run) for None."""
    if device is None:
        from .parallel import local_device_index

        device = local_device_index()
    return device


def _new_counters(device):
    """A zeroed ``qldpc_counters`` image (int64 words) on GPU ``device``."""
    torch = _torch()
    return torch.zeros(_native.COUNTER_WORDS, dtype=torch.int64, device=torch.device("cuda", device))


def _launch_prep(counters, logical_mode, stream):
    """(mode, stream) of a fused launch that accumulates into ``counters``."""
    torch = _torch()
    if counters is None:
        raise ValueError("counters buffer required")
    return _logical_mode(logical_mode), (stream if stream is not None else _stream_handle(torch, counters.device))


def _syndromes(synd, m=None):
    """``synd`` as a contiguous uint8 0/1 array [B, m]; with ``m``, the width is checked."""
    s = np.ascontiguousarray(np.atleast_2d(np.asarray(synd)).astype(np.int64) % 2, dtype=np.uint8)
    if m is not None and s.shape[1] != m:
        raise ValueError(f"syndrome length {s.shape[1]} != number of checks {m}")
    return s


def _channel_probs(channel_probs, n, check_length=True):
    """A scalar or a length-``n`` vector of priors as a contiguous float64 vector."""
    probs = np.asarray(channel_probs, dtype=np.float64)
    if probs.ndim == 0:
        probs = np.full(n, float(probs))
    if check_length and probs.shape != (n,):
        raise ValueError(f"channel_probs must have length {n}")
    return np.ascontiguousarray(probs)


def _side_bytes(side, B, n):
    """Side bytes ``[B, n]`` of a side decode as a contiguous uint8 array (only bit 0 is read)."""
    s = np.ascontiguousarray(np.atleast_2d(np.asarray(side)), dtype=np.uint8)
    if s.shape != (B, n):
        raise ValueError(f"side must be [{B}, {n}], not {list(s.shape)}")
    return s


CHANNEL_UPDATES = {None: 0, "x->z": 1, "z->x": 2}


def bp_method_code(bp_method) -> int:
    if isinstance(bp_method, (int, np.integer)):
        return int(bp_method)
    key = str(bp_method).lower()
    if key not in METHODS:
        raise ValueError(f"unknown bp_method {bp_method!r}")
    return METHODS[key]


def osd_method_code(osd_method) -> int:
    if isinstance(osd_method, (int, np.integer)):
        return int(osd_method)
    key = str(osd_method).lower()
    if key not in OSD_METHODS:
        raise ValueError(f"unknown osd_method {osd_method!r}")
    return OSD_METHODS[key]


LSD_METHODS = {"lsd_0": 0, "lsd_e": 1, "lsd_cs": 2}


def lsd_method_code(lsd_method) -> int:
    if isinstance(lsd_method, (int, np.integer)):
        return int(lsd_method)
    key = str(lsd_method).lower()
    if key not in LSD_METHODS:
        raise ValueError(f"unknown lsd_method {lsd_method!r}")
    return LSD_METHODS[key]


class _Handle:
    """Owner of one C-ABI handle: ``_create`` fills ``handle``, ``__del__`` frees it with the
    library function the class names in ``_destroy``."""

    _destroy = None

    def _create(self, what: str, *args):
        """``handle`` from the library's ``what(*args, &handle)``."""
        h = ctypes.c_void_p()
        _native.check(getattr(_native.lib(), what)(*args, ctypes.byref(h)), what)
        self.handle = h

    def _ints(self, fn: str, what: str, count: int) -> list:
        """The ``count`` int32 values the library's ``fn(handle, &v0, &v1, ..)`` reports."""
        v = [ctypes.c_int32() for _ in range(count)]
        _native.check(getattr(_native.lib(), fn)(self.handle, *[ctypes.byref(x) for x in v]), what)
        return [x.value for x in v]

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and _native._lib is not None:  # the library is gone at interpreter shutdown
            getattr(_native.lib(), self._destroy)(h)
            self.handle = None


def _decode_buffers(graph, synd, check_width=True):
    """(torch, device, syndromes [B, m], corrections [B, n], iterations [B], converged [B]) on
    ``graph``'s GPU: the host syndromes normalised and uploaded, and the output buffers of one
    batched decode."""
    torch = _torch()
    s = _syndromes(synd, graph.m if check_width else None)
    B = s.shape[0]
    dev = torch.device("cuda", graph.device)
    return (torch, dev, torch.from_numpy(s).to(dev), torch.empty((B, graph.n), dtype=torch.uint8, device=dev),
            torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.uint8, device=dev))


class DeviceGraph(_Handle):
    """A parity-check matrix uploaded once (``qldpc_graph_create``)."""

    _destroy = "qldpc_graph_destroy"

    def __init__(self, H, device: int | None = None):
        c = H if isinstance(H, CSR) else CSR.from_dense(H)
        device = _device_index(device)
        self.csr = c
        self.m, self.n = c.m, c.n
        self.device = device
        self._rp = np.ascontiguousarray(c.row_ptr, dtype=np.int32)
        self._ci = np.ascontiguousarray(c.col_idx, dtype=np.int32)
        self._create("qldpc_graph_create", device, c.m, c.n, _np_ptr(self._rp), _np_ptr(self._ci))

    def info(self):
        return dict(zip(["m", "n", "nnz", "max_row_deg", "max_col_deg"],
                        self._ints("qldpc_graph_info", "graph_info", 5)))


@dataclass(frozen=True)
class RelayParams:
    """The chain of a Relay-BP decoder (``qldpc_bp_create_relay``, include/qldpc_hip.h): ``pre_iter``
    iterations at memory strength ``pre_gamma``, then ``num_legs`` legs of ``leg_iter`` iterations
    whose per-variable strengths are drawn from ``[gamma_lo, gamma_hi]`` by ``gamma_seed``; the
    chain stops at ``stop_nconv`` solutions and keeps the lightest."""

    pre_iter: int
    pre_gamma: float = 0.125
    num_legs: int = 0
    leg_iter: int = 0
    gamma_lo: float = -0.24
    gamma_hi: float = 0.66
    stop_nconv: int = 1
    gamma_seed: int = 0

    @staticmethod
    def of(relay) -> "RelayParams":
        return relay if isinstance(relay, RelayParams) else RelayParams(**dict(relay))

    @property
    def max_iter(self) -> int:
        return int(self.pre_iter) + int(self.num_legs) * int(self.leg_iter)

    def abi(self, ms_scaling_factor, precision) -> tuple:
        """The parameter block of the C entry points, in their order."""
        return (int(self.pre_iter), float(self.pre_gamma), int(self.num_legs), int(self.leg_iter),
                float(self.gamma_lo), float(self.gamma_hi), int(self.stop_nconv), _seed64(self.gamma_seed),
                float(ms_scaling_factor), int(precision))


class DeviceBP(_Handle):
    """``ldpc.bp_decoder`` equivalent on the GPU (``qldpc_bp_create``).

    ``relay``: a :class:`RelayParams` (or a dict of its fields) makes the handle a Relay-BP decoder
    (engine 7, ``qldpc_bp_create_relay``): min-sum only, ``max_iter`` is then the chain's total.

    ``schedule``: ``"parallel"`` (the reference's flooding schedule) or ``"serial"``: min-sum on the
    serial, variable-by-variable schedule (engine 8, ``qldpc_bp_create_serial``, the law in
    include/qldpc_hip.h), with soft output when ``soft`` is set.

    ``anneal_iters``: moves of the annealed V-slot placement the fp64 engine-3 families run at
    creation (host time, one core: ~0.18 us per move; default 4000 per edge capped at 2^25, memoised
    per process for the same graph).  0 keeps the greedy placement (decodes identically; the placement
    only moves LDS bank conflicts), for short runs over many codes."""

    _destroy = "qldpc_bp_destroy"

    def __init__(self, H, channel_probs, max_iter: int = 0, bp_method="minimum_sum", ms_scaling_factor=0.625,
                 precision: int = 64, vars_per_thread: int = 0, device: int | None = None, graph: DeviceGraph | None = None,
                 min_col_slots: int = 0, soft: bool = False, hbm: bool = False, anneal_iters: int | None = None,
                 relay=None, schedule: str = "parallel"):
        if schedule not in ("parallel", "serial"):
            raise ValueError(f"schedule must be 'parallel' or 'serial', not {schedule!r}")
        if schedule == "serial" and (bp_method_code(bp_method) != 1 or relay is not None):
            raise ValueError("schedule='serial' is minimum_sum on its own engine, without relay legs")
        if anneal_iters is not None:  # read by qldpc_bp_create (QLDPC_M2S_ANNEAL) at creation only
            old = os.environ.get("QLDPC_M2S_ANNEAL")
            os.environ["QLDPC_M2S_ANNEAL"] = str(int(anneal_iters))
            try:
                self.__init__(H, channel_probs, max_iter, bp_method, ms_scaling_factor, precision, vars_per_thread,
                              device, graph, min_col_slots, soft, hbm, None, relay, schedule)
            finally:
                if old is None:
                    os.environ.pop("QLDPC_M2S_ANNEAL", None)
                else:
                    os.environ["QLDPC_M2S_ANNEAL"] = old
            return
        self.graph = graph if graph is not None else DeviceGraph(H, device=device)
        n = self.graph.n
        self.channel_probs = _channel_probs(channel_probs, n)
        self.max_iter = int(max_iter) if int(max_iter) > 0 else n
        self.bp_method = bp_method_code(bp_method)
        self.ms_scaling_factor = float(ms_scaling_factor)
        self.precision = int(precision)
        self.soft = bool(soft)
        self.relay = RelayParams.of(relay) if relay is not None else None
        self.schedule = schedule
        common = (self.graph.handle, _np_ptr(self.channel_probs), self.max_iter)
        if schedule == "serial":
            if hbm:
                raise NotImplementedError("the serial schedule runs on its own engine, not the HBM-resident one")
            self._create("qldpc_bp_create_serial", *common, self.ms_scaling_factor, self.precision, int(self.soft))
        elif self.relay is not None:
            if self.bp_method != 1 or self.soft or hbm:
                raise NotImplementedError("Relay-BP is minimum_sum on its own engine, without soft output")
            self.max_iter = self.relay.max_iter
            self._create("qldpc_bp_create_relay", *common[:2], *self.relay.abi(self.ms_scaling_factor, self.precision))
        elif hbm:
            # engine 6: HBM-resident messages (automatic when no LDS engine holds the image)
            if self.bp_method != 1:
                raise NotImplementedError("the HBM-resident engine implements minimum_sum")
            self._create("qldpc_bp_create_hbm", *common, self.ms_scaling_factor, self.precision)
        elif self.soft and self.bp_method == 1:
            # BP+OSD: engine 1 hands back the final posteriors (qldpc_bp_create_soft); a product-sum
            # decoder (engine 5) writes ldpc's log(1 / ratio) posteriors from the default create
            self._create("qldpc_bp_create_soft", *common, self.ms_scaling_factor, self.precision)
        else:
            self._create("qldpc_bp_create", *common, self.bp_method, self.ms_scaling_factor, self.precision,
                         int(vars_per_thread), int(min_col_slots))

    @property
    def m(self):
        return self.graph.m

    @property
    def n(self):
        return self.graph.n

    def set_channel_probs(self, channel_probs):
        """New priors on the same handle (``qldpc_bp_set_channel_probs``)."""
        probs = _channel_probs(channel_probs, self.graph.n)
        _native.check(_native.lib().qldpc_bp_set_channel_probs(self.handle, _np_ptr(probs)),
                      "qldpc_bp_set_channel_probs")
        self.channel_probs = probs

    def set_side_probs(self, p0, p1):
        """Side priors (``qldpc_bp_set_side_probs``, engines 7 and 8): the two tables a side decode
        selects from per syndrome and variable (``side`` bit 0 -> ``p0``, 1 -> ``p1``).  A scalar
        broadcasts to ``n``."""
        n = self.graph.n
        a, b = _channel_probs(p0, n), _channel_probs(p1, n)
        _native.check(_native.lib().qldpc_bp_set_side_probs(self.handle, _np_ptr(a), _np_ptr(b)),
                      "qldpc_bp_set_side_probs")
        self.side_probs = (a, b)

    def geometry(self):
        g = dict(zip(["threads", "vars_per_thread", "lds_bytes", "blocks_per_cu"],
                     self._ints("qldpc_bp_geometry", "bp_geometry", 4)))
        g["engine"], = self._ints("qldpc_bp_engine", "bp_engine", 1)
        g["degree3_slots"], = self._ints("qldpc_bp_degree3_slots", "bp_degree3_slots", 1)
        g["gather_conflicts"] = tuple(self._ints("qldpc_bp_bank_stats", "bp_bank_stats", 2))
        g["kernel_id"], g["row_chunks"] = self._ints("qldpc_bp_kernel_id", "bp_kernel_id", 2)
        lm = (ctypes.c_int64 * 6)()
        _native.check(_native.lib().qldpc_bp_lds_model(self.handle, lm), "bp_lds_model")
        g["lds_model"] = dict(zip(["cs_gather", "cs_gather_extra", "v_read", "v_read_extra", "v_store", "v_store_extra"],
                                  list(lm)))
        return g

    def decode_batch_device(self, synd_dev, corr_dev, iters_dev=None, conv_dev=None, stream=None, side=None):
        """Decode device uint8 syndromes [B, m] into device corrections [B, n] (async).  ``side``: device
        uint8 side bytes [B, n] for a side decode (``qldpc_bp_decode_batch_side``)."""
        torch = _torch()
        B = int(synd_dev.shape[0])
        assert synd_dev.dtype == torch.uint8 and synd_dev.is_contiguous() and synd_dev.shape[1] == self.m
        assert corr_dev.dtype == torch.uint8 and corr_dev.is_contiguous() and tuple(corr_dev.shape) == (B, self.n)
        if side is not None:
            assert side.dtype == torch.uint8 and side.is_contiguous() and tuple(side.shape) == (B, self.n)
            _native.check(_native.lib().qldpc_bp_decode_batch_side(
                self.handle, _ptr(synd_dev), _ptr(side), _ptr(corr_dev), _ptr(iters_dev), _ptr(conv_dev), B,
                _stream(stream, synd_dev.device)), "qldpc_bp_decode_batch_side")
            return
        _native.check(_native.lib().qldpc_bp_decode_batch(
            self.handle, _ptr(synd_dev), _ptr(corr_dev), _ptr(iters_dev), _ptr(conv_dev), B,
            _stream(stream, synd_dev.device)), "qldpc_bp_decode_batch")

    def decode_batch(self, synd, side=None):
        """Host convenience: ``synd`` [B, m] (0/1) -> (corr [B, n] int, iters [B], converged [B]).
        ``side`` [B, n]: a side decode on the handle's side priors (:meth:`set_side_probs`)."""
        torch, dev, sd, corr, iters, conv = _decode_buffers(self.graph, synd)
        sb = None if side is None else torch.from_numpy(_side_bytes(side, sd.shape[0], self.graph.n)).to(dev)
        self.decode_batch_device(sd, corr, iters, conv, side=sb)
        torch.cuda.synchronize(dev)
        return corr.cpu().numpy().astype(np.int64), iters.cpu().numpy(), conv.cpu().numpy().astype(bool)

    def _decode_soft_device(self, sd, corr, iters, conv, stream, side=None):
        """Soft decode of device syndromes ``sd`` (async); returns the posteriors [B, n] float64.
        ``side``: device side bytes [B, n] of a side decode.  A Relay-BP handle (engine 7) and every
        side decode go through ``qldpc_bp_decode_batch_side_soft``."""
        torch = _torch()
        post = torch.empty(corr.shape, dtype=torch.float64, device=sd.device)
        if side is not None or self.relay is not None:
            _native.check(_native.lib().qldpc_bp_decode_batch_side_soft(
                self.handle, _ptr(sd), _ptr(side), _ptr(corr), _ptr(iters), _ptr(conv), _ptr(post), sd.shape[0],
                stream), "qldpc_bp_decode_batch_side_soft")
            return post
        _native.check(_native.lib().qldpc_bp_decode_batch_soft(
            self.handle, _ptr(sd), _ptr(corr), _ptr(iters), _ptr(conv), _ptr(post), sd.shape[0], stream),
            "qldpc_bp_decode_batch_soft")
        return post

    def decode_batch_soft(self, synd, side=None):
        """Like :meth:`decode_batch` plus the final posteriors ``post`` [B, n] float64
        (ldpc's ``log_prob_ratios``); needs ``soft=True``, or a Relay-BP handle without legs
        (``num_legs = 0``).  ``side`` [B, n]: a side decode (engines 7 and 8)."""
        torch, dev, sd, corr, iters, conv = _decode_buffers(self.graph, synd)
        sb = None if side is None else torch.from_numpy(_side_bytes(side, sd.shape[0], self.graph.n)).to(dev)
        post = self._decode_soft_device(sd, corr, iters, conv, _stream_handle(torch, dev), side=sb)
        torch.cuda.synchronize(dev)
        return (corr.cpu().numpy().astype(np.int64), iters.cpu().numpy(), conv.cpu().numpy().astype(bool),
                post.cpu().numpy())


def plan_bp(H, channel_probs, bp_method="minimum_sum", precision: int = 64, vars_per_thread: int = 0,
            min_col_slots: int = 0) -> dict:
    """The route :class:`DeviceBP` would take for this graph (``qldpc_bp_plan``), under the QLDPC_*
    switches of the environment, decided on the host: needs the library, not a GPU.  The keys are
    those of :meth:`DeviceBP.geometry` that do not depend on the device or the built tables."""
    graph = DeviceGraph(H, device=0)  # host-side handle; the plan never touches the device
    probs = np.ascontiguousarray(np.broadcast_to(np.asarray(channel_probs, dtype=np.float64), (graph.n,)))
    out = (ctypes.c_int32 * 8)()
    _native.check(_native.lib().qldpc_bp_plan(graph.handle, _np_ptr(probs), bp_method_code(bp_method), int(precision),
                                              int(vars_per_thread), int(min_col_slots), out, 8), "qldpc_bp_plan")
    return dict(zip(["engine", "kernel_id", "row_chunks", "threads", "vars_per_thread", "lds_bytes", "degree3_slots",
                     "degree2_slots"], list(out)))


class HostOSD(_Handle):
    """Ordered-statistics post-processing stage (``qldpc_osd_*``, csrc/osd.hip).

    Native host code (GF(2) elimination on bit-packed columns, a std::thread
    pool over syndromes); it consumes the GPU BP's posteriors.  Needs only the
    library, not a GPU.
    """

    _destroy = "qldpc_osd_destroy"

    def __init__(self, H, channel_probs, osd_method="osd_e", osd_order=10):
        c = H if isinstance(H, CSR) else CSR.from_dense(H)
        self.m, self.n = c.m, c.n
        self.osd_method = osd_method_code(osd_method)
        self.osd_order = int(osd_order)
        self._probs = _channel_probs(channel_probs, self.n, check_length=False)
        rp = np.ascontiguousarray(c.row_ptr, dtype=np.int32)
        ci = np.ascontiguousarray(c.col_idx, dtype=np.int32)
        self._create("qldpc_osd_create", self.m, self.n, _np_ptr(rp), _np_ptr(ci), _np_ptr(self._probs),
                     self.osd_method, self.osd_order)
        self.rank, = self._ints("qldpc_osd_rank", "qldpc_osd_rank", 1)

    def set_side_probs(self, p0, p1):
        """Side tables (``qldpc_osd_set_side_probs``): a side decode weighs column j of syndrome b with
        log(1 / p_s[j]), s = ``side[b, j] & 1``.  A scalar broadcasts to ``n``."""
        a, b = _channel_probs(p0, self.n, check_length=False), _channel_probs(p1, self.n, check_length=False)
        _native.check(_native.lib().qldpc_osd_set_side_probs(self.handle, _np_ptr(a), _np_ptr(b)),
                      "qldpc_osd_set_side_probs")
        self.side_probs = (a, b)

    def decode_batch(self, synd, post, conv=None, bp_corr=None, threads: int = 0, side=None):
        """(osd0 [B, n], osdw [B, n]) uint8; converged rows (``conv``) copy ``bp_corr``.  ``side``
        [B, n]: a side decode on the handle's side tables (:meth:`set_side_probs`)."""
        s = _syndromes(synd, self.m)
        B = s.shape[0]
        pst = np.ascontiguousarray(np.asarray(post, dtype=np.float64).reshape(B, self.n))
        cv = None if conv is None else np.ascontiguousarray(np.asarray(conv).reshape(B), dtype=np.uint8)
        bc = None if bp_corr is None else np.ascontiguousarray(np.asarray(bp_corr).reshape(B, self.n),
                                                                 dtype=np.uint8)
        o0 = np.zeros((B, self.n), np.uint8)
        ow = np.zeros((B, self.n), np.uint8)
        vp = lambda a: None if a is None else _np_ptr(a)  # noqa: E731
        if side is not None:
            sb = _side_bytes(side, B, self.n)
            _native.check(_native.lib().qldpc_osd_decode_batch_side(
                self.handle, vp(s), vp(pst), vp(cv), vp(bc), vp(sb), vp(o0), vp(ow), B, int(threads)),
                "qldpc_osd_decode_batch_side")
            return o0, ow
        _native.check(_native.lib().qldpc_osd_decode_batch(self.handle, vp(s), vp(pst), vp(cv), vp(bc), vp(o0),
                                                           vp(ow), B, int(threads)), "qldpc_osd_decode_batch")
        return o0, ow


class DeviceOSD(_Handle):
    """OSD on the GPU (``qldpc_osd_gpu_*``): one workgroup per non-converged syndrome, fed
    straight from the soft-output BP's device buffers.  Uniform priors weigh candidates by
    popcount; non-uniform ones (the circuit-level DEM priors) by sum log(1/p_j) in column order,
    as the host stage.  ``supported`` says whether a graph qualifies (n <= ``MAX_N``, osd_e order <=
    ``MAX_OSD_E_ORDER``, the host stage's cap: its candidate table has 2^order rows)."""

    MAX_N = 8192
    MAX_OSD_E_ORDER = 20
    _destroy = "qldpc_osd_gpu_destroy"

    @staticmethod
    def supported(n, channel_probs, osd_method, osd_order) -> bool:
        p = np.broadcast_to(np.asarray(channel_probs, dtype=np.float64), (n,))
        try:
            meth = osd_method_code(osd_method)
        except ValueError:
            return False
        return (n <= DeviceOSD.MAX_N and bool(np.all((p > 0) & (p < 1))) and meth in (0, 1, 2)
                and not (meth == 1 and int(osd_order) > DeviceOSD.MAX_OSD_E_ORDER))

    def __init__(self, graph: DeviceGraph, channel_probs, osd_method="osd_e", osd_order=10):
        self.graph = graph
        self.osd_method = osd_method_code(osd_method)
        self.osd_order = int(osd_order)
        self._probs = _channel_probs(channel_probs, graph.n, check_length=False)
        self._create("qldpc_osd_gpu_create", graph.handle, _np_ptr(self._probs), self.osd_method, self.osd_order)

    def geometry(self) -> dict:
        """The elimination layout the handle chose: register-row words, column-window words (always
        0: the key stays for the ABI), threads per workgroup and the persistent grid."""
        return dict(zip(("row_words", "window_words", "threads", "workgroups"),
                        self._ints("qldpc_osd_gpu_geometry", "qldpc_osd_gpu_geometry", 4)))

    def set_side_probs(self, p0, p1):
        """Side tables on the GPU handle (``qldpc_osd_gpu_set_side_probs``), as :meth:`HostOSD.set_side_probs`."""
        n = self.graph.n
        a, b = _channel_probs(p0, n, check_length=False), _channel_probs(p1, n, check_length=False)
        _native.check(_native.lib().qldpc_osd_gpu_set_side_probs(self.handle, _np_ptr(a), _np_ptr(b)),
                      "qldpc_osd_gpu_set_side_probs")
        self.side_probs = (a, b)

    def decode_device(self, synd_dev, post_dev, conv_dev, corr_dev, out0_dev, outw_dev, stream=None, side_dev=None):
        """``side_dev``: device uint8 side bytes [B, n] of a side decode (``qldpc_osd_gpu_decode_side``)."""
        B = int(synd_dev.shape[0])
        if side_dev is not None:
            torch = _torch()
            assert side_dev.dtype == torch.uint8 and side_dev.is_contiguous()
            assert tuple(side_dev.shape) == (B, self.graph.n)
            _native.check(_native.lib().qldpc_osd_gpu_decode_side(
                self.handle, _ptr(synd_dev), _ptr(post_dev), _ptr(conv_dev), _ptr(corr_dev), _ptr(side_dev),
                _ptr(out0_dev), _ptr(outw_dev), B, _stream(stream, synd_dev.device)), "qldpc_osd_gpu_decode_side")
            return
        _native.check(_native.lib().qldpc_osd_gpu_decode(
            self.handle, _ptr(synd_dev), _ptr(post_dev), _ptr(conv_dev), _ptr(corr_dev), _ptr(out0_dev),
            _ptr(outw_dev), B, _stream(stream, synd_dev.device)), "qldpc_osd_gpu_decode")

    def bposd_batch(self, bp: "DeviceBP", synd, host_post: bool = True, side=None):
        """Soft BP (``bp``, soft=True) then GPU OSD, all on the device: ``synd`` [B, m] ->
        (osdw, osd0, bp_corr, iters, conv, post) as host arrays (``post`` stays a device
        tensor when ``host_post`` is False: 8 bytes per variable not worth copying back).
        ``side`` [B, n]: both stages are side decodes on the same bytes."""
        torch, dev, sd, corr, iters, conv = _decode_buffers(self.graph, synd, check_width=False)
        o0 = torch.empty_like(corr)
        ow = torch.empty_like(corr)
        st = _stream_handle(torch, dev)
        sb = None if side is None else torch.from_numpy(_side_bytes(side, sd.shape[0], self.graph.n)).to(dev)
        post = bp._decode_soft_device(sd, corr, iters, conv, st, side=sb)
        self.decode_device(sd, post, conv, corr, o0, ow, st, side_dev=sb)
        torch.cuda.synchronize(dev)
        return (ow.cpu().numpy(), o0.cpu().numpy(), corr.cpu().numpy().astype(np.int64), iters.cpu().numpy(),
                conv.cpu().numpy().astype(bool), post.cpu().numpy() if host_post else post)


class HostLSD(HostOSD):
    """BP+LSD's second stage on the host (``qldpc_osd_create_lsd``, csrc/lsd.hip): clusters grown
    around the unsatisfied checks in BP's reliability order, ``bits_per_step`` columns per cluster
    and round, elimination inside the clusters alone (the law: include/qldpc_hip.h).  A
    :class:`HostOSD` in every call.  At order 0 (``lsd_method="lsd_0"`` or ``lsd_order=0``) it uses no
    channel weights, so ``osd0 == osdw`` and a side decode equals the plain one.  ``lsd_method`` "lsd_e" /
    "lsd_cs" with ``lsd_order`` > 0 (``qldpc_osd_create_lsd_order``) grow every cluster to ``lsd_order``
    free columns and weigh candidates by ``channel_probs``: ``osdw`` is then the lightest, ``osd0`` the
    OSD-0 solution on the same clusters, and side tables are refused (``QLDPC_ENOTSUP``)."""

    def __init__(self, H, bits_per_step: int = 1, channel_probs=None, lsd_method="lsd_0", lsd_order: int = 0):
        c = H if isinstance(H, CSR) else CSR.from_dense(H)
        self.m, self.n = c.m, c.n
        self.osd_method, self.osd_order = 0, 0
        self.bits_per_step = int(bits_per_step)
        self.lsd_method, self.lsd_order = lsd_method_code(lsd_method), int(lsd_order)
        self._probs = None if channel_probs is None else _channel_probs(channel_probs, self.n)  # (the C side reads n)
        rp = np.ascontiguousarray(c.row_ptr, dtype=np.int32)
        ci = np.ascontiguousarray(c.col_idx, dtype=np.int32)
        self._create("qldpc_osd_create_lsd_order", self.m, self.n, _np_ptr(rp), _np_ptr(ci),
                     None if self._probs is None else _np_ptr(self._probs), self.bits_per_step, self.lsd_method,
                     self.lsd_order)
        self.rank, = self._ints("qldpc_osd_rank", "qldpc_osd_rank", 1)

    def weights(self) -> np.ndarray:
        """The integer candidate weights wq [n] of the handle (``qldpc_lsd_weights``)."""
        wq = np.zeros(self.n, np.int64)
        _native.check(_native.lib().qldpc_lsd_weights(self.handle, _np_ptr(wq)), "qldpc_lsd_weights")
        return wq

    def decode_batch_stats(self, synd, post, conv=None, bp_corr=None, threads: int = 0):
        """(x [B, n] uint8, stats [B, 4] int32 = valid, rounds, active columns, clusters)."""
        s = _syndromes(synd, self.m)
        B = s.shape[0]
        pst = np.ascontiguousarray(np.asarray(post, dtype=np.float64).reshape(B, self.n))
        cv = None if conv is None else np.ascontiguousarray(np.asarray(conv).reshape(B), dtype=np.uint8)
        bc = None if bp_corr is None else np.ascontiguousarray(np.asarray(bp_corr).reshape(B, self.n),
                                                                 dtype=np.uint8)
        x = np.zeros((B, self.n), np.uint8)
        st = np.zeros((B, 4), np.int32)
        vp = lambda a: None if a is None else _np_ptr(a)  # noqa: E731
        _native.check(_native.lib().qldpc_lsd_decode_batch_stats(
            self.handle, vp(s), vp(pst), vp(cv), vp(bc), vp(x), vp(st), B, int(threads)),
            "qldpc_lsd_decode_batch_stats")
        return x, st


class DeviceLSD(DeviceOSD):
    """BP+LSD's second stage on the GPU (``qldpc_osd_gpu_create_lsd``): one workgroup per
    non-converged syndrome, the whole cluster growth and solution inside the kernel.  A
    :class:`DeviceOSD` in every call (``DeviceMC.set_osd`` / ``set_staged_osd``, the
    phenomenological and circuit loops, ``bposd_batch``).  ``supported`` is the envelope of order 0; a handle
    of order > 0 keeps 4 m more bytes of tables in LDS, so near m = n = 8192 its creation can still answer
    ``QLDPC_ENOTSUP`` (:class:`~.decoders.BPLSD_Decoder` then keeps the host stage)."""

    MAX_M = 8192

    @staticmethod
    def supported(m, n) -> bool:  # noqa: D102 (the GPU stage's envelope)
        return m <= DeviceLSD.MAX_M and n <= DeviceOSD.MAX_N

    def __init__(self, graph: DeviceGraph, bits_per_step: int = 1, channel_probs=None, lsd_method="lsd_0",
                 lsd_order: int = 0):
        self.graph = graph
        self.osd_method, self.osd_order = 0, 0
        self.bits_per_step = int(bits_per_step)
        self.lsd_method, self.lsd_order = lsd_method_code(lsd_method), int(lsd_order)
        self._probs = None if channel_probs is None else _channel_probs(channel_probs, graph.n)
        self._create("qldpc_osd_gpu_create_lsd_order", graph.handle,
                     None if self._probs is None else _np_ptr(self._probs), self.bits_per_step, self.lsd_method,
                     self.lsd_order)

    def geometry(self) -> dict:
        """:meth:`DeviceOSD.geometry` (``row_words`` = 0) plus ``lds_rows``, the row capacity of the
        LDS image (0: the image lives in the HBM slice alone), and ``lds_bytes`` per workgroup."""
        g = super().geometry()
        g["lds_rows"], g["lds_bytes"] = self._ints("qldpc_lsd_gpu_info", "qldpc_lsd_gpu_info", 2)
        return g

    def retries(self) -> int:
        """Decodes since the last call that outgrew the LDS image and were decoded again on the HBM slice
        (``qldpc_lsd_gpu_retries``; waits for the device)."""
        v = ctypes.c_uint64()
        _native.check(_native.lib().qldpc_lsd_gpu_retries(self.handle, ctypes.byref(v)), "qldpc_lsd_gpu_retries")
        return int(v.value)

    def bplsd_batch_stats(self, bp: "DeviceBP", synd, side=None):
        """:meth:`DeviceOSD.bposd_batch` through ``qldpc_lsd_gpu_decode``: soft BP, then this stage with
        its statistics -> (x, stats [B, 4], bp_corr, iters, conv, post as a device tensor)."""
        torch, dev, sd, corr, iters, conv = _decode_buffers(self.graph, synd, check_width=False)
        x = torch.empty_like(corr)
        stats = torch.zeros((sd.shape[0], 4), dtype=torch.int32, device=dev)
        st = _stream_handle(torch, dev)
        sb = None if side is None else torch.from_numpy(_side_bytes(side, sd.shape[0], self.graph.n)).to(dev)
        post = bp._decode_soft_device(sd, corr, iters, conv, st, side=sb)
        self.decode_device_stats(sd, post, conv, corr, x, stats, st)
        torch.cuda.synchronize(dev)
        return (x.cpu().numpy(), stats.cpu().numpy(), corr.cpu().numpy().astype(np.int64), iters.cpu().numpy(),
                conv.cpu().numpy().astype(bool), post)

    def decode_device_stats(self, synd_dev, post_dev, conv_dev, corr_dev, out_dev, stats_dev, stream=None):
        _native.check(_native.lib().qldpc_lsd_gpu_decode(
            self.handle, _ptr(synd_dev), _ptr(post_dev), _ptr(conv_dev), _ptr(corr_dev), _ptr(out_dev),
            _ptr(stats_dev), int(synd_dev.shape[0]), _stream(stream, synd_dev.device)), "qldpc_lsd_gpu_decode")

    def decode_batch_stats(self, synd, post, conv=None, bp_corr=None):
        """Host arrays in, (x [B, n] uint8, stats [B, 4] int32) out: :meth:`HostLSD.decode_batch_stats`
        on the GPU."""
        torch = _torch()
        s = _syndromes(synd, self.graph.m)
        B, n = s.shape[0], self.graph.n
        dev = torch.device("cuda", self.graph.device)

        def up(a, shape, dtype):
            return None if a is None else torch.from_numpy(
                np.ascontiguousarray(np.asarray(a).reshape(shape), dtype=dtype)).to(dev)

        sd, pd = torch.from_numpy(s).to(dev), up(post, (B, n), np.float64)
        cd, bd = up(conv, (B,), np.uint8), up(bp_corr, (B, n), np.uint8)
        x = torch.zeros((B, n), dtype=torch.uint8, device=dev)
        st = torch.zeros((B, 4), dtype=torch.int32, device=dev)
        self.decode_device_stats(sd, pd, cd, bd, x, st)
        torch.cuda.synchronize(dev)
        return x.cpu().numpy(), st.cpu().numpy()


class DeviceFirstMin(_Handle):
    """``FirstMinBPDecoder`` (``src/Decoders.py:49-74``) on the GPU (``qldpc_firstmin_*``): one-iteration
    min-sum BP repeated on the running syndrome while its weight does not grow, at most
    ``max_iter`` accepted steps, the whole loop in one kernel (one workgroup per syndrome)."""

    _destroy = "qldpc_firstmin_destroy"

    def __init__(self, H, channel_probs, max_iter: int, ms_scaling_factor=0.625, precision: int = 64,
                 device: int | None = None, graph: DeviceGraph | None = None):
        self.graph = graph if graph is not None else DeviceGraph(H, device=device)
        self._probs = _channel_probs(channel_probs, self.graph.n)
        self.max_iter = int(max_iter)
        self._create("qldpc_firstmin_create", self.graph.handle, _np_ptr(self._probs), self.max_iter,
                     float(ms_scaling_factor), int(precision))

    THREADS = 256  # per workgroup, in both loop kernels (csrc/firstmin.hip)

    def geometry(self) -> dict:
        """The launch ``decode_device`` would make now (``qldpc_firstmin_info``): ``grid`` resident
        workgroups of the workgroup kernel, ``lds_bytes`` per workgroup of the kernel it takes and
        ``wave`` (1: one wave per syndrome, 0: one workgroup; ``QLDPC_FM_WAVE`` is read per call)."""
        g = dict(zip(("grid", "lds_bytes", "wave"), self._ints("qldpc_firstmin_info", "qldpc_firstmin_info", 3)))
        g["threads"] = self.THREADS
        return g

    def decode_device(self, synd_dev, corr_dev, steps_dev=None, stream=None):
        _native.check(_native.lib().qldpc_firstmin_decode(
            self.handle, _ptr(synd_dev), _ptr(corr_dev), _ptr(steps_dev), int(synd_dev.shape[0]),
            _stream(stream, synd_dev.device)), "qldpc_firstmin_decode")

    def decode_batch(self, synd):
        """[B, m] syndromes -> (corrections [B, n] int64, accepted steps [B] int32)."""
        torch = _torch()
        S = _syndromes(synd, self.graph.m)
        B, n = S.shape[0], self.graph.n
        dev = torch.device("cuda", self.graph.device)
        sd = torch.from_numpy(S).to(dev)
        corr = torch.empty((B, n), dtype=torch.uint8, device=dev)
        steps = torch.empty(B, dtype=torch.int32, device=dev)
        self.decode_device(sd, corr, steps)
        torch.cuda.synchronize(dev)
        return corr.cpu().numpy().astype(np.int64), steps.cpu().numpy()


@dataclass
class MCResult:
    shots: int
    failures: int
    sector_decodes: list
    sector_iters: list
    sector_nonconv: list
    sector_fail: list
    iter_hist: np.ndarray  # [2, HIST_BINS]
    fail: np.ndarray | None = None
    err: np.ndarray | None = None
    corr: np.ndarray | None = None
    iters: np.ndarray | None = None
    trace: np.ndarray | None = None
    detobs: np.ndarray | None = None

    @staticmethod
    def from_words(w: np.ndarray) -> "MCResult":
        w = np.asarray(w, dtype=np.int64)
        hb = _native.HIST_BINS
        return MCResult(int(w[0]), int(w[1]), w[2:4].tolist(), w[4:6].tolist(), w[6:8].tolist(), w[8:10].tolist(),
                        w[10:10 + 2 * hb].reshape(2, hb).copy())

    def merge(self, o: "MCResult") -> "MCResult":
        return MCResult(self.shots + o.shots, self.failures + o.failures,
                        [a + b for a, b in zip(self.sector_decodes, o.sector_decodes)],
                        [a + b for a, b in zip(self.sector_iters, o.sector_iters)],
                        [a + b for a, b in zip(self.sector_nonconv, o.sector_nonconv)],
                        [a + b for a, b in zip(self.sector_fail, o.sector_fail)], self.iter_hist + o.iter_hist)


def _upload_uniforms(uniforms, device, shots, per_shot):
    """External uniforms ``[shots, per_shot]`` (CPython ``random()`` values) as a float64 tensor on
    GPU ``device``; None stays None (the kernels then draw from Philox)."""
    torch = _torch()
    if uniforms is None:
        return None
    u = torch.from_numpy(np.ascontiguousarray(uniforms, dtype=np.float64)).to(torch.device("cuda", device))
    if tuple(u.shape) != (shots, per_shot):
        raise ValueError(f"uniforms must be [{shots}, {per_shot}]")
    return u


def _run_and_read(device, launch, per_shot: dict) -> MCResult:
    """One synchronous run of a fused loop on GPU ``device``: fresh counters, ``launch(counters,
    *buffers)``, synchronise, the counters as an :class:`MCResult`.  ``per_shot`` maps MCResult
    fields to (shape, dtype name) of the zeroed device buffers the launch fills, in the launch's
    argument order; they are read back into those fields."""
    torch = _torch()
    dev = torch.device("cuda", device)
    cnt = _new_counters(device)
    bufs = [torch.zeros(shape, dtype=getattr(torch, dtype), device=dev) for shape, dtype in per_shot.values()]
    launch(cnt, *bufs)
    torch.cuda.synchronize(dev)
    res = MCResult.from_words(cnt.cpu().numpy())
    for name, b in zip(per_shot, bufs):
        setattr(res, name, b.cpu().numpy())
    return res


class DeviceMC(_Handle):
    """Fused shot loop of ``CodeSimulator_DataError`` on one GPU (``qldpc_mc_*``).

    Sector X decodes X errors with the hz decoder and checks lz; sector Z
    decodes Z errors with the hx decoder and checks lx.  ``staged=True`` forces the staged
    pipeline (``qldpc_mc_create_staged``), the one :meth:`launch_weight` runs on.
    """

    _destroy = "qldpc_mc_destroy"

    def __init__(self, code: CSSCode, dec_x: DeviceBP | None, dec_z: DeviceBP | None, staged: bool = False):
        self.code = code
        self.dec_x, self.dec_z = dec_x, dec_z
        dev = (dec_x or dec_z).graph.device
        self.device = dev
        self.staged = bool(staged)
        self.lz = DeviceGraph(code.csr("lz"), device=dev) if dec_x is not None else None
        self.lx = DeviceGraph(code.csr("lx"), device=dev) if dec_z is not None else None
        self._create("qldpc_mc_create_staged" if staged else "qldpc_mc_create", _handle(dec_x), _handle(self.lz),
                     _handle(dec_z), _handle(self.lx))

    def set_osd(self, osd_x: "DeviceOSD | None", osd_z: "DeviceOSD | None"):
        """BP+OSD in the fused loop (``qldpc_mc_set_osd``): decodes that reach max_iter go through the
        GPU OSD stage and their failures are re-checked on the device."""
        self._osd = (osd_x, osd_z)  # keep the handles alive
        _native.check(_native.lib().qldpc_mc_set_osd(self.handle, _handle(osd_x), _handle(osd_z)), "qldpc_mc_set_osd")

    def set_staged_osd(self, osd_x: "DeviceOSD | None", osd_z: "DeviceOSD | None"):
        """BP+OSD in the staged loop (``qldpc_mc_set_staged_osd``): each sector's soft BP (engine 7
        without legs, or engine 8 with ``soft=True``) is followed by the GPU OSD over the batch, and
        OSD's correction is the sector's.  With a channel update the second sector's OSD is a side
        decode (:meth:`DeviceOSD.set_side_probs`).  Staged handles only."""
        self._staged_osd = (osd_x, osd_z)  # keep the handles alive
        _native.check(_native.lib().qldpc_mc_set_staged_osd(self.handle, _handle(osd_x), _handle(osd_z)),
                      "qldpc_mc_set_staged_osd")

    def set_channel_update(self, direction):
        """X/Z-correlated decoding (``qldpc_mc_set_channel_update``): None, ``"x->z"`` or ``"z->x"``.  The
        first sector's corrections are the side bytes of the second sector's decode, whose decoder
        needs side priors (:meth:`DeviceBP.set_side_probs`).  Staged handles only."""
        if direction not in CHANNEL_UPDATES:
            raise ValueError(f"channel update must be None, 'x->z' or 'z->x', not {direction!r}")
        _native.check(_native.lib().qldpc_mc_set_channel_update(self.handle, CHANNEL_UPDATES[direction]),
                      "qldpc_mc_set_channel_update")
        self.channel_update = direction

    def new_counters(self):
        return _new_counters(self.device)

    def launch(self, px, py, pz, seed, shot_begin, shot_count, logical_mode="X", counters=None, uniforms=None,
               fail=None, err=None, corr=None, iters=None, grid_blocks=0, stream=None):
        """Asynchronous launch on the current stream; counters accumulate in ``counters`` (device int64)."""
        mode, s = _launch_prep(counters, logical_mode, stream)
        _native.check(_native.lib().qldpc_mc_launch(
            self.handle, float(px), float(py), float(pz), _seed64(seed), int(shot_begin), int(shot_count),
            mode, _ptr(uniforms), _ptr(counters), _ptr(fail), _ptr(err), _ptr(corr), _ptr(iters), int(grid_blocks), s),
            "qldpc_mc_launch")

    def _per_shot(self, shot_count, per_shot) -> dict:
        """The per-shot buffers of :meth:`launch` / :meth:`launch_weight` for :func:`_run_and_read`."""
        S, n = int(shot_count), self.code.N
        if not per_shot:
            return {}
        return {"fail": (S, "uint8"), "err": ((S, n), "uint8"), "corr": ((S, 2, n), "uint8"), "iters": ((S, 2), "int32")}

    def run(self, px, py, pz, seed, shot_begin, shot_count, logical_mode="X", uniforms=None, per_shot=False,
            grid_blocks=0) -> MCResult:
        S = int(shot_count)
        u = _upload_uniforms(uniforms, self.device, S, self.code.N)

        def launch(cnt, *b):
            self.launch(px, py, pz, seed, shot_begin, S, logical_mode, cnt, u, *(b or (None,) * 4), grid_blocks)

        return _run_and_read(self.device, launch, self._per_shot(S, per_shot))

    def launch_weight(self, weight, px, py, pz, seed, shot_begin, shot_count, logical_mode="X", counters=None,
                      fail=None, err=None, corr=None, iters=None, stream=None):
        """:meth:`launch` on errors of fixed ``weight`` (``qldpc_mc_launch_weight``): uniform random
        ``weight``-subsets of the qubits with Pauli classes in the ratio ``px : py : pz``.  Needs a
        ``staged=True`` handle."""
        mode, s = _launch_prep(counters, logical_mode, stream)
        _native.check(_native.lib().qldpc_mc_launch_weight(
            self.handle, int(weight), float(px), float(py), float(pz), _seed64(seed), int(shot_begin),
            int(shot_count), mode, _ptr(counters), _ptr(fail), _ptr(err), _ptr(corr), _ptr(iters), s),
            "qldpc_mc_launch_weight")

    def run_weight(self, weight, px, py, pz, seed, shot_begin, shot_count, logical_mode="X",
                   per_shot=False) -> MCResult:
        S = int(shot_count)
        return _run_and_read(self.device, lambda cnt, *b: self.launch_weight(
            weight, px, py, pz, seed, shot_begin, S, logical_mode, cnt, *b), self._per_shot(S, per_shot))


def sample_errors_weight(n, weight, px, py, pz, seed, shot_begin, shot_count, host: bool = False,
                         device: int | None = None, stream=None):
    """``qldpc_sample_errors_weight``: ``shot_count`` errors of exactly ``weight`` non-zero Pauli
    classes on ``n`` qubits, the sampler of :meth:`DeviceMC.launch_weight` alone, as a uint8
    ``[S, n]`` device tensor (bit0 = x, bit1 = z).  ``host=True``: the same law in plain C++
    (``qldpc_sample_errors_weight_host``, no GPU needed) as a numpy array."""
    S = int(shot_count)
    args = (int(weight), float(px), float(py), float(pz), _seed64(seed), int(shot_begin), S, int(n))
    if host:
        out = np.zeros((max(S, 0), max(int(n), 0)), dtype=np.uint8)
        _native.check(_native.lib().qldpc_sample_errors_weight_host(*args, _np_ptr(out)),
                      "qldpc_sample_errors_weight_host")
        return out
    torch = _torch()
    dev = torch.device("cuda", _device_index(device))
    out = torch.empty((S, int(n)), dtype=torch.uint8, device=dev)
    s = _stream(stream, dev)
    with torch.cuda.device(dev):
        _native.check(_native.lib().qldpc_sample_errors_weight(*args, _ptr(out), s), "qldpc_sample_errors_weight")
    return out


def relay_gammas(n, relay, precision: int = 64):
    """``qldpc_relay_gammas``: the memory strengths ``[num_legs + 1, n]`` of a Relay-BP decoder with
    the :class:`RelayParams` ``relay`` (row 0 = ``pre_gamma``), as the kernels hold them (rounded to
    float for ``precision`` 32), widened to float64.  Host only: needs the library, not a GPU."""
    r = RelayParams.of(relay)
    out = np.zeros((max(int(r.num_legs), -1) + 1, int(n)), dtype=np.float64)
    _native.check(_native.lib().qldpc_relay_gammas(int(n), float(r.pre_gamma), int(r.num_legs), float(r.gamma_lo),
                                                   float(r.gamma_hi), _seed64(r.gamma_seed), int(precision),
                                                   _np_ptr(out)), "qldpc_relay_gammas")
    return out


def relay_decode_host(H, channel_probs, relay, synd, ms_scaling_factor=0.625, precision: int = 64, threads: int = 0):
    """``qldpc_relay_decode_host``: the Relay-BP law in plain C++ on host memory (no GPU, any graph):
    ``synd`` [B, m] -> (corr [B, n] int64, iters [B], converged [B] bool, solutions found [B])."""
    c = H if isinstance(H, CSR) else CSR.from_dense(H)
    r = RelayParams.of(relay)
    s = _syndromes(synd, c.m)
    B = s.shape[0]
    probs = _channel_probs(channel_probs, c.n)
    rp = np.ascontiguousarray(c.row_ptr, dtype=np.int32)
    ci = np.ascontiguousarray(c.col_idx, dtype=np.int32)
    corr = np.zeros((B, c.n), np.uint8)
    iters = np.zeros(B, np.int32)
    conv = np.zeros(B, np.uint8)
    nsol = np.zeros(B, np.int32)
    _native.check(_native.lib().qldpc_relay_decode_host(
        c.m, c.n, _np_ptr(rp), _np_ptr(ci), _np_ptr(probs), *r.abi(ms_scaling_factor, precision), _np_ptr(s),
        _np_ptr(corr), _np_ptr(iters), _np_ptr(conv), _np_ptr(nsol), B, int(threads)), "qldpc_relay_decode_host")
    return corr.astype(np.int64), iters, conv.astype(bool), nsol


def _host_side_args(H, p0, p1, synd, side):
    c = H if isinstance(H, CSR) else CSR.from_dense(H)
    s = _syndromes(synd, c.m)
    B = s.shape[0]
    return (c, s, B, _channel_probs(p0, c.n), _channel_probs(p1, c.n), _side_bytes(side, B, c.n),
            np.ascontiguousarray(c.row_ptr, dtype=np.int32), np.ascontiguousarray(c.col_idx, dtype=np.int32))


def relay_decode_host_side(H, p0, p1, relay, synd, side, ms_scaling_factor=0.625, precision: int = 64,
                           threads: int = 0):
    """``qldpc_relay_decode_host_side``: :func:`relay_decode_host` under side priors: variable j of
    syndrome b takes its prior and solution weight from ``p1`` when ``side[b, j] & 1``, else ``p0``."""
    c, s, B, a, b, sb, rp, ci = _host_side_args(H, p0, p1, synd, side)
    r = RelayParams.of(relay)
    corr = np.zeros((B, c.n), np.uint8)
    iters = np.zeros(B, np.int32)
    conv = np.zeros(B, np.uint8)
    nsol = np.zeros(B, np.int32)
    _native.check(_native.lib().qldpc_relay_decode_host_side(
        c.m, c.n, _np_ptr(rp), _np_ptr(ci), _np_ptr(a), _np_ptr(b), _np_ptr(sb), *r.abi(ms_scaling_factor, precision),
        _np_ptr(s), _np_ptr(corr), _np_ptr(iters), _np_ptr(conv), _np_ptr(nsol), B, int(threads)),
        "qldpc_relay_decode_host_side")
    return corr.astype(np.int64), iters, conv.astype(bool), nsol


def serial_decode_host_side(H, p0, p1, max_iter, synd, side, ms_scaling_factor=0.625, precision: int = 64,
                            threads: int = 0):
    """``qldpc_serial_decode_host_side``: :func:`serial_decode_host` under side priors (no posteriors):
    ``synd`` [B, m], ``side`` [B, n] -> (corr [B, n] int64, iters [B], converged [B] bool)."""
    c, s, B, a, b, sb, rp, ci = _host_side_args(H, p0, p1, synd, side)
    corr = np.zeros((B, c.n), np.uint8)
    iters = np.zeros(B, np.int32)
    conv = np.zeros(B, np.uint8)
    _native.check(_native.lib().qldpc_serial_decode_host_side(
        c.m, c.n, _np_ptr(rp), _np_ptr(ci), _np_ptr(a), _np_ptr(b), _np_ptr(sb), int(max_iter),
        float(ms_scaling_factor), int(precision), _np_ptr(s), _np_ptr(corr), _np_ptr(iters), _np_ptr(conv), B,
        int(threads)), "qldpc_serial_decode_host_side")
    return corr.astype(np.int64), iters, conv.astype(bool)


def serial_layers(H):
    """``qldpc_serial_layers``: the layer of every variable under the serial schedule's first-fit rule
    (include/qldpc_hip.h) and the number of layers.  Host only: needs the library, not a GPU."""
    c = H if isinstance(H, CSR) else CSR.from_dense(H)
    rp = np.ascontiguousarray(c.row_ptr, dtype=np.int32)
    ci = np.ascontiguousarray(c.col_idx, dtype=np.int32)
    layer = np.zeros(max(c.n, 1), np.int32)
    num = ctypes.c_int32(0)
    _native.check(_native.lib().qldpc_serial_layers(c.m, c.n, _np_ptr(rp), _np_ptr(ci), _np_ptr(layer),
                                                    ctypes.byref(num)), "qldpc_serial_layers")
    return layer[:c.n], int(num.value)


def serial_decode_host(H, channel_probs, max_iter, synd, ms_scaling_factor=0.625, precision: int = 64,
                       threads: int = 0):
    """``qldpc_serial_decode_host``: the serial-schedule min-sum law in plain C++ on host memory (no
    GPU, any graph): ``synd`` [B, m] -> (corr [B, n] int64, iters [B], converged [B] bool, posteriors
    [B, n] float64)."""
    c = H if isinstance(H, CSR) else CSR.from_dense(H)
    s = _syndromes(synd, c.m)
    B = s.shape[0]
    probs = _channel_probs(channel_probs, c.n)
    rp = np.ascontiguousarray(c.row_ptr, dtype=np.int32)
    ci = np.ascontiguousarray(c.col_idx, dtype=np.int32)
    corr = np.zeros((B, c.n), np.uint8)
    iters = np.zeros(B, np.int32)
    conv = np.zeros(B, np.uint8)
    post = np.zeros((B, c.n), np.float64)
    _native.check(_native.lib().qldpc_serial_decode_host(
        c.m, c.n, _np_ptr(rp), _np_ptr(ci), _np_ptr(probs), int(max_iter), float(ms_scaling_factor), int(precision),
        _np_ptr(s), _np_ptr(corr), _np_ptr(iters), _np_ptr(conv), _np_ptr(post), B, int(threads)),
        "qldpc_serial_decode_host")
    return corr.astype(np.int64), iters, conv.astype(bool), post


def sample_errors(n, px, py, pz, seed, shot_begin, shot_count, uniforms=None, device: int | None = None,
                  stream=None):
    """``qldpc_sample_errors``: the sampling step of the fused kernels alone
    (``CodeSimulator_DataError._generate_error``, src/Simulators.py:89-115) as a uint8
    ``[S, n]`` device tensor (bit0 = x, bit1 = z), from the Philox stream keyed by the
    global shot index or from external uniforms ``[S, n]`` (CPython ``random()`` values)."""
    torch = _torch()
    dev = torch.device("cuda", _device_index(device))
    S = int(shot_count)
    out = torch.empty((S, int(n)), dtype=torch.uint8, device=dev)
    u = None
    if uniforms is not None:
        u = uniforms if isinstance(uniforms, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(uniforms, dtype=np.float64))
        u = u.to(dev, dtype=torch.float64).contiguous()
        if tuple(u.shape) != (S, int(n)):
            raise ValueError(f"uniforms must be [{S}, {n}]")
    s = _stream(stream, dev)
    with torch.cuda.device(dev):
        _native.check(_native.lib().qldpc_sample_errors(
            float(px), float(py), float(pz), _seed64(seed), int(shot_begin), S, int(n), _ptr(u), _ptr(out), s),
            "qldpc_sample_errors")
    return out


def run_sharded(mcs, comms, px, py, pz, seed, shot_begin, shot_count, logical_mode="Total") -> MCResult:
    """``qldpc_mc_run_sharded``: one host thread drives one :class:`DeviceMC` per GPU (each on its
    own device's decoders) over contiguous blocks of the global shots, and sums the counters with
    one grouped RCCL all-reduce (``comms`` from :meth:`parallel.NativeComm.init_all`, same device
    order; None for one device).  The totals equal one device running all the shots."""
    mcs = list(mcs)
    nd = len(mcs)
    arr = (ctypes.c_void_p * nd)(*[m.handle.value for m in mcs])
    carr = None
    if comms is not None:
        comms = list(comms)
        if len(comms) != nd:
            raise ValueError("one communicator per MC handle")
        carr = (ctypes.c_void_p * nd)(*[c.handle.value for c in comms])
    out = _native.Counters()
    _native.check(_native.lib().qldpc_mc_run_sharded(
        ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p)),
        ctypes.cast(carr, ctypes.POINTER(ctypes.c_void_p)) if carr is not None else None, nd, float(px), float(py),
        float(pz), _seed64(seed), int(shot_begin), int(shot_count), _logical_mode(logical_mode), ctypes.byref(out)),
        "qldpc_mc_run_sharded")
    return MCResult.from_words(np.frombuffer(bytes(out), dtype=np.int64))


class DevicePhenl(_Handle):
    """Phenomenological space-time shot loop of ``CodeSimulator_Phenon_SpaceTime`` on one GPU (``qldpc_phenl_*``).

    ``st_x`` / ``st_z`` decode the X / Z detector histories on the space-time
    graphs of hz / hx; ``dec2_x`` / ``dec2_z`` decode the perfect final round.
    """

    _destroy = "qldpc_phenl_destroy"

    def __init__(self, code: CSSCode, st_x: DeviceBP, st_z: DeviceBP, dec2_x: DeviceBP, dec2_z: DeviceBP,
                 num_rep: int, max_batch: int = 0):
        self.code = code
        self.num_rep = int(num_rep)
        self.decoders = (st_x, st_z, dec2_x, dec2_z)
        dev = dec2_x.graph.device
        self.device = dev
        self.lz = DeviceGraph(code.csr("lz"), device=dev)
        self.lx = DeviceGraph(code.csr("lx"), device=dev)
        self._create("qldpc_phenl_create", st_x.handle, st_z.handle, dec2_x.handle, dec2_z.handle, self.lz.handle,
                     self.lx.handle, self.num_rep, int(max_batch))

    def set_final_osd(self, osd_x: "DeviceOSD | None", osd_z: "DeviceOSD | None"):
        """BP+OSD final round (decoder2 = BPOSD_Decoder): ``qldpc_phenl_set_final_osd``."""
        for o, d in ((osd_x, self.decoders[2]), (osd_z, self.decoders[3])):
            if o is not None and o.graph.n != d.n:
                raise ValueError("OSD graph does not match the final-round decoder")
        self._osd2 = (osd_x, osd_z)  # keep the handles alive
        _native.check(_native.lib().qldpc_phenl_set_final_osd(self.handle, _handle(osd_x), _handle(osd_z)),
                      "qldpc_phenl_set_final_osd")

    def set_round_firstmin(self, fm_x: "DeviceFirstMin | None", fm_z: "DeviceFirstMin | None"):
        """Noisy rounds decoded by FirstMinBPDecoder (``qldpc_phenl_set_round_firstmin``): each
        handle must be built on exactly its sector's space-time graph."""
        self._fm1 = (fm_x, fm_z)  # keep the handles alive
        _native.check(_native.lib().qldpc_phenl_set_round_firstmin(self.handle, _handle(fm_x), _handle(fm_z)),
                      "qldpc_phenl_set_round_firstmin")

    def trace_len(self, num_rounds: int) -> int:
        v = ctypes.c_int64()
        _native.check(_native.lib().qldpc_phenl_trace_len(self.handle, int(num_rounds), ctypes.byref(v)),
                      "qldpc_phenl_trace_len")
        return v.value

    def uniforms_per_sample(self, num_rounds: int) -> int:
        c = self.code
        return ((num_rounds - 1) * self.num_rep + 1) * (c.N + c.hx.shape[0] + c.hz.shape[0])

    def new_counters(self):
        return _new_counters(self.device)

    def launch(self, px, py, pz, q, seed, shot_begin, shot_count, num_rounds, logical_mode="Total", counters=None,
               uniforms=None, fail=None, trace=None, stream=None):
        mode, s = _launch_prep(counters, logical_mode, stream)
        _native.check(_native.lib().qldpc_phenl_launch(
            self.handle, float(px), float(py), float(pz), float(q), _seed64(seed), int(shot_begin),
            int(shot_count), int(num_rounds), mode, _ptr(uniforms), _ptr(counters), _ptr(fail), _ptr(trace), s),
            "qldpc_phenl_launch")

    def run(self, px, py, pz, q, seed, shot_begin, shot_count, num_rounds, logical_mode="Total", uniforms=None,
            per_shot=False) -> MCResult:
        S = int(shot_count)
        u = _upload_uniforms(uniforms, self.device, S, self.uniforms_per_sample(num_rounds))
        bufs = {"fail": (S, "uint8"), "trace": ((S, self.trace_len(num_rounds)), "uint8")} if per_shot else {}

        def launch(cnt, *b):
            self.launch(px, py, pz, q, seed, shot_begin, S, num_rounds, logical_mode, cnt, u, *b)

        return _run_and_read(self.device, launch, bufs)


class DeviceCircuit(_Handle):
    """Circuit-level space-time shot loop of ``CodeSimulator_Circuit_SpaceTime`` on one GPU
    (``qldpc_circ_*``, csrc/circuit.hip).

    ``dem`` is the FULL circuit's detector error model (:class:`~.circuit.DetectorErrorModel`),
    ``dec1`` decodes each round on h1 (num_rep·m rows), ``dec2`` the final layer on h2; ``hs``
    (h1_space_cor), ``L1`` and ``L2`` are dense 0/1 matrices as ``GenCorrecHyperGraph`` /
    ``GenFaultHyperGraph`` return them.  ``osd``: a :class:`DeviceOSD` (uniform priors) or a
    :class:`HostOSD` on h2 makes decoder2 BP+OSD (``dec2`` built with ``soft=True``).  ``sampler``:
    "skip" (default: geometric gaps per mechanism and global 64-sample word) or "keyed" (one Philox
    uniform per (sample, mechanism)); both exact and shard-invariant, different draws
    (``qldpc_circ_set_sampler``).
    """

    SAMPLERS = {"keyed": 0, "skip": 1}
    _destroy = "qldpc_circ_destroy"

    def __init__(self, dem, dec1: "DeviceBP | None" = None, hs=None, L1=None, dec2: "DeviceBP | None" = None, L2=None,
                 num_rounds: int = 0, num_rep: int = 1, osd=None, max_batch: int = 0, device: int | None = None,
                 sampler: str = "skip"):
        sampler_only = dec1 is None and dec2 is None
        if device is None and dec1 is not None:
            device = dec1.graph.device
        dev = _device_index(device)
        self.device = dev
        self.dem = dem
        self.decoders = (dec1, dec2)
        self.num_rounds, self.num_rep = int(num_rounds), int(num_rep)
        mats = [dem.check_matrix(), dem.observable_matrix()] + ([] if sampler_only else [hs, L1, L2])
        self._g = [DeviceGraph(np.asarray(a, dtype=np.uint8) % 2, device=dev) for a in mats]
        self._probs = np.ascontiguousarray(np.asarray(dem.probs, dtype=np.float64))
        hd = (lambda i: None) if sampler_only else (lambda i: self._g[i].handle)  # noqa: E731
        self._create("qldpc_circ_create", self._g[0].handle, self._g[1].handle, _np_ptr(self._probs),
                     None if sampler_only else dec1.handle, hd(2), hd(3), None if sampler_only else dec2.handle, hd(4),
                     self.num_rounds, self.num_rep, int(max_batch))
        self._set_sampler_and_osd(sampler, osd)

    def _set_sampler_and_osd(self, sampler, osd):
        """The tail of construction: the DEM sampler and decoder2's OSD stage."""
        self.sampler = sampler
        _native.check(_native.lib().qldpc_circ_set_sampler(self.handle, self.SAMPLERS[sampler]),
                      "qldpc_circ_set_sampler")
        self._osd = osd
        if osd is not None:
            gpu = osd.handle if isinstance(osd, DeviceOSD) else None
            host = osd.handle if isinstance(osd, HostOSD) else None
            _native.check(_native.lib().qldpc_circ_set_final_osd(self.handle, gpu, host), "qldpc_circ_set_final_osd")

    @property
    def num_detectors(self) -> int:
        return self.dem.num_detectors

    @property
    def num_observables(self) -> int:
        return self.dem.num_observables

    def new_counters(self):
        return _new_counters(self.device)

    def launch(self, seed, shot_begin, shot_count, counters, fail=None, detobs=None, stream=None):
        _native.check(_native.lib().qldpc_circ_launch(
            self.handle, _seed64(seed), int(shot_begin), int(shot_count), _ptr(counters), _ptr(fail), _ptr(detobs),
            _stream(stream, counters.device)), "qldpc_circ_launch")

    def sample(self, seed, shot_begin, shot_count):
        """Detector + observable bits [S, D + K] (uint8, host) of samples ``shot_begin..`` — the
        ``detector_sampler.sample(shots, append_observables=True)`` of the reference."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        S = int(shot_count)
        out = torch.zeros((S, self.num_detectors + self.num_observables), dtype=torch.uint8, device=dev)
        _native.check(_native.lib().qldpc_circ_sample(self.handle, _seed64(seed), int(shot_begin), S, _ptr(out),
                                                      _stream_handle(torch, dev)), "qldpc_circ_sample")
        torch.cuda.synchronize(dev)
        return out.cpu().numpy()

    def run(self, seed, shot_begin, shot_count, per_shot: bool = False) -> "MCResult":
        """Counters of ``shot_count`` samples (``per_shot``: also ``fail`` [S] and the sampled
        detector / observable bits ``detobs`` [S, D + K] as host arrays)."""
        S = int(shot_count)
        bufs = {"fail": (S, "uint8"), "detobs": ((S, self.num_detectors + self.num_observables), "uint8")} \
            if per_shot else {}
        return _run_and_read(self.device, lambda cnt, *b: self.launch(seed, shot_begin, S, cnt, *b), bufs)


def _dem_csr(rows_of, num_rows: int, num_cols: int):
    """CSR of a DEM matrix from its per-mechanism row lists (``dem.dets`` / ``dem.obs``), without the
    dense [rows x mechanisms] array: the threshold sweeps reach 10^4 detectors x 10^5 mechanisms."""
    lens = np.fromiter((len(r) for r in rows_of), dtype=np.int64, count=len(rows_of))
    rows = np.fromiter((d for r in rows_of for d in r), dtype=np.int64, count=int(lens.sum()))
    cols = np.repeat(np.arange(len(rows_of), dtype=np.int64), lens)
    order = np.lexsort((cols, rows))
    row_ptr = np.zeros(num_rows + 1, dtype=np.int64)
    np.add.at(row_ptr, rows + 1, 1)
    return CSR(int(num_rows), int(num_cols), np.cumsum(row_ptr).astype(np.int32), cols[order].astype(np.int32))


class DeviceCircuitSingleShot(DeviceCircuit):
    """Single-shot circuit loop of ``CodeSimulator_Circuit`` on one GPU (``qldpc_circ_create_single_shot``,
    csrc/circuit.hip): ``dem`` is the single-shot circuit's DEM (``num_cycles * m`` detectors),
    ``dec1`` decodes every cycle but the last on ``[hx | I]``, ``dec2`` the last one on ``hx``; only
    the data part of a decoder1 correction is applied (``hx``, ``lx``: dense 0/1 matrices of the
    evaluated sector).  ``firstmin``: a :class:`DeviceFirstMin` on ``[hx | I]`` decodes the cycles
    instead (``dec1`` may then be None).  ``launch`` / ``sample`` / ``run``, the OSD and the sampler
    are :class:`DeviceCircuit`'s; counters: sector 0 = decoder1 (``num_cycles - 1`` per sample),
    sector 1 = decoder2."""

    def __init__(self, dem, dec1: "DeviceBP | None", hx, lx, dec2: "DeviceBP", num_cycles: int, osd=None,
                 firstmin: "DeviceFirstMin | None" = None, max_batch: int = 0, sampler: str = "skip"):
        dev = dec2.graph.device
        self.device = dev
        self.dem = dem
        self.decoders = (dec1, dec2)
        self.num_cycles = int(num_cycles)
        self.num_rounds, self.num_rep = self.num_cycles - 1, 1
        hx = np.asarray(hx, dtype=np.uint8) % 2
        lx = np.asarray(lx, dtype=np.uint8) % 2
        m = hx.shape[0]
        pad = np.zeros((lx.shape[0], m), np.uint8)
        M = dem.num_errors
        mats = [_dem_csr(dem.dets, dem.num_detectors, M), _dem_csr(dem.obs, dem.num_observables, M),
                np.hstack([hx, np.zeros((m, m), np.uint8)]), np.hstack([lx, pad]), lx]
        self._g = [DeviceGraph(a, device=dev) for a in mats]
        self._probs = np.ascontiguousarray(np.asarray(dem.probs, dtype=np.float64))
        self._create("qldpc_circ_create_single_shot", self._g[0].handle, self._g[1].handle, _np_ptr(self._probs),
                     _handle(dec1), self._g[2].handle, self._g[3].handle, dec2.handle, self._g[4].handle,
                     self.num_cycles, int(max_batch))
        self._set_sampler_and_osd(sampler, osd)
        self._fm1 = None
        if firstmin is not None:
            self.set_round_firstmin(firstmin)

    def set_round_firstmin(self, fm: "DeviceFirstMin | None"):
        """Cycles decoded by FirstMinBPDecoder (``qldpc_circ_set_round_firstmin``); None: back to dec1."""
        _native.check(_native.lib().qldpc_circ_set_round_firstmin(self.handle, _handle(fm)),
                      "qldpc_circ_set_round_firstmin")
        self._fm1 = fm  # keep the handle alive

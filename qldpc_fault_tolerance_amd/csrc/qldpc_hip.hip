// qldpc_hip.hip — host runtime + C ABI (include/qldpc_hip.h) of the MI355X engine.
//
// Graph/decoder/MC handles own their device buffers; launches take a caller
// stream.  Three kernel engines are built:
//   engine 3 (default) — bp_reg.h: engine 2's LDS image with each thread's
//                        variables (edge addresses, priors, own messages)
//                        resident in VGPRs, compile-time VPL <= 8, column
//                        degree <= 4 and an image addressable with 16 bits;
//   engine 2           — bp_slot.h: small workgroups with streamed variables,
//                        row-major v2c slots, check-centric gather, NS decodes
//                        in flight per workgroup (any graph that fits LDS);
//   engine 1           — bp_kernels.h: per-check LDS state updated by
//                        returning LDS atomics (kept for A/B measurements,
//                        selected with QLDPC_ENGINE=1).
// Variants (fp32/fp64 × variables per thread × max column degree × slots) are
// selected per graph at create time.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/qldpc_hip.h"
#include "variants.h"
#include "runtime.h"

using namespace qldpc;
using namespace qldpc_rt;

thread_local std::string qldpc_rt::g_err;

namespace {

const int kVplSet[] = {1, 2, 3, 4, 5, 6, 7, 8, 10, 12};
constexpr int kLdsMax = 160 * 1024;
constexpr int kChunkMax = 1024;

int env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return (e && *e) ? std::atoi(e) : dflt;
}

}  // namespace

// --------------------------------------------------------------- dispatch
namespace {

Variant get_variant(int precision, int vpl, int dmax) {
  if (precision == 32) return dmax == 4 ? get_variant_f32_d4(vpl) : get_variant_f32_d8(vpl);
  return dmax == 4 ? get_variant_f64_d4(vpl) : get_variant_f64_d8(vpl);
}

SVariant get_svariant(int precision, int dmax, int ns) {
  if (precision == 32) return dmax == 4 ? get_svariant_f32_d4(ns) : get_svariant_f32_d8(ns);
  return dmax == 4 ? get_svariant_f64_d4(ns) : get_svariant_f64_d8(ns);
}

SVariant get_rvariant(int precision, int vpl, int d3k, int dmax) {
  if (precision == 32 && dmax == 5) return get_rvariant_f32_d5(vpl, d3k);
  if (precision == 32 && dmax == 6) return get_rvariant_f32_d6(vpl, d3k);
  return precision == 32 ? get_rvariant_f32(vpl, d3k) : get_rvariant_f64(vpl);
}

// fp64 engine-3 kernels built for <= 256-thread workgroups (engine id 103:
// 256-VGPR budget, own v2c in VGPRs, compile-time D3K); QLDPC_F64W=0 disables.
bool use_f64w(const Route& r) {
  // column degree 5 (kern_r_f64_d5.hip): VPL 4-5 only
  // (column degree 5 also with rows of 9-10 = 5 chunks: the lifted-product [h | I] graphs, round 6)
  return r.engine == 3 && r.precision == 64 &&
         (r.DMAX == 4 || (r.DMAX == 5 && (r.VPL <= 5 || (r.VPL == 6 && r.nch == 5)))) && r.ea_shift == 0 && r.TB <= 256 &&
         r.VPL >= 4 && r.VPL <= 8 && (r.nch == 3 || r.nch == 4 || (r.DMAX == 5 && r.nch == 5)) &&
         env_int("QLDPC_F64W", 1) != 0;
}

// fp32 engine-3 kernels with the compile-time 2-chunk check phase (rows of <= 8 edges);
// QLDPC_F32W=0 falls back to the runtime-width check loop.
bool use_f32w(const Route& r) {
  return r.engine == 3 && r.precision == 32 && r.DMAX == 4 && r.ea_shift == 0 && r.VPL >= 5 && r.VPL <= 8 && r.nch == 2 &&
         env_int("QLDPC_F32W", 1) != 0;
}

#if QLDPC_STAMPS
// diagnostic build: phase-cycle sums of the fused MC kernels (bp_reg.h, QLDPC_STAMPS)
unsigned long long* debug_stamps_buffer() {
  static unsigned long long* buf = nullptr;
  if (!buf && hipMalloc(&buf, 10 * sizeof(unsigned long long)) == hipSuccess) (void)hipMemset(buf, 0, 80);
  return buf;
}
#endif

// Slot-family kernels of an engine (2 or 3).
SVariant slot_variant(const Route& r) {
  const SVariant none{nullptr, nullptr, nullptr, nullptr};
  const bool e3 = r.engine == 3, f64 = r.precision == 64;
  // fp32 space-time family with byte F words (rows of 2 chunks + a tail slot, 512 threads, 2 per CU)
  if (r.fb) {
    const bool ok = e3 && !f64 && r.DMAX == 4 && r.ea_shift == 2 && r.nch == 2 && r.tail && r.TB == 512;
    return ok ? get_rvariant_f32_stfb(r.VPL, r.d3k, r.d2k) : none;
  }
  // fp64 m2-in-slot family (rows of 3 chunks + a tail slot, <= 256 threads, 3 workgroups per CU)
  if (r.m2s) {
    // the fp64 space-time graphs: rows of 4 chunks + a tail slot, dword-scaled addresses, 1024
    // threads (engine id 111313, round 6)
    if (e3 && f64 && r.DMAX == 4 && r.ea_shift == 2 && r.nch == 4 && r.tail && r.TB >= 512)
      return get_rvariant_f64_m2st(r.VPL, r.d3k, r.d2k);
    // rows of 8 (4 chunks, no tail array), column degree 5, 256 threads (128 / 192 for small graphs): engine id 10103
    if (e3 && f64 && r.DMAX == 5 && r.ea_shift == 0 && r.nch == 4 && !r.tail && r.TB <= 256)
      return r.m2s_pk ? get_rvariant_f64_m2s8pk(r.VPL, r.d3k) : get_rvariant_f64_m2s8(r.VPL, r.d3k);
    const bool ok = e3 && f64 && r.DMAX == 4 && r.ea_shift == 0 && r.nch == 3 && r.tail && r.TB <= 256;
    return ok ? get_rvariant_f64_m2s(r.VPL, r.d3k) : none;
  }
  // fp64 tail layout (rows of 4 chunks + a tail slot, dword-scaled addresses, 1024 threads)
  if (r.tail) {
    const bool ok = e3 && r.DMAX == 4 && r.ea_shift == 2 && r.nch == (f64 ? 4 : 2) && (r.TB > 512 || (f64 && r.TB == 512));
    if (!ok) return none;
    return f64 ? get_rvariant_f64_st(r.VPL, r.d3k, r.d2k) : get_rvariant_f32_st(r.VPL, r.d3k);
  }
  if (use_f64w(r)) return r.DMAX == 5 ? get_rvariant_f64_w_d5(r.VPL, r.d3k, r.nch) : get_rvariant_f64_w(r.VPL, r.d3k, r.nch);
  if (use_f32w(r)) return get_rvariant_f32_w(r.VPL, r.d3k);
  if (e3 && r.ea_shift == 2) return (!f64 && r.DMAX == 4) ? get_rvariant_f32_big(r.VPL, r.d3k) : none;
  return e3 ? get_rvariant(r.precision, r.VPL, r.d3k, r.DMAX) : get_svariant(r.precision, r.DMAX, r.NS);
}

// The id the handles report for that kernel (qldpc_bp_kernel_id): the engine, or the engine-3 family
// in slot_variant's order.
int route_kernel_id(const Route& r) {
  if (r.engine != 3) return r.engine;
  if (r.m2s)
    return (r.tail && r.nch == 4) ? 11313 + 100000 * std::min(r.d2k, 1) : r.tail ? 11103 : r.m2s_pk ? 10203 : 10103;
  if (r.fb) return 21013 + ((r.d3k >= 8 && r.d2k > 0) ? 100000 * std::min(r.d2k, 4) : 0);  // + D2K digit
  if (r.tail) return 1013 + ((r.precision == 64 && r.VPL == 6 && r.d2k >= 1 && r.d3k >= 1) ? 100000 : 0);
  return use_f64w(r) ? 103 : r.ea_shift == 2 ? 13 : 3;
}

int round_up(int x, int a) { return (x + a - 1) / a * a; }

// ---- engine 1 geometry: threads per shot TB (multiple of 64, <= 512)
// Largest vars-per-thread whose kernels compile without register spills (gfx950,
// -Rpass-analysis=kernel-resource-usage).
int max_spill_free_vpl(int precision, int dmax) {
  if (precision == 32) return dmax == 4 ? 10 : 5;
  return dmax == 4 ? 6 : 3;
}

int choose_geometry(int n, int m, int requested_vpl, int vmax, int& TB, int& VPL) {
  if (requested_vpl > 0) {
    bool ok = false;
    for (int v : kVplSet) ok |= (v == requested_vpl);
    if (!ok) return set_err(QLDPC_EINVAL, "vars_per_thread must be one of 1-8,10,12");
    VPL = requested_vpl;
    TB = round_up((n + VPL - 1) / VPL, 64);
    if (TB > kMaxThreads) return set_err(QLDPC_EINVAL, "vars_per_thread too small for this graph (>512 threads)");
  } else {
    double best = 1e30;
    for (int v : kVplSet) {
      const int tb = round_up((n + v - 1) / v, 64);
      if (tb > kMaxThreads || v > vmax) continue;
      const double waste = (double)(tb * v - n) / (double)(tb * v);
      const double score = waste + (v < 4 ? 0.25 : 0.0) + 0.01 * v;
      if (score < best) {
        best = score;
        TB = tb;
        VPL = v;
      }
    }
    if (best >= 1e30) return set_err(QLDPC_ENOTSUP, "graph too large for the register-resident kernel");
  }
  if ((m + TB - 1) / TB > 32) return set_err(QLDPC_ENOTSUP, "too many checks per thread (m > 32*threads)");
  return 0;
}

size_t lds_for(int precision, int mmax) {
  const size_t pair = precision == 32 ? 8 : 16;
  return pair * 2 * (size_t)mmax + 4 * 2 * (size_t)mmax + 64;
}

// ---- engine 2 geometry: threads per shot TB (multiple of 64, 64..1024) and a
// runtime count of variables per thread VPL = ceil(n / TB) <= 32.  Default TB
// 256; QLDPC_TB or vars_per_thread override it.
int choose_sgeometry(int n, int m, int requested_vpl, int& TB, int& VPL) {
  const int forced_tb = env_int("QLDPC_TB", 0);
  if (requested_vpl > 0) {
    VPL = requested_vpl;
    TB = round_up((n + VPL - 1) / VPL, 64);
  } else if (forced_tb > 0) {
    TB = round_up(forced_tb, 64);
    VPL = (n + TB - 1) / TB;
  } else {
    // 256 threads (4 waves) per shot measured best on n225..n1600 (DESIGN.md
    // §Kernels): four workgroups per CU, short check-phase tails.
    TB = std::min(256, round_up(n, 64));
    VPL = (n + TB - 1) / TB;
    if (VPL > kMaxVplS) {
      TB = std::min(kMaxThreadsS, round_up((n + kMaxVplS - 1) / kMaxVplS, 64));
      VPL = (n + TB - 1) / TB;
    }
  }
  if (TB > kMaxThreadsS || TB < 64) return set_err(QLDPC_EINVAL, "threads per shot out of range (64..1024)");
  if (VPL > kMaxVplS) return set_err(QLDPC_ENOTSUP, "more than 32 variables per thread (n > 32768)");
  if ((m + TB - 1) / TB > 32) return set_err(QLDPC_ENOTSUP, "too many checks per thread (m > 32*threads)");
  return 0;
}

// ---- engine 3 geometry: compile-time VPL <= 8.  Default: the smallest
// power-of-two TB (64..1024) with VPL = ceil(n / TB) <= 7 -- measured best or
// within 4 % of the best on n126..n1600 (profiles/r01/geometry_sweep_e3.txt:
// n1600 256x7, n625 128x5, n225 64x4, GBC A4 256x4, GBC A1 64x2; fewer,
// longer threads win through the software-pipelined variable loop and shorter
// check-phase tails).  QLDPC_TB or vars_per_thread override it.  Returns
// nonzero if engine 3 cannot take the graph (the caller falls back to engine 2).
constexpr int kMaxVplR = 8;
constexpr int kPrefVplR = 7;
int choose_rgeometry(int n, int m, int requested_vpl, int& TB, int& VPL, int pref = kPrefVplR, int vmax = kMaxVplR) {
  const int forced_tb = env_int("QLDPC_TB", 0);
  if (requested_vpl > 0) {
    VPL = requested_vpl;
    TB = round_up((n + VPL - 1) / VPL, 64);
  } else if (forced_tb > 0) {
    TB = round_up(forced_tb, 64);
    VPL = (n + TB - 1) / TB;
  } else {
    TB = 64;
    while (TB < kMaxThreadsS && ((n + TB - 1) / TB > pref || (m + TB - 1) / TB > 32)) TB *= 2;
    VPL = (n + TB - 1) / TB;
  }
  if (TB > kMaxThreadsS || TB < 64 || VPL < 1 || VPL > vmax || (m + TB - 1) / TB > 32) return 1;
  return 0;
}

// The engine-3 LDS image of a route over `vslots` V slots and `mmax` checks (the graph's own, or
// the larger of two sectors'), and a workgroup's LDS bytes with it.
RLayout route_layout(const Route& r, int vslots, int mmax) {
  return r_layout(r.engine, vslots, mmax, r.precision == 32 ? 4 : 8, r.tail, r.m2s, r.fb);
}
size_t route_lds(const Route& r, int vslots, int mmax) {
  return r_lds_bytes((int)route_layout(r, vslots, mmax).total, kChunkMax);
}

// Engine 3 addresses its image with 16-bit byte offsets; with dword-scaled offsets
// (kernel id 13, ea_shift 2) it reaches 256 KiB.
bool route_fits(const Route& r, int vslots, int mmax) {
  return route_layout(r, vslots, mmax).lred <= (65536u << r.ea_shift) && route_lds(r, vslots, mmax) <= (size_t)kLdsMax;
}

// Slots per workgroup: QLDPC_NS, else 1 (independent workgroups interleave
// better than lock-stepped slots).
int choose_ns(int img) {
  const int forced = env_int("QLDPC_NS", 1);
  const int ns = (forced == 2 || forced == 4) ? forced : 1;
  return slot_lds_bytes(ns, img, kChunkMax) <= (size_t)kLdsMax ? ns : 1;
}

int device_cus(int dev, int& cus) {
  hipDeviceProp_t prop;
  QLDPC_HIP(hipGetDeviceProperties(&prop, dev));
  cus = prop.multiProcessorCount;
  return 0;
}

}  // namespace

// ================================================================== C ABI
extern "C" {

#if QLDPC_STAMPS
// diagnostic builds only (not in include/qldpc_hip.h): read and clear the phase-cycle sums
int qldpc_debug_stamps(unsigned long long* out) {
  unsigned long long* b = debug_stamps_buffer();
  if (!b || hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, b, 80, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return hipMemset(b, 0, 80) == hipSuccess ? 0 : -1;
}
#endif

int qldpc_abi_version(void) { return QLDPC_ABI_VERSION; }

const char* qldpc_last_error(void) { return qldpc_rt::g_err.c_str(); }

int qldpc_build_flags(void) { return 0; }

int qldpc_device_count(int* out) {
  if (!out) return set_err(QLDPC_EINVAL, "out is NULL");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *out = 0;
    return set_err(QLDPC_EHIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *out = c;
  return 0;
}

int qldpc_graph_create(int device, int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                       qldpc_graph** out) {
  if (!out || !row_ptr || (m > 0 && !col_idx)) return set_err(QLDPC_EINVAL, "NULL argument");
  if (m < 0 || n <= 0) return set_err(QLDPC_EINVAL, "bad shape");
  if (m >= 0xFFFF) return set_err(QLDPC_ENOTSUP, "more than 65534 checks");
  if (row_ptr[0] != 0) return set_err(QLDPC_EINVAL, "row_ptr[0] != 0");
  auto* g = new qldpc_graph();
  g->device = device;
  g->m = m;
  g->n = n;
  g->nnz = row_ptr[m];
  g->row_ptr.assign(row_ptr, row_ptr + m + 1);
  g->col_idx.assign(col_idx, col_idx + g->nnz);
  g->col_rows.assign(n, {});
  for (int i = 0; i < m; ++i) {
    if (row_ptr[i + 1] < row_ptr[i]) {
      delete g;
      return set_err(QLDPC_EINVAL, "row_ptr not monotone");
    }
    g->max_row = std::max(g->max_row, row_ptr[i + 1] - row_ptr[i]);
    for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
      const int c = col_idx[e];
      if (c < 0 || c >= n || (e > row_ptr[i] && col_idx[e - 1] >= c)) {
        delete g;
        return set_err(QLDPC_EINVAL, "col_idx out of range or not strictly ascending within a row");
      }
      g->col_rows[c].push_back(i);
    }
  }
  for (int j = 0; j < n; ++j) g->max_col = std::max<int>(g->max_col, (int)g->col_rows[j].size());
  *out = g;
  return 0;
}

int qldpc_graph_destroy(qldpc_graph* g) {
  delete g;
  return 0;
}

int qldpc_graph_info(const qldpc_graph* g, int32_t* m, int32_t* n, int32_t* nnz, int32_t* max_row_deg,
                     int32_t* max_col_deg) {
  if (!g) return set_err(QLDPC_EINVAL, "NULL graph");
  if (m) *m = g->m;
  if (n) *n = g->n;
  if (nnz) *nnz = g->nnz;
  if (max_row_deg) *max_row_deg = g->max_row;
  if (max_col_deg) *max_col_deg = g->max_col;
  return 0;
}

static int upload_llr(qldpc_bp* bp) {
  const int TB = bp->route.TB, VPL = bp->route.VPL, n = bp->g->n;
  if (bp->route.engine == 7) return relay_upload_priors(bp);  // L0 and the integer solution weights
  if (bp->route.engine == 8) return serial_upload_priors(bp);
  if (bp->route.engine == 6) {  // HBM engine: log((1-p)/p) per variable, variable order
    std::vector<double> l64(n);
    for (int j = 0; j < n; ++j) l64[j] = std::log((1.0 - bp->probs[j]) / bp->probs[j]);  // glibc log, as Cython
    if (bp->route.precision == 32) {
      std::vector<float> l32(l64.begin(), l64.end());
      QLDPC_HIP(hipMemcpy(bp->llr.p, l32.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    } else {
      QLDPC_HIP(hipMemcpy(bp->llr.p, l64.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    }
    return 0;
  }
  if (bp->route.engine == 5) {  // product-sum priors: ratio p / (1 - p), computed in double (oracle ws_priors)
    std::vector<double> r64(n);
    for (int j = 0; j < n; ++j) r64[j] = bp->probs[j] / (1.0 - bp->probs[j]);
    if (bp->route.precision == 32) {
      std::vector<float> r32(r64.begin(), r64.end());
      QLDPC_HIP(hipMemcpy(bp->llr.p, r32.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    } else {
      QLDPC_HIP(hipMemcpy(bp->llr.p, r64.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    }
    return 0;
  }
  const size_t cnt = (size_t)VPL * TB;
  std::vector<double> l64(cnt, 1.0);
  for (int k = 0; k < VPL; ++k)
    for (int t = 0; t < TB; ++t) {
      const int j = bp->slot_var.empty() ? (k * TB + t < n ? k * TB + t : -1) : bp->slot_var[(size_t)k * TB + t];
      if (j >= 0) l64[(size_t)k * TB + t] = std::log((1.0 - bp->probs[j]) / bp->probs[j]);  // glibc log, as Cython
    }
  if (bp->route.precision == 32) {
    std::vector<float> l32(cnt);
    for (size_t i = 0; i < cnt; ++i) l32[i] = (float)l64[i];
    QLDPC_HIP(hipMemcpy(bp->llr.p, l32.data(), cnt * sizeof(float), hipMemcpyHostToDevice));
  } else {
    QLDPC_HIP(hipMemcpy(bp->llr.p, l64.data(), cnt * sizeof(double), hipMemcpyHostToDevice));
  }
  return 0;
}

// Variables in column order, stably sorted by degree class: a variable's class is the number of
// `bounds` its degree exceeds ({}: the identity, {3}: degree <= 3 first, {2, 3}: <= 2, then 3, then more).
static std::vector<int32_t> degree_sorted(const qldpc_graph* g, std::initializer_list<int> bounds) {
  std::vector<int32_t> order;
  order.reserve(g->n);
  for (size_t c = 0; c <= bounds.size(); ++c)
    for (int j = 0; j < g->n; ++j) {
      size_t cj = 0;
      for (int b : bounds) cj += (int)g->col_rows[j].size() > b;
      if (cj == c) order.push_back(j);
    }
  return order;
}

// Leading whole variable slots whose variables (padding aside) all have degree <= d: a kernel's
// compile-time D3K (d = 3) / D2K (d = 2).
static int leading_slots(const qldpc_graph* g, const std::vector<int32_t>& slot_var, int TB, int VPL, int d) {
  for (int k = 0; k < VPL; ++k)
    for (int t = 0; t < TB; ++t) {
      const int j = slot_var[(size_t)k * TB + t];
      if (j >= 0 && (int)g->col_rows[j].size() > d) return k;
    }
  return VPL;
}

// Engine-2/3 edge table: for slot (k, t) holding variable j = slot_var[k*TB+t]
// and its d-th check i (rows ascending), the word ((i + 1) | slot<<16) where
// slot is the position of edge (i, j) in row i of the row-major V image (after
// the 16-byte sink), with the 16-byte chunks of row i XOR-swizzled so that
// consecutive rows read by consecutive lanes hit distinct LDS banks.  Missing
// edges are the word 0 (dummies, bp_slot.h).
//
// Where an edge sits inside its row is free (the check phase takes an
// order-independent min / second min / parity), so with `vbase_dw` >= 0 (engine
// 3, fp32: dword offset of V in the image) the positions are chosen greedily,
// per v2c store instruction of the variable phase (slot (k, t), 32-lane half
// wave), to spread its 32 stores over the 32 banks: at most 2 per bank, which
// ds_write_b32 absorbs for free (MI355X_MICROARCH.md §LDS).  vbase_dw < 0
// keeps the ascending-column order.
//
// `lab` (engine 3, may be empty = identity) relabels the checks: check i keeps
// its CS entry at lab[i] + 1 and its row at position lab[i] of V (see
// label_checks below).  The F words and the check phase follow the labels; the
// decode path maps syndromes through the inverse permutation (bp->rperm).
// Slot plan of the fp64 space-time m2s family (engine id 111313, kern_r_f64_m2st.hip): the slot map
// (variable of every physical position k * tb + t, -1 = padding), its D2K / D3K, the private dummy
// count, the narrow-wave masks and the waves live in the last variable slot.  Round 6: the degree
// classes 1 / 2 / 3 / 4 in column order fill the LOGICAL positions slot-major; per variable slot k <
// kNwSlots of compile-time width w_k (2 below D2K, 3 below D3K, else DM) the leading logical waves whose
// variables all have degree <= w_k - 1 compute that slot one edge slot narrower (a wave-uniform branch,
// SSector::nw bit 16 k + physical wave): config 5 executes 15,360 edge slots per iteration for 15,288
// edges instead of 16,640, with 68 private dummies instead of 1,348.  Then (balance) the logical waves
// are placed on physical waves so that the four SIMDs (wave w on SIMD w mod 4) carry equal edge slots
// per iteration: config 5's logical waves execute 13-17 edge slots per thread (the five holding the
// sixth variable slot 17), 62 / 59 / 59 / 60 per SIMD in wave order, 60 on every SIMD placed (longest
// first onto the least loaded SIMD).  !narrow: the classes <= 2 / 3 / 4, no narrow waves.
struct StPlan {
  std::vector<int32_t> slots;
  int d2 = 0, d3 = 0, nd = 0;
  uint32_t nw = 0, live_last = 0;
};
static StPlan st_plan(const qldpc_graph* g, int tb, int vpl, int DM, bool narrow, bool balance) {
  StPlan P;
  const std::vector<int32_t> order = narrow ? degree_sorted(g, {1, 2, 3}) : degree_sorted(g, {2, 3});
  std::vector<int32_t> logical((size_t)vpl * tb, -1);  // variable of every logical position
  std::vector<int> deg((size_t)vpl * tb, -1);
  for (int p = 0; p < g->n && p < vpl * tb; ++p) {
    logical[p] = order[p];
    deg[p] = (int)g->col_rows[order[p]].size();
  }
  P.d2 = leading_slots(g, logical, tb, vpl, 2);
  P.d3 = leading_slots(g, logical, tb, vpl, 3);
  const int nwv = (tb + 63) / 64;
  std::vector<int> W(vpl, 0), units(nwv, 0);
  for (int k = 0; k < vpl; ++k) {
    const int w = k < P.d2 ? 2 : k < P.d3 ? 3 : DM;
    if (narrow && k < kNwSlots && nwv <= 16)
      for (; W[k] < nwv; ++W[k]) {
        bool ok = true;
        for (int t = W[k] * 64; t < W[k] * 64 + 64 && t < tb && ok; ++t) ok = deg[(size_t)k * tb + t] <= w - 1;
        if (!ok) break;
      }
    for (int v = 0; v < nwv; ++v) {
      bool live = k < vpl - 1;
      for (int t = v * 64; t < v * 64 + 64 && t < tb && !live; ++t) live = deg[(size_t)k * tb + t] >= 0;
      if (live) units[v] += w - (v < W[k] ? 1 : 0);
    }
    for (int t = 0; t < tb; ++t) {
      const int d = deg[(size_t)k * tb + t];
      if (d >= 0) P.nd += w - ((t >> 6) < W[k] ? 1 : 0) - d;
    }
  }
  // logical wave -> physical wave (identity, or balanced over the 4 SIMDs: longest first, least loaded)
  std::vector<int> phys(nwv);
  for (int v = 0; v < nwv; ++v) phys[v] = v;
  if (balance && nwv % 4 == 0 && nwv <= 16) {
    std::vector<int> byu(nwv);
    for (int v = 0; v < nwv; ++v) byu[v] = v;
    std::stable_sort(byu.begin(), byu.end(), [&](int a, int b) { return units[a] > units[b]; });
    int load[4] = {0, 0, 0, 0}, cnt[4] = {0, 0, 0, 0};
    for (int v : byu) {
      int best = -1;
      for (int q = 0; q < 4; ++q)
        if (cnt[q] < nwv / 4 && (best < 0 || load[q] < load[best])) best = q;
      phys[v] = best + 4 * cnt[best]++;
      load[best] += units[v];
    }
  }
  P.slots.assign((size_t)vpl * tb, -1);
  for (int p = 0; p < g->n && p < vpl * tb; ++p) {
    const int k = p / tb, t = p % tb;
    P.slots[(size_t)k * tb + phys[t >> 6] * 64 + (t & 63)] = order[p];
  }
  for (int v = 0; v < nwv && v < 32; ++v) {
    bool live = false;
    for (int t = v * 64; t < v * 64 + 64 && t < tb && !live; ++t) live = deg[(size_t)(vpl - 1) * tb + t] >= 0;
    if (live) P.live_last |= 1u << phys[v];
    for (int k = 0; k < kNwSlots && k < vpl; ++k)
      if (v < W[k]) P.nw |= 1u << (16 * k + phys[v]);
  }
  return P;
}

// `m2s`: place for the families whose variable phase also reads each edge's V slot (r.m2s).
static void build_slot_edges(const qldpc_graph* g, const Route& r, const std::vector<int32_t>& slot_var,
                             std::vector<uint32_t>& out, int vbase_dw, const std::vector<int>& lab, int m2s, int dummy0,
                             int* ndummy, int anneal, int anneal_iters = -1, int tail_base = -1) {
  const int TB = r.TB, VPL = r.VPL, DM = r.DMAX, tsize = r.precision == 32 ? 4 : 8, nch = r.nch, tail = r.tail;
  const int d3k = r.d3k, d2k = r.d2k;
  const uint32_t nw = r.nw;
  const int nv = 16 / tsize;  // messages per 16-byte chunk
  const int rw = nch * nv;
  const int rwt = rw + (tail ? 1 : 0);  // tail layouts: logical slot rw = the row's tail slot
  // first tail slot: right after V (bp_reg.h r_layout), i.e. after the private dummy slots when the
  // layout has them (tail_base, the space-time m2s family)
  const int tail0 = tail_base >= 0 ? tail_base : (1 + g->m * nch) * nv;
  const int swz_mask = (nch == 2) ? 1 : (nch == 4) ? 3 : 0;
  const int swz_shift = (nch == 2) ? 3 : 2;
  auto L = [&](int i) { return lab.empty() ? i : lab[i]; };
  auto phys = [&](int i, int ls) {
    const int r = L(i);
    if (ls == rw) return tail0 + r;
    return nv + r * rw + ((ls / nv) ^ ((r >> swz_shift) & swz_mask)) * nv + ls % nv;
  };
  // logical slot of every edge (CSR order); default = ascending column position
  std::vector<int> lslot(g->nnz);
  for (int i = 0; i < g->m; ++i)
    for (int e = g->row_ptr[i]; e < g->row_ptr[i + 1]; ++e) lslot[e] = e - g->row_ptr[i];
  auto edge_of = [&](int i, int j) {
    const int32_t* b = g->col_idx.data() + g->row_ptr[i];
    const int32_t* e = g->col_idx.data() + g->row_ptr[i + 1];
    return (int)(std::lower_bound(b, e, (int32_t)j) - g->col_idx.data());
  };
  // v2c store instructions: ds_write_b32 (float) = 2 groups of 32 lanes over 32
  // banks; ds_write_b64 (double) = 4 groups of 16 contiguous lanes, an 8-byte
  // slot s on bank pair s mod 16 (MI355X_MICROARCH.md §LDS)
  const int sg = tsize == 4 ? 32 : 16, nb = tsize == 4 ? 32 : 16;
  const int vbase_u = vbase_dw < 0 ? 0 : (tsize == 4 ? vbase_dw : vbase_dw / 2);
  if (vbase_dw >= 0 && rwt <= 32 && m2s) {
    // m2s (fp64): the variable phase also READS each edge's V slot (ds_read_b64: 2 groups of 32
    // lanes, 8-byte slot s on bank pair s mod 32), besides storing it (ds_write_b64: 4 groups of 16
    // contiguous lanes, bank pair s mod 16).  Place per 32-lane group: distinct s mod 32 over the
    // group first, distinct s mod 16 within each 16-lane half second.
    std::vector<uint32_t> used(g->m, 0u);
    const bool greedy = env_int("QLDPC_M2S_GREEDY", 1) != 0;
    for (int k = 0; k < VPL && greedy; ++k)
      for (int d = 0; d < DM; ++d)
        for (int h0 = 0; h0 < TB; h0 += 32) {
          int c32[32] = {0}, c16[2][16] = {{0}};
          for (int t = h0; t < h0 + 32 && t < TB; ++t) {
            const int j = slot_var[(size_t)k * TB + t];
            if (j < 0 || d >= (int)g->col_rows[j].size()) continue;
            const int i = g->col_rows[j][d];
            const int hf = (t - h0) >> 4;
            int best = -1, bc = 1 << 30;
            for (int ls = 0; ls < rwt; ++ls) {
              if ((used[i] >> ls) & 1u) continue;
              const int sl = vbase_u + phys(i, ls);
              const int c = 4 * c32[sl % 32] + c16[hf][sl % 16];
              if (c < bc) {
                bc = c;
                best = ls;
              }
            }
            used[i] |= 1u << best;
            const int sl = vbase_u + phys(i, best);
            c32[sl % 32]++;
            c16[hf][sl % 16]++;
            lslot[edge_of(i, j)] = best;
          }
        }
  } else if (vbase_dw >= 0 && rwt <= 32) {
    std::vector<uint32_t> used(g->m, 0u);
    for (int k = 0; k < VPL; ++k)
      for (int d = 0; d < DM; ++d)
        for (int h0 = 0; h0 < TB; h0 += sg) {
          int cnt[32] = {0};
          for (int t = h0; t < h0 + sg && t < TB; ++t) {
            const int j = slot_var[(size_t)k * TB + t];
            if (j < 0 || d >= (int)g->col_rows[j].size()) continue;
            const int i = g->col_rows[j][d];
            int best = -1, bc = 1 << 30;
            for (int ls = 0; ls < rwt; ++ls) {
              if ((used[i] >> ls) & 1u) continue;
              const int c = cnt[(vbase_u + phys(i, ls)) % nb];
              if (c < bc) {
                bc = c;
                best = ls;
              }
            }
            used[i] |= 1u << best;
            cnt[(vbase_u + phys(i, best)) % nb]++;
            lslot[edge_of(i, j)] = best;
          }
        }
  }
  // Annealed placement (round 4, fp64 engine-3 families; `anneal` 1: the variable phase reads and
  // stores each edge's V slot (m2s, the 1024-thread tail family), 2: stores only (own v2c in VGPRs)).
  if (anneal && vbase_dw >= 0 && rwt <= 32) {
    // Then a seeded annealed local search over the rows' slot permutations (swap the positions of
    // two edges of one row, or move one into a free position) on the EXACT cost of the lane-group
    // bank model (qldpc_bp_lds_model): per 32-lane read group the maximum number of addresses on one
    // bank pair (slot mod 32), per 16-lane store group the same over slot mod 16; objective = reads
    // + ws * stores, temperature T0 falling linearly to 0 (round 4; tools/dev/place_opt3.cpp is the
    // offline study: 20 M moves take the n1600 hz model from 362 / 715 to 327 / 442 cycles).
    // default 4000 moves per edge, capped at 2^25 moves (~6 s on one host core; n1600: 21.5 M moves,
    // ~3.9 s; measured +3.1 %: 1.221 M vs 1.184 M shots/s, bank-conflict share 0.338 -> 0.276,
    // profiles/r04/passd/); QLDPC_M2S_ANNEAL=<moves> or DeviceBP(anneal_iters=...) overrides it (0 =
    // the greedy placement only, for short runs).  The result is memoised per process for the same
    // graph, lane map and layout (decoders for other error rates of one code reuse it); the memo keeps
    // at most kAnnealMemo placements (a sweep over many codes does not grow it without bound)
    const int iters_env = anneal_iters >= 0 ? anneal_iters : env_int("QLDPC_M2S_ANNEAL", -1);
    const int iters = iters_env >= 0 ? iters_env : (int)std::min<long long>(4000LL * g->nnz, 1LL << 25);
    constexpr size_t kAnnealMemo = 16;
    static std::mutex memo_mu;
    static std::map<uint64_t, std::vector<int>> memo;
    uint64_t key = 0xcbf29ce484222325ull;
    auto mix = [&](uint64_t v) { key = (key ^ v) * 0x100000001b3ull; };
    bool hit = false;
    if (iters > 0) {
      for (int v : {g->m, g->n, TB, VPL, DM, nch, tail, vbase_u, iters, anneal, env_int("QLDPC_M2S_ANNEAL_T", 50),
                    env_int("QLDPC_M2S_ANNEAL_WS", 1000)})
        mix((uint64_t)(uint32_t)v);
      for (int32_t v : slot_var) mix((uint64_t)(uint32_t)v);
      for (int32_t v : g->col_idx) mix((uint64_t)(uint32_t)v);
      for (int v : lslot) mix((uint64_t)(uint32_t)v);  // the greedy start
      std::lock_guard<std::mutex> lk(memo_mu);
      auto it = memo.find(key);
      if (it != memo.end() && it->second.size() == lslot.size()) {
        lslot = it->second;
        hit = true;
      }
    }
    if (iters > 0 && !hit) {
      const double T0 = env_int("QLDPC_M2S_ANNEAL_T", 50) * 1e-3, ws = env_int("QLDPC_M2S_ANNEAL_WS", 1000) * 1e-3;
      const double wr = anneal == 1 ? 1.0 : 0.0;  // 2: the family keeps its own v2c in VGPRs (no V reads)
      const int nrg = VPL * DM * ((TB + 31) / 32), nwg = VPL * DM * ((TB + 15) / 16);
      std::vector<int> erg(g->nnz, -1), ewg(g->nnz, -1);
      for (int k = 0; k < VPL; ++k)
        for (int t = 0; t < TB; ++t) {
          const int j = slot_var[(size_t)k * TB + t];
          if (j < 0) continue;
          const auto& rows = g->col_rows[j];
          for (int d = 0; d < (int)rows.size() && d < DM; ++d) {
            const int e = edge_of(rows[d], j);
            erg[e] = (k * DM + d) * ((TB + 31) / 32) + t / 32;
            ewg[e] = (k * DM + d) * ((TB + 15) / 16) + t / 16;
          }
        }
      // per group: addresses per bank and a histogram of those counts (max in O(1) amortised)
      struct BankG {
        uint8_t cnt[32] = {0};
        int hist[64] = {0};
        int mx = 0;
        void add(int b) { hist[cnt[b]]--; hist[++cnt[b]]++; mx = std::max(mx, (int)cnt[b]); }
        void sub(int b) { hist[cnt[b]]--; hist[--cnt[b]]++; while (mx > 0 && hist[mx] == 0) --mx; }
        int cost() const { return mx > 1 ? mx : 1; }
      };
      std::vector<BankG> RG(nrg), WG(nwg);
      std::vector<int> at((size_t)g->m * rwt, -1);  // position -> edge per row (-1 = free)
      auto put = [&](int e, int i, int sg) {
        const int sl = vbase_u + phys(i, lslot[e]);
        if (sg > 0) { RG[erg[e]].add(sl % 32); WG[ewg[e]].add(sl % 16); }
        else { RG[erg[e]].sub(sl % 32); WG[ewg[e]].sub(sl % 16); }
      };
      for (int i = 0; i < g->m; ++i)
        for (int e = g->row_ptr[i]; e < g->row_ptr[i + 1]; ++e) {
          at[(size_t)i * rwt + lslot[e]] = e;
          if (erg[e] >= 0) put(e, i, +1);
        }
      uint64_t rs = 0x2545F4914F6CDD1Dull;
      auto rnd = [&]() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; };
      auto cost2 = [&](int ea, int eb) {  // cost of the (deduplicated) groups of two edges
        double c = 0;
        int r0 = -1, w0 = -1;
        for (int e : {ea, eb}) {
          if (e < 0) continue;
          if (erg[e] != r0) c += wr * RG[erg[e]].cost();
          if (ewg[e] != w0) c += ws * WG[ewg[e]].cost();
          r0 = erg[e];
          w0 = ewg[e];
        }
        return c;
      };
      for (int it = 0; it < iters; ++it) {
        const int i = (int)(rnd() % (uint64_t)g->m);
        const int a = (int)(rnd() % (uint64_t)rwt), b = (int)(rnd() % (uint64_t)rwt);
        if (a == b) continue;
        const int ea = at[(size_t)i * rwt + a], eb = at[(size_t)i * rwt + b];
        if ((ea < 0 || erg[ea] < 0) && (eb < 0 || erg[eb] < 0)) continue;
        if ((ea >= 0 && erg[ea] < 0) || (eb >= 0 && erg[eb] < 0)) continue;
        const double before = cost2(ea, eb);
        auto swap_ab = [&]() {
          if (ea >= 0) put(ea, i, -1);
          if (eb >= 0) put(eb, i, -1);
          if (ea >= 0) lslot[ea] = lslot[ea] == a ? b : a;
          if (eb >= 0) lslot[eb] = lslot[eb] == a ? b : a;
          if (ea >= 0) put(ea, i, +1);
          if (eb >= 0) put(eb, i, +1);
        };
        swap_ab();
        const double dlt = cost2(ea, eb) - before;
        const double T = T0 * (1.0 - (double)it / iters);
        const bool take = dlt <= 0 || (T > 0 && (double)(rnd() % 1000000) / 1e6 < std::exp(-dlt / T));
        if (take) {
          at[(size_t)i * rwt + a] = eb;
          at[(size_t)i * rwt + b] = ea;
        } else {
          swap_ab();
        }
      }
      std::lock_guard<std::mutex> lk(memo_mu);
      if (memo.size() >= kAnnealMemo) memo.clear();
      memo[key] = lslot;
    }
  }
  out.assign((size_t)VPL * DM * TB, kNoEdgeS);
  for (int k = 0; k < VPL; ++k)
    for (int t = 0; t < TB; ++t) {
      const int j = slot_var[(size_t)k * TB + t];
      if (j < 0) continue;
      const auto& rows = g->col_rows[j];
      for (int d = 0; d < (int)rows.size(); ++d) {
        const int i = rows[d];
        const int slot = phys(i, lslot[edge_of(i, j)]);
        out[((size_t)k * DM + d) * TB + t] = (uint32_t)(L(i) + 1) | ((uint32_t)slot << 16);
      }
    }
  // m2s rows of 8 / space-time rows: the missing edges of real variables (slots k >= d3k hold DM
  // edge slots, d2k <= k < d3k three, k < d2k two; one fewer in the narrow waves of `nw`) get private
  // V slots from dummy0 on, lane-consecutive per (k, d) (conflict-free reads and stores), and the
  // dummy CS entry 0
  int nd = 0;
  if (dummy0 >= 0)
    for (int k = 0; k < VPL; ++k)
      for (int d = 0; d < DM; ++d)
        for (int t = 0; t < TB; ++t) {
          const int j = slot_var[(size_t)k * TB + t];
          const int w = (k < d2k ? 2 : k < d3k ? 3 : DM) - (k < kNwSlots && ((nw >> (16 * k + (t >> 6))) & 1u) ? 1 : 0);
          if (j >= 0 && d >= (int)g->col_rows[j].size() && d < w)
            out[((size_t)k * DM + d) * TB + t] = (uint32_t)(dummy0 + nd++) << 16;
        }
  if (ndummy) *ndummy = nd;
}

// Static LDS model of one engine-3 fp64 variable phase (per workgroup and iteration): LDS-array
// cycles and the extra (bank-conflict) cycles of the CS gathers, the V-slot reads (one-word m2s
// families) and the v2c stores, from the final edge table.  Lane groups and bank mapping of
// MI355X_MICROARCH.md §LDS: ds_read_b64 2 x 32 lanes, bank pair (a / 8) mod 32; ds_read_b128 the
// 4 lane sets of 16 (kB128 below), bank quad (a / 16) mod 16; ds_write_b64 4 x 16 contiguous
// lanes, bank pair (a / 8) mod 16.  Identical addresses broadcast.  A group costs max over its
// banks of the distinct addresses there (1 = conflict-free).  Compared against SQ_LDS_BANK_CONFLICT
// / SQ_LDS_IDX_ACTIVE (tools/lds_model.py).
static void lds_model_var_phase(const std::vector<uint32_t>& edges, const Route& r, uint32_t vbase, int64_t* out) {
  const int TB = r.TB, VPL = r.VPL, DM = r.DMAX, d3k = r.d3k;
  const bool m2s = r.m2s != 0;
  static const int kB128[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                   {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                   {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                   {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
  for (int q = 0; q < 6; ++q) out[q] = 0;
  auto group_cost = [](const std::vector<std::pair<uint32_t, uint32_t>>& ab) {  // (bank, address)
    std::vector<std::pair<uint32_t, uint32_t>> v(ab);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    int mx = 0;
    for (size_t i = 0; i < v.size();) {
      size_t j = i;
      while (j < v.size() && v[j].first == v[i].first) ++j;
      mx = std::max(mx, (int)(j - i));
      i = j;
    }
    return std::max(mx, 1);
  };
  for (int k = 0; k < VPL; ++k)
    for (int d = 0; d < DM; ++d) {
      if (k < d3k && d >= 3) continue;  // compile-time degree-3 slots issue no 4th edge
      for (int w = 0; w * 64 < TB; ++w) {
        auto lane_word = [&](int l) {
          const int t = w * 64 + l;
          return t < TB ? edges[((size_t)k * DM + d) * TB + t] : 0u;
        };
        // CS gathers
        if (m2s) {
          for (int h = 0; h < 2; ++h) {
            std::vector<std::pair<uint32_t, uint32_t>> ab;
            for (int l = h * 32; l < h * 32 + 32; ++l) {
              const uint32_t a = (lane_word(l) & 0xFFFFu) * 8u;
              ab.emplace_back((a / 8u) % 32u, a);
            }
            const int c = group_cost(ab);
            out[0] += c;
            out[1] += c - 1;
          }
        } else {
          for (int h = 0; h < 4; ++h) {
            std::vector<std::pair<uint32_t, uint32_t>> ab;
            for (int q = 0; q < 16; ++q) {
              const uint32_t a = (lane_word(kB128[h][q]) & 0xFFFFu) * 16u;
              ab.emplace_back((a / 16u) % 16u, a);
            }
            const int c = group_cost(ab);
            out[0] += c;
            out[1] += c - 1;
          }
        }
        // V-slot reads (m2s) and v2c stores
        for (int h = 0; h < 2 && m2s; ++h) {
          std::vector<std::pair<uint32_t, uint32_t>> ab;
          for (int l = h * 32; l < h * 32 + 32; ++l) {
            const uint32_t a = vbase + (lane_word(l) >> 16) * 8u;
            ab.emplace_back((a / 8u) % 32u, a);
          }
          const int c = group_cost(ab);
          out[2] += c;
          out[3] += c - 1;
        }
        for (int h = 0; h < 4; ++h) {
          std::vector<std::pair<uint32_t, uint32_t>> ab;
          for (int l = h * 16; l < h * 16 + 16; ++l) {
            const uint32_t a = vbase + (lane_word(l) >> 16) * 8u;
            ab.emplace_back((a / 8u) % 16u, a);
          }
          const int c = group_cost(ab);
          out[4] += c;
          out[5] += c - 1;
        }
      }
    }
}

// Engine-3 check labelling against LDS bank conflicts.  The variable phase
// gathers CS[lab[i] + 1] for the d-th check of each lane's variable: one
// ds_read_b64 (float: 8-byte entries, 2 groups of 32 lanes, bank pair = entry
// mod 32) or ds_read_b128 (double: 16-byte entries, the 4 lane groups of 16 of
// MI355X_MICROARCH.md §LDS, bank quad = entry mod 16) per (slot k, edge d).
// Distinct checks of one lane group that share a colour (entry mod NC) cost an
// extra LDS cycle each (one check gathered by several lanes broadcasts).  The
// labels are a permutation; a seeded local search swaps the labels of two
// checks whenever that does not increase Σ_groups Σ_colours count² (= the group
// size exactly when every group is conflict free).  For double it also balances
// each 16-lane v2c store group over the two row-label parities (ds_write_b64:
// a row of 8 slots covers half of the 16 bank pairs), so build_slot_edges's
// in-row placement can make the stores conflict free too.  Pure host work, done
// once per decoder; the arithmetic is untouched (labels only move storage).
static std::vector<int> label_checks(const qldpc_graph* g, const Route& r, const std::vector<int32_t>& slot_var,
                                     int* cost_before, int* cost_after) {
  const int TB = r.TB, VPL = r.VPL, DM = r.DMAX, tsize = r.precision == 32 ? 4 : 8, m2s = r.m2s;
  const int m = g->m;
  std::vector<int> lab(m);
  for (int i = 0; i < m; ++i) lab[i] = i;
  if (m < 2) return lab;
  // CS entries of 8 bytes (fp32 pairs; fp64 m2s words): ds_read_b64 gathers, 2 groups of 32 lanes,
  // bank pair = entry mod 32.  16-byte fp64 pairs: ds_read_b128, bank quad = entry mod 16.
  const bool cs8 = tsize == 4 || m2s;
  const int NC = cs8 ? 32 : 16;
  static const int kB128[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                   {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                   {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                   {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
  // groups (gather groups first, then double's store groups), as check lists
  std::vector<int> gs{0}, gm;
  std::vector<char> gstore;
  auto add_group = [&](int k, int d, int w, const int* lanes, int nl, bool store) {
    const size_t start = gm.size();
    for (int q = 0; q < nl; ++q) {
      const int t = w * 64 + lanes[q];
      if (t >= TB) continue;
      const int j = slot_var[(size_t)k * TB + t];
      if (j < 0 || d >= (int)g->col_rows[j].size()) continue;
      const int i = g->col_rows[j][d];
      if (std::find(gm.begin() + start, gm.end(), i) == gm.end()) gm.push_back(i);
    }
    if (gm.size() - start >= 2) {
      gs.push_back((int)gm.size());
      gstore.push_back(store ? 1 : 0);
    } else {
      gm.resize(start);
    }
  };
  int lanes32[2][32], lanes16[4][16];
  for (int q = 0; q < 64; ++q) {
    lanes32[q / 32][q % 32] = q;
    lanes16[q / 16][q % 16] = q;
  }
  for (int k = 0; k < VPL; ++k)
    for (int d = 0; d < DM; ++d)
      for (int w = 0; w * 64 < TB; ++w) {
        if (cs8) {
          for (int h = 0; h < 2; ++h) add_group(k, d, w, lanes32[h], 32, false);
        } else {
          for (int h = 0; h < 4; ++h) add_group(k, d, w, kB128[h], 16, false);
        }
        if (tsize == 8)
          for (int h = 0; h < 4; ++h) add_group(k, d, w, lanes16[h], 16, true);
      }
  const int ng = (int)gstore.size();
  if (ng == 0) return lab;
  std::vector<std::vector<int>> of(m);  // groups of each check
  for (int q = 0; q < ng; ++q)
    for (int e = gs[q]; e < gs[q + 1]; ++e) of[gm[e]].push_back(q);
  // colour of a label in a group: gathers (label + 1) mod NC, stores the row parity
  auto col = [&](int q, int l) { return gstore[q] ? (l & 1) : (l + 1) % NC; };
  const int W = 32;
  // weights of the two kinds of groups in the objective (double: the stores
  // conflict far more than the gathers of structured codes)
  const int wg = env_int("QLDPC_LABEL_WG", tsize == 4 ? 1 : 1), ws = env_int("QLDPC_LABEL_WS", 4);
  std::vector<int> gw(ng);
  for (int q = 0; q < ng; ++q) gw[q] = gstore[q] ? ws : wg;
  std::vector<int> cnt((size_t)ng * W, 0);
  long long cost = 0;
  for (int q = 0; q < ng; ++q)
    for (int e = gs[q]; e < gs[q + 1]; ++e) {
      int& c = cnt[(size_t)q * W + col(q, lab[gm[e]])];
      cost += (long long)gw[q] * (2 * c + 1);
      ++c;
    }
  auto conflicts = [&]() {  // extra gather cycles: Σ (max count - 1) over gather groups
    int tot = 0;
    for (int q = 0; q < ng; ++q) {
      if (gstore[q]) continue;
      int mx = 0;
      for (int c = 0; c < W; ++c) mx = std::max(mx, cnt[(size_t)q * W + c]);
      tot += mx - 1;
    }
    return tot;
  };
  if (cost_before) *cost_before = conflicts();
  uint64_t rs = 0x9E3779B97F4A7C15ull ^ (uint64_t)m * 0x100000001B3ull;
  auto rnd = [&]() {
    rs ^= rs << 13;
    rs ^= rs >> 7;
    rs ^= rs << 17;
    return rs;
  };
  const long long iters = std::min<long long>(4000000LL, (long long)m * env_int("QLDPC_LABEL_IT", 600));
  for (long long it = 0; it < iters; ++it) {
    const int a = (int)(rnd() % (uint64_t)m), b = (int)(rnd() % (uint64_t)m);
    if (a == b) continue;
    const int la = lab[a], lb = lab[b];
    // delta of Σ count² when a takes label lb and b takes la
    long long delta = 0;
    auto move = [&](int q, int from, int to) {
      const int cf = col(q, from), ct = col(q, to);
      if (cf == ct) return;
      int& x = cnt[(size_t)q * W + cf];
      int& y = cnt[(size_t)q * W + ct];
      delta += (long long)gw[q] * ((2 * y + 1) - (2 * x - 1));
      --x;
      ++y;
    };
    for (int q : of[a]) move(q, la, lb);
    for (int q : of[b]) move(q, lb, la);
    if (delta <= 0 && (delta < 0 || (rnd() & 3) == 0)) {
      lab[a] = lb;
      lab[b] = la;
      cost += delta;
    } else {  // undo (reverse order)
      for (int q : of[b]) {
        const int cf = col(q, lb), ct = col(q, la);
        if (cf == ct) continue;
        ++cnt[(size_t)q * W + cf];
        --cnt[(size_t)q * W + ct];
      }
      for (int q : of[a]) {
        const int cf = col(q, la), ct = col(q, lb);
        if (cf == ct) continue;
        ++cnt[(size_t)q * W + cf];
        --cnt[(size_t)q * W + ct];
      }
    }
  }
  if (cost_after) *cost_after = conflicts();
  return lab;
}

// The plain CSR and CSC of bp's graph on the device (edge ids in row-major order, rows ascending per
// column): what the row-ordered / column-ordered passes of engines 5 and 7 walk.
static int upload_csr_csc(qldpc_bp* bp) {
  const qldpc_graph* g = bp->g;
  const int E = g->nnz;
  std::vector<int32_t> cp(g->n + 1, 0), ce;
  ce.reserve(E);
  for (int j = 0; j < g->n; ++j) {
    for (int i : g->col_rows[j]) {
      const int* b = g->col_idx.data() + g->row_ptr[i];
      const int* e = g->col_idx.data() + g->row_ptr[i + 1];
      ce.push_back((int32_t)(std::lower_bound(b, e, j) - g->col_idx.data()));
    }
    cp[j + 1] = (int32_t)ce.size();
  }
  int rc;
  if ((rc = bp->ps_rp.alloc((size_t)(g->m + 1) * 4)) || (rc = bp->ps_ci.alloc((size_t)std::max(1, E) * 4)) ||
      (rc = bp->ps_cp.alloc((size_t)(g->n + 1) * 4)) || (rc = bp->ps_ce.alloc((size_t)std::max(1, E) * 4)))
    return rc;
  if (hipMemcpy(bp->ps_rp.p, g->row_ptr.data(), (size_t)(g->m + 1) * 4, hipMemcpyHostToDevice) != hipSuccess ||
      (E && hipMemcpy(bp->ps_ci.p, g->col_idx.data(), (size_t)E * 4, hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(bp->ps_cp.p, cp.data(), cp.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
      (E && hipMemcpy(bp->ps_ce.p, ce.data(), (size_t)E * 4, hipMemcpyHostToDevice) != hipSuccess))
    return set_err(QLDPC_EHIP, "upload the graph's CSR / CSC");
  return 0;
}

// Engine 5 (product-sum): the row-ordered / column-ordered products need the
// plain CSR and CSC (edge ids in row-major order, rows ascending per column).
static int create_ps(qldpc_graph* g, const double* channel_probs, int32_t max_iter, int32_t precision,
                     qldpc_bp** out) {
  auto* bp = new qldpc_bp();
  bp->g = g;
  bp->route.engine = 5;
  bp->method = QLDPC_PRODUCT_SUM;
  bp->route.precision = precision;
  bp->max_iter = max_iter > 0 ? max_iter : g->n;
  bp->alpha = 0;
  bp->route.TB = 256;
  bp->route.VPL = (g->n + 255) / 256;
  bp->probs.assign(channel_probs, channel_probs + g->n);
  auto fail = [&](int code) {
    for (DevBuf* d : {&bp->llr, &bp->ps_rp, &bp->ps_ci, &bp->ps_cp, &bp->ps_ce, &bp->ps_ws}) d->release();
    delete bp;
    return code;
  };
  const int E = g->nnz;
  int rc;
  if ((rc = upload_csr_csc(bp)) || (rc = bp->llr.alloc((size_t)g->n * (precision == 32 ? 4 : 8)))) return fail(rc);
  if ((rc = upload_llr(bp))) return fail(rc);
  // messages in LDS when 2E values fit in 96 KiB (>= 1 workgroup per CU with room), else in HBM
  const bool lds_msgs = ps_lds_bytes(precision, g->m, g->n, E, true) <= 96 * 1024;
  bp->route.lds_bytes = (int)ps_lds_bytes(precision, g->m, g->n, E, lds_msgs);
  if (bp->route.lds_bytes > kLdsMax) return fail(set_err(QLDPC_ENOTSUP, "graph too large for the product-sum engine"));
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, ps_kernel(precision), bp->route.TB, bp->route.lds_bytes) != hipSuccess)
    nb = 1;
  bp->blocks_per_cu = std::max(1, nb);
  if ((rc = device_cus(g->device, bp->cus))) return fail(rc);
  bp->ps_grid = (long long)bp->blocks_per_cu * bp->cus;
  if (!lds_msgs && (rc = bp->ps_ws.alloc((size_t)bp->ps_grid * 2 * E * (precision == 32 ? 4 : 8)))) return fail(rc);
  *out = bp;
  return 0;
}

static int create_min_sum(qldpc_graph* g, const double* channel_probs, int32_t max_iter, int32_t bp_method,
                          double ms_scaling_factor, int32_t precision, int32_t vars_per_thread,
                          int32_t min_col_slots, int forced_engine, qldpc_bp** out);

// The one-iteration first-min step kernel of a max_iter = 1 min-sum decoder (decode_batch routes
// its decodes there), built when the decoder is created and whenever its priors change, so that
// decode_batch only launches kernels (no synchronous uploads or occupancy queries between
// stream-ordered launches).  Graphs past the kernel's LDS envelope keep the engine.
static void bp1_prepare(qldpc_bp* bp) {
  if (bp->bp1) {
    qldpc_firstmin_destroy(bp->bp1);
    bp->bp1 = nullptr;
  }
  // (a relay decoder with one iteration in all still runs its own law: memory term, solution weights;
  // one serial sweep is not one flooding iteration)
  bp->bp1_off = !(bp->max_iter == 1 && bp->method == 1) || bp->route.engine >= 7 || env_int("QLDPC_BP1", 1) == 0;
  if (bp->bp1_off) return;
  const std::string keep = qldpc_rt::g_err;  // an ENOTSUP here is not the caller's error
  if (qldpc_firstmin_create(bp->g, bp->probs.data(), 0, bp->alpha, bp->route.precision, &bp->bp1) != 0) {
    bp->bp1 = nullptr;
    bp->bp1_off = true;
    qldpc_rt::g_err = keep;
  }
}

int qldpc_bp_create(qldpc_graph* g, const double* channel_probs, int32_t max_iter, int32_t bp_method,
                    double ms_scaling_factor, int32_t precision, int32_t vars_per_thread, int32_t min_col_slots,
                    qldpc_bp** out) {
  return create_min_sum(g, channel_probs, max_iter, bp_method, ms_scaling_factor, precision, vars_per_thread,
                        min_col_slots, 0, out);
}

// Engine 6: HBM-resident messages, one decode per lane (any graph; chosen automatically when
// no LDS engine holds the per-decode image).
int qldpc_bp_create_hbm(qldpc_graph* g, const double* channel_probs, int32_t max_iter, double ms_scaling_factor,
                        int32_t precision, qldpc_bp** out) {
  return create_min_sum(g, channel_probs, max_iter, QLDPC_MIN_SUM, ms_scaling_factor, precision, 0, 0, 6, out);
}

// Engine 1 is the one whose decode kernel can hand back the final posteriors.
int qldpc_bp_create_soft(qldpc_graph* g, const double* channel_probs, int32_t max_iter, double ms_scaling_factor,
                         int32_t precision, qldpc_bp** out) {
  return create_min_sum(g, channel_probs, max_iter, QLDPC_MIN_SUM, ms_scaling_factor, precision, 0, 0, 1, out);
}

// ------------------------------------------------------------- route plan
// Host only: no hip* call, no device buffer (qldpc_bp_plan runs it on a machine without a GPU).

static bool uniform_priors(const double* probs, int n) {
  for (int j = 1; j < n; ++j)
    if (probs[j] != probs[0]) return false;
  return true;
}

static int validate_create(const qldpc_graph* g, const double* channel_probs, int precision, int bp_method) {
  if (!g || !channel_probs) return set_err(QLDPC_EINVAL, "NULL argument");
  if (precision != 32 && precision != 64) return set_err(QLDPC_EINVAL, "precision must be 32 or 64");
  if (bp_method != QLDPC_MIN_SUM && bp_method != QLDPC_PRODUCT_SUM)
    return set_err(QLDPC_EINVAL, "bp_method must be 0 (product_sum) or 1 (minimum_sum)");
  // (n = 0 never gets a graph handle; the kernels read the first row and column unconditionally)
  if (g->m <= 0) return set_err(QLDPC_EINVAL, "a decoder needs at least one check (m = 0)");
  return 0;
}

static bool fits(const Route& c, const qldpc_graph* g) { return route_fits(c, route_vslots(c, g->m), g->m); }

// engine 6: messages in HBM, one decode per lane (bp_hbm.hip) -- requested, or when no LDS engine
// serves the graph (`why`; QLDPC_HBM_FALLBACK=0 makes that an error instead)
static int to_hbm(const qldpc_graph* g, Route& r, std::vector<int32_t>& slot_var, const char* why = nullptr) {
  if (why && env_int("QLDPC_HBM_FALLBACK", 1) == 0) return set_err(QLDPC_ENOTSUP, why);
  // the engine's row / column records (hbm_prepare refuses the same graphs with the same message)
  if (g->max_row > kHbmMaxDeg || g->max_col > kHbmMaxDeg)
    return set_err(QLDPC_ENOTSUP, "HBM engine: row or column degree above 12");
  r.engine = 6;
  r.TB = kHbmThreads;
  r.VPL = 1;
  r.lds_bytes = 0;
  r.ea_shift = r.tail = r.m2s = r.fb = r.m2s_pk = r.vslots_dummy = r.d3k = r.d2k = 0;
  r.nw = r.live_last = 0;
  slot_var.clear();
  return 0;
}

// rows one message wider than whole chunks (space-time graphs: rows of 9 = 4 fp64 / 2 fp32
// chunks + 1): chunk rows + a tail slot per row, dword-scaled addresses, 1024-thread
// workgroups.  fp64: the image fits LDS at all (162.7 KB instead of 176 KB); fp32: the check
// phase reads 36 instead of 48 bytes per row through the compile-time-width loop.  fp64 images
// past the 16-bit layout's 64 KiB take it too (round 6: e.g. hgp_34_n1600 over two rounds, 1536 x
// 4736, 117 KB, which ran on engine 2 before: fp64 engine 3 has no dword-scaled plain layout), and
// so do fp64 rows of 8 (the tail slot stays empty: GenBicycleA3 / A4 over 2-5 rounds) and graphs
// whose geometry is 512 threads (hgp_34_n625 over three rounds, 900 x 2775: two decodes per CU)
static void admit_tail(const qldpc_graph* g, int vars_per_thread, Route& r) {
  const bool f64t = r.precision == 64 && env_int("QLDPC_E3_TAIL64", 1) != 0;
  Route plain = r;
  plain.ea_shift = f64t ? 0 : 2;
  if (!(r.engine == 3 && r.DMAX == 4 && (g->max_row == 9 || (f64t && g->max_row == 8)) && env_int("QLDPC_E3_TAIL", 1) != 0 &&
        (r.precision == 32 || !fits(plain, g))))
    return;
  Route c = r;
  c.tail = 1;
  c.nch = r.precision == 32 ? 2 : 4;  // 8 messages
  c.ea_shift = 2;
  // fp32: byte F words shrink the image below half a CU (config 5: 85.1 -> 79.6 KB), so two
  // 512-thread decodes share a CU (bp_reg.h eng_fb; QLDPC_E3_FB=0 keeps one 1024-thread decode)
  Route fb = c;
  fb.fb = 1;
  fb.TB = 512;
  fb.VPL = (g->n + 511) / 512;
  int tb = 0, vpl = 0;
  if (r.precision == 32 && vars_per_thread <= 0 && env_int("QLDPC_TB", 0) <= 0 && env_int("QLDPC_E3_FB", 1) != 0 &&
      fb.VPL >= 9 && fb.VPL <= 12 && (g->m + 511) / 512 <= 32 && fits(fb, g) &&
      2 * route_lds(fb, route_vslots(fb, g->m), g->m) <= (size_t)kLdsMax)
    r = fb;
  else if (fits(c, g) && !choose_rgeometry(g->n, g->m, vars_per_thread, tb, vpl) && (tb > 512 || (f64t && tb == 512)) &&
           vpl >= 4 && vpl <= 8)
    r = c;
}

// fp64 "m2 in slot" family (bp_reg.h eng_m2s, kern_r_f64_m2s.hip): one-word check state, m2 in
// the argmin edge's V slot, rows of up to 7 edges as 3 chunks + a tail slot, <= 256 threads.
// The headline hgp_34_n1600 image drops from 65.0 KB to 52.3 KB: 3 workgroups per CU instead
// of 2.  The kernel keeps no dummy edges for real variables, so every column degree must be
// 3 or 4 with the degree-3 variables filling whole variable slots (host degree sort).
// (`uniform`: the kernels hold one prior for every variable)
static void admit_m2s(const qldpc_graph* g, bool uniform, int vars_per_thread, Route& r) {
  if (!(r.engine == 3 && r.precision == 64 && r.DMAX == 4 && !r.tail && g->max_row >= 1 && g->max_row <= 7 &&
        env_int("QLDPC_M2S", 1) != 0 && env_int("QLDPC_DEGSORT", 1) != 0))
    return;
  int tb = 0, vpl = 0, n3 = 0, nother = 0;
  for (int j = 0; j < g->n; ++j) {
    const int d = (int)g->col_rows[j].size();
    n3 += d == 3;
    nother += d != 3 && d != 4;
  }
  Route c = r;
  c.tail = 1;
  c.m2s = 1;
  c.nch = 3;
  c.ea_shift = 0;
  if (nother || !uniform || choose_rgeometry(g->n, g->m, vars_per_thread, tb, vpl) || tb > 256 || vpl < 4 || vpl > 8 ||
      !(n3 % tb == 0 || n3 == g->n) || !fits(c, g))
    return;
  r = c;
}

// fp64 space-time graphs on the tail layout (rows of 8 / 9 as 4 chunks + a tail slot, 1024 threads,
// one decode per CU): the one-word check state too (round 6, kern_r_f64_m2st.hip, engine id
// 111313).  The two-word tail family re-reads each edge's own previous v2c from LDS (its 128-VGPR
// budget had no room for it) and gathers 16-byte check states: 24 B of variable-phase reads per
// edge.  Here the own v2c lives in VGPRs (118 with the uniform prior in SGPRs, no scratch) and an
// edge reads the 8-byte CS and its own slot: 16 B.  Real variables never touch a shared dummy:
// the measurement variables in 3-edge slots and the degree-3 ones in 4-edge slots get private
// dummy V slots (config 5: 1,348, 10.8 KB), placed before the tail array.  Uniform priors only.
// Known, out of scope here: admitted for d2 >= 1 against a kernel compiled for D2K = 1.
static void admit_m2st(const qldpc_graph* g, bool uniform, int vars_per_thread, Route& r) {
  if (!(r.engine == 3 && r.precision == 64 && r.DMAX == 4 && r.tail && !r.fb && !r.m2s && r.nch == 4 &&
        env_int("QLDPC_M2ST", 1) != 0 && env_int("QLDPC_DEGSORT", 1) != 0 && env_int("QLDPC_D2K", 1) != 0))
    return;
  int tb = 0, vpl = 0;
  if (!uniform || choose_rgeometry(g->n, g->m, vars_per_thread, tb, vpl) || tb < 512) return;
  // the slot map plan_route makes below (st_plan), its D2K / D3K and the private dummies of
  // build_slot_edges
  const StPlan P = st_plan(g, tb, vpl, r.DMAX, env_int("QLDPC_NW", 1) != 0, env_int("QLDPC_NW_BAL", 1) != 0);
  Route c = r;
  c.m2s = 1;
  c.vslots_dummy = P.nd;
  c.nw = P.nw;
  c.live_last = P.live_last;
#if QLDPC_DIAG_NOLAST
  // diagnostic builds only (results invalid): no wave runs the last variable slot, to time the
  // cost of the waves that hold it
  c.live_last = 0;
#endif
  if (g->max_col <= r.DMAX && P.d2 >= 1 && route_vslots(c, g->m) < 0x3FFFF && get_rvariant_f64_m2st(vpl, P.d3, P.d2).dec_k &&
      fits(c, g))
    r = c;
}

// fp64 column degree 5 graphs that come out at 512 threads x <= 3 variables (LP_Matg8_L21 / L30's
// [h | I], 315 x 1029 / 450 x 1470): the two-word degree-5 family at 256 threads x 5 / 6 variables
// instead of engine 2 (round 6; QLDPC_D5_256=0 keeps the old geometry).  Admits by choosing
// vars_per_thread for the geometry call of plan_route.
static void admit_d5_256(const qldpc_graph* g, const Route& r, int pref, int& vars_per_thread, int& vmax) {
  if (!(r.engine == 3 && r.precision == 64 && r.DMAX == 5 && vars_per_thread <= 0 && env_int("QLDPC_TB", 0) <= 0 &&
        env_int("QLDPC_D5_256", 1) != 0 && g->max_row > 8 && g->max_row <= 10))
    return;
  int tb = 0, vpl = 0;
  if (choose_rgeometry(g->n, g->m, 0, tb, vpl, pref, vmax) || tb <= 256) return;
  for (int v = 5; v <= 6 && vars_per_thread <= 0; ++v) {
    int tb5 = 0, vpl5 = 0;
    if (!choose_rgeometry(g->n, g->m, v, tb5, vpl5, pref, 6) && tb5 <= 256) {
      vars_per_thread = v;
      vmax = std::max(vmax, v);
    }
  }
}

// the m2s family for rows of 8 and column degree 5 (kern_r_f64_m2s8.hip, engine id 10103): the
// lifted-product codes (LP_Matg8_L30: 750 degree-3 and 270 degree-5 columns, rows of 8).  Rows of
// 4 chunks, no tail array.  Slots k >= D3K hold 5 edge slots; a real variable with fewer edges
// there (a degree-3 variable in the slot shared with the degree-5 class) gets a PRIVATE dummy V
// slot per missing edge, past the rows, and the dummy CS entry 0 (+0, parity 0): no other lane
// writes that slot, so the variable phase always reads its own previous v2c back and takes
// c2v = +-0, which leaves every sum bit-exact (w-domain sums are never -0).  The two-word family
// runs these graphs at 2 workgroups per CU (256 VGPRs); the one-word state fits 3.
static void admit_m2s8(const qldpc_graph* g, bool uniform, int pref, int vmax, int& vars_per_thread, Route& r) {
  if (!(r.engine == 3 && r.precision == 64 && r.DMAX == 5 && !r.tail && !r.m2s && g->max_row >= 1 && g->max_row <= 8 &&
        env_int("QLDPC_M2S", 1) != 0 && env_int("QLDPC_M2S8", 1) != 0 && env_int("QLDPC_DEGSORT", 1) != 0))
    return;
  int tb = 0, vpl = 0, n3 = 0, small_vpt = 0;
  for (int j = 0; j < g->n; ++j) n3 += g->col_rows[j].size() <= 3;
  if (!uniform || choose_rgeometry(g->n, g->m, vars_per_thread, tb, vpl, pref, vmax)) return;
  // smaller graphs (LP_Matg8_L16 / L21, the Threshold notebook's codes: 544 / 714 columns) come out
  // at 256 threads x 3 variables, below the family's 4-6: run them at the most variables per thread
  // (<= 5 for degree 5) whose workgroup is smaller, 128 x 5 / 192 x 5 (round 6; they ran on engine 2
  // before).  The geometry call of plan_route then takes this VPL.
  if (tb == 256 && vpl < 4 && vars_per_thread <= 0 && env_int("QLDPC_TB", 0) <= 0 && env_int("QLDPC_M2S8_SMALL", 1) != 0)
    for (int v = std::min(6, vmax); v >= 4 && !small_vpt; --v) {
      int tb2 = 0, vpl2 = 0;
      if (!choose_rgeometry(g->n, g->m, v, tb2, vpl2, pref, vmax) && tb2 < 256 && vpl2 == v) {
        tb = tb2;
        vpl = vpl2;
        small_vpt = v;
      }
    }
  if (!((tb == 256 || (tb < 256 && small_vpt > 0)) && vpl >= 4 && vpl <= 6)) return;
  // the slot map of plan_route: degree <= 3 first, so slots k < n3 / tb (whole) hold degree <= 3 only
  const int d3 = n3 == g->n ? vpl : n3 / tb;
  const std::vector<int32_t> order = degree_sorted(g, {3});
  Route c = r;
  c.m2s = 1;
  c.nch = 4;
  c.ea_shift = 0;
  for (int p = 0; p < g->n; ++p) c.vslots_dummy += ((p / tb) < d3 ? 3 : r.DMAX) - (int)g->col_rows[order[p]].size();
  if (route_vslots(c, g->m) >= 0xFFFF || !fits(c, g)) return;
  r = c;
  if (small_vpt > 0) vars_per_thread = small_vpt;
  // packed absolute addresses, 4 workgroups per CU: LP L30 fp64 4.08 M vs 3.67 M shots/s
  // (0.622 vs 0.561 of the LDS roofline, profiles/r04/passd/); QLDPC_M2S8_PK=0 keeps 10103
  r.m2s_pk = env_int("QLDPC_M2S8_PK", 1) != 0 && vpl <= 5 && 4 * route_lds(c, route_vslots(c, g->m), g->m) <= (size_t)kLdsMax;
}

// The route of a min-sum decoder and its slot map (engines 2-3: the variable of every (k, t) slot,
// -1 = padding), from the graph, whether the priors are uniform, and the QLDPC_* switches.
static int plan_route(const qldpc_graph* g, bool uniform, int precision, int vars_per_thread, int min_col_slots,
                      int forced_engine, Route& r, std::vector<int32_t>& slot_var) {
  const int want_engine = forced_engine ? forced_engine : env_int("QLDPC_ENGINE", 3);
  if (want_engine == 4) return set_err(QLDPC_ENOTSUP, "engine 4 (c2v computed by the check phase) was removed");
  r = Route();
  slot_var.clear();
  r.precision = precision;
  r.engine = ((want_engine >= 1 && want_engine <= 3) || want_engine == 6) ? want_engine : 3;
  // column degree > 8: beyond the LDS engines' edge slots -> engine 6 (row and column degree <= 12); soft BP stays engine 1
  if ((g->max_col > 8 || min_col_slots > 8) && r.engine != 6) {
    if (r.engine == 1) return set_err(QLDPC_ENOTSUP, "column degree > 8");
    r.engine = 6;
  }
  const int colmax = std::max(g->max_col, min_col_slots);
  r.DMAX = colmax <= 4 ? 4 : 8;
  // engine 3 also takes fp32 graphs with column degree 5-6 (lifted-product codes), exact slot count
  if (r.engine == 3 && precision == 32 && colmax > 4 && colmax <= 6 && env_int("QLDPC_E3_D56", 1) != 0) r.DMAX = colmax;
  // fp64: column degree 5 on the <= 256-thread family (checked with the geometry below)
  if (r.engine == 3 && precision == 64 && colmax == 5 && env_int("QLDPC_E3_D56", 1) != 0) r.DMAX = 5;
  if (r.engine == 6) return to_hbm(g, r, slot_var);
  const int tsize = precision == 32 ? 4 : 8;
  if (r.engine == 1) {
    const int rc = choose_geometry(g->n, g->m, vars_per_thread, max_spill_free_vpl(precision, r.DMAX), r.TB, r.VPL);
    if (rc) return rc;
    r.lds_bytes = (int)lds_for(precision, g->m);
    return get_variant(precision, r.VPL, r.DMAX).dec_k ? 0 : set_err(QLDPC_ENOTSUP, "no kernel variant");
  }
  r.nch = (std::max(1, g->max_row) * tsize + 15) / 16;
  // no LDS image addresses this many slots: HBM-resident messages (engine 6)
  if (route_vslots(r, g->m) >= 0xFFFF)
    return to_hbm(g, r, slot_var, "V image exceeds 65535 message slots (QLDPC_HBM_FALLBACK=0)");
  // degree-5/6 variables hold 2.5x the registers of degree-4 ones: fewer per thread
  const int pref = r.DMAX == 4 ? kPrefVplR : 4;
  int vmax = r.DMAX == 4 ? kMaxVplR : 5;
  // images of 64-256 KiB (space-time graphs): engine 3 with dword-scaled addresses (fp32, 4 slots)
  Route big = r;
  big.ea_shift = 2;
  if (r.engine == 3 && precision == 32 && r.DMAX == 4 && !fits(r, g) && fits(big, g) && env_int("QLDPC_E3_BIG", 1) != 0) r = big;
  admit_tail(g, vars_per_thread, r);
  admit_m2s(g, uniform, vars_per_thread, r);
  admit_m2st(g, uniform, vars_per_thread, r);
  admit_d5_256(g, r, pref, vars_per_thread, vmax);
  admit_m2s8(g, uniform, pref, vmax, vars_per_thread, r);
  if (r.engine == 3 && ((r.DMAX != 4 && r.DMAX != 5 && r.DMAX != 6) ||
                        (!r.fb && choose_rgeometry(g->n, g->m, vars_per_thread, r.TB, r.VPL, pref, vmax)) || !fits(r, g) ||
                        (precision == 64 && r.DMAX == 5 && !r.m2s && !use_f64w(r)))) {
    r.ea_shift = r.tail = r.m2s = r.vslots_dummy = r.m2s_pk = r.fb = 0;
    r.engine = 2;  // graph outside the register engines' envelope
    r.nch = (std::max(1, g->max_row) * tsize + 15) / 16;
    if (r.DMAX == 5 || r.DMAX == 6) r.DMAX = 8;  // engine 2 kernels come in 4 and 8 slots
  }
  const int vslots = route_vslots(r, g->m);
  if (r.engine == 3) {
    r.NS = 1;
    r.lds_bytes = (int)route_lds(r, vslots, g->m);
  } else {
    const int rc = choose_sgeometry(g->n, g->m, vars_per_thread, r.TB, r.VPL);
    if (rc) return rc;
    const int img = (int)slot_img_bytes(vslots, g->m, tsize);
    r.NS = choose_ns(img);
    r.lds_bytes = (int)slot_lds_bytes(r.NS, img, kChunkMax);
    // big images leave room for few workgroups per CU: widen the workgroup so
    // the CU still holds >= 16 waves (ST n1225 fp32: 1 x 1024 threads, 2x the
    // samples/s of 1 x 256, bench.py --workload phenl)
    const int bpc = std::max(1, kLdsMax / std::max(1, r.lds_bytes));
    if (vars_per_thread <= 0 && env_int("QLDPC_TB", 0) <= 0 && bpc * r.TB / 64 < 16) {
      const int tb = std::min(kMaxThreadsS, round_up((16 + bpc - 1) / bpc * 64, 64));
      if (tb > r.TB) {
        r.TB = tb;
        r.VPL = (g->n + tb - 1) / tb;
      }
    }
  }
  // no LDS engine holds this decode: HBM-resident messages
  if (r.lds_bytes > kLdsMax) return to_hbm(g, r, slot_var, "per-shot LDS image exceeds 160 KiB (QLDPC_HBM_FALLBACK=0)");
  // slot -> variable map: identity, or (engine 3) degree <= 3 variables first
  const bool sort3 = r.engine == 3 && r.DMAX >= 4 && env_int("QLDPC_DEGSORT", 1) != 0;
  // byte-F kernels also keep degree <= 2 variables (the space-time measurement columns) in
  // compile-time 2-edge slots: those go first
  const bool sort2 = sort3 && (r.fb || (r.tail && precision == 64 && (!r.m2s || r.nch == 4))) && env_int("QLDPC_D2K", 1) != 0;
  if (r.engine == 3 && precision == 64 && r.tail && r.m2s && r.nch == 4) {
    // (the fp64 space-time m2s family: st_plan's order, degree classes 1 / 2 / 3 / 4 with narrow waves)
    slot_var = st_plan(g, r.TB, r.VPL, r.DMAX, env_int("QLDPC_NW", 1) != 0, env_int("QLDPC_NW_BAL", 1) != 0).slots;
  } else {
    slot_var = sort2 ? degree_sorted(g, {2, 3}) : sort3 ? degree_sorted(g, {3}) : degree_sorted(g, {});
    slot_var.resize((size_t)r.VPL * r.TB, -1);
  }
  r.d3k = sort3 ? leading_slots(g, slot_var, r.TB, r.VPL, 3) : 0;
  r.d2k = sort2 ? leading_slots(g, slot_var, r.TB, r.VPL, 2) : 0;
  // fp64 engine-3 kernels are built with D3K = 0 only, except the <= 256-thread family
  if (precision != 32 && !use_f64w(r) && !r.tail && !r.m2s) r.d3k = 0;
  if (slot_variant(r).dec_k) return 0;
  // no kernel compiled for this engine-3 geometry (e.g. fp32 images past 64 KiB at 8 variables per
  // thread, GenBicycleA4 over five rounds): the HBM-resident engine serves any graph
  return r.engine == 3 ? to_hbm(g, r, slot_var, "no kernel variant") : set_err(QLDPC_ENOTSUP, "no kernel variant");
}

// ------------------------------------------------------------ host tables
struct HostTables {
  std::vector<uint32_t> edges;  // engine 1: packed u16 check ids; engines 2-3: edge words
  std::vector<int> lab;         // engine 3: label of each check (empty = identity)
  std::vector<uint8_t> rdeg;    // engine 3: row degrees by check label
};

// The host tables of a planned decoder (bp->route, bp->slot_var), plus its label / LDS-model
// statistics.
static int build_tables(qldpc_bp* bp, HostTables& T) {
  const qldpc_graph* g = bp->g;
  const Route& r = bp->route;
  if (r.engine == 1) {
    const int TB = r.TB, VPL = r.VPL, DM = r.DMAX, D2 = DM / 2;
    T.edges.assign((size_t)VPL * D2 * TB, 0xFFFFFFFFu);
    for (int k = 0; k < VPL; ++k)
      for (int t = 0; t < TB; ++t) {
        const int j = k * TB + t;
        if (j >= g->n) continue;
        const auto& rows = g->col_rows[j];
        for (int d = 0; d < DM; ++d) {
          const uint32_t v = d < (int)rows.size() ? (uint32_t)rows[d] : 0xFFFFu;
          uint32_t& w = T.edges[((size_t)k * D2 + d / 2) * TB + t];
          w = (d & 1) ? ((w & 0xFFFFu) | (v << 16)) : ((w & 0xFFFF0000u) | v);
        }
      }
    return 0;
  }
  const int tsize = r.precision == 32 ? 4 : 8;
  const RLayout L = route_layout(r, route_vslots(r, g->m), g->m);
  // fp64 two-word families (measured +3 % with the bank-aware fp64 v2c placement); fp32 gathers of
  // the structured codes are already near conflict-free, and the m2s family runs 2.5 % faster on
  // the identity labels (1.188 M vs 1.159 M shots/s, profiles/r03/m2s_ab/ab_label.txt): off there
  // (QLDPC_LABEL=1 forces it on)
  if (r.engine == 3 && env_int("QLDPC_LABEL", r.precision == 64 && !r.m2s ? 1 : 0) != 0)
    T.lab = label_checks(g, r, bp->slot_var, &bp->gather_conf[0], &bp->gather_conf[1]);
  const bool f64e3 = r.engine == 3 && r.precision == 64;
  int ndummy = 0;
  build_slot_edges(g, r, bp->slot_var, T.edges, (r.engine == 3 && env_int("QLDPC_BANKOPT", 1) != 0) ? (int)(L.v / 4) : -1,
                   T.lab, r.m2s && env_int("QLDPC_M2S_PLACE", 1) != 0,
                   r.vslots_dummy ? (1 + g->m * r.nch) * (16 / tsize) : -1, &ndummy,
                   !f64e3 ? 0 : (r.m2s || r.tail) ? 1 : env_int("QLDPC_ANNEAL_2W", 1) != 0 ? 2 : 0, -1,
                   (r.tail && r.vslots_dummy) ? (int)(L.t - L.v) / tsize : -1);
  if (ndummy != r.vslots_dummy) return set_err(QLDPC_EINVAL, "m2s private dummy slot count mismatch");
  if (f64e3 && r.ea_shift == 0) lds_model_var_phase(T.edges, r, L.v, bp->lds_model);
  if (r.engine == 3) {
    // row degrees by check label: the kernels keep their parity in F (bp_reg.h, w domain)
    T.rdeg.resize(std::max(1, g->m));
    for (int i = 0; i < g->m; ++i) T.rdeg[T.lab.empty() ? i : T.lab[i]] = (uint8_t)(g->row_ptr[i + 1] - g->row_ptr[i]);
  }
  return 0;
}

static int upload(DevBuf& buf, const void* src, size_t bytes, const char* what) {
  if (const int rc = buf.alloc(std::max<size_t>(bytes, 1))) return rc;
  if (bytes && hipMemcpy(buf.p, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return set_err(QLDPC_EHIP, what);
  return 0;
}

// validate -> plan the route -> build the host tables -> upload -> occupancy -> first-min step
static int create_min_sum(qldpc_graph* g, const double* channel_probs, int32_t max_iter, int32_t bp_method,
                          double ms_scaling_factor, int32_t precision, int32_t vars_per_thread,
                          int32_t min_col_slots, int forced_engine, qldpc_bp** out) {
  if (!out) return set_err(QLDPC_EINVAL, "NULL argument");
  int rc = validate_create(g, channel_probs, precision, bp_method);
  if (rc) return rc;
  QLDPC_HIP(hipSetDevice(g->device));
  if (bp_method == QLDPC_PRODUCT_SUM) return create_ps(g, channel_probs, max_iter, precision, out);
  auto* bp = new qldpc_bp();
  auto fail = [&](int code) {
    qldpc_bp_destroy(bp);
    return code;
  };
  bp->g = g;
  bp->max_iter = max_iter > 0 ? max_iter : g->n;
  bp->method = bp_method;
  bp->alpha = ms_scaling_factor;
  bp->probs.assign(channel_probs, channel_probs + g->n);
  if ((rc = plan_route(g, uniform_priors(channel_probs, g->n), precision, vars_per_thread,
                       min_col_slots, forced_engine, bp->route, bp->slot_var)))
    return fail(rc);
  const Route& r = bp->route;
  const int tsize = precision == 32 ? 4 : 8;
  const void* kern;
  if (r.engine == 6) {
    if ((rc = hbm_prepare(bp)) || (rc = bp->llr.alloc((size_t)g->n * tsize))) return fail(rc);
    kern = hbm_kernel(precision);
  } else {
    HostTables T;
    if ((rc = build_tables(bp, T))) return fail(rc);
    bp->npos = g->n;
    if (!T.lab.empty()) {
      std::vector<int32_t> inv(g->m);
      for (int i = 0; i < g->m; ++i) inv[T.lab[i]] = i;
      if ((rc = upload(bp->rperm, inv.data(), inv.size() * 4, "upload check labels"))) return fail(rc);
    }
    if ((r.engine == 3 && (rc = upload(bp->rdeg, T.rdeg.data(), T.rdeg.size(), "upload row degrees"))) ||
        (rc = upload(bp->vchk, T.edges.data(), T.edges.size() * 4, "upload edge table")) ||
        (!bp->slot_var.empty() && (rc = upload(bp->perm, bp->slot_var.data(), bp->slot_var.size() * 4, "upload slot map"))) ||
        (rc = bp->llr.alloc((size_t)r.VPL * r.TB * tsize)))
      return fail(rc);
    kern = r.engine == 1 ? get_variant(precision, r.VPL, r.DMAX).dec_k : slot_variant(r).dec_k;
  }
  if ((rc = upload_llr(bp))) return fail(rc);
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, r.TB, r.lds_bytes) != hipSuccess) nb = 1;
  bp->blocks_per_cu = std::max(1, nb);
  if ((rc = device_cus(g->device, bp->cus))) return fail(rc);
  bp1_prepare(bp);
  *out = bp;
  return 0;
}

int qldpc_bp_plan(const qldpc_graph* g, const double* channel_probs, int32_t bp_method, int32_t precision,
                  int32_t vars_per_thread, int32_t min_col_slots, int32_t* out, int32_t out_len) {
  if (!out || out_len < 8) return set_err(QLDPC_EINVAL, "out needs 8 entries");
  int rc = validate_create(g, channel_probs, precision, bp_method);
  if (rc) return rc;
  if (bp_method == QLDPC_PRODUCT_SUM) return set_err(QLDPC_ENOTSUP, "the product-sum geometry needs the device");
  Route r;
  std::vector<int32_t> slot_var;
  if ((rc = plan_route(g, uniform_priors(channel_probs, g->n), precision, vars_per_thread,
                       min_col_slots, 0, r, slot_var)))
    return rc;
  const int32_t v[8] = {r.engine, route_kernel_id(r), r.nch, r.TB, r.VPL, r.lds_bytes, r.engine == 3 ? r.d3k : 0,
                        r.engine == 3 ? r.d2k : 0};
  std::copy(v, v + 8, out);
  return 0;
}

int qldpc_bp_destroy(qldpc_bp* bp) {
  if (!bp) return 0;
  if (bp->bp1) qldpc_firstmin_destroy(bp->bp1);
  for (DevBuf* d : {&bp->vchk, &bp->llr, &bp->rdeg, &bp->perm, &bp->rperm, &bp->work, &bp->ps_rp, &bp->ps_ci, &bp->ps_cp,
                    &bp->ps_ce, &bp->ps_ws, &bp->h_rp, &bp->h_rcol, &bp->h_rcpos, &bp->h_cp, &bp->h_crpos, &bp->h_ws,
                    &bp->rl_gam, &bp->rl_wq, &bp->sr_cr, &bp->sr_ord, &bp->sr_lp, &bp->side_llr, &bp->side_wq})
    d->release();
  delete bp;
  return 0;
}

// Engine 7 (relay.hip): Relay-BP, min-sum with a memory term run as a chain of legs.
int qldpc_bp_create_relay(qldpc_graph* g, const double* channel_probs, int32_t pre_iter, double pre_gamma,
                          int32_t num_legs, int32_t leg_iter, double gamma_lo, double gamma_hi, int32_t stop_nconv,
                          uint64_t gamma_seed, double ms_scaling_factor, int32_t precision, qldpc_bp** out) {
  if (!out) return set_err(QLDPC_EINVAL, "NULL argument");
  int rc = validate_create(g, channel_probs, precision, QLDPC_MIN_SUM);
  if (rc) return rc;
  if ((rc = relay_check_params(g->n, pre_iter, pre_gamma, num_legs, leg_iter, gamma_lo, gamma_hi, stop_nconv, precision)))
    return rc;
  if ((long long)pre_iter + (long long)num_legs * leg_iter > 0x7fffffffLL)
    return set_err(QLDPC_EINVAL, "relay: pre_iter + num_legs * leg_iter overflows");
  QLDPC_HIP(hipSetDevice(g->device));
  auto* bp = new qldpc_bp();
  auto fail = [&](int code) {
    qldpc_bp_destroy(bp);
    return code;
  };
  bp->g = g;
  bp->route.engine = 7;
  bp->route.precision = precision;
  bp->route.TB = 256;
  bp->route.VPL = (g->n + 255) / 256;
  bp->method = QLDPC_MIN_SUM;
  bp->alpha = ms_scaling_factor;
  bp->rl_pre_iter = pre_iter;
  bp->rl_legs = num_legs;
  bp->rl_leg_iter = num_legs > 0 ? leg_iter : 0;
  bp->rl_stop = stop_nconv;
  bp->rl_pre_gamma = pre_gamma;
  bp->rl_lo = gamma_lo;
  bp->rl_hi = gamma_hi;
  bp->rl_seed = gamma_seed;
  bp->max_iter = pre_iter + num_legs * bp->rl_leg_iter;
  bp->probs.assign(channel_probs, channel_probs + g->n);
  bp->bp1_off = true;
  const int E = g->nnz;
  const size_t tsize = precision == 32 ? 4 : 8;
  if ((rc = upload_csr_csc(bp)) || (rc = bp->llr.alloc(std::max<size_t>(1, g->n) * tsize)) ||
      (rc = bp->rl_wq.alloc(std::max<size_t>(1, g->n) * 8)) ||
      (rc = bp->rl_gam.alloc(std::max<size_t>(1, (size_t)(num_legs + 1) * g->n) * tsize)) || (rc = upload_llr(bp)) ||
      (rc = relay_upload_gammas(bp)))
    return fail(rc);
  // the whole per-decode image in LDS when it fits 160 KiB, else the messages in an HBM workspace
  const bool lds_msgs =
      relay_lds_bytes(precision, g->m, g->n, E, true, false) <= (size_t)kLdsMax && env_int("QLDPC_RELAY_WS", 0) != 1;
  size_t lds = relay_lds_bytes(precision, g->m, g->n, E, lds_msgs, false);
  if (lds > (size_t)kLdsMax) return fail(set_err(QLDPC_ENOTSUP, "graph too large for the relay engine's LDS state"));
  // the graph's CSR / CSC staged in LDS as 16-bit words when that costs no resident workgroup (of
  // the 8 that 256-thread workgroups can reach); QLDPC_RELAY_IDX=0 keeps the global walk
  const size_t lds_idx = relay_lds_bytes(precision, g->m, g->n, E, lds_msgs, true);
  auto resident = [](size_t bytes) { return std::min<size_t>(8, (size_t)kLdsMax / std::max<size_t>(1, bytes)); };
  bp->rl_idx = E <= 0xffff && g->n <= 0xffff && g->m <= 0xffff && lds_idx <= (size_t)kLdsMax &&
               resident(lds_idx) == resident(lds) && env_int("QLDPC_RELAY_IDX", 1) != 0;
  if (bp->rl_idx) lds = lds_idx;
  bp->route.lds_bytes = (int)lds;
  bp->route.TB = relay_threads(lds, g->m, g->n);
  bp->route.VPL = (g->n + bp->route.TB - 1) / bp->route.TB;
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, relay_kernel_ptr(precision, bp->rl_idx), bp->route.TB,
                                                   bp->route.lds_bytes) != hipSuccess)
    nb = 1;
  bp->blocks_per_cu = std::max(1, nb);
  if ((rc = device_cus(g->device, bp->cus))) return fail(rc);
  bp->ps_grid = (long long)bp->blocks_per_cu * bp->cus;
  if (!lds_msgs && (rc = bp->ps_ws.alloc(std::max<size_t>(1, (size_t)bp->ps_grid * 2 * E * tsize)))) return fail(rc);
  *out = bp;
  return 0;
}

// Engine 8 (serial.hip): min-sum BP on the serial schedule, run as layers of independent variables.
int qldpc_bp_create_serial(qldpc_graph* g, const double* channel_probs, int32_t max_iter, double ms_scaling_factor,
                           int32_t precision, int32_t soft, qldpc_bp** out) {
  if (!out) return set_err(QLDPC_EINVAL, "NULL argument");
  int rc = validate_create(g, channel_probs, precision, QLDPC_MIN_SUM);
  if (rc) return rc;
  if ((rc = serial_check_params(g->n, max_iter, precision))) return rc;
  QLDPC_HIP(hipSetDevice(g->device));
  auto* bp = new qldpc_bp();
  auto fail = [&](int code) {
    qldpc_bp_destroy(bp);
    return code;
  };
  bp->g = g;
  bp->route.engine = 8;
  bp->route.precision = precision;
  bp->method = QLDPC_MIN_SUM;
  bp->alpha = ms_scaling_factor;
  bp->max_iter = max_iter;
  bp->probs.assign(channel_probs, channel_probs + g->n);
  bp->bp1_off = true;
  bp->sr_soft = soft != 0;
  if ((rc = upload_csr_csc(bp)) || (rc = bp->llr.alloc(std::max<size_t>(1, g->n) * (precision == 32 ? 4 : 8))) ||
      (rc = upload_llr(bp)) || (rc = device_cus(g->device, bp->cus)) ||
      (rc = serial_prepare(bp, env_int("QLDPC_SERIAL_WS", 0) == 1, env_int("QLDPC_SERIAL_IDX", 1) != 0,
                           env_int("QLDPC_SERIAL_TB", 0), kLdsMax)))
    return fail(rc);
  *out = bp;
  return 0;
}

int qldpc_bp_set_channel_probs(qldpc_bp* bp, const double* channel_probs) {
  if (!bp || !channel_probs) return set_err(QLDPC_EINVAL, "NULL argument");
  if (bp->route.m2s && !uniform_priors(channel_probs, bp->g->n))
    return set_err(QLDPC_ENOTSUP, "this decoder's kernels hold one uniform prior: create a new decoder for "
                                  "non-uniform channel_probs");
  bp->probs.assign(channel_probs, channel_probs + bp->g->n);
  const int rc = upload_llr(bp);
  if (rc) return rc;
  bp1_prepare(bp);  // rebuilt from the new priors
  return 0;
}

// Side priors of an engine-7 / engine-8 decoder: the two-row tables qldpc_bp_decode_batch_side selects
// from per syndrome and variable.  The handle's ordinary priors and every other entry point are untouched.
int qldpc_bp_set_side_probs(qldpc_bp* bp, const double* p0, const double* p1) {
  if (!bp || ((!p0 || !p1) && bp->g->n > 0)) return set_err(QLDPC_EINVAL, "NULL argument");
  if (bp->route.engine != 7 && bp->route.engine != 8)
    return set_err(QLDPC_ENOTSUP, "side priors need a Relay-BP (engine 7) or serial-schedule (engine 8) decoder");
  if (int rc = side_probs_check(bp->g->n, p0, p1)) return rc;
  QLDPC_HIP(hipSetDevice(bp->g->device));
  // (the copies are synchronous: a side decode already queued has read its tables before they change
  // only if the caller synchronised, as for qldpc_bp_set_channel_probs)
  const int rc = bp->route.engine == 7 ? relay_upload_side(bp, p0, p1) : serial_upload_side(bp, p0, p1);
  if (rc) return rc;
  // a side decode's persistent grid: what the side variant keeps resident on the plain variant's image
  // (it may need a few more registers), never more than the workspace has slices for
  const void* kern = bp->route.engine == 7 ? relay_kernel_ptr(bp->route.precision, bp->rl_idx, true)
                                           : serial_kernel_ptr(bp->route.precision, bp->sr_idx, true);
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, bp->route.TB, bp->route.lds_bytes) != hipSuccess) nb = 1;
  bp->side_grid = std::min<long long>(bp->ps_grid, (long long)std::max(1, nb) * bp->cus);
  bp->side_set = true;
  return 0;
}

int qldpc_bp_decode_batch_side(qldpc_bp* bp, const uint8_t* d_synd, const uint8_t* d_side, uint8_t* d_corr,
                               int32_t* d_iters, uint8_t* d_conv, int64_t B, void* stream) {
  if (!bp || (B > 0 && (!d_synd || !d_corr))) return set_err(QLDPC_EINVAL, "NULL argument");
  if (bp->route.engine != 7 && bp->route.engine != 8)
    return set_err(QLDPC_ENOTSUP, "a side decode needs a Relay-BP (engine 7) or serial-schedule (engine 8) decoder");
  if (!bp->side_set) return set_err(QLDPC_EINVAL, "no side priors set (qldpc_bp_set_side_probs)");
  if (B > 0 && !d_side && bp->g->n > 0) return set_err(QLDPC_EINVAL, "NULL side bytes");
  if (B <= 0) return B < 0 ? set_err(QLDPC_EINVAL, "B < 0") : 0;
  QLDPC_HIP(hipSetDevice(bp->g->device));
  if (bp->g->n == 0) d_side = nullptr;  // no variable selects anything
  if (bp->route.engine == 7)
    return relay_decode_launch(bp, d_synd, d_corr, d_iters, d_conv, B, (hipStream_t)stream, d_side);
  return serial_decode_launch(bp, d_synd, d_corr, d_iters, d_conv, nullptr, B, (hipStream_t)stream, d_side);
}

// true when qldpc_bp_decode_batch_side_soft serves the decoder: an engine-8 handle created with
// soft = 1, or an engine-7 handle without a chain (a chain's best solution has no single posterior)
static bool side_soft_capable(const qldpc_bp* bp) {
  return (bp->route.engine == 8 && bp->sr_soft) || (bp->route.engine == 7 && bp->rl_legs == 0);
}

// The soft output of a side decode (d_side = NULL: of the plain decode): corr / iters / conv are
// qldpc_bp_decode_batch[_side]'s, d_post the posteriors after the last iteration.
int qldpc_bp_decode_batch_side_soft(qldpc_bp* bp, const uint8_t* d_synd, const uint8_t* d_side, uint8_t* d_corr,
                                    int32_t* d_iters, uint8_t* d_conv, double* d_post, int64_t B, void* stream) {
  if (!bp || (B > 0 && (!d_synd || !d_corr || !d_post))) return set_err(QLDPC_EINVAL, "NULL argument");
  if (!side_soft_capable(bp))
    return set_err(QLDPC_ENOTSUP,
                   "soft side output needs a serial decoder created with soft = 1 or a Relay-BP decoder with num_legs = 0");
  if (d_side && !bp->side_set) return set_err(QLDPC_EINVAL, "no side priors set (qldpc_bp_set_side_probs)");
  if (B <= 0) return B < 0 ? set_err(QLDPC_EINVAL, "B < 0") : 0;
  QLDPC_HIP(hipSetDevice(bp->g->device));
  if (bp->g->n == 0) d_side = nullptr;  // no variable selects anything
  if (bp->route.engine == 7)
    return relay_decode_launch(bp, d_synd, d_corr, d_iters, d_conv, B, (hipStream_t)stream, d_side, d_post);
  return serial_decode_launch(bp, d_synd, d_corr, d_iters, d_conv, d_post, B, (hipStream_t)stream, d_side);
}

int qldpc_bp_degree3_slots(const qldpc_bp* bp, int32_t* d3k) {
  if (!bp || !d3k) return set_err(QLDPC_EINVAL, "NULL argument");
  *d3k = bp->route.engine == 3 ? bp->route.d3k : 0;
  return 0;
}

int qldpc_bp_lds_model(const qldpc_bp* bp, int64_t* out6) {
  if (!bp || !out6) return set_err(QLDPC_EINVAL, "NULL argument");
  for (int q = 0; q < 6; ++q) out6[q] = bp->lds_model[q];
  return 0;
}

int qldpc_m2s_place_model(const qldpc_graph* g, int32_t anneal_iters, int64_t* out6) {
  if (!g || !out6) return set_err(QLDPC_EINVAL, "NULL argument");
  // the decoder build of the fp64 m2s family (qldpc_bp_create), host side only: geometry, degree
  // sort, greedy + annealed V-slot placement, then the static LDS model of its variable phase
  int n3 = 0;
  for (int j = 0; j < g->n; ++j) {
    const int d = (int)g->col_rows[j].size();
    if (d != 3 && d != 4) return set_err(QLDPC_ENOTSUP, "m2s placement model: column degrees 3 / 4 only");
    n3 += d == 3;
  }
  Route r;  // the m2s route of admit_m2s at the default geometry
  r.engine = 3;
  r.tail = r.m2s = 1;
  r.nch = 3;
  if (g->max_row < 1 || g->max_row > 7 || choose_rgeometry(g->n, g->m, 0, r.TB, r.VPL) || r.TB > 256 || r.VPL < 4 ||
      r.VPL > 8 || !(n3 % r.TB == 0 || n3 == g->n))
    return set_err(QLDPC_ENOTSUP, "graph outside the m2s envelope (rows <= 7, <= 256 threads x 4-8 slots)");
  std::vector<int32_t> slot_var = degree_sorted(g, {3});
  slot_var.resize((size_t)r.VPL * r.TB, -1);
  r.d3k = leading_slots(g, slot_var, r.TB, r.VPL, 3);
  const uint32_t vbase = route_layout(r, route_vslots(r, g->m), g->m).v;
  std::vector<uint32_t> edges;
  build_slot_edges(g, r, slot_var, edges, (int)(vbase / 4), {}, 1, -1, nullptr, 1, anneal_iters);
  lds_model_var_phase(edges, r, vbase, out6);
  return 0;
}

int qldpc_bp_bank_stats(const qldpc_bp* bp, int32_t* before, int32_t* after) {
  if (!bp) return set_err(QLDPC_EINVAL, "NULL decoder");
  if (before) *before = bp->gather_conf[0];
  if (after) *after = bp->gather_conf[1];
  return 0;
}

int qldpc_bp_kernel_id(const qldpc_bp* bp, int32_t* kernel_id, int32_t* row_chunks) {
  if (!bp) return set_err(QLDPC_EINVAL, "NULL decoder");
  if (kernel_id) *kernel_id = route_kernel_id(bp->route);
  if (row_chunks) *row_chunks = bp->route.nch;
  return 0;
}

int qldpc_bp_engine(const qldpc_bp* bp, int32_t* engine) {
  if (!bp || !engine) return set_err(QLDPC_EINVAL, "NULL argument");
  *engine = bp->route.engine;
  return 0;
}

int qldpc_bp_geometry(const qldpc_bp* bp, int32_t* threads, int32_t* vpl, int32_t* lds_bytes,
                      int32_t* blocks_per_cu) {
  if (!bp) return set_err(QLDPC_EINVAL, "NULL decoder");
  if (threads) *threads = bp->route.TB;
  if (vpl) *vpl = bp->route.VPL;
  if (lds_bytes) *lds_bytes = bp->route.lds_bytes;
  if (blocks_per_cu) *blocks_per_cu = bp->blocks_per_cu;
  return 0;
}

static SectorDev sector_of(const qldpc_bp* bp, const unsigned long long* lmask, int kw) {
  SectorDev s;
  s.vchk = static_cast<const uint32_t*>(bp->vchk.p);
  s.llr = bp->llr.p;
  s.lmask = lmask;
  s.m = bp->g->m;
  s.n = bp->g->n;
  s.kw = kw;
  s.max_iter = bp->max_iter;
  s.alpha = bp->alpha;
  return s;
}

static SSector ssector_of(const qldpc_bp* bp, const unsigned long long* lmask, int kw) {
  SSector s;
  s.edges = static_cast<const uint32_t*>(bp->vchk.p);
  s.llr = bp->llr.p;
  s.lmask = lmask;
  s.rdeg = static_cast<const uint8_t*>(bp->rdeg.p);
  s.perm = static_cast<const int32_t*>(bp->perm.p);
  s.rperm = static_cast<const int32_t*>(bp->rperm.p);
  s.d3k = bp->route.d3k;
  s.m = bp->g->m;
  s.n = bp->g->n;
  s.kw = kw;
  s.max_iter = bp->max_iter;
  s.nch = bp->route.nch;
  s.vpl = bp->route.VPL;
  s.alpha = bp->alpha;
  s.rows = nullptr;
  s.vlast = s.vnl = 0;
  s.npos = bp->npos > 0 ? bp->npos : bp->g->n;
  s.nw = bp->route.nw;
  s.live_last = bp->route.live_last;
  return s;
}

// Shots (or syndromes) per chunk of a slot kernel: enough chunks to give every
// resident workgroup work, at most kChunkMax (the LDS fail bitmaps' size).
static int chunk_for(long long count, long long grid, int ns) {
  long long c = (count + grid - 1) / grid;
  c = std::max<long long>(c, ns);
  c = std::min<long long>(c, kChunkMax);
  return (int)c;
}

static int decode_batch(qldpc_bp* bp, const uint8_t* d_synd, uint8_t* d_corr, int32_t* d_iters, uint8_t* d_conv,
                        double* d_post, int64_t B, void* stream);

int qldpc_bp_decode_batch(qldpc_bp* bp, const uint8_t* d_synd, uint8_t* d_corr, int32_t* d_iters, uint8_t* d_conv,
                          int64_t B, void* stream) {
  return decode_batch(bp, d_synd, d_corr, d_iters, d_conv, nullptr, B, stream);
}

int qldpc_bp_decode_batch_soft(qldpc_bp* bp, const uint8_t* d_synd, uint8_t* d_corr, int32_t* d_iters,
                               uint8_t* d_conv, double* d_post, int64_t B, void* stream) {
  if (!bp || (B > 0 && !d_post)) return set_err(QLDPC_EINVAL, "NULL argument");
  // engine 1 (min-sum, qldpc_bp_create_soft) or engine 5 (product-sum: any qldpc_bp_create decoder with
  // bp_method 0 writes ldpc's log_prob_ratios on request)
  if (bp->route.engine != 1 && bp->route.engine != 5 && !(bp->route.engine == 8 && bp->sr_soft))
    return set_err(QLDPC_ENOTSUP, "soft output needs a decoder from qldpc_bp_create_soft (min-sum), a product-sum decoder or a serial decoder created with soft = 1");
  return decode_batch(bp, d_synd, d_corr, d_iters, d_conv, d_post, B, stream);
}

static int decode_batch(qldpc_bp* bp, const uint8_t* d_synd, uint8_t* d_corr, int32_t* d_iters, uint8_t* d_conv,
                        double* d_post, int64_t B, void* stream) {
  if (!bp || (B > 0 && (!d_synd || !d_corr))) return set_err(QLDPC_EINVAL, "NULL argument");
  if (B == 0) return 0;
  QLDPC_HIP(hipSetDevice(bp->g->device));
  // max_iter = 1 min-sum (the circuit loop's h1 rounds: max_iter = int(18 / 10)): a one-iteration BP
  // from fresh state is the first-min step kernel (per-edge magnitudes fixed by the priors, bit-exact
  // with every engine); QLDPC_BP1=0 keeps the engine
  // (built with the decoder and on every qldpc_bp_set_channel_probs, bp1_prepare: no uploads here)
  if (!d_post && bp->bp1) return qldpc_rt::bp1_decode(bp->bp1, d_synd, d_corr, d_iters, d_conv, B, (hipStream_t)stream);
  if (bp->route.engine == 5) return ps_decode_launch(bp, d_synd, d_corr, d_iters, d_conv, B, (hipStream_t)stream, d_post);
  if (bp->route.engine == 6) return hbm_decode_launch(bp, d_synd, d_corr, d_iters, d_conv, B, (hipStream_t)stream);
  if (bp->route.engine == 7) return relay_decode_launch(bp, d_synd, d_corr, d_iters, d_conv, B, (hipStream_t)stream);
  if (bp->route.engine == 8) return serial_decode_launch(bp, d_synd, d_corr, d_iters, d_conv, d_post, B, (hipStream_t)stream);
  const long long cap = (long long)bp->blocks_per_cu * bp->cus;
  if (bp->route.engine == 1) {
    DecArgs a;
    a.sec = sector_of(bp, nullptr, 0);
    a.synd = d_synd;
    a.corr = d_corr;
    a.iters = d_iters;
    a.conv = d_conv;
    a.post = d_post;
    a.B = B;
    const int grid = (int)std::max<long long>(1, std::min<long long>(B, cap));
    Variant v = get_variant(bp->route.precision, bp->route.VPL, bp->route.DMAX);
    QLDPC_HIP(v.dec(dim3(grid), dim3(bp->route.TB), bp->route.lds_bytes, (hipStream_t)stream, a));
  } else {
    const int tsize = bp->route.precision == 32 ? 4 : 8;
    SDecArgs a;
    a.sec = ssector_of(bp, nullptr, 0);
    a.synd = d_synd;
    a.corr = d_corr;
    a.iters = d_iters;
    a.conv = d_conv;
    a.B = B;
    a.mmax = bp->g->m;
    a.vslots = route_vslots(bp->route, bp->g->m);
    a.img_bytes = (int)slot_img_bytes(a.vslots, a.mmax, tsize);
    a.chunk = chunk_for(B, cap, bp->route.NS);
    a.work = nullptr;
#if QLDPC_STAMPS
    a.stamps = debug_stamps_buffer();
#else
    a.stamps = nullptr;
#endif
    if (bp->route.engine >= 3 && env_int("QLDPC_DYN", 1) != 0) {  // chunk queue, ~64 chunks per workgroup
      if (!bp->work.p && bp->work.alloc(16)) return QLDPC_ENOMEM;
      // at most kMaxQueuePops pops of the one queue counter per launch: small graphs run many
      // workgroups per CU and decode a syndrome in microseconds, and 65,536 one-syndrome pops of one
      // address serialised at ~12 ns each (0.8 ms per launch whatever max_iter; round 5 probe,
      // tools/dev/probe_small_dec.py)
      constexpr long long kMaxQueuePops = 8192;
      a.chunk = (int)std::max<long long>(1, std::min<long long>(kChunkMax, B / (cap * std::max(1, env_int("QLDPC_DYN_PER", 64)))));
      a.chunk = (int)std::min<long long>(kChunkMax, std::max<long long>(a.chunk, (B + kMaxQueuePops - 1) / kMaxQueuePops));
      QLDPC_HIP(hipMemsetAsync(bp->work.p, 0, 4, (hipStream_t)stream));
      a.work = static_cast<unsigned int*>(bp->work.p);
    }
    const long long nchunks = (B + a.chunk - 1) / a.chunk;
    const int grid = (int)std::max<long long>(1, std::min<long long>(nchunks, cap));
    SVariant v = slot_variant(bp->route);
    QLDPC_HIP(v.dec(dim3(grid), dim3(bp->route.TB), bp->route.lds_bytes, (hipStream_t)stream, a));
  }
  return 0;
}

static int build_lmask(const qldpc_graph* L, int n, DevBuf& buf, int& kw) {
  if (!L) {
    kw = 0;
    return 0;
  }
  if (L->n != n) return set_err(QLDPC_EINVAL, "logical operator width != code length");
  kw = (L->m + 63) / 64;
  if (kw > 4) return set_err(QLDPC_ENOTSUP, "more than 256 logical operators");
  if (kw == 0) kw = 1;
  std::vector<unsigned long long> mask((size_t)n * kw, 0ull);
  for (int r = 0; r < L->m; ++r)
    for (int e = L->row_ptr[r]; e < L->row_ptr[r + 1]; ++e)
      mask[(size_t)L->col_idx[e] * kw + r / 64] |= 1ull << (r % 64);
  int rc = buf.alloc(mask.size() * 8);
  if (rc) return rc;
  QLDPC_HIP(hipMemcpy(buf.p, mask.data(), mask.size() * 8, hipMemcpyHostToDevice));
  return 0;
}

// staged pipeline around decode_batch (staged.hip): any decoder pair
static int mc_create_staged(qldpc_bp* dec_x, const qldpc_graph* logical_x, qldpc_bp* dec_z,
                            const qldpc_graph* logical_z, qldpc_mc** out) {
  qldpc_bp* d0 = dec_x ? dec_x : dec_z;
  if (dec_x && dec_z && (dec_x->g->n != dec_z->g->n || dec_x->g->device != dec_z->g->device))
    return set_err(QLDPC_EINVAL, "sector decoders differ in code length or device");
  QLDPC_HIP(hipSetDevice(d0->g->device));
  auto* mc = new qldpc_mc();
  mc->dec[0] = dec_x;
  mc->dec[1] = dec_z;
  mc->route = d0->route;
  int rc = mc->counters.alloc(sizeof(qldpc_counters));
  if (!rc) rc = staged_mc_prepare(mc, logical_x, logical_z);
  if (rc) {
    staged_mc_release(mc);
    mc->counters.release();
    delete mc;
    return rc;
  }
  *out = mc;
  return 0;
}

int qldpc_mc_create_staged(qldpc_bp* dec_x, const qldpc_graph* logical_x, qldpc_bp* dec_z,
                           const qldpc_graph* logical_z, qldpc_mc** out) {
  if (!out || (!dec_x && !dec_z)) return set_err(QLDPC_EINVAL, "need at least one sector decoder");
  return mc_create_staged(dec_x, logical_x, dec_z, logical_z, out);
}

int qldpc_mc_create(qldpc_bp* dec_x, const qldpc_graph* logical_x, qldpc_bp* dec_z, const qldpc_graph* logical_z,
                    qldpc_mc** out) {
  if (!out || (!dec_x && !dec_z)) return set_err(QLDPC_EINVAL, "need at least one sector decoder");
  qldpc_bp* d0 = dec_x ? dec_x : dec_z;
  const bool staged = (dec_x && dec_x->route.engine >= 5) || (dec_z && dec_z->route.engine >= 5) ||
                      // (the space-time tail families, two-word or one-word: decode_batch kernels only)
                      (dec_x && dec_x->route.tail && (!dec_x->route.m2s || dec_x->route.nch == 4)) ||
                      (dec_z && dec_z->route.tail && (!dec_z->route.m2s || dec_z->route.nch == 4)) ||
                      // the fused kernel runs one layout family for both sectors
                      (dec_x && dec_z &&
                       (dec_x->route.m2s != dec_z->route.m2s || dec_x->route.tail != dec_z->route.tail || dec_x->route.fb != dec_z->route.fb ||
                        dec_x->route.m2s_pk != dec_z->route.m2s_pk)) ||
                      // the one-slot family (m2s) keeps no dummy edge on a real variable:
                      // the kernel's compile-time D3K must be each sector's own (a degree-3
                      // variable past it would run the 4-edge path and read the shared dummy slot)
                      (dec_x && dec_z && dec_x->route.m2s && dec_x->route.d3k != dec_z->route.d3k) ||
                      // one launch shape, variant and address scale for both sectors: sectors whose
                      // plans differ in any of them (hx and hz of unequal column degrees) decode
                      // one after the other (code length and device stay errors: mc_create_staged)
                      (dec_x && dec_z &&
                       (dec_x->route.TB != dec_z->route.TB || dec_x->route.VPL != dec_z->route.VPL ||
                        dec_x->route.DMAX != dec_z->route.DMAX || dec_x->route.precision != dec_z->route.precision ||
                        dec_x->route.engine != dec_z->route.engine || dec_x->route.ea_shift != dec_z->route.ea_shift)) ||
                      env_int("QLDPC_MC_STAGED", 0) == 1;
  if (staged) return mc_create_staged(dec_x, logical_x, dec_z, logical_z, out);
  if (dec_x && dec_z) {
    if (dec_x->g->n != dec_z->g->n) return set_err(QLDPC_EINVAL, "sector code lengths differ");
    if (dec_x->g->device != dec_z->g->device) return set_err(QLDPC_EINVAL, "sector decoders on different devices");
  }
  QLDPC_HIP(hipSetDevice(d0->g->device));
  auto* mc = new qldpc_mc();
  auto fail = [&](int code) {
    mc->lmask[0].release();
    mc->lmask[1].release();
    mc->counters.release();
    mc->work.release();
    delete mc;
    return code;
  };
  mc->dec[0] = dec_x;
  mc->dec[1] = dec_z;
  int rc = 0;
  if (dec_x && (rc = build_lmask(logical_x, dec_x->g->n, mc->lmask[0], mc->kw[0]))) return fail(rc);
  if (dec_z && (rc = build_lmask(logical_z, dec_z->g->n, mc->lmask[1], mc->kw[1]))) return fail(rc);
  // the sectors' common route: one kernel serves both
  mc->route = d0->route;
  // only slots that hold degree <= 3 variables in both sectors skip slot 4; the fused kernels have no D2K
  mc->route.d3k = std::min(dec_x ? dec_x->route.d3k : 1 << 20, dec_z ? dec_z->route.d3k : 1 << 20);
  mc->route.d2k = 0;
  // compile-time row width (fp64 <= 256-thread family)
  if (dec_x && dec_z && dec_x->route.nch != dec_z->route.nch) mc->route.nch = 0;
  mc->mmax = std::max(dec_x ? dec_x->g->m : 0, dec_z ? dec_z->g->m : 0);
  const void* kern;
  if (mc->route.engine == 1) {
    mc->route.lds_bytes = (int)lds_for(mc->route.precision, mc->mmax);
    kern = get_variant(mc->route.precision, mc->route.VPL, mc->route.DMAX).mc_k;
  } else {
    const int tsize = mc->route.precision == 32 ? 4 : 8;
    for (qldpc_bp* d : {dec_x, dec_z})
      if (d)
        mc->vslots = std::max(mc->vslots, route_vslots(d->route, d->g->m));
    mc->img_bytes = (int)slot_img_bytes(mc->vslots, mc->mmax, tsize);
    if (mc->route.engine >= 3) {
      if (!route_fits(mc->route, mc->vslots, mc->mmax)) {
        // each sector's own image fits (its decoder exists); only their common image does not
        // (no test reaches this branch: no known pair fits alone and not together)
        if (dec_x && dec_z) {
          fail(0);
          return mc_create_staged(dec_x, logical_x, dec_z, logical_z, out);
        }
        return fail(set_err(QLDPC_ENOTSUP, "sector images exceed the register engines' 64 KiB addressing (QLDPC_ENGINE=2)"));
      }
      mc->route.NS = 1;
      mc->route.lds_bytes = (int)route_lds(mc->route, mc->vslots, mc->mmax);
    } else {
      mc->route.NS = choose_ns(mc->img_bytes);
      mc->route.lds_bytes = (int)slot_lds_bytes(mc->route.NS, mc->img_bytes, kChunkMax);
    }
    kern = slot_variant(mc->route).mc_k;
  }
  if (mc->route.lds_bytes > kLdsMax) return fail(set_err(QLDPC_ENOTSUP, "per-shot LDS image exceeds 160 KiB"));
  if (!kern) return fail(set_err(QLDPC_ENOTSUP, "no kernel variant"));
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, mc->route.TB, mc->route.lds_bytes) != hipSuccess) nb = 1;
  mc->blocks_per_cu = std::max(1, nb);
  mc->cus = d0->cus;
  if ((rc = mc->counters.alloc(sizeof(qldpc_counters))) || (rc = mc->work.alloc(16))) return fail(rc);
  *out = mc;
  return 0;
}

// X/Z-correlated decoding on a staged handle: the first sector's corrections are the side bytes of
// the second sector's decode (qldpc_bp_decode_batch_side).  1 = x->z (hz decoder first), 2 = z->x.
int qldpc_mc_set_channel_update(qldpc_mc* mc, int32_t direction) {
  if (!mc) return set_err(QLDPC_EINVAL, "NULL mc");
  if (direction < 0 || direction > 2) return set_err(QLDPC_EINVAL, "direction must be 0 (off), 1 (x->z) or 2 (z->x)");
  if (!mc->staged) return set_err(QLDPC_ENOTSUP, "channel update needs a staged handle (qldpc_mc_create_staged)");
  if (mc->osd[0] || mc->osd[1]) return set_err(QLDPC_ENOTSUP, "channel update does not run with the BP+OSD stage");
  if (direction == 0) {
    mc->chan_dir = 0;
    return 0;
  }
  if (!mc->dec[0] || !mc->dec[1]) return set_err(QLDPC_EINVAL, "channel update needs both sector decoders");
  const qldpc_bp* second = mc->dec[direction == 1 ? 1 : 0];
  if (!second->side_set)
    return set_err(QLDPC_EINVAL, "channel update needs side priors on the second sector's decoder "
                                 "(qldpc_bp_set_side_probs)");
  // with a BP+OSD stage (qldpc_mc_set_staged_osd) the second sector's OSD is a side decode too
  if (qldpc_osd_gpu* so = mc->sosd[direction == 1 ? 1 : 0]; so && !osd_gpu_has_side(so))
    return set_err(QLDPC_EINVAL, "channel update needs side tables on the second sector's OSD handle "
                                 "(qldpc_osd_gpu_set_side_probs)");
  if (!mc->s_side.p) {
    QLDPC_HIP(hipSetDevice(second->g->device));
    if (int rc = mc->s_side.alloc(std::max<size_t>(1, (size_t)second->g->n * (size_t)mc->sbatch))) return rc;
  }
  mc->chan_dir = direction;
  return 0;
}

int qldpc_mc_set_osd(qldpc_mc* mc, qldpc_osd_gpu* osd_x, qldpc_osd_gpu* osd_z) {
  if (!mc) return set_err(QLDPC_EINVAL, "NULL mc");
  if (mc->chan_dir && (osd_x || osd_z))
    return set_err(QLDPC_ENOTSUP, "BP+OSD does not run on a handle with a channel update direction set");
  qldpc_osd_gpu* o[2] = {osd_x, osd_z};
  for (int q = 0; q < 2; ++q) {
    if (!o[q]) continue;
    if (mc->staged || mc->route.engine != 3)
      return set_err(QLDPC_ENOTSUP, "BP+OSD shot loop needs the fused engine-3 MC kernel");
    if (!mc->dec[q] || !osd_gpu_matches(o[q], mc->dec[q]->g))
      return set_err(QLDPC_EINVAL, q == 0 ? "X-sector OSD handle was built on a different graph than dec_x"
                                          : "Z-sector OSD handle was built on a different graph than dec_z");
  }
  mc->osd[0] = osd_x;
  mc->osd[1] = osd_z;
  mc->c_cap = 0;  // the next launch (re)allocates the capture buffers of every enabled sector
  return 0;
}

// BP+OSD in the staged shot loop: per sector, BP with soft output (qldpc_bp_decode_batch_side_soft),
// then the GPU OSD over the batch with BP's conv flags; outw is the sector's correction.
int qldpc_mc_set_staged_osd(qldpc_mc* mc, qldpc_osd_gpu* osd_x, qldpc_osd_gpu* osd_z) {
  if (!mc) return set_err(QLDPC_EINVAL, "NULL mc");
  if (!mc->staged) return set_err(QLDPC_ENOTSUP, "the staged BP+OSD stage needs a staged handle (qldpc_mc_create_staged)");
  qldpc_osd_gpu* o[2] = {osd_x, osd_z};
  for (int q = 0; q < 2; ++q) {
    if (!o[q]) continue;
    if (!mc->dec[q] || !osd_gpu_matches(o[q], mc->dec[q]->g))
      return set_err(QLDPC_EINVAL, q == 0 ? "X-sector OSD handle was built on a different graph than dec_x"
                                          : "Z-sector OSD handle was built on a different graph than dec_z");
    if (!side_soft_capable(mc->dec[q]))
      return set_err(QLDPC_ENOTSUP, "the staged BP+OSD stage needs soft output of the sector decoder: a serial "
                                    "decoder created with soft = 1 or a Relay-BP decoder with num_legs = 0");
  }
  if (mc->chan_dir)
    if (qldpc_osd_gpu* so = o[mc->chan_dir == 1 ? 1 : 0]; so && !osd_gpu_has_side(so))
      return set_err(QLDPC_EINVAL, "channel update needs side tables on the second sector's OSD handle "
                                   "(qldpc_osd_gpu_set_side_probs)");
  if (osd_x || osd_z) {
    const qldpc_bp* d0 = mc->dec[0] ? mc->dec[0] : mc->dec[1];
    const long long n = std::max(1, d0->g->n);
    // the posterior buffer [batch][n] doubles within QLDPC_OSD_CAPTURE_MB: the batch only ever shrinks
    // (every per-batch buffer of the handle was cut for a batch at least this large), and shot keying
    // does not depend on it
    // (read as a real number here: a fraction of a megabyte bounds the batch of a small code)
    const char* e = std::getenv("QLDPC_OSD_CAPTURE_MB");
    const double mb = e && std::atof(e) > 0.0 ? std::min(std::atof(e), 1048576.0) : 2048.0;
    const long long fit = std::max<long long>(64, (long long)(mb * 1048576.0) / (n * 8) / 64 * 64);
    const long long B = std::min(mc->sbatch, fit);
    QLDPC_HIP(hipSetDevice(d0->g->device));
    if (mc->s_post.bytes < (size_t)B * n * 8) {
      QLDPC_HIP(hipDeviceSynchronize());
      mc->s_post.release();
      mc->s_bpcorr.release();
      if (int rc = mc->s_post.alloc((size_t)B * n * 8)) return rc;
      if (int rc = mc->s_bpcorr.alloc((size_t)B * n)) return rc;
    }
    mc->sbatch = B;
  }
  mc->sosd[0] = osd_x;
  mc->sosd[1] = osd_z;
  return 0;
}

int qldpc_mc_destroy(qldpc_mc* mc) {
  if (!mc) return 0;
  for (int q = 0; q < 2; ++q)
    for (DevBuf* d : {&mc->c_post[q], &mc->c_synd[q], &mc->c_err[q], &mc->c_shot[q], &mc->c_outw[q]}) d->release();
  mc->c_n.release();
  mc->c_fail.release();
  mc->lmask[0].release();
  mc->lmask[1].release();
  mc->counters.release();
  mc->work.release();
  mc->cls_cache.release();
  staged_mc_release(mc);
  delete mc;
  return 0;
}

static unsigned long long ceil_2p53(double t) {
  if (!(t > 0.0)) return 0ull;
  if (t >= 1.0) return 1ull << 53;
  return (unsigned long long)std::ceil(std::ldexp(t, 53));
}

int qldpc_mc_launch(qldpc_mc* mc, double px, double py, double pz, uint64_t seed, uint64_t shot_begin,
                    int64_t shot_count, int32_t logical_mode, const double* d_uniforms, void* d_counters,
                    uint8_t* d_fail, uint8_t* d_err, uint8_t* d_corr, int32_t* d_iters, int32_t grid_blocks,
                    void* stream) {
  if (!mc || !d_counters) return set_err(QLDPC_EINVAL, "NULL argument");
  if (logical_mode < 0 || logical_mode > 2) return set_err(QLDPC_EINVAL, "logical_mode must be 0 (X), 1 (Z), 2 (Total)");
  if (!(px >= 0 && py >= 0 && pz >= 0)) return set_err(QLDPC_EINVAL, "negative Pauli probability");
  if (shot_count <= 0) return 0;
  const bool need[2] = {logical_mode != 1, logical_mode != 0};
  for (int q = 0; q < 2; ++q) {
    if (!need[q]) continue;
    if (!mc->dec[q]) return set_err(QLDPC_EINVAL, q == 0 ? "logical_mode needs the X sector (hz decoder)"
                                                          : "logical_mode needs the Z sector (hx decoder)");
    if (!mc->staged && !mc->lmask[q].p) return set_err(QLDPC_EINVAL, "sector has no logical operators");
  }
  if (mc->staged) {
    QLDPC_HIP(hipSetDevice((mc->dec[0] ? mc->dec[0] : mc->dec[1])->g->device));
    return staged_mc_launch(mc, px, py, pz, seed, shot_begin, shot_count, logical_mode, d_uniforms, d_counters, d_fail,
                            d_err, d_corr, d_iters, (hipStream_t)stream);
  }
  QLDPC_HIP(hipSetDevice((mc->dec[0] ? mc->dec[0] : mc->dec[1])->g->device));
  const bool bposd = mc->route.engine != 1 && ((need[0] && mc->osd[0]) || (need[1] && mc->osd[1]));
  if (bposd) {
    // capture slots per sector, bounded by a memory budget (QLDPC_OSD_CAPTURE_MB per sector,
    // default 2048); a launch larger than that runs as pieces of at most c_cap shots, each
    // shot claims at most one slot per sector, so no candidate can ever be dropped
    long long slot_bytes = 0;
    for (int q = 0; q < 2; ++q)
      if (need[q] && mc->osd[q]) {
        const long long n = mc->dec[q]->g->n, m = mc->dec[q]->g->m;
        slot_bytes = std::max(slot_bytes, n * 8 + m + n + 8 + n);
      }
    const long long budget = (long long)std::max(1, env_int("QLDPC_OSD_CAPTURE_MB", 2048)) << 20;
    const long long slots = std::max<long long>(1024, budget / slot_bytes);
    if (shot_count > slots) {
      const long long n = (mc->dec[0] ? mc->dec[0] : mc->dec[1])->g->n;
      for (long long off = 0; off < shot_count; off += slots) {
        const long long c = std::min(slots, shot_count - off);
        int rc = qldpc_mc_launch(mc, px, py, pz, seed, shot_begin + (uint64_t)off, c, logical_mode,
                                 d_uniforms ? d_uniforms + off * n : nullptr, d_counters, d_fail ? d_fail + off : nullptr,
                                 d_err ? d_err + off * n : nullptr, d_corr ? d_corr + off * 2 * n : nullptr,
                                 d_iters ? d_iters + off * 2 : nullptr, grid_blocks, stream);
        if (rc) return rc;
      }
      return 0;
    }
  }
  const long long cap = (long long)mc->blocks_per_cu * mc->cus;
  // thresholds of the 3-way split, in the evaluation order of src/Simulators.py:102-108
  const double t1 = pz, t2 = pz + px, t3 = (pz + px) + py;
  if (mc->route.engine == 1) {
    McArgs a;
    std::memset(&a, 0, sizeof(a));
    for (int q = 0; q < 2; ++q) {
      if (!need[q]) continue;
      a.sec[a.nsec] = sector_of(mc->dec[q], static_cast<const unsigned long long*>(mc->lmask[q].p), mc->kw[q]);
      a.sec_id[a.nsec++] = q;
    }
    a.logical_mode = logical_mode;
    a.mmax = mc->mmax;
    a.t1 = t1; a.t2 = t2; a.t3 = t3;
    a.K1 = ceil_2p53(t1); a.K2 = ceil_2p53(t2); a.K3 = ceil_2p53(t3);
    a.seed = seed; a.shot_begin = shot_begin; a.shot_count = shot_count;
    a.uniforms = d_uniforms;
    a.counters = static_cast<unsigned long long*>(d_counters);
    a.fail = d_fail; a.err = d_err; a.corr = d_corr; a.iters = d_iters;
    long long grid = grid_blocks > 0 ? grid_blocks : cap;
    grid = std::max<long long>(1, std::min<long long>(grid, shot_count));
    Variant v = get_variant(mc->route.precision, mc->route.VPL, mc->route.DMAX);
    QLDPC_HIP(v.mc(dim3((unsigned)grid), dim3(mc->route.TB), mc->route.lds_bytes, (hipStream_t)stream, a));
  } else {
    SMcArgs a;
    std::memset(&a, 0, sizeof(a));
    int ids[2] = {0, 0};
    for (int q = 0; q < 2; ++q) {
      if (!need[q]) continue;
      a.sec[a.nsec] = ssector_of(mc->dec[q], static_cast<const unsigned long long*>(mc->lmask[q].p), mc->kw[q]);
      ids[a.nsec++] = q;
    }
    a.sec_id0 = ids[0];
    a.sec_id1 = ids[1];
    a.logical_mode = logical_mode;
    a.mmax = mc->mmax;
    a.vslots = mc->vslots;
    a.img_bytes = mc->img_bytes;
    const long long want = grid_blocks > 0 ? grid_blocks : cap;
    a.chunk = chunk_for(shot_count, want, mc->route.NS);
    // engine 3: chunks from a queue, ~64 per workgroup (no tail behind the slowest static share)
    if (mc->route.engine >= 3 && mc->work.p && env_int("QLDPC_DYN", 1) != 0) {
      const int per = std::max(1, env_int("QLDPC_DYN_PER", 64));  // measured plateau 64-128 (n1600)
      a.chunk = (int)std::max<long long>(1, std::min<long long>(kChunkMax, shot_count / (want * per)));
      QLDPC_HIP(hipMemsetAsync(mc->work.p, 0, 4, (hipStream_t)stream));
      a.work = static_cast<unsigned int*>(mc->work.p);
    }
    a.t1 = t1; a.t2 = t2; a.t3 = t3;
    a.K1 = ceil_2p53(t1); a.K2 = ceil_2p53(t2); a.K3 = ceil_2p53(t3);
    a.seed = seed; a.shot_begin = shot_begin; a.shot_count = shot_count;
    a.uniforms = d_uniforms;
    a.counters = static_cast<unsigned long long*>(d_counters);
    a.fail = d_fail; a.err = d_err; a.corr = d_corr; a.iters = d_iters;
#if QLDPC_STAMPS
    a.stamps = debug_stamps_buffer();
#endif
    const long long nchunks = (shot_count + a.chunk - 1) / a.chunk;
    if (nchunks > 0x7fffffffLL) return set_err(QLDPC_EINVAL, "too many shots for one launch (chunk count >= 2^31)");
    const long long grid = std::max<long long>(1, std::min<long long>(nchunks, want));
    // both sectors drawing Philox errors: the first sector's pass caches each shot's classes for the
    // second (SMcArgs::cls_cache; [grid][chunk][TB] u16, one Philox draw per (shot, variable) instead of
    // two; QLDPC_CLS_CACHE=0 draws in both passes)
    // The cache is keyed by (thread, variable slot): the second sector reads a word back as the
    // classes of its own slots' variables, so both sectors must hold the same variable in every
    // slot.  The degree sort gives hx and hz different slot maps whenever their columns of degree
    // <= 3 sit at different positions; such a pair draws in both passes.
    a.cls_cache = nullptr;
    const size_t cc_need = (size_t)grid * (size_t)a.chunk * (size_t)mc->route.TB * 2;
    const bool same_slots = a.nsec == 2 && mc->dec[0]->slot_var == mc->dec[1]->slot_var;
    // (bounded: 256 MiB covers every bundled code at the bench's launch sizes; huge launches of small
    // codes, e.g. 10^9 shots of GenBicycleA1 at 1024-shot chunks, would need ~0.7 GB: they draw twice)
    if (same_slots && !d_uniforms && mc->route.VPL <= 8 && env_int("QLDPC_CLS_CACHE", 1) != 0 && cc_need <= (256u << 20)) {
      const size_t need = cc_need;
      if (mc->cls_cache.bytes < need) {
        mc->cls_cache.release();
        int rc = mc->cls_cache.alloc(need);
        if (rc) return rc;
      }
      a.cls_cache = static_cast<uint16_t*>(mc->cls_cache.p);
    }
    // BP+OSD: capture buffers with one slot per shot of this launch (<= the budgeted slots)
    hipStream_t st = (hipStream_t)stream;
    if (bposd) {
      if (mc->c_cap < shot_count) {
        for (int q = 0; q < 2; ++q) {
          for (DevBuf* d : {&mc->c_post[q], &mc->c_synd[q], &mc->c_err[q], &mc->c_shot[q], &mc->c_outw[q]}) d->release();
          if (!mc->dec[q] || !mc->osd[q]) continue;
          const int n = mc->dec[q]->g->n, m = mc->dec[q]->g->m;
          int rc;
          if ((rc = mc->c_post[q].alloc((size_t)shot_count * n * 8)) || (rc = mc->c_synd[q].alloc((size_t)shot_count * m)) ||
              (rc = mc->c_err[q].alloc((size_t)shot_count * n)) || (rc = mc->c_shot[q].alloc((size_t)shot_count * 8)) ||
              (rc = mc->c_outw[q].alloc((size_t)shot_count * n)))
            return rc;
        }
        mc->c_fail.release();
        int rc;
        if ((rc = mc->c_fail.alloc((size_t)shot_count)) || (!mc->c_n.p && (rc = mc->c_n.alloc(16)))) return rc;
        mc->c_cap = shot_count;
      }
      QLDPC_HIP(hipMemsetAsync(mc->c_n.p, 0, 16, st));
      a.c_n = static_cast<unsigned int*>(mc->c_n.p);
      a.c_cap = shot_count;
      for (int q = 0; q < 2; ++q) {
        const bool on = need[q] && mc->osd[q];
        a.c_post[q] = on ? static_cast<double*>(mc->c_post[q].p) : nullptr;
        a.c_synd[q] = on ? static_cast<uint8_t*>(mc->c_synd[q].p) : nullptr;
        a.c_err[q] = on ? static_cast<uint8_t*>(mc->c_err[q].p) : nullptr;
        a.c_shot[q] = on ? static_cast<long long*>(mc->c_shot[q].p) : nullptr;
      }
      if (!a.fail) a.fail = static_cast<uint8_t*>(mc->c_fail.p);  // per-shot verdicts the OSD stage revises
    }
    SVariant v = slot_variant(mc->route);
    QLDPC_HIP(v.mc(dim3((unsigned)grid), dim3(mc->route.TB), mc->route.lds_bytes, st, a));
    if (bposd) {
      unsigned int nc[4] = {0, 0, 0, 0};
      QLDPC_HIP(hipMemcpyAsync(nc, mc->c_n.p, 16, hipMemcpyDeviceToHost, st));
      QLDPC_HIP(hipStreamSynchronize(st));
      for (int q = 0; q < 2; ++q) {
        if (!(need[q] && mc->osd[q]) || nc[q] == 0) continue;
        if ((long long)nc[q] > a.c_cap)  // cannot happen (one slot per shot and sector): never drop silently
          return set_err(QLDPC_EINVAL, "BP+OSD capture overflow: more candidates than capture slots");
        const long long ncand = nc[q];
        int rc = osd_gpu_bposd_stage(mc->osd[q], static_cast<const uint8_t*>(mc->c_synd[q].p),
                                     static_cast<const double*>(mc->c_post[q].p), static_cast<const uint8_t*>(mc->c_err[q].p),
                                     static_cast<const long long*>(mc->c_shot[q].p), static_cast<uint8_t*>(mc->c_outw[q].p),
                                     ncand, static_cast<const unsigned long long*>(mc->lmask[q].p), mc->kw[q], q,
                                     logical_mode, a.fail, static_cast<unsigned long long*>(d_counters), st);
        if (rc) return rc;
      }
    }
  }
  return 0;
}

int qldpc_mc_launch_weight(qldpc_mc* mc, int32_t weight, double px, double py, double pz, uint64_t seed,
                           uint64_t shot_begin, int64_t shot_count, int32_t logical_mode, void* d_counters,
                           uint8_t* d_fail, uint8_t* d_err, uint8_t* d_corr, int32_t* d_iters, void* stream) {
  if (!mc || !d_counters) return set_err(QLDPC_EINVAL, "NULL argument");
  if (logical_mode < 0 || logical_mode > 2) return set_err(QLDPC_EINVAL, "logical_mode must be 0 (X), 1 (Z), 2 (Total)");
  if (!mc->staged)
    return set_err(QLDPC_ENOTSUP, "fixed-weight shots need a staged handle (qldpc_mc_create_staged)");
  if (mc->osd[0] || mc->osd[1]) return set_err(QLDPC_ENOTSUP, "fixed-weight shots do not run the BP+OSD stage");
  const qldpc_bp* d0 = mc->dec[0] ? mc->dec[0] : mc->dec[1];
  StagedWeight fw;
  fw.weight = weight;
  if (int rc = weight_thresholds(weight, d0->g->n, px, py, pz, &fw.K1, &fw.K2)) return rc;
  if (shot_count <= 0) return 0;
  const bool need[2] = {logical_mode != 1, logical_mode != 0};
  for (int q = 0; q < 2; ++q)
    if (need[q] && !mc->dec[q])
      return set_err(QLDPC_EINVAL, q == 0 ? "logical_mode needs the X sector (hz decoder)"
                                          : "logical_mode needs the Z sector (hx decoder)");
  QLDPC_HIP(hipSetDevice(d0->g->device));
  return staged_mc_launch(mc, px, py, pz, seed, shot_begin, shot_count, logical_mode, nullptr, d_counters, d_fail,
                          d_err, d_corr, d_iters, (hipStream_t)stream, &fw);
}

int qldpc_mc_run(qldpc_mc* mc, double px, double py, double pz, uint64_t seed, uint64_t shot_begin,
                 int64_t shot_count, int32_t logical_mode, qldpc_counters* out, void* stream) {
  if (!mc || !out) return set_err(QLDPC_EINVAL, "NULL argument");
  hipStream_t s = (hipStream_t)stream;
  QLDPC_HIP(hipMemsetAsync(mc->counters.p, 0, sizeof(qldpc_counters), s));
  int rc = qldpc_mc_launch(mc, px, py, pz, seed, shot_begin, shot_count, logical_mode, nullptr, mc->counters.p,
                           nullptr, nullptr, nullptr, nullptr, 0, stream);
  if (rc) return rc;
  qldpc_counters c;
  QLDPC_HIP(hipMemcpyAsync(&c, mc->counters.p, sizeof(c), hipMemcpyDeviceToHost, s));
  QLDPC_HIP(hipStreamSynchronize(s));
  out->shots += c.shots;
  out->failures += c.failures;
  for (int q = 0; q < 2; ++q) {
    out->sector_decodes[q] += c.sector_decodes[q];
    out->sector_iters[q] += c.sector_iters[q];
    out->sector_nonconv[q] += c.sector_nonconv[q];
    out->sector_fail[q] += c.sector_fail[q];
    for (int b = 0; b < QLDPC_HIST_BINS; ++b) out->iter_hist[q][b] += c.iter_hist[q][b];
  }
  return 0;
}

}  // extern "C"

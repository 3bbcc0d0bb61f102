// osd.hip — ordered-statistics post-processing (BP+OSD) of non-converged BP
// decodes: the `bposd_decoder(..., osd_method, osd_order)` the reference's
// BPOSD_Decoder wraps (src/Decoders.py:26-41; osd_method="osd_e", osd_order=10
// in every notebook).  Host code: the GPU BP decode (engine 1,
// qldpc_bp_decode_batch_soft) hands over the final posteriors, and this stage
// runs GF(2) elimination per non-converged syndrome on host threads.
//
// Algorithm (ldpc 0.1 OSD, restated; oracle/oracle.py osd_decode follows the
// same spec literally with an LU solve per candidate):
//   1. columns sorted by posterior log-probability ratio, ascending (stable);
//   2. LU-style elimination choosing, for pivot i = 0..rank-1, the first column
//      in the current order independent of the earlier pivots and SWAPPING it
//      into position i (Neal's mod2sparse_decomp with the "first" strategy) — the
//      non-pivot columns Ht = cols[rank:] inherit that swap order;
//   3. OSD-0: x_S = H_S^-1 s on the pivots, 0 elsewhere;
//   4. OSD-E: every t in {0,1}^w on Ht[0:w] (w = min(order, n-rank)), natural
//      binary order; OSD-CS: weight-1 t over all of Ht, then weight-2 t inside
//      Ht[0:w]; candidate x_S = H_S^-1 (s + H_T t); keep the first candidate of
//      strictly smaller soft weight sum_{j: x_j=1} log(1/p_j) (ascending j).
// Linear algebra: pivot columns are found by xor-basis insertion on m-bit
// column vectors, each basis vector carrying its combination of pivots, so
// H_S^-1 g is one basis reduction; candidates use linearity,
// x(s + sum t_j h_j) = x(s) + sum t_j x(h_j), i.e. one rank-bit xor each.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <numeric>
#include <thread>
#include <utility>
#include <vector>

#include "osd_types.h"
#include "runtime.h"

using qldpc_rt::set_err;

namespace {

using u64 = unsigned long long;

inline int ctz64(u64 x) { return __builtin_ctzll(x); }

// Column vectors over rows, xor basis keyed by the lowest set row bit.
struct Basis {
  int W = 0, RW = 0;
  std::vector<int32_t> key;  // row bit -> basis slot or -1
  std::vector<u64> vec;      // [slot][W]
  std::vector<u64> comb;     // [slot][RW] pivots combined into the slot
  int count = 0;

  void init(int m, int rank) {
    W = (m + 63) / 64;
    RW = std::max(1, (rank + 63) / 64);
    key.assign(m, -1);
    vec.assign((size_t)std::max(rank, 1) * W, 0);
    comb.assign((size_t)std::max(rank, 1) * RW, 0);
    count = 0;
  }
  // Reduce v (W words) in place, accumulating the used combination into c (RW words).
  // Returns the lowest set bit left, or -1 if v reduced to zero.
  int reduce(u64* v, u64* c) const {
    for (;;) {
      int b = -1;
      for (int q = 0; q < W; ++q)
        if (v[q]) {
          b = q * 64 + ctz64(v[q]);
          break;
        }
      if (b < 0) return -1;
      const int s = key[b];
      if (s < 0) return b;
      const u64* bv = &vec[(size_t)s * W];
      const u64* bc = &comb[(size_t)s * RW];
      for (int q = b / 64; q < W; ++q) v[q] ^= bv[q];
      for (int q = 0; q < RW; ++q) c[q] ^= bc[q];
    }
  }
  // Reduce a syndrome v in place on the key rows alone, accumulating into c: a set bit no basis
  // vector is keyed by is passed over, where reduce() stops at it.  The key rows are Neal's pivot
  // rows (both take the lowest row that keeps the pivot block non-singular), so c solves the pivot
  // rows' equations exactly and ignores the others, as ldpc's LU solve does: the same as reduce()
  // for a syndrome in the column space, and the LU solve's answer for one outside it.
  void solve(u64* v, u64* c) const {
    for (int q0 = 0; q0 < W; ++q0) {
      u64 pend = v[q0];
      while (pend) {
        const int t = ctz64(pend);
        pend &= pend - 1;
        const int s = key[q0 * 64 + t];
        if (s < 0) continue;
        const u64* bv = &vec[(size_t)s * W];
        const u64* bc = &comb[(size_t)s * RW];
        for (int q = q0; q < W; ++q) v[q] ^= bv[q];
        for (int q = 0; q < RW; ++q) c[q] ^= bc[q];
        pend = v[q0] & ~((2ull << t) - 1);  // the bits above t, as the xor left them
      }
    }
  }
};

void load_col(const qldpc_osd& O, int j, u64* v, int W) {
  std::fill(v, v + W, 0ull);
  for (int r : O.col_rows[j]) v[r >> 6] ^= 1ull << (r & 63);
}

int gf2_rank(const qldpc_osd& O) {
  Basis B;
  B.init(O.m, std::min(O.m, O.n));
  std::vector<u64> v(B.W), c(B.RW);
  int rank = 0;
  for (int j = 0; j < O.n && rank < O.m; ++j) {
    load_col(O, j, v.data(), B.W);
    std::fill(c.begin(), c.end(), 0ull);
    const int b = B.reduce(v.data(), c.data());
    if (b >= 0) {
      B.key[b] = rank;
      std::copy(v.begin(), v.end(), &B.vec[(size_t)rank * B.W]);
      ++rank;
    }
  }
  return rank;
}

struct Work {
  Basis B;
  std::vector<int32_t> cols, pivpos, ht;
  std::vector<u64> v, c, xs, xh, X;
  std::vector<uint8_t> cand;
};

double soft_weight(const double* w, int n, const uint8_t* x) {
  double s = 0.0;
  for (int j = 0; j < n; ++j)
    if (x[j]) s += w[j];
  return s;
}

// Decode one non-converged syndrome; writes OSD-0 and OSD-w corrections.  sw: the syndrome's own
// weights [n] of a side decode (always the soft-weight path), or null for the handle's.
void osd_one(const qldpc_osd& O, Work& K, const uint8_t* synd, const double* post, uint8_t* out0, uint8_t* outw,
             const double* sw = nullptr) {
  const int m = O.m, n = O.n, rank = O.rank;
  const bool uniform = O.uniform && !sw;
  const double* wt = sw ? sw : O.w.data();
  K.cols.resize(n);
  std::iota(K.cols.begin(), K.cols.end(), 0);
  std::stable_sort(K.cols.begin(), K.cols.end(), [&](int a, int b) { return post[a] < post[b]; });
  Basis& B = K.B;
  B.init(m, rank);
  const int W = B.W, RW = B.RW;
  K.v.resize(W);
  K.c.resize(RW);
  // 1. greedy pivots in sorted order (positions recorded for the swap replay)
  K.pivpos.clear();
  for (int pos = 0; pos < n && (int)K.pivpos.size() < rank; ++pos) {
    load_col(O, K.cols[pos], K.v.data(), W);
    std::fill(K.c.begin(), K.c.end(), 0ull);
    const int b = B.reduce(K.v.data(), K.c.data());
    if (b < 0) continue;
    const int s = B.count++;
    B.key[b] = s;
    K.c[s >> 6] ^= 1ull << (s & 63);
    std::copy(K.v.begin(), K.v.end(), &B.vec[(size_t)s * W]);
    std::copy(K.c.begin(), K.c.end(), &B.comb[(size_t)s * RW]);
    K.pivpos.push_back(pos);
  }
  const int r = (int)K.pivpos.size();
  // 2. Neal's swap: pivot i moves to position i, the column there to its place
  for (int i = 0; i < r; ++i) std::swap(K.cols[i], K.cols[K.pivpos[i]]);
  const int k = n - r;
  K.ht.assign(K.cols.begin() + r, K.cols.end());
  // 3. OSD-0
  K.xs.assign(RW, 0ull);
  std::fill(K.v.begin(), K.v.end(), 0ull);
  for (int i = 0; i < m; ++i)
    if (synd[i] & 1u) K.v[i >> 6] ^= 1ull << (i & 63);
  B.solve(K.v.data(), K.xs.data());
  auto expand = [&](const u64* x, uint8_t* dst) {
    std::fill(dst, dst + n, (uint8_t)0);
    for (int i = 0; i < r; ++i)
      if ((x[i >> 6] >> (i & 63)) & 1ull) dst[K.cols[i]] = 1;
  };
  expand(K.xs.data(), out0);
  if (O.method == 0 || O.order == 0 || k == 0) {
    std::copy(out0, out0 + n, outw);
    return;
  }
  const int w = std::min(O.order, k);
  const int nh = O.method == 2 ? k : w;  // columns whose x(h_j) is needed
  K.xh.assign((size_t)nh * RW, 0ull);
  for (int j = 0; j < nh; ++j) {
    load_col(O, K.ht[j], K.v.data(), W);
    B.reduce(K.v.data(), &K.xh[(size_t)j * RW]);
  }
  K.cand.resize(n);
  // weight of OSD-0; candidates must be strictly lighter
  long long best_cnt = 0;
  double best_w = 0.0;
  if (uniform) {
    for (int q = 0; q < RW; ++q) best_cnt += __builtin_popcountll(K.xs[q]);
  } else {
    best_w = soft_weight(wt, n, out0);
  }
  std::copy(out0, out0 + n, outw);
  // candidate: x = xs ^ (xor of xh over t's bits); t bits are Ht positions
  auto consider = [&](const u64* x, const int* tj, int nt) {
    if (uniform) {
      long long cnt = nt;
      for (int q = 0; q < RW; ++q) cnt += __builtin_popcountll(x[q]);
      if (cnt >= best_cnt) return;
      best_cnt = cnt;
      expand(x, outw);
      for (int a = 0; a < nt; ++a) outw[K.ht[tj[a]]] = 1;
    } else {
      expand(x, K.cand.data());
      for (int a = 0; a < nt; ++a) K.cand[K.ht[tj[a]]] = 1;
      const double cw = soft_weight(wt, n, K.cand.data());
      if (cw >= best_w) return;
      best_w = cw;
      std::copy(K.cand.begin(), K.cand.end(), outw);
    }
  };
  std::vector<u64> tmp(RW);
  if (O.method == 1) {  // osd_e: all 2^w inputs, natural order (l = 0 is OSD-0 itself)
    const long long L = 1ll << w;
    K.X.assign((size_t)L * RW, 0ull);
    std::copy(K.xs.begin(), K.xs.end(), K.X.begin());
    int tj[64];
    for (long long l = 1; l < L; ++l) {
      const u64* prev = &K.X[(size_t)(l & (l - 1)) * RW];
      const u64* h = &K.xh[(size_t)ctz64((u64)l) * RW];
      u64* cur = &K.X[(size_t)l * RW];
      for (int q = 0; q < RW; ++q) cur[q] = prev[q] ^ h[q];
      int nt = 0;
      for (u64 b = (u64)l; b; b &= b - 1) tj[nt++] = ctz64(b);
      consider(cur, tj, nt);
    }
  } else {  // osd_cs: weight-1 over all of Ht, then weight-2 pairs inside Ht[0:w]
    for (int j = 0; j < k; ++j) {
      for (int q = 0; q < RW; ++q) tmp[q] = K.xs[q] ^ K.xh[(size_t)j * RW + q];
      consider(tmp.data(), &j, 1);
    }
    for (int i = 0; i < w; ++i)
      for (int j = i + 1; j < w; ++j) {
        for (int q = 0; q < RW; ++q) tmp[q] = K.xs[q] ^ K.xh[(size_t)i * RW + q] ^ K.xh[(size_t)j * RW + q];
        const int tj[2] = {i, j};
        consider(tmp.data(), tj, 2);
      }
  }
}

// w_s = log(1 / p_s) of a side table, as qldpc_osd_create computes w; false on an entry outside (0, 1)
bool side_weights(const double* p, int n, std::vector<double>& w) {
  w.resize(n);
  for (int j = 0; j < n; ++j) {
    if (!(p[j] > 0.0 && p[j] < 1.0)) return false;
    w[j] = std::log(1.0 / p[j]);
  }
  return true;
}

int osd_decode_batch_impl(const qldpc_osd* osd, const uint8_t* synd, const double* post, const uint8_t* conv,
                          const uint8_t* bp_corr, const uint8_t* side, uint8_t* out_osd0, uint8_t* out_osdw,
                          int64_t B, int32_t threads);

}  // namespace

extern "C" {

int qldpc_osd_create(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                     const double* channel_probs, int32_t osd_method, int32_t osd_order, qldpc_osd** out) {
  if (!row_ptr || !channel_probs || !out) return set_err(QLDPC_EINVAL, "NULL argument");
  if (m < 0 || n <= 0) return set_err(QLDPC_EINVAL, "bad matrix shape");
  // (a matrix without entries has no column indices: qldpc_osd_gpu_create hands over an empty vector's data())
  if (!col_idx && row_ptr[m] > 0) return set_err(QLDPC_EINVAL, "NULL argument");
  if (osd_method < 0 || osd_method > 2) return set_err(QLDPC_EINVAL, "osd_method must be 0 (osd_0), 1 (osd_e) or 2 (osd_cs)");
  if (osd_order < 0 || (osd_method == 1 && osd_order > 20))
    return set_err(QLDPC_EINVAL, "osd_order must be >= 0 (and <= 20 for osd_e)");
  auto* O = new qldpc_osd();
  O->m = m;
  O->n = n;
  O->method = osd_method;
  O->order = osd_order;
  O->col_rows.assign(n, {});
  for (int i = 0; i < m; ++i)
    for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
      const int j = col_idx[e];
      if (j < 0 || j >= n) {
        delete O;
        return set_err(QLDPC_EINVAL, "column index out of range");
      }
      O->col_rows[j].push_back(i);
    }
  O->w.resize(n);
  for (int j = 0; j < n; ++j) {
    if (!(channel_probs[j] > 0.0 && channel_probs[j] < 1.0)) {
      delete O;
      return set_err(QLDPC_EINVAL, "channel_probs must lie in (0, 1)");
    }
    O->w[j] = std::log(1.0 / channel_probs[j]);
    if (O->w[j] != O->w[0]) O->uniform = false;
  }
  O->rank = gf2_rank(*O);
  *out = O;
  return 0;
}

int qldpc_osd_destroy(qldpc_osd* osd) {
  delete osd;
  return 0;
}

int qldpc_osd_rank(const qldpc_osd* osd, int32_t* rank) {
  if (!osd || !rank) return set_err(QLDPC_EINVAL, "NULL argument");
  *rank = osd->rank;
  return 0;
}

int qldpc_osd_set_side_probs(qldpc_osd* osd, const double* p0, const double* p1) {
  if (!osd || !p0 || !p1) return set_err(QLDPC_EINVAL, "NULL argument");
  if (osd->lsd_k && osd->lsd_w > 0)
    return set_err(QLDPC_ENOTSUP, "LSD of order > 0 has no side decode (its candidates are weighed by the handle's priors)");
  std::vector<double> w0, w1;
  if (!side_weights(p0, osd->n, w0) || !side_weights(p1, osd->n, w1))
    return set_err(QLDPC_EINVAL, "side probabilities must lie in (0, 1)");
  osd->ws0.swap(w0);
  osd->ws1.swap(w1);
  return 0;
}

int qldpc_osd_decode_batch(const qldpc_osd* osd, const uint8_t* synd, const double* post, const uint8_t* conv,
                           const uint8_t* bp_corr, uint8_t* out_osd0, uint8_t* out_osdw, int64_t B,
                           int32_t threads) {
  return osd_decode_batch_impl(osd, synd, post, conv, bp_corr, nullptr, out_osd0, out_osdw, B, threads);
}

int qldpc_osd_decode_batch_side(const qldpc_osd* osd, const uint8_t* synd, const double* post, const uint8_t* conv,
                                const uint8_t* bp_corr, const uint8_t* side, uint8_t* out_osd0, uint8_t* out_osdw,
                                int64_t B, int32_t threads) {
  if (!osd || (B > 0 && !side)) return set_err(QLDPC_EINVAL, "NULL argument");
  if (osd->ws0.empty()) return set_err(QLDPC_EINVAL, "side decode without side tables (qldpc_osd_set_side_probs)");
  return osd_decode_batch_impl(osd, synd, post, conv, bp_corr, side, out_osd0, out_osdw, B, threads);
}

}  // extern "C"

namespace {
int osd_decode_batch_impl(const qldpc_osd* osd, const uint8_t* synd, const double* post, const uint8_t* conv,
                          const uint8_t* bp_corr, const uint8_t* side, uint8_t* out_osd0, uint8_t* out_osdw,
                          int64_t B, int32_t threads) {
  if (!osd || (B > 0 && (!synd || !post || !out_osdw))) return set_err(QLDPC_EINVAL, "NULL argument");
  if (conv && !bp_corr) return set_err(QLDPC_EINVAL, "conv needs bp_corr");
  if (B <= 0) return 0;
  // an LSD stage (qldpc_osd_create_lsd) weighs no candidates: its side decode is its plain decode
  if (osd->lsd_k)
    return qldpc_rt::lsd_decode_batch_host(osd, synd, post, conv, bp_corr, out_osd0, out_osdw, nullptr, B, threads);
  const int m = osd->m, n = osd->n;
  std::vector<int64_t> todo;
  for (int64_t b = 0; b < B; ++b) {
    if (conv && conv[b]) {
      std::copy(bp_corr + b * n, bp_corr + (b + 1) * n, out_osdw + b * n);
      if (out_osd0) std::copy(bp_corr + b * n, bp_corr + (b + 1) * n, out_osd0 + b * n);
    } else {
      todo.push_back(b);
    }
  }
  int T = threads;
  if (T <= 0) {  // the process's CPU share when the launcher states it (OMP_NUM_THREADS), else all cores
    const char* e = std::getenv("OMP_NUM_THREADS");
    T = e ? std::atoi(e) : 0;
    if (T <= 0) T = (int)std::max(1u, std::thread::hardware_concurrency());
  }
  T = (int)std::min<int64_t>(T, (int64_t)todo.size());
  if (T <= 0) return 0;
  auto run = [&](int t) {
    Work K;
    std::vector<uint8_t> o0(n);
    std::vector<double> sw(side ? n : 0);
    for (size_t a = t; a < todo.size(); a += T) {
      const int64_t b = todo[a];
      if (side)
        for (int j = 0; j < n; ++j) sw[j] = (side[b * n + j] & 1u) ? osd->ws1[j] : osd->ws0[j];
      osd_one(*osd, K, synd + b * m, post + b * n, out_osd0 ? out_osd0 + b * n : o0.data(), out_osdw + b * n,
              side ? sw.data() : nullptr);
    }
  };
  if (T == 1) {
    run(0);
  } else {
    std::vector<std::thread> pool;
    for (int t = 0; t < T; ++t) pool.emplace_back(run, t);
    for (auto& th : pool) th.join();
  }
  return 0;
}
}  // namespace

// ===========================================================================
// GPU OSD: one workgroup per syndrome, persistent over the batch (uniform priors: popcount
// weights; non-uniform: soft weights summed in column order, candidate step 6').  Same algorithm and outputs as the host stage above, laid out for the
// GPU: the columns are bitonic-sorted in LDS by (posterior, index) — a stable
// ascending order — and H is loaded with its columns permuted into that order,
// word-major (word q of row i at q*m + i) in a per-workgroup HBM slice, so a
// pivot search tests one coalesced word per row and a row update xors
// coalesced words.  Full Gauss-Jordan over the positions in order finds the
// same greedy pivots (the x of an independent pivot set is unique, whatever
// pivot rows are chosen); the OSD inputs are then bit-vectors over the pivot
// index, and every candidate's weight (popcount, the order relation of the
// uniform soft weight) is reduced to the lexicographic minimum of
// (weight, candidate index) = the first strictly lightest in ldpc's order.
namespace {

constexpr int kOsdThreads = 256;      // HBM-slice image: memory-latency bound, 3 workgroups per CU
constexpr int kOsdThreadsLds = 1024;  // LDS-resident image: one workgroup per CU, 16 waves on its rows

#ifndef QLDPC_STAMPS
#define QLDPC_STAMPS 0
#endif
// diagnostic builds (QLDPC_STAMPS): per-step cycle sums of osd_gpu_kernel, wave 0 of each
// workgroup: [0] sort, [1] H load, [2] Gauss-Jordan, [3] swaps + bit-vectors, [4] candidates,
// [5] outputs, [6] syndromes, [7] positions visited, [8] of [2]: pivot searches + their barrier,
// [9] of [2] (register rows): pivot-row publication + its barrier
__device__ unsigned long long g_osd_stamps[16];
__device__ inline unsigned long long osd_stamp() {
#if QLDPC_STAMPS
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
#else
  return 0;
#endif
}
constexpr int kOsdMaxN = 8192;
constexpr uint8_t kOsdRedo = 0xFF;  // mark of the early-out behind the register-row pivot loop (never written)
// register-row mode: pivot-row words read per batch ahead of their xors
constexpr int kOsdXB = 8;

struct OsdGpuArgs {
  const int32_t* rp;
  const int32_t* ci;
  const uint8_t* synd;     // [B][m]
  const double* post;      // [B][n]
  const uint8_t* conv;     // [B] or null
  const long long* shot;   // [B] or null: fused-loop capture slots, < 0 = BP converged (skipped)
  const uint8_t* bp_corr;  // [B][n] or null
  const double* softw;     // [n] log(1 / p_j) for non-uniform priors, or null (uniform: popcount weights)
  uint8_t* out0;           // [B][n] or null
  uint8_t* outw;           // [B][n]
  u64* ws;                 // per workgroup: M [W][m] | X [(1 + nh)][RW]
  int32_t* iws;            // per workgroup: pivrow [rank] | pivpos [rank] | swp [n]
  long long B;
  int m, n, W, RW, rank, method, order, NP;
  int m_lds;  // 1: the matrix lives in LDS, aliasing the sort tables (copied out first), else in the HBM slice
  int bits_off;  // LDS byte offset of the used / syndrome bit-vectors
  int pbuf_off;  // register-row mode: LDS byte offset of the pivot-row broadcast buffer
  int win;  // always 0 (see the early-out behind the register-row pivot loop)
  long long ws_words, iws_ints;
  // side decodes (the SIDE instantiations alone read these; softw is then w_0, never null)
  const double* softw1;  // [n] w_1
  const uint8_t* side;   // [B][n], bit 0 selects the weight table per column
};

// dst[q*m] ^= src[q*m] for q < W: no aliasing between the two rows, so the loads can run ahead
// of the stores (in-place xors through one pointer would serialize word by word)
__device__ inline void row_xor(u64* __restrict__ dst, const u64* __restrict__ src, int W, int m) {
#pragma unroll 8
  for (int q = 0; q < W; ++q) dst[(size_t)q * m] ^= src[(size_t)q * m];
}

// minimum of a 32-bit value over the 64 lanes of a wave (all lanes active) in 6 DPP VALU + 1
// readlane: quad and row rotations give every lane its 16-lane row's minimum, row_bcast:15 /
// row_bcast:31 fold rows 0-1 / 2-3 / all into lane 63 (the GFX9 DPP broadcasts; the s_nops are
// the DPP read-after-VALU-write wait states)
__device__ inline uint32_t wave_min_u32_bc(uint32_t v) {
  asm volatile(
      "s_nop 1\n\t"
      "v_min_u32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_min_u32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_min_u32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_min_u32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_min_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_min_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
      "s_nop 1"
      : "+v"(v));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// v_ffbl_b32: index of the lowest set bit, 0xFFFFFFFF for 0
__device__ inline uint32_t ffbl_u32(uint32_t x) {
  uint32_t r;
  asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}

// LDS max at byte address a by the calling lanes, completed before return (plain ds_max_u32: the
// compiler's atomic optimizer would wrap a builtin atomic in a first-lane election per call)
__device__ inline void lds_max_u32_sync(uint32_t a, uint32_t v) {
  asm volatile("ds_max_u32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : : "v"(a), "v"(v) : "memory");
}

__device__ inline u64 ord_key(double x) {
  if (x == 0.0) x = 0.0;  // -0 ties +0, as std::stable_sort's `<` has it
  const u64 u = (u64)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// WR > 0: register-row mode (m <= LB, W <= WR): thread i keeps row i of the permuted H in WR
// u64 registers through the whole Gauss-Jordan; a pivot's owner publishes the pivot row's words
// q.. in an LDS buffer and the rows that have the pivot bit xor them in registers, so a row
// update costs no LDS writes (the word-major LDS / HBM image paid one 8-byte store per word and
// row).  The reduced rows go to the HBM slice afterwards for the candidate bit-vectors.
//
// SIDE: the side decode (qldpc_osd_gpu_decode_side), a compile-time switch so that the plain
// instantiations are the code they were.  Step 6' alone differs: always taken, and its weights are
// the syndrome's own, w_{side[b][j] & 1}[j], staged once per syndrome in the workgroup's slice.
template <int LB, int WR = 0, bool SIDE = false>
__global__ void __launch_bounds__(LB) osd_gpu_kernel(OsdGpuArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, TB = blockDim.x;
  const int m = A.m, n = A.n, W = A.W, RW = A.RW, NP = A.NP, rank = A.rank;
  u64* skey = reinterpret_cast<u64*>(smem);                    // [NP]
  int32_t* sidx = reinterpret_cast<int32_t*>(skey + NP);       // [NP] -> cols (sorted position -> column)
  int32_t* pos = sidx + NP;                                    // [n]  column -> sorted position
  uint32_t* used = reinterpret_cast<uint32_t*>(smem + A.bits_off);  // [ceil(m/32)]
  uint32_t* sb = used + (m + 31) / 32;                         // [ceil(m/32)] syndrome, reduced
  __shared__ int s_piv[3], s_npiv;  // s_piv triple-buffered by position: reset two columns ahead
  __shared__ uint32_t s_pivx;       // register rows: (search step << 17) | (0x1FFFF - key), max over the waves
  __shared__ u64 s_best, s_bestw;
  u64* Mg = A.ws + (size_t)blockIdx.x * A.ws_words;
  u64* X = Mg + (size_t)W * m;  // X[0] = S0, X[1 + j] = x(h_j)
  // matrix: LDS when it fits (at offset 0, over the sort tables, which are copied to the
  // workgroup's HBM ints first), else the per-workgroup HBM slice
  // (compile-time per instantiation, so the accesses are ds_* or global_*, never flat)
  constexpr bool kRR = WR > 0;
  constexpr bool kMLds = !kRR && LB == kOsdThreadsLds;
  u64* M = kMLds ? reinterpret_cast<u64*>(smem) : Mg;  // register-row mode: Mg holds the reduced rows
  int32_t* pivrow = A.iws + (size_t)blockIdx.x * A.iws_ints;
  int32_t* pivpos = pivrow + rank;
  int32_t* swp = pivpos + rank;
  int32_t* gsidx = swp + n;   // [n] LDS mode: sorted position -> column
  int32_t* gpos = gsidx + n;  // [n] LDS mode: column -> sorted position
  const int32_t* sidxr = kMLds ? gsidx : sidx;
  const int k = n - rank;
  const int w = A.order < k ? A.order : k;
  const int nh = A.method == 2 ? k : w;

  unsigned long long st[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long t0 = osd_stamp(), t1;
#define OSD_ST(k)              \
  if (QLDPC_STAMPS) {          \
    t1 = osd_stamp();          \
    st[k] += t1 - t0;          \
    t0 = t1;                   \
  }
  for (long long b = blockIdx.x; b < A.B; b += gridDim.x) {
    uint8_t* ow = A.outw + b * (long long)n;
    uint8_t* o0 = A.out0 ? A.out0 + b * (long long)n : nullptr;
    if (A.shot && A.shot[b] < 0) continue;  // captured decode that converged at max_iter: no OSD
    if (A.conv && A.conv[b]) {  // BP converged: bposd_decoder returns the BP decoding
      for (int j = tid; j < n; j += TB) {
        const uint8_t v = A.bp_corr[b * (long long)n + j];
        ow[j] = v;
        if (o0) o0[j] = v;
      }
      continue;  // uniform over the workgroup
    }
    const double* post = A.post + b * (long long)n;
    const uint8_t* synd = A.synd + b * (long long)m;
    // 1. stable ascending sort of the columns by posterior (bitonic on (key, index))
    for (int q = tid; q < NP; q += TB) {
      skey[q] = q < n ? ord_key(post[q]) : ~0ull;
      sidx[q] = q < n ? q : 0x7FFFFFFF;
    }
    __syncthreads();
    for (int size = 2; size <= NP; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int q = tid; q < NP / 2; q += TB) {
          const int lo = 2 * q - (q & (stride - 1));
          const int hi = lo + stride;
          const bool up = (lo & size) == 0;
          const u64 ka = skey[lo], kb = skey[hi];
          const int ia = sidx[lo], ib = sidx[hi];
          const bool gt = ka > kb || (ka == kb && ia > ib);
          if (gt == up) {
            skey[lo] = kb; skey[hi] = ka;
            sidx[lo] = ib; sidx[hi] = ia;
          }
        }
        __syncthreads();
      }
    OSD_ST(0)
    if (kMLds) {
      for (int q = tid; q < n; q += TB) {
        const int c = sidx[q];
        gsidx[q] = c;
        gpos[c] = q;
      }
    } else {
      for (int q = tid; q < n; q += TB) pos[sidx[q]] = q;
    }
    for (int q = tid; q < (m + 31) / 32; q += TB) {
      used[q] = 0;
      uint32_t v = 0;
      for (int t = 0; t < 32 && q * 32 + t < m; ++t) v |= (uint32_t)(synd[q * 32 + t] & 1u) << t;
      sb[q] = v;
    }
    if (tid == 0) {
      s_npiv = 0;
      s_piv[0] = s_piv[1] = s_piv[2] = 0x7FFFFFFF;
      s_pivx = 0u;
    }
    __syncthreads();
    if constexpr (kRR) {
      // 2-3 (register rows): row tid of the permuted H, words by compile-time index
      u64 row[WR];
#pragma unroll
      for (int q = 0; q < WR; ++q) row[q] = 0;
      uint32_t sbit = 0;
      if (tid < m) {
        for (int e = A.rp[tid]; e < A.rp[tid + 1]; ++e) {
          const int p = pos[A.ci[e]];
          const int pq = p >> 6;
          const u64 bit = 1ull << (p & 63);
#pragma unroll
          for (int q = 0; q < WR; ++q) row[q] ^= (pq == q) ? bit : 0ull;
        }
        sbit = synd[tid] & 1u;
      }
      u64* pbuf = reinterpret_cast<u64*>(smem + A.pbuf_off);  // [WR] pivot row, [WR] its syndrome bit
      OSD_ST(1)
      int npiv = 0;   // uniform
      // Per-pivot loop.  Positions without a candidate row change nothing, so one search step finds
      // the next pivot of this word directly: the lexicographic minimum of (first set bit >= b, row)
      // over the unused rows = the first position with a candidate and its lowest row, as the
      // position-by-position greedy scan picks it (ldpc's pivot set), without a barrier per
      // dependent position.  A pivot step is bound by every wave's own instruction stream (all
      // waves meet at its two barriers; profiles/r04/passo/), so the step's winner is the maximum
      // of (step << 17) | (0x1FFFF - key) over one ds_max per wave: a stale value from an earlier
      // step never matches the step, so the slot needs no re-arming.  Pivots go to an LDS list
      // over the (dead) sort keys: (position << 11) | row.
      int32_t* lkk = reinterpret_cast<int32_t*>(smem);
      const uint32_t pivx_a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)(&s_pivx);
      uint32_t step = 0;  // uniform
      uint32_t um = tid < m ? ~0u : 0u;  // ~0 while row tid is a candidate (unused, < m), else 0
#pragma unroll
      for (int q = 0; q < WR; ++q) {
        if (q * 64 >= n || npiv >= rank) break;  // uniform
        const int bend = n - q * 64 < 64 ? n - q * 64 : 64;
        const u64 wmask = bend < 64 ? (1ull << bend) - 1ull : ~0ull;
        int b = 0;
        for (;;) {  // uniform
          ++step;
          asm volatile("" : "+s"(step));  // opaque: no strength-reduced copies of step << 17 per word
          unsigned long long ts0 = 0;
          if (QLDPC_STAMPS) {
            ts0 = osd_stamp();
            st[7] += 1;
          }
          const u64 lowm = (~0ull << b) & wmask;
          // key = (first set bit >= b << 11) | row; a row without one gets first bit 0xFFFFFFFF
          // (v_ffbl of 0), i.e. a key >= 0xFFFFF800, above every real key (<= 0x1FFFF)
          const uint32_t ml = (uint32_t)row[q] & (uint32_t)lowm & um;
          const uint32_t mh = (uint32_t)(row[q] >> 32) & (uint32_t)(lowm >> 32) & um;
          const uint32_t fl = ffbl_u32(ml), fh = ffbl_u32(mh) | 32u;
          uint32_t key = ((fl < fh ? fl : fh) << 11) | (uint32_t)tid;
          key = wave_min_u32_bc(key);
          if ((tid & 63) == 0 && key <= 0x1FFFFu) lds_max_u32_sync(pivx_a, (step << 17) | (0x1FFFFu - key));
          __syncthreads();
          if (QLDPC_STAMPS) {
            const unsigned long long t = osd_stamp();
            st[8] += t - ts0;
            ts0 = t;
          }
          const uint32_t vx = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_pivx);  // uniform
          if ((vx >> 17) != step) break;  // no pivot left in this word (uniform)
          const uint32_t kk = 0x1FFFFu - (vx & 0x1FFFFu);
          const int fb = (int)(kk >> 11), r = (int)(kk & 2047u);
          const bool hb = ((row[q] >> fb) & 1ull) != 0;
          if (tid == r) {
            um = 0u;
#pragma unroll
            for (int q2 = q; q2 < WR; ++q2) pbuf[q2] = row[q2];
            pbuf[WR] = sbit;
            lkk[npiv] = (int)(((uint32_t)q << 17) | kk);  // ((q * 64 + fb) << 11) | r, from the uniform key
          }
          ++npiv;
          __syncthreads();
          if (QLDPC_STAMPS) st[9] += osd_stamp() - ts0;
          if (hb && tid != r) {
            // pivot-row words read kOsdXB ahead of their xors (a rolling buffer): written as
            // read-xor pairs, the compiler chained them with a wait after each read (13 LDS round
            // trips per pivot on the 25-word rows, round 4 asm review)
            constexpr int XB = kOsdXB;
            u64 buf[XB];
#pragma unroll
            for (int u = 0; u < XB; ++u)
              if (q + u < WR) buf[u] = pbuf[q + u];
            const uint32_t ps = (uint32_t)pbuf[WR];
#pragma unroll
            for (int q2 = q; q2 < WR; ++q2) {
              const u64 pv = buf[(q2 - q) % XB];
              if (q2 + XB < WR) buf[(q2 - q) % XB] = pbuf[q2 + XB];
              row[q2] ^= pv;
            }
            sbit ^= ps;
          }
          b = fb + 1;
          if (b >= bend || npiv >= rank) break;  // uniform
        }
      }
      // the pivot list -> pivrow / pivpos (every lkk write precedes one of the loop's barriers)
      for (int i = tid; i < npiv; i += TB) {
        const int v = lkk[i];
        pivrow[i] = v & 2047;
        pivpos[i] = v >> 11;
      }
      // The one remnant of the removed column-window launch (A.win is always 0, so this never
      // runs): without this uniform early-out behind the pivot loop the compiler places SGPR spill
      // reloads inside the loop (+4 to +8 instructions per pivot step), measured 0.9 % (n1600) and
      // 2 % (n225) slower in the BP+OSD shot loop.
      if (A.win == 1 && npiv < rank) {
        if (tid == 0) ow[0] = kOsdRedo;
        __syncthreads();
        continue;
      }
      // reduced rows -> the HBM slice (word-major), syndrome bits -> sb
      if (tid < m) {
        // opaque row pointer: the compiler otherwise hoists the WR word addresses out of the
        // syndrome loop, 2 * WR VGPRs live through the whole elimination (round 4 asm review)
        u64* mrow = Mg + tid;
        asm volatile("" : "+v"(mrow));
#pragma unroll
        for (int q = 0; q < WR; ++q)
          if (q < W) mrow[(size_t)q * m] = row[q];
      }
      const unsigned long long sbal = __ballot(tid < m && sbit);
      if ((tid & 63) == 0) {
        const int w0 = tid >> 5;
        if (w0 < (m + 31) / 32) sb[w0] = (uint32_t)sbal;
        if (w0 + 1 < (m + 31) / 32) sb[w0 + 1] = (uint32_t)(sbal >> 32);
      }
      if (tid == 0) s_npiv = npiv;
      __syncthreads();
    } else {
    // 2. H with permuted columns, word-major; each thread owns whole rows (LDS mode: the
    // barrier above ended every read of the sort tables this overwrites)
    const int32_t* posr = kMLds ? gpos : pos;
    for (int i = tid; i < m; i += TB) {
      for (int q = 0; q < W; ++q) M[(size_t)q * m + i] = 0;
      for (int e = A.rp[i]; e < A.rp[i + 1]; ++e) {
        const int p = posr[A.ci[e]];
        M[(size_t)(p >> 6) * m + i] ^= 1ull << (p & 63);
      }
    }
    __syncthreads();
    OSD_ST(1)
    // 3. Gauss-Jordan over positions in order (greedy pivots = ldpc's pivot set).
    // Barriers: one per dependent position, two per pivot.  Slot p%3 of s_piv collects
    // column p's pivot row; thread 0 re-arms slot (p+2)%3 after this column's first
    // barrier (its last reader, column p-1, is past that barrier; its next writer,
    // column p+2, is behind column p+1's barrier).  used / pivrow / s_npiv change
    // between the two barriers of a pivot column, while nobody reads them.
    // Memory shape: M sits in an HBM (MALL/L2) slice, so every dependent round trip costs
    // ~1 us.  The search batch-loads column p's word of all the thread's rows at once and
    // keeps which of them have the bit (M does not change until the elimination); the
    // elimination loads the pivot row and the target row by blocks of kBW words, all loads of
    // a block ahead of its stores (in-place xors of one array would otherwise serialize).
    constexpr int kRowsPT = 2048 / LB;  // rows per thread kept in a mask (m <= 2048)
    const bool masked = m <= kRowsPT * TB;
    for (int p = 0; p < n; ++p) {
      if (s_npiv >= rank) break;
      unsigned long long ts0 = 0;
      if (QLDPC_STAMPS) {
        ts0 = osd_stamp();
        st[7] += 1;
      }
      const u64* Mp = M + (size_t)(p >> 6) * m;
      const u64 bit = 1ull << (p & 63);
      const int slot = p % 3;
      uint32_t hasb = 0;  // bit j: row tid + j*TB has column p set (masked mode)
      int cand = 0x7FFFFFFF;
      if (masked) {
        u64 wv[kRowsPT];
#pragma unroll
        for (int j = 0; j < kRowsPT; ++j) {
          const int i = tid + j * TB;
          wv[j] = i < m ? Mp[i] : 0ull;
        }
        // the wave's first candidate row by ballot (rows tid + j*TB are consecutive per wave for
        // each j): one LDS atomic per wave instead of one per candidate lane
        int wcand = 0x7FFFFFFF;
#pragma unroll
        for (int j = 0; j < kRowsPT; ++j) {
          const int i = tid + j * TB;
          const bool hb = (wv[j] & bit) != 0;
          if (hb) hasb |= 1u << j;
          const unsigned long long bal = __ballot(hb && !((used[i >> 5] >> (i & 31)) & 1u));
          if (wcand == 0x7FFFFFFF && bal) wcand = (tid & ~63) + j * TB + (__ffsll((long long)bal) - 1);
        }
        if ((tid & 63) == 0) cand = wcand;
      } else {
        for (int i = tid; i < m; i += TB)
          if (!((used[i >> 5] >> (i & 31)) & 1u) && (Mp[i] & bit)) {
            cand = i;
            break;
          }
      }
      if (cand != 0x7FFFFFFF) atomicMin(&s_piv[slot], cand);
      __syncthreads();
      if (QLDPC_STAMPS) st[8] += osd_stamp() - ts0;
      const int r = s_piv[slot];
      if (tid == 0) s_piv[(p + 2) % 3] = 0x7FFFFFFF;
      if (r == 0x7FFFFFFF) continue;  // dependent position (uniform)
      const uint32_t sr = (sb[r >> 5] >> (r & 31)) & 1u;
      if (tid == 0) {
        used[r >> 5] |= 1u << (r & 31);
        pivrow[s_npiv] = r;
        pivpos[s_npiv] = p;
        s_npiv = s_npiv + 1;
      }
      const u64* Mr = M + r;
      if (masked) {
        // syndrome bits of the updated rows: one ballot per row slot, two LDS xors per wave
#pragma unroll 1
        for (int j = 0; j < kRowsPT; ++j) {
          const int i = tid + j * TB;
          const bool upd = ((hasb >> j) & 1u) != 0 && i != r;
          if (upd) row_xor(M + i, Mr, W, m);
          if (sr) {
            const unsigned long long bal = __ballot(upd);
            const int i0 = (tid & ~63) + j * TB;  // 32-aligned: TB and the wave base are multiples of 64
            if ((tid & 63) == 0 && bal) {
              if ((uint32_t)bal) atomicXor(&sb[i0 >> 5], (uint32_t)bal);
              if ((uint32_t)(bal >> 32)) atomicXor(&sb[(i0 >> 5) + 1], (uint32_t)(bal >> 32));
            }
          }
        }
      } else {
        for (int i = tid; i < m; i += TB) {
          if (i == r || !(Mp[i] & bit)) continue;
          row_xor(M + i, Mr, W, m);
          if (sr) atomicXor(&sb[i >> 5], 1u << (i & 31));
        }
      }
      __syncthreads();
    }
    }
    const int r = s_npiv;
    OSD_ST(2)
    const int RWr = (r + 63) / 64;
    // 4. Neal's column swaps -> non-pivot order Ht.  Only the non-pivot positions swp[r + j],
    // j < nh, are used: each is the identity traced backwards through the transpositions
    // (i, pivpos[i]), i = r-1 .. 0 -- one thread per needed position, no serial replay.
    // (Register-row mode stages pivpos in LDS first: the trace reads it r times.)
    const int32_t* pp = pivpos;
    if constexpr (kRR) {
      int32_t* lpp = reinterpret_cast<int32_t*>(smem + A.pbuf_off + (size_t)(WR + 1) * 8);  // after the pivot-row buffer
      for (int i = tid; i < r; i += TB) lpp[i] = pivpos[i];
      __syncthreads();
      pp = lpp;
    }
    for (int x = r + tid; x < r + nh && x < n; x += TB) {
      int cur = x;
      for (int i = r - 1; i >= 0; --i) {
        const int pi = pp[i];
        cur = cur == i ? pi : (cur == pi ? i : cur);
      }
      swp[x] = cur;
    }
    __syncthreads();
    // 5. S0 and x(h_j) as bit-vectors over the pivot index: one wave per 64-bit word, lane c
    // forms bit c (pivot q*64 + c) and a ballot packs the word
    for (int t = tid >> 6; t < (1 + nh) * RWr; t += TB >> 6) {  // uniform per wave
      const int j = t / RWr, q = t % RWr;
      const int c = tid & 63, i = q * 64 + c;
      bool bitv = false;
      if (i < r) {
        const int row = pivrow[i];
        if (j == 0) {
          bitv = ((sb[row >> 5] >> (row & 31)) & 1u) != 0;
        } else {
          const int hp = swp[r + j - 1];
          bitv = ((M[(size_t)(hp >> 6) * m + row] >> (hp & 63)) & 1ull) != 0;
        }
      }
      const unsigned long long v = __ballot(bitv);
      if (c == 0) X[(size_t)j * RW + q] = v;
    }
    if (tid == 0) s_best = ~0ull;
    __syncthreads();
    OSD_ST(3)
    // 6. candidates: lexicographic min of (weight, index)
    long long L = 1;
    if (A.method == 1 && w > 0) L = 1ll << w;
    if (A.method == 2 && w >= 0) L = 1 + (long long)k + (long long)w * (w - 1) / 2;
    if (A.method == 0 || A.order == 0 || k == 0) L = 1;
    // candidate c -> its OSD input t: the bits of c (osd_e, natural binary order), or the weight-1
    // then weight-2 inputs (osd_cs); tj[] = Ht indices
    auto cand_input = [&](long long c, int* tj, unsigned long long& ebits) -> int {
      ebits = 0;
      if (A.method == 1) {
        ebits = (unsigned long long)c;
        return __popcll(ebits);
      }
      if (c >= 1 && c <= k) {
        tj[0] = (int)(c - 1);
        return 1;
      }
      if (c > k) {
        long long rem = c - 1 - k;
        int i = 0;
        while (rem >= w - 1 - i) {
          rem -= w - 1 - i;
          ++i;
        }
        tj[0] = i;
        tj[1] = i + 1 + (int)rem;
        return 2;
      }
      return 0;
    };
    if (SIDE || A.softw) {
      // 6'. non-uniform priors (qldpc_osd_gpu_create with channel_probs that differ): the soft weight
      // sum_{j: x_j = 1} log(1 / p_j), added in ascending COLUMN order as the host stage's
      // soft_weight (and ldpc) adds it, so the candidates go to column space first: Xc[j] = X[j]
      // with pivot index i moved to its column, one ballot per 64 columns (colpiv: column -> pivot
      // index or -1); a candidate is then Xc[0] ^ (its Xc[1 + t]) | (its Ht columns), and its weight
      // one ascending walk over the set bits.  Winner: the lexicographic minimum of (weight, c), i.e.
      // the first strictly lightest candidate, as the uniform path.
      int32_t* colpiv = gpos + n;            // [n]
      u64* Xc = X + (size_t)(1 + nh) * RW;   // [(1 + nh)][W]
      const double* wt = A.softw;
      if constexpr (SIDE) {
        // the syndrome's weights, all n rewritten per syndrome (nothing of the last one's is read),
        // visible to the candidate walk through the barriers below
        double* wsel = reinterpret_cast<double*>(Xc + (size_t)(1 + nh) * W);  // [n]
        const uint8_t* sd = A.side + b * (long long)n;
        for (int j = tid; j < n; j += TB) wsel[j] = (sd[j] & 1u) ? A.softw1[j] : A.softw[j];
        wt = wsel;
      }
      for (int j = tid; j < n; j += TB) colpiv[j] = -1;
      __syncthreads();
      for (int i = tid; i < r; i += TB) colpiv[sidxr[pivpos[i]]] = i;
      __syncthreads();
      for (int t = tid >> 6; t < (1 + nh) * W; t += TB >> 6) {  // uniform per wave
        const int j = t / W, q = t % W;
        const int col = q * 64 + (tid & 63);
        bool bitv = false;
        if (col < n) {
          const int pi = colpiv[col];
          if (pi >= 0) bitv = ((X[(size_t)j * RW + (pi >> 6)] >> (pi & 63)) & 1ull) != 0;
        }
        const unsigned long long v = __ballot(bitv);
        if ((tid & 63) == 0) Xc[(size_t)j * W + q] = v;
      }
      if (tid == 0) s_bestw = ~0ull;
      __syncthreads();
      double bw = __builtin_huge_val();
      long long bc = -1;
      for (long long c = tid; c < L; c += TB) {
        int tj[2];
        unsigned long long ebits;
        const int nt = cand_input(c, tj, ebits);
        double sw = 0.0;
        for (int q = 0; q < W; ++q) {
          u64 v = Xc[q];
          if (A.method == 1) {
            for (unsigned long long e = ebits; e; e &= e - 1) {
              const int t = __ffsll((long long)e) - 1;
              v ^= Xc[(size_t)(1 + t) * W + q];
              const int hc = sidxr[swp[r + t]];
              if ((hc >> 6) == q) v |= 1ull << (hc & 63);
            }
          } else {
            for (int a = 0; a < nt; ++a) {
              v ^= Xc[(size_t)(1 + tj[a]) * W + q];
              const int hc = sidxr[swp[r + tj[a]]];
              if ((hc >> 6) == q) v |= 1ull << (hc & 63);
            }
          }
          for (; v; v &= v - 1) sw += wt[q * 64 + __ffsll((long long)v) - 1];
        }
        if (sw < bw) {  // c ascends per thread: the first of equal weights stays
          bw = sw;
          bc = c;
        }
      }
      // non-negative doubles order as their bit patterns
      const u64 wb = bc >= 0 ? (u64)__double_as_longlong(bw) : ~0ull;
      if (bc >= 0) atomicMin(&s_bestw, wb);
      __syncthreads();
      if (bc >= 0 && wb == s_bestw) atomicMin(&s_best, (u64)bc);
      __syncthreads();
    } else {
    u64 best = ~0ull;
    for (long long c = tid; c < L; c += TB) {
      int tj[2];
      unsigned long long ebits;
      const int nt = cand_input(c, tj, ebits);
      long long cnt = nt;
      for (int q = 0; q < RWr; ++q) {
        u64 v = X[q];
        if (A.method == 1) {
          for (unsigned long long e = ebits; e; e &= e - 1) v ^= X[(size_t)(1 + __ffsll((long long)e) - 1) * RW + q];
        } else {
          for (int a = 0; a < nt; ++a) v ^= X[(size_t)(1 + tj[a]) * RW + q];
        }
        cnt += __popcll(v);
      }
      const u64 key = ((u64)cnt << 40) | (u64)c;
      if (key < best) best = key;
    }
    if (best != ~0ull) atomicMin(&s_best, best);
    __syncthreads();
    }
    OSD_ST(4)
    // 7. outputs
    const long long cw = (long long)(s_best & ((1ull << 40) - 1));
    int tw[2];
    int ntw = 0;
    unsigned long long ewb = 0;
    if (A.method == 1) {
      ewb = (unsigned long long)cw;
    } else if (cw >= 1 && cw <= k) {
      tw[0] = (int)(cw - 1);
      ntw = 1;
    } else if (cw > k) {
      long long rem = cw - 1 - k;
      int i = 0;
      while (rem >= w - 1 - i) {
        rem -= w - 1 - i;
        ++i;
      }
      tw[0] = i;
      tw[1] = i + 1 + (int)rem;
      ntw = 2;
    }
    for (int j = tid; j < n; j += TB) {
      ow[j] = 0;
      if (o0) o0[j] = 0;
    }
    __syncthreads();
    for (int i = tid; i < r; i += TB) {
      const int q = i >> 6, c = i & 63;
      const u64 s0 = (X[q] >> c) & 1ull;
      u64 v = X[q];
      if (A.method == 1) {
        for (unsigned long long e = ewb; e; e &= e - 1) v ^= X[(size_t)(1 + __ffsll((long long)e) - 1) * RW + q];
      } else {
        for (int a = 0; a < ntw; ++a) v ^= X[(size_t)(1 + tw[a]) * RW + q];
      }
      const int col = sidxr[pivpos[i]];
      ow[col] = (uint8_t)((v >> c) & 1ull);
      if (o0) o0[col] = (uint8_t)s0;
    }
    if (tid == 0) {
      if (A.method == 1) {
        for (unsigned long long e = ewb; e; e &= e - 1) ow[sidxr[swp[r + __ffsll((long long)e) - 1]]] = 1;
      } else {
        for (int a = 0; a < ntw; ++a) ow[sidxr[swp[r + tw[a]]]] = 1;
      }
    }
    __syncthreads();
    OSD_ST(5)
    if (QLDPC_STAMPS) st[6] += 1;
  }
#undef OSD_ST
  if (QLDPC_STAMPS && tid == 0)
    for (int k2 = 0; k2 < 16; ++k2) atomicAdd(&g_osd_stamps[k2], st[k2]);
}

}  // namespace

namespace {

// BP+OSD failure re-check of the fused shot loop's candidates (qldpc_mc_set_osd): per
// candidate, the residual r = e ^ x_osd against H (src/Simulators.py:139-160: a syndrome
// mismatch counts as a failure) and the logical operators (column masks, as the MC kernel uses);
// a sector verdict the OSD turned into a success clears that sector's bit of the shot's fail
// flags and takes the shot out of the sector / total failure counters.
__global__ void __launch_bounds__(256) osd_recheck_kernel(const int32_t* rp, const int32_t* ci, int m, int n,
                                                          const unsigned long long* lmask, int kw, const uint8_t* err,
                                                          const uint8_t* outw, const long long* shot, long long ncand,
                                                          int q, int logical_mode, uint8_t* fail,
                                                          unsigned long long* counters) {
  __shared__ uint32_t lsyn[8];
  __shared__ int hbad;
  const int tid = threadIdx.x;
  for (long long b = blockIdx.x; b < ncand; b += gridDim.x) {
    const long long s = shot[b];
    if (s < 0) continue;  // converged at max_iter: the BP verdict stands (uniform)
    if (tid < 8) lsyn[tid] = 0;
    if (tid == 0) hbad = 0;
    __syncthreads();
    const uint8_t* e = err + b * (long long)n;
    const uint8_t* x = outw + b * (long long)n;
    for (int j = tid; j < n; j += blockDim.x)
      if ((e[j] ^ x[j]) & 1u)
        for (int w = 0; w < kw; ++w) {
          const unsigned long long v = lmask[(long long)j * kw + w];
          if ((uint32_t)v) atomicXor(&lsyn[2 * w], (uint32_t)v);
          if ((uint32_t)(v >> 32)) atomicXor(&lsyn[2 * w + 1], (uint32_t)(v >> 32));
        }
    for (int i = tid; i < m; i += blockDim.x) {
      uint32_t par = 0;
      for (int k = rp[i]; k < rp[i + 1]; ++k) par ^= (uint32_t)(e[ci[k]] ^ x[ci[k]]);
      if (par & 1u) hbad = 1;
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t any = (uint32_t)hbad;
      for (int w = 0; w < 8; ++w) any |= lsyn[w];
      if (!any) {
        const uint32_t old = fail[s], nw = old & ~(1u << q);
        fail[s] = (uint8_t)nw;
        atomicAdd(&counters[8 + q], ~0ull);  // sector failures - 1
        auto tot = [&](uint32_t f) { return logical_mode == 0 ? (f & 1u) : logical_mode == 1 ? (f >> 1) & 1u : (f != 0); };
        if (tot(old) && !tot(nw)) atomicAdd(&counters[1], ~0ull);  // failures - 1
      }
    }
    __syncthreads();
  }
}

}  // namespace

namespace {
// register-row kernels: the compile-time row widths (words) built, smallest first
// Rows up to 16 words: 1024-thread workgroups (128 VGPRs); 20-25 words: 768 threads = 3 waves
// per SIMD, 168 VGPRs (m <= 768: hgp_34_n1600's 768 x 1600 exactly; wider rows spill).  One row
// per thread: 2 or 3 rows per thread in 384 / 256 threads (fewer waves reading each broadcast
// pivot word) measured 16 % / 26 % slower on n1600 (the per-pivot chain is latency-bound).
constexpr int kOsdWR[] = {2, 4, 8, 12, 16, 20, 25};
inline int osd_rr_threads(int wr) { return wr <= 16 ? 1024 : 768; }
using OsdKern = void (*)(OsdGpuArgs);
template <bool SIDE>
OsdKern osd_rr_kernel_of(int wr) {
  switch (wr) {
    case 2: return &osd_gpu_kernel<1024, 2, SIDE>;
    case 4: return &osd_gpu_kernel<1024, 4, SIDE>;
    case 8: return &osd_gpu_kernel<1024, 8, SIDE>;
    case 12: return &osd_gpu_kernel<1024, 12, SIDE>;
    case 16: return &osd_gpu_kernel<1024, 16, SIDE>;
    case 20: return &osd_gpu_kernel<768, 20, SIDE>;
    case 25: return &osd_gpu_kernel<768, 25, SIDE>;
    default: return nullptr;
  }
}
OsdKern osd_rr_kernel(int wr, bool side = false) {
  return side ? osd_rr_kernel_of<true>(wr) : osd_rr_kernel_of<false>(wr);
}
}  // namespace

namespace qldpc_rt {
// BP+OSD stage of the fused shot loop for one sector: GPU OSD on the ncand captured
// candidates, then the failure re-check (osd_recheck_kernel).
int osd_gpu_bposd_stage(qldpc_osd_gpu* osd, const uint8_t* synd, const double* post, const uint8_t* err,
                        const long long* shot, uint8_t* outw, long long ncand, const unsigned long long* lmask, int kw,
                        int q, int logical_mode, uint8_t* fail, unsigned long long* counters, hipStream_t stream) {
  if (ncand <= 0) return 0;
  int rc = osd_gpu_decode_slots(osd, synd, post, nullptr, shot, nullptr, nullptr, outw, ncand, stream);
  if (rc) return rc;
  const int grid = (int)std::min<long long>(ncand, 4096);
  hipLaunchKernelGGL(osd_recheck_kernel, dim3(grid), dim3(256), 0, stream, static_cast<const int32_t*>(osd->rp.p),
                     static_cast<const int32_t*>(osd->ci.p), osd->host.m, osd->host.n, lmask, kw, err, outw, shot,
                     ncand, q, logical_mode, fail, counters);
  QLDPC_HIP(hipGetLastError());
  return 0;
}

// true when the host OSD stage was built on exactly this graph (shape and edges)
bool osd_host_matches(const qldpc_osd* o, const qldpc_graph* g) {
  return o && g && o->m == g->m && o->n == g->n && o->col_rows == g->col_rows;
}

// true when the GPU OSD handle was built on exactly this graph (shape and edges)
bool osd_gpu_matches(const qldpc_osd_gpu* o, const qldpc_graph* g) {
  return o && g && o->host.m == g->m && o->host.n == g->n && o->host.col_rows == g->col_rows;
}

bool osd_gpu_has_side(const qldpc_osd_gpu* o) { return o && o->sw0.p; }
}  // namespace qldpc_rt

extern "C" {

int qldpc_osd_gpu_create(const qldpc_graph* g, const double* channel_probs, int32_t osd_method, int32_t osd_order,
                         qldpc_osd_gpu** out) {
  if (!g || !channel_probs || !out) return set_err(QLDPC_EINVAL, "NULL argument");
  qldpc_osd* O = nullptr;
  int rc = qldpc_osd_create(g->m, g->n, g->row_ptr.data(), g->col_idx.data(), channel_probs, osd_method, osd_order,
                            &O);
  if (rc) return rc;
  rc = qldpc_rt::osd_gpu_from_host(g, O, out);
  qldpc_osd_destroy(O);
  return rc;
}

}  // extern "C"

// The GPU OSD of a host OSD stage built on graph g (same method, order, rank and soft weights
// log(1 / p_j), copied: no re-derivation from probabilities).  qldpc_osd_gpu_create and the circuit
// loop (a host stage handed to qldpc_circ_set_final_osd runs on the GPU) both build through here.
int qldpc_rt::osd_gpu_from_host(const qldpc_graph* g, const qldpc_osd* O, qldpc_osd_gpu** out) {
  if (!g || !O || !out) return set_err(QLDPC_EINVAL, "NULL argument");
  if (!osd_host_matches(O, g)) return set_err(QLDPC_EINVAL, "host OSD stage was built on a different graph");
  if (O->lsd_k) return lsd_gpu_from_host(g, O, out);
  const int osd_method = O->method, osd_order = O->order;
  int rc = 0;
  if (g->n > kOsdMaxN || (osd_method == 1 && osd_order > 20))  // 20: the host stage's cap (qldpc_osd_create)
    return set_err(QLDPC_ENOTSUP, "GPU OSD: n > 8192 or osd_e order > 20");
  auto* G = new qldpc_osd_gpu();
  G->host = *O;
  G->device = g->device;
  const int m = g->m, n = g->n, rank = G->host.rank, k = n - rank;
  const int w = std::min(G->host.order, k);
  G->W = (n + 63) / 64;
  G->RW = std::max(1, (rank + 63) / 64);
  G->NP = 1;
  while (G->NP < n) G->NP <<= 1;
  G->nh = G->host.method == 2 ? k : w;
  // LDS: sort tables (skey, sidx, pos), then the used / syndrome bit-vectors.  The Gauss-Jordan
  // image goes to LDS too when it fits over the sort tables (those are copied to HBM ints before
  // the image is built): every pivot search / row update is then an LDS access instead of a
  // ~1 us HBM round trip.  QLDPC_OSD_LDS=0 keeps the image in the HBM slice.
  const size_t lsort = ((size_t)G->NP * 12 + (size_t)n * 4 + 15) & ~(size_t)15;
  const size_t mbytes = ((size_t)G->W * m * 8 + 15) & ~(size_t)15;
  const size_t lbits = (size_t)((m + 31) / 32) * 8 + 64;
  const char* lds_env = std::getenv("QLDPC_OSD_LDS");
  const bool want_lds = !lds_env || std::atoi(lds_env) != 0;
  // register-row mode (one row per thread of a 1024-thread workgroup, row words in VGPRs) when
  // m <= 1024 and n <= 2048; QLDPC_OSD_RR=0 keeps the LDS / HBM image
  const char* rr_env = std::getenv("QLDPC_OSD_RR");
  if (!rr_env || std::atoi(rr_env) != 0)
    for (int wr : kOsdWR)
      if (wr >= G->W) {
        if (m <= osd_rr_threads(wr)) {
          G->wr = wr;
          G->rr_tb = std::max(64, (m + 63) / 64 * 64);  // one row per thread, no idle waves
        }
        break;
      }
  G->m_lds = (!G->wr && want_lds && std::max(lsort, mbytes) + lbits <= (size_t)160 * 1024 - 256) ? 1 : 0;  // 256: static LDS
  G->bits_off = (int)(G->m_lds ? std::max(lsort, mbytes) : lsort);
  G->pbuf_off = (int)(((size_t)G->bits_off + lbits + 15) & ~(size_t)15);
  // register-row mode: pivot-row buffer, then pivpos staged for the swap trace (rank ints)
  G->lds = G->wr ? (size_t)G->pbuf_off + (size_t)(G->wr + 1) * 8 + (size_t)std::max(1, rank) * 4
                 : (size_t)G->bits_off + lbits;
  // non-uniform priors: the candidates' column-space vectors Xc [(1 + nh)][W] after X, and the
  // column -> pivot map [n] after the sort maps
  G->ws_words = (long long)G->W * m + (long long)(1 + G->nh) * G->RW +
                (G->host.uniform ? 0ll : (long long)(1 + G->nh) * G->W);
  G->iws_ints = 2ll * rank + 4ll * n;
  auto fail = [&](int code) {
    G->rp.release(); G->ci.release(); G->ws.release(); G->iws.release(); G->softw.release();
    G->sw0.release(); G->sw1.release();
    delete G;
    return code;
  };
  if (hipSetDevice(g->device) != hipSuccess) return fail(set_err(QLDPC_EHIP, "hipSetDevice"));
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g->device) != hipSuccess || cus <= 0)
    return fail(set_err(QLDPC_EHIP, "device CU count"));
  int nb = 0;
  const void* kf = G->wr ? reinterpret_cast<const void*>(osd_rr_kernel(G->wr))
                  : G->m_lds ? reinterpret_cast<const void*>(&osd_gpu_kernel<kOsdThreadsLds>)
                             : reinterpret_cast<const void*>(&osd_gpu_kernel<kOsdThreads>);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kf,
                                                   G->wr ? G->rr_tb : G->m_lds ? kOsdThreadsLds : kOsdThreads,
                                                   G->lds) != hipSuccess || nb <= 0)
    nb = 1;
  G->grid = cus * nb;
  const size_t E = g->col_idx.size();
  if ((rc = G->rp.alloc((size_t)(m + 1) * 4)) || (rc = G->ci.alloc(std::max<size_t>(E, 1) * 4)) ||
      (rc = G->ws.alloc((size_t)G->grid * G->ws_words * 8)) ||
      (rc = G->iws.alloc((size_t)G->grid * G->iws_ints * 4)) ||
      (!G->host.uniform && (rc = G->softw.alloc((size_t)n * 8))))
    return fail(rc);
  if (!G->host.uniform && hipMemcpy(G->softw.p, G->host.w.data(), (size_t)n * 8, hipMemcpyHostToDevice) != hipSuccess)
    return fail(set_err(QLDPC_EHIP, "upload OSD soft weights"));
  if (hipMemcpy(G->rp.p, g->row_ptr.data(), (size_t)(m + 1) * 4, hipMemcpyHostToDevice) != hipSuccess ||
      (E && hipMemcpy(G->ci.p, g->col_idx.data(), E * 4, hipMemcpyHostToDevice) != hipSuccess))
    return fail(set_err(QLDPC_EHIP, "upload OSD graph"));
  *out = G;
  return 0;
}

extern "C" {

int qldpc_osd_gpu_geometry(const qldpc_osd_gpu* osd, int32_t* row_words, int32_t* window_words, int32_t* threads,
                           int32_t* workgroups) {
  if (!osd || !row_words || !window_words || !threads || !workgroups) return set_err(QLDPC_EINVAL, "NULL argument");
  *row_words = osd->wr;
  *window_words = 0;  // kept for the ABI: no layout holds a column window
  if (osd->host.lsd_k) {  // the cluster kernel (lsd.hip): no register rows
    *threads = qldpc_rt::lsd_gpu_threads();
    *workgroups = osd->grid;
    return 0;
  }
  *threads = osd->wr ? osd->rr_tb : osd->m_lds ? kOsdThreadsLds : kOsdThreads;
  *workgroups = osd->grid;
  return 0;
}

int qldpc_osd_gpu_destroy(qldpc_osd_gpu* osd) {
  if (!osd) return 0;
  osd->rp.release(); osd->ci.release(); osd->ws.release(); osd->iws.release(); osd->softw.release();
  osd->sw0.release(); osd->sw1.release(); osd->cp.release(); osd->ce.release(); osd->lsd_retries.release(); osd->lsd_wq.release();
  delete osd;
  return 0;
}

#if QLDPC_STAMPS
// diagnostic builds only: read and clear osd_gpu_kernel's step-cycle sums
int qldpc_debug_osd_stamps(unsigned long long* out) {
  unsigned long long z[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(out, HIP_SYMBOL(g_osd_stamps), 128) != hipSuccess)
    return -1;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_osd_stamps), z, 128) == hipSuccess ? 0 : -1;
}
#endif

}  // extern "C"

namespace qldpc_rt {
// qldpc_osd_gpu_decode with the fused loop's capture-slot shot indices (slots < 0 are skipped)
int osd_gpu_decode_slots(qldpc_osd_gpu* osd, const uint8_t* d_synd, const double* d_post, const uint8_t* d_conv,
                         const long long* d_shot, const uint8_t* d_bp_corr, uint8_t* d_out0, uint8_t* d_outw,
                         int64_t B, void* stream) {
  return osd_gpu_decode_any(osd, d_synd, d_post, d_conv, d_shot, d_bp_corr, nullptr, d_out0, d_outw, B, stream);
}

// d_side != null: the side decode (the SIDE kernels, weights from the handle's side tables)
int osd_gpu_decode_any(qldpc_osd_gpu* osd, const uint8_t* d_synd, const double* d_post, const uint8_t* d_conv,
                       const long long* d_shot, const uint8_t* d_bp_corr, const uint8_t* d_side, uint8_t* d_out0,
                       uint8_t* d_outw, int64_t B, void* stream) {
  if (!osd || (B > 0 && (!d_synd || !d_post || !d_outw))) return set_err(QLDPC_EINVAL, "NULL argument");
  if (d_conv && !d_bp_corr) return set_err(QLDPC_EINVAL, "conv needs bp_corr");
  if (B <= 0) return 0;
  if (osd->host.lsd_k) {  // LSD handle: the cluster kernel; a side decode is its plain decode (no weights)
    if (d_side && !osd->sw0.p)
      return set_err(QLDPC_EINVAL, "side decode without side tables (qldpc_osd_gpu_set_side_probs)");
    return lsd_gpu_launch(osd, d_synd, d_post, d_conv, d_shot, d_bp_corr, d_out0, d_outw, nullptr, B, stream);
  }
  QLDPC_HIP(hipSetDevice(osd->device));
  OsdGpuArgs a;
  a.rp = static_cast<const int32_t*>(osd->rp.p);
  a.ci = static_cast<const int32_t*>(osd->ci.p);
  a.synd = d_synd; a.post = d_post; a.conv = d_conv; a.shot = d_shot; a.bp_corr = d_bp_corr; a.out0 = d_out0;
  a.softw = osd->host.uniform ? nullptr : static_cast<const double*>(osd->softw.p);
  a.softw1 = nullptr;
  a.side = d_side;
  if (d_side) {
    if (!osd->sw0.p) return set_err(QLDPC_EINVAL, "side decode without side tables (qldpc_osd_gpu_set_side_probs)");
    a.softw = static_cast<const double*>(osd->sw0.p);
    a.softw1 = static_cast<const double*>(osd->sw1.p);
  }
  a.outw = d_outw;
  a.ws = static_cast<u64*>(osd->ws.p);
  a.iws = static_cast<int32_t*>(osd->iws.p);
  a.B = B;
  a.m = osd->host.m; a.n = osd->host.n; a.W = osd->W; a.RW = osd->RW; a.rank = osd->host.rank;
  a.method = osd->host.method; a.order = osd->host.order; a.NP = osd->NP; a.m_lds = osd->m_lds; a.bits_off = osd->bits_off;
  a.pbuf_off = osd->pbuf_off;
  a.win = 0;
  a.ws_words = osd->ws_words; a.iws_ints = osd->iws_ints;
  const int grid = (int)std::min<long long>(B, osd->grid);
  if (d_side) {
    if (osd->wr)
      hipLaunchKernelGGL(osd_rr_kernel(osd->wr, true), dim3(grid), dim3(osd->rr_tb), osd->lds, (hipStream_t)stream, a);
    else if (osd->m_lds)
      hipLaunchKernelGGL((osd_gpu_kernel<kOsdThreadsLds, 0, true>), dim3(grid), dim3(kOsdThreadsLds), osd->lds,
                         (hipStream_t)stream, a);
    else
      hipLaunchKernelGGL((osd_gpu_kernel<kOsdThreads, 0, true>), dim3(grid), dim3(kOsdThreads), osd->lds,
                         (hipStream_t)stream, a);
  } else if (osd->wr)
    hipLaunchKernelGGL(osd_rr_kernel(osd->wr), dim3(grid), dim3(osd->rr_tb), osd->lds, (hipStream_t)stream, a);
  else if (osd->m_lds)
    hipLaunchKernelGGL(osd_gpu_kernel<kOsdThreadsLds>, dim3(grid), dim3(kOsdThreadsLds), osd->lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(osd_gpu_kernel<kOsdThreads>, dim3(grid), dim3(kOsdThreads), osd->lds, (hipStream_t)stream, a);
  QLDPC_HIP(hipGetLastError());
  return 0;
}
}  // namespace qldpc_rt

extern "C" {
int qldpc_osd_gpu_decode(qldpc_osd_gpu* osd, const uint8_t* d_synd, const double* d_post, const uint8_t* d_conv,
                         const uint8_t* d_bp_corr, uint8_t* d_out0, uint8_t* d_outw, int64_t B, void* stream) {
  return qldpc_rt::osd_gpu_decode_slots(osd, d_synd, d_post, d_conv, nullptr, d_bp_corr, d_out0, d_outw, B, stream);
}

// Side tables of the GPU handle: the same law and checks as qldpc_osd_set_side_probs.  The workspace
// grows to the soft path's (Xc, which a uniform handle does not have) plus the staged weights [n]
// per workgroup; the grid, the LDS layout and so qldpc_osd_gpu_geometry stay as they are.
int qldpc_osd_gpu_set_side_probs(qldpc_osd_gpu* osd, const double* p0, const double* p1) {
  if (!osd || !p0 || !p1) return set_err(QLDPC_EINVAL, "NULL argument");
  int rc = qldpc_osd_set_side_probs(&osd->host, p0, p1);
  if (rc) return rc;
  const int n = osd->host.n;
  QLDPC_HIP(hipSetDevice(osd->device));
  QLDPC_HIP(hipDeviceSynchronize());  // no decode in flight on the workspace that is replaced
  const long long words = (long long)osd->W * osd->host.m + (long long)(1 + osd->nh) * osd->RW +
                          (long long)(1 + osd->nh) * osd->W + n;
  if (!osd->host.lsd_k && words > osd->ws_words) {  // (an LSD handle's workspace holds no weights)
    osd->ws.release();
    osd->ws_words = words;
    if ((rc = osd->ws.alloc((size_t)osd->grid * osd->ws_words * 8))) return rc;
  }
  if (!osd->sw0.p && ((rc = osd->sw0.alloc((size_t)n * 8)) || (rc = osd->sw1.alloc((size_t)n * 8)))) return rc;
  QLDPC_HIP(hipMemcpy(osd->sw0.p, osd->host.ws0.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  QLDPC_HIP(hipMemcpy(osd->sw1.p, osd->host.ws1.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  return 0;
}

int qldpc_osd_gpu_decode_side(qldpc_osd_gpu* osd, const uint8_t* d_synd, const double* d_post, const uint8_t* d_conv,
                              const uint8_t* d_bp_corr, const uint8_t* d_side, uint8_t* d_out0, uint8_t* d_outw,
                              int64_t B, void* stream) {
  if (!osd || (B > 0 && !d_side)) return set_err(QLDPC_EINVAL, "NULL argument");
  if (!osd->sw0.p) return set_err(QLDPC_EINVAL, "side decode without side tables (qldpc_osd_gpu_set_side_probs)");
  return qldpc_rt::osd_gpu_decode_any(osd, d_synd, d_post, d_conv, nullptr, d_bp_corr, d_side, d_out0, d_outw, B,
                                      stream);
}

}  // extern "C"

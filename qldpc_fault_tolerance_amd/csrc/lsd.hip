// lsd.hip — localised statistics decoding of order 0 (BP+LSD; Hillmann et al. 2024) as a second stage
// behind soft-output BP, beside osd.hip and reached through the same two handles.  THE LAW is stated in
// include/qldpc_hip.h ("BP+LSD"): clusters grow around the unsatisfied checks in BP's reliability order
// until each is consistent, and elimination happens inside the clusters alone.  Every choice of the law
// is a set or a total order, so the host stage and the kernel below may work in any order they like.
//
// Linear algebra, both stages: clusters share no row, so ONE Gauss-Jordan-reduced xor basis of the
// active columns (bit-vectors over the active rows) serves all clusters.  Adding a column is an
// insertion: reduce it by the basis vectors whose pivot bit it has, and if something is left, take its
// lowest bit as the pivot and clear that bit from every other vector and from the reduced syndrome.  A
// row that joins later has zeros in every older column, so nothing is ever re-eliminated.  The rows where
// the reduced syndrome is non-zero name the invalid clusters.  The law's solution re-inserts the active
// columns in column order, each kept vector carrying the combination of kept columns it stands for.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <numeric>
#include <thread>
#include <vector>

#include "osd_types.h"
#include "runtime.h"

using qldpc_rt::set_err;

namespace {

using u64 = unsigned long long;

// ---------------------------------------------------------------------------------------------------
// host stage
// ---------------------------------------------------------------------------------------------------

// Gauss-Jordan-reduced xor basis over m row bits; each vector carries a combination word vector (CW)
struct LsdBasis {
  int W = 0, CW = 0, nv = 0;
  std::vector<u64> vec, comb, sred, scomb;
  std::vector<int32_t> piv;
  void init(int m, int cw) {
    W = (m + 63) / 64;
    CW = cw;
    nv = 0;
    vec.clear();
    comb.clear();
    piv.clear();
    sred.assign(std::max(W, 1), 0ull);
    scomb.assign(std::max(CW, 1), 0ull);
  }
  static bool bit(const u64* v, int b) { return (v[b >> 6] >> (b & 63)) & 1ull; }
  // v [W], c [CW] are consumed; true when v was independent of the basis
  bool insert(u64* v, u64* c) {
    for (int i = 0; i < nv; ++i)
      if (bit(v, piv[i])) {
        for (int q = 0; q < W; ++q) v[q] ^= vec[(size_t)i * W + q];
        for (int q = 0; q < CW; ++q) c[q] ^= comb[(size_t)i * CW + q];
      }
    int p = -1;
    for (int q = 0; q < W && p < 0; ++q)
      if (v[q]) p = q * 64 + __builtin_ctzll(v[q]);
    if (p < 0) return false;
    for (int i = 0; i < nv; ++i)
      if (bit(&vec[(size_t)i * W], p)) {
        for (int q = 0; q < W; ++q) vec[(size_t)i * W + q] ^= v[q];
        for (int q = 0; q < CW; ++q) comb[(size_t)i * CW + q] ^= c[q];
      }
    if (bit(sred.data(), p)) {
      for (int q = 0; q < W; ++q) sred[q] ^= v[q];
      for (int q = 0; q < CW; ++q) scomb[q] ^= c[q];
    }
    vec.insert(vec.end(), v, v + W);
    if (CW) comb.insert(comb.end(), c, c + CW);
    piv.push_back(p);
    ++nv;
    return true;
  }
};

struct LsdWork {
  LsdBasis B;
  std::vector<int32_t> order, rank, parent, A, R, picks, kept;
  std::vector<uint8_t> inA, inR, bad;
  std::vector<std::vector<int32_t>> cand;
  std::vector<u64> v, c;
  // order > 0: free counts by root; the free columns in column order with dep(f) over the kept slots;
  // the cluster being searched
  std::vector<int32_t> fre, depcol, fl, pick, best;
  std::vector<u64> dep;
  std::vector<uint8_t> done;
  int find(int i) {
    while (parent[i] != i) i = parent[i] = parent[parent[i]];
    return i;
  }
};

void lsd_load_col(const qldpc_osd& O, int j, u64* v, int W) {
  std::fill(v, v + W, 0ull);
  for (int r : O.col_rows[j]) v[r >> 6] ^= 1ull << (r & 63);
}

void lsd_search(const qldpc_osd& O, LsdWork& K, int CW, uint8_t* x);

// x0 (or null): the union of the candidates 0; x: the union of the winners
void lsd_one(const qldpc_osd& O, LsdWork& K, const uint8_t* synd, const double* post, uint8_t* x0, uint8_t* x,
             int32_t* stats) {
  const int m = O.m, n = O.n, k = O.lsd_k, w = O.lsd_w;
  const int W = (m + 63) / 64;
  std::fill(x, x + n, (uint8_t)0);
  K.order.resize(n);
  std::iota(K.order.begin(), K.order.end(), 0);
  std::stable_sort(K.order.begin(), K.order.end(), [&](int a, int b) { return post[a] < post[b]; });
  K.rank.resize(n);
  for (int p = 0; p < n; ++p) K.rank[K.order[p]] = p;
  K.parent.resize(m);
  std::iota(K.parent.begin(), K.parent.end(), 0);
  K.inA.assign(n, 0);
  K.inR.assign(m, 0);
  K.bad.assign(m, 0);
  K.A.clear();
  K.R.clear();
  K.cand.resize(m);
  K.v.resize(std::max(W, 1));
  K.B.init(m, 0);
  for (int i = 0; i < m; ++i)
    if (synd[i] & 1u) {
      K.inR[i] = 1;
      K.R.push_back(i);
      K.B.sred[i >> 6] |= 1ull << (i & 63);
    }
  int rounds = 0;
  if (!K.R.empty())
    for (;;) {
      // the nominating clusters, by root: the invalid ones, and the valid ones with fewer than w free
      // columns (columns less basis vectors: the rank of a cluster does not depend on the insertion order)
      bool any = false;
      for (int i : K.R) K.bad[K.find(i)] = 0;
      for (int i : K.R)
        if (LsdBasis::bit(K.B.sred.data(), i)) K.bad[K.find(i)] = 1, any = true;
      if (w > 0) {
        K.fre.resize(m);
        for (int i : K.R) K.fre[K.find(i)] = 0;
        for (int j : K.A) ++K.fre[K.find(O.col_rows[j][0])];
        for (int p : K.B.piv) --K.fre[K.find(p)];
        for (int i : K.R) {
          const int r = K.find(i);
          if (!K.bad[r] && K.fre[r] < w) K.bad[r] = 2, any = true;
        }
      }
      if (!any) break;
      // their boundaries, and the first k of each in column order
      for (int i : K.R) K.cand[K.find(i)].clear();
      for (int i : K.R) {
        const int r = K.find(i);
        if (!K.bad[r]) continue;
        for (int e = O.row_ptr[i]; e < O.row_ptr[i + 1]; ++e)
          if (!K.inA[O.col_idx[e]]) K.cand[r].push_back(K.rank[O.col_idx[e]]);
      }
      K.picks.clear();
      for (int i : K.R) {
        if (K.find(i) != i || !K.bad[i]) continue;
        auto& c = K.cand[i];
        std::sort(c.begin(), c.end());
        c.erase(std::unique(c.begin(), c.end()), c.end());
        for (int t = 0; t < (int)c.size() && t < k; ++t) K.picks.push_back(K.order[c[t]]);
      }
      if (K.picks.empty()) break;
      ++rounds;
      for (int j : K.picks) {
        if (K.inA[j]) continue;  // nominated twice: joins once
        K.inA[j] = 1;
        K.A.push_back(j);
        const auto& rows = O.col_rows[j];
        for (int r : rows) {
          if (!K.inR[r]) K.inR[r] = 1, K.R.push_back(r);
          K.parent[K.find(r)] = K.find(rows[0]);
        }
        lsd_load_col(O, j, K.v.data(), W);
        K.B.insert(K.v.data(), nullptr);
      }
    }
  // unsolvable clusters and the count of clusters at the end
  int valid = 1, ncl = 0;
  for (int i : K.R) K.bad[K.find(i)] = 0;
  for (int i : K.R) {
    if (K.find(i) == i) ++ncl;
    if (LsdBasis::bit(K.B.sred.data(), i)) K.bad[K.find(i)] = 1, valid = 0;
  }
  // the law's solution: the active columns again in column order, with combinations
  std::sort(K.A.begin(), K.A.end(), [&](int a, int b) { return K.rank[a] < K.rank[b]; });
  const int CW = ((int)std::min<size_t>(K.A.size(), (size_t)m) + 63) / 64;
  LsdBasis& F = K.B;
  F.init(m, CW);
  for (int i = 0; i < m; ++i)
    if (synd[i] & 1u) F.sred[i >> 6] |= 1ull << (i & 63);
  K.c.resize(std::max(CW, 1));
  K.kept.clear();
  K.depcol.clear();
  K.dep.clear();
  for (int j : K.A) {
    lsd_load_col(O, j, K.v.data(), W);
    std::fill(K.c.begin(), K.c.end(), 0ull);
    const int t = (int)K.kept.size();
    if (t < CW * 64) K.c[t >> 6] |= 1ull << (t & 63);
    if (F.insert(K.v.data(), K.c.data())) {
      K.kept.push_back(j);
    } else if (w > 0) {  // a free column: what is left of its combination is dep(f)
      if (t < CW * 64) K.c[t >> 6] &= ~(1ull << (t & 63));
      K.depcol.push_back(j);
      K.dep.insert(K.dep.end(), K.c.begin(), K.c.begin() + CW);
    }
  }
  for (int t = 0; t < (int)K.kept.size(); ++t) {
    const int j = K.kept[t];
    if (LsdBasis::bit(F.scomb.data(), t) && !K.bad[K.find(O.col_rows[j][0])]) x[j] = 1;
  }
  if (x0) std::copy(x, x + n, x0);
  if (w > 0 && !K.depcol.empty()) lsd_search(O, K, CW, x);
  if (stats) {
    stats[0] = valid;
    stats[1] = rounds;
    stats[2] = (int32_t)K.A.size();
    stats[3] = ncl;
  }
}

// The candidate search of order w > 0 on every valid final cluster, one after another: the cluster's free
// columns F in column order (the re-insertion met them in that order), T = the first min(w, |F|), the
// candidates of the method in the law's order.  A candidate is weighed by its difference to candidate 0,
// sum wq over t plus, over the kept slots of xor dep(f), -wq where x0 is set and +wq where it is not: an
// integer, so the comparison is that of the full weights.  x holds x0 on entry and the winners on return.
void lsd_search(const qldpc_osd& O, LsdWork& K, int CW, uint8_t* x) {
  const int w = O.lsd_w, nf = (int)K.depcol.size();
  const long long* wq = O.lsd_wq.data();
  const u64* x0 = K.B.scomb.data();
  auto root = [&](int e) { return K.find(O.col_rows[K.depcol[e]][0]); };
  auto delta = [&](const std::vector<int32_t>& t) {
    long long d = 0;
    for (int e : t) d += wq[K.depcol[e]];
    for (int q = 0; q < CW; ++q) {
      u64 D = 0;
      for (int e : t) D ^= K.dep[(size_t)e * CW + q];
      for (; D; D &= D - 1) {
        const int b = __builtin_ctzll(D);
        const long long wt = wq[K.kept[q * 64 + b]];
        d += ((x0[q] >> b) & 1ull) ? -wt : wt;
      }
    }
    return d;
  };
  K.done.assign(O.m, 0);
  for (int e0 = 0; e0 < nf; ++e0) {
    const int r = root(e0);
    if (K.bad[r] || K.done[r]) continue;
    K.done[r] = 1;
    K.fl.clear();
    for (int e = e0; e < nf; ++e)
      if (root(e) == r) K.fl.push_back(e);
    const int nF = (int)K.fl.size(), T = std::min(w, nF);
    long long bw = 0;
    K.best.clear();
    auto weigh = [&]() {
      const long long d = delta(K.pick);
      if (d < bw) bw = d, K.best = K.pick;
    };
    if (O.lsd_method == 1) {
      for (uint32_t c = 1; c < (1u << T); ++c) {
        K.pick.clear();
        for (int i = 0; i < T; ++i)
          if ((c >> i) & 1u) K.pick.push_back(K.fl[i]);
        weigh();
      }
    } else {
      for (int a = 0; a < nF; ++a) K.pick.assign(1, K.fl[a]), weigh();
      for (int a = 0; a < T; ++a)
        for (int b = a + 1; b < T; ++b) K.pick.assign({K.fl[a], K.fl[b]}), weigh();
    }
    for (int e : K.best) {
      x[K.depcol[e]] = 1;
      for (int q = 0; q < CW; ++q)
        for (u64 D = K.dep[(size_t)e * CW + q]; D; D &= D - 1) x[K.kept[q * 64 + __builtin_ctzll(D)]] ^= 1;
    }
  }
}

int lsd_rank(const qldpc_osd& O) {
  LsdBasis B;
  B.init(O.m, 0);
  std::vector<u64> v(std::max(B.W, 1));
  int rank = 0;
  for (int j = 0; j < O.n && rank < O.m; ++j) {
    lsd_load_col(O, j, v.data(), B.W);
    if (B.insert(v.data(), nullptr)) ++rank;
  }
  return rank;
}

}  // namespace

int qldpc_rt::lsd_decode_batch_host(const qldpc_osd* osd, const uint8_t* synd, const double* post,
                                    const uint8_t* conv, const uint8_t* bp_corr, uint8_t* out_osd0,
                                    uint8_t* out_osdw, int32_t* stats, int64_t B, int32_t threads) {
  if (!osd || !osd->lsd_k || (B > 0 && (!synd || !post || !out_osdw))) return set_err(QLDPC_EINVAL, "NULL argument");
  if (conv && !bp_corr) return set_err(QLDPC_EINVAL, "conv needs bp_corr");
  if (B <= 0) return 0;
  const int m = osd->m, n = osd->n;
  std::vector<int64_t> todo;
  for (int64_t b = 0; b < B; ++b) {
    if (conv && conv[b]) {
      std::copy(bp_corr + b * n, bp_corr + (b + 1) * n, out_osdw + b * n);
      if (out_osd0) std::copy(bp_corr + b * n, bp_corr + (b + 1) * n, out_osd0 + b * n);
      if (stats) stats[4 * b] = 1, stats[4 * b + 1] = stats[4 * b + 2] = stats[4 * b + 3] = 0;
    } else {
      todo.push_back(b);
    }
  }
  int T = threads;
  if (T <= 0) {
    const char* e = std::getenv("OMP_NUM_THREADS");
    T = e ? std::atoi(e) : 0;
    if (T <= 0) T = (int)std::max(1u, std::thread::hardware_concurrency());
  }
  T = (int)std::min<int64_t>(T, (int64_t)todo.size());
  if (T <= 0) return 0;
  auto run = [&](int t) {
    LsdWork K;
    for (size_t a = t; a < todo.size(); a += T) {
      const int64_t b = todo[a];
      lsd_one(*osd, K, synd + b * m, post + b * n, out_osd0 ? out_osd0 + b * n : nullptr, out_osdw + b * n,
              stats ? stats + 4 * b : nullptr);
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

extern "C" {

int qldpc_osd_create_lsd_order(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                               const double* channel_probs, int32_t bits_per_step, int32_t lsd_method,
                               int32_t lsd_order, qldpc_osd** out) {
  if (!row_ptr || !out) return set_err(QLDPC_EINVAL, "NULL argument");
  if (m < 0 || n <= 0) return set_err(QLDPC_EINVAL, "bad matrix shape");
  if (!col_idx && row_ptr[m] > 0) return set_err(QLDPC_EINVAL, "NULL argument");
  if (bits_per_step < 1) return set_err(QLDPC_EINVAL, "bits_per_step must be >= 1");
  if (lsd_method < 0 || lsd_method > 2)
    return set_err(QLDPC_EINVAL, "lsd_method must be 0 (lsd_0), 1 (lsd_e) or 2 (lsd_cs)");
  if (lsd_order < 0 || (lsd_method == 1 && lsd_order > 12) || (lsd_method == 2 && lsd_order > 64))
    return set_err(QLDPC_EINVAL, "lsd_order must be >= 0, <= 12 for lsd_e and <= 64 for lsd_cs");
  const int w = lsd_method ? lsd_order : 0;
  bool priors = channel_probs != nullptr;
  for (int j = 0; priors && j < n; ++j) priors = channel_probs[j] > 0.0 && channel_probs[j] < 1.0;
  if (w > 0 && !priors) return set_err(QLDPC_EINVAL, "LSD of order > 0 needs channel_probs in (0, 1)");
  auto* O = new qldpc_osd();
  O->lsd_method = w ? lsd_method : 0;
  O->lsd_w = w;
  if (priors) {
    O->lsd_wq.resize(n);
    for (int j = 0; j < n; ++j) {
      const double q = std::floor(std::log(1.0 / channel_probs[j]) * 4294967296.0 + 0.5);
      O->lsd_wq[j] = q < 5.6e14 ? (long long)q : (1LL << 49);  // (1 / p overflows for a denormal p)
    }
  }
  O->m = m;
  O->n = n;
  O->method = 0;
  O->order = 0;
  O->lsd_k = bits_per_step;
  O->col_rows.assign(n, {});
  O->row_ptr.assign(row_ptr, row_ptr + m + 1);
  O->col_idx.assign(col_idx, col_idx + (col_idx ? row_ptr[m] : 0));
  for (int i = 0; i < m; ++i)
    for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
      const int j = col_idx[e];
      if (j < 0 || j >= n) {
        delete O;
        return set_err(QLDPC_EINVAL, "column index out of range");
      }
      O->col_rows[j].push_back(i);
    }
  O->w.assign(n, 0.0);  // the OSD weights stay unused: LSD weighs its candidates by lsd_wq
  O->rank = lsd_rank(*O);
  *out = O;
  return 0;
}

int qldpc_osd_create_lsd(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                         int32_t bits_per_step, qldpc_osd** out) {
  return qldpc_osd_create_lsd_order(m, n, row_ptr, col_idx, nullptr, bits_per_step, 0, 0, out);
}

int qldpc_lsd_weights(const qldpc_osd* osd, int64_t* wq) {
  if (!osd || !osd->lsd_k || !wq) return set_err(QLDPC_EINVAL, "not an LSD stage, or NULL argument");
  if (osd->lsd_wq.empty()) return set_err(QLDPC_EINVAL, "the stage was created without channel_probs in (0, 1)");
  std::copy(osd->lsd_wq.begin(), osd->lsd_wq.end(), wq);
  return 0;
}

int qldpc_lsd_decode_batch_stats(const qldpc_osd* osd, const uint8_t* synd, const double* post, const uint8_t* conv,
                                 const uint8_t* bp_corr, uint8_t* out, int32_t* stats, int64_t B, int32_t threads) {
  if (!osd || !osd->lsd_k) return set_err(QLDPC_EINVAL, "not an LSD stage (qldpc_osd_create_lsd)");
  return qldpc_rt::lsd_decode_batch_host(osd, synd, post, conv, bp_corr, nullptr, out, stats, B, threads);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// GPU stage: one 256-thread workgroup per non-converged syndrome, persistent over the batch, the whole
// decode inside the kernel.
//   sort    : the LDS bitonic sort of osd_gpu_kernel on (orderable posterior bits, index) -> rank16
//   state   : active-column / active-row bitsets, a slot per active row (the image's bit index),
//             32-bit row labels (minimum row index of the cluster, by min-label propagation over the
//             active columns), per-cluster nomination words keyed by the label
//   round   : labels; the rows with a reduced-syndrome bit mark their labels invalid; k passes of
//             atomicMin((rank << 13) | column) over the boundary of each invalid cluster, each pass
//             above the cluster's previous pick; the picked columns join once (atomicOr on a pending
//             bitset), their rows take slots, and each column is inserted into the basis
//   solution: the active columns ordered by rank (a rank bitset and its prefix popcounts), re-inserted
//             with combination words; x = the reduced syndrome's combination, cleared on the clusters
//             that are still inconsistent
// The image (slot -> row, kept column, pivot as 16-bit words, then cap vectors of 2 * cap / 64 words:
// row part | combination part) lives in LDS with a row capacity `cap` cut at create time; a syndrome
// whose active rows outgrow it is decoded again from the start on the workgroup's HBM slice, whose
// capacity is m.  The law does not depend on the order of insertions, so both give the same answer.
// No static __shared__: every byte is in the dynamic allocation counted by lsd_layout.
// ---------------------------------------------------------------------------------------------------
namespace {

constexpr int kLsdThreads = 256;
constexpr int kLsdMaxN = 8192;
constexpr int kLsdPer = kLsdMaxN / kLsdThreads;  // columns per thread at the envelope
constexpr uint32_t kInf = 0xFFFFFFFFu;
constexpr size_t kLdsMax = (size_t)160 * 1024;

struct LsdLay {
  int rank16, rlabel, nom, prev, rslot, acols, inA, pend, posb, inR, inv, scan, vbuf, sred, ctl, fre, img;
  size_t sort_end;
};

inline size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

// ord: a handle of order > 0, which also counts free columns per label (fre)
LsdLay lsd_layout(int m, int n, int NP, bool ord) {
  LsdLay L;
  const int RWh = (m + 63) / 64 > 0 ? (m + 63) / 64 : 1;
  size_t o = 0;
  L.rank16 = (int)o; o = al16(o + (size_t)n * 2);
  L.sort_end = o + (size_t)NP * 12;  // skey | sidx: dead before the tables below are initialised
  L.rlabel = (int)o; o = al16(o + (size_t)m * 4);
  L.nom = (int)o; o = al16(o + (size_t)m * 4);
  L.prev = (int)o; o = al16(o + (size_t)m * 2);
  L.rslot = (int)o; o = al16(o + (size_t)m * 2);
  L.acols = (int)o; o = al16(o + (size_t)n * 2);
  const size_t nb = (size_t)((n + 31) / 32) * 4, mb = (size_t)((m + 31) / 32) * 4;
  L.inA = (int)o; o = al16(o + nb);
  L.pend = (int)o; o = al16(o + nb);
  L.posb = (int)o; o = al16(o + nb);
  L.inR = (int)o; o = al16(o + mb);
  L.inv = (int)o; o = al16(o + mb);
  L.scan = (int)o; o = al16(o + (size_t)kLsdThreads * 4);
  L.vbuf = (int)o; o = al16(o + (size_t)RWh * 16);
  L.sred = (int)o; o = al16(o + (size_t)RWh * 16);
  L.ctl = (int)o; o = al16(o + 64);
  L.fre = (int)o; o = al16(o + (ord ? (size_t)m * 4 : 0));
  L.img = (int)o;
  return L;
}

// bytes of an image of row capacity cap (a multiple of 64) that keeps dcap dep vectors (order > 0: cap / 64
// words and a 16-bit column each, behind the basis vectors; 0 at order 0)
inline size_t lsd_img_bytes(int cap, int dcap) {
  return (((size_t)cap * 6 + 15) & ~(size_t)15) + (size_t)cap * (cap / 64) * 16 + (size_t)dcap * (cap / 64) * 8 +
         al16((size_t)dcap * 2);
}

// the LDS image keeps as many dep vectors as rows; more free columns than that take the HBM slice (n of them)
inline size_t lsd_lds_total(const LsdLay& L, int cap, bool ord) {
  return std::max(L.sort_end, (size_t)L.img + (cap ? lsd_img_bytes(cap, ord ? cap : 0) : 0));
}

// largest row capacity (multiple of 64, <= m rounded up) whose workgroup fits the budget
int lsd_cap_fit(const LsdLay& L, int m, size_t budget, bool ord) {
  for (int cap = (m + 63) / 64 * 64; cap >= 64; cap -= 64)
    if (lsd_lds_total(L, cap, ord) <= budget) return cap;
  return 0;
}

struct LsdArgs {
  const int32_t *rp, *ci, *cp, *ce;
  const uint8_t* synd;
  const double* post;
  const uint8_t* conv;
  const long long* shot;
  const uint8_t* bp_corr;
  uint8_t *out0, *outw;
  int32_t* stats;
  unsigned char* ws;  // per workgroup: an image of capacity cap_h
  unsigned long long* retries;  // decodes that outgrew the LDS image and ran again on the HBM slice
  long long ws_bytes, B;
  int m, n, NP, k, cap_l, cap_h;
  LsdLay L;
  // order > 0: wq [n] (read-only, global), the method (1 lsd_e, 2 lsd_cs), the order, dep vectors per image
  const long long* wq;
  int method, w, dcap_l, dcap_h;
};

__device__ inline u64 lsd_ord_key(double x) {
  if (x == 0.0) x = 0.0;  // -0 ties +0, as std::stable_sort's `<` has it
  const u64 u = (u64)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

enum { C_NR = 0, C_NNEW, C_CH, C_NOM, C_UNS, C_NCL, C_NF };

struct LsdCtx {
  const LsdArgs* A;
  uint16_t *rank16, *prev, *rslot, *acols;
  uint32_t *rlabel, *nom, *inA, *pend, *posb, *inR, *inv, *scan, *ctl;
  u64 *vbuf, *sred;
  // the image
  uint16_t *slotrow, *keptcol, *piv;
  u64* vec;
  int cap, S;  // S: words of a vector's row part = of its combination part
  int nvec, RW, CW;
  // order > 0: free columns per label; the free columns of the solution pass in column order, dep(f) over
  // the kept slots (S words each)
  uint32_t* fre;
  u64* dep;
  uint16_t* depcol;
  int dcap, nf;
};

__device__ inline bool bit32(const uint32_t* b, int i) { return (b[i >> 5] >> (i & 31)) & 1u; }

// Insert column c; comb: the solution pass (combination bit, kept column recorded; ORD: a dependent column
// leaves its combination of kept columns as a dep vector).  Uniform.
template <bool ORD>
__device__ __forceinline__ void lsd_insert(LsdCtx& X, int c, bool comb) {
  const int tid = threadIdx.x, TB = kLsdThreads;
  const int S = X.S, RW = X.RW, nvec = X.nvec, VS = 2 * S;
  const int32_t* cp = X.A->cp;
  const int32_t* ce = X.A->ce;
  __syncthreads();  // the previous insertion's readers of vbuf / sred are done
  // full rank on every row the image can hold: the column is dependent (ORD: its dep is still wanted; it
  // takes no combination bit of its own)
  const bool full = nvec >= X.cap;
  if (full && !(ORD && comb)) return;
  if (comb && !full && (nvec >> 6) + 1 > X.CW) {  // a new combination word: zero it in the older vectors
    for (int i = tid; i < nvec; i += TB) X.vec[(size_t)i * VS + S + X.CW] = 0;
    if (tid == 0) X.sred[S + X.CW] = 0;
    X.CW += 1;
  }
  const int CW = comb ? X.CW : 0;
  for (int q = tid; q < RW; q += TB) X.vbuf[q] = 0;
  for (int q = tid; q < CW; q += TB) X.vbuf[S + q] = 0;
  __syncthreads();
  uint32_t* v32 = reinterpret_cast<uint32_t*>(X.vbuf);
  for (int e = cp[c] + tid; e < cp[c + 1]; e += TB) {
    const int s = X.rslot[ce[e]];
    atomicOr(&v32[s >> 5], 1u << (s & 31));
  }
  if (comb && !full && tid == 0) X.vbuf[S + (nvec >> 6)] = 1ull << (nvec & 63);
  __syncthreads();
  // reduce by the vectors whose pivot bit the column has (tested before any xor lands)
  uint32_t hit = 0;
  for (int i = tid, j = 0; i < nvec; i += TB, ++j) {
    const int p = X.piv[i];
    if ((X.vbuf[p >> 6] >> (p & 63)) & 1ull) hit |= 1u << j;
  }
  __syncthreads();
  for (int i = tid, j = 0; i < nvec; i += TB, ++j)
    if ((hit >> j) & 1u) {
      const u64* bv = X.vec + (size_t)i * VS;
      for (int q = 0; q < RW; ++q)
        if (bv[q]) atomicXor(&X.vbuf[q], bv[q]);
      for (int q = 0; q < CW; ++q)
        if (bv[S + q]) atomicXor(&X.vbuf[S + q], bv[S + q]);
    }
  __syncthreads();
  int p = -1;
  for (int q = 0; q < RW; ++q) {
    const u64 w = X.vbuf[q];
    if (w) {
      p = q * 64 + __builtin_ctzll(w);
      break;
    }
  }
  if (p < 0) {  // dependent on the basis (uniform)
    if (ORD && comb) {
      const int f = X.nf;
      X.nf = f + 1;  // counted past dcap too: the decode is then taken again on the HBM slice
      if (f < X.dcap) {
        for (int q = tid; q < S; q += TB) {
          u64 d = q < CW ? X.vbuf[S + q] : 0ull;
          if (!full && q == (nvec >> 6)) d &= ~(1ull << (nvec & 63));
          X.dep[(size_t)f * S + q] = d;
        }
        if (tid == 0) X.depcol[f] = (uint16_t)c;
      }
    }
    return;
  }
  const bool sp = (X.sred[p >> 6] >> (p & 63)) & 1ull;
  __syncthreads();
  for (int i = tid; i < nvec; i += TB) {
    u64* bv = X.vec + (size_t)i * VS;
    if ((bv[p >> 6] >> (p & 63)) & 1ull) {
      for (int q = 0; q < RW; ++q) bv[q] ^= X.vbuf[q];
      for (int q = 0; q < CW; ++q) bv[S + q] ^= X.vbuf[S + q];
    }
  }
  u64* nv = X.vec + (size_t)nvec * VS;
  for (int q = tid; q < RW; q += TB) {
    nv[q] = X.vbuf[q];
    if (sp) X.sred[q] ^= X.vbuf[q];
  }
  for (int q = tid; q < CW; q += TB) {
    nv[S + q] = X.vbuf[S + q];
    if (sp) X.sred[S + q] ^= X.vbuf[S + q];
  }
  if (tid == 0) {
    X.piv[nvec] = (uint16_t)p;
    if (comb) X.keptcol[nvec] = (uint16_t)c;
  }
  X.nvec = nvec + 1;
}

// the reduced syndrome starts as s on the seed rows, which hold slots [0, ns)
__device__ inline void lsd_seed_syndrome(LsdCtx& X, int ns, int RW) {
  for (int q = threadIdx.x; q < RW; q += kLsdThreads) {
    const int lo = q * 64;
    X.sred[q] = ns >= lo + 64 ? ~0ull : ns > lo ? (1ull << (ns - lo)) - 1ull : 0ull;
  }
}

// The dep entries of candidate c (1-based, the law's order) of a cluster with nF free columns, T of them in
// the search set: lsd_e (method 1) sets bit i of `mask` for T[i]; lsd_cs gives one or two positions e0 < e1
// of the cluster's list (e1 < 0: a single).
__device__ inline void lsd_candidate(int method, int c, int nF, int T, uint32_t& mask, int& e0, int& e1) {
  mask = 0;
  e0 = e1 = -1;
  if (method == 1) {
    mask = (uint32_t)c;
  } else if (c <= nF) {
    e0 = c - 1;
  } else {
    int r = c - nF - 1, a = 0;
    while (r >= T - 1 - a) r -= T - 1 - a, ++a;
    e0 = a;
    e1 = a + 1 + r;
  }
}

// xor of word q of the candidate's dep vectors; fl: the cluster's entries in column order
__device__ inline u64 lsd_cand_word(const LsdCtx& X, const uint16_t* fl, uint32_t mask, int e0, int e1, int q) {
  u64 D = 0;
  for (uint32_t mm = mask; mm; mm &= mm - 1) D ^= X.dep[(size_t)fl[__builtin_ctz(mm)] * X.S + q];
  if (e0 >= 0) D ^= X.dep[(size_t)fl[e0] * X.S + q];
  if (e1 >= 0) D ^= X.dep[(size_t)fl[e1] * X.S + q];
  return D;
}

// The candidate search (order > 0) after the solution pass: the valid clusters that have a free column, one
// after another in the order of their first free column.  Thread 0 lists the cluster's free columns (they
// lie in column order in dep); the candidates are spread over the threads, each weighed by its difference to
// candidate 0 (sum wq over its free columns, and over the kept slots of its xor of dep vectors -wq where
// candidate 0 is set, +wq where it is not), and reduced to (least difference, least index): candidate 0 has
// (0, 0), so only a strictly lighter candidate replaces it and the first of equals wins.  The winner's xor
// goes into the comb part of vbuf, its free columns into pend.  nom[L] = 0 marks a cluster as searched
// (every word of nom is kInf after the rounds).  Uniform; ends with a barrier.
__device__ __forceinline__ void lsd_search(LsdCtx& X) {
  const LsdArgs& A = *X.A;
  const int tid = threadIdx.x, TB = kLsdThreads;
  const int nf = X.nf, S = X.S, CW = X.CW;
  uint16_t* fl = X.acols;  // (the solution pass was the last reader of acols)
  long long* red = reinterpret_cast<long long*>(X.scan);
  for (int i0 = 0; i0 < nf; ++i0) {
    const uint32_t L = X.rlabel[A.ce[A.cp[X.depcol[i0]]]];
    const bool skip = bit32(X.inv, (int)L) || X.nom[L] != kInf;
    __syncthreads();  // every thread has read nom[L] and is done with the cluster before
    if (skip) continue;
    if (tid == 0) {
      int cnt = 0;
      for (int i = i0; i < nf; ++i)
        if (X.rlabel[A.ce[A.cp[X.depcol[i]]]] == L) fl[cnt++] = (uint16_t)i;
      X.ctl[C_NF] = (uint32_t)cnt;
      X.nom[L] = 0;
    }
    __syncthreads();
    const int nF = (int)X.ctl[C_NF], T = min(A.w, nF);
    const int ncand = A.method == 1 ? (1 << T) - 1 : nF + T * (T - 1) / 2;
    long long bw = 0;
    int bc = 0;
    for (int c = 1 + tid; c <= ncand; c += TB) {
      uint32_t mask;
      int e0, e1;
      lsd_candidate(A.method, c, nF, T, mask, e0, e1);
      long long d = 0;
      for (uint32_t mm = mask; mm; mm &= mm - 1) d += A.wq[X.depcol[fl[__builtin_ctz(mm)]]];
      if (e0 >= 0) d += A.wq[X.depcol[fl[e0]]];
      if (e1 >= 0) d += A.wq[X.depcol[fl[e1]]];
      for (int q = 0; q < CW; ++q) {
        const u64 x0 = X.sred[S + q];
        for (u64 D = lsd_cand_word(X, fl, mask, e0, e1, q); D; D &= D - 1) {
          const int b = __builtin_ctzll(D);
          const long long wt = A.wq[X.keptcol[q * 64 + b]];
          d += ((x0 >> b) & 1ull) ? -wt : wt;
        }
      }
      if (d < bw) bw = d, bc = c;  // c ascends: the first of a thread's equals stays
    }
    for (int off = 32; off > 0; off >>= 1) {
      const long long ow_ = __shfl_xor(bw, off);
      const int oc = __shfl_xor(bc, off);
      if (ow_ < bw || (ow_ == bw && oc < bc)) bw = ow_, bc = oc;
    }
    if ((tid & 63) == 0) red[2 * (tid >> 6)] = bw, red[2 * (tid >> 6) + 1] = bc;
    __syncthreads();
    for (int v = 0; v < TB / 64; ++v) {
      const long long ow_ = red[2 * v];
      const int oc = (int)red[2 * v + 1];
      if (ow_ < bw || (ow_ == bw && oc < bc)) bw = ow_, bc = oc;
    }
    if (bc) {
      uint32_t mask;
      int e0, e1;
      lsd_candidate(A.method, bc, nF, T, mask, e0, e1);
      for (int q = tid; q < CW; q += TB) X.vbuf[S + q] ^= lsd_cand_word(X, fl, mask, e0, e1, q);
      if (tid == 0) {
        for (uint32_t mm = mask; mm; mm &= mm - 1) {
          const int f = X.depcol[fl[__builtin_ctz(mm)]];
          X.pend[f >> 5] |= 1u << (f & 31);
        }
        if (e0 >= 0) X.pend[X.depcol[fl[e0]] >> 5] |= 1u << (X.depcol[fl[e0]] & 31);
        if (e1 >= 0) X.pend[X.depcol[fl[e1]] >> 5] |= 1u << (X.depcol[fl[e1]] & 31);
      }
    }
  }
  __syncthreads();
}

// One syndrome on the image at `img` of row capacity cap and dcap dep vectors.  false: the active rows
// outgrew cap, or the free columns dcap (nothing was written).  Uniform over the workgroup.
template <bool ORD>
__device__ __forceinline__ bool lsd_decode(LsdCtx& X, unsigned char* img, int cap, int dcap, const uint8_t* synd, uint8_t* ow,
                           uint8_t* o0, int32_t* stats) {
  const LsdArgs& A = *X.A;
  const int tid = threadIdx.x, TB = kLsdThreads;
  const int m = A.m, n = A.n, k = A.k;
  X.cap = cap;
  X.S = cap / 64;
  X.slotrow = reinterpret_cast<uint16_t*>(img);
  X.keptcol = X.slotrow + cap;
  X.piv = X.keptcol + cap;
  X.vec = reinterpret_cast<u64*>(img + (((size_t)cap * 6 + 15) & ~(size_t)15));
  if (ORD) {
    X.dep = X.vec + (size_t)cap * 2 * X.S;
    X.depcol = reinterpret_cast<uint16_t*>(X.dep + (size_t)dcap * X.S);
    X.dcap = dcap;
    X.nf = 0;
  }
  const int nbw = (n + 31) / 32, mbw = (m + 31) / 32;
  __syncthreads();
  for (int i = tid; i < m; i += TB) {
    X.rlabel[i] = (uint32_t)i;
    X.nom[i] = kInf;
    X.prev[i] = 0;
    X.rslot[i] = 0xFFFF;
  }
  for (int q = tid; q < nbw; q += TB) X.inA[q] = X.pend[q] = X.posb[q] = 0;
  for (int q = tid; q < mbw; q += TB) X.inR[q] = X.inv[q] = 0;
  if (tid < 16) X.ctl[tid] = 0;
  __syncthreads();
  for (int i = tid; i < m; i += TB)
    if (synd[i] & 1u) {
      const uint32_t s = atomicAdd(&X.ctl[C_NR], 1u);
      if ((int)s < cap) {
        X.rslot[i] = (uint16_t)s;
        X.slotrow[s] = (uint16_t)i;
      }
      atomicOr(&X.inR[i >> 5], 1u << (i & 31));
    }
  __syncthreads();
  const int ns = (int)X.ctl[C_NR];
  int nR = ns, nA = 0, rounds = 0;
  if (ns > cap) return false;
  if (ns == 0) {
    for (int j = tid; j < n; j += TB) {
      ow[j] = 0;
      if (o0) o0[j] = 0;
    }
    if (stats && tid == 0) stats[0] = 1, stats[1] = stats[2] = stats[3] = 0;
    return true;
  }
  X.nvec = 0;
  X.CW = 0;
  X.RW = (nR + 63) / 64;
  lsd_seed_syndrome(X, ns, X.RW);
  for (;;) {
    // labels: minimum row index of the cluster
    for (;;) {
      if (tid == 0) X.ctl[C_CH] = 0;
      __syncthreads();
      for (int a = tid; a < nA; a += TB) {
        const int c = X.acols[a];
        uint32_t lc = kInf;
        for (int e = A.cp[c]; e < A.cp[c + 1]; ++e) lc = min(lc, X.rlabel[A.ce[e]]);
        for (int e = A.cp[c]; e < A.cp[c + 1]; ++e)
          if (X.rlabel[A.ce[e]] > lc) {
            atomicMin(&X.rlabel[A.ce[e]], lc);
            X.ctl[C_CH] = 1;
          }
      }
      __syncthreads();
      const uint32_t ch = X.ctl[C_CH];
      __syncthreads();
      if (!ch) break;
    }
    // invalid clusters; every cluster may pick from rank 0 again
    for (int q = tid; q < mbw; q += TB) X.inv[q] = 0;
    for (int q = tid; q < nbw; q += TB) X.pend[q] = 0;
    for (int s = tid; s < nR; s += TB) {
      X.prev[X.slotrow[s]] = 0;
      if (ORD) X.fre[X.slotrow[s]] = 0;
    }
    __syncthreads();
    for (int s = tid; s < nR; s += TB)
      if ((X.sred[s >> 6] >> (s & 63)) & 1ull) {
        const uint32_t L = X.rlabel[X.slotrow[s]];
        atomicOr(&X.inv[L >> 5], 1u << (L & 31));
      }
    if (ORD) {
      // free(C) by label: active columns less basis vectors; a valid cluster with fewer than w nominates too
      // (inv holds the nominating labels until the round ends; it is formed anew after the last one)
      for (int a = tid; a < nA; a += TB) atomicAdd(&X.fre[X.rlabel[A.ce[A.cp[X.acols[a]]]]], 1u);
      for (int i = tid; i < X.nvec; i += TB) atomicSub(&X.fre[X.rlabel[X.slotrow[X.piv[i]]]], 1u);
      __syncthreads();
      for (int s = tid; s < nR; s += TB) {
        const uint32_t L = X.rlabel[X.slotrow[s]];
        if ((int)X.fre[L] < A.w) atomicOr(&X.inv[L >> 5], 1u << (L & 31));
      }
    }
    __syncthreads();
    for (int pass = 0; pass < k; ++pass) {
      for (int s = tid; s < nR; s += TB) {
        const int i = X.slotrow[s];
        const uint32_t L = X.rlabel[i];
        if (!bit32(X.inv, (int)L)) continue;
        const uint32_t pv = X.prev[L];
        for (int e = A.rp[i]; e < A.rp[i + 1]; ++e) {
          const int c = A.ci[e];
          const uint32_t r = X.rank16[c];
          if (!bit32(X.inA, c) && r >= pv) atomicMin(&X.nom[L], (r << 13) | (uint32_t)c);
        }
      }
      if (tid == 0) X.ctl[C_NOM] = 0;
      __syncthreads();
      for (int s = tid; s < nR; s += TB) {
        const int i = X.slotrow[s];
        const uint32_t key = X.nom[i];
        if (key == kInf) continue;  // (only a cluster's root row is ever a key)
        X.nom[i] = kInf;
        X.prev[i] = (uint16_t)((key >> 13) + 1u);
        X.ctl[C_NOM] = 1;
        const int c = (int)(key & 8191u);
        const uint32_t old = atomicOr(&X.pend[c >> 5], 1u << (c & 31));
        if (!((old >> (c & 31)) & 1u)) X.acols[nA + (int)atomicAdd(&X.ctl[C_NNEW], 1u)] = (uint16_t)c;
      }
      __syncthreads();
      const uint32_t nom = X.ctl[C_NOM];
      __syncthreads();
      if (!nom) break;  // boundaries are exhausted: later passes would find nothing
    }
    const int nnew = (int)X.ctl[C_NNEW];
    if (nnew == 0) break;
    ++rounds;
    // the picked columns join A, their rows join R and take slots
    for (int a = nA + tid; a < nA + nnew; a += TB) {
      const int c = X.acols[a];
      atomicOr(&X.inA[c >> 5], 1u << (c & 31));
      for (int e = A.cp[c]; e < A.cp[c + 1]; ++e) {
        const int r = A.ce[e];
        const uint32_t old = atomicOr(&X.inR[r >> 5], 1u << (r & 31));
        if (!((old >> (r & 31)) & 1u)) {
          const uint32_t s = atomicAdd(&X.ctl[C_NR], 1u);
          if ((int)s < cap) {
            X.rslot[r] = (uint16_t)s;
            X.slotrow[s] = (uint16_t)r;
          }
        }
      }
    }
    __syncthreads();
    nR = (int)X.ctl[C_NR];
    if (nR > cap) return false;
    const int RWn = (nR + 63) / 64;
    if (RWn > X.RW) {  // new row words: zero in the older vectors and the reduced syndrome
      for (int i = tid; i < X.nvec; i += TB)
        for (int q = X.RW; q < RWn; ++q) X.vec[(size_t)i * 2 * X.S + q] = 0;
      for (int q = X.RW + tid; q < RWn; q += TB) X.sred[q] = 0;
      X.RW = RWn;
    }
    if (tid == 0) X.ctl[C_NNEW] = 0;
    for (int a = nA; a < nA + nnew; ++a) lsd_insert<ORD>(X, X.acols[a], false);
    nA += nnew;
    __syncthreads();
  }
  // the labels are those of the final clusters (the last round added nothing)
  // A in column order: a bitset over ranks, its prefix popcounts, each column to its place
  for (int a = tid; a < nA; a += TB) {
    const uint32_t r = X.rank16[X.acols[a]];
    atomicOr(&X.posb[r >> 5], 1u << (r & 31));
  }
  __syncthreads();
  X.scan[tid] = tid < nbw ? (uint32_t)__popc(X.posb[tid]) : 0u;
  __syncthreads();
  for (int off = 1; off < TB; off <<= 1) {
    const uint32_t v = tid >= off ? X.scan[tid - off] : 0u;
    __syncthreads();
    X.scan[tid] += v;
    __syncthreads();
  }
  uint32_t place[kLsdPer];
#pragma unroll
  for (int j = 0; j < kLsdPer; ++j) {
    const int a = tid + j * TB;
    place[j] = kInf;
    if (a < nA) {
      const uint32_t c = X.acols[a], r = X.rank16[c], w = r >> 5;
      const uint32_t before = (w ? X.scan[w - 1] : 0u) + (uint32_t)__popc(X.posb[w] & ((1u << (r & 31)) - 1u));
      place[j] = (before << 16) | c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kLsdPer; ++j)
    if (place[j] != kInf) X.acols[place[j] >> 16] = (uint16_t)(place[j] & 0xFFFFu);
  __syncthreads();
  X.nvec = 0;
  X.CW = 0;
  lsd_seed_syndrome(X, ns, X.RW);
  for (int a = 0; a < nA; ++a) lsd_insert<ORD>(X, X.acols[a], true);
  __syncthreads();
  if (ORD && X.nf > X.dcap) return false;
  // clusters still inconsistent are unsolvable: x = 0 on them
  for (int q = tid; q < mbw; q += TB) X.inv[q] = 0;
  __syncthreads();
  for (int s = tid; s < nR; s += TB) {
    const int i = X.slotrow[s];
    if (X.rlabel[i] == (uint32_t)i) atomicAdd(&X.ctl[C_NCL], 1u);
    if ((X.sred[s >> 6] >> (s & 63)) & 1ull) {
      const uint32_t L = X.rlabel[i];
      atomicOr(&X.inv[L >> 5], 1u << (L & 31));
      X.ctl[C_UNS] = 1;
    }
  }
  if (ORD) {
    // the winners: the kept slots start as candidate 0 (the comb part of vbuf is free now), the winning free
    // columns are collected in pend; the clusters are then searched one after another
    for (int q = tid; q < X.CW; q += TB) X.vbuf[X.S + q] = X.sred[X.S + q];
    for (int q = tid; q < nbw; q += TB) X.pend[q] = 0;
    __syncthreads();
    if (X.nf > 0) lsd_search(X);
    for (int j = tid; j < n; j += TB) {
      ow[j] = bit32(X.pend, j) ? 1 : 0;
      if (o0) o0[j] = 0;
    }
    __syncthreads();
    for (int t = tid; t < X.nvec; t += TB) {
      const bool b0 = (X.sred[X.S + (t >> 6)] >> (t & 63)) & 1ull, bw = (X.vbuf[X.S + (t >> 6)] >> (t & 63)) & 1ull;
      if (!b0 && !bw) continue;
      const int c = X.keptcol[t];
      if (!bit32(X.inv, (int)X.rlabel[A.ce[A.cp[c]]])) {
        if (bw) ow[c] = 1;
        if (o0 && b0) o0[c] = 1;
      }
    }
  } else {
    for (int j = tid; j < n; j += TB) {
      ow[j] = 0;
      if (o0) o0[j] = 0;
    }
    __syncthreads();
    for (int t = tid; t < X.nvec; t += TB)
      if ((X.sred[X.S + (t >> 6)] >> (t & 63)) & 1ull) {
        const int c = X.keptcol[t];
        if (!bit32(X.inv, (int)X.rlabel[A.ce[A.cp[c]]])) {
          ow[c] = 1;
          if (o0) o0[c] = 1;
        }
      }
  }
  if (stats && tid == 0) {
    stats[0] = X.ctl[C_UNS] ? 0 : 1;
    stats[1] = rounds;
    stats[2] = nA;
    stats[3] = (int32_t)X.ctl[C_NCL];
  }
  return true;
}

template <bool ORD>
__global__ void __launch_bounds__(kLsdThreads) lsd_gpu_kernel(LsdArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, TB = kLsdThreads;
  const int m = A.m, n = A.n, NP = A.NP;
  LsdCtx X;
  X.A = &A;
  X.rank16 = reinterpret_cast<uint16_t*>(smem + A.L.rank16);
  X.rlabel = reinterpret_cast<uint32_t*>(smem + A.L.rlabel);
  X.nom = reinterpret_cast<uint32_t*>(smem + A.L.nom);
  X.prev = reinterpret_cast<uint16_t*>(smem + A.L.prev);
  X.rslot = reinterpret_cast<uint16_t*>(smem + A.L.rslot);
  X.acols = reinterpret_cast<uint16_t*>(smem + A.L.acols);
  X.inA = reinterpret_cast<uint32_t*>(smem + A.L.inA);
  X.pend = reinterpret_cast<uint32_t*>(smem + A.L.pend);
  X.posb = reinterpret_cast<uint32_t*>(smem + A.L.posb);
  X.inR = reinterpret_cast<uint32_t*>(smem + A.L.inR);
  X.inv = reinterpret_cast<uint32_t*>(smem + A.L.inv);
  X.scan = reinterpret_cast<uint32_t*>(smem + A.L.scan);
  X.vbuf = reinterpret_cast<u64*>(smem + A.L.vbuf);
  X.sred = reinterpret_cast<u64*>(smem + A.L.sred);
  X.ctl = reinterpret_cast<uint32_t*>(smem + A.L.ctl);
  if (ORD) X.fre = reinterpret_cast<uint32_t*>(smem + A.L.fre);
  u64* skey = reinterpret_cast<u64*>(smem + A.L.rlabel);  // the sort tables, under the state tables
  int32_t* sidx = reinterpret_cast<int32_t*>(skey + NP);
  unsigned char* gimg = A.ws + (size_t)blockIdx.x * A.ws_bytes;
  for (long long b = blockIdx.x; b < A.B; b += gridDim.x) {
    uint8_t* ow = A.outw + b * (long long)n;
    uint8_t* o0 = A.out0 ? A.out0 + b * (long long)n : nullptr;
    int32_t* stats = A.stats ? A.stats + 4 * b : nullptr;
    if (A.shot && A.shot[b] < 0) continue;  // captured decode that converged at max_iter
    if (A.conv && A.conv[b]) {
      for (int j = tid; j < n; j += TB) {
        const uint8_t v = A.bp_corr[b * (long long)n + j];
        ow[j] = v;
        if (o0) o0[j] = v;
      }
      if (stats && tid == 0) stats[0] = 1, stats[1] = stats[2] = stats[3] = 0;
      continue;
    }
    const double* post = A.post + b * (long long)n;
    const uint8_t* synd = A.synd + b * (long long)m;
    __syncthreads();  // the previous syndrome's readers of the state tables are done
    for (int q = tid; q < NP; q += TB) {
      skey[q] = q < n ? lsd_ord_key(post[q]) : ~0ull;
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
    for (int q = tid; q < n; q += TB) X.rank16[sidx[q]] = (uint16_t)q;
    // (lsd_decode opens with a barrier before it writes the tables over the sort)
    bool done = false;
    if (A.cap_l) done = lsd_decode<ORD>(X, smem + A.L.img, A.cap_l, A.dcap_l, synd, ow, o0, stats);
    if (!done) {
      if (A.cap_l && tid == 0) atomicAdd(A.retries, 1ull);
      lsd_decode<ORD>(X, gimg, A.cap_h, A.dcap_h, synd, ow, o0, stats);
    }
  }
}

}  // namespace

int qldpc_rt::lsd_gpu_threads() { return kLsdThreads; }

int qldpc_rt::lsd_gpu_from_host(const qldpc_graph* g, const qldpc_osd* O, qldpc_osd_gpu** out) {
  if (!g || !O || !out || !O->lsd_k) return set_err(QLDPC_EINVAL, "NULL argument");
  if (g->n > kLsdMaxN || g->m > kLsdMaxN) return set_err(QLDPC_ENOTSUP, "GPU LSD: m or n > 8192");
  auto* G = new qldpc_osd_gpu();
  G->host = *O;
  G->device = g->device;
  const int m = g->m, n = g->n;
  G->NP = 1;
  while (G->NP < n) G->NP <<= 1;
  const bool ord = O->lsd_w > 0;
  const LsdLay L = lsd_layout(m, n, G->NP, ord);
  // the LDS image: within 64 KiB per workgroup (two or more workgroups per CU) when that holds every row
  // or at least 128 of them, else up to 128 rows in a workgroup of any size; QLDPC_LSD_WS=1: HBM alone
  const char* ws_env = std::getenv("QLDPC_LSD_WS");
  int cap = 0;
  if (!(ws_env && std::atoi(ws_env) == 1) && m > 0) {
    cap = lsd_cap_fit(L, m, (size_t)64 * 1024, ord);
    if (cap < 128 && cap < (m + 63) / 64 * 64) cap = std::min(lsd_cap_fit(L, m, kLdsMax, ord), 128);
  }
  G->lsd_cap = cap;
  G->lds = lsd_lds_total(L, cap, ord);
  const int cap_h = std::max(64, (m + 63) / 64 * 64);
  G->ws_words = (long long)((lsd_img_bytes(cap_h, ord ? n : 0) + 7) / 8);
  auto fail = [&](int code) {
    qldpc_osd_gpu_destroy(G);
    return code;
  };
  if (G->lds > kLdsMax) return fail(set_err(QLDPC_ENOTSUP, "GPU LSD: tables exceed LDS"));
  if (hipSetDevice(g->device) != hipSuccess) return fail(set_err(QLDPC_EHIP, "hipSetDevice"));
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g->device) != hipSuccess || cus <= 0)
    return fail(set_err(QLDPC_EHIP, "device CU count"));
  int nb = 0;
  const void* kern = ord ? reinterpret_cast<const void*>(&lsd_gpu_kernel<true>)
                         : reinterpret_cast<const void*>(&lsd_gpu_kernel<false>);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, kLsdThreads, G->lds) != hipSuccess || nb <= 0)
    nb = 1;
  // the HBM slices (every workgroup has one: the LDS image's overflow route) within 256 MiB
  const long long slice = G->ws_words * 8;
  G->grid = (int)std::max<long long>(1, std::min<long long>((long long)cus * nb, (256ll << 20) / slice));
  const size_t E = g->col_idx.size();
  std::vector<int32_t> cp(n + 1, 0), ce(std::max<size_t>(E, 1), 0);
  for (int j = 0; j < n; ++j) {
    cp[j + 1] = cp[j] + (int)g->col_rows[j].size();
    std::copy(g->col_rows[j].begin(), g->col_rows[j].end(), ce.begin() + cp[j]);
  }
  int rc = 0;
  if ((rc = G->rp.alloc((size_t)(m + 1) * 4)) || (rc = G->ci.alloc(std::max<size_t>(E, 1) * 4)) ||
      (rc = G->cp.alloc((size_t)(n + 1) * 4)) || (rc = G->ce.alloc(std::max<size_t>(E, 1) * 4)) ||
      (rc = G->ws.alloc((size_t)G->grid * slice)) || (rc = G->lsd_retries.alloc(8)) ||
      (ord && (rc = G->lsd_wq.alloc((size_t)n * 8))))
    return fail(rc);
  if (ord && hipMemcpy(G->lsd_wq.p, O->lsd_wq.data(), (size_t)n * 8, hipMemcpyHostToDevice) != hipSuccess)
    return fail(set_err(QLDPC_EHIP, "upload LSD weights"));
  if (hipMemset(G->lsd_retries.p, 0, 8) != hipSuccess) return fail(set_err(QLDPC_EHIP, "clear LSD retry counter"));
  if (hipMemcpy(G->rp.p, g->row_ptr.data(), (size_t)(m + 1) * 4, hipMemcpyHostToDevice) != hipSuccess ||
      (E && hipMemcpy(G->ci.p, g->col_idx.data(), E * 4, hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(G->cp.p, cp.data(), (size_t)(n + 1) * 4, hipMemcpyHostToDevice) != hipSuccess ||
      (E && hipMemcpy(G->ce.p, ce.data(), E * 4, hipMemcpyHostToDevice) != hipSuccess))
    return fail(set_err(QLDPC_EHIP, "upload LSD graph"));
  *out = G;
  return 0;
}

int qldpc_rt::lsd_gpu_launch(qldpc_osd_gpu* osd, const uint8_t* d_synd, const double* d_post, const uint8_t* d_conv,
                             const long long* d_shot, const uint8_t* d_bp_corr, uint8_t* d_out0, uint8_t* d_outw,
                             int32_t* d_stats, int64_t B, void* stream) {
  if (!osd || !osd->host.lsd_k || (B > 0 && (!d_synd || !d_post || !d_outw)))
    return set_err(QLDPC_EINVAL, "NULL argument");
  if (d_conv && !d_bp_corr) return set_err(QLDPC_EINVAL, "conv needs bp_corr");
  if (B <= 0) return 0;
  QLDPC_HIP(hipSetDevice(osd->device));
  LsdArgs a;
  a.rp = static_cast<const int32_t*>(osd->rp.p);
  a.ci = static_cast<const int32_t*>(osd->ci.p);
  a.cp = static_cast<const int32_t*>(osd->cp.p);
  a.ce = static_cast<const int32_t*>(osd->ce.p);
  a.synd = d_synd; a.post = d_post; a.conv = d_conv; a.shot = d_shot; a.bp_corr = d_bp_corr;
  a.out0 = d_out0; a.outw = d_outw; a.stats = d_stats;
  a.ws = static_cast<unsigned char*>(osd->ws.p);
  a.ws_bytes = osd->ws_words * 8;
  a.retries = static_cast<unsigned long long*>(osd->lsd_retries.p);
  a.B = B;
  a.m = osd->host.m; a.n = osd->host.n; a.NP = osd->NP; a.k = osd->host.lsd_k;
  a.cap_l = osd->lsd_cap;
  a.cap_h = std::max(64, (a.m + 63) / 64 * 64);
  const bool ord = osd->host.lsd_w > 0;
  a.L = lsd_layout(a.m, a.n, a.NP, ord);
  a.wq = static_cast<const long long*>(osd->lsd_wq.p);
  a.method = osd->host.lsd_method; a.w = osd->host.lsd_w;
  a.dcap_l = ord ? a.cap_l : 0;
  a.dcap_h = ord ? a.n : 0;
  const int grid = (int)std::min<long long>(B, osd->grid);
  if (ord)
    hipLaunchKernelGGL(lsd_gpu_kernel<true>, dim3(grid), dim3(kLsdThreads), osd->lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(lsd_gpu_kernel<false>, dim3(grid), dim3(kLsdThreads), osd->lds, (hipStream_t)stream, a);
  QLDPC_HIP(hipGetLastError());
  return 0;
}

extern "C" {

int qldpc_osd_gpu_create_lsd_order(const qldpc_graph* g, const double* channel_probs, int32_t bits_per_step,
                                   int32_t lsd_method, int32_t lsd_order, qldpc_osd_gpu** out) {
  if (!g || !out) return set_err(QLDPC_EINVAL, "NULL argument");
  qldpc_osd* O = nullptr;
  int rc = qldpc_osd_create_lsd_order(g->m, g->n, g->row_ptr.data(), g->col_idx.data(), channel_probs, bits_per_step,
                                      lsd_method, lsd_order, &O);
  if (rc) return rc;
  rc = qldpc_rt::lsd_gpu_from_host(g, O, out);
  qldpc_osd_destroy(O);
  return rc;
}

int qldpc_osd_gpu_create_lsd(const qldpc_graph* g, int32_t bits_per_step, qldpc_osd_gpu** out) {
  return qldpc_osd_gpu_create_lsd_order(g, nullptr, bits_per_step, 0, 0, out);
}

int qldpc_lsd_gpu_decode(qldpc_osd_gpu* osd, const uint8_t* d_synd, const double* d_post, const uint8_t* d_conv,
                         const uint8_t* d_bp_corr, uint8_t* d_out, int32_t* d_stats, int64_t B, void* stream) {
  if (!osd || !osd->host.lsd_k) return set_err(QLDPC_EINVAL, "not an LSD handle (qldpc_osd_gpu_create_lsd)");
  return qldpc_rt::lsd_gpu_launch(osd, d_synd, d_post, d_conv, nullptr, d_bp_corr, nullptr, d_out, d_stats, B, stream);
}

// the LDS row capacity of the active image (0: HBM alone) and the LDS bytes per workgroup (tests, DESIGN)
int qldpc_lsd_gpu_info(const qldpc_osd_gpu* osd, int32_t* lds_rows, int32_t* lds_bytes) {
  if (!osd || !osd->host.lsd_k) return set_err(QLDPC_EINVAL, "not an LSD handle (qldpc_osd_gpu_create_lsd)");
  if (lds_rows) *lds_rows = osd->lsd_cap;
  if (lds_bytes) *lds_bytes = (int32_t)osd->lds;
  return 0;
}


// decodes since the last call that outgrew the LDS image and were decoded again on the HBM slice
// (tools/lsd_compare.py); waits for the device
int qldpc_lsd_gpu_retries(qldpc_osd_gpu* osd, uint64_t* count) {
  if (!osd || !osd->host.lsd_k || !count) return set_err(QLDPC_EINVAL, "not an LSD handle, or NULL argument");
  QLDPC_HIP(hipSetDevice(osd->device));
  QLDPC_HIP(hipDeviceSynchronize());
  unsigned long long v = 0;
  QLDPC_HIP(hipMemcpy(&v, osd->lsd_retries.p, 8, hipMemcpyDeviceToHost));
  QLDPC_HIP(hipMemset(osd->lsd_retries.p, 0, 8));
  *count = v;
  return 0;
}

}  // extern "C"

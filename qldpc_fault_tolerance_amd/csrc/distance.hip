// distance.hip — random information-set minimum-distance search (qldpc_dist_*).
//
// One trial: order the n columns by a Philox key, run a greedy Gauss-Jordan of the generator matrix
// G (rows x n, with the pairing bits P = G L^T riding along as extra columns) over the columns in
// that order, and take the lexicographic minimum of (weight, pivot position) over the reduced rows
// that hold a pivot and (when P is given) have non-zero pairing.  The reduced row set is unique for
// a pivot set, so neither the row that takes a pivot nor the grid shape can change an output.
//
// qldpc_dist_run_host is the contract written out in word-packed C++ (one thread, no HIP call): the
// checker of the kernel and the path for matrices outside its envelope.
//
// dist_kernel<WT>: one workgroup per trial, persistent over the trials blockIdx.x + i * gridDim.x.
// Thread r keeps row r (code words, then pairing words, WT u64 in all) in registers through the whole
// elimination, as osd.hip's register-row mode does.  The column order comes from a bitonic sort of
// (key << 32 | column) in LDS.  Per visited column: a ballot picks each wave's first eligible row,
// which publishes its words in the wave's slot of this step's parity and bids its row number with an
// LDS atomic minimum; after ONE barrier every thread knows the winner, and the rows with the bit set
// xor the winner's published words (broadcast LDS reads) into their registers.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "runtime.h"

using qldpc_rt::set_err;
typedef unsigned long long u64;

namespace {

constexpr uint32_t kStreamDistance = 0x51D50005u;
constexpr uint32_t kNoCand = 0x7FFFFFFFu;
constexpr int kDistMaxThreads = 1024;  // rows of the device envelope (one row per thread)
constexpr int kDistMaxWords = 28;      // code + pairing words per row: 56 of the 128 VGPRs at 1024 threads
constexpr int kDistSortMax = 2048;     // columns of the LDS sort (kDistMaxWords * 64 = 1792 fit)
constexpr int kDistIdxBits = 11;       // pivot positions < 2048 in the (weight, position) key

// first output word of Philox4x32-10 (Salmon et al., SC'11; the generator of bp_kernels.h and
// oracle_philox4x32_10) for counter (c, t_lo, t_hi, stream tag) and key (seed_lo, seed_hi)
__host__ __device__ inline uint32_t dist_key(u64 seed, u64 trial, uint32_t col) {
  uint32_t c0 = col, c1 = (uint32_t)trial, c2 = (uint32_t)(trial >> 32), c3 = kStreamDistance;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int r = 0; r < 10; ++r) {
    const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

struct DistArgs {
  const u64* g;     // [rows][WT] rows (code words, pairing words, zero padding)
  int32_t* tmin;    // [trials] per-trial minimum weight (kNoCand: no candidate)
  u64* best;        // [grid][2] the workgroup's best (weight, trial)
  u64* wit;         // [grid][wn] its witness row
  u64 seed, trial_begin;
  long long trials;
  int rows, n, wn, np, has_pair;
};

// word qc (uniform) of a register row: a compare-select chain the compiler keeps in VGPRs
template <int WT>
__device__ __attribute__((always_inline)) inline u64 dist_pick(const u64 (&row)[WT], int qc) {
  u64 w = 0;
#pragma unroll
  for (int q = 0; q < WT; ++q)
    if (q == qc) w = row[q];
  return w;
}

template <int WT>
__global__ void __launch_bounds__(kDistMaxThreads) dist_kernel(DistArgs A) {
  __shared__ u64 s_sort[kDistSortMax];
  __shared__ u64 s_wslot[2][kDistMaxThreads / 64][WT];
  __shared__ int s_piv[3];
  __shared__ uint32_t s_min;
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x, lane = tid & 63, wave = tid >> 6;
  const int rows = A.rows, n = A.n, wn = A.wn, np = A.np;
  uint32_t bestw = kNoCand;
  if (tid == 0) {
    A.best[2 * (size_t)blockIdx.x] = kNoCand;
    A.best[2 * (size_t)blockIdx.x + 1] = 0;
  }
  for (long long ti = blockIdx.x; ti < A.trials; ti += gridDim.x) {
    const u64 t = A.trial_begin + (u64)ti;
    // 1. column keys and their order
    for (int c = tid; c < np; c += nthr)
      s_sort[c] = c < n ? ((u64)dist_key(A.seed, t, (uint32_t)c) << 32) | (u64)c : ~0ull;
    if (tid < 3) s_piv[tid] = 0x7FFFFFFF;
    if (tid == 0) s_min = kNoCand;
    __syncthreads();
    for (int k = 2; k <= np; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < np; i += nthr) {
          const int l = i ^ j;
          if (l > i) {
            const u64 a = s_sort[i], b = s_sort[l];
            if ((a > b) == ((i & k) == 0)) {
              s_sort[i] = b;
              s_sort[l] = a;
            }
          }
        }
        __syncthreads();
      }
    // 2. greedy Gauss-Jordan in that order, row tid in registers
    u64 row[WT];
#pragma unroll
    for (int q = 0; q < WT; ++q) row[q] = tid < rows ? A.g[(size_t)tid * WT + q] : 0ull;
    bool used = tid >= rows;
    int myidx = -1, npiv = 0, slot = 0, par = 0;
    for (int j = 0; j < n && npiv < rows; ++j) {  // uniform
      const uint32_t c = (uint32_t)s_sort[j];
      const bool bit = (dist_pick<WT>(row, (int)(c >> 6)) >> (c & 63u)) & 1ull;
      const u64 bal = __ballot(bit && !used);
      if (bal != 0ull && lane == __ffsll((long long)bal) - 1) {
#pragma unroll
        for (int q = 0; q < WT; ++q) s_wslot[par][wave][q] = row[q];
        atomicMin(&s_piv[slot], tid);
      }
      __syncthreads();
      const int r = s_piv[slot];
      // re-arm the slot of two steps ahead: its last readers passed this step's barrier
      if (tid == 0) s_piv[slot == 0 ? 2 : slot - 1] = 0x7FFFFFFF;
      const u64* pr = s_wslot[par][r >> 6 & (kDistMaxThreads / 64 - 1)];
      slot = slot == 2 ? 0 : slot + 1;
      par ^= 1;
      if (r == 0x7FFFFFFF) continue;  // no row left for this column (uniform)
      if (tid == r) {
        used = true;
        myidx = j;
      } else if (bit) {
        // eight words at a time: all WT loads in flight at once would double the row's registers
#pragma unroll
        for (int q0 = 0; q0 < WT; q0 += 8) {
#pragma unroll
          for (int q = q0; q < (q0 + 8 < WT ? q0 + 8 : WT); ++q) row[q] ^= pr[q];
          asm volatile("" ::: "memory");
        }
      }
      ++npiv;
    }
    // 3. candidates: rows that hold a pivot (and pair with a logical operator)
    uint32_t wgt = 0;
    u64 pairing = 0;
#pragma unroll
    for (int q = 0; q < WT; ++q) {
      if (q < wn) wgt += (uint32_t)__popcll(row[q]);
      else pairing |= row[q];
    }
    uint32_t key = (myidx >= 0 && (!A.has_pair || pairing != 0ull)) ? (wgt << kDistIdxBits) | (uint32_t)myidx : kNoCand;
    const uint32_t mykey = key;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)key, d, 64);
      key = o < key ? o : key;
    }
    if (lane == 0 && key != kNoCand) atomicMin(&s_min, key);
    __syncthreads();
    key = s_min;
    const uint32_t w = key == kNoCand ? kNoCand : key >> kDistIdxBits;
    if (tid == 0) A.tmin[ti] = (int32_t)w;
    if (w < bestw) {  // uniform; trials ascend inside a workgroup, so ties keep the earlier one
      bestw = w;
      if (mykey == key) {  // pivot positions are distinct: one thread
        for (int q = 0; q < WT; ++q)
          if (q < wn) A.wit[(size_t)blockIdx.x * wn + q] = row[q];
        A.best[2 * (size_t)blockIdx.x] = w;
        A.best[2 * (size_t)blockIdx.x + 1] = t;
      }
    }
    __syncthreads();  // s_min / s_sort are rewritten by the next trial
  }
}

const void* dist_kernel_for(int wt) {
  switch (wt) {
    case 2: return reinterpret_cast<const void*>(&dist_kernel<2>);
    case 4: return reinterpret_cast<const void*>(&dist_kernel<4>);
    case 8: return reinterpret_cast<const void*>(&dist_kernel<8>);
    case 12: return reinterpret_cast<const void*>(&dist_kernel<12>);
    case 16: return reinterpret_cast<const void*>(&dist_kernel<16>);
    case 20: return reinterpret_cast<const void*>(&dist_kernel<20>);
    case 24: return reinterpret_cast<const void*>(&dist_kernel<24>);
    case 26: return reinterpret_cast<const void*>(&dist_kernel<26>);
    case 28: return reinterpret_cast<const void*>(&dist_kernel<28>);
  }
  return nullptr;
}

int dist_template_words(int wt) {
  for (int c : {2, 4, 8, 12, 16, 20, 24, 26, 28})
    if (wt <= c) return c;
  return 0;
}

size_t dist_lds_bytes(int wtpl) {
  return sizeof(u64) * kDistSortMax + sizeof(u64) * 2 * (kDistMaxThreads / 64) * (size_t)wtpl + 4 * sizeof(int);
}

}  // namespace

struct qldpc_dist {
  int device = -1;
  int rows = 0, n = 0, k = 0;
  int wn = 0, wk = 0;  // code / pairing words per row
  bool has_pair = false;
  std::vector<u64> g;  // [rows][wn + wk]
  // device handles
  int wtpl = 0, threads = 0, cus = 0, np = 0;
  qldpc_rt::DevBuf d_g, d_tmin, d_best, d_wit;
};

extern "C" {

int qldpc_dist_create(int device, int32_t rows, int32_t n, int32_t k, const uint64_t* gen_words,
                      const uint64_t* pair_words, qldpc_dist** out) {
  if (!out) return set_err(QLDPC_EINVAL, "qldpc_dist_create: out is NULL");
  *out = nullptr;
  if (rows < 0 || n <= 0 || k < 0 || device < -1)
    return set_err(QLDPC_EINVAL, "qldpc_dist_create: need rows >= 0, n > 0, k >= 0, device >= -1");
  if (rows > 0 && !gen_words) return set_err(QLDPC_EINVAL, "qldpc_dist_create: gen_words is NULL");
  if ((k > 0) != (pair_words != nullptr))
    return set_err(QLDPC_EINVAL, "qldpc_dist_create: pair_words goes with k > 0 (and only with it)");
  qldpc_dist* h = new (std::nothrow) qldpc_dist;
  if (!h) return set_err(QLDPC_ENOMEM, "qldpc_dist_create: out of memory");
  h->device = device;
  h->rows = rows;
  h->n = n;
  h->k = k;
  h->wn = (n + 63) / 64;
  h->wk = (k + 63) / 64;
  h->has_pair = k > 0;
  const int wt = h->wn + h->wk;
  h->g.assign((size_t)rows * wt, 0ull);
  const u64 nmask = (n & 63) ? (1ull << (n & 63)) - 1ull : ~0ull;
  const u64 kmask = (k & 63) ? (1ull << (k & 63)) - 1ull : ~0ull;
  for (int r = 0; r < rows; ++r) {
    u64* dst = &h->g[(size_t)r * wt];
    for (int q = 0; q < h->wn; ++q) dst[q] = gen_words[(size_t)r * h->wn + q];
    for (int q = 0; q < h->wk; ++q) dst[h->wn + q] = pair_words[(size_t)r * h->wk + q];
    if ((dst[h->wn - 1] & ~nmask) || (h->wk && (dst[wt - 1] & ~kmask))) {
      delete h;
      return set_err(QLDPC_EINVAL, "qldpc_dist_create: bits set past column n (or pairing bit k)");
    }
  }
  if (device >= 0) {
    h->wtpl = dist_template_words(wt);
    if (rows > kDistMaxThreads || h->wtpl == 0 || rows == 0) {
      delete h;
      return set_err(QLDPC_ENOTSUP, "qldpc_dist_create: the kernel takes 1..1024 rows and at most 28 row words "
                                    "(code + pairing); use a host handle (device = -1)");
    }
    h->threads = (rows + 63) / 64 * 64;
    h->np = 2;
    while (h->np < n) h->np <<= 1;
    auto fail = [&](int rc) {
      h->d_g.release();
      delete h;
      return rc;
    };
    if (hipSetDevice(device) != hipSuccess) return fail(set_err(QLDPC_EHIP, "hipSetDevice"));
    if (hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || h->cus <= 0)
      return fail(set_err(QLDPC_EHIP, "hipDeviceGetAttribute(MultiprocessorCount)"));
    std::vector<u64> wm((size_t)rows * h->wtpl, 0ull);
    for (int r = 0; r < rows; ++r)
      for (int q = 0; q < wt; ++q) wm[(size_t)r * h->wtpl + q] = h->g[(size_t)r * wt + q];
    if (int rc = h->d_g.alloc(wm.size() * sizeof(u64))) return fail(rc);
    if (hipMemcpy(h->d_g.p, wm.data(), wm.size() * sizeof(u64), hipMemcpyHostToDevice) != hipSuccess)
      return fail(set_err(QLDPC_EHIP, "hipMemcpy(generator)"));
  }
  *out = h;
  return QLDPC_OK;
}

int qldpc_dist_destroy(qldpc_dist* h) {
  if (!h) return QLDPC_OK;
  if (h->device >= 0) {
    h->d_g.release();
    h->d_tmin.release();
    h->d_best.release();
    h->d_wit.release();
  }
  delete h;
  return QLDPC_OK;
}

int qldpc_dist_geometry(const qldpc_dist* h, int32_t* threads, int32_t* row_words, int32_t* pair_words,
                        int32_t* lds_bytes) {
  if (!h) return set_err(QLDPC_EINVAL, "qldpc_dist_geometry: NULL handle");
  if (threads) *threads = h->threads;
  if (row_words) *row_words = h->wn;
  if (pair_words) *pair_words = h->wk;
  if (lds_bytes) *lds_bytes = h->device >= 0 ? (int32_t)dist_lds_bytes(h->wtpl) : 0;
  return QLDPC_OK;
}

static int dist_check_run(const qldpc_dist* h, int64_t trials, const int32_t* best_weight, const uint64_t* best_trial,
                          const uint64_t* witness_words, const char* who) {
  if (!h || !best_weight || !best_trial || !witness_words || trials < 0)
    return set_err(QLDPC_EINVAL, std::string(who) + ": NULL handle / output or trials < 0");
  return QLDPC_OK;
}

int qldpc_dist_run_host(qldpc_dist* h, uint64_t seed, uint64_t trial_begin, int64_t trials, int32_t* trial_min,
                        int32_t* best_weight, uint64_t* best_trial, uint64_t* witness_words) {
  if (int rc = dist_check_run(h, trials, best_weight, best_trial, witness_words, "qldpc_dist_run_host")) return rc;
  const int rows = h->rows, n = h->n, wn = h->wn, wt = h->wn + h->wk;
  *best_weight = (int32_t)kNoCand;
  *best_trial = 0;
  std::memset(witness_words, 0, sizeof(uint64_t) * wn);
  std::vector<u64> ord(n), R;
  std::vector<int> pivpos(rows);
  for (int64_t ti = 0; ti < trials; ++ti) {
    const u64 t = trial_begin + (u64)ti;
    for (int c = 0; c < n; ++c) ord[c] = ((u64)dist_key(seed, t, (uint32_t)c) << 32) | (u64)c;
    std::sort(ord.begin(), ord.end());
    R = h->g;
    std::fill(pivpos.begin(), pivpos.end(), -1);
    int npiv = 0;
    for (int j = 0; j < n && npiv < rows; ++j) {
      const uint32_t c = (uint32_t)ord[j];
      const int q = (int)(c >> 6);
      const u64 m = 1ull << (c & 63u);
      int p = -1;
      for (int r = 0; r < rows; ++r)
        if (pivpos[r] < 0 && (R[(size_t)r * wt + q] & m)) {
          p = r;
          break;
        }
      if (p < 0) continue;
      pivpos[p] = j;
      ++npiv;
      const u64* src = &R[(size_t)p * wt];
      for (int r = 0; r < rows; ++r)
        if (r != p && (R[(size_t)r * wt + q] & m)) {
          u64* dst = &R[(size_t)r * wt];
          for (int x = 0; x < wt; ++x) dst[x] ^= src[x];
        }
    }
    uint32_t bw = kNoCand;
    int bi = -1, br = -1;
    for (int r = 0; r < rows; ++r) {
      if (pivpos[r] < 0) continue;
      const u64* v = &R[(size_t)r * wt];
      if (h->has_pair) {
        u64 any = 0;
        for (int x = wn; x < wt; ++x) any |= v[x];
        if (!any) continue;
      }
      uint32_t w = 0;
      for (int x = 0; x < wn; ++x) w += (uint32_t)__builtin_popcountll(v[x]);
      if (w < bw || (w == bw && pivpos[r] < bi)) {
        bw = w;
        bi = pivpos[r];
        br = r;
      }
    }
    if (trial_min) trial_min[ti] = (int32_t)bw;
    if (br >= 0 && bw < (uint32_t)*best_weight) {
      *best_weight = (int32_t)bw;
      *best_trial = t;
      std::memcpy(witness_words, &R[(size_t)br * wt], sizeof(uint64_t) * wn);
    }
  }
  return QLDPC_OK;
}

int qldpc_dist_run(qldpc_dist* h, uint64_t seed, uint64_t trial_begin, int64_t trials, int32_t workgroups,
                   int32_t* trial_min, int32_t* best_weight, uint64_t* best_trial, uint64_t* witness_words,
                   void* stream) {
  if (int rc = dist_check_run(h, trials, best_weight, best_trial, witness_words, "qldpc_dist_run")) return rc;
  if (h->device < 0) return set_err(QLDPC_EINVAL, "qldpc_dist_run: host-only handle (use qldpc_dist_run_host)");
  if (workgroups < 0) return set_err(QLDPC_EINVAL, "qldpc_dist_run: workgroups < 0");
  *best_weight = (int32_t)kNoCand;
  *best_trial = 0;
  std::memset(witness_words, 0, sizeof(uint64_t) * h->wn);
  if (trials == 0) return QLDPC_OK;
  QLDPC_HIP(hipSetDevice(h->device));
  // default grid: 1024 / threads workgroups per CU (1024 threads' worth; LDS may keep fewer resident)
  long long grid = workgroups > 0 ? workgroups : (long long)h->cus * (kDistMaxThreads / h->threads);
  if (grid > trials) grid = trials;
  if (h->d_tmin.bytes < sizeof(int32_t) * (size_t)trials) {
    h->d_tmin.release();
    if (int rc = h->d_tmin.alloc(sizeof(int32_t) * (size_t)trials)) return rc;
  }
  if (h->d_best.bytes < sizeof(u64) * 2 * (size_t)grid) {
    h->d_best.release();
    h->d_wit.release();
    if (int rc = h->d_best.alloc(sizeof(u64) * 2 * (size_t)grid)) return rc;
    if (int rc = h->d_wit.alloc(sizeof(u64) * (size_t)h->wn * (size_t)grid)) {
      h->d_best.release();  // the two are sized together: the next call allocates both again
      return rc;
    }
  }
  DistArgs a;
  a.g = (const u64*)h->d_g.p;
  a.tmin = (int32_t*)h->d_tmin.p;
  a.best = (u64*)h->d_best.p;
  a.wit = (u64*)h->d_wit.p;
  a.seed = seed;
  a.trial_begin = trial_begin;
  a.trials = trials;
  a.rows = h->rows;
  a.n = h->n;
  a.wn = h->wn;
  a.np = h->np;
  a.has_pair = h->has_pair ? 1 : 0;
  const void* fn = dist_kernel_for(h->wtpl);
  void* params[] = {&a};
  hipStream_t st = (hipStream_t)stream;
  QLDPC_HIP(hipLaunchKernel(fn, dim3((unsigned)grid), dim3((unsigned)h->threads), params, 0, st));
  std::vector<u64> best(2 * (size_t)grid), wit((size_t)h->wn * (size_t)grid);
  std::vector<int32_t> tmin_tmp;
  int32_t* tm = trial_min;
  if (!tm) {
    tmin_tmp.resize((size_t)trials);
    tm = tmin_tmp.data();
  }
  QLDPC_HIP(hipMemcpyAsync(tm, h->d_tmin.p, sizeof(int32_t) * (size_t)trials, hipMemcpyDeviceToHost, st));
  QLDPC_HIP(hipMemcpyAsync(best.data(), h->d_best.p, sizeof(u64) * best.size(), hipMemcpyDeviceToHost, st));
  QLDPC_HIP(hipMemcpyAsync(wit.data(), h->d_wit.p, sizeof(u64) * wit.size(), hipMemcpyDeviceToHost, st));
  QLDPC_HIP(hipStreamSynchronize(st));
  long long bg = -1;
  for (long long b = 0; b < grid; ++b) {
    if (best[2 * b] == kNoCand) continue;
    if (bg < 0 || best[2 * b] < best[2 * bg] || (best[2 * b] == best[2 * bg] && best[2 * b + 1] < best[2 * bg + 1]))
      bg = b;
  }
  if (bg >= 0) {
    *best_weight = (int32_t)best[2 * bg];
    *best_trial = best[2 * bg + 1];
    std::memcpy(witness_words, &wit[(size_t)bg * h->wn], sizeof(uint64_t) * h->wn);
  }
  return QLDPC_OK;
}

}  // extern "C"

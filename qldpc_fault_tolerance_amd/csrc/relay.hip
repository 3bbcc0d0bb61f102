// relay.hip — engine 7: Relay-BP (min-sum BP with a per-variable memory term, run as a chain of legs).
//
// THE LAW (the contract; tests/relay_ref.py restates it in Python, relay_decode_one below in plain
// C++).  T = double or float, every operation in T in the order of bp_ms_* (oracle/qldpc_oracle.c):
//   priors   L0_j = (T) log((1 - p_j) / p_j) (double, libm); wq_j = (int64) floor(L0_j(double) 2^32 + 0.5);
//   gammas   gam[0][j] = (T) pre_gamma; gam[r][j] = (T)(lo + (hi - lo) u), r = 1 .. R, in double, with
//            u = ((o0 >> 5) 2^26 + (o1 >> 6)) / 2^53, (o0 .. o3) = Philox4x32-10(key = (seed_lo, seed_hi),
//            ctr = (j, r, 0, 0x51D50007));
//   decode   M_j <- L0_j, nsol <- 0, bestW <- +inf, iters <- 0; for leg r = 0 .. R (T_0 = pre_iter, else
//            leg_iter): bias_j = ((T)1 - gam[r][j]) L0_j + gam[r][j] M_j (two rounded products, one
//            rounded sum: never an FMA), every bit-to-check message of column j <- bias_j; for t = 1 ..
//            T_r: the check pass of bp_ms (alpha = 1 - 2^-t when ms_scaling_factor is 0), the variable
//            pass of bp_ms with bias_j (recomputed from the current M_j) in place of the prior, M_j <-
//            the column's final sum, dec_j = (M_j <= 0), iters += 1, and the leg ends when H dec == s.
//            A converged leg is a solution: nsol += 1, W = sum of wq_j over dec_j = 1, and it becomes
//            `best` when W < bestW (strict: the earlier solution wins ties); nsol == stop_nconv stops
//            the chain.  M carries into the next leg, the messages restart from the new bias.
//   output   corr = best if nsol > 0 else the last dec; conv = (nsol > 0); iters <= T0 + R Tr.
// With R = 0 and pre_gamma = 0 the bias is L0_j + 0 M_j = L0_j exactly (M_j is finite): plain min-sum.
//
// Kernel (relay_kernel), modelled on bp_ps.hip: one decode per workgroup at a time (256 threads; 512 or
// 1024 when LDS leaves so few workgroups resident that the CU's 32 waves are not reached), workgroups
// persistent over the batch, the whole chain inside the kernel.  A thread walks a whole row in the
// check pass and a whole column (rows ascending) in the variable pass, so the sums keep bp_ms's
// order.  Per-decode state: b2c / c2b (2 E values of T, row-major edge order) in LDS when the image
// fits 160 KiB, else in a per-workgroup slice of an HBM workspace (QLDPC_RELAY_WS=1 forces that);
// M[n] (T), the solution weight (one 64-bit LDS word, integer atomics: order-free), two convergence
// flags, dec / best / syndrome bytes always in LDS; the graph's CSR / CSC beside them as 16-bit words
// when that costs no resident workgroup (QLDPC_RELAY_IDX=0: walked in global memory).  nsol, bestW
// and the iteration count are workgroup-uniform registers: every thread derives them from the same
// LDS words after a barrier,
// so leg and iteration exits are uniform and every barrier is reached by every thread.  M_j, dec_j
// and best_j are read and written by column j's thread only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <thread>
#include <vector>

#include "runtime.h"

using namespace qldpc_rt;

namespace {

constexpr int kRelayThreads = 256;     // workgroup width of graphs whose image leaves 8 workgroups per CU
constexpr int kRelayMaxThreads = 1024;  // ... widened up to this when LDS leaves fewer (qldpc_bp_create_relay)
constexpr uint32_t kStreamRelay = 0x51D50007u;

template <typename T>
struct Sentinel;
template <>
struct Sentinel<double> {
  static constexpr double v = 1e308;
};
template <>
struct Sentinel<float> {
  static constexpr float v = FLT_MAX;
};

// bias_j = (1 - g) L0 + g M: two rounded products and one rounded sum
template <typename T>
__host__ __device__ inline T relay_bias(T g, T l0, T mem) {
#pragma clang fp contract(off)
  const T a = ((T)1 - g) * l0;
  const T b = g * mem;
  return a + b;
}

template <typename T>
__host__ __device__ inline T relay_alpha(double alpha, int t) {
  return alpha == 0.0 ? (T)(1.0 - ldexp(1.0, -t)) : (T)alpha;
}

struct RelayArgs {
  const int32_t* rp;     // CSR row pointers [m+1]
  const int32_t* ci;     // CSR columns (ascending) [E]
  const int32_t* cp;     // CSC column pointers [n+1]
  const int32_t* ce;     // CSC: edge ids (row-major numbering), rows ascending [E]
  const void* llr;       // T [n]: L0 (a side decode: T [2][n], the rows of p0 and p1)
  const void* gam;       // T [num_legs + 1][n]
  const long long* wq;   // [n] integer solution weights (a side decode: [2][n])
  const uint8_t* side;   // [B][n], bit 0 selects the prior's row (a side decode), else NULL
  void* ws;              // HBM message workspace (T [grid][2E]) or NULL (messages in LDS)
  const uint8_t* synd;   // [B][m]
  uint8_t* corr;         // [B][n]
  int32_t* iters;        // [B] or NULL
  uint8_t* conv;         // [B] or NULL
  long long B;
  double alpha;
  int m, n, E, pre_iter, leg_iter, num_legs, stop_nconv;
  double* post;          // [B][n] or NULL: M after the last iteration (qldpc_bp_decode_batch_side_soft, num_legs = 0)
};

// LDS: [b2c, c2b: 2E x T when in LDS][M: n x T][wsum: 8][flag: 2 x 4][dec: n][best: n][syn: m]
//      [rp: m + 1][cp: n + 1][ci: E][ce: E] as I = uint16_t when the graph's indices are staged
// I = int32_t walks the CSR / CSC in global memory: every step of a row or column walk then waits
// on a dependent global load (index -> message address), 1.27x the time per iteration on
// hgp_34_n1600; the staged copy is made once per workgroup, not per syndrome.
// SIDE (qldpc_bp_decode_batch_side): variable j of syndrome b takes its prior and its solution weight
// from row side[b][j] & 1 of the two-row tables.  The bit is read once per syndrome into bit 1 of
// dec[j] (and travels into best[j] with it), so the image keeps its size and the variable pass still
// issues one global load for its prior; every reader of dec / best masks bit 0.
template <typename T, typename I, bool SIDE>
__global__ void __launch_bounds__(kRelayMaxThreads) relay_kernel(RelayArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, TB = blockDim.x;
  const int m = A.m, n = A.n, E = A.E;
  T* b2c;
  unsigned char* rest;
  if (A.ws) {
    b2c = static_cast<T*>(A.ws) + (size_t)blockIdx.x * 2 * E;
    rest = smem;
  } else {
    b2c = reinterpret_cast<T*>(smem);
    rest = smem + (size_t)2 * E * sizeof(T);
  }
  T* c2b = b2c + E;
  T* M = reinterpret_cast<T*>(rest);
  unsigned char* tail = rest + (((size_t)n * sizeof(T) + 7) & ~(size_t)7);
  unsigned long long* wsum = reinterpret_cast<unsigned long long*>(tail);
  int* flag = reinterpret_cast<int*>(tail + 8);  // [2]
  uint8_t* dec = tail + 16;
  uint8_t* best = dec + n;
  uint8_t* syn = best + n;
  const I *rp, *ci, *cp, *ce;
  if constexpr (sizeof(I) == 2) {  // (the host takes this variant only when E and n fit 16 bits)
    I* lrp = reinterpret_cast<I*>(tail + (((size_t)16 + 2 * (size_t)n + (size_t)m + 1) & ~(size_t)1));
    I* lcp = lrp + (m + 1);
    I* lci = lcp + (n + 1);
    I* lce = lci + E;
    for (int i = tid; i <= m; i += TB) lrp[i] = (I)A.rp[i];
    for (int j = tid; j <= n; j += TB) lcp[j] = (I)A.cp[j];
    for (int e = tid; e < E; e += TB) {
      lci[e] = (I)A.ci[e];
      lce[e] = (I)A.ce[e];
    }
    rp = lrp;
    cp = lcp;
    ci = lci;
    ce = lce;  // first read after the barrier that opens the first syndrome
  } else {
    rp = A.rp;
    cp = A.cp;
    ci = A.ci;
    ce = A.ce;
  }
  const T* L0 = static_cast<const T*>(A.llr);
  const T sentinel = Sentinel<T>::v;
  // the prior of variable j under the side bit its own thread keeps in dec[j]
  auto prior = [&](int j) -> T {
    if constexpr (SIDE)
      return L0[(size_t)(dec[j] >> 1) * n + j];
    else
      return L0[j];
  };
  for (long long b = blockIdx.x; b < A.B; b += gridDim.x) {
    // every per-syndrome word starts afresh: M, the flags, the weight word; nsol / bestW are registers
    // (SIDE: and the side bit of every variable, before its prior is first read)
    for (int i = tid; i < m; i += TB) syn[i] = A.synd[b * m + i] & 1;
    for (int j = tid; j < n; j += TB) {
      if constexpr (SIDE)
        dec[j] = (uint8_t)((A.side[b * n + j] & 1) << 1);
      else
        dec[j] = 0;
      M[j] = prior(j);
      best[j] = 0;
    }
    if (tid == 0) {
      flag[0] = flag[1] = 0;
      *wsum = 0ull;
    }
    int nsol = 0, total = 0, fc = 0;
    long long bestW = 0x7fffffffffffffffLL;
    __syncthreads();
    for (int r = 0; r <= A.num_legs; ++r) {
      const int Tr = r == 0 ? A.pre_iter : A.leg_iter;
      const T* gam = static_cast<const T*>(A.gam) + (size_t)r * n;
      for (int j = tid; j < n; j += TB) {
        const T bias = relay_bias<T>(gam[j], prior(j), M[j]);
        for (int k = cp[j]; k < cp[j + 1]; ++k) b2c[ce[k]] = bias;
      }
      __syncthreads();
      bool converged = false;
      for (int t = 1; t <= Tr; ++t) {
        const T alpha = relay_alpha<T>(A.alpha, t);
        // check pass, bp_ms row order: forward minima, then backward minima, sign and scale
        for (int i = tid; i < m; i += TB) {
          const int e0 = rp[i], e1 = rp[i + 1];
          T temp = sentinel;
          int sgn = syn[i];
          for (int e = e0; e < e1; ++e) {
            const T v = b2c[e];
            c2b[e] = temp;
            const T a = fabs(v);
            if (a < temp) temp = a;
            if (v <= 0) sgn += 1;
          }
          // sign of edge e = syndrome + the non-positive messages of the OTHER edges: the row's
          // total minus the edge's own (the forward + backward counts of bp_ms)
          const int all = sgn;
          temp = sentinel;
          for (int e = e1 - 1; e >= e0; --e) {
            const T v = b2c[e];
            T c = c2b[e];
            if (temp < c) c = temp;
            const int s = all - (v <= 0 ? 1 : 0);
            c2b[e] = c * ((s & 1) ? -alpha : alpha);
            const T a = fabs(v);
            if (a < temp) temp = a;
          }
        }
        __syncthreads();
        // variable pass, rows ascending: prefix sums from the bias, then suffix sums
        for (int j = tid; j < n; j += TB) {
          const int k0 = cp[j], k1 = cp[j + 1];
          T temp = relay_bias<T>(gam[j], prior(j), M[j]);
          for (int k = k0; k < k1; ++k) {
            const int e = ce[k];
            b2c[e] = temp;
            temp += c2b[e];
          }
          M[j] = temp;
          if constexpr (SIDE)
            dec[j] = (uint8_t)((dec[j] & 2) | (temp <= 0 ? 1 : 0));
          else
            dec[j] = temp <= 0 ? 1 : 0;
          temp = (T)0;
          for (int k = k1 - 1; k >= k0; --k) {
            const int e = ce[k];
            b2c[e] += temp;
            temp += c2b[e];
          }
        }
        __syncthreads();
        // H dec == s ?  (one shared flag, double-buffered over the iteration count of the decode)
        int* f = &flag[fc & 1];
        for (int i = tid; i < m; i += TB) {
          uint32_t par = syn[i];
          for (int e = rp[i]; e < rp[i + 1]; ++e) par ^= dec[ci[e]];
          if constexpr (SIDE) par &= 1u;
          if (par) *f = 1;
        }
        if (tid == 0) flag[(fc + 1) & 1] = 0;
        __syncthreads();
        ++fc;
        ++total;
        if (*f == 0) {
          converged = true;
          break;
        }
      }
      if (!converged) continue;
      // a solution: its integer weight, summed in any order
      ++nsol;
      long long part = 0;
      for (int j = tid; j < n; j += TB) {
        if constexpr (SIDE) {
          if (dec[j] & 1) part += A.wq[(size_t)(dec[j] >> 1) * n + j];
        } else {
          if (dec[j]) part += A.wq[j];
        }
      }
      if (part != 0) atomicAdd(wsum, (unsigned long long)part);
      __syncthreads();
      const long long W = (long long)*wsum;
      if (W < bestW) {
        bestW = W;
        for (int j = tid; j < n; j += TB) best[j] = dec[j];
      }
      __syncthreads();
      if (tid == 0) *wsum = 0ull;  // read again only after the barriers of another leg
      if (nsol >= A.stop_nconv) break;
    }
    for (int j = tid; j < n; j += TB) {
      if constexpr (SIDE)
        A.corr[b * n + j] = (nsol > 0 ? best[j] : dec[j]) & 1;
      else
        A.corr[b * n + j] = nsol > 0 ? best[j] : dec[j];
      // soft output: M is the LDS word the last variable pass left (no leg follows: num_legs = 0)
      if (A.post) A.post[b * n + j] = (double)M[j];
    }
    if (tid == 0) {
      if (A.iters) A.iters[b] = total;
      if (A.conv) A.conv[b] = nsol > 0 ? 1 : 0;
    }
    __syncthreads();
  }
}

// Philox4x32-10 on the host (oracle_philox4x32_10)
void philox_host(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t o[4]) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

int check_params(int64_t n, int32_t pre_iter, double pre_gamma, int32_t num_legs, int32_t leg_iter, double gamma_lo,
                 double gamma_hi, int32_t stop_nconv, int32_t precision) {
  if (n < 0) return set_err(QLDPC_EINVAL, "n < 0");
  if (precision != 32 && precision != 64) return set_err(QLDPC_EINVAL, "precision must be 32 or 64");
  if (pre_iter < 1) return set_err(QLDPC_EINVAL, "relay: pre_iter must be >= 1");
  if (num_legs < 0) return set_err(QLDPC_EINVAL, "relay: num_legs must be >= 0");
  if (num_legs > 0 && leg_iter < 1) return set_err(QLDPC_EINVAL, "relay: leg_iter must be >= 1 when num_legs > 0");
  if (stop_nconv < 1) return set_err(QLDPC_EINVAL, "relay: stop_nconv must be >= 1");
  if (!std::isfinite(pre_gamma) || !std::isfinite(gamma_lo) || !std::isfinite(gamma_hi))
    return set_err(QLDPC_EINVAL, "relay: memory strengths must be finite");
  if (gamma_lo > gamma_hi) return set_err(QLDPC_EINVAL, "relay: gamma_lo > gamma_hi");
  return 0;
}

double relay_gamma(int j, int r, double pre_gamma, double lo, double hi, uint64_t seed) {
  if (r == 0) return pre_gamma;
  uint32_t o[4];
  philox_host((uint32_t)j, (uint32_t)r, 0u, kStreamRelay, (uint32_t)seed, (uint32_t)(seed >> 32), o);
  const double u = (double)(((uint64_t)(o[0] >> 5) << 26) | (uint64_t)(o[1] >> 6)) * (1.0 / 9007199254740992.0);
  return lo + (hi - lo) * u;
}

// the tables of a decoder in T: L0, gammas [R + 1][n], integer weights
template <typename T>
struct RelayTables {
  std::vector<T> l0, gam;
  std::vector<long long> wq;
};

template <typename T>
void relay_priors(const double* probs, int n, std::vector<T>& l0, std::vector<long long>& wq) {
  l0.resize(n);
  wq.resize(n);
  for (int j = 0; j < n; ++j) {
    const double l = std::log((1.0 - probs[j]) / probs[j]);  // glibc log, as Cython
    l0[j] = (T)l;
    const double w = std::floor(l * 4294967296.0 + 0.5);
    // (p = 0 or 1 has no finite weight: saturate instead of converting an infinity)
    wq[j] = !(w < 4.6e18) ? (1LL << 62) : !(w > -4.6e18) ? -(1LL << 62) : (long long)w;
  }
}

template <typename T>
void relay_gam_table(int n, double pre_gamma, int R, double lo, double hi, uint64_t seed, std::vector<T>& gam) {
  gam.resize((size_t)(R + 1) * n);
  for (int r = 0; r <= R; ++r)
    for (int j = 0; j < n; ++j) gam[(size_t)r * n + j] = (T)relay_gamma(j, r, pre_gamma, lo, hi, seed);
}

struct HostGraph {
  int m, n, E;
  const int32_t *rp, *ci;
  std::vector<int32_t> cp, ce;
};

struct RelayParams {
  int pre_iter, num_legs, leg_iter, stop_nconv;
  double alpha;
};

// THE LAW for one syndrome, sequential loops in the oracle's order
template <typename T>
void relay_decode_one(const HostGraph& g, const RelayParams& P, const RelayTables<T>& tb, const uint8_t* synd,
                      uint8_t* corr, int32_t* iters, uint8_t* conv, int32_t* nsol_out, std::vector<T>& b2c,
                      std::vector<T>& c2b, std::vector<int>& sg, std::vector<T>& M, std::vector<uint8_t>& dec,
                      std::vector<uint8_t>& best) {
  const int m = g.m, n = g.n;
  const T sentinel = Sentinel<T>::v;
  for (int j = 0; j < n; ++j) {
    M[j] = tb.l0[j];
    dec[j] = 0;
  }
  int nsol = 0, total = 0;
  long long bestW = std::numeric_limits<long long>::max();
  for (int r = 0; r <= P.num_legs; ++r) {
    const int Tr = r == 0 ? P.pre_iter : P.leg_iter;
    const T* gam = tb.gam.data() + (size_t)r * n;
    for (int j = 0; j < n; ++j) {
      const T bias = relay_bias<T>(gam[j], tb.l0[j], M[j]);
      for (int k = g.cp[j]; k < g.cp[j + 1]; ++k) b2c[g.ce[k]] = bias;
    }
    bool converged = false;
    for (int t = 1; t <= Tr; ++t) {
      const T alpha = relay_alpha<T>(P.alpha, t);
      for (int i = 0; i < m; ++i) {
        const int e0 = g.rp[i], e1 = g.rp[i + 1];
        T temp = sentinel;
        int sgn = (synd[i] & 1) ? 1 : 0;
        for (int e = e0; e < e1; ++e) {
          c2b[e] = temp;
          sg[e] = sgn;
          const T a = std::fabs(b2c[e]);
          if (a < temp) temp = a;
          if (b2c[e] <= 0) sgn += 1;
        }
        temp = sentinel;
        sgn = 0;
        for (int e = e1 - 1; e >= e0; --e) {
          if (temp < c2b[e]) c2b[e] = temp;
          sg[e] += sgn;
          c2b[e] *= ((sg[e] & 1) ? -alpha : alpha);
          const T a = std::fabs(b2c[e]);
          if (a < temp) temp = a;
          if (b2c[e] <= 0) sgn += 1;
        }
      }
      for (int j = 0; j < n; ++j) {
        const int k0 = g.cp[j], k1 = g.cp[j + 1];
        T temp = relay_bias<T>(gam[j], tb.l0[j], M[j]);
        for (int k = k0; k < k1; ++k) {
          const int e = g.ce[k];
          b2c[e] = temp;
          temp += c2b[e];
        }
        M[j] = temp;
        dec[j] = temp <= 0 ? 1 : 0;
        temp = (T)0;
        for (int k = k1 - 1; k >= k0; --k) {
          const int e = g.ce[k];
          b2c[e] += temp;
          temp += c2b[e];
        }
      }
      ++total;
      bool ok = true;
      for (int i = 0; i < m && ok; ++i) {
        uint8_t a = synd[i] & 1;
        for (int e = g.rp[i]; e < g.rp[i + 1]; ++e) a ^= dec[g.ci[e]];
        ok = a == 0;
      }
      if (ok) {
        converged = true;
        break;
      }
    }
    if (!converged) continue;
    ++nsol;
    long long W = 0;
    for (int j = 0; j < n; ++j)
      if (dec[j]) W += tb.wq[j];
    if (W < bestW) {
      bestW = W;
      std::copy(dec.begin(), dec.begin() + n, best.begin());
    }
    if (nsol >= P.stop_nconv) break;
  }
  std::copy(nsol > 0 ? best.begin() : dec.begin(), (nsol > 0 ? best.begin() : dec.begin()) + n, corr);
  if (iters) *iters = total;
  if (conv) *conv = nsol > 0 ? 1 : 0;
  if (nsol_out) *nsol_out = nsol;
}

// probs1 / side non-NULL: the side law, each syndrome's L0 and weights selected from the tables of
// probs (side bit 0) and probs1 (side bit 1) before the same per-syndrome routine runs
template <typename T>
void relay_decode_host_t(const HostGraph& g, const RelayParams& P, const double* probs, const double* probs1,
                         const uint8_t* side, double pre_gamma, double lo, double hi, uint64_t seed,
                         const uint8_t* synd, uint8_t* corr, int32_t* iters, uint8_t* conv, int32_t* nsol, int64_t B,
                         int threads) {
  RelayTables<T> tb, tb1;
  relay_priors<T>(probs, g.n, tb.l0, tb.wq);
  if (side) relay_priors<T>(probs1, g.n, tb1.l0, tb1.wq);
  relay_gam_table<T>(g.n, pre_gamma, P.num_legs, lo, hi, seed, tb.gam);
  std::atomic<int64_t> next(0);
  auto work = [&]() {
    const size_t E = (size_t)std::max(1, g.E), n1 = (size_t)g.n + 1;
    std::vector<T> b2c(E), c2b(E), M(n1);
    std::vector<int> sg(E);
    std::vector<uint8_t> dec(n1), best(n1);
    RelayTables<T> sel;
    if (side) sel = tb;
    for (int64_t b = next.fetch_add(1); b < B; b = next.fetch_add(1)) {
      if (side) {
        const uint8_t* sb = side + (size_t)b * g.n;
        for (int j = 0; j < g.n; ++j) {
          const RelayTables<T>& from = (sb[j] & 1) ? tb1 : tb;
          sel.l0[j] = from.l0[j];
          sel.wq[j] = from.wq[j];
        }
      }
      relay_decode_one<T>(g, P, side ? sel : tb, synd + (size_t)b * g.m, corr + (size_t)b * g.n,
                          iters ? iters + b : nullptr, conv ? conv + b : nullptr, nsol ? nsol + b : nullptr, b2c, c2b,
                          sg, M, dec, best);
    }
  };
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(threads, B));
  if (nt == 1) {
    work();
    return;
  }
  std::vector<std::thread> pool;
  for (int t = 0; t < nt; ++t) pool.emplace_back(work);
  for (auto& t : pool) t.join();
}

size_t relay_lds(int precision, int m, int n, int E, bool lds_messages, bool lds_index) {
  const size_t ts = precision == 32 ? 4 : 8;
  size_t tail = (((size_t)n * ts + 7) & ~(size_t)7) + 16 + 2 * (size_t)n + (size_t)m;
  if (lds_index) tail = ((tail + 1) & ~(size_t)1) + 2 * ((size_t)(m + 1) + (size_t)(n + 1) + 2 * (size_t)E);
  return (lds_messages ? (size_t)2 * E * ts : 0) + ((tail + 15) / 16) * 16;
}

}  // namespace

namespace qldpc_rt {

size_t relay_lds_bytes(int precision, int m, int n, int E, bool lds_messages, bool lds_index) {
  return relay_lds(precision, m, n, E, lds_messages, lds_index);
}

// 256 threads, doubled (up to 1024) while the workgroups LDS leaves resident stay within the CU's 32
// waves and there are rows or columns left to give the new threads: a graph with one resident
// workgroup would otherwise run 4 waves per CU on serial, latency-bound row and column walks
int relay_threads(size_t lds_bytes, int m, int n) {
  const size_t resident = std::max<size_t>(1, std::min<size_t>(8, (size_t)(160 * 1024) / std::max<size_t>(1, lds_bytes)));
  int tb = kRelayThreads;
  while (tb < kRelayMaxThreads && resident * (size_t)(2 * tb / 64) <= 32 && tb < std::max(m, n)) tb *= 2;
  return tb;
}

const void* relay_kernel_ptr(int precision, bool lds_index, bool side) {
  if (side) {
    if (lds_index)
      return precision == 32 ? reinterpret_cast<const void*>(&relay_kernel<float, uint16_t, true>)
                             : reinterpret_cast<const void*>(&relay_kernel<double, uint16_t, true>);
    return precision == 32 ? reinterpret_cast<const void*>(&relay_kernel<float, int32_t, true>)
                           : reinterpret_cast<const void*>(&relay_kernel<double, int32_t, true>);
  }
  if (lds_index)
    return precision == 32 ? reinterpret_cast<const void*>(&relay_kernel<float, uint16_t, false>)
                           : reinterpret_cast<const void*>(&relay_kernel<double, uint16_t, false>);
  return precision == 32 ? reinterpret_cast<const void*>(&relay_kernel<float, int32_t, false>)
                         : reinterpret_cast<const void*>(&relay_kernel<double, int32_t, false>);
}

int relay_check_params(int64_t n, int32_t pre_iter, double pre_gamma, int32_t num_legs, int32_t leg_iter,
                       double gamma_lo, double gamma_hi, int32_t stop_nconv, int32_t precision) {
  return check_params(n, pre_iter, pre_gamma, num_legs, leg_iter, gamma_lo, gamma_hi, stop_nconv, precision);
}

// L0 and the integer weights from bp->probs (creation and qldpc_bp_set_channel_probs)
int relay_upload_priors(qldpc_bp* bp) {
  const int n = bp->g->n;
  std::vector<long long> wq;
  if (bp->route.precision == 32) {
    std::vector<float> l0;
    relay_priors<float>(bp->probs.data(), n, l0, wq);
    if (n) QLDPC_HIP(hipMemcpy(bp->llr.p, l0.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  } else {
    std::vector<double> l0;
    relay_priors<double>(bp->probs.data(), n, l0, wq);
    if (n) QLDPC_HIP(hipMemcpy(bp->llr.p, l0.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  }
  if (n) QLDPC_HIP(hipMemcpy(bp->rl_wq.p, wq.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  return 0;
}

// the two-row L0 and weight tables of a side decode (qldpc_bp_set_side_probs): row 0 from p0, row 1 from p1
int relay_upload_side(qldpc_bp* bp, const double* p0, const double* p1) {
  const int n = bp->g->n;
  const size_t ts = bp->route.precision == 32 ? 4 : 8;
  int rc;
  if (!bp->side_llr.p && (rc = bp->side_llr.alloc(std::max<size_t>(1, (size_t)2 * n) * ts))) return rc;
  if (!bp->side_wq.p && (rc = bp->side_wq.alloc(std::max<size_t>(1, (size_t)2 * n) * 8))) return rc;
  const double* rows[2] = {p0, p1};
  for (int r = 0; r < 2 && n; ++r) {
    std::vector<long long> wq;
    if (bp->route.precision == 32) {
      std::vector<float> l0;
      relay_priors<float>(rows[r], n, l0, wq);
      QLDPC_HIP(hipMemcpy(static_cast<float*>(bp->side_llr.p) + (size_t)r * n, l0.data(), (size_t)n * 4,
                          hipMemcpyHostToDevice));
    } else {
      std::vector<double> l0;
      relay_priors<double>(rows[r], n, l0, wq);
      QLDPC_HIP(hipMemcpy(static_cast<double*>(bp->side_llr.p) + (size_t)r * n, l0.data(), (size_t)n * 8,
                          hipMemcpyHostToDevice));
    }
    QLDPC_HIP(hipMemcpy(static_cast<long long*>(bp->side_wq.p) + (size_t)r * n, wq.data(), (size_t)n * 8,
                        hipMemcpyHostToDevice));
  }
  return 0;
}

// the gamma table of bp's relay parameters, in T, on the device
int relay_upload_gammas(qldpc_bp* bp) {
  const int n = bp->g->n, R = bp->rl_legs;
  const size_t cnt = (size_t)(R + 1) * n;
  if (!cnt) return 0;
  if (bp->route.precision == 32) {
    std::vector<float> gam;
    relay_gam_table<float>(n, bp->rl_pre_gamma, R, bp->rl_lo, bp->rl_hi, bp->rl_seed, gam);
    QLDPC_HIP(hipMemcpy(bp->rl_gam.p, gam.data(), cnt * 4, hipMemcpyHostToDevice));
  } else {
    std::vector<double> gam;
    relay_gam_table<double>(n, bp->rl_pre_gamma, R, bp->rl_lo, bp->rl_hi, bp->rl_seed, gam);
    QLDPC_HIP(hipMemcpy(bp->rl_gam.p, gam.data(), cnt * 8, hipMemcpyHostToDevice));
  }
  return 0;
}

template <typename T, typename I>
static void relay_launch(const RelayArgs& a, dim3 grid, dim3 block, size_t lds, hipStream_t stream) {
  if (a.side)
    hipLaunchKernelGGL((relay_kernel<T, I, true>), grid, block, lds, stream, a);
  else
    hipLaunchKernelGGL((relay_kernel<T, I, false>), grid, block, lds, stream, a);
}

int relay_decode_launch(const qldpc_bp* bp, const uint8_t* synd, uint8_t* corr, int32_t* iters, uint8_t* conv,
                        int64_t B, hipStream_t stream, const uint8_t* side, double* post) {
  const qldpc_graph* g = bp->g;
  RelayArgs a;
  a.post = post;
  a.rp = static_cast<const int32_t*>(bp->ps_rp.p);
  a.ci = static_cast<const int32_t*>(bp->ps_ci.p);
  a.cp = static_cast<const int32_t*>(bp->ps_cp.p);
  a.ce = static_cast<const int32_t*>(bp->ps_ce.p);
  a.llr = side ? bp->side_llr.p : bp->llr.p;
  a.gam = bp->rl_gam.p;
  a.wq = static_cast<const long long*>(side ? bp->side_wq.p : bp->rl_wq.p);
  a.side = side;
  a.ws = bp->ps_ws.p;
  a.synd = synd;
  a.corr = corr;
  a.iters = iters;
  a.conv = conv;
  a.B = B;
  a.alpha = bp->alpha;
  a.m = g->m;
  a.n = g->n;
  a.E = g->nnz;
  a.pre_iter = bp->rl_pre_iter;
  a.leg_iter = bp->rl_leg_iter;
  a.num_legs = bp->rl_legs;
  a.stop_nconv = bp->rl_stop;
  // the workspace has one slice per workgroup of ps_grid: never launch more (side_grid <= ps_grid)
  const int grid = (int)std::max<long long>(1, std::min<long long>(B, side ? bp->side_grid : bp->ps_grid));
  const dim3 g3(grid), b3(bp->route.TB);
  const size_t lds = bp->route.lds_bytes;
  // (the side variants run on the plain variant's LDS image and workspace slices)
  if (bp->route.precision == 32) {
    if (bp->rl_idx)
      relay_launch<float, uint16_t>(a, g3, b3, lds, stream);
    else
      relay_launch<float, int32_t>(a, g3, b3, lds, stream);
  } else {
    if (bp->rl_idx)
      relay_launch<double, uint16_t>(a, g3, b3, lds, stream);
    else
      relay_launch<double, int32_t>(a, g3, b3, lds, stream);
  }
  QLDPC_HIP(hipGetLastError());
  return 0;
}

}  // namespace qldpc_rt

extern "C" {

int qldpc_relay_gammas(int32_t n, double pre_gamma, int32_t num_legs, double gamma_lo, double gamma_hi,
                       uint64_t gamma_seed, int32_t precision, double* out) {
  if (int rc = check_params(n, 1, pre_gamma, num_legs, 1, gamma_lo, gamma_hi, 1, precision)) return rc;
  if (!out && n > 0) return set_err(QLDPC_EINVAL, "NULL out");
  for (int r = 0; r <= num_legs; ++r)
    for (int j = 0; j < n; ++j) {
      const double g = relay_gamma(j, r, pre_gamma, gamma_lo, gamma_hi, gamma_seed);
      out[(size_t)r * n + j] = precision == 32 ? (double)(float)g : g;
    }
  return 0;
}

// qldpc_relay_decode_host (p1 = side = NULL) and qldpc_relay_decode_host_side
static int relay_decode_host_any(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                                 const double* channel_probs, const double* p1, const uint8_t* side, int32_t pre_iter,
                                 double pre_gamma, int32_t num_legs, int32_t leg_iter, double gamma_lo, double gamma_hi,
                                 int32_t stop_nconv, uint64_t gamma_seed, double ms_scaling_factor, int32_t precision,
                                 const uint8_t* synd, uint8_t* corr, int32_t* iters, uint8_t* conv, int32_t* nsol,
                                 int64_t B, int32_t threads) {
  if (m < 0 || n < 0 || !row_ptr || (!col_idx && row_ptr[m] > 0) || (!channel_probs && n > 0))
    return set_err(QLDPC_EINVAL, "bad graph or NULL argument");
  if (int rc = check_params(n, pre_iter, pre_gamma, num_legs, leg_iter, gamma_lo, gamma_hi, stop_nconv, precision))
    return rc;
  if (B < 0 || (B > 0 && ((!synd && m > 0) || (!corr && n > 0)))) return set_err(QLDPC_EINVAL, "NULL argument");
  HostGraph g;
  g.m = m;
  g.n = n;
  g.rp = row_ptr;
  g.ci = col_idx;
  if (row_ptr[0] != 0) return set_err(QLDPC_EINVAL, "row_ptr[0] != 0");
  for (int i = 0; i < m; ++i) {
    if (row_ptr[i + 1] < row_ptr[i]) return set_err(QLDPC_EINVAL, "row_ptr not monotone");
    for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e)
      if (col_idx[e] < 0 || col_idx[e] >= n || (e > row_ptr[i] && col_idx[e - 1] >= col_idx[e]))
        return set_err(QLDPC_EINVAL, "col_idx out of range or not strictly ascending within a row");
  }
  g.E = row_ptr[m];
  // CSC with row-major edge ids, rows ascending per column
  g.cp.assign((size_t)n + 1, 0);
  g.ce.resize((size_t)std::max(1, g.E));
  for (int e = 0; e < g.E; ++e) g.cp[col_idx[e] + 1]++;
  for (int j = 0; j < n; ++j) g.cp[j + 1] += g.cp[j];
  {
    std::vector<int32_t> fill(g.cp.begin(), g.cp.end() - 1);
    for (int i = 0; i < m; ++i)
      for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) g.ce[fill[col_idx[e]]++] = e;
  }
  if (B == 0) return 0;
  int nt = threads;
  if (nt <= 0) {
    const char* e = std::getenv("OMP_NUM_THREADS");
    nt = (e && *e) ? std::atoi(e) : (int)std::thread::hardware_concurrency();
    if (nt <= 0) nt = 1;
  }
  const RelayParams P{pre_iter, num_legs, leg_iter, stop_nconv, ms_scaling_factor};
  if (precision == 32)
    relay_decode_host_t<float>(g, P, channel_probs, p1, side, pre_gamma, gamma_lo, gamma_hi, gamma_seed, synd, corr,
                               iters, conv, nsol, B, nt);
  else
    relay_decode_host_t<double>(g, P, channel_probs, p1, side, pre_gamma, gamma_lo, gamma_hi, gamma_seed, synd, corr,
                                iters, conv, nsol, B, nt);
  return 0;
}

int qldpc_relay_decode_host(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                            const double* channel_probs, int32_t pre_iter, double pre_gamma, int32_t num_legs,
                            int32_t leg_iter, double gamma_lo, double gamma_hi, int32_t stop_nconv,
                            uint64_t gamma_seed, double ms_scaling_factor, int32_t precision, const uint8_t* synd,
                            uint8_t* corr, int32_t* iters, uint8_t* conv, int32_t* nsol, int64_t B, int32_t threads) {
  return relay_decode_host_any(m, n, row_ptr, col_idx, channel_probs, nullptr, nullptr, pre_iter, pre_gamma, num_legs,
                               leg_iter, gamma_lo, gamma_hi, stop_nconv, gamma_seed, ms_scaling_factor, precision, synd,
                               corr, iters, conv, nsol, B, threads);
}

int qldpc_relay_decode_host_side(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                                 const double* p0, const double* p1, const uint8_t* side, int32_t pre_iter,
                                 double pre_gamma, int32_t num_legs, int32_t leg_iter, double gamma_lo, double gamma_hi,
                                 int32_t stop_nconv, uint64_t gamma_seed, double ms_scaling_factor, int32_t precision,
                                 const uint8_t* synd, uint8_t* corr, int32_t* iters, uint8_t* conv, int32_t* nsol,
                                 int64_t B, int32_t threads) {
  if (n > 0 && (!p0 || !p1)) return set_err(QLDPC_EINVAL, "NULL side prior table");
  if (B > 0 && n > 0 && !side) return set_err(QLDPC_EINVAL, "NULL side bytes");
  if (int rc = side_probs_check(n, p0, p1)) return rc;
  // (n = 0: no variable selects anything, the plain routine serves)
  return relay_decode_host_any(m, n, row_ptr, col_idx, p0, n > 0 ? p1 : nullptr, n > 0 ? side : nullptr, pre_iter,
                               pre_gamma, num_legs, leg_iter, gamma_lo, gamma_hi, stop_nconv, gamma_seed,
                               ms_scaling_factor, precision, synd, corr, iters, conv, nsol, B, threads);
}

}  // extern "C"

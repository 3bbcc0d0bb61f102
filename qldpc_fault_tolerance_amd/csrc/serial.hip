// serial.hip — engine 8: min-sum BP on the serial (variable-by-variable, "layered") schedule.
//
// THE LAW (the contract; tests/serial_ref.py restates it in Python, serial_decode_one below in plain
// C++).  There is no reference counterpart.  T = double or float, every operation in T; the primitives
// are those of bp_ms_* (oracle/qldpc_oracle.c):
//   priors   L0_j = (T) log((1 - p_j) / p_j), computed in double with libm;
//   layers   layer(j) = the smallest l >= 0 such that no variable j' < j with layer(j') = l shares a
//            check with j (first-fit in ascending variable index).  The sweep order pi is the variables
//            sorted by (layer, index).  Two variables of one layer share no check, so updating a layer
//            in parallel equals the sequential sweep in order pi; the host law is that sweep;
//   start    b2c[e] = L0_col(e) for every edge;
//   iteration t = 1 .. max_iter: a_t = (T) ms_scaling_factor, or (T)(1 - 2^-t) when that is 0.  For
//            each variable j in order pi:
//            1. for each edge e of column j, rows ascending, with i = row(e): mag = the minimum of
//               |b2c[e']| over the other edges e' of row i, or the sentinel (1e308 for double, FLT_MAX
//               for float) when there is none; s = synd_i + the number of those e' with b2c[e'] <= 0;
//               c2b[e] = mag * (s odd ? -a_t : a_t);
//            2. the variable pass of bp_ms on column j alone: forward over the column's edges, temp =
//               L0_j, for each edge b2c[e] = temp, temp = temp + c2b[e]; post_j = temp, dec_j = (temp
//               <= 0); backward, temp = 0, for each edge in reverse b2c[e] = b2c[e] + temp, temp = temp
//               + c2b[e].
//            After the sweep iters = t; the decode stops with conv = 1 when H dec == synd;
//   output   corr = dec of the last sweep; iters; conv; the soft output is post_j widened to double.
// A minimum and a parity count do not depend on the order a row is walked in; the column sums keep the
// stated order.
//
// Kernel (serial_kernel), on relay_kernel's shape: one decode per workgroup at a time, workgroups
// persistent over the batch, the whole decode inside the kernel.  Only b2c lives across variables (E
// values of T, row-major edge order): in LDS when the image fits 160 KiB, else in a per-workgroup
// slice of an HBM workspace (QLDPC_SERIAL_WS=1 forces that).  A sweep is one step per layer: a thread
// takes one variable of the layer (strided when the layer is wider than the workgroup), reads the
// rows of its checks and writes its own column; the column's c2b values stay in that thread's
// registers (columns of degree > kSerialRegDeg compute them twice instead).  A barrier closes each
// layer, the convergence test closes each sweep.  The graph's CSR / CSC and the layer table sit
// beside b2c as 16-bit words when they fit that range and cost no resident workgroup
// (QLDPC_SERIAL_IDX=0: walked in global memory).  The iteration count is a workgroup-uniform
// register and the convergence flag is read by every thread after a barrier, so every exit is
// uniform and every barrier is reached by every thread.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <thread>
#include <vector>

#include "runtime.h"

using namespace qldpc_rt;

namespace {

constexpr int kSerialMaxThreads = 256;
constexpr int kSerialRegDeg = 8;  // columns up to this degree keep their c2b values in registers

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

template <typename T>
__host__ __device__ inline T serial_alpha(double alpha, int t) {
  return alpha == 0.0 ? (T)(1.0 - ldexp(1.0, -t)) : (T)alpha;
}

// step 1 of the law for edge e of row i (e0 .. e1 - 1): the other edges' minimum and parity
template <typename T>
__host__ __device__ inline T serial_c2b(const T* b2c, int e0, int e1, int e, int syn, T alpha) {
  T mag = Sentinel<T>::v;
  int s = syn;
  for (int x = e0; x < e1; ++x) {
    if (x == e) continue;
    const T v = b2c[x];
    const T a = fabs(v);
    if (a < mag) mag = a;
    if (v <= 0) s += 1;
  }
  return mag * ((s & 1) ? -alpha : alpha);
}

struct SerialArgs {
  const int32_t* rp;    // CSR row pointers [m+1]
  const int32_t* ci;    // CSR columns (ascending) [E]
  const int32_t* cp;    // CSC column pointers [n+1]
  const int32_t* ce;    // CSC: edge ids (row-major numbering), rows ascending [E]
  const int32_t* cr;    // CSC: rows [E]
  const int32_t* ord;   // the sweep order pi [n]
  const int32_t* lp;    // layer l = ord[lp[l] .. lp[l+1]) [layers + 1]
  const void* llr;      // T [n]: L0 (a side decode: T [2][n], the rows of p0 and p1)
  const uint8_t* side;  // [B][n], bit 0 selects the prior's row (a side decode), else NULL
  void* ws;             // HBM message workspace (T [grid][E]) or NULL (messages in LDS)
  const uint8_t* synd;  // [B][m]
  uint8_t* corr;        // [B][n]
  int32_t* iters;       // [B] or NULL
  uint8_t* conv;        // [B] or NULL
  double* post;         // [B][n] or NULL
  long long B;
  double alpha;
  int m, n, E, layers, max_iter, soft;
};

// LDS: [b2c: E x T when in LDS][post: n x T on a soft handle][flag: 2 x 4][dec: n][syn: m]
//      [rp: m + 1][cp: n + 1][lp: layers + 1][ord: n][ci: E][ce: E][cr: E] as I = uint16_t when the
//      graph's indices are staged; I = int32_t walks them in global memory.
// SIDE (qldpc_bp_decode_batch_side): variable j of syndrome b takes its prior from row side[b][j] & 1
// of the two-row table.  The bit is read once per syndrome into bit 1 of dec[j], so the image keeps
// its size and the variable pass still issues one global load for its prior; every reader of dec
// masks bit 0.
template <typename T, typename I, bool SIDE>
__global__ void __launch_bounds__(kSerialMaxThreads) serial_kernel(SerialArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, TB = blockDim.x;
  const int m = A.m, n = A.n, E = A.E, L = A.layers;
  T* b2c;
  unsigned char* rest;
  if (A.ws) {
    b2c = static_cast<T*>(A.ws) + (size_t)blockIdx.x * E;
    rest = smem;
  } else {
    b2c = reinterpret_cast<T*>(smem);
    rest = smem + (((size_t)E * sizeof(T) + 7) & ~(size_t)7);
  }
  T* pst = reinterpret_cast<T*>(rest);  // touched on a soft handle only
  unsigned char* tail = rest + (A.soft ? (((size_t)n * sizeof(T) + 7) & ~(size_t)7) : 0);
  int* flag = reinterpret_cast<int*>(tail);  // [2]
  uint8_t* dec = tail + 8;
  uint8_t* syn = dec + n;
  const I *rp, *ci, *cp, *ce, *cr, *ord, *lp;
  if constexpr (sizeof(I) == 2) {  // (the host takes this variant only when E, n and m fit 16 bits)
    I* lrp = reinterpret_cast<I*>(tail + (((size_t)8 + (size_t)n + (size_t)m + 1) & ~(size_t)1));
    I* lcp = lrp + (m + 1);
    I* llp = lcp + (n + 1);
    I* lord = llp + (L + 1);
    I* lci = lord + n;
    I* lce = lci + E;
    I* lcr = lce + E;
    for (int i = tid; i <= m; i += TB) lrp[i] = (I)A.rp[i];
    for (int j = tid; j <= n; j += TB) lcp[j] = (I)A.cp[j];
    for (int l = tid; l <= L; l += TB) llp[l] = (I)A.lp[l];
    for (int j = tid; j < n; j += TB) lord[j] = (I)A.ord[j];
    for (int e = tid; e < E; e += TB) {
      lci[e] = (I)A.ci[e];
      lce[e] = (I)A.ce[e];
      lcr[e] = (I)A.cr[e];
    }
    rp = lrp;
    cp = lcp;
    lp = llp;
    ord = lord;
    ci = lci;
    ce = lce;
    cr = lcr;  // first read after the barrier that opens the first syndrome
  } else {
    rp = A.rp;
    cp = A.cp;
    lp = A.lp;
    ord = A.ord;
    ci = A.ci;
    ce = A.ce;
    cr = A.cr;
  }
  const T* L0 = static_cast<const T*>(A.llr);
  for (long long b = blockIdx.x; b < A.B; b += gridDim.x) {
    for (int i = tid; i < m; i += TB) syn[i] = A.synd[b * m + i] & 1;
    if constexpr (SIDE) {
      // the side bits of this syndrome replace the previous one's before any prior is read
      const uint8_t* sb = A.side + b * n;
      for (int j = tid; j < n; j += TB) dec[j] = (uint8_t)((sb[j] & 1) << 1);
      for (int e = tid; e < E; e += TB) {
        const int j = ci[e];
        b2c[e] = L0[(size_t)(sb[j] & 1) * n + j];
      }
    } else {
      for (int e = tid; e < E; e += TB) b2c[e] = L0[ci[e]];
    }
    if (tid == 0) flag[0] = flag[1] = 0;
    int total = 0;
    bool converged = false;
    __syncthreads();
    for (int t = 1; t <= A.max_iter; ++t) {
      const T alpha = serial_alpha<T>(A.alpha, t);
      for (int l = 0; l < L; ++l) {
        const int q1 = lp[l + 1];
        for (int q = lp[l] + tid; q < q1; q += TB) {
          const int j = ord[q];
          const int k0 = cp[j], deg = cp[j + 1] - k0;
          uint8_t sbit = 0;
          if constexpr (SIDE) sbit = dec[j] & 2;
          T temp = SIDE ? L0[(size_t)(sbit >> 1) * n + j] : L0[j];
          if (deg <= kSerialRegDeg) {
            T c[kSerialRegDeg], pre[kSerialRegDeg];
#pragma unroll
            for (int kk = 0; kk < kSerialRegDeg; ++kk)
              if (kk < deg) {
                const int i = cr[k0 + kk];
                c[kk] = serial_c2b<T>(b2c, rp[i], rp[i + 1], ce[k0 + kk], syn[i], alpha);
              }
#pragma unroll
            for (int kk = 0; kk < kSerialRegDeg; ++kk)
              if (kk < deg) {
                pre[kk] = temp;
                temp += c[kk];
              }
            const T sum = temp;
            temp = (T)0;
#pragma unroll
            for (int kk = kSerialRegDeg - 1; kk >= 0; --kk)
              if (kk < deg) {
                b2c[ce[k0 + kk]] = pre[kk] + temp;
                temp += c[kk];
              }
            temp = sum;
          } else {
            // a row's other edges belong to other layers and its own edge is never read, so the
            // backward pass computes the same c2b again
            for (int k = k0; k < k0 + deg; ++k) {
              const int i = cr[k], e = ce[k];
              const T c = serial_c2b<T>(b2c, rp[i], rp[i + 1], e, syn[i], alpha);
              b2c[e] = temp;
              temp += c;
            }
            const T sum = temp;
            temp = (T)0;
            for (int k = k0 + deg - 1; k >= k0; --k) {
              const int i = cr[k], e = ce[k];
              const T c = serial_c2b<T>(b2c, rp[i], rp[i + 1], e, syn[i], alpha);
              b2c[e] += temp;
              temp += c;
            }
            temp = sum;
          }
          if (A.soft) pst[j] = temp;
          dec[j] = SIDE ? (uint8_t)(sbit | (temp <= 0 ? 1 : 0)) : (temp <= 0 ? 1 : 0);
        }
        __syncthreads();
      }
      // H dec == s ?  (one shared flag, double-buffered over the iterations of the decode)
      int* f = &flag[total & 1];
      for (int i = tid; i < m; i += TB) {
        uint32_t par = syn[i];
        for (int e = rp[i]; e < rp[i + 1]; ++e) par ^= dec[ci[e]];
        if constexpr (SIDE) par &= 1u;
        if (par) *f = 1;
      }
      if (tid == 0) flag[(total + 1) & 1] = 0;
      __syncthreads();
      ++total;
      const bool done = *f == 0;
      // this word is cleared in the next sweep's test, after that sweep's layer barriers; a graph
      // without variables has none, so every thread's read is closed by a barrier here
      if (L == 0) __syncthreads();
      if (done) {
        converged = true;
        break;
      }
    }
    for (int j = tid; j < n; j += TB) {
      A.corr[b * n + j] = SIDE ? (dec[j] & 1) : dec[j];
      if (A.post) A.post[b * n + j] = (double)pst[j];
    }
    if (tid == 0) {
      if (A.iters) A.iters[b] = total;
      if (A.conv) A.conv[b] = converged ? 1 : 0;
    }
    __syncthreads();
  }
}

int check_params(int64_t n, int32_t max_iter, int32_t precision) {
  if (n < 0) return set_err(QLDPC_EINVAL, "n < 0");
  if (precision != 32 && precision != 64) return set_err(QLDPC_EINVAL, "precision must be 32 or 64");
  if (max_iter < 1) return set_err(QLDPC_EINVAL, "serial: max_iter must be >= 1");
  return 0;
}

int check_csr(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx) {
  if (m < 0 || n < 0 || !row_ptr || (!col_idx && row_ptr[m] > 0)) return set_err(QLDPC_EINVAL, "bad graph or NULL argument");
  if (row_ptr[0] != 0) return set_err(QLDPC_EINVAL, "row_ptr[0] != 0");
  for (int i = 0; i < m; ++i) {
    if (row_ptr[i + 1] < row_ptr[i]) return set_err(QLDPC_EINVAL, "row_ptr not monotone");
    for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e)
      if (col_idx[e] < 0 || col_idx[e] >= n || (e > row_ptr[i] && col_idx[e - 1] >= col_idx[e]))
        return set_err(QLDPC_EINVAL, "col_idx out of range or not strictly ascending within a row");
  }
  return 0;
}

struct HostGraph {
  int m, n, E;
  const int32_t *rp, *ci;
  std::vector<int32_t> cp, ce, cr;  // CSC: edge ids (row-major numbering) and rows, rows ascending
};

void build_csc(HostGraph& g) {
  g.E = g.rp[g.m];
  g.cp.assign((size_t)g.n + 1, 0);
  g.ce.resize((size_t)std::max(1, g.E));
  g.cr.resize((size_t)std::max(1, g.E));
  for (int e = 0; e < g.E; ++e) g.cp[g.ci[e] + 1]++;
  for (int j = 0; j < g.n; ++j) g.cp[j + 1] += g.cp[j];
  std::vector<int32_t> fill(g.cp.begin(), g.cp.end() - 1);
  for (int i = 0; i < g.m; ++i)
    for (int e = g.rp[i]; e < g.rp[i + 1]; ++e) {
      const int k = fill[g.ci[e]]++;
      g.ce[k] = e;
      g.cr[k] = i;
    }
}

// first-fit layers in ascending variable index; returns the number of layers
int first_fit_layers(const HostGraph& g, std::vector<int32_t>& layer) {
  layer.assign((size_t)g.n, 0);
  std::vector<std::vector<int32_t>> used((size_t)g.m);  // layers taken by a check's earlier variables
  std::vector<int32_t> stamp;                           // stamp[l] == j + 1: layer l is closed to j
  int layers = 0;
  for (int j = 0; j < g.n; ++j) {
    for (int k = g.cp[j]; k < g.cp[j + 1]; ++k)
      for (int32_t l : used[g.cr[k]]) stamp[l] = j + 1;
    int l = 0;
    while (l < (int)stamp.size() && stamp[l] == j + 1) ++l;
    if (l == (int)stamp.size()) stamp.push_back(0);
    layer[j] = l;
    layers = std::max(layers, l + 1);
    for (int k = g.cp[j]; k < g.cp[j + 1]; ++k) used[g.cr[k]].push_back(l);
  }
  return layers;
}

// pi and the layer boundaries from the layer of each variable
void sweep_order(const std::vector<int32_t>& layer, int layers, std::vector<int32_t>& ord, std::vector<int32_t>& lp) {
  const int n = (int)layer.size();
  lp.assign((size_t)layers + 1, 0);
  for (int j = 0; j < n; ++j) lp[layer[j] + 1]++;
  for (int l = 0; l < layers; ++l) lp[l + 1] += lp[l];
  ord.resize((size_t)std::max(1, n));
  std::vector<int32_t> fill(lp.begin(), lp.end() - 1);
  for (int j = 0; j < n; ++j) ord[fill[layer[j]]++] = j;
}

template <typename T>
void serial_priors(const double* probs, int n, std::vector<T>& l0) {
  l0.resize((size_t)std::max(1, n));
  for (int j = 0; j < n; ++j) l0[j] = (T)std::log((1.0 - probs[j]) / probs[j]);  // glibc log, as Cython
}

// THE LAW for one syndrome: the sequential sweep in order pi
template <typename T>
void serial_decode_one(const HostGraph& g, const std::vector<int32_t>& ord, const std::vector<T>& l0, int max_iter,
                       double alpha_in, const uint8_t* synd, uint8_t* corr, int32_t* iters, uint8_t* conv, double* post,
                       std::vector<T>& b2c, std::vector<T>& c2b, std::vector<T>& pst, std::vector<uint8_t>& dec) {
  const int m = g.m, n = g.n;
  for (int e = 0; e < g.E; ++e) b2c[e] = l0[g.ci[e]];
  int total = 0;
  bool converged = false;
  for (int t = 1; t <= max_iter && !converged; ++t) {
    const T alpha = serial_alpha<T>(alpha_in, t);
    for (int q = 0; q < n; ++q) {
      const int j = ord[q];
      const int k0 = g.cp[j], k1 = g.cp[j + 1];
      for (int k = k0; k < k1; ++k) {
        const int i = g.cr[k];
        c2b[k - k0] = serial_c2b<T>(b2c.data(), g.rp[i], g.rp[i + 1], g.ce[k], synd[i] & 1, alpha);
      }
      T temp = l0[j];
      for (int k = k0; k < k1; ++k) {
        b2c[g.ce[k]] = temp;
        temp = temp + c2b[k - k0];
      }
      pst[j] = temp;
      dec[j] = temp <= 0 ? 1 : 0;
      temp = (T)0;
      for (int k = k1 - 1; k >= k0; --k) {
        b2c[g.ce[k]] = b2c[g.ce[k]] + temp;
        temp = temp + c2b[k - k0];
      }
    }
    ++total;
    converged = true;
    for (int i = 0; i < m && converged; ++i) {
      uint8_t a = synd[i] & 1;
      for (int e = g.rp[i]; e < g.rp[i + 1]; ++e) a ^= dec[g.ci[e]];
      converged = a == 0;
    }
  }
  std::copy(dec.begin(), dec.begin() + n, corr);
  if (iters) *iters = total;
  if (conv) *conv = converged ? 1 : 0;
  if (post)
    for (int j = 0; j < n; ++j) post[j] = (double)pst[j];
}

// probs1 / side non-NULL: the side law, each syndrome's L0 selected from the tables of probs (side bit
// 0) and probs1 (side bit 1) before the same per-syndrome routine runs
template <typename T>
void serial_decode_host_t(const HostGraph& g, const std::vector<int32_t>& ord, const double* probs,
                          const double* probs1, const uint8_t* side, int max_iter, double alpha, const uint8_t* synd,
                          uint8_t* corr, int32_t* iters, uint8_t* conv, double* post, int64_t B, int threads) {
  std::vector<T> l0, l1;
  serial_priors<T>(probs, g.n, l0);
  if (side) serial_priors<T>(probs1, g.n, l1);
  int maxdeg = 1;
  for (int j = 0; j < g.n; ++j) maxdeg = std::max(maxdeg, g.cp[j + 1] - g.cp[j]);
  std::atomic<int64_t> next(0);
  auto work = [&]() {
    std::vector<T> b2c((size_t)std::max(1, g.E)), c2b((size_t)maxdeg), pst((size_t)g.n + 1);
    std::vector<uint8_t> dec((size_t)g.n + 1);
    std::vector<T> sel;
    if (side) sel = l0;
    for (int64_t b = next.fetch_add(1); b < B; b = next.fetch_add(1)) {
      if (side) {
        const uint8_t* sb = side + (size_t)b * g.n;
        for (int j = 0; j < g.n; ++j) sel[j] = (sb[j] & 1) ? l1[j] : l0[j];
      }
      serial_decode_one<T>(g, ord, side ? sel : l0, max_iter, alpha, synd + (size_t)b * g.m, corr + (size_t)b * g.n,
                           iters ? iters + b : nullptr, conv ? conv + b : nullptr,
                           post ? post + (size_t)b * g.n : nullptr, b2c, c2b, pst, dec);
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

size_t serial_lds(int precision, int m, int n, int E, int layers, bool soft, bool lds_messages, bool lds_index) {
  const size_t ts = precision == 32 ? 4 : 8;
  size_t tail = (soft ? (((size_t)n * ts + 7) & ~(size_t)7) : 0) + 8 + (size_t)n + (size_t)m;
  if (lds_index)
    tail = ((tail + 1) & ~(size_t)1) +
           2 * ((size_t)(m + 1) + (size_t)(n + 1) + (size_t)(layers + 1) + (size_t)n + 3 * (size_t)E);
  return (lds_messages ? (((size_t)E * ts + 7) & ~(size_t)7) : 0) + ((tail + 15) / 16) * 16;
}

template <typename T, typename I>
void launch(const SerialArgs& a, int grid, int tb, size_t lds, hipStream_t stream) {
  if (a.side)
    hipLaunchKernelGGL((serial_kernel<T, I, true>), dim3(grid), dim3(tb), lds, stream, a);
  else
    hipLaunchKernelGGL((serial_kernel<T, I, false>), dim3(grid), dim3(tb), lds, stream, a);
}

}  // namespace

namespace qldpc_rt {

int serial_check_params(int64_t n, int32_t max_iter, int32_t precision) { return check_params(n, max_iter, precision); }

const void* serial_kernel_ptr(int precision, bool lds_index, bool side) {
  if (side) {
    if (lds_index)
      return precision == 32 ? reinterpret_cast<const void*>(&serial_kernel<float, uint16_t, true>)
                             : reinterpret_cast<const void*>(&serial_kernel<double, uint16_t, true>);
    return precision == 32 ? reinterpret_cast<const void*>(&serial_kernel<float, int32_t, true>)
                           : reinterpret_cast<const void*>(&serial_kernel<double, int32_t, true>);
  }
  if (lds_index)
    return precision == 32 ? reinterpret_cast<const void*>(&serial_kernel<float, uint16_t, false>)
                           : reinterpret_cast<const void*>(&serial_kernel<double, uint16_t, false>);
  return precision == 32 ? reinterpret_cast<const void*>(&serial_kernel<float, int32_t, false>)
                         : reinterpret_cast<const void*>(&serial_kernel<double, int32_t, false>);
}

int serial_upload_priors(qldpc_bp* bp) {
  const int n = bp->g->n;
  if (!n) return 0;
  if (bp->route.precision == 32) {
    std::vector<float> l0;
    serial_priors<float>(bp->probs.data(), n, l0);
    QLDPC_HIP(hipMemcpy(bp->llr.p, l0.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  } else {
    std::vector<double> l0;
    serial_priors<double>(bp->probs.data(), n, l0);
    QLDPC_HIP(hipMemcpy(bp->llr.p, l0.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  }
  return 0;
}

// the two-row L0 table of a side decode (qldpc_bp_set_side_probs): row 0 from p0, row 1 from p1
int serial_upload_side(qldpc_bp* bp, const double* p0, const double* p1) {
  const int n = bp->g->n;
  const size_t ts = bp->route.precision == 32 ? 4 : 8;
  int rc;
  if (!bp->side_llr.p && (rc = bp->side_llr.alloc(std::max<size_t>(1, (size_t)2 * n) * ts))) return rc;
  const double* rows[2] = {p0, p1};
  for (int r = 0; r < 2 && n; ++r) {
    if (bp->route.precision == 32) {
      std::vector<float> l0;
      serial_priors<float>(rows[r], n, l0);
      QLDPC_HIP(hipMemcpy(static_cast<float*>(bp->side_llr.p) + (size_t)r * n, l0.data(), (size_t)n * 4,
                          hipMemcpyHostToDevice));
    } else {
      std::vector<double> l0;
      serial_priors<double>(rows[r], n, l0);
      QLDPC_HIP(hipMemcpy(static_cast<double*>(bp->side_llr.p) + (size_t)r * n, l0.data(), (size_t)n * 8,
                          hipMemcpyHostToDevice));
    }
  }
  return 0;
}

// The layer table and the CSC rows of bp's graph on the device, and the launch geometry: messages in
// LDS or in the workspace, indices staged or not, the workgroup width.
int serial_prepare(qldpc_bp* bp, bool force_ws, bool allow_idx, int want_tb, int lds_max) {
  const qldpc_graph* g = bp->g;
  const int m = g->m, n = g->n, E = g->nnz, precision = bp->route.precision;
  HostGraph h;
  h.m = m;
  h.n = n;
  h.rp = g->row_ptr.data();
  h.ci = g->col_idx.data();
  build_csc(h);
  std::vector<int32_t> layer, ord, lp;
  const int layers = first_fit_layers(h, layer);
  sweep_order(layer, layers, ord, lp);
  bp->sr_layers = layers;
  int rc;
  if ((rc = bp->sr_cr.alloc((size_t)std::max(1, E) * 4)) || (rc = bp->sr_ord.alloc((size_t)std::max(1, n) * 4)) ||
      (rc = bp->sr_lp.alloc((size_t)(layers + 1) * 4)))
    return rc;
  if ((E && hipMemcpy(bp->sr_cr.p, h.cr.data(), (size_t)E * 4, hipMemcpyHostToDevice) != hipSuccess) ||
      (n && hipMemcpy(bp->sr_ord.p, ord.data(), (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(bp->sr_lp.p, lp.data(), (size_t)(layers + 1) * 4, hipMemcpyHostToDevice) != hipSuccess)
    return set_err(QLDPC_EHIP, "upload the serial engine's layer table");
  const bool soft = bp->sr_soft;
  // the whole per-decode image in LDS when it fits, else the messages in an HBM workspace
  const bool lds_msgs = !force_ws && serial_lds(precision, m, n, E, layers, soft, true, false) <= (size_t)lds_max;
  size_t lds = serial_lds(precision, m, n, E, layers, soft, lds_msgs, false);
  if (lds > (size_t)lds_max) return set_err(QLDPC_ENOTSUP, "graph too large for the serial engine's LDS state");
  // the widest layer decides the width: a narrower workgroup leaves no more threads idle, pays less
  // per barrier and lets more decodes share a CU
  int widest = 1;
  for (int l = 0; l < layers; ++l) widest = std::max(widest, lp[l + 1] - lp[l]);
  int tb = 64;
  while (tb < kSerialMaxThreads && tb < widest) tb *= 2;
  if (want_tb == 64 || want_tb == 128 || want_tb == 256) tb = want_tb;
  // indices as 16-bit words in LDS when that costs no resident workgroup: the runtime's occupancy of
  // each variant at its own LDS size (registers, waves and LDS together)
  auto resident = [&](bool idx, size_t bytes) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, serial_kernel_ptr(precision, idx), tb, bytes) != hipSuccess)
      nb = 1;
    return std::max(1, nb);
  };
  const size_t lds_idx = serial_lds(precision, m, n, E, layers, soft, lds_msgs, true);
  bp->blocks_per_cu = resident(false, lds);
  // (staging them at the price of resident workgroups was measured and dropped: hgp_34_n1600 fp64
  // falls from 3 workgroups per CU to 1 and from 118 k to 63 k shots/s)
  if (allow_idx && E <= 0xffff && n <= 0xffff && m <= 0xffff && lds_idx <= (size_t)lds_max) {
    const int with_idx = resident(true, lds_idx);
    if (with_idx >= bp->blocks_per_cu) {
      bp->sr_idx = true;
      bp->blocks_per_cu = with_idx;
      lds = lds_idx;
    }
  }
  bp->route.lds_bytes = (int)lds;
  bp->route.TB = tb;
  bp->route.VPL = (widest + tb - 1) / tb;
  bp->ps_grid = (long long)bp->blocks_per_cu * bp->cus;
  if (!lds_msgs && (rc = bp->ps_ws.alloc(std::max<size_t>(1, (size_t)bp->ps_grid * E * (precision == 32 ? 4 : 8)))))
    return rc;
  return 0;
}

int serial_decode_launch(const qldpc_bp* bp, const uint8_t* synd, uint8_t* corr, int32_t* iters, uint8_t* conv,
                         double* post, int64_t B, hipStream_t stream, const uint8_t* side) {
  const qldpc_graph* g = bp->g;
  SerialArgs a;
  a.rp = static_cast<const int32_t*>(bp->ps_rp.p);
  a.ci = static_cast<const int32_t*>(bp->ps_ci.p);
  a.cp = static_cast<const int32_t*>(bp->ps_cp.p);
  a.ce = static_cast<const int32_t*>(bp->ps_ce.p);
  a.cr = static_cast<const int32_t*>(bp->sr_cr.p);
  a.ord = static_cast<const int32_t*>(bp->sr_ord.p);
  a.lp = static_cast<const int32_t*>(bp->sr_lp.p);
  a.llr = side ? bp->side_llr.p : bp->llr.p;
  a.side = side;
  a.ws = bp->ps_ws.p;
  a.synd = synd;
  a.corr = corr;
  a.iters = iters;
  a.conv = conv;
  a.post = post;
  a.B = B;
  a.alpha = bp->alpha;
  a.m = g->m;
  a.n = g->n;
  a.E = g->nnz;
  a.layers = bp->sr_layers;
  a.max_iter = bp->max_iter;
  a.soft = bp->sr_soft ? 1 : 0;
  // the workspace has one slice per workgroup of ps_grid: never launch more (side_grid <= ps_grid)
  const int grid = (int)std::max<long long>(1, std::min<long long>(B, side ? bp->side_grid : bp->ps_grid));
  const size_t lds = bp->route.lds_bytes;
  if (bp->route.precision == 32) {
    if (bp->sr_idx)
      launch<float, uint16_t>(a, grid, bp->route.TB, lds, stream);
    else
      launch<float, int32_t>(a, grid, bp->route.TB, lds, stream);
  } else {
    if (bp->sr_idx)
      launch<double, uint16_t>(a, grid, bp->route.TB, lds, stream);
    else
      launch<double, int32_t>(a, grid, bp->route.TB, lds, stream);
  }
  QLDPC_HIP(hipGetLastError());
  return 0;
}

}  // namespace qldpc_rt

extern "C" {

int qldpc_serial_layers(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx, int32_t* layer_out,
                        int32_t* num_layers) {
  if (int rc = check_csr(m, n, row_ptr, col_idx)) return rc;
  if (!layer_out && n > 0) return set_err(QLDPC_EINVAL, "NULL layer_out");
  HostGraph g;
  g.m = m;
  g.n = n;
  g.rp = row_ptr;
  g.ci = col_idx;
  build_csc(g);
  std::vector<int32_t> layer;
  const int layers = first_fit_layers(g, layer);
  std::copy(layer.begin(), layer.end(), layer_out);
  if (num_layers) *num_layers = layers;
  return 0;
}

// qldpc_serial_decode_host (p1 = side = NULL) and qldpc_serial_decode_host_side
static int serial_decode_host_any(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                                  const double* channel_probs, const double* p1, const uint8_t* side, int32_t max_iter,
                                  double ms_scaling_factor, int32_t precision, const uint8_t* synd, uint8_t* corr,
                                  int32_t* iters, uint8_t* conv, double* post, int64_t B, int32_t threads) {
  if (int rc = check_csr(m, n, row_ptr, col_idx)) return rc;
  if (!channel_probs && n > 0) return set_err(QLDPC_EINVAL, "NULL channel_probs");
  if (int rc = check_params(n, max_iter, precision)) return rc;
  if (B < 0 || (B > 0 && ((!synd && m > 0) || (!corr && n > 0)))) return set_err(QLDPC_EINVAL, "NULL argument");
  if (B == 0) return 0;
  HostGraph g;
  g.m = m;
  g.n = n;
  g.rp = row_ptr;
  g.ci = col_idx;
  build_csc(g);
  std::vector<int32_t> layer, ord, lp;
  const int layers = first_fit_layers(g, layer);
  sweep_order(layer, layers, ord, lp);
  int nt = threads;
  if (nt <= 0) {
    const char* e = std::getenv("OMP_NUM_THREADS");
    nt = (e && *e) ? std::atoi(e) : (int)std::thread::hardware_concurrency();
    if (nt <= 0) nt = 1;
  }
  if (precision == 32)
    serial_decode_host_t<float>(g, ord, channel_probs, p1, side, max_iter, ms_scaling_factor, synd, corr, iters, conv,
                                post, B, nt);
  else
    serial_decode_host_t<double>(g, ord, channel_probs, p1, side, max_iter, ms_scaling_factor, synd, corr, iters, conv,
                                 post, B, nt);
  return 0;
}

int qldpc_serial_decode_host(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                             const double* channel_probs, int32_t max_iter, double ms_scaling_factor, int32_t precision,
                             const uint8_t* synd, uint8_t* corr, int32_t* iters, uint8_t* conv, double* post, int64_t B,
                             int32_t threads) {
  return serial_decode_host_any(m, n, row_ptr, col_idx, channel_probs, nullptr, nullptr, max_iter, ms_scaling_factor,
                                precision, synd, corr, iters, conv, post, B, threads);
}

int qldpc_serial_decode_host_side(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                                  const double* p0, const double* p1, const uint8_t* side, int32_t max_iter,
                                  double ms_scaling_factor, int32_t precision, const uint8_t* synd, uint8_t* corr,
                                  int32_t* iters, uint8_t* conv, int64_t B, int32_t threads) {
  if (n > 0 && (!p0 || !p1)) return set_err(QLDPC_EINVAL, "NULL side prior table");
  if (B > 0 && n > 0 && !side) return set_err(QLDPC_EINVAL, "NULL side bytes");
  if (int rc = side_probs_check(n, p0, p1)) return rc;
  // (n = 0: no variable selects anything, the plain routine serves)
  return serial_decode_host_any(m, n, row_ptr, col_idx, p0, n > 0 ? p1 : nullptr, n > 0 ? side : nullptr, max_iter,
                                ms_scaling_factor, precision, synd, corr, iters, conv, nullptr, B, threads);
}

}  // extern "C"

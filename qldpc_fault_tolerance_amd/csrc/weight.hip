// weight.hip — fixed-weight depolarizing errors for the staged data-error pipeline (staged.hip):
// the sampler behind qldpc_mc_launch_weight and qldpc_sample_errors_weight[_host].
//
// Conditioned on its weight w, a depolarizing error on n qubits is a uniform random w-subset of the
// qubits with i.i.d. Pauli classes in the ratio px : py : pz.  THE LAW (the contract; tests/weight_ref.py
// replays it in Python integers): shot s (global, 64-bit), weight w, step i = 0 .. w-1, t = n - w + i:
//   (o0, o1, o2, o3) = Philox4x32-10(ctr = (i, s_lo, s_hi, 0x51D50006), key = (seed_lo, seed_hi));
//   r = (((o1 << 32) | o0) * (t + 1)) >> 64          (64 x 64 -> high 64: uniform on 0 .. t)
//   qubit = r if r was not picked in steps 0 .. i-1, else t            (Floyd's subset algorithm)
//   k = ((o2 >> 5) << 26) | (o3 >> 6)                (53 bits, the form of philox_k53)
//   class Z (2) if k < K1 = ceil(2^53 pz / T), else X (1) if k < K2 = ceil(2^53 (pz + px) / T), else Y (3),
//   T = (pz + px) + py, the sums and quotients in doubles on the host, in the order of the reference's
//   three-way split (src/Simulators.py:102-108).  Only the ratios of px, py, pz matter.
// The multiply-high draw is not exactly uniform: value v of 0 .. t gets floor or ceil of 2^64 / (t + 1)
// of the 2^64 inputs, a bias of at most (t + 1) / 2^64 < 2^-52 per step for n <= 4096.  No rejection
// step removes it (it is eleven orders of magnitude below any Monte Carlo error this feeds).
// A shot's error depends on (seed, s, w, n, px : py : pz) only: not on the grid, the batch size or how
// a range is cut into launches.  The same (seed, s) at two weights REUSES draws (step i of weight w
// and of weight w' read the same Philox block), so strata that must be independent need disjoint shot
// ranges (CodeSimulator_DataError.FailureSpectrum gives every stratum its own).
//
// Kernel (wt_sample): one workgroup of four waves per 64-shot word.  Wave 0 draws, one lane per shot:
// each lane keeps its error as two n-bit masks (x bits, z bits; picked = x | z since every class sets
// one of them) in LDS, lane-interleaved: dword k of lane l at index k·64 + l.  A lane touches its own
// column only, at bank l mod 32 whatever k is, so the data-dependent membership test and the bit sets
// of the Floyd loop are conflict-free (ds_read_b32 / ds_write_b32 serve lanes 0-31 and 32-63 as two
// groups).  After a barrier all four waves emit, wave v the dwords k = v, v + 4, ...: word [j][wd] of both
// components for the dword's 32 qubits j by ballots over the 64 lanes (lane b keeps the ballot of bit
// b and lanes 0-31 store), so every word of the batch is written exactly once: no atomics, no
// dependence on ordering, no zero fill of the target.  (Emission, 2 ballots per qubit, is most of the
// kernel at w << n: with one wave per word a 65,536-shot batch is one wave per SIMD and as slow as
// that wave's n ballots; four waves cut it 1.9x at w = 16, see DESIGN.md.)  Lanes past the last shot of a
// partial word draw nothing and keep zero masks.
// LDS: 2 · ceil(n / 32) · 64 · 4 B = 512 · ceil(n / 32) B per workgroup (n = 1600: 25 KiB, 6
// workgroups = 24 waves per CU; n = 225: 4 KiB, the 32-wave cap).  Cap: n <= kWeightMaxN = 4096
// (64 KiB, the default dynamic-LDS limit; 2 workgroups per CU); QLDPC_ENOTSUP beyond.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "bp_kernels.h"
#include "runtime.h"

using namespace qldpc;
using namespace qldpc_rt;

namespace {

constexpr uint32_t kStreamWeight = 0x51D50006u;
constexpr int kWeightMaxN = 4096;
constexpr int kWeightWaves = 4;

struct WeightArgs {
  unsigned long long* cur[2];  // [n][W] X / Z error words (overwritten), or
  uint8_t* err;                // [count][n] classes (bit0 x, bit1 z) when cur[0] is NULL
  unsigned long long seed, shot0;  // shot0: global index of this launch's first shot
  unsigned long long K1, K2;
  long long count;  // shots of this launch
  int n, w, W;      // W = ceil(count / 64)
};

// grid: x = word wd (64 shots); block: kWeightWaves waves (wave 0 draws, all of them emit)
template <bool kBytes>
__global__ void __launch_bounds__(64 * kWeightWaves) wt_sample(WeightArgs A) {
  extern __shared__ uint32_t wt_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long wd = blockIdx.x;
  const long long sl = wd * 64 + lane;
  const int K = (A.n + 31) >> 5;
  uint32_t* X = wt_lds + lane;                    // dword k of this lane: X[k * 64]
  uint32_t* Z = wt_lds + (size_t)K * 64 + lane;
  for (int k = wv; k < K; k += kWeightWaves) X[k * 64] = Z[k * 64] = 0u;
  __syncthreads();
  if (wv == 0 && sl < A.count) {
    const unsigned long long shot = A.shot0 + (unsigned long long)sl;
    for (int i = 0; i < A.w; ++i) {
      const uint32_t t = (uint32_t)(A.n - A.w + i);
      uint32_t o0, o1, o2, o3;
      philox4x32_10_x4((uint32_t)i, (uint32_t)shot, (uint32_t)(shot >> 32), kStreamWeight, (uint32_t)A.seed,
                       (uint32_t)(A.seed >> 32), o0, o1, o2, o3);
      // r <= t < n: the masks' dword index stays below K
      const uint32_t r = (uint32_t)__umul64hi(((unsigned long long)o1 << 32) | o0, (unsigned long long)t + 1ull);
      const bool taken = ((X[(r >> 5) * 64] | Z[(r >> 5) * 64]) >> (r & 31u)) & 1u;
      const uint32_t q = taken ? t : r;
      const unsigned long long k53 = ((unsigned long long)(o2 >> 5) << 26) | (unsigned long long)(o3 >> 6);
      const uint32_t cls = k53 < A.K1 ? 2u : k53 < A.K2 ? 1u : 3u;
      const uint32_t bit = 1u << (q & 31u);
      if (cls & 1u) X[(q >> 5) * 64] |= bit;
      if (cls & 2u) Z[(q >> 5) * 64] |= bit;
    }
  }
  __syncthreads();  // the other waves read wave 0's columns below
  if (!kBytes) {
    for (int k = wv; k < K; k += kWeightWaves) {
      const uint32_t xm = X[k * 64], zm = Z[k * 64];
      unsigned long long ox = 0ull, oz = 0ull;
#pragma unroll
      for (int b = 0; b < 32; ++b) {
        const unsigned long long bx = __ballot((xm >> b) & 1u), bz = __ballot((zm >> b) & 1u);
        if (lane == b) {
          ox = bx;
          oz = bz;
        }
      }
      const int j = k * 32 + lane;
      if (lane < 32 && j < A.n) {
        A.cur[0][(long long)j * A.W + wd] = ox;
        A.cur[1][(long long)j * A.W + wd] = oz;
      }
    }
  } else {
    const int nb = (int)(A.count - wd * 64 < 64 ? A.count - wd * 64 : 64);
    if (lane < 32)
      for (int k = wv; k < K; k += kWeightWaves) {
        const int j = k * 32 + lane;
        if (j >= A.n) continue;
        for (int s = 0; s < nb; ++s) {
          const uint32_t xm = wt_lds[k * 64 + s], zm = wt_lds[(size_t)K * 64 + k * 64 + s];
          A.err[(wd * 64 + s) * A.n + j] = (uint8_t)(((xm >> lane) & 1u) | (((zm >> lane) & 1u) << 1));
        }
      }
  }
}

unsigned long long ceil53(double t) {
  if (!(t > 0.0)) return 0ull;
  if (t >= 1.0) return 1ull << 53;
  return (unsigned long long)std::ceil(std::ldexp(t, 53));
}

// Philox4x32-10 on the host (the kernel's philox4x32_10_x4; oracle_philox4x32_10)
void philox_host(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t o[4]) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

int launch(WeightArgs& A, bool bytes, hipStream_t st) {
  if (A.n > kWeightMaxN)
    return set_err(QLDPC_ENOTSUP, "fixed-weight sampler: n > 4096 (its per-lane masks fill 64 KiB of LDS there)");
  if (A.W <= 0) return 0;
  const size_t lds = (size_t)2 * ((A.n + 31) / 32) * 64 * 4;
  if (bytes)
    hipLaunchKernelGGL(wt_sample<true>, dim3((unsigned)A.W), dim3(64 * kWeightWaves), lds, st, A);
  else
    hipLaunchKernelGGL(wt_sample<false>, dim3((unsigned)A.W), dim3(64 * kWeightWaves), lds, st, A);
  QLDPC_HIP(hipGetLastError());
  return 0;
}

}  // namespace

namespace qldpc_rt {

int weight_thresholds(int64_t weight, int64_t n, double px, double py, double pz, unsigned long long* K1,
                      unsigned long long* K2) {
  if (n <= 0) return set_err(QLDPC_EINVAL, "n <= 0");
  if (weight < 0 || weight > n) return set_err(QLDPC_EINVAL, "weight must be in 0 .. n");
  if (!(px >= 0 && py >= 0 && pz >= 0)) return set_err(QLDPC_EINVAL, "negative Pauli probability");
  const double T = (pz + px) + py;
  if (!(T > 0.0)) {
    if (weight > 0) return set_err(QLDPC_EINVAL, "px = py = pz = 0 with weight > 0: no Pauli class to draw");
    *K1 = *K2 = 0ull;
    return 0;
  }
  if (!std::isfinite(T)) return set_err(QLDPC_EINVAL, "Pauli probabilities are not finite");
  *K1 = ceil53(pz / T);
  *K2 = ceil53((pz + px) / T);
  return 0;
}

int weight_sample_words(int weight, unsigned long long K1, unsigned long long K2, uint64_t seed, uint64_t shot0,
                        long long count, int n, int W, unsigned long long* cur_x, unsigned long long* cur_z,
                        hipStream_t st) {
  WeightArgs A;
  A.cur[0] = cur_x; A.cur[1] = cur_z;
  A.err = nullptr;
  A.seed = seed; A.shot0 = shot0;
  A.K1 = K1; A.K2 = K2;
  A.count = count;
  A.n = n; A.w = weight; A.W = W;
  return launch(A, false, st);
}

}  // namespace qldpc_rt

extern "C" {

int qldpc_sample_errors_weight(int32_t weight, double px, double py, double pz, uint64_t seed, uint64_t shot_begin,
                               int64_t shot_count, int32_t n, uint8_t* d_err, void* stream) {
  if (!d_err) return set_err(QLDPC_EINVAL, "NULL d_err");
  WeightArgs A;
  if (int rc = weight_thresholds(weight, n, px, py, pz, &A.K1, &A.K2)) return rc;
  if (shot_count <= 0) return 0;
  if ((shot_count + 63) / 64 > 0x7fffffffLL) return set_err(QLDPC_EINVAL, "too many shots for one launch");
  A.cur[0] = A.cur[1] = nullptr;
  A.err = d_err;
  A.seed = seed; A.shot0 = shot_begin;
  A.count = shot_count;
  A.n = n; A.w = weight; A.W = (int)((shot_count + 63) / 64);
  return launch(A, true, (hipStream_t)stream);
}

int qldpc_sample_errors_weight_host(int32_t weight, double px, double py, double pz, uint64_t seed,
                                    uint64_t shot_begin, int64_t shot_count, int32_t n, uint8_t* err) {
  if (!err) return set_err(QLDPC_EINVAL, "NULL err");
  unsigned long long K1, K2;
  if (int rc = weight_thresholds(weight, n, px, py, pz, &K1, &K2)) return rc;
  for (int64_t b = 0; b < shot_count; ++b) {
    const uint64_t shot = shot_begin + (uint64_t)b;
    uint8_t* e = err + (size_t)b * (size_t)n;
    for (int32_t j = 0; j < n; ++j) e[j] = 0;
    for (int32_t i = 0; i < weight; ++i) {
      const uint32_t t = (uint32_t)(n - weight + i);
      uint32_t o[4];
      philox_host((uint32_t)i, (uint32_t)shot, (uint32_t)(shot >> 32), kStreamWeight, (uint32_t)seed,
                  (uint32_t)(seed >> 32), o);
      const unsigned __int128 x = ((unsigned __int128)o[1] << 32) | o[0];
      const uint32_t r = (uint32_t)((x * (unsigned __int128)(t + 1u)) >> 64);
      const uint32_t q = e[r] ? t : r;
      const uint64_t k53 = ((uint64_t)(o[2] >> 5) << 26) | (uint64_t)(o[3] >> 6);
      e[q] = k53 < K1 ? 2 : k53 < K2 ? 1 : 3;
    }
  }
  return 0;
}

}  // extern "C"

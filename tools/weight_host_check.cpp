// weight_host_check.cpp — stand-alone exerciser of the host form of the fixed-weight error sampler
// (qldpc_sample_errors_weight_host), for a sanitizer build of that host code:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -I include -Xarch_host -fsanitize=address,undefined \
//       qldpc_fault_tolerance_amd/csrc/weight.hip tools/weight_host_check.cpp -o weight_host_check
//   ./weight_host_check
//
// It makes no HIP call, so it runs without a GPU.  Cases: (n, w) = (225, 225) (every step but the first
// few collides), (65, 64), (1, 1), (64, 0), a range that crosses s_hi, split ranges, and the EINVAL paths.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "qldpc_hip.h"

namespace qldpc_rt {
thread_local std::string g_err;  // the library defines it in qldpc_hip.hip
}

static int fails = 0;
#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      std::printf("FAIL line %d: %s\n", __LINE__, #x);      \
      ++fails;                                              \
    }                                                       \
  } while (0)

static void shape(int n, int w, double px, double py, double pz) {
  const int64_t S = 130;
  const uint64_t s0 = (1ull << 32) - 64;
  std::vector<uint8_t> all((size_t)S * n, 0xEE), a((size_t)50 * n, 0xEE), b((size_t)80 * n, 0xEE);
  CHECK(qldpc_sample_errors_weight_host(w, px, py, pz, 9, s0, S, n, all.data()) == QLDPC_OK);
  CHECK(qldpc_sample_errors_weight_host(w, px, py, pz, 9, s0, 50, n, a.data()) == QLDPC_OK);
  CHECK(qldpc_sample_errors_weight_host(w, px, py, pz, 9, s0 + 50, 80, n, b.data()) == QLDPC_OK);
  for (int64_t s = 0; s < S; ++s) {
    int cnt = 0;
    for (int j = 0; j < n; ++j) {
      const uint8_t c = all[(size_t)s * n + j];
      CHECK(c <= 3);
      cnt += c != 0;
      CHECK(c == (s < 50 ? a[(size_t)s * n + j] : b[(size_t)(s - 50) * n + j]));
      if (py == 0 && pz == 0) CHECK(c <= 1);
    }
    CHECK(cnt == w);
  }
}

int main() {
  shape(225, 225, 1, 1, 1);
  shape(65, 64, 0.01, 0.002, 0.03);
  shape(1, 1, 1, 0, 0);
  shape(64, 0, 0, 0, 0);
  shape(1600, 16, 1, 1, 1);
  uint8_t e[8];
  CHECK(qldpc_sample_errors_weight_host(-1, 1, 1, 1, 0, 0, 1, 8, e) == QLDPC_EINVAL);
  CHECK(qldpc_sample_errors_weight_host(9, 1, 1, 1, 0, 0, 1, 8, e) == QLDPC_EINVAL);
  CHECK(qldpc_sample_errors_weight_host(2, 0, 0, 0, 0, 0, 1, 8, e) == QLDPC_EINVAL);
  CHECK(qldpc_sample_errors_weight_host(2, -1, 1, 1, 0, 0, 1, 8, e) == QLDPC_EINVAL);
  CHECK(qldpc_sample_errors_weight_host(2, 1, 1, 1, 0, 0, 1, 0, e) == QLDPC_EINVAL);
  CHECK(qldpc_sample_errors_weight_host(2, 1, 1, 1, 0, 0, 1, 8, nullptr) == QLDPC_EINVAL);
  CHECK(qldpc_sample_errors_weight_host(2, 1, 1, 1, 0, 0, 0, 8, e) == QLDPC_OK);
  std::printf(fails ? "weight_host_check: %d FAILED\n" : "weight_host_check: ok\n", fails);
  return fails ? 1 : 0;
}

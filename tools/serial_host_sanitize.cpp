// Stand-alone sanitizer check of the host serial-schedule min-sum law (qldpc_serial_decode_host /
// qldpc_serial_layers, csrc/serial.hip): a fixed graph, seeded syndromes, both precisions, one and
// several threads.  Host code only: no kernel is launched and no device is needed.  Build and run (from
// the repository root):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -I include \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/serial_host_sanitize.cpp qldpc_fault_tolerance_amd/csrc/serial.hip -o serial_host_sanitize
//   ./serial_host_sanitize
//
// Exit status 0 and "serial host law: ok" mean every decode ran clean, the layers are independent
// and every converged decode satisfies its syndrome.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "qldpc_hip.h"

namespace qldpc_rt {
thread_local std::string g_err;  // the library's error slot (qldpc_hip.hip is not linked here)
}

int main() {
  // 41 x 45: ring rows {i, i + 1, i + 7} (mod 44) with row 5 emptied and column 44 never used, plus one
  // wide row: unequal degrees, an empty row and an empty column
  const int m = 41, n = 45;
  std::vector<int32_t> rp{0}, ci;
  for (int i = 0; i < 40; ++i) {
    std::vector<int32_t> r;
    if (i != 5) r = {i % 44, (i + 1) % 44, (i + 7) % 44};
    std::sort(r.begin(), r.end());
    ci.insert(ci.end(), r.begin(), r.end());
    rp.push_back((int32_t)ci.size());
  }
  for (int j = 0; j < 44; j += 4) ci.push_back(j);
  rp.push_back((int32_t)ci.size());
  std::vector<double> probs(n);
  for (int j = 0; j < n; ++j) probs[j] = 0.01 + 0.002 * j;
  int bad = 0;
  // the layers: no two variables of a layer in one row
  std::vector<int32_t> layer(n);
  int32_t layers = 0;
  if (qldpc_serial_layers(m, n, rp.data(), ci.data(), layer.data(), &layers) != 0 || layers < 2) ++bad;
  for (int i = 0; i < m; ++i)
    for (int a = rp[i]; a < rp[i + 1]; ++a)
      for (int b = a + 1; b < rp[i + 1]; ++b)
        if (layer[ci[a]] == layer[ci[b]]) ++bad;
  const int64_t B = 96;
  std::vector<uint8_t> synd((size_t)B * m, 0);
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (int64_t b = 0; b < B; ++b) {
    std::vector<uint8_t> e(n, 0);
    for (int j = 0; j < n; ++j) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      e[j] = (s >> 40) % 100 < (uint64_t)(2 + b % 12);
    }
    for (int i = 0; i < m; ++i)
      for (int k = rp[i]; k < rp[i + 1]; ++k) synd[(size_t)b * m + i] ^= e[ci[k]];
    if (b % 17 == 3) synd[(size_t)b * m + 5] = 1;  // the empty row's bit: no solution exists
  }
  long solved = 0, total_it = 0;
  for (int precision : {64, 32})
    for (double alpha : {0.625, 0.0})
      for (int threads : {1, 3})
        for (int max_iter : {1, 9}) {
          std::vector<uint8_t> corr((size_t)B * n), conv(B);
          std::vector<int32_t> it(B);
          std::vector<double> post((size_t)B * n);
          const bool lean = threads == 3 && max_iter == 1;  // the optional outputs left out
          const int rc = qldpc_serial_decode_host(m, n, rp.data(), ci.data(), probs.data(), max_iter, alpha, precision,
                                                  synd.data(), corr.data(), lean ? nullptr : it.data(),
                                                  lean ? nullptr : conv.data(), lean ? nullptr : post.data(), B, threads);
          if (rc != 0) {
            std::printf("rc %d: %s\n", rc, qldpc_rt::g_err.c_str());
            ++bad;
            continue;
          }
          if (lean) continue;
          for (int64_t b = 0; b < B; ++b) {
            total_it += it[b];
            if (it[b] < 1 || it[b] > max_iter || (!conv[b] && it[b] != max_iter)) ++bad;
            for (int j = 0; j < n; ++j)
              if (corr[(size_t)b * n + j] != (post[(size_t)b * n + j] <= 0 ? 1 : 0)) ++bad;
            if (!conv[b]) continue;
            ++solved;
            for (int i = 0; i < m; ++i) {
              uint8_t a = synd[(size_t)b * m + i];
              for (int k = rp[i]; k < rp[i + 1]; ++k) a ^= corr[(size_t)b * n + ci[k]];
              if (a) ++bad;
            }
          }
        }
  // the argument checks return before any table is touched
  if (qldpc_serial_decode_host(m, n, rp.data(), ci.data(), probs.data(), 0, 0.625, 64, synd.data(), nullptr, nullptr,
                               nullptr, nullptr, 1, 1) != QLDPC_EINVAL)
    ++bad;
  if (qldpc_serial_decode_host(m, n, rp.data(), ci.data(), probs.data(), 3, 0.625, 16, synd.data(), nullptr, nullptr,
                               nullptr, nullptr, 1, 1) != QLDPC_EINVAL)
    ++bad;
  std::printf("serial host law: %s (%ld converged decodes, %ld iterations, %d violations)\n", bad ? "FAILED" : "ok",
              solved, total_it, bad);
  return bad ? 1 : 0;
}

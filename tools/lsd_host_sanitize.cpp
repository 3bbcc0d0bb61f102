// Stand-alone sanitizer check of the host BP+LSD law (qldpc_osd_create_lsd / qldpc_lsd_decode_batch_stats,
// csrc/lsd.hip, behind the qldpc_osd handle of csrc/osd.hip): a fixed rank-deficient graph, seeded
// syndromes and posteriors with ties and infinities, bits_per_step 1, 2, 3 and 64, one and several
// threads; then the law of higher order (qldpc_osd_create_lsd_order) on the same batch: lsd_e 1, 4 and 12,
// lsd_cs 4 and 64 at bits_per_step 1 and 2 under uniform and mixed priors.  Host code only: no kernel is
// launched and no device is needed.  Build and run (from the
// repository root):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -I include \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/lsd_host_sanitize.cpp qldpc_fault_tolerance_amd/csrc/lsd.hip \
//         qldpc_fault_tolerance_amd/csrc/osd.hip -o lsd_host_sanitize
//   ./lsd_host_sanitize
//
// Exit status 0 and "lsd host law: ok" mean every decode ran clean, every output with valid = 1
// satisfies its syndrome, exactly the inconsistent syndromes report valid = 0, and the results do not
// depend on the thread count or the entry point; at higher order also that the winners are never heavier
// than the candidates 0 under the handle's integer weights, and that order 0 through the new call is the
// order-0 stage.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "qldpc_hip.h"

namespace qldpc_rt {
thread_local std::string g_err;  // the library's error slot (qldpc_hip.hip is not linked here)
}

int main() {
  // 42 x 45: ring rows {i, i + 1, i + 7} (mod 44) with row 5 emptied and column 44 never used, one wide
  // row, and a copy of row 0 as the last row
  const int m = 42, n = 45;
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
  for (int j : {0, 1, 7}) ci.push_back(j);
  rp.push_back((int32_t)ci.size());
  const int64_t B = 96;
  std::vector<uint8_t> synd((size_t)B * m, 0), bad_s(B, 0), conv(B, 0), bp((size_t)B * n, 1);
  std::vector<double> post((size_t)B * n);
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&] {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 40;
  };
  for (int64_t b = 0; b < B; ++b) {
    std::vector<uint8_t> e(n, 0);
    for (int j = 0; j < n; ++j) {
      e[j] = b % 16 != 7 && next() % 100 < (uint64_t)(2 + b % 12);  // b = 7 mod 16: the all-zero syndrome
      const int v = (int)(next() % 9) - 4;
      post[(size_t)b * n + j] = j % 13 == 3 ? INFINITY : j % 11 == 5 ? -INFINITY : j % 7 == 2 ? -0.0 : 0.5 * v;
    }
    for (int i = 0; i < m; ++i)
      for (int k = rp[i]; k < rp[i + 1]; ++k) synd[(size_t)b * m + i] ^= e[ci[k]];
    if (b % 17 == 3) synd[(size_t)b * m + 5] = 1, bad_s[b] = 1;                              // the empty row's bit
    if (b % 19 == 4) synd[(size_t)b * m + 41] = 1 ^ synd[(size_t)b * m + 0], bad_s[b] = 1;  // the copies disagree
    conv[b] = b % 23 == 9;
  }
  int bad = 0;
  long cols = 0, rounds = 0;
  for (int k : {1, 2, 3, 64}) {
    qldpc_osd* O = nullptr;
    if (qldpc_osd_create_lsd(m, n, rp.data(), ci.data(), k, &O) != 0) {
      std::printf("create: %s\n", qldpc_rt::g_err.c_str());
      return 1;
    }
    std::vector<uint8_t> x1((size_t)B * n), x3((size_t)B * n), o0((size_t)B * n), ow((size_t)B * n);
    std::vector<int32_t> st1((size_t)B * 4), st3((size_t)B * 4);
    if (qldpc_lsd_decode_batch_stats(O, synd.data(), post.data(), nullptr, nullptr, x1.data(), st1.data(), B, 1) != 0 ||
        qldpc_lsd_decode_batch_stats(O, synd.data(), post.data(), nullptr, nullptr, x3.data(), st3.data(), B, 3) != 0)
      ++bad;
    if (x1 != x3 || st1 != st3) ++bad;
    for (int64_t b = 0; b < B; ++b) {
      const int32_t* st = &st1[(size_t)b * 4];
      cols += st[2];
      rounds += st[1];
      if (st[0] != !bad_s[b]) ++bad;
      if (!st[0]) continue;
      for (int i = 0; i < m; ++i) {
        uint8_t a = synd[(size_t)b * m + i];
        for (int e = rp[i]; e < rp[i + 1]; ++e) a ^= x1[(size_t)b * n + ci[e]];
        if (a) ++bad;
      }
    }
    // through the OSD entry points: both outputs, converged entries copy bp_corr, a side decode is the plain one
    std::vector<double> p0(n, 0.01), p1(n, 0.3);
    if (qldpc_osd_decode_batch(O, synd.data(), post.data(), conv.data(), bp.data(), o0.data(), ow.data(), B, 2) != 0) ++bad;
    if (o0 != ow) ++bad;
    for (int64_t b = 0; b < B; ++b)
      for (int j = 0; j < n; ++j)
        if (ow[(size_t)b * n + j] != (conv[b] ? 1 : x1[(size_t)b * n + j])) ++bad;
    if (qldpc_osd_decode_batch_side(O, synd.data(), post.data(), conv.data(), bp.data(), bp.data(), o0.data(), ow.data(),
                                    B, 2) != QLDPC_EINVAL)
      ++bad;  // no side tables yet
    std::vector<uint8_t> s0((size_t)B * n), sw((size_t)B * n);
    if (qldpc_osd_set_side_probs(O, p0.data(), p1.data()) != 0 ||
        qldpc_osd_decode_batch_side(O, synd.data(), post.data(), conv.data(), bp.data(), bp.data(), s0.data(), sw.data(),
                                    B, 2) != 0 ||
        s0 != ow || sw != ow)
      ++bad;
    int32_t rank = -1;
    if (qldpc_osd_rank(O, &rank) != 0 || rank < 1 || rank > 40) ++bad;  // an empty row and a copied row
    qldpc_osd_destroy(O);
  }
  // higher order: both outputs solve the syndrome where valid = 1, the winners weigh no more than the
  // candidates 0, and one and several threads agree
  long replaced = 0;
  for (int mixed = 0; mixed < 2; ++mixed) {
    std::vector<double> pr(n);
    for (int j = 0; j < n; ++j) pr[j] = mixed ? (j % 4 == 0 ? 0.07 : 0.01 + 0.29 * (double)(next() % 1000) / 1000.0) : 0.05;
    for (int k : {1, 2})
      for (auto mw : {std::pair<int, int>{1, 1}, {1, 4}, {1, 12}, {2, 4}, {2, 64}, {0, 3}, {1, 0}}) {
        qldpc_osd* O = nullptr;
        if (qldpc_osd_create_lsd_order(m, n, rp.data(), ci.data(), pr.data(), k, mw.first, mw.second, &O) != 0) {
          std::printf("create_lsd_order: %s\n", qldpc_rt::g_err.c_str());
          return 1;
        }
        std::vector<long long> wq(n);
        if (qldpc_lsd_weights(O, reinterpret_cast<int64_t*>(wq.data())) != 0) ++bad;
        std::vector<uint8_t> o0((size_t)B * n), ow((size_t)B * n), p0((size_t)B * n), pw((size_t)B * n), xs((size_t)B * n);
        std::vector<int32_t> st((size_t)B * 4);
        if (qldpc_osd_decode_batch(O, synd.data(), post.data(), nullptr, nullptr, o0.data(), ow.data(), B, 1) != 0 ||
            qldpc_osd_decode_batch(O, synd.data(), post.data(), nullptr, nullptr, p0.data(), pw.data(), B, 3) != 0 ||
            qldpc_lsd_decode_batch_stats(O, synd.data(), post.data(), nullptr, nullptr, xs.data(), st.data(), B, 2) != 0)
          ++bad;
        if (o0 != p0 || ow != pw || xs != ow) ++bad;
        const bool order0 = mw.first == 0 || mw.second == 0;
        if (order0 && o0 != ow) ++bad;
        for (int64_t b = 0; b < B; ++b) {
          if (st[(size_t)b * 4] != !bad_s[b]) ++bad;
          long long w0 = 0, ww = 0;
          for (int j = 0; j < n; ++j) {
            w0 += o0[(size_t)b * n + j] ? wq[j] : 0;
            ww += ow[(size_t)b * n + j] ? wq[j] : 0;
          }
          if (ww > w0) ++bad;
          if (ww < w0) ++replaced;
          if (!st[(size_t)b * 4]) continue;
          for (const auto* x : {&o0, &ow})
            for (int i = 0; i < m; ++i) {
              uint8_t a = synd[(size_t)b * m + i];
              for (int e = rp[i]; e < rp[i + 1]; ++e) a ^= (*x)[(size_t)b * n + ci[e]];
              if (a) ++bad;
            }
        }
        std::vector<double> q0(n, 0.01), q1(n, 0.3);
        if (qldpc_osd_set_side_probs(O, q0.data(), q1.data()) != (order0 ? 0 : QLDPC_ENOTSUP)) ++bad;
        qldpc_osd_destroy(O);
      }
  }
  if (replaced == 0) ++bad;
  qldpc_osd* O = nullptr;
  std::vector<double> pr(n, 0.05);
  if (qldpc_osd_create_lsd_order(m, n, rp.data(), ci.data(), pr.data(), 1, 1, 13, &O) != QLDPC_EINVAL) ++bad;
  if (qldpc_osd_create_lsd_order(m, n, rp.data(), ci.data(), pr.data(), 1, 2, 65, &O) != QLDPC_EINVAL) ++bad;
  if (qldpc_osd_create_lsd_order(m, n, rp.data(), ci.data(), pr.data(), 1, 3, 1, &O) != QLDPC_EINVAL) ++bad;
  if (qldpc_osd_create_lsd_order(m, n, rp.data(), ci.data(), pr.data(), 1, 1, -1, &O) != QLDPC_EINVAL) ++bad;
  if (qldpc_osd_create_lsd_order(m, n, rp.data(), ci.data(), nullptr, 1, 1, 2, &O) != QLDPC_EINVAL) ++bad;
  pr[7] = 1.0;
  if (qldpc_osd_create_lsd_order(m, n, rp.data(), ci.data(), pr.data(), 1, 2, 2, &O) != QLDPC_EINVAL) ++bad;
  if (qldpc_osd_create_lsd(m, n, rp.data(), ci.data(), 0, &O) != QLDPC_EINVAL) ++bad;
  if (qldpc_osd_create_lsd(m, n, nullptr, ci.data(), 1, &O) != QLDPC_EINVAL) ++bad;
  if (qldpc_osd_create_lsd(m, 3, rp.data(), ci.data(), 1, &O) != QLDPC_EINVAL) ++bad;
  std::printf("lsd host law: %s (%ld active columns, %ld rounds, %ld lighter winners, %d violations)\n",
              bad ? "FAILED" : "ok", cols, rounds, replaced, bad);
  return bad ? 1 : 0;
}

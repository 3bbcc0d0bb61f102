// osd_types.h — the second-stage handles of include/qldpc_hip.h, shared by osd.hip (ordered-statistics
// decoding) and lsd.hip (cluster-local elimination, reached through the same two handles).
#pragma once
#include <cstdint>
#include <vector>

#include "runtime.h"

struct qldpc_osd {
  int m = 0, n = 0, method = 1, order = 0, rank = 0;
  std::vector<std::vector<int32_t>> col_rows;
  std::vector<double> w;  // log(1/p_j)
  bool uniform = true;
  // side tables (qldpc_osd_set_side_probs): w_s[j] = log(1 / p_s[j]); a side decode weighs column j of
  // syndrome b with w_{side[b][j] & 1}[j].  Empty until set.
  std::vector<double> ws0, ws1;
  // qldpc_osd_create_lsd: bits_per_step >= 1 makes the handle an LSD stage (lsd.hip), which reads the
  // rows of H as well; 0 = OSD
  int lsd_k = 0;
  std::vector<int32_t> row_ptr, col_idx;
  // qldpc_osd_create_lsd_order: the candidate search on the grown clusters.  lsd_w = the order in force
  // (0 under method 0: today's order-0 stage), lsd_wq [n] = floor(log(1 / p_j) 2^32 + 0.5), empty without
  // priors in (0, 1)
  int lsd_method = 0, lsd_w = 0;
  std::vector<long long> lsd_wq;
};

struct qldpc_osd_gpu {
  qldpc_osd host;  // shape, method, order, rank
  int device = 0, grid = 0, W = 0, RW = 0, NP = 0, nh = 0, m_lds = 0, bits_off = 0;
  int wr = 0, pbuf_off = 0;  // register-row mode: compile-time words per row (0 = off), LDS pivot buffer
  int rr_tb = 0;             // register-row mode: threads per workgroup = m rounded up to waves
  size_t lds = 0;
  long long ws_words = 0, iws_ints = 0;
  qldpc_rt::DevBuf rp, ci, ws, iws, softw;  // softw: [n] log(1 / p_j) when the priors are not uniform
  qldpc_rt::DevBuf sw0, sw1;  // side tables [n] each (qldpc_osd_gpu_set_side_probs), else empty
  // LSD handle (host.lsd_k >= 1, lsd.hip): the columns of H (CSC) beside rp / ci, the LDS row-slot
  // capacity of the active image (0: the image lives in the HBM slice ws alone)
  qldpc_rt::DevBuf cp, ce, lsd_retries;
  int lsd_cap = 0;
  qldpc_rt::DevBuf lsd_wq;  // [n] candidate weights of a handle of order > 0, else empty
};

namespace qldpc_rt {
// lsd.hip: the host law over a batch (stats int32 [B][4] or null), the GPU handle of an LSD host
// stage, and its launch (d_stats int32 [B][4] or null)
int lsd_decode_batch_host(const qldpc_osd* osd, const uint8_t* synd, const double* post, const uint8_t* conv,
                          const uint8_t* bp_corr, uint8_t* out_osd0, uint8_t* out_osdw, int32_t* stats, int64_t B,
                          int32_t threads);
int lsd_gpu_from_host(const qldpc_graph* g, const qldpc_osd* host, qldpc_osd_gpu** out);
int lsd_gpu_launch(qldpc_osd_gpu* osd, const uint8_t* d_synd, const double* d_post, const uint8_t* d_conv,
                   const long long* d_shot, const uint8_t* d_bp_corr, uint8_t* d_out0, uint8_t* d_outw,
                   int32_t* d_stats, int64_t B, void* stream);
int lsd_gpu_threads();
}  // namespace qldpc_rt

// runtime.h — host-side internals shared by the engine's translation units:
// the thread-local error message behind qldpc_last_error(), device buffers,
// and the opaque handle types of include/qldpc_hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/qldpc_hip.h"
#include "route.h"

namespace qldpc_rt {

extern thread_local std::string g_err;

inline int set_err(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define QLDPC_HIP(x)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (x);                                                                    \
    if (e_ != hipSuccess) return qldpc_rt::set_err(QLDPC_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

// the two prior tables of a side decode: every entry finite and strictly inside (0, 1)
inline int side_probs_check(int64_t n, const double* p0, const double* p1) {
  for (int64_t j = 0; j < n; ++j)
    for (const double* p : {p0, p1})
      if (!std::isfinite(p[j]) || !(p[j] > 0.0) || !(p[j] < 1.0))
        return set_err(QLDPC_EINVAL, "side prior outside (0, 1) at variable " + std::to_string(j));
  return 0;
}

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int alloc(size_t b) {
    bytes = b;
    if (b == 0) return 0;
    if (hipMalloc(&p, b) != hipSuccess) {
      p = nullptr;
      return set_err(QLDPC_ENOMEM, "hipMalloc failed");
    }
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

}  // namespace qldpc_rt

struct qldpc_graph {
  int device = 0;
  int m = 0, n = 0, nnz = 0, max_row = 0, max_col = 0;
  std::vector<int32_t> row_ptr, col_idx;
  std::vector<std::vector<int32_t>> col_rows;  // rows of each column, ascending
};

struct qldpc_bp {
  qldpc_graph* g = nullptr;
  qldpc_rt::Route route;
  int max_iter = 0, method = 1;
  double alpha = 0.625;
  int blocks_per_cu = 0, cus = 0;
  std::vector<double> probs;
  // max_iter = 1 min-sum decodes (qldpc_bp_decode_batch): the first-min step kernel's one-iteration
  // BP (firstmin.hip), built on first use from these priors; dropped when they change
  qldpc_firstmin* bp1 = nullptr;
  bool bp1_off = false;
  qldpc_rt::DevBuf vchk, llr;  // engine 1: packed u16 check ids; engines 2-3: edge words (check | slot<<16)
  qldpc_rt::DevBuf rdeg;       // engine 3: u8 row degrees (by check label)
  int npos = 0;       // 1 + the last slot position holding a variable (SSector::npos)
  qldpc_rt::DevBuf work;       // engine 3 decode_batch: chunk-queue head
  std::vector<int32_t> slot_var;  // engines 2-3: variable of each (k, t) slot (-1 = padding)
  qldpc_rt::DevBuf perm;
  qldpc_rt::DevBuf rperm;  // engine 3: original check of each check label (label_checks)
  int gather_conf[2] = {0, 0};  // engine 3: extra gather cycles per pass before / after labelling
  // engine-3 fp64 variable phase, static LDS model per workgroup-iteration (qldpc_bp_lds_model):
  // CS gather cycles / extra, V-slot read cycles / extra, v2c store group-cycles / extra
  int64_t lds_model[6] = {0, 0, 0, 0, 0, 0};
  // engines 5 (product-sum, bp_ps.hip) and 7 (relay, relay.hip): CSR / CSC on the device, optional
  // HBM message workspace, the persistent grid the workspace is cut for
  qldpc_rt::DevBuf ps_rp, ps_ci, ps_cp, ps_ce, ps_ws;
  long long ps_grid = 0;
  // engine 7 (relay.hip): the chain's parameters (max_iter = pre_iter + legs * leg_iter), the gamma
  // table T [legs + 1][n] and the integer solution weights [n]; llr holds L0 in variable order
  int rl_pre_iter = 0, rl_legs = 0, rl_leg_iter = 0, rl_stop = 1;
  double rl_pre_gamma = 0, rl_lo = 0, rl_hi = 0;
  uint64_t rl_seed = 0;
  qldpc_rt::DevBuf rl_gam, rl_wq;
  bool rl_idx = false;  // the graph's CSR / CSC staged in LDS as 16-bit words
  // engine 8 (serial.hip): the CSC rows [E], the sweep order [n] and the layer boundaries [layers + 1]
  // beside engine 5's CSR / CSC; llr holds L0 in variable order
  qldpc_rt::DevBuf sr_cr, sr_ord, sr_lp;
  int sr_layers = 0;
  bool sr_idx = false;   // the index arrays staged in LDS as 16-bit words
  bool sr_soft = false;  // the kernel keeps the posteriors (qldpc_bp_decode_batch_soft)
  // engines 7 and 8, side priors (qldpc_bp_set_side_probs): L0 as T [2][n] (row 0 from p0, row 1 from
  // p1) and, engine 7, the integer solution weights [2][n]; qldpc_bp_decode_batch_side reads them
  qldpc_rt::DevBuf side_llr, side_wq;
  bool side_set = false;
  long long side_grid = 0;  // persistent grid of a side decode: the side variant's own residency, <= ps_grid
  // engine 6 (HBM-resident messages, bp_hbm.hip): uniform edge tables and the message workspace
  qldpc_rt::DevBuf h_rp, h_rcol, h_rcpos, h_cp, h_crpos, h_ws;
};

struct qldpc_mc {
  qldpc_bp* dec[2] = {nullptr, nullptr};
  int kw[2] = {0, 0};
  qldpc_rt::DevBuf lmask[2];
  qldpc_rt::DevBuf counters;
  qldpc_rt::DevBuf work;  // engine 3: chunk-queue head
  qldpc_rt::DevBuf cls_cache;  // engine 3, both sectors: sampled classes of the first sector's pass (SMcArgs)
  qldpc_rt::Route route;  // the sectors' common route (qldpc_mc_create)
  int blocks_per_cu = 0, cus = 0;
  int mmax = 0, vslots = 0, img_bytes = 0;
  // staged pipeline (staged.hip): product-sum decoders, or QLDPC_MC_STAGED=1
  bool staged = false;
  long long sbatch = 0;
  // BP+OSD (qldpc_mc_set_osd): GPU OSD per sector on the decodes that reached max_iter.
  // c_cap capture slots per sector (bounded by QLDPC_OSD_CAPTURE_MB); a launch is split into
  // pieces of at most c_cap shots, so a slot can never be lost (one slot per shot and sector)
  qldpc_osd_gpu* osd[2] = {nullptr, nullptr};
  long long c_cap = 0;
  qldpc_rt::DevBuf c_post[2], c_synd[2], c_err[2], c_shot[2], c_outw[2], c_n, c_fail;
  int sm[2] = {0, 0}, sk[2] = {0, 0};
  qldpc_rt::DevBuf s_rp[2], s_ci[2], s_cur[2], s_failw[2], s_D, s_det, s_corr, s_iters, s_conv;
  // qldpc_mc_set_channel_update: 0 = off, 1 = x->z, 2 = z->x; s_side [sbatch][n] keeps the first
  // sector's corrections as the side bytes of the second sector's decode
  int chan_dir = 0;
  qldpc_rt::DevBuf s_side;
  // qldpc_mc_set_staged_osd: GPU OSD per sector behind the staged loop's soft BP; s_post [sbatch][n]
  // doubles and s_bpcorr [sbatch][n] hold BP's posteriors and corrections for the OSD launch
  qldpc_osd_gpu* sosd[2] = {nullptr, nullptr};
  qldpc_rt::DevBuf s_post, s_bpcorr;
};


namespace qldpc_rt {

// engine 5 (bp_ps.hip)
size_t ps_lds_bytes(int precision, int m, int n, int E, bool lds_messages);
const void* ps_kernel(int precision);
int ps_decode_launch(const qldpc_bp* bp, const uint8_t* synd, uint8_t* corr, int32_t* iters, uint8_t* conv, int64_t B,
                     hipStream_t stream,
                     double* post = nullptr);

// engine 7 (relay.hip)
size_t relay_lds_bytes(int precision, int m, int n, int E, bool lds_messages, bool lds_index);
const void* relay_kernel_ptr(int precision, bool lds_index, bool side = false);
int relay_threads(size_t lds_bytes, int m, int n);
int relay_check_params(int64_t n, int32_t pre_iter, double pre_gamma, int32_t num_legs, int32_t leg_iter,
                       double gamma_lo, double gamma_hi, int32_t stop_nconv, int32_t precision);
int relay_upload_priors(qldpc_bp* bp);
int relay_upload_gammas(qldpc_bp* bp);
int relay_upload_side(qldpc_bp* bp, const double* p0, const double* p1);
// side non-NULL: the side decode (uint8 [B][n], bit 0), on the handle's side tables
int relay_decode_launch(const qldpc_bp* bp, const uint8_t* synd, uint8_t* corr, int32_t* iters, uint8_t* conv,
                        int64_t B, hipStream_t stream, const uint8_t* side = nullptr, double* post = nullptr);

// engine 8 (serial.hip)
int serial_check_params(int64_t n, int32_t max_iter, int32_t precision);
const void* serial_kernel_ptr(int precision, bool lds_index, bool side = false);
int serial_upload_priors(qldpc_bp* bp);
int serial_prepare(qldpc_bp* bp, bool force_ws, bool allow_idx, int want_tb, int lds_max);
int serial_upload_side(qldpc_bp* bp, const double* p0, const double* p1);
int serial_decode_launch(const qldpc_bp* bp, const uint8_t* synd, uint8_t* corr, int32_t* iters, uint8_t* conv,
                         double* post, int64_t B, hipStream_t stream, const uint8_t* side = nullptr);

// GPU OSD handle built on this graph? (osd.hip; qldpc_phenl_set_final_osd checks it)
bool osd_gpu_matches(const qldpc_osd_gpu* o, const qldpc_graph* g);
// side tables set on the GPU OSD handle? (qldpc_osd_gpu_set_side_probs)
bool osd_gpu_has_side(const qldpc_osd_gpu* o);
// host OSD stage built on this graph? (osd.hip; qldpc_circ_set_final_osd checks it)
bool osd_host_matches(const qldpc_osd* o, const qldpc_graph* g);
// GPU OSD handle from a host OSD stage on graph g: same method / order / rank / soft weights (osd.hip)
int osd_gpu_from_host(const qldpc_graph* g, const qldpc_osd* host, qldpc_osd_gpu** out);
// true when the first-min decoder was built on exactly this graph (shape and edges) and device
bool firstmin_matches(const qldpc_firstmin* fm, const qldpc_graph* g);
// one-iteration min-sum BP through a first-min handle (built with max_iter 0): corrections, iterations
// (1) and convergence (H d == s), the qldpc_bp_decode_batch contract at max_iter = 1
int bp1_decode(qldpc_firstmin* fm, const uint8_t* d_synd, uint8_t* d_corr, int32_t* d_iters, uint8_t* d_conv,
               int64_t B, hipStream_t stream);
// BP+OSD stage of the fused shot loop, one sector (osd.hip)
int osd_gpu_bposd_stage(qldpc_osd_gpu* osd, const uint8_t* synd, const double* post, const uint8_t* err,
                        const long long* shot, uint8_t* outw, long long ncand, const unsigned long long* lmask, int kw,
                        int q, int logical_mode, uint8_t* fail, unsigned long long* counters, hipStream_t stream);
// qldpc_osd_gpu_decode that skips the capture slots whose shot index is < 0 (osd.hip)
int osd_gpu_decode_slots(qldpc_osd_gpu* osd, const uint8_t* d_synd, const double* d_post, const uint8_t* d_conv,
                         const long long* d_shot, const uint8_t* d_bp_corr, uint8_t* d_out0, uint8_t* d_outw,
                         int64_t B, void* stream);
// the same with side bytes (d_side != null: qldpc_osd_gpu_decode_side's kernels and tables)
int osd_gpu_decode_any(qldpc_osd_gpu* osd, const uint8_t* d_synd, const double* d_post, const uint8_t* d_conv,
                       const long long* d_shot, const uint8_t* d_bp_corr, const uint8_t* d_side, uint8_t* d_out0,
                       uint8_t* d_outw, int64_t B, void* stream);

// engine 6 (bp_hbm.hip)
int hbm_prepare(qldpc_bp* bp);
const void* hbm_kernel(int precision);
int hbm_decode_launch(qldpc_bp* bp, const uint8_t* synd, uint8_t* corr, int32_t* iters, uint8_t* conv, int64_t B,
                      hipStream_t stream);

// staged data-error shot loop (staged.hip): bit-sliced sampling / syndromes /
// checks around qldpc_bp_decode_batch, for decoders the fused kernels do not serve
int staged_mc_prepare(qldpc_mc* mc, const qldpc_graph* logical_x, const qldpc_graph* logical_z);
void staged_mc_release(qldpc_mc* mc);
// fixed-weight sampling (weight.hip) in place of the i.i.d. channel: weight and class thresholds
struct StagedWeight {
  int weight;
  unsigned long long K1, K2;
};
int staged_mc_launch(qldpc_mc* mc, double px, double py, double pz, uint64_t seed, uint64_t shot_begin,
                     int64_t shot_count, int32_t logical_mode, const double* d_uniforms, void* d_counters,
                     uint8_t* d_fail, uint8_t* d_err, uint8_t* d_corr, int32_t* d_iters, hipStream_t stream,
                     const StagedWeight* fixed = nullptr);

// fixed-weight error sampler (weight.hip).  weight_thresholds: argument checks (QLDPC_EINVAL) and the
// class thresholds K1 = ceil(2^53 pz / T), K2 = ceil(2^53 (pz + px) / T).  weight_sample_words: shots
// shot0 .. shot0 + count - 1 into the bit-sliced [n][W] X / Z error words, every word overwritten.
int weight_thresholds(int64_t weight, int64_t n, double px, double py, double pz, unsigned long long* K1,
                      unsigned long long* K2);
int weight_sample_words(int weight, unsigned long long K1, unsigned long long K2, uint64_t seed, uint64_t shot0,
                        long long count, int n, int W, unsigned long long* cur_x, unsigned long long* cur_z,
                        hipStream_t stream);

}  // namespace qldpc_rt

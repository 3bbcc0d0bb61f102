// route.h — the route of a min-sum decoder: everything that names its kernel and launch shape.
// plan_route (qldpc_hip.hip) decides it from the graph, the precision and the QLDPC_* switches, on
// the host alone; route_vslots, slot_variant and route_kernel_id are the only readers that
// interpret it.  A fused MC handle holds the common route of its sectors (qldpc_mc_create).
#pragma once
#include <cstdint>

namespace qldpc_rt {

constexpr int kHbmThreads = 256;  // engine 6 workgroup (bp_hbm.hip)
constexpr int kHbmMaxDeg = 12;    // engine 6 row / column records (bp_hbm.hip): the degrees it takes

struct Route {
  int engine = 2, precision = 64;
  int DMAX = 4, TB = 64, VPL = 1, NS = 1;
  int nch = 0;  // 16-byte chunks per check row (MC: 0 when the sectors differ)
  // engine 3 sorts degree <= 3 variables first so that slots k < d3k skip the 4th edge slot
  // (MC: min over sectors)
  int d3k = 0;
  int d2k = 0;  // byte-F family: compile-time degree-2 slot count (slots of the measurement variables)
  int ea_shift = 0;  // engine 3: 2 = dword-scaled LDS addresses in the edge words (images > 64 KiB)
  int tail = 0;      // engine 3: 1 = rows of nch chunks + one tail slot per row (bp_reg.h eng_tail)
  int m2s = 0;       // engine 3: 1 = one-word check state, m2 in the argmin slot (bp_reg.h eng_m2s)
  int fb = 0;        // engine 3: 1 = byte F words (fp32 space-time family, 512 threads; bp_reg.h eng_fb)
  int m2s_pk = 0;        // m2s rows of 8 with packed absolute edge addresses (engine id 10203)
  int vslots_dummy = 0;  // m2s rows of 8 (engine id 10103): private V slots of real variables' missing edges
  uint32_t nw = 0;         // narrow waves of the fp64 space-time m2s family (SSector::nw)
  uint32_t live_last = 0;  // its waves live in the last variable slot (SSector::live_last)
  int lds_bytes = 0;
};

// V slots of the LDS image of a graph with m checks
inline int route_vslots(const Route& r, int m) {
  return (1 + m * r.nch) * (r.precision == 32 ? 4 : 2) + r.vslots_dummy;
}

}  // namespace qldpc_rt

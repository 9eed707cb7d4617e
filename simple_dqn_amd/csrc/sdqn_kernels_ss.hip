// sdqn_kernels_ss.hip — executor of the SS_* / SSH_* launch forms (launch_route.h): the SAMPLE-STATIONARY convolution launches (round 6), own
// translation unit like every other family of launch variants.  When a form runs is resolve_route's business (menu table: DESIGN.md 12).
//   float32, B >= 128 (conv_ss.h):   conv2_fwd  a1 [2][B][20][20][32] -> a2 [2][B][81][64]   4 x 4 stride 2   (deepqnetwork.py:85)
//                                    conv3_fwd  a2 [2][B][9][9][64]   -> a3 [2][B][49][64]   3 x 3 stride 1   (deepqnetwork.py:87)
//     each alone (SS_CONV2_* / SS_CONV3_*), or both as ONE launch at K_CONV2_FWD (SS_CHAIN_*: conv_ss_chain_kernel, a workgroup's conv3
//     follows its own conv2 behind a barrier)
//   float16, any B (conv_ssh.h):     [conv1 ->] conv2 -> conv3 as one launch at K_CONV2_FWD (SSH_CHAIN_*: conv_ssh_chain_kernel), and conv3_dgrad ->
//     conv2_dgrad as one launch at K_CONV3_DGRAD (SSH_DGRAD_CHAIN*: conv_ssh_dgrad_chain_kernel; deepqnetwork.py:162)
#include <stdlib.h>
#include "conv_ss.h"
#include "conv_ssh.h"
#include "kernels.h"

namespace sdqn {

// two samples per workgroup when one per workgroup would not fit the chip in one round (nz B > 256 workgroups), else one
// (the last three numbers: pixel / row / sample padding of the LDS image in floats — conflict-free fragment reads, tools/exp/ss_bank_search.py)
typedef ss::Cfg<P1, Q1, K1, 4, 4, ST2, P2, Q2, 2, 4, 20, 56> C2S2;
typedef ss::Cfg<P1, Q1, K1, 4, 4, ST2, P2, Q2, 1, 4, 20, 0> C2S1;
typedef ss::Cfg<P2, Q2, K2, 3, 3, 1, P3, Q3, 2, 8, 48, 16> C3S2;
typedef ss::Cfg<P2, Q2, K2, 3, 3, 1, P3, Q3, 1, 8, 48, 0> C3S1;

static ssh::Args ssh_chain_args(const StepArgs& a, int ns) {
  const int z1 = a.nz > 1 ? 1 : 0;
  ssh::Args c; c.a1 = a.h_a1; c.a2 = a.h_a2; c.a3 = a.h_a3; c.B = a.B; c.G = (a.B + ns - 1) / ns;
  c.w2[0] = a.wht[0] + OFF2; c.w2[1] = a.wht[z1] + OFF2; c.w3[0] = a.wht[0] + OFF3; c.w3[1] = a.wht[z1] + OFF3;
  c.src = a.src; c.idx = a.idx; c.from_ring = a.from_ring; c.post_off = a.post_off; c.a1w = a.h_a1; c.w1[0] = a.wht[0] + OFF1; c.w1[1] = a.wht[z1] + OFF1;
  return c;
}

hipError_t launch_ss(const Route& r, int, const StepArgs& a, const LaunchTune& t, hipStream_t s) {
  switch (r.form) {
    case SSH_DGRAD_CHAIN: case SSH_DGRAD_CHAIN_WB: {
      ssh::DArgs c; c.d3p = a.h_d3p; c.w3 = a.wh[0] + OFF3; c.w2 = a.wh[0] + OFF2; c.a2 = a.h_a2; c.a1 = a.h_a1; c.d2 = a.h_d2; c.d1 = a.h_d1; c.B = a.B;
      return r.form == SSH_DGRAD_CHAIN ? ssh::launch_dgrad_chain<true>(c, s) : ssh::launch_dgrad_chain<false>(c, s);
    }
    case SSH_CHAIN_C1_NS2: return ssh::launch_chain<2, true, true>(ssh_chain_args(a, 2), a.nz, s);
    case SSH_CHAIN_C1_NS2_WB: return ssh::launch_chain<2, false, true>(ssh_chain_args(a, 2), a.nz, s);
    case SSH_CHAIN_C1_NS1: return ssh::launch_chain<1, true, true>(ssh_chain_args(a, 1), a.nz, s);
    case SSH_CHAIN_C1_NS1_WB: return ssh::launch_chain<1, false, true>(ssh_chain_args(a, 1), a.nz, s);
    case SSH_CHAIN_NS2: return ssh::launch_chain<2, true, false>(ssh_chain_args(a, 2), a.nz, s);
    case SSH_CHAIN_NS2_WB: return ssh::launch_chain<2, false, false>(ssh_chain_args(a, 2), a.nz, s);
    case SSH_CHAIN_NS1: return ssh::launch_chain<1, true, false>(ssh_chain_args(a, 1), a.nz, s);
    case SSH_CHAIN_NS1_WB: return ssh::launch_chain<1, false, false>(ssh_chain_args(a, 1), a.nz, s);
    case SS_CHAIN_NS2: case SS_CHAIN_NS1: case SS_CONV2_NS2: case SS_CONV2_NS1: case SS_CONV3_NS2: case SS_CONV3_NS1: break;
    default: return hipErrorInvalidValue;
  }
  const int ns = (r.form == SS_CHAIN_NS2 || r.form == SS_CONV2_NS2 || r.form == SS_CONV3_NS2) ? 2 : 1;
  ss::Args c2, c3;
  c2.B = c3.B = a.B; c2.G = c3.G = (a.B + ns - 1) / ns; c2.dbg = c3.dbg = 0;
#ifdef SDQN_TIMING
  if (const char* e = getenv("SDQN_SS_DBG")) c2.dbg = c3.dbg = atoi(e);
#endif
  c2.in = a.a1; c2.out = a.a2; c2.w[0] = a.theta[0] + OFF2; c2.w[1] = a.theta[a.nz > 1 ? 1 : 0] + OFF2; c2.wt = (t.wt & WT_CONV2_FWD) ? 1 : 0;
  c3.in = a.a2; c3.out = a.a3; c3.w[0] = a.theta[0] + OFF3; c3.w[1] = a.theta[a.nz > 1 ? 1 : 0] + OFF3; c3.wt = (t.wt & WT_CONV3_FWD) ? 1 : 0;
  if (r.form == SS_CHAIN_NS2 || r.form == SS_CHAIN_NS1) {
    ss::ChainArgs cc; cc.l1 = c2; cc.l2 = c3;
    return ns == 2 ? ss::launch_chain<C2S2, C3S2>(cc, a.nz, s) : ss::launch_chain<C2S1, C3S1>(cc, a.nz, s);
  }
  if (r.form == SS_CONV2_NS2 || r.form == SS_CONV2_NS1) return ns == 2 ? ss::launch<C2S2>(c2, a.nz, s) : ss::launch<C2S1>(c2, a.nz, s);
  return ns == 2 ? ss::launch<C3S2>(c3, a.nz, s) : ss::launch<C3S1>(c3, a.nz, s);
}

#ifdef SDQN_TIMING
hipError_t set_timing_buffer_ss(unsigned long long* p) { return hipMemcpyToSymbol(HIP_SYMBOL(g_sdqn_dbg), &p, sizeof p); }
#endif

}  // namespace sdqn

// launch_route.h — WHICH kernel runs for a stage of the train step, decided once and in one place.  Plain C++17 (no HIP include: tests/emul
// builds it with g++).  resolve_route() maps (kernel id, RouteKey, LaunchTune) to a Route = the translation unit that launches + the concrete
// launch form there, or "rides in the launch of another id"; the executors (launch_lat / _ext / _r3 / _bt / _ss, one per translation unit)
// only build arguments for the form they are handed.  Priority, first match wins:
//   sample-stationary chains -> block tiles -> round-3 variants -> float16 (ext) -> batch-norm -> nw override -> throughput regime -> default.
// tests/test_launch_route.py pins the whole table (tests/golden/launch_routes.txt) and the riding rules; DESIGN.md 12 prints it.
#pragma once
#include <cstdint>

namespace sdqn {

enum KernelId {
  K_CONV1_FWD = 0, K_CONV2_FWD, K_CONV3_FWD, K_FC4_FWD, K_HEAD,
  K_FC4_DGRAD, K_FC4_WGRAD, K_CONV3_DGRAD, K_CONV3_WGRAD, K_CONV2_DGRAD, K_CONV2_WGRAD,
  K_CONV1_WGRAD, K_UPDATE, K_ALLREDUCE, K_GATHER, K_PREP,
  K_BWD3,      // one launch: conv3_dgrad + conv3_wgrad + fc4_wgrad (all depend on fc4_dgrad only)
  K_BWD2,      // one launch: conv2_dgrad + conv2_wgrad (both depend on conv3_dgrad only) + a share of fc4_wgrad
  K_BWD1,      // one launch: conv1_wgrad + the last share of fc4_wgrad
  K_BN,        // --batch_norm: one BatchNorm layer, forward ([partial +] apply) or backward (partial + apply)
  K_SHIFT,     // --random_shift: the shifted minibatch, one launch in front of the step (sdqn_shift.hip); the id of a retired round-3 launch, reused
  K_RESERVED_21, K_RESERVED_22, K_RESERVED_23,   // ids of retired round-3 launches: the numbers are public (options bt:/xcd:/nw:<id>, profile_read), nothing launches them
  K_WGRADS,    // round 4 (float16, B >= 128): fc4_wgrad (+ fused RMSProp) || conv3_wgrad || conv2_wgrad in one launch, after the block-tile dgrad chain
  K_ACT,       // round 4: the acting forward (batch of one) as ONE launch (sdqn_act.hip)
  K_COLLECT,   // --train_envs: one lockstep of N games of catch written into the laned ring (sdqn_env.hip; not a launch of the train step)
  K_TARGET,    // --target_tau: the soft target update, one launch behind the step's update launch (sdqn_target.hip / generic_net.hip)
  K_COUNT
};
// HeadArgs::train / StepPlan::head_train: what the K_HEAD launch runs.  The numbers are public (tools/step_trace prints them into the goldens)
enum HeadMode {
  HEAD_PREDICT = 0,     // predict only (z = 0)
  HEAD_TRAIN,           // train step
  HEAD_DOUBLE,          // train step with Double DQN targets (--double_dqn)
  HEAD_MUNCHAUSEN,      // ... with Munchausen targets (--munchausen; munchausen_head_kernel, sdqn_munchausen.hip)
  HEAD_BOOTSTRAP,       // train step of a K-head bootstrapped net (--bootstrap_heads; bootstrap_head_kernel, sdqn_bootstrap.hip, its BootArgs beside HeadArgs)
  HEAD_ADVANTAGE,       // train step with advantage-learning targets (--advantage_learning; advantage_head_kernel, sdqn_advantage.hip)
  HEAD_QUANTILE,        // train step of an N-quantile net (--quantiles N > 1; quantile_head_kernel, sdqn_quantile.hip, its QuantArgs beside HeadArgs;
                        // HeadArgs::clip_error is the Huber threshold kappa there)
  HEAD_DUELING,         // train step of a dueling net (--dueling; dueling_head_kernel, sdqn_dueling.hip, its DuelArgs beside HeadArgs)
  HEAD_CQL              // train step with the conservative Q-learning regulariser (--cql_alpha; cql_head_kernel, sdqn_cql.hip)
};
static_assert(HEAD_TRAIN == 1 && HEAD_DOUBLE == 2 && HEAD_MUNCHAUSEN == 3 && HEAD_BOOTSTRAP == 4 && HEAD_ADVANTAGE == 5 && HEAD_QUANTILE == 6 && HEAD_DUELING == 7 && HEAD_CQL == 8, "head modes are public numbers");
static_assert(K_BN == 19 && K_WGRADS == 24 && K_ACT == 25 && K_COLLECT == 26 && K_TARGET == 27 && K_COUNT == 28, "kernel ids are public numbers");

// LaunchTune::variant — the launch variants the step's orchestration asks for (sdqn_api_step.hip decides, resolve_route tests); bit 0 is unused
enum LaunchVariant {
  LV_CONV3_C36 = 2,           // conv3_fwd on 36-deep K-chunks (sdqn_kernels_r3.hip)
  LV_CONV1_FWD_BF16 = 4,      // conv1_fwd on packed-bf16 MFMA (sdqn_kernels_r3.hip)
  LV_CONV1_WGRAD_BF16 = 8,    // conv1_wgrad on packed-bf16 MFMA (sdqn_kernels_r3.hip)
  LV_C1W_IN_WGRADS = 16,      // float16, B >= 128: conv1_wgrad rides in the K_WGRADS launch and K_BWD1 launches nothing (sdqn_kernels_bt.hip)
  LV_C1W_FIRST = 32,          // ... with its workgroups first in the block-id order
};
// LaunchTune::wt / option "wt" — write-through (sc1) epilogue stores, one bit per launch (WT_UPDATE reaches its kernel as UpdateArgs::wt)
enum WriteThrough {
  WT_CONV2_FWD = 1, WT_CONV3_FWD = 2, WT_FC4_FWD = 4, WT_FC4_DGRAD = 8, WT_BWD3 = 16, WT_BWD2 = 32, WT_CONV1_WGRAD = 64, WT_CONV1_FWD = 128,
  WT_UPDATE = 256, WT_ALL = 511
};
// host-side launch choices that never reach a kernel (kept out of StepArgs: kernel-argument bytes are not free)
struct LaunchTune {
  int nw_override[12];      // tuning hook: waves per tile for kernel id i (0 = built-in choice)
  const int64_t* host_idx;  // ring paths, B <= 32: this step's sampled indexes in HOST memory (they ride in the kernel arguments of conv1_bf16_kernel)
  int r3_xcd;               // round-3 kernels' XCD-contiguous tile maps: bit 0 conv1_fwd (bf16), bit 1 conv1_wgrad (bf16)
  int wt;                   // WriteThrough bits
  int bt[K_COUNT];          // block-tile / sample-stationary menu per kernel id: 0 = built-in, n > 0 = menu entry, < 0 = latency engine (table: DESIGN.md 12)
  int variant;              // LaunchVariant bits
};

// what routing reads of a launch's StepArgs, and nothing else (kernels.h: route_key fills it)
struct RouteKey {
  int B, nz;
  int h16;                  // 0 float32, 1 float16 with fp32-MFMA weight gradients, 2 float16 throughout
  int bn;
  int f4w_count;            // fc4_wgrad tiles riding in this backward launch
  int from_ring, tps1;
  bool has_src;             // StepArgs::src != nullptr
  bool has_w1p;             // conv1's bf16 planes of every net slot of this launch exist
  bool has_host_idx;        // LaunchTune::host_idx != nullptr
};

enum RouteUnit { U_NONE = 0, U_LAT, U_EXT, U_R3, U_BT, U_SS };      // U_NONE: rides in the launch of Route::rides_in

// the concrete launch inside its unit.  *_MENU0 + n = menu entry n of that family (LaunchTune::bt[id]); NS1 / NS2 = samples per workgroup;
// WB = plain (write-back) stores where the built-in form writes through
enum RouteForm {
  FORM_NONE = 0,            // launches nothing
  FORM_INVALID,             // the options name a launch that does not exist (an nw override outside 1 / 2 / 4 / 8 / 16, an id without kernels): hipErrorInvalidValue
  // sdqn_kernels_ss.hip
  SS_CONV2_NS1, SS_CONV2_NS2, SS_CONV3_NS1, SS_CONV3_NS2, SS_CHAIN_NS1, SS_CHAIN_NS2,      // float32, B >= 128: conv2 / conv3 forward alone, or as one launch at K_CONV2_FWD
  SSH_CHAIN_NS1, SSH_CHAIN_NS2, SSH_CHAIN_NS1_WB, SSH_CHAIN_NS2_WB,                         // float16: conv2 -> conv3 forward at K_CONV2_FWD
  SSH_CHAIN_C1_NS1, SSH_CHAIN_C1_NS2, SSH_CHAIN_C1_NS1_WB, SSH_CHAIN_C1_NS2_WB,             //   ... with conv1 in front of it
  SSH_DGRAD_CHAIN, SSH_DGRAD_CHAIN_WB,                                                      // float16, B >= 128: conv3_dgrad -> conv2_dgrad at K_CONV3_DGRAD
  // sdqn_kernels_bt.hip
  BT_CONV1_H_DIV255, BT_CONV1_H_EXACT, BT_CONV1_H_EXACT_WB,     // float16 conv1 forward, one workgroup per (net, sample)
  BT_C1W_H_DIV255, BT_C1W_H_EXACT,                              // float16 conv1 weight gradient on 80-position chunks
  BT_C1W_BYTES, BT_C1W_TR,                                      // float32 conv1 weight gradient: single-byte LDS reads / transpose reads
  BT_WGRADS, BT_WGRADS_D4, BT_WGRADS_D3, BT_WGRADS_C1W_LAST, BT_WGRADS_C1W_FIRST,      // float16 K_WGRADS: 2 / 4 / 3 chunks in flight; conv1_wgrad riding
  BT_H_MENU0, BT_H_MENU1, BT_H_MENU2, BT_H_MENU3, BT_H_MENU4, BT_H_MENU5, BT_H_MENU6,   // float16 forward / dgrad block shapes
  BT_SINGLE_MENU0, BT_SINGLE_MENU1, BT_SINGLE_MENU2, BT_SINGLE_MENU3, BT_SINGLE_MENU4, BT_SINGLE_MENU5, BT_SINGLE_MENU6, BT_SINGLE_MENU7, BT_SINGLE_MENU8,
  BT_FUSED_MENU0, BT_FUSED_MENU1, BT_FUSED_MENU2, BT_FUSED_MENU3, BT_FUSED_MENU4, BT_FUSED_MENU5, BT_FUSED_MENU6, BT_FUSED_MENU7,
  // sdqn_kernels_r3.hip
  R3_CONV1_BF16, R3_CONV1_BF16_IDX, R3_CONV1_BF16_ROWS,        // per-tile kernel, with the indexes in the arguments, persistent rows kernel (B >= 128)
  R3_C1W_BF16, R3_C1W_BF16_IDX,
  R3_WT_H16_B32, R3_WT_B32, R3_WT_B128,                         // the default launch forms with write-through epilogues
  R3_CONV3_C36, R3_CONV3_C36_WT,
  // sdqn_kernels_ext.hip (float16 on the latency engine)
  EXT_NW1, EXT_NW2, EXT_NW4, EXT_NW8, EXT_NW16,
  EXT_HW_B32, EXT_HW,                                           // h16 == 2: weight gradients on packed-fp16 MFMA (B <= 32 / above)
  EXT_DEFAULT_B32, EXT_DEFAULT,
  // sdqn_kernels.hip (float32 on the latency engine)
  LAT_BN, LAT_BN_B128,                                          // raw (pre-BatchNorm) forward outputs
  LAT_NW2, LAT_NW4, LAT_NW8, LAT_NW9, LAT_NW16,                 // nw override (9: conv3_fwd staged on 9 waves)
  LAT_THROUGHPUT, LAT_THROUGHPUT_F4W,                           // B >= 128 (F4W: fc4_wgrad rides in bwd3)
  LAT_DEFAULT, LAT_DEFAULT_F4W, LAT_DEFAULT_B32_F4W,            // (F4W: a share of fc4_wgrad rides in the backward launch; B <= 32: one wave per tile)
  LAT_F4W_NW1, LAT_F4W_NW2, LAT_F4W_NW4, LAT_F4W_NW8,           // fc4_wgrad alone: K = B
  FORM_COUNT
};

struct Route { RouteUnit unit; RouteForm form; int rides_in; };      // rides_in: a kernel id when unit == U_NONE, else -1

namespace route {
constexpr uint32_t bit(int id) { return id >= 0 && id < 32 ? 1u << id : 0u; }
constexpr bool in(uint32_t set, int id) { return (set & bit(id)) != 0; }
constexpr int C1W_CHUNK = 80;        // conv1_wgrad's block-tile kernels take K slabs of whole 80-position chunks (sdqn_kernels_bt.hip: C1W_CH)
constexpr bool c1w_slabs_fit(const RouteKey& k) { return (k.tps1 * 32) % C1W_CHUNK == 0; }
constexpr uint32_t FWD_DGRAD = bit(K_CONV1_FWD) | bit(K_CONV2_FWD) | bit(K_CONV3_FWD) | bit(K_FC4_FWD) | bit(K_FC4_DGRAD) | bit(K_CONV3_DGRAD) | bit(K_CONV2_DGRAD);
constexpr uint32_t WGRADS = bit(K_FC4_WGRAD) | bit(K_CONV3_WGRAD) | bit(K_CONV2_WGRAD) | bit(K_CONV1_WGRAD);
constexpr uint32_t FUSED = bit(K_BWD3) | bit(K_BWD2) | bit(K_BWD1);
// ---- which (id, menu entry) pairs exist: bit n of the row = menu entry n ------------------------------------------------------------------
constexpr int BT_MENU_MAX = 8;
constexpr uint16_t ANY = 0xFFFF;                 // one block shape, whatever the entry
constexpr uint16_t bt_single_menu(int id) {      // float32, B >= 128 (sdqn_kernels_bt.hip: launch_single)
  return id == K_CONV2_FWD || id == K_CONV3_FWD ? 0x07F : id == K_FC4_FWD ? 0x13F : id == K_FC4_DGRAD ? 0x03F
       : id == K_FC4_WGRAD || id == K_CONV3_DGRAD || id == K_CONV3_WGRAD || id == K_CONV2_DGRAD || id == K_CONV2_WGRAD ? ANY : 0;
}
constexpr uint16_t bt_fused_menu(int id, bool f4w) {      // launch_fused: bwd2 has no form that carries fc4_wgrad tiles
  return id == K_BWD3 || (id == K_BWD2 && !f4w) ? 0x09F : 0;
}
constexpr uint16_t bt_h_menu(int id) {           // float16, B >= 128 (launch_single_h)
  return id == K_CONV2_FWD || id == K_CONV3_FWD || id == K_CONV3_DGRAD || id == K_CONV2_DGRAD ? 0x4F : id == K_FC4_FWD || id == K_FC4_DGRAD ? 0x0F : 0;
}
constexpr bool menu_has(uint16_t row, int entry) { return row == ANY || (entry >= 0 && entry <= BT_MENU_MAX && ((row >> entry) & 1)); }
// ---- which ids each latency-engine family launches ---------------------------------------------------------------------------------------
constexpr uint32_t LAT_BN_IDS = bit(K_CONV1_FWD) | bit(K_CONV2_FWD) | bit(K_CONV3_FWD);
constexpr uint32_t LAT_NW_IDS = (FWD_DGRAD | WGRADS) & ~bit(K_FC4_WGRAD);        // (fc4_wgrad's wave count follows B)
constexpr uint32_t LAT_THROUGHPUT_IDS = FWD_DGRAD | bit(K_BWD3) | bit(K_BWD2);
constexpr uint32_t LAT_DEFAULT_IDS = FWD_DGRAD | WGRADS | FUSED;
constexpr uint32_t EXT_NW_IDS = FWD_DGRAD | WGRADS;
constexpr uint32_t EXT_HW_IDS = WGRADS | FUSED | bit(K_WGRADS);
constexpr uint32_t EXT_DEFAULT_IDS = FWD_DGRAD | WGRADS | FUSED | bit(K_WGRADS);
// write-through bit of a launch id in each R3_WT_* family (0: the family has no such launch)
constexpr int r3_wt_h16_b32(int id) {
  return id == K_CONV1_FWD ? WT_CONV1_FWD : id == K_CONV2_FWD ? WT_CONV2_FWD : id == K_CONV3_FWD ? WT_CONV3_FWD : id == K_FC4_FWD ? WT_FC4_FWD
       : id == K_FC4_DGRAD ? WT_FC4_DGRAD : id == K_BWD2 ? WT_BWD2 : id == K_BWD1 ? WT_CONV1_WGRAD : 0;
}
constexpr int r3_wt_f32(int id, bool b128, bool f4w, bool c1w_bf16) {      // bwd3 only with, bwd2 / bwd1 only without fc4_wgrad tiles
  return id == K_CONV2_FWD ? WT_CONV2_FWD : id == K_CONV3_FWD && b128 ? WT_CONV3_FWD : id == K_FC4_FWD ? WT_FC4_FWD : id == K_FC4_DGRAD ? WT_FC4_DGRAD
       : id == K_BWD3 && f4w ? WT_BWD3 : id == K_BWD2 && !f4w ? WT_BWD2 : id == K_BWD1 && b128 && !f4w && !c1w_bf16 ? WT_CONV1_WGRAD : 0;
}

inline Route launches(RouteUnit u, RouteForm f) { return Route{u, f, -1}; }
inline Route rides(int in_id) { return Route{U_NONE, FORM_NONE, in_id}; }
inline bool nw_set(int id, const LaunchTune& t) { return id >= 0 && id < 12 && t.nw_override[id] > 0; }
// a chain's menu: 0 / 7 = the chain, 8 = its second form, anything else (or an nw override) hands the launch back
inline bool chain_menu(int id, const LaunchTune& t) { return (t.bt[id] == 0 || t.bt[id] == 7 || t.bt[id] == 8) && !(t.nw_override[id] > 0); }

// float32, B >= 128: does conv2 / conv3 forward run on the sample-stationary routine?  bt[id]: 0 = where its workgroups fill the chip, 7 / 8 = always
inline bool ss_takes(int id, const RouteKey& k, const LaunchTune& t) {
  if (k.B < 128 || k.bn || k.h16) return false;
  if (k.nz == 3 && t.bt[id] == 0 && t.nw_override[id] == 0) return true;    // --double_dqn: the third slot rides in the same launches
  if (!chain_menu(id, t)) return false;
  // one workgroup per CU, NS whole samples each: the routine pays when its workgroups fill (nearly) whole rounds of the chip's 256 CUs —
  // B = 128 and 256 with both nets, B = 256 alone (predict) — and loses to the block-tile engine's finer blocks in between (measured,
  // conv2 / conv3 forward, us: B = 160: 23.8 / 17.4 against 20.7 / 14.0; B = 256: 26.1 / 18.9 against 28.7 / 22.3): below 80 % it declines
  const int ns = k.nz * k.B > 256 ? 2 : 1;
  const int wgs = k.nz * ((k.B + ns - 1) / ns), rounds = (wgs + 255) / 256;
  return t.bt[id] != 0 || wgs * 5 >= rounds * 256 * 4;
}
// ... both layers there: ONE launch at K_CONV2_FWD, nothing at K_CONV3_FWD — unless menu entry 8 asks for the two launches (tests, same-box A/B)
inline bool ss_chains(const RouteKey& k, const LaunchTune& t) {
  return ss_takes(K_CONV2_FWD, k, t) && ss_takes(K_CONV3_FWD, k, t) && t.bt[K_CONV2_FWD] != 8 && t.bt[K_CONV3_FWD] != 8;
}
// float16, ANY batch size: conv2 -> conv3 forward as one launch.  No fill rule — the launch is data movement and latency, not matrix time, and
// wins wherever it was measured (fused-loop steps/s, chain against the launches it replaces: B = 32 18 894 vs 17 594, 64 13 399 vs 12 006,
// 100 10 487 vs 9 115, 160 12 181 vs 11 711, 192 11 786 vs 11 138)
inline bool ssh_takes(const RouteKey& k, const LaunchTune& t) {
  return k.h16 && !k.bn && chain_menu(K_CONV2_FWD, t) && chain_menu(K_CONV3_FWD, t) && t.bt[K_CONV2_FWD] == t.bt[K_CONV3_FWD];
}
// float16, B >= 128 (where the two dgrads are launches of their own): conv3_dgrad -> conv2_dgrad as one launch.  Measured with the forward
// chain on, steps/s: B = 128 14 761 vs 13 641, 160 13 451 vs 12 181, 192 13 059 vs 11 786, 256 11 900 vs 10 575
inline bool ssh_dgrad_takes(const RouteKey& k, const LaunchTune& t) {
  return k.h16 && k.B >= 128 && !k.bn && chain_menu(K_CONV3_DGRAD, t) && chain_menu(K_CONV2_DGRAD, t) && t.bt[K_CONV3_DGRAD] == t.bt[K_CONV2_DGRAD];
}
// float16: conv1 rides in FRONT of the forward chain wherever the chain runs and nothing asks for a conv1 launch of its own
inline bool ssh_c1(const RouteKey& k, const LaunchTune& t) {
  return ssh_takes(k, t) && t.bt[K_CONV1_FWD] == 0 && t.nw_override[K_CONV1_FWD] == 0 && k.has_src;
}

inline bool route_ss(int id, const RouteKey& k, const LaunchTune& t, Route& r) {
  const bool ns2 = k.nz * k.B > 256;
  if (id == K_CONV1_FWD) {
    if (!(k.h16 && ssh_c1(k, t))) return false;
    r = rides(K_CONV2_FWD); return true;
  }
  if (id == K_CONV3_DGRAD || id == K_CONV2_DGRAD) {
    if (!ssh_dgrad_takes(k, t)) return false;
    r = id == K_CONV2_DGRAD ? rides(K_CONV3_DGRAD) : launches(U_SS, t.bt[K_CONV3_DGRAD] != 8 ? SSH_DGRAD_CHAIN : SSH_DGRAD_CHAIN_WB);
    return true;
  }
  if (id != K_CONV2_FWD && id != K_CONV3_FWD) return false;
  if (k.h16) {
    if (!ssh_takes(k, t)) return false;
    if (id == K_CONV3_FWD) { r = rides(K_CONV2_FWD); return true; }
    const bool wb = t.bt[K_CONV2_FWD] == 8;
    const RouteForm f = ssh_c1(k, t) ? (ns2 ? (wb ? SSH_CHAIN_C1_NS2_WB : SSH_CHAIN_C1_NS2) : (wb ? SSH_CHAIN_C1_NS1_WB : SSH_CHAIN_C1_NS1))
                                     : (ns2 ? (wb ? SSH_CHAIN_NS2_WB : SSH_CHAIN_NS2) : (wb ? SSH_CHAIN_NS1_WB : SSH_CHAIN_NS1));
    r = launches(U_SS, f); return true;
  }
  if (!ss_takes(id, k, t)) return false;
  if (ss_chains(k, t)) r = id == K_CONV3_FWD ? rides(K_CONV2_FWD) : launches(U_SS, ns2 ? SS_CHAIN_NS2 : SS_CHAIN_NS1);
  else if (id == K_CONV2_FWD) r = launches(U_SS, ns2 ? SS_CONV2_NS2 : SS_CONV2_NS1);
  else r = launches(U_SS, ns2 ? SS_CONV3_NS2 : SS_CONV3_NS1);
  return true;
}

// the block-tile engine and the hand-written kernels beside it: B >= 128, and float16's exact-byte conv1 kernels below that
inline bool route_bt(int id, const RouteKey& k, const LaunchTune& t, Route& r) {
  if (k.bn || id < 0 || id >= K_COUNT || t.bt[id] < 0) return false;
  const int m = t.bt[id];
  const bool nw = nw_set(id, t);
  if (k.B < 128) {
    // conv1 forward, one workgroup per (net, sample): pays from 2 x 48 workgroups up (fused-loop steps/s against the latency engine's tiles:
    // B = 32 18 490 vs 18 755, 48 14 833 vs 14 527, 64 13 943 vs 13 370, 100 11 198 vs 10 453); menu entry 7 = always, 6 = never
    if (k.h16 && id == K_CONV1_FWD && (m == 7 || (m == 0 && k.B >= 48)) && t.nw_override[id] == 0) { r = launches(U_BT, BT_CONV1_H_EXACT); return true; }
    if (k.h16 == 2 && id == K_BWD1 && m == 7 && k.f4w_count == 0 && c1w_slabs_fit(k)) { r = launches(U_BT, BT_C1W_H_EXACT); return true; }
    return false;
  }
  if (k.h16) {
    if (id == K_WGRADS && k.h16 == 2) {
      // LV_C1W_IN_WGRADS (the step orchestration's decision): conv1's weight gradient rides in this launch and K_BWD1 launches nothing
      if (t.variant & LV_C1W_IN_WGRADS) r = launches(U_BT, (t.variant & LV_C1W_FIRST) ? BT_WGRADS_C1W_FIRST : BT_WGRADS_C1W_LAST);
      else r = launches(U_BT, m == 1 ? BT_WGRADS_D4 : m == 2 ? BT_WGRADS_D3 : BT_WGRADS);
      return true;
    }
    if (id == K_CONV1_FWD && m <= 2 && t.nw_override[id] == 0) {
      r = launches(U_BT, m == 1 ? BT_CONV1_H_DIV255 : m == 2 ? BT_CONV1_H_EXACT_WB : BT_CONV1_H_EXACT); return true;
    }
    if (id == K_BWD1 && (t.variant & LV_C1W_IN_WGRADS)) { r = rides(K_WGRADS); return true; }
    if (id == K_BWD1 && k.h16 == 2 && k.f4w_count == 0) {
      if (!c1w_slabs_fit(k)) return false;
      r = launches(U_BT, m == 1 ? BT_C1W_H_DIV255 : BT_C1W_H_EXACT); return true;
    }
    if (id >= 12 || nw || !menu_has(bt_h_menu(id), m)) return false;
    r = launches(U_BT, (RouteForm)(BT_H_MENU0 + m)); return true;
  }
  // fc4 forward has 64 blocks of 64 x 64 per K slab and measured slower here than on the latency engine (21.0 vs 18.1 us at B = 256 with 7
  // slabs and unconditional ring loads): block-tile only on request (menu entry > 0)
  if (id == K_FC4_FWD && m == 0) return false;
  if (nw) return false;                       // explicit latency-engine tuning hooks win
  if ((id == K_BWD1 && k.f4w_count == 0) || id == K_CONV1_WGRAD) {
    if (!c1w_slabs_fit(k)) return false;      // other slab sizes stay on the latency engine's kernel
    r = launches(U_BT, m == 1 ? BT_C1W_BYTES : BT_C1W_TR); return true;
  }
  if (menu_has(bt_fused_menu(id, k.f4w_count > 0), m)) { r = launches(U_BT, (RouteForm)(BT_FUSED_MENU0 + m)); return true; }
  if (menu_has(bt_single_menu(id), m)) { r = launches(U_BT, (RouteForm)(BT_SINGLE_MENU0 + (m <= BT_MENU_MAX ? m : 0))); return true; }
  return false;
}

// round-3 launch variants: asked for by LaunchVariant bits or write-through bits
inline bool route_r3(int id, const RouteKey& k, const LaunchTune& t, Route& r) {
  const bool idx = k.has_host_idx && k.from_ring && k.B <= 32, f32 = !k.h16 && !k.bn;
  if (id == K_CONV1_FWD && (t.variant & LV_CONV1_FWD_BF16) && f32 && k.has_w1p) {
    // (throughput regime: the persistent rows kernel; option bt:0 = -1: the per-tile kernel, the test reference)
    r = launches(U_R3, k.B >= 128 && t.bt[K_CONV1_FWD] >= 0 ? R3_CONV1_BF16_ROWS : idx ? R3_CONV1_BF16_IDX : R3_CONV1_BF16); return true;
  }
  if ((id == K_BWD1 || id == K_CONV1_WGRAD) && (t.variant & LV_CONV1_WGRAD_BF16) && (id == K_CONV1_WGRAD || k.f4w_count == 0) && f32) {
    r = launches(U_R3, idx ? R3_C1W_BF16_IDX : R3_C1W_BF16); return true;
  }
  if (t.wt && !k.bn && !nw_set(id, t)) {      // write-through epilogues: the default launch forms with the *WT problems
    if (k.B <= 32 && k.h16 == 2 && (t.wt & r3_wt_h16_b32(id))) { r = launches(U_R3, R3_WT_H16_B32); return true; }
    if ((k.B <= 32 || k.B >= 128) && !k.h16 && (t.wt & r3_wt_f32(id, k.B >= 128, k.f4w_count > 0, (t.variant & LV_CONV1_WGRAD_BF16) != 0))) {
      r = launches(U_R3, k.B >= 128 ? R3_WT_B128 : R3_WT_B32); return true;
    }
  }
  if (id == K_CONV3_FWD && (t.variant & LV_CONV3_C36) && k.B < 128 && f32) {
    r = launches(U_R3, (t.wt & WT_CONV3_FWD) && k.B <= 32 ? R3_CONV3_C36_WT : R3_CONV3_C36); return true;
  }
  return false;
}

inline RouteForm nw_form(int nw, RouteForm f1, RouteForm f2, RouteForm f4, RouteForm f8, RouteForm f16) {
  return nw == 1 ? f1 : nw == 2 ? f2 : nw == 4 ? f4 : nw == 8 ? f8 : nw == 16 ? f16 : FORM_INVALID;
}
// float16 on the latency engine takes whatever is left of a float16 step
inline Route route_ext(int id, const RouteKey& k, const LaunchTune& t) {
  if (nw_set(id, t) && in(EXT_NW_IDS, id)) return launches(U_EXT, nw_form(t.nw_override[id], EXT_NW1, EXT_NW2, EXT_NW4, EXT_NW8, EXT_NW16));
  if (k.h16 == 2 && in(EXT_HW_IDS, id)) return launches(U_EXT, k.B <= 32 ? EXT_HW_B32 : EXT_HW);
  return launches(U_EXT, !in(EXT_DEFAULT_IDS, id) ? FORM_INVALID : k.B <= 32 ? EXT_DEFAULT_B32 : EXT_DEFAULT);
}
inline Route route_lat(int id, const RouteKey& k, const LaunchTune& t) {
  const bool f4w = k.f4w_count > 0;
  if (k.bn && in(LAT_BN_IDS, id)) return launches(U_LAT, k.B >= 128 && id != K_CONV1_FWD ? LAT_BN_B128 : LAT_BN);
  if (nw_set(id, t) && in(LAT_NW_IDS, id)) {
    const int nw = t.nw_override[id];
    return launches(U_LAT, id == K_CONV3_FWD && nw == 9 ? LAT_NW9 : nw_form(nw, FORM_INVALID, LAT_NW2, LAT_NW4, LAT_NW8, LAT_NW16));
  }
  if (k.B >= 128 && in(LAT_THROUGHPUT_IDS, id)) return launches(U_LAT, id == K_BWD3 && f4w ? LAT_THROUGHPUT_F4W : LAT_THROUGHPUT);
  if (!in(LAT_DEFAULT_IDS, id)) return launches(U_LAT, FORM_INVALID);
  if (id == K_FC4_WGRAD) return launches(U_LAT, k.B <= 32 ? LAT_F4W_NW1 : k.B <= 64 ? LAT_F4W_NW2 : k.B <= 128 ? LAT_F4W_NW4 : LAT_F4W_NW8);
  if (in(FUSED, id) && f4w && (k.B <= 32 || id == K_BWD3)) return launches(U_LAT, k.B <= 32 ? LAT_DEFAULT_B32_F4W : LAT_DEFAULT_F4W);
  return launches(U_LAT, LAT_DEFAULT);
}
}  // namespace route

inline Route resolve_route(int id, const RouteKey& k, const LaunchTune& t) {
  Route r;
  if (k.B >= 128 || k.h16) {             // throughput regime, and float16 at any batch size
    if (route::route_ss(id, k, t, r)) return r;
    if (route::route_bt(id, k, t, r)) return r;
  }
  if ((t.variant || t.wt) && route::route_r3(id, k, t, r)) return r;
  return k.h16 ? route::route_ext(id, k, t) : route::route_lat(id, k, t);
}

inline const char* route_unit_name(RouteUnit u) {
  static const char* const n[] = {"none", "lat", "ext", "r3", "bt", "ss"};
  return u >= U_NONE && u <= U_SS ? n[u] : "?";
}
inline const char* route_form_name(RouteForm f) {
  static const char* const n[] = {
  "FORM_NONE", "FORM_INVALID", "SS_CONV2_NS1", "SS_CONV2_NS2", "SS_CONV3_NS1", "SS_CONV3_NS2", "SS_CHAIN_NS1", "SS_CHAIN_NS2", "SSH_CHAIN_NS1",
  "SSH_CHAIN_NS2", "SSH_CHAIN_NS1_WB", "SSH_CHAIN_NS2_WB", "SSH_CHAIN_C1_NS1", "SSH_CHAIN_C1_NS2", "SSH_CHAIN_C1_NS1_WB", "SSH_CHAIN_C1_NS2_WB",
  "SSH_DGRAD_CHAIN", "SSH_DGRAD_CHAIN_WB", "BT_CONV1_H_DIV255", "BT_CONV1_H_EXACT", "BT_CONV1_H_EXACT_WB", "BT_C1W_H_DIV255", "BT_C1W_H_EXACT",
  "BT_C1W_BYTES", "BT_C1W_TR", "BT_WGRADS", "BT_WGRADS_D4", "BT_WGRADS_D3", "BT_WGRADS_C1W_LAST", "BT_WGRADS_C1W_FIRST", "BT_H_MENU0", "BT_H_MENU1",
  "BT_H_MENU2", "BT_H_MENU3", "BT_H_MENU4", "BT_H_MENU5", "BT_H_MENU6", "BT_SINGLE_MENU0", "BT_SINGLE_MENU1", "BT_SINGLE_MENU2", "BT_SINGLE_MENU3",
  "BT_SINGLE_MENU4", "BT_SINGLE_MENU5", "BT_SINGLE_MENU6", "BT_SINGLE_MENU7", "BT_SINGLE_MENU8", "BT_FUSED_MENU0", "BT_FUSED_MENU1",
  "BT_FUSED_MENU2", "BT_FUSED_MENU3", "BT_FUSED_MENU4", "BT_FUSED_MENU5", "BT_FUSED_MENU6", "BT_FUSED_MENU7", "R3_CONV1_BF16", "R3_CONV1_BF16_IDX",
  "R3_CONV1_BF16_ROWS", "R3_C1W_BF16", "R3_C1W_BF16_IDX", "R3_WT_H16_B32", "R3_WT_B32", "R3_WT_B128", "R3_CONV3_C36", "R3_CONV3_C36_WT", "EXT_NW1",
  "EXT_NW2", "EXT_NW4", "EXT_NW8", "EXT_NW16", "EXT_HW_B32", "EXT_HW", "EXT_DEFAULT_B32", "EXT_DEFAULT", "LAT_BN", "LAT_BN_B128", "LAT_NW2",
  "LAT_NW4", "LAT_NW8", "LAT_NW9", "LAT_NW16", "LAT_THROUGHPUT", "LAT_THROUGHPUT_F4W", "LAT_DEFAULT", "LAT_DEFAULT_F4W", "LAT_DEFAULT_B32_F4W",
  "LAT_F4W_NW1", "LAT_F4W_NW2", "LAT_F4W_NW4", "LAT_F4W_NW8"};
  static_assert(sizeof n / sizeof n[0] == FORM_COUNT, "one name per RouteForm, in enum order");
  return f >= 0 && f < FORM_COUNT ? n[f] : "?";
}

}  // namespace sdqn

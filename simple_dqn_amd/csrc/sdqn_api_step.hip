// sdqn_api_step.hip — the train / predict step: launch orchestration (deepqnetwork.py:107-186) and the fused replay loops (agent.py:108-114)
#include "api_internal.h"

hipError_t dp_allreduce(sdqn_net_s* h, void* buf, size_t count, int dtype, void* comm, hipStream_t s) {
  h->nccl_rc = g_rccl.AllReduce(buf, buf, count, dtype, /*ncclSum*/ 0, comm, s);
  return h->nccl_rc == 0 ? hipSuccess : hipErrorUnknown;
}

// ---- the step ---------------------------------------------------------------------------------------------
// fc4's RMSProp rides in its weight-gradient tiles: only when the step's one update launch applies everything else (clipping and the
// data-parallel forms need ALL of g before any of it is applied), nobody wants to read the fc4 gradient, and the optimizer is RMSProp
static int plan_fuse_rms(const sdqn_net_s* h, UpdateForm update) { return (update == UPD_SINGLE && !h->keep_grads && h->cfg.optimizer == 0) ? 1 : 0; }
StepArgs step_args(sdqn_net_s* h) {
  StepArgs a; memset(&a, 0, sizeof a);
  a.B = h->B; a.A = h->A; a.nz = 2; a.theta[0] = h->theta; a.theta[1] = h->theta_t;
  a.a1 = h->a1; a.a2 = h->a2; a.a3 = h->a3; a.slab4 = h->slab4; a.a4 = h->a4; a.d4 = h->d4; a.d3p = h->d3p; a.d2p = h->d2p; a.d3 = h->d3; a.d2 = h->d2;
  a.d1 = h->d1; a.g = h->g; a.slab1 = h->slab1; a.slab2 = h->slab2; a.slab3 = h->slab3;
  a.S4 = h->S4; a.tps1 = h->tps1; a.tps2 = h->tps2; a.tps3 = h->tps3;

  a.xcd_map = h->xcd_map ? 7 : 0;
  a.arg_preload = h->arg_preload ? 1 : 0;
  if (h->cfg.datatype == 1) {
    a.h16 = h->h16_wgrad_mfma ? 2 : 1; a.h_a1 = h->h_a1; a.h_a2 = h->h_a2; a.h_a3 = h->h_a3; a.h_d4 = h->h_d4; a.h_d3p = h->h_d3p; a.h_d3 = h->h_d3;
    a.h_d2p = h->h_d2p; a.h_d2 = h->h_d2; a.h_d1 = h->h_d1; a.wh[0] = h->wh[0]; a.wh[1] = h->wh[1]; a.wht[0] = h->wht[0]; a.wht[1] = h->wht[1];
    a.wh_w = h->wh[0]; a.wht_w = h->wht[0];
    a.loss_scale = (float)h->cfg.loss_scale; a.inv_loss_scale = (float)(1.0 / h->cfg.loss_scale);
  }
  a.f4w_first = 0; a.f4w_count = F4_TILES;
  a.w1p[0] = h->w1p[0]; a.w1p[1] = h->w1p[1];
  a.fuse_rms = plan_fuse_rms(h, update_form(h));
  a.theta_w = h->theta; a.state = h->state; a.bsz = (float)h->B;
  a.rho = (float)h->cfg.decay_rate; a.one_minus_rho = (float)(1.0 - h->cfg.decay_rate);
  a.lr = (float)h->cfg.learning_rate; a.eps = (float)h->cfg.epsilon;
  a.post_off = h->opt.n_step;                  // ring paths: poststate = state(i + n - 1) (problems.h soff)
  return a;
}
double nstep_gamma_n(int n, double gamma) { double g = 1.0; for (int k = 0; k < n; ++k) g = g * gamma; return g; }
int nstep_match(const sdqn_net_s* h, const sdqn_replay_s* r) {
  const int rn = r->ns.n > 1 ? r->ns.n : 1;
  if (rn == 1 && h->opt.n_step == 1) return SDQN_OK;
  ARGCHK(rn == h->opt.n_step, "replay memory n_step %d != network n_step %d", rn, h->opt.n_step);
  ARGCHK(r->ns.gamma == h->cfg.discount_rate, "replay memory n-step discount %.17g != network discount_rate %.17g", r->ns.gamma, h->cfg.discount_rate);
  ARGCHK(r->ns.min_reward == h->cfg.min_reward && r->ns.max_reward == h->cfg.max_reward,
         "replay memory n-step reward clip [%g, %g] != network [%g, %g]", r->ns.min_reward, r->ns.max_reward, h->cfg.min_reward, h->cfg.max_reward);
  return SDQN_OK;
}
HeadArgs head_args(sdqn_net_s* h, int train) {
  HeadArgs hd; memset(&hd, 0, sizeof hd);
  hd.st_actions = h->st_act; hd.st_rewards = h->st_rew; hd.st_terminals = h->st_term;
  hd.q = h->q; hd.maxq = h->maxq; hd.dq = h->dq; hd.cost_terms = h->cost_terms;
  hd.discount = h->cfg.discount_rate; hd.min_reward = h->cfg.min_reward; hd.max_reward = h->cfg.max_reward;
  hd.clip_error = (float)h->cfg.clip_error; hd.train = train;
  if (h->opt.n_step > 1) { hd.nstep = h->opt.n_step; hd.gamma_n = h->opt.gamma_n; }      // (gamma_n is the n_step setter's: whoever fills a TrainOptions by hand with n_step > 1 sets it too, nstep_gamma_n)
  return hd;
}
// Overlapped data parallel: the previous step's fc4 all-reduce + update may still be running on g_comm.  Everything
// on the library stream that touches W4, its optimizer state or the fc4 gradient must come after it.
int join_comm(sdqn_net_s* h) {
  if (h->w4_pending) { HIPCHK(hipStreamWaitEvent(g_stream, h->ev_w4, 0)); h->w4_pending = false; }
  return SDQN_OK;
}
// --batch_norm: one BatchNorm layer's arguments (bn_kernels.hip)
BnArgs bn_args(sdqn_net_s* h, const StepArgs& a, int layer, int train) {
  BnArgs b; memset(&b, 0, sizeof b);
  const int pix[4] = {PIX1, PIX2, PIX3, 1};
  b.layer = layer; b.C = bn_features(layer); b.rows = a.B * pix[layer]; b.nz = a.nz; b.train = train; b.B = a.B;
  b.theta[0] = h->theta; b.theta[1] = h->theta_t; b.off_bn = h->NPW; b.partial = h->bn_partial;
  b.mean = h->bn_mean + bn_off(layer) / 2; b.rstd = h->bn_rstd + bn_off(layer) / 2; b.g = h->g;
  switch (layer) {
    case 0: b.x = h->x1; b.a = h->a1; b.d = h->d1; break;
    case 1: b.x = h->x2; b.a = h->a2; b.d = h->d2; b.dpad = h->d2p; b.PQ = PIX2; b.Qw = Q2; b.PD = PD2; b.pad = 1; break;
    case 2: b.x = h->x3; b.a = h->a3; b.d = h->d3; b.dpad = h->d3p; b.PQ = PIX3; b.Qw = Q3; b.PD = PD3; b.pad = 2; break;
    default: b.x = h->slab4; b.S4 = a.S4; b.a = h->a4; b.d = h->d4; break;
  }
  return b;
}
// tuning hook: per-launch XCD map mask override (sdqn_net_set_option "xcd:<id>", value = mask + 1; 0 = built-in)
#define XCD_TUNE(ARGS, KID) do { if (h->xcd_mask[KID] > 0) (ARGS).xcd_map = h->xcd_mask[KID] - 1; } while (0)
hipError_t launch_tuned(sdqn_net_s* h, int id, StepArgs a, hipStream_t s, int variant) {
  XCD_TUNE(a, id);
  LaunchTune t;
  for (int i = 0; i < 12; ++i) t.nw_override[i] = h->nw_override[i];
  for (int i = 0; i < K_COUNT; ++i) t.bt[i] = h->bt_on ? h->bt[i] : -1;
  t.variant = variant; t.host_idx = h->host_idx_cur; t.r3_xcd = h->r3_xcd; t.wt = h->wt;
  return launch_kernel(id, a, t, s);
}
static StepArgs planned(const StepArgs& a, const LaunchPlan& p) {
  StepArgs b = a; b.xcd_map = (a.xcd_map & p.xcd_keep) | p.xcd_bits; b.f4w_first = p.f4w_first; b.f4w_count = p.f4w_count;
  return b;
}
#define PLANNED_LAUNCH(KID, ARGS, L) LAUNCH(KID, launch_tuned(h, KID, planned(ARGS, (L)[KID]), g_stream, (L)[KID].variant))
// the forward's four GEMM launches (l[K_CONV1_FWD .. K_FC4_FWD]); --batch_norm: as the step's arguments have them
static void plan_forward(const sdqn_net_s* h, LaunchPlan* l) {
  if (h->bn) return;
  // XCD-contiguous tile map where it wins time (tools/sweep_xcd.py, tools/ab_options.py): conv1_fwd +0.5 %, conv2_fwd
  // +0.2 %, fc4_fwd +0.6 % of the step rate; slower for conv3_fwd, fc4_dgrad and every backward launch
  l[K_CONV1_FWD].xcd_keep = l[K_FC4_FWD].xcd_keep = 0; l[K_CONV1_FWD].xcd_bits = l[K_FC4_FWD].xcd_bits = 1;
  if (h->B < 128) { l[K_CONV2_FWD].xcd_keep = 0; l[K_CONV2_FWD].xcd_bits = 1; }   // block-tile routines (B >= 128): conv2_fwd 28.8 / 8.8 us round-robin, 28.9 / 9.0 on the map (fp32 / float16)
  if (h->conv1_bf16 && h->nw_override[K_CONV1_FWD] == 0) l[K_CONV1_FWD].variant = LV_CONV1_FWD_BF16;
  if (h->conv3_c36 && h->nw_override[K_CONV3_FWD] == 0) l[K_CONV3_FWD].variant = LV_CONV3_C36;
}
// deepqnetwork.py:83-89.  With batch_norm: [Convolution|Linear] -> BatchNorm -> Rectlin.  The GEMM stage writes the raw linear output
// (x_l), the BatchNorm pass turns it into the activation the next stage reads; training-mode statistics for the online net of a
// train step (:129), running statistics for the target net (:120) and predict (:180)
static int forward(sdqn_net_s* h, const StepArgs& a, const HeadArgs& hd, const LaunchPlan* l) {
  StepArgs f = a; f.bn = h->bn ? 1 : 0;
  float* const raw[3] = {h->x1, h->x2, h->x3}; float* StepArgs::* const out[3] = {&StepArgs::a1, &StepArgs::a2, &StepArgs::a3};
#define BN_FWD(L) do { if (h->bn) LAUNCH(K_BN, launch_bn_forward(bn_args(h, a, (L), hd.train != 0), g_stream)); } while (0)
  for (int c = K_CONV1_FWD; c <= K_CONV3_FWD; ++c) {           // (the three ids are the layer numbers)
    StepArgs fc = f; if (h->bn) fc.*out[c] = raw[c];
    PLANNED_LAUNCH(c, fc, l);
    BN_FWD(c);
  }
  { int rc = join_comm(h); if (rc) return rc; }                // conv1..3 of this step overlap the previous step's fc4 all-reduce
  PLANNED_LAUNCH(K_FC4_FWD, f, l);
  BN_FWD(3);
  const BootArgs boot = {h->opt.boot_K, game_actions(h), h->opt.boot_thresh, bootstrap_mask_seed(h->opt.boot_seed), a.idx};   // (read when HEAD_BOOTSTRAP; the ring indexes: set by the ring paths alone)
  const QuantArgs quant = {h->opt.quant_N, game_actions(h), h->quant_targets};      // (read when HEAD_QUANTILE)
  const DuelArgs duel = {h->opt.dueling ? 1 : 0, game_actions(h), h->duel_step};      // (read when HEAD_DUELING)
  LAUNCH(K_HEAD, launch_head(f, hd, g_stream, h->head_q_system, &boot, &quant, &duel));      // (head_q_system: the acting path, never with batch_norm)
  return SDQN_OK;
}
int run_forward(sdqn_net_s* h, const StepArgs& a, const HeadArgs& hd) {
  LaunchPlan l[K_FC4_FWD + 1]; plan_forward(h, l);
  h->redo_acts_live = false;               // (a forward of its own writes slot 0 of a1..a4: no longer the last train step's activations)
  return forward(h, a, hd, l);
}
UpdateArgs make_update_args(sdqn_net_s* h, const StepArgs& a) {
  UpdateArgs u; memset(&u, 0, sizeof u);
  u.arg_preload = a.arg_preload;
  u.theta = h->theta; u.state = h->state; u.g = h->g;
  u.slab[0] = h->slab1; u.slab[1] = h->slab2; u.slab[2] = h->slab3; u.ns[0] = h->ns1; u.ns[1] = h->ns2; u.ns[2] = h->ns3;
  u.dq = h->dq; u.a4 = h->a4; u.cost_terms = h->cost_terms; u.cost_out = h->cost_out; u.cost_accum = h->cost_accum;
  u.B = h->B; u.A = h->A;
  u.rho = (float)h->cfg.decay_rate; u.one_minus_rho = (float)(1.0 - h->cfg.decay_rate);
  u.lr = (float)h->cfg.learning_rate; u.eps = (float)h->cfg.epsilon;
  u.skip_fc4 = a.fuse_rms;
  u.opt = h->cfg.optimizer; u.state2 = h->state2;
  if (h->cfg.datatype == 1) { u.wh = h->wh[0]; u.wht = h->wht[0]; }
  u.w1p = h->w1p[0];
  u.wt = (h->wt & WT_UPDATE) ? 1 : 0;
  u.bn_first = h->bn ? h->NPW : 0;
  if (u.opt == 1) {            // Neon Adam [neon-recalled]: t = epoch + 1, l = lr*sqrt(1-b2^t)/(1-b1^t), math in Python floats
    const double b1 = h->cfg.beta_1, b2 = h->cfg.beta_2, t = (double)h->epoch + 1.0;
    u.beta1 = (float)b1; u.one_minus_beta1 = (float)(1.0 - b1); u.beta2 = (float)b2; u.one_minus_beta2 = (float)(1.0 - b2);
    u.lr_t = (float)(h->cfg.learning_rate * sqrt(1.0 - pow(b2, t)) / (1.0 - pow(b1, t)));
  }
  return u;
}
// One train step after the minibatch is in place (deepqnetwork.py:119-172): forward of both nets, head, backward, optimizer.
// Which launches run is a function of (batch regime, datatype, batch_norm, data-parallel form) only — `step_structure` below names it,
// DESIGN.md 12 tabulates it, tests/test_step_structure.py enumerates it:
//   fused      fc4_dgrad | bwd3 = conv3_dgrad || conv3_wgrad || fc4_wgrad (+ RMSProp of W4) | bwd2 = conv2_dgrad || conv2_wgrad | bwd1 = conv1_wgrad
//   h16_bt     float16, B >= 128: fc4_dgrad | conv3_dgrad | conv2_dgrad | wgrads = fc4_wgrad (+ RMSProp) || conv3_wgrad || conv2_wgrad | bwd1
//   dp_overlap fused, with ALL of fc4_wgrad in bwd3 and its all-reduce + update on the second communicator's stream
//   unfused    one launch per problem (option fused_launches = 0; batch_norm inserts its own passes between them)
StepStructure step_structure(const sdqn_net_s* h) {
  // --clip_grad_norm: the overlapped form applies fc4 before the whole gradient's norm exists, so a clipped step runs the serial form
  if (h->comm && h->comm2 && h->dp_overlap && h->fused_launches && !clip_on(h)) return STEP_DP_OVERLAP;
  if (h->cfg.datatype == 1 && h->B >= 128 && h->bt_on && !h->bn && h->fused_launches && h->bt[K_CONV3_DGRAD] >= 0 && h->bt[K_CONV2_DGRAD] >= 0 &&
      h->nw_override[K_CONV3_DGRAD] == 0 && h->nw_override[K_CONV2_DGRAD] == 0) return STEP_H16_BT;
  return h->fused_launches ? STEP_FUSED : STEP_UNFUSED;
}
// how the optimizer pass runs: 0 one update launch (fc4's RMSProp rode in its weight-gradient tiles) | 1 serial data parallel: local sums,
// one all-reduce of the flat gradient, apply | 2 overlapped data parallel (fc4's part already on its way) | 3 grad_only (local sums, nothing applied)
// | 4 single GPU with --clip_grad_norm: local sums, the two clip launches, apply (the serial data-parallel form clips inside form 1)
static UpdateForm update_form_of(const sdqn_net_s* h, StepStructure structure) {
  if (structure == STEP_DP_OVERLAP) return UPD_DP_OVERLAP;
  if (h->comm) return UPD_DP_SERIAL;
  if (h->grad_only) return UPD_GRAD_ONLY;
  // --dueling masks g between its sums and their application: the split tail a clipped step runs, with or without the clip's own launches
  // --noisy_nets forms g_sigma from g between the same two launches
  return (clip_on(h) || h->opt.dueling || h->noisy) ? UPD_CLIP : UPD_SINGLE;
}
UpdateForm update_form(const sdqn_net_s* h) { return update_form_of(h, step_structure(h)); }
// --clip_grad_norm: g holds the complete gradient sums (all layers [+ the BatchNorm beta | gamma block]); bsz is the divisor the
// optimizer pass behind this will use.  Two launches in the update slot; g is scaled in place, or left bit for bit when nothing is clipped.
int clip_gradient(sdqn_net_s* h, double bsz) {
  if (!clip_on(h)) return SDQN_OK;
  const int64_t n = h->NPW + (h->bn ? BN_PARAMS : 0);
  LAUNCH(K_UPDATE, launch_grad_sqnorm(h->g, n, h->clip_buf, g_stream));
  LAUNCH(K_UPDATE, launch_grad_scale(h->g, n, h->clip_buf, bsz, h->clip_grad_norm, h->clip_buf + CLIP_GRID, g_stream));
  h->clip_ran = true;
  return SDQN_OK;
}
extern "C" int sdqn_net_step_structure(sdqn_net_t h, int* structure, int* update) {
  ARGCHK(h && structure && update, "NULL argument");
  if (h->gen) { *structure = 4; *update = clip_on(h) ? (int)UPD_CLIP : 0; return SDQN_OK; }
  *structure = (int)step_structure(h); *update = (int)update_form(h);
  return SDQN_OK;
}
// --double_dqn: Q(theta, poststates), the argmax of the Double DQN target.  Without batch_norm it is the third net slot of the step's
// own forward launches (nz = 3: online weights, poststates; problems.h wslot / sslot), and the head takes a* from it.  With batch_norm
// the online slot's training-mode BatchNorm pass updates the running statistics that an inference-mode third slot of the same launch
// would read, so there it is a forward of its own in front of the step (run_extra_forward: online weights, poststates, running
// statistics as they stand before the step).  Without a target net (theta- aliases theta) Double DQN is standard DQN: nothing changes.
bool ddqn_active(const sdqn_net_s* h) { return h->opt.double_dqn && h->theta_t != h->theta; }
// A forward of its own in front of the step: the predict forward (nz = 1) of weight slot `wz` (0 online, 1 target: the net's theta and
// its wh / wht / w1p copies move to slot-0 position) on state slot `sz` (0 prestates; 1 poststates: post_off frames further in the ring,
// replay_memory.py:71-72, or the second half of the [2][B][STATE] staging), its Q-values left in q slot 2.  It uses slot 0 of the
// activation buffers, which the step's own forward overwrites behind it.
//   --double_dqn with --batch_norm: (0, 1)        --munchausen / --advantage_learning: (1, 0), qbar of the prestates
static int run_extra_forward(sdqn_net_s* h, const StepArgs& a, int wz, int sz, const LaunchPlan* l) {
  StepArgs p = a; p.nz = 1;
  if (wz) { p.theta[0] = a.theta[1]; p.wh[0] = a.wh[1]; p.wht[0] = a.wht[1]; p.w1p[0] = a.w1p[1]; }
  if (sz) p.src = a.from_ring ? a.src + (size_t)soff(a.post_off, 1) * FRAME : a.src + (size_t)a.B * STATE;
  HeadArgs hp = head_args(h, HEAD_PREDICT); hp.q = h->q + (size_t)2 * a.B * h->A;
  return forward(h, p, hp, l);
}
// Everything a train step decides, once, from the handle alone: no HIP call, no side effect (api_internal.h: StepPlan)
StepPlan step_plan(const sdqn_net_s* h) {
  StepPlan p;
  p.structure = step_structure(h); p.update = update_form_of(h, p.structure);
  p.fuse_rms = plan_fuse_rms(h, p.update); p.side_fc4 = p.structure == STEP_DP_OVERLAP;
  // the head of the one option that is on (option_table.h lets no two of them through); Double DQN's only with a target net (ddqn_active)
  const int head = option_head(active_options(h));
  p.head_train = head == HEAD_DOUBLE && !ddqn_active(h) ? 0 : head;
  // --munchausen / --advantage_learning: the target net on the prestates in front of the step | --double_dqn: its own forward with
  // --batch_norm, else a third slot of the step's (comment at ddqn_active)
  p.extra_fwd = (p.head_train == HEAD_MUNCHAUSEN || p.head_train == HEAD_ADVANTAGE) ? 1 : (p.head_train == HEAD_DOUBLE && h->bn) ? 2 : 0;
  p.nz = (p.head_train == HEAD_DOUBLE && !h->bn) ? 3 : 2;
  LaunchPlan* l = p.launch;
  plan_forward(h, l);
  // The backward.  conv1's weight gradient on packed-bf16 MFMA (sdqn_kernels_r3.hip) in every launch structure (same bits); B < 128 only: in the
  // throughput regime the on-the-fly split of delta1 makes it VALU-bound (3 580 vs 4 063 steps/s at B = 256; option value 2 forces it)
  const bool f32 = h->cfg.datatype == 0 && !h->bn;
  const int c1w = ((h->conv1w_bf16 == 2 || (h->conv1w_bf16 == 1 && h->B < 128)) && f32 && h->nw_override[K_CONV1_WGRAD] == 0) ? LV_CONV1_WGRAD_BF16 : 0;
  // round 4, B >= 128 float32: the backward launches on the XCD-contiguous block / tile maps (the blocks that share a weight panel share an L2):
  // fc4_dgrad 15.1 -> 14.4 us, bwd2 38.9 -> 37.5, bwd3 39.7 -> 39.2; 4 802 -> 4 867 steps/s at B = 256 (placement only: same bits)
  const bool bt_xcd = h->B >= 128 && f32 && h->bt_on && h->bt_xcd;
  if (bt_xcd) l[K_FC4_DGRAD].xcd_bits = 1;
  switch (p.structure) {
  case STEP_DP_OVERLAP:
    // data parallel, overlapped: ALL of fc4_wgrad rides the first backward launch, so the 6.4 MB fc4 gradient is
    // complete two launches before the step ends; its all-reduce and its optimizer update run on g_comm
    // (second communicator) under K_BWD2, K_BWD1, the conv/fc5 all-reduce + update and the next step's conv1..3.
    l[K_BWD2].f4w_count = l[K_BWD1].f4w_count = 0; l[K_BWD1].variant = c1w;
    break;
  case STEP_FUSED:
    // fc4 wgrad (1568 tiles at B <= 32) may be spread over the three backward launches as background traffic (options f4_share3 / f4_share2;
    // built-in: all of it in bwd3); for B > 32 (K-split workgroups) it all rides in the first one
    if (h->B <= 32) {
      const int s3 = h->f4_share[0] * F4_TILES / 100, s2 = h->f4_share[1] * F4_TILES / 100;
      l[K_BWD3].f4w_count = s3;
      l[K_BWD2].f4w_first = s3; l[K_BWD2].f4w_count = s2;
      l[K_BWD1].f4w_first = s3 + s2; l[K_BWD1].f4w_count = F4_TILES - s3 - s2;
    } else l[K_BWD2].f4w_count = l[K_BWD1].f4w_count = 0;
    if (bt_xcd) l[K_BWD3].xcd_bits = l[K_BWD2].xcd_bits = 7;
    // B <= 32: the fc4_wgrad tiles of bwd3 (third problem of the launch) on the XCD-contiguous map — a tile row's 16 tiles share a3's columns
    // (10.29 -> 10.10 us, 15 315 -> 15 345 steps/s in alternating rate loops; the conv3 problems are slower on it: round-robin as before)
    if (h->B <= 32 && f32 && h->bt_xcd) l[K_BWD3].xcd_bits |= 4;
    // conv1_wgrad on the XCD-contiguous tile map: the 8 m-tiles of a K-slab read the same frames, so a slab's tiles belong on ONE XCD's L2
    // (L2 <-> fabric traffic of the launch 15.8 -> 4.0 MB = 1.4x algorithmic, rocprofv3 PMC; step rate -0.1 %: the re-reads were MALL hits)
    l[K_BWD1].xcd_bits = 2;
    l[K_BWD1].variant = l[K_BWD1].f4w_count == 0 ? c1w : 0;
    break;
  case STEP_H16_BT:
    // round 4, float16 at B >= 128: the two dgrads run on the half block-tile routine as launches of their own (15.6 / 18.1 -> ~7 / 8 us:
    // operands leave L2 once per workgroup), and every weight gradient that does not need delta1 shares ONE launch behind them (it packs
    // better than the two fused backward launches did) — five launches where there were four, 19 us less (tools/exp/README.md)
    if (h->bt_xcd) l[K_WGRADS].xcd_bits = 7;          // the weight-gradient launch on XCD-contiguous block maps (the blocks of a K slab share their operand rows): 20.1 -> 17.0 us at B = 256
    l[K_BWD1].f4w_count = 0; l[K_BWD1].xcd_bits = 2;
    // round 6: conv1's weight gradient (c1w_h_kernel's K-slab workgroups) as a fourth block range of the weight-gradient launch — delta1 is
    // complete by then — where that kernel applies (packed-fp16 weight gradients, slabs of whole 80-position chunks) and nothing asks for
    // another form (bt:18 / bt:24 = 0; option c1w_in_wgrads: 0 = off, 1 = its workgroups last (built-in), 2 = first)
    if (h->c1w_in_wgrads && h->h16_wgrad_mfma && (h->tps1 * 32) % 80 == 0 && h->bt[K_BWD1] == 0 && h->bt[K_WGRADS] == 0 && h->nw_override[K_CONV1_WGRAD] == 0)
      l[K_WGRADS].variant = l[K_BWD1].variant = LV_C1W_IN_WGRADS | (h->c1w_in_wgrads == 2 ? LV_C1W_FIRST : 0);
    break;
  case STEP_UNFUSED: l[K_CONV1_WGRAD].variant = c1w; break;
  }
  // The optimizer tail.  single: one launch.  clip: what the serial data-parallel form does without its all-reduce (one rank).  grad_only: that
  // form stopped after its local sums (nothing applied, nothing clipped).  dp_overlap: the conv + fc5 gradients (0.3 MB) only — fc4's part
  // is already on its way on g_comm
  TailPlan& t = p.tail;
  t.reduce_first = p.update != UPD_SINGLE;
  if (p.update == UPD_DP_OVERLAP) t.exchange = XCH_GROUPED;
  // fp16 mode: half payload, fp32 accumulation in the optimizer, overflow -> the step is skipped on all ranks
  else if (p.update == UPD_DP_SERIAL) t.exchange = (h->cfg.datatype == 1 && h->dp_half && h->gh) ? XCH_HALF : XCH_F32;
  t.ovf = t.exchange == XCH_HALF;
  t.clip = clip_on(h) && (p.update == UPD_CLIP || p.update == UPD_DP_SERIAL);      // the all-reduced gradient, every rank alike
  t.mask = h->opt.dueling && p.update != UPD_GRAD_ONLY;                                // likewise, in every applying form (fc5 is never applied on the side stream)
  t.noisy = h->noisy && p.update == UPD_CLIP;                                      // --noisy_nets (single GPU only: sdqn_net_set_noisy): the sigma launch; run_train composes around the step
  t.apply_mode = p.update == UPD_SINGLE ? 0 : p.update == UPD_GRAD_ONLY ? -1 : 2;
  t.divisor = (double)h->B * (double)(h->comm ? h->nranks : 1);
  t.skip_fc4 = p.side_fc4 ? 1 : p.fuse_rms;
  return p;
}
// the overlapped form's side stream: fc4's gradient is complete behind bwd3 — its all-reduce and its update run on g_comm (second communicator)
static int side_fc4_update(sdqn_net_s* h, const StepArgs& a, const TailPlan& t) {
  HIPCHK(hipEventRecord(h->ev_g4, g_stream));
  HIPCHK(hipStreamWaitEvent(g_comm, h->ev_g4, 0));
  LAUNCH_ON(g_comm, K_ALLREDUCE, dp_allreduce(h, h->g + OFF4, (size_t)NW4, /*ncclFloat32*/ 7, h->comm2, g_comm));
  UpdateArgs u4 = make_update_args(h, a);
  u4.mode = 2; u4.only_fc4 = 1; u4.skip_fc4 = 0; u4.bsz = (float)t.divisor;
  LAUNCH_ON(g_comm, K_UPDATE, launch_update(u4, g_comm));
  HIPCHK(hipEventRecord(h->ev_w4, g_comm));
  h->w4_pending = true;
  return SDQN_OK;
}
// [local sums] -> [exchange] -> [mask] -> [clip] -> apply -> [BatchNorm parameters] (api_internal.h: TailPlan); `next` rides in the last update launch
int run_update_tail(sdqn_net_s* h, UpdateArgs u, const TailPlan& t, const PrepArgs* next) {
  u.skip_fc4 = t.skip_fc4; u.next.B = 0;
  if (t.reduce_first) {
    u.mode = 1; u.bsz = (float)h->B;
    if (t.apply_mode < 0 && next) u.next = *next;
    LAUNCH(K_UPDATE, launch_update(u, g_stream));
  }
  if (t.apply_mode < 0) return SDQN_OK;
  switch (t.exchange) {
  case XCH_GROUPED:
    if (g_rccl.GroupStart && g_rccl.GroupEnd) NCCLCHK(g_rccl.GroupStart());
    LAUNCH(K_ALLREDUCE, dp_allreduce(h, h->g, (size_t)OFF4, 7, h->comm, g_stream));
    LAUNCH(K_ALLREDUCE, dp_allreduce(h, h->g + OFF5, (size_t)(h->NP - OFF5), 7, h->comm, g_stream));
    if (g_rccl.GroupStart && g_rccl.GroupEnd) NCCLCHK(g_rccl.GroupEnd());
    break;
  case XCH_HALF:
    LAUNCH(K_UPDATE, launch_grad_to_half(h->g, h->gh, h->NP, h->ovf_flag, g_stream));
    LAUNCH(K_ALLREDUCE, dp_allreduce(h, h->gh, (size_t)h->NP, /*ncclFloat16*/ 6, h->comm, g_stream));
    LAUNCH(K_UPDATE, launch_grad_from_half(h->gh, h->g, h->NP, h->ovf_flag, g_stream));
    break;
  case XCH_F32: LAUNCH(K_ALLREDUCE, dp_allreduce(h, h->g, (size_t)h->NP, /*ncclFloat32*/ 7, h->comm, g_stream)); break;
  case XCH_NONE: break;
  }
  if (t.ovf) { u.ovf_flag = h->ovf_flag; u.ovf_count = h->ovf_count; u.ovf_dynamic = h->dp_half_scale_log2 < 0 ? 1 : 0; }
  if (t.mask) LAUNCH(K_UPDATE, launch_dueling_mask(h->g + OFF5, false, h->A, NFC, g_stream));      // --dueling: the clip measures, the optimizer reads the masked g
  if (t.noisy) {                           // --noisy_nets: sigma moves by the same rule, divisor and learning rate as mu, on g * e of this step's xi
    NoisyTailArgs nt; memset(&nt, 0, sizeof nt);
    nt.g = h->g; nt.sigma = h->nz_sigma[0]; nt.state = h->nz_state; nt.state2 = h->nz_state2; nt.eps = h->nz_eps;
    nt.gsig = h->keep_grads ? h->nz_gsig : nullptr; nt.n = h->NP - OFF4;
    nt.u = u; nt.u.bsz = (float)t.divisor; nt.u.next.B = 0;
    LAUNCH(K_UPDATE, launch_noisy_tail(nt, g_stream));
  }
  if (t.clip) { int rc = clip_gradient(h, t.divisor); if (rc) return rc; }
  u.mode = t.apply_mode; u.bsz = (float)t.divisor;
  if (next) u.next = *next;
  LAUNCH(K_UPDATE, launch_update(u, g_stream));
  if (h->bn) LAUNCH(K_BN, launch_bn_update(u, g_stream));
  return SDQN_OK;
}
// The backward's launches per structure, in order.  Critical path: fc4_dgrad -> conv3_dgrad -> conv2_dgrad -> conv1_wgrad; the other weight
// gradients only need the delta of their layer and share a launch with the dgrad that is computed from the same delta.  BWD_BN + l
// (--batch_norm only): the delta arriving at layer l (masked by its Rectlin) first goes back through BatchNorm l, in place.  Unfused:
// fc4_wgrad may update W4 in place (fused RMSProp), so it must not start before fc4_dgrad has read W4 — same stream, after it; fc4_wgrad
// needs d4 and a3, conv3_wgrad d3p and a2, conv2_wgrad d2p and a1.
enum { BWD_END = -1, BWD_SIDE_FC4 = -2, BWD_BN = -8 };
static const int BWD_SEQ[4][12] = {
  /* STEP_FUSED      */ {BWD_BN + 3, K_FC4_DGRAD, BWD_BN + 2, K_BWD3, BWD_SIDE_FC4, BWD_BN + 1, K_BWD2, BWD_BN + 0, K_BWD1, BWD_END},
  /* STEP_H16_BT     */ {K_FC4_DGRAD, K_CONV3_DGRAD, K_CONV2_DGRAD, K_WGRADS, K_BWD1, BWD_END},
  /* STEP_DP_OVERLAP */ {BWD_BN + 3, K_FC4_DGRAD, BWD_BN + 2, K_BWD3, BWD_SIDE_FC4, BWD_BN + 1, K_BWD2, BWD_BN + 0, K_BWD1, BWD_END},
  /* STEP_UNFUSED    */ {BWD_BN + 3, K_FC4_DGRAD, BWD_BN + 2, K_FC4_WGRAD, K_CONV3_WGRAD, K_CONV3_DGRAD, BWD_BN + 1, K_CONV2_WGRAD, K_CONV2_DGRAD, BWD_BN + 0, K_CONV1_WGRAD, BWD_END}};
// --noisy_nets: one launch writes the effective buffers of net slots 0 .. nets - 1 under xi_step
int noisy_compose(sdqn_net_s* h, int64_t step, int nets) {
  NoisyArgs n; memset(&n, 0, sizeof n);
  n.mu[0] = h->theta; n.mu[1] = h->theta_t; n.sigma[0] = h->nz_sigma[0]; n.sigma[1] = h->nz_sigma[1]; n.eff[0] = h->nz_eff[0]; n.eff[1] = h->nz_eff[1];
  n.eps = h->nz_eps; n.seed = h->nz_seed; n.step = (uint64_t)step; n.NP = h->NP; n.A = h->A;
  n.nets = (nets > 1 && h->theta_t != h->theta) ? 2 : 1;
  LAUNCH(K_UPDATE, launch_noisy_compose(n, g_stream));
  return SDQN_OK;
}
int noisy_fresh(sdqn_net_s* h) {
  if (!h->noisy || !h->nz_stale) return SDQN_OK;
  { int rc = join_comm(h); if (rc) return rc; }
  h->nz_stale = false;
  return noisy_compose(h, h->nz_step, 2);
}
int run_train(sdqn_net_s* h, const StepArgs& a0, const HeadArgs& hd0, const PrepArgs* next) {
  const StepPlan plan = step_plan(h);
  // --noisy_nets: step t = nz_step + 1 draws xi_t (online) and xi'_t (target); both forwards, the Double DQN slot and the backward
  // read the effective buffers, the optimizer tail moves mu (theta) and sigma, and the online net's fc slices are composed again from the
  // updated parameters under the same xi_t: what the acting paths read until the next step
  StepArgs a = a0;
  if (plan.tail.noisy) {
    int rcn = noisy_compose(h, h->nz_step + 1, 2); if (rcn) return rcn;
    h->nz_stale = false;
    a.theta[0] = h->nz_eff[0]; a.theta[1] = h->nz_eff[1];      // (without a target net the two alias, as theta and theta_t do)
  }
  HeadArgs hd = hd0;
  if (plan.head_train) hd.train = plan.head_train;
  if (plan.head_train == HEAD_MUNCHAUSEN) { hd.mu_alpha = h->opt.mu_alpha; hd.mu_tau = h->opt.mu_tau; hd.mu_clip = h->opt.mu_clip; }
  if (plan.head_train == HEAD_ADVANTAGE) { hd.al_alpha = h->opt.al_alpha; hd.al_persistent = h->opt.al_persistent ? 1 : 0; }
  if (plan.head_train == HEAD_CQL) hd.cql_alpha = h->opt.cql_alpha;
  if (plan.extra_fwd) { int rc0 = run_extra_forward(h, a, plan.extra_fwd == 1, plan.extra_fwd == 2, plan.launch); if (rc0) return rc0; }
  StepArgs af = a; af.nz = plan.nz;        // the forward's arguments (the backward keeps a: its launches know two slots only)
  int rc = forward(h, af, hd, plan.launch); if (rc) return rc;
  for (const int* s = BWD_SEQ[plan.structure]; *s != BWD_END; ++s) {
    if (*s >= 0) PLANNED_LAUNCH(*s, a, plan.launch);
    else if (*s == BWD_SIDE_FC4) { if (plan.side_fc4) { rc = side_fc4_update(h, a, plan.tail); if (rc) return rc; } }
    else if (h->bn) LAUNCH(K_BN, launch_bn_backward(bn_args(h, a, *s - BWD_BN, 1), g_stream));
  }
  rc = run_update_tail(h, make_update_args(h, a), plan.tail, next); if (rc) return rc;
  // (the whole online buffer: the apply launch has moved the conv slices too, and the acting forward reads them from here)
  if (plan.tail.noisy) { h->nz_step += 1; rc = noisy_compose(h, h->nz_step, 1); if (rc) return rc; }
  h->train_iterations += 1;                                                   // deepqnetwork.py:168
  h->spec_pending = false;                 // the online parameters move: a forward enqueued before this step no longer is "predict now"
  h->redo_acts_live = true;
  if (plan.update == UPD_GRAD_ONLY) return SDQN_OK;
  return step_applied(h, true);            // the regulariser, the blend of --target_tau, the interval events
}
// small read-backs: `bytes` of device memory into the pinned scratch h->h_f, waited for
static int fetch_small(sdqn_net_s* h, const void* src, size_t bytes) {
  HIPCHK(hipMemcpyAsync(h->h_f, src, bytes, hipMemcpyDeviceToHost, g_stream));
  HIPCHK(hipStreamSynchronize(g_stream));
  return SDQN_OK;
}
// The last step's cost / the mean over the n_steps steps since the cost sum was cleared.  Both wait for the stream, so both end with what
// every synchronising net call reports: the prioritized memories' device flags (action out of range, non-finite TD error).
int read_cost(sdqn_net_s* h, float* cost_out) {
  if (h->gen) { double c; GENCHK(h->gen->read_cost(&c)); *cost_out = (float)c; }
  else { int rc = fetch_small(h, h->cost_out, 4); if (rc) return rc; *cost_out = h->h_f[0]; }
  return per_check_all();
}
int read_mean_cost(sdqn_net_s* h, int n_steps, float* mean_cost) {
  double sum;
  if (h->gen) GENCHK(h->gen->read_cost_sum(&sum));
  else { int rc = fetch_small(h, h->cost_accum, 8); if (rc) return rc; memcpy(&sum, h->h_f, 8); }
  *mean_cost = n_steps ? (float)(sum / n_steps) : 0.0f;
  return per_check_all();
}
// The predict forward (what sdqn_net_predict launches) on states already on the device, tuned path: the net's full batch, or B states.
int predict_forward_tuned(sdqn_net_s* h, const uint8_t* states, const HeadArgs& hd, int B, bool noisy) {
  StepArgs a = step_args(h); a.nz = 1; a.from_ring = 0; a.src = states;
  if (noisy && h->noisy) a.theta[0] = h->nz_eff[0];       // --noisy_nets: the collecting-mode forward (the caller has run noisy_fresh)
  if (B) a.B = B;
  return run_forward(h, a, hd);
}
// ... on either path: `rows` states are wanted (the tuned forward runs its full batch, the generic one these rows); *q: where the Q-values
// [rows][A] will lie, *q_f64: as doubles (a float64 network)
int predict_forward(sdqn_net_s* h, const uint8_t* states, int rows, const void** q, int* q_f64, bool noisy) {
  if (h->gen) { GENCHK(h->gen->forward_dev(states, rows)); *q = h->gen->q_dev(); *q_f64 = h->gen->is_f64() ? 1 : 0; return SDQN_OK; }
  *q = h->q; *q_f64 = 0;
  return predict_forward_tuned(h, states, head_args(h, HEAD_PREDICT), 0, noisy);
}

extern "C" int sdqn_net_predict_f64(sdqn_net_t h, const uint8_t* states, double* q_out) {
  ARGCHK(h && states && q_out, "NULL argument");
  if (h->gen) { GENCHK(h->gen->predict_host(states, h->B, q_out, true)); return SDQN_OK; }
  std::vector<float> tmp((size_t)h->B * h->A);
  int rc = sdqn_net_predict(h, states, tmp.data()); if (rc) return rc;
  for (size_t i = 0; i < tmp.size(); ++i) q_out[i] = (double)tmp[i];
  return SDQN_OK;
}
static int predict_host(sdqn_net_s* h, const uint8_t* states, float* q_out, bool noisy) {
  HIPCHK(hipMemcpyAsync(h->st_states, states, (size_t)h->B * STATE, hipMemcpyHostToDevice, g_stream));
  int rc = predict_forward_tuned(h, h->st_states, head_args(h, HEAD_PREDICT), 0, noisy); if (rc) return rc;
  rc = fetch_small(h, h->q, (size_t)h->B * h->A * 4); if (rc) return rc;
  memcpy(q_out, h->h_f, (size_t)h->B * h->A * 4);                             // (B, A): deepqnetwork.py:186 qvalues.T
  return SDQN_OK;
}
extern "C" int sdqn_net_predict(sdqn_net_t h, const uint8_t* states, float* q_out) {
  ARGCHK(h && states && q_out, "NULL argument");
  if (h->gen) { GENCHK(h->gen->predict_host(states, h->B, q_out, false)); return SDQN_OK; }
  return predict_host(h, states, q_out, false);                               // (--noisy_nets: mu alone, a score is deterministic)
}
// --noisy_nets: the collecting-mode Q-values — the online net's current parameters under the last train step's noise (xi_0 before the first)
extern "C" int sdqn_net_predict_noisy(sdqn_net_t h, const uint8_t* states, float* q_out) {
  ARGCHK(h && states && q_out, "NULL argument");
  ARGCHK(h->noisy, "the network is not a noisy net (sdqn_net_set_noisy)");
  { int rc = noisy_fresh(h); if (rc) return rc; }
  return predict_host(h, states, q_out, true);
}

// the one-launch forward's 8 stripe partials [8][ACT_Q_STRIDE] -> Q-values, added in stripe order; false if a stripe never arrived
bool act_sum_partials(const float* part, int A, float* q_out) {
  for (int k = 0; k < A; ++k) {
    float qv = 0.0f;
    for (int sp = 0; sp < 8; ++sp) {
      uint32_t w; memcpy(&w, part + sp * ACT_Q_STRIDE + k, 4);
      if (w == 0xFFFFFFFFu) return false;
      qv = sp ? qv + part[sp * ACT_Q_STRIDE + k] : part[sp * ACT_Q_STRIDE + k];
    }
    q_out[k] = qv;
  }
  return true;
}
extern "C" int sdqn_net_predict_one(sdqn_net_t h, const uint8_t* state, float* q_out) {
  ARGCHK(h && state && q_out, "NULL argument");
  if (h->gen) { GENCHK(h->gen->predict_host(state, 1, q_out, false)); return SDQN_OK; }
  HIPCHK(hipMemcpyAsync(h->st_states, state, (size_t)STATE, hipMemcpyHostToDevice, g_stream));
  if (noisy_acting(h)) { int rcn = noisy_fresh(h); if (rcn) return rcn; }      // --noisy_nets, train phase: the effective weights
  if (h->act_on && !h->prof_on) {            // the one-launch forward (sdqn_act.hip): the same kernel predict_state runs, the same numbers
    { int rcj = join_comm(h); if (rcj) return rcj; }
    ActArgs aa; memset(&aa, 0, sizeof aa);
    aa.state = h->st_states; aa.theta = noisy_acting(h) ? h->nz_eff[0] : h->theta; aa.scratch = h->act_scratch; aa.ctl = h->act_ctl;
    aa.q = h->act_q; aa.A = h->A; aa.seq = h->act_seq++;
    HIPCHK(hipMemsetAsync(h->act_q, 0xFF, (size_t)Q_SLOT_FLOATS * 4, g_stream));          // (an abandoned launch leaves NaNs, checked below)
    LAUNCH(K_ACT, launch_act(aa, false, g_stream));
    { int rcf = fetch_small(h, h->act_q, (size_t)Q_SLOT_FLOATS * 4); if (rcf) return rcf; }
    if (act_sum_partials(h->h_f, h->A, q_out)) return SDQN_OK;
    h->act_on = false; h->act_fallbacks += 1;
    fprintf(stderr, "simple_dqn_amd: the one-launch acting forward did not complete; using the five-launch forward from now on\n");
  }
  int rc = predict_forward_tuned(h, h->st_states, head_args(h, HEAD_PREDICT), 1, noisy_acting(h)); if (rc) return rc;   // same buffers, batch of one
  rc = fetch_small(h, h->q, (size_t)h->A * 4); if (rc) return rc;
  memcpy(q_out, h->h_f, (size_t)h->A * 4);
  return SDQN_OK;
}

// returns: rewards are the n-step returns R as float64 bits, terminals the done flags (sdqn_net_train_host_returns)
static int train_host_tuple(sdqn_net_t h, const uint8_t* pre, const uint8_t* actions, const int64_t* rewards,
                            const uint8_t* post, const uint8_t* terminals, float* cost_out, bool returns) {
  // the one-shot "minibatch buffers are clean" declarations are consumed FIRST: an argument error below must not leave one armed for a
  // later call whose buffers were edited in place
  sdqn_replay_s* owner = nullptr;                               // (handles are created / destroyed / used from ONE host thread: sdqn.h)
  bool reuse = false;                                           // train on the device copy the last gather left (no state upload)
  for (sdqn_replay_s* r : g_replays) {
    if (h && pre && post && pre == r->h_pre && post == r->h_post && r->B == h->B) { owner = r; reuse = r->mb_clean_declared && (r->mb_host_gen == r->mb_dev_gen || r->mb_clean_on_device); }
    r->mb_clean_declared = false; r->mb_clean_on_device = false;          // one-shot, whoever it was meant for
  }
  ARGCHK(h && pre && actions && rewards && post && terminals, "NULL argument");
  if (returns) ARGCHK(h->opt.n_step > 1, "sdqn_net_train_host_returns needs option n_step > 1 (network n_step %d)", h->opt.n_step);
  else ARGCHK(h->opt.n_step == 1, "network n_step %d: integer rewards are refused, train with returns (sdqn_net_train_host_returns)", h->opt.n_step);
  for (int i = 0; i < h->B; ++i) ARGCHK(actions[i] < game_actions(h), "action %d out of range at %d", (int)actions[i], i);
  ARGCHK(h->opt.boot_K == 1 || h->opt.boot_P >= 1.0, "%s: bootstrap_mask_probability %g < 1 needs the ring index of every sample — train from the replay memory "
         "(sdqn_net_train_many / sdqn_net_train_replay); the tuple path serves bootstrap_heads %d with probability 1 only",
         returns ? "sdqn_net_train_host_returns" : "sdqn_net_train_host", h->opt.boot_P, h->opt.boot_K);
  const bool ours = owner != nullptr;
  if (ours) { int rcn = nstep_match(h, owner); if (rcn) return rcn; rcn = check_replay_geometry(h, owner); if (rcn) return rcn; }
  ARGCHK(h->opt.boot_K == 1 || !per_owns_minibatch(owner), "bootstrap_heads %d cannot be combined with prioritized_replay", h->opt.boot_K);
  ARGCHK(h->opt.quant_N == 1 || !per_owns_minibatch(owner), "quantiles %d cannot be combined with prioritized_replay", h->opt.quant_N);
  if (h->gen) {
    if (h->opt.boot_K > 1) GENCHK(h->gen->boot_idx(nullptr));
    const bool per = per_owns_minibatch(owner);                 // prioritized memory: weighted step + priority write-back
    if (per) per_gen_arm(h, owner);
    const hipError_t ge = reuse ? h->gen->train_dev_host_meta(owner->d_pre, owner->d_post, actions, rewards, terminals, h->epoch)
                                : h->gen->train_host(pre, actions, rewards, post, terminals, h->epoch);
    if (per) { int rcp = per_gen_finish(h, owner); if (ge == hipSuccess && rcp) return rcp; }
    GENCHK(ge);
    { int rcb = gen_step_done(h); if (rcb) return rcb; }
    return cost_out ? read_cost(h, cost_out) : SDQN_OK;
  }
  const size_t sb = (size_t)h->B * STATE, small = (size_t)h->B * 10;
  // No stream synchronisation (round 1 paid a full PCIe + sync bubble per step here): the caller's arrays are free to
  // change after return because they are either copied into a pinned double buffer of the library first (pageable
  // arrays), or ARE the pinned minibatch buffers of one of this library's ReplayMemory handles — what getMinibatch() returns
  // for prestates / poststates —, whose next overwrite by the library (gather + D2H) is ordered behind this H2D on the library
  // stream; a HOST write to them could still race the DMA, so in that case the call returns only after the upload has completed
  // (event wait AFTER every launch of the step is enqueued: the GPU never idles for it, the host waits ~30 us it would otherwise
  // spend ahead of the stream).  Either way: once train() has returned the caller's five arrays are free, like the reference's.
  // Round 3: when those pinned buffers still hold exactly what the last gather put on the device and the caller says it has not
  // written into them (`reuse`), nothing is uploaded at all — the step reads the device copy in place.
  // Round 5: actions / rewards / terminals too.  The gather that filled the device minibatch also left ring[idx] of the three small
  // arrays next to it (d_rew | d_act | d_term) and the library kept what those values were (mb_snap, taken from the host master at
  // enqueue time); when the caller passes back exactly those values — what getMinibatch() returned, untouched — the step reads the
  // device copy and the call uploads nothing at all (no 10 B x batch H2D, no staging slot, no event: ~6 us of a ~75 us iteration).
  // Any difference (a caller that clips rewards, edits an action, ...) takes the upload below, as before.
  const size_t nb = (size_t)h->B;
  const bool small_dev = reuse && owner->mb_snap && owner->mb_snap_gen == owner->mb_dev_gen &&
                         !memcmp(owner->mb_snap, rewards, nb * 8) && !memcmp(owner->mb_snap + nb * 8, actions, nb) &&
                         !memcmp(owner->mb_snap + nb * 9, terminals, nb);
  if (!small_dev) {
    const int sl = h->stage_next; h->stage_next ^= 1;
    if (!h->h_stage[sl]) {
      HIPCHK(hipHostMalloc((void**)&h->h_stage[sl], 2 * sb + small, hipHostMallocDefault));
      HIPCHK(hipEventCreateWithFlags(&h->stage_ev[sl], hipEventDisableTiming));
    }
    if (h->stage_busy[sl]) { HIPCHK(hipEventSynchronize(h->stage_ev[sl])); h->stage_busy[sl] = false; }
    uint8_t* st = h->h_stage[sl];
    if (!ours) { memcpy(st, pre, sb); memcpy(st + sb, post, sb); }
    uint8_t* sm = st + 2 * sb;                                                  // [rewards 8 B | actions B | terminals B], as on the device
    memcpy(sm, rewards, nb * 8); memcpy(sm + nb * 8, actions, nb); memcpy(sm + nb * 9, terminals, nb);
    // every copy is a packet of its own in the stream: 2 instead of 5 (1 with `reuse`, 0 with `small_dev`)
    if (!reuse) {
      HIPCHK(hipMemcpyAsync(h->st_states, ours ? pre : st, 2 * sb, hipMemcpyHostToDevice, g_stream));     // (a ReplayMemory's pre | post are one block too)
      if (ours) { HIPCHK(hipEventRecord(owner->mb_upload_ev, g_stream)); }   // waited for before this call returns
    }
    HIPCHK(hipMemcpyAsync(h->st_rew, sm, small, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipEventRecord(h->stage_ev[sl], g_stream)); h->stage_busy[sl] = true;
  }
  h->tuple_calls += 1; h->tuple_states_skipped += reuse ? 1 : 0; h->tuple_small_skipped += small_dev ? 1 : 0;
  StepArgs a = step_args(h); a.from_ring = 0; a.src = reuse ? owner->d_pre : h->st_states;
  HeadArgs hd = head_args(h, HEAD_TRAIN);
  if (small_dev) { hd.st_actions = owner->d_act; hd.st_rewards = owner->d_rew; hd.st_terminals = owner->d_term; }
  // prioritized memory, minibatch gathered from its last sample: weighted step + priority write-back (a foreign tuple: the standard step)
  int rc = per_owns_minibatch(owner) ? per_train_host_step(h, owner, a, hd) : run_train(h, a, hd); if (rc) return rc;
  if (ours && !reuse) { HIPCHK(hipEventSynchronize(owner->mb_upload_ev)); }
  return cost_out ? read_cost(h, cost_out) : SDQN_OK;
}

extern "C" int sdqn_net_train_host(sdqn_net_t h, const uint8_t* pre, const uint8_t* actions, const int64_t* rewards,
                                   const uint8_t* post, const uint8_t* terminals, float* cost_out) {
  return train_host_tuple(h, pre, actions, rewards, post, terminals, cost_out, false);
}
extern "C" int sdqn_net_train_host_returns(sdqn_net_t h, const uint8_t* pre, const uint8_t* actions, const double* returns,
                                           const uint8_t* post, const uint8_t* dones, float* cost_out) {
  return train_host_tuple(h, pre, actions, reinterpret_cast<const int64_t*>(returns), post, dones, cost_out, true);
}

extern "C" int sdqn_net_tuple_counters(sdqn_net_t h, int64_t* calls, int64_t* states_in_place, int64_t* nothing_uploaded) {
  ARGCHK(h, "NULL handle");
  if (calls) *calls = h->tuple_calls; if (states_in_place) *states_in_place = h->tuple_states_skipped;
  if (nothing_uploaded) *nothing_uploaded = h->tuple_small_skipped;
  return SDQN_OK;
}

PrepArgs prep_args(sdqn_net_s* h, sdqn_replay_s* r, const int64_t* pinned_idx) {
  PrepArgs p; memset(&p, 0, sizeof p);
  p.idx_pinned = pinned_idx; p.meta = r->d_meta; p.idx = h->d_idx; p.actions = h->st_act;
  p.rewards = h->st_rew; p.terminals = h->st_term; p.B = h->B;
  p.ns = r->ns;                                  // (nstep_match: the net's n)
  if (h->B <= 32 && h->prep_inline) {            // the slot's host copy (pinned_idx is its device alias)
    memcpy(p.idx_in, r->h_idx + (pinned_idx - r->d_idx_view), (size_t)h->B * sizeof(int64_t));
    p.idx_in_valid = 1;
  }
  return p;
}
// ring paths take (a, r, t) from the ring: an action the network has no output for would index past the Q row in the
// head kernel (which clamps) and train garbage silently; the tuple API checks the same thing (sdqn_net_train_host)
int check_ring_actions(sdqn_net_s* h, sdqn_replay_s* r, const int64_t* idx) {
  for (int i = 0; i < r->B; ++i)
    ARGCHK(idx[i] >= 0 && idx[i] < r->size && r->actions[idx[i]] < game_actions(h),
           "ring slot %lld holds action %d but the network has %d actions", (long long)idx[i], (int)r->actions[idx[i]], game_actions(h));
  return SDQN_OK;
}
// A step that reads its states from the ring, its indexes in h->d_idx: the arguments, and the step.  host_idx: the host copy of those
// indexes (conv1's tiles take them from the kernel arguments: launch_tuned), nullptr when they were sampled on the device (conv1 reads HBM)
StepArgs ring_step_args(sdqn_net_s* h, const sdqn_replay_s* r) {
  StepArgs a = step_args(h); a.from_ring = 1; a.src = r->d_ring; a.idx = h->d_idx;
  return a;
}
// --random_shift: the step's 2 B shifted states into r's device minibatch, from the ring at the indexes in didx
int shift_minibatch(sdqn_net_s* h, sdqn_replay_s* r, const int64_t* didx) {
  ARGCHK(h->shift_P < r->H && h->shift_P < r->W, "random_shift %d needs screens larger than the shift (replay memory %dx%d)", h->shift_P, r->H, r->W);
  ShiftArgs s; memset(&s, 0, sizeof s);
  s.ring = r->d_ring; s.idx = didx; s.pre = r->d_pre; s.post = r->d_post; s.shifts = h->shift_out; s.size = r->size;
  s.seed = h->shift_seed; s.step = (uint64_t)h->shift_step;
  s.B = r->B; s.hist = r->hist; s.H = r->H; s.W = r->W; s.P = h->shift_P; s.post_off = r->ns.n > 1 ? r->ns.n : 1;      // (problems.h soff)
  r->mb_dev_gen++;                                  // (the launch overwrites the device minibatch: gather_args)
  LAUNCH(K_SHIFT, launch_shift_gather(s, g_stream));
  h->shift_step += 1;
  return SDQN_OK;
}
int run_ring_step(sdqn_net_s* h, sdqn_replay_s* r, const int64_t* host_idx, const HeadArgs& hd, const PrepArgs* next) {
  if (h->shift_P > 0) {            // the step that reads a device minibatch in place (sdqn_net_train_host with states_in_place), on the shifted one;
    int rcs = shift_minibatch(h, r, h->d_idx); if (rcs) return rcs;      // (a, r, t) stay where prep left them
    StepArgs a = step_args(h); a.from_ring = 0; a.src = r->d_pre; a.idx = h->d_idx;      // (idx: the bootstrap head's masks are keyed by ring index)
    return run_train(h, a, hd, next);
  }
  h->host_idx_cur = host_idx;
  const int rc = run_train(h, ring_step_args(h, r), hd, next);
  h->host_idx_cur = nullptr;
  return rc;
}
// do_prep: launch the standalone prep for THIS step; next_pinned: fold the NEXT step's prep into the update
static int train_replay_slot(sdqn_net_s* h, sdqn_replay_s* r, const int64_t* pinned_idx, bool do_prep = true,
                             const int64_t* next_pinned = nullptr, double* zero8 = nullptr) {
  if (do_prep) { PrepArgs p = prep_args(h, r, pinned_idx); LAUNCH(K_PREP, launch_prep(p, g_stream, zero8)); }
  const int64_t* host_idx = r->h_idx + (pinned_idx - r->d_idx_view);      // the slot's HOST address (pinned_idx is its device alias)
  PrepArgs np; if (next_pinned) np = prep_args(h, r, next_pinned);
  return run_ring_step(h, r, host_idx, head_args(h, HEAD_TRAIN), next_pinned ? &np : nullptr);
}
// float64 / other geometries: sample on the host, gather on the device into the replay handle's minibatch buffers, train from there
static int gen_train_replay(sdqn_net_s* h, sdqn_replay_s* r, const int64_t* idx_host) {
  int slot; const int64_t* didx; int rc = check_ring_actions(h, r, idx_host); if (rc) return rc;
  rc = replay_push_idx(r, idx_host, &slot, &didx); if (rc) return rc;
  rc = replay_gather_generic(r, didx); if (rc) return rc;
  if (h->shift_P > 0) { rc = shift_minibatch(h, r, didx); if (rc) return rc; }      // --random_shift: the states again, shifted; (a, r, t) stay
  if (h->opt.boot_K > 1) GENCHK(h->gen->boot_idx(didx));                    // (copied on the stream, in front of the slot's release)
  rc = replay_release_idx_batched(r, slot, false); if (rc) return rc;
  GENCHK(h->gen->train_dev(r->d_pre, r->d_post, r->d_act, r->d_rew, r->d_term, h->epoch));
  return gen_step_done(h);
}
// does this replay memory's geometry fit this network?  (tuned path: 84 x 84 x 4; generic path: the configured state size)
int check_replay_geometry(const sdqn_net_s* h, const sdqn_replay_s* r) {
  const int64_t want = h->gen ? (int64_t)h->gen->state_bytes() : (int64_t)STATE;
  ARGCHK(h->gen ? r->state == want : r->tuned_geom, "replay geometry (%dx%d, history %d: %lld bytes per state) differs from the network's (%lld bytes per state)",
         r->H, r->W, r->hist, (long long)r->state, (long long)want);
  return SDQN_OK;
}
// what the entry points that train from a replay memory ask first: its batch size, n-step settings and geometry are the network's
static int check_replay_fits(const sdqn_net_s* h, const sdqn_replay_s* r) {
  ARGCHK(r->B == h->B, "replay batch_size %d != network batch_size %d", r->B, h->B);
  ARGCHK(h->opt.boot_K == 1 || !r->per, "bootstrap_heads %d cannot be combined with prioritized_replay", h->opt.boot_K);
  ARGCHK(h->opt.quant_N == 1 || !r->per, "quantiles %d cannot be combined with prioritized_replay", h->opt.quant_N);
  const int rc = nstep_match(h, r);
  return rc ? rc : check_replay_geometry(h, r);
}
extern "C" int sdqn_net_train_replay(sdqn_net_t h, sdqn_replay_t r, const int64_t* idx_host, float* cost_out) {
  ARGCHK(h && r && idx_host, "NULL argument");
  int rc = check_replay_fits(h, r); if (rc) return rc;
  if (r->per) return per_train_replay(h, r, idx_host, cost_out);
  if (h->gen) rc = gen_train_replay(h, r, idx_host);
  else {
    int slot; const int64_t* didx; rc = check_ring_actions(h, r, idx_host); if (rc) return rc;
    rc = replay_push_idx(r, idx_host, &slot, &didx); if (rc) return rc;
    rc = train_replay_slot(h, r, didx); if (rc) return rc;
    rc = replay_release_idx_batched(r, slot, false);
  }
  if (rc) return rc;
  return cost_out ? read_cost(h, cost_out) : SDQN_OK;
}
extern "C" int sdqn_net_train_many(sdqn_net_t h, sdqn_replay_t r, uint32_t* mt, int n_steps, float* mean_cost) {
  ARGCHK(h && r && mt && n_steps >= 0, "bad arguments");
  int rc = check_replay_fits(h, r); if (rc) return rc;
  if (h->gen) GENCHK(h->gen->reset_cost_sum());                                     // the cost sum of this call's steps
  else if (n_steps == 0) HIPCHK(hipMemsetAsync(h->cost_accum, 0, 8, g_stream));     // (otherwise the first step's prep launch clears it)
  if (r->per) return per_train_many(h, r, mt, n_steps, mean_cost);
  std::vector<int64_t> idx((size_t)r->B);
  if (h->gen) {
    for (int i = 0; i < n_steps; ++i) {
      rc = replay_sample_uniform(r, mt, idx.data(), nullptr); if (rc) return rc;
      rc = gen_train_replay(h, r, idx.data()); if (rc) return rc;
    }
    rc = replay_flush_pending(r); if (rc) return rc;
    return mean_cost ? read_mean_cost(h, n_steps, mean_cost) : SDQN_OK;
  }
  // sample one step ahead: step i's update launch also performs step i+1's prep (index copy + metadata gather)
  int slot = -1, next_slot = -1; const int64_t *pinned = nullptr, *next_pinned = nullptr;
  auto sample = [&](int* sl, const int64_t** pin) -> int {
    int rc = replay_sample_uniform(r, mt, idx.data(), nullptr); if (rc) return rc;
    rc = check_ring_actions(h, r, idx.data()); if (rc) return rc;
    return replay_push_idx(r, idx.data(), sl, pin);
  };
  if (n_steps > 0) { rc = sample(&slot, &pinned); if (rc) return rc; }
  for (int i = 0; i < n_steps; ++i) {
    next_pinned = nullptr;
    if (i + 1 < n_steps) { rc = sample(&next_slot, &next_pinned); if (rc) return rc; }
    rc = train_replay_slot(h, r, pinned, /*do_prep=*/i == 0, next_pinned, i == 0 ? h->cost_accum : nullptr); if (rc) return rc;
    rc = replay_release_idx_batched(r, slot, false); if (rc) return rc;
    slot = next_slot; pinned = next_pinned;
  }
  return mean_cost ? read_mean_cost(h, n_steps, mean_cost) : SDQN_OK;
}
// ---- train_many without waiting for the cost (agent.py:108-114 + deepqnetwork.py:168-172 when the callback can take the cost later) ----------
// The mean cost of the call's steps is copied into a pinned ring slot by the stream itself; sdqn_net_cost_collect polls the slot (bounded).
// A ticket is valid until COST_RING further deferred calls have been made.
extern "C" int sdqn_net_train_many_deferred(sdqn_net_t h, sdqn_replay_t r, uint32_t* mt, int n_steps, int64_t* ticket) {
  ARGCHK(h && ticket && n_steps >= 1, "bad arguments");
  if (!h->cost_ring) HIPCHK(hipHostMalloc((void**)&h->cost_ring, COST_RING * sizeof(double), hipHostMallocDefault));
  const int slot = (int)(h->cost_ticket % COST_RING);
  if (h->gen) {
    float c = 0.0f; int rc = sdqn_net_train_many(h, r, mt, n_steps, &c); if (rc) return rc;
    h->cost_ring[slot] = (double)c * n_steps;
  } else {
    int rc = sdqn_net_train_many(h, r, mt, n_steps, nullptr); if (rc) return rc;
    uint64_t s1 = ~0ull; memcpy(&h->cost_ring[slot], &s1, 8);                          // sentinel: a NaN no cost sum produces
    HIPCHK(hipMemcpyAsync(&h->cost_ring[slot], h->cost_accum, 8, hipMemcpyDeviceToHost, g_stream));
  }
  h->cost_steps[slot] = n_steps;
  *ticket = h->cost_ticket++;
  return SDQN_OK;
}
extern "C" int sdqn_net_cost_collect(sdqn_net_t h, int64_t ticket, float* mean_cost) {
  ARGCHK(h && mean_cost, "NULL argument");
  ARGCHK(h->cost_ring && ticket >= 0 && ticket < h->cost_ticket && ticket + COST_RING > h->cost_ticket, "stale or unknown cost ticket");
  const int slot = (int)(ticket % COST_RING);
  volatile uint64_t* w = reinterpret_cast<volatile uint64_t*>(&h->cost_ring[slot]);
  const auto t0 = std::chrono::steady_clock::now();
  while (*w == ~0ull) {
    if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) { HIPCHK(hipStreamSynchronize(g_stream)); break; }
  }
  ARGCHK(*w != ~0ull, "the cost of ticket %lld was never delivered", (long long)ticket);
  uint64_t bits = *w; double sum; memcpy(&sum, &bits, 8);
  *mean_cost = (float)(sum / h->cost_steps[slot]);
  return per_check_all();
}
// ---- --random_shift ---------------------------------------------------------------------------------------------------
extern "C" int sdqn_net_set_random_shift(sdqn_net_t h, int P, uint64_t seed) {
  ARGCHK(h, "NULL handle");
  ARGCHK(P >= 0 && P <= SHIFT_MAX_PAD, "random_shift %d out of range [0, %d]", P, SHIFT_MAX_PAD);
  if (P > 0) {
    ARGCHK(!h->bn, "random_shift cannot be combined with batch_norm: the shift would change the batch statistics");
    ARGCHK(P < h->cfg.screen_height && P < h->cfg.screen_width, "random_shift %d needs screens larger than the shift (%dx%d)", P, h->cfg.screen_height, h->cfg.screen_width);
    if (!h->shift_out) { int rc = dalloc(h, (void**)&h->shift_out, (size_t)h->B * 4); if (rc) return rc; }
  }
  h->shift_P = P; h->shift_seed = seed; h->shift_step = 0;
  return SDQN_OK;
}
extern "C" int sdqn_net_get_random_shift(sdqn_net_t h, int* P, int64_t* step_counter) {
  ARGCHK(h, "NULL handle");
  if (P) *P = h->shift_P; if (step_counter) *step_counter = h->shift_step;
  return SDQN_OK;
}
extern "C" int sdqn_random_shift_draw(uint64_t seed, uint64_t step, int64_t n, int s, int P, int* dy, int* dx) {
  ARGCHK(dy && dx, "NULL argument");
  ARGCHK(P >= 0 && P <= SHIFT_MAX_PAD && n >= 0 && (s == 0 || s == 1), "bad arguments (P %d, n %lld, s %d)", P, (long long)n, s);
  shift_draw(seed, step, (uint64_t)n, (uint64_t)s, P, *dy, *dx);
  return SDQN_OK;
}
extern "C" int sdqn_net_last_shifts(sdqn_net_t h, int8_t* out) {
  ARGCHK(h && out, "NULL argument");
  ARGCHK(h->shift_out && h->shift_step > 0, "no train step has run with random_shift > 0 (sdqn_net_set_random_shift)");
  HIPCHK(hipMemcpyAsync(out, h->shift_out, (size_t)h->B * 4, hipMemcpyDeviceToHost, g_stream));
  HIPCHK(hipStreamSynchronize(g_stream));
  return SDQN_OK;
}
extern "C" int sdqn_mt_words(uint64_t* words) { ARGCHK(words, "NULL argument"); *words = mt_words_drawn(); return SDQN_OK; }

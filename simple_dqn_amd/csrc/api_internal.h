// api_internal.h — what the translation units of the host side share (sdqn_api_*.hip): handles, library-wide state, error / launch
// macros, and the prototypes of the functions that cross a file boundary.  Nothing here is part of the C ABI (include/sdqn.h).
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <string.h>
#include <string>
#include <vector>
#include <chrono>
#include <thread>

#include "../../include/sdqn.h"
#include "kernels.h"
#include "generic_net.h"
#include "sampler.h"
#include "sdqn_per.h"
#include "sdqn_clip.h"
#include "noisy.h"
#include "shift.h"
#include "redo.h"
#include "reset.h"
#include "regularize.h"
#include "option_table.h"
#include "train_options.h"

using namespace sdqn;


static constexpr int Q_SLOT_FLOATS = 8 * ACT_Q_STRIDE;   // one slot: [A] Q-values (head kernel) or 8 stripe partials [8][ACT_Q_STRIDE] (one-launch forward)
static constexpr int COST_RING = 64;
static constexpr int Q_SLOTS = 8;       // host-mapped Q-value slots of the acting path (sdqn_net_predict_state)

extern thread_local std::string g_err;
void set_error(const char* fmt, ...);
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
  set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); return SDQN_ERR_HIP; } } while (0)
#define ARGCHK(c, ...) do { if (!(c)) { set_error(__VA_ARGS__); return SDQN_ERR_ARG; } } while (0)

extern hipStream_t g_stream;      // the library stream: everything is ordered on it
extern hipStream_t g_side;        // second stream (the dp probe's cross-stream round trip)
extern hipStream_t g_comm;        // data parallel: the fc4 gradient all-reduce + fc4 update run here, beside the compute stream
extern hipEvent_t g_ev[5];        // fork/join events (timing disabled)
extern int g_dev;                 // device the library streams live on (bound by the first device call)
#define STREAMCHK() do { int r_ = ensure_stream(); if (r_) return r_; } while (0)

const int NSLOT = 64;     // pinned index slots: kernels read the sampled indexes zero-copy
// --prioritized_replay (sdqn_per.hip): the device priorities / sum-tree of one replay handle and what the host keeps about them
struct PerState {
  PerTree t;                                 // device arrays (t.err: mapped host word)
  double alpha = 0.6, eps = 1e-6, beta = 0.4;
  float* newp = nullptr;                     // [B] the head's new priorities (|delta| + eps)^alpha of the last PER step
  int64_t* sidx = nullptr; float* w = nullptr;   // [B] the last sample's indexes and importance weights
  std::vector<PerSeg> rw; bool full = true;  // slots (re)written since the last sampling launch / everything
  std::vector<int64_t> h_sidx;               // host copy of the last sdqn_replay_sample
  bool sample_live = false, gathered = false;   // ... not trained on yet / ... and the last gather took exactly those indexes
};
struct sdqn_replay_s {
  int64_t size = 0; int H = 0, W = 0, hist = 0, B = 0, flags = 0;
  int64_t frame = 0, state = 0;                    // bytes per screen / per state (hist screens); the tuned kernels need 84 x 84 x 4
  bool tuned_geom = true;
  int64_t count = 0, current = 0;
  uint8_t* screens = nullptr; uint8_t* actions = nullptr; int64_t* rewards = nullptr; uint8_t* terminals = nullptr;  // pinned master
  MetaRec* h_meta = nullptr;                       // pinned packed metadata (source of the per-add H2D)
  uint8_t* d_ring = nullptr; MetaRec* d_meta = nullptr;
  uint8_t *d_pre = nullptr, *d_post = nullptr, *d_act = nullptr, *d_term = nullptr; int64_t* d_rew = nullptr;
  uint8_t *h_pre = nullptr, *h_post = nullptr, *h_act = nullptr, *h_term = nullptr; int64_t* h_rew = nullptr;
  int64_t* h_idx = nullptr; int64_t* d_idx_view = nullptr;      // [NSLOT][B] pinned + its device alias
  hipEvent_t slot_ev[NSLOT]; bool slot_busy[NSLOT]; int next_slot = 0;
  int slot_cover[NSLOT]; int pending[NSLOT]; int npending = 0;   // batched release (train_many): slot s is free once slot_ev[slot_cover[s]] has completed
  // tuple API: the device copy of the gathered minibatch (d_pre | d_post) stays valid after getMinibatch() has brought it down; a
  // train(tuple) call on the very same pinned arrays may read it in place instead of uploading 2 x B x state bytes again — when the
  // host copy is as new as the device copy (generations) AND the caller has declared that it did not write into the host arrays
  // (sdqn_replay_declare_minibatch_clean: one-shot, consumed by the next sdqn_net_train_host)
  uint64_t mb_dev_gen = 1, mb_host_gen = 0; bool mb_clean_declared = false, mb_clean_on_device = false;
  hipEvent_t mb_upload_ev = nullptr;      // tuple API: the H2D of h_pre | h_post issued by sdqn_net_train_host (waited for before that call returns)
  // what the last sdqn_replay_gather left in d_rew | d_act | d_term, as [rewards 8 B x B | actions B | terminals B] taken from the host
  // master at enqueue time (== the device metadata in stream order), and the device generation it belongs to: a tuple whose small
  // arrays equal it trains on the device copy (sdqn_net_train_host)
  uint8_t* mb_snap = nullptr; uint64_t mb_snap_gen = 0;
  uint64_t mb_gather_gen = 0;   // device-minibatch generation the last sdqn_replay_gather left (sdqn_replay_declare_minibatch_on_device(h, UINT64_MAX) names it)
  PerState* per = nullptr;      // prioritized replay (nullptr: uniform sampling)
  NStepArgs ns = {1, 0, 0.0, 0.0, 0.0};   // --n_step (sdqn_replay_set_n_step; n = 1: standard transitions)
  // --train_envs (sdqn_replay_set_lanes): lanes > 0 splits the ring into `lanes` rings of lane_len slots that advance
  // together — one fill and one write position for all; count / current stay 0 and every path that reads them asks the helpers below
  int lanes = 0; int64_t lane_len = 0, lane_fill = 0, lane_pos = 0;
};
// index i can be the current frame of a sampled transition: its prestate and its n steps lie in filled slots (of ONE lane)
inline bool replay_idx_ok(const sdqn_replay_s* r, int64_t i) {
  if (!r->lanes) return i >= r->hist && i + r->ns.n - 1 < r->count;
  if (i < 0 || i >= r->size) return false;
  const int64_t l = i % r->lane_len;
  return l >= r->hist && l + r->ns.n - 1 < r->lane_fill;
}
inline int64_t replay_filled(const sdqn_replay_s* r) { return r->lanes ? r->lanes * r->lane_fill : r->count; }
extern std::vector<sdqn_replay_s*> g_replays;      // live handles: sdqn_net_train_host recognises their pinned minibatch buffers

struct Id128 { char b[128]; };   // ncclUniqueId is passed BY VALUE to ncclCommInitRank
struct Rccl {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, Id128, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;   // optional (replica sync at dp_init)
  int (*CommDestroy)(void*) = nullptr;
  int (*CommSplit)(void*, int, int, void**, void*) = nullptr;      // optional (second communicator for the overlapped all-reduce)
  int (*CommAbort)(void*) = nullptr;                              // optional (tears down a communicator whose collective never completed)
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  int (*CommCount)(void*, int*) = nullptr;
  int (*CommUserRank)(void*, int*) = nullptr;
  int (*CommCuDevice)(void*, int*) = nullptr;
};
extern Rccl g_rccl;
#define NCCLCHK(x) do { int e_ = (x); if (e_ != 0) { set_error("%s -> %s", #x, g_rccl.GetErrorString ? g_rccl.GetErrorString(e_) : "rccl error"); return SDQN_ERR_RCCL; } } while (0)

struct ProfPair { int id; hipEvent_t a, b; };
struct sdqn_net_s {
  GenericNet* gen = nullptr;               // float64 / non-84x84x4 configurations: the whole network lives there (generic_net.hip)
  sdqn_net_cfg cfg; int B = 0, A = 0; int64_t NP = 0;   // NP: floats per flat buffer (weights [+ BatchNorm params + running stats])
  int64_t NPW = 0;                         // weights only = offset of the BatchNorm block
  bool bn = false;                         // --batch_norm
  float *x1 = nullptr, *x2 = nullptr, *x3 = nullptr;          // raw linear outputs [2][B*PIX][K] (BatchNorm input; kept for the backward pass)
  float *bn_mean = nullptr, *bn_rstd = nullptr; double* bn_partial = nullptr;
  float *theta = nullptr, *theta_t = nullptr, *state = nullptr, *state2 = nullptr, *g = nullptr;
  int epoch = 0;
  float *a1 = nullptr, *a2 = nullptr, *a3 = nullptr, *slab4 = nullptr, *a4 = nullptr, *d4 = nullptr;
  float *d3 = nullptr, *d2 = nullptr;
  // fp16 mode (cfg.datatype == 1)
  half_t *h_a1 = nullptr, *h_a2 = nullptr, *h_a3 = nullptr, *h_d4 = nullptr, *h_d3p = nullptr, *h_d3 = nullptr,
         *h_d2p = nullptr, *h_d2 = nullptr, *h_d1 = nullptr, *wh[2] = {nullptr, nullptr}, *wht[2] = {nullptr, nullptr};
  float *d3p = nullptr, *d2p = nullptr, *d1 = nullptr, *slab1 = nullptr, *slab2 = nullptr, *slab3 = nullptr;
  float *q = nullptr, *maxq = nullptr, *dq = nullptr, *cost_terms = nullptr, *cost_out = nullptr; double* cost_accum = nullptr;
  // The target options' state (train_options.h): written by the API setters alone, read by both train paths — the generic net
  // holds a pointer to this member.  What each option adds to a tuned step:
  //   double_dqn: the forward launches carry a third net slot (problems.h: wslot)             munchausen / al_alpha > 0 (§22, §28): a forward
  //   of the target net on the prestates in front of every train step (q slot 2) and a head of their own           cql_alpha > 0 (§35), boot_K > 1
  //   (§27), quant_N > 1 (§29), dueling (§32): a head of their own, no launch more; the net's A outputs are K Q-heads / N quantiles of
  //   game_actions(h) actions, or V and A - 1 advantages (fc5's entries outside the two blocks are +0.0 in theta, theta_t and g: TailPlan::mask)
  TrainOptions opt;
  // slots3: a1..a3, slab4, a4, q (and h_a1..h_a3) have room for the third net slot (ensure_slots3: first use of double_dqn / munchausen / al_alpha)
  bool slots3 = false;
  // boot_q: [B][game actions] acting rows of the game loops (one select / mean / dueling launch; the three options are refused together), allocated on
  // first use.  boot_vote / boot_episode: the single-environment acting paths (sdqn_net_act_greedy) — majority vote (testing) or the Q-head of copy 0's
  // episode boot_episode (collecting)
  void* boot_q = nullptr; int boot_vote = 0; int64_t boot_episode = 0;
  // the last tuned step's read-outs, allocated by the setters: quant_targets [B][quant_N] (sdqn_net_debug_read "quantile_targets"), duel_step [2][B]
  // y and delta ("dueling_step")
  float* quant_targets = nullptr; float* duel_step = nullptr;
  // --noisy_nets (sdqn_net_set_noisy; noisy.h, sdqn_noisy.hip): fc4 and fc5 are W = mu + sigma * (e_out * e_in); theta / theta_t hold
  // mu.  nz_sigma: [NP - OFF4] per net, internal layout (the target's aliases the online one without a target net); nz_eff: the effective flat
  // buffers the step's kernels read; nz_state / nz_state2: sigma's optimizer state; nz_eps: [2][NOISY_EPS_NET] the factor vectors last composed;
  // nz_gsig: g_sigma of the last step (option keep_gradients).  nz_step: train steps run as a noisy net = the t of the xi_t the effective
  // buffers hold between steps.  nz_stale: mu or sigma changed outside a train step, the buffers are recomposed before their next use
  // (noisy_fresh).  nz_collecting: the single-environment acting paths use the effective weights (train phase) or mu (test phase)
  bool noisy = false, nz_stale = false, nz_collecting = true; double nz_sigma0 = 0.5; uint64_t nz_seed = 0; int64_t nz_step = 0;
  float *nz_sigma[2] = {nullptr, nullptr}, *nz_eff[2] = {nullptr, nullptr}, *nz_state = nullptr, *nz_state2 = nullptr, *nz_eps = nullptr, *nz_gsig = nullptr;
  // --random_shift (sdqn_net_set_random_shift; shift.h, sdqn_shift.hip): shift_P > 0: every train step that samples from a replay
  // memory (sdqn_net_train_many / _deferred / _replay, prioritized or not) first writes the shifted minibatch into the memory's device
  // minibatch (one launch, shift_minibatch) and runs as the step that reads a device minibatch in place.  shift_step: such steps enqueued =
  // the t of the next step's draws; shift_out: [B][2][2] the (dy, dx) the last launch drew, allocated by the setter.  0: nothing changes
  int shift_P = 0; uint64_t shift_seed = 0; int64_t shift_step = 0; int8_t* shift_out = nullptr;
  // --redo_interval (sdqn_net_set_redo; redo.h, sdqn_redo.hip): redo_interval > 0: every applied train step t (train_iterations) with
  // t % redo_interval == 0 is followed by one recycle event on the library stream (step_applied).  redo_partial / redo_scores / redo_info:
  // the score reduction's partial sums, the 672 scores and the last event's record {event, step, four dormant counts}, allocated on first use
  // (the setter with interval > 0, or the first sdqn_net_redo_scores).  redo_events: events enqueued = the number of the last one.
  // redo_acts_live: slot 0 of a1..a4 holds the online net's prestate activations of the last train step (a forward of its own overwrites them)
  int redo_interval = 0; double redo_tau = 0.1; uint64_t redo_seed = 0; int64_t redo_events = 0; bool redo_acts_live = false;
  double* redo_partial = nullptr; float* redo_scores = nullptr; int64_t* redo_info = nullptr;
  // --reset_interval (sdqn_net_set_reset; reset.h, sdqn_reset.hip): reset_interval > 0: every applied train step t with
  // t % reset_interval == 0 is followed by one reset event on the library stream (step_applied, behind the recycle event): the last
  // reset_layers layers redrawn, the others shrunk by reset_alpha and perturbed, both nets, the optimizer state cleared.  reset_info: the last
  // event's record {event, step}, allocated by the setter or the first sdqn_net_reset_now.  reset_events: events enqueued = the last one's number
  int reset_interval = 0, reset_layers = 2; double reset_alpha = 1.0; uint64_t reset_seed = 0; int64_t reset_events = 0; int64_t* reset_info = nullptr;
  // --weight_decay / --l2_init (sdqn_net_set_regularizer; regularize.h, sdqn_regularize.hip): either > 0: every applied train step is
  // followed by one regulariser launch on the online weights, in front of the soft target update (with --target_tau the two are ONE launch:
  // step_applied).  reg_anchor: [NPW] the weights L2-init pulls toward, allocated and taken when reg_lambda first leaves 0
  // (sdqn_net_anchor_now takes it again); reg_norms: weight_norms' partials and results, allocated by the first read-out.  Both 0: nothing runs
  double reg_wd = 0.0, reg_lambda = 0.0; float* reg_anchor = nullptr; double* reg_norms = nullptr;
  double target_tau = 0.0;                 // --target_tau (sdqn_net_set_target_tau): > 0: every train step is followed by one soft target update
  // --clip_grad_norm (sdqn_net_set_clip_grad_norm): > 0: the flat gradient is scaled to this global L2 norm (of the MEAN
  // gradient) between its reduction and its application.  clip_buf: [CLIP_GRID] partials | {norm, scale} of the last clipped step,
  // allocated when the option is first switched on; clip_ran: such a step has been enqueued
  double clip_grad_norm = 0.0; double* clip_buf = nullptr; bool clip_ran = false;
  uint8_t *st_states = nullptr, *st_act = nullptr, *st_term = nullptr; int64_t* st_rew = nullptr; int64_t* d_idx = nullptr;
  float* h_f = nullptr;                    // pinned scratch for small read-backs
  // acting path (round 4): the head kernel of a predict_state forward writes its Q-values straight into mapped host memory (q_host; q_host_dev
  // = its device alias) and the host polls for them.  spec_*: a forward enqueued AHEAD of its use by sdqn_net_act_step (speculation) — valid
  // while the state buffer generation and the parameters are what they were when it was enqueued
  float *q_host = nullptr, *q_host_dev = nullptr;      // Q_SLOTS slots of 32 floats: every enqueued acting forward gets its OWN slot, so a
  int q_slot = 0;                                       // speculation that was dropped (still in flight) cannot write into the slot being polled
  bool head_q_system = false;              // (run_forward: this forward's head writes system-scope)
  // the acting forward as ONE launch (sdqn_act.hip; float32, no batch-norm): per-XCC scratch copies, fc4 partial slots, control blocks
  float *act_scratch = nullptr, *act_q = nullptr; unsigned* act_ctl = nullptr; unsigned act_seq = 0;
  bool act_on = false, act_last = false, act_inject = false; int act_fallbacks = 0;
  int64_t tuple_calls = 0, tuple_states_skipped = 0, tuple_small_skipped = 0;   // sdqn_net_train_host: calls / calls without the state upload / without any upload
      // act_inject (tests): the next one-launch forward finds its work already claimed and delivers nothing     // act_last: the forward being collected came from that launch
  // deferred cost read-back (sdqn_net_train_many_deferred): pinned ring of cost sums the stream copies into
  double* cost_ring = nullptr; int cost_steps[64] = {0}; int64_t cost_ticket = 0;
  bool spec_pending = false; const void* spec_sb = nullptr; uint64_t spec_gen = 0;
  uint8_t* h_stage[2] = {nullptr, nullptr}; hipEvent_t stage_ev[2] = {nullptr, nullptr}; bool stage_busy[2] = {false, false}; int stage_next = 0;
                                           // tuple API (sdqn_net_train_host): pinned double buffer for the caller's pageable minibatch
  int S4 = 7, S4_cap = 7, tps1 = 1, tps2 = 1, tps3 = 1, ns1 = 1, ns2 = 1, ns3 = 1;
  int64_t train_iterations = 0;
  bool keep_grads = false;                 // true: fc4 gradient materialised in g (readable with which=3), no fused RMSProp
  half_t* gh = nullptr; int* ovf_flag = nullptr; int64_t* ovf_count = nullptr;    // fp16 data parallel: half gradient payload, overflow flag / skipped steps
  int dp_half = 1, dp_half_scale_log2 = -1;  // fp16 mode: all-reduce the gradient as half; -1 = dynamic payload scale (starts at 2^10, device-side), >= 0 = fixed 2^n
  bool h16_wgrad_mfma = true;              // fp16 mode: weight gradients on packed-fp16 MFMA (LDS transposes); false = fp32 MFMA with half operands
  int c1w_in_wgrads = 1;                   // fp16 mode, B >= 128: conv1's weight gradient as a block range of the weight-gradient launch (0 off, 1 last, 2 first)
  bool half_payload_pending = false;       // sdqn_net_grad_from_half ran: the next sdqn_net_apply_update honours the overflow flag / moves the scale
  bool grad_only = false;                  // true: a train step stops after the local gradient sums (update mode 1): what a
                                           // data-parallel rank has before the all-reduce; sdqn_net_apply_update finishes it
  int nw_override[12] = {0};               // tuning hook
  int f4_share[2] = {100, 0};               // % of the fc4-wgrad tiles in bwd3 / bwd2 (rest in bwd1)
  int ns_cap[3] = {1, 1, 1};               // slabs the split-K buffers were allocated for (tuning hook "tps:<layer>")
  bool bt_xcd = true;                      // round 4, B >= 128: XCD-contiguous block maps for fc4_dgrad / bwd3 / bwd2 (float32) and the weight-gradient launch (float16); option "bt_xcd"
  bool bt_on = true; int bt[K_COUNT] = {0};  // round 4, B >= 128 float32: block-tile engine (sdqn_kernels_bt.hip); per kernel id 0 = built-in block shape, n = menu entry, -1 = latency engine
  int xcd_mask[K_COUNT] = {0};             // tuning hook "xcd:<kernel id>": per-launch problem mask (-1 = built-in)
  bool xcd_map = false;                    // XCD-contiguous tile map for EVERY launch: traffic ~ algorithmic, step ~1 % slower (bwd3);
                                           // built-in: only where it also wins time (fc4_fwd: the 7 K-slabs of a tile's W4 panel share an L2)
  bool conv1_bf16 = true;                  // round 3: conv1_fwd on packed-bf16 MFMA (bytes x 3-way bf16 split of W1; sdqn_kernels_r3.hip)
  unsigned short* w1p[2] = {nullptr, nullptr};   // the three bf16 planes of W1, online / target net ([3][32][256] each)
  const int64_t* host_idx_cur = nullptr;   // ring paths: host copy of the indexes of the step being enqueued (valid during run_train only)
  int r3_xcd = 2;                          // XCD-contiguous tile maps of the round-3 kernels: bit 0 conv1_fwd (bf16), bit 1 conv1_wgrad (bf16)
  bool prep_inline = true;                 // B <= 32: the next step's indexes ride in the update launch's kernel arguments (no PCIe read in its prep block)
  int wt = WT_ALL;                         // write-through epilogue stores, bit per launch (kernels.h: WriteThrough)
  int conv1w_bf16 = 1;                 // round 3: conv1_wgrad on packed-bf16 MFMA (bytes x on-the-fly bf16 split of delta1)
  bool conv3_c36 = true;                   // round 3: conv3_fwd on 36-deep K-chunks (one chunk per wave; sdqn_kernels_r3.hip)
  bool arg_preload = true;                 // the B < 128 fp32 step kernels take their hot arguments from the leading block (gemm_engine.h: Lead); 0: from the struct
  bool fused_launches = true;              // independent backward stages share one launch (K_BWD3, K_BWD2)
  // profiler
  bool prof_on = false; int prof_filter = -1;
  int prof_mode = 1;                                        // 1: kernel-packet timestamps (hipExtLaunchKernel), 0: hipEventRecord markers around the launch
  int prof_every = 1; int64_t prof_seen[K_COUNT] = {0};     // bracket only every prof_every-th launch of a kernel (an event pair costs ~2-3 us of queue time)
  std::vector<ProfPair> prof_pending; std::vector<hipEvent_t> prof_free;
  double prof_ms[K_COUNT]; int64_t prof_n[K_COUNT];
  // data parallel
  void* comm = nullptr; int rank = 0, nranks = 1; int nccl_rc = 0;
  // overlapped data parallel (run_train): comm2 carries the fc4 gradient (95 % of the bytes) on g_comm while the
  // compute stream finishes the backward pass and starts the next forward; ev_w4 = "W4 of the last step is updated"
  void* comm2 = nullptr; hipEvent_t ev_g4 = nullptr, ev_w4 = nullptr; bool w4_pending = false;
  bool dp_sync_replicas = true;   // dp_init broadcasts rank 0's theta / theta_t / optimizer state (set_option "dp_sync_replicas" 0: keep own)
  // Overlapped form (fc4's 95 % of the payload all-reduced + applied on a second communicator / stream under the rest of the step).
  // dp_overlap_req: -1 AUTO (default, round 4): sdqn_dp_init creates the second communicator whenever nranks >= 2, but the form only
  //   becomes ACTIVE (dp_overlap) after sdqn_dp_probe succeeded on EVERY rank (the caller votes over its control plane) and
  //   sdqn_dp_set_overlap(1) was called; any rank timing out -> sdqn_dp_set_overlap(0) on all ranks: second communicator torn down,
  //   the serial form (one all-reduce on the library stream) runs.  1: forced on at dp_init (single-rank tests), 0: never.
  int dp_overlap_req = -1;
  bool dp_overlap = false;        // the overlapped form is active
  int dp_probe_result = -1;       // -1 not probed, 0 timed out / failed, 1 ok (sdqn_dp_probe)
  int wt_kid = -1; unsigned long long* wt_words = nullptr;     // timing build: per-wave stamps around launches of this id (pinned: {buffer, null, blocks})
  // --train_envs (sdqn_env_collect): the copies' records and the two state-window buffers stay here between calls, so a
  // training run is one continuous stream of games
  uint8_t* col_win = nullptr; void* col_recs = nullptr; int col_N = 0; int64_t col_t = 0; size_t col_state = 0; int col_game = 0;    // (col_game: which game the copies play)
  std::vector<void*> allocs;
};
#define GENCHK(x) do { hipError_t ge_ = (x); if (ge_ != hipSuccess) { set_error("%s -> %s", #x, hipGetErrorString(ge_)); return ge_ == hipErrorInvalidValue ? SDQN_ERR_ARG : SDQN_ERR_HIP; } } while (0)

constexpr int SB_SLOTS = 64;
uint64_t next_statebuf_gen();
struct sdqn_statebuf_s {
  uint8_t* d = nullptr;          // [SB_SLOTS][FRAME]
  uint8_t* host = nullptr;       // [hist][FRAME] mirror in state_buffer.py order (oldest first)
  uint8_t* stage = nullptr;      // pinned [SB_SLOTS][FRAME]: staging slot i feeds ring slot i
  int hist = 0;
  int64_t frame = 0;             // bytes per screen
  int pos = 0;                   // slot of the newest frame; window = slots [pos-hist+1, pos]
  uint64_t gen = next_statebuf_gen();   // bumped by every add / reset: identifies the state a speculative forward was enqueued for
                                 // (own 2^40 range per buffer: a buffer allocated where a destroyed one lay never matches its generations)
};

// which launches a train step is made of / how its optimizer pass runs (sdqn_api_step.hip: step_structure, update_form)
enum StepStructure { STEP_FUSED = 0, STEP_H16_BT = 1, STEP_DP_OVERLAP = 2, STEP_UNFUSED = 3 };
enum UpdateForm { UPD_SINGLE = 0, UPD_DP_SERIAL = 1, UPD_DP_OVERLAP = 2, UPD_GRAD_ONLY = 3, UPD_CLIP = 4 };
// What one launch of the step gets on top of the step's arguments: xcd_map = (the step's & xcd_keep) | xcd_bits, the fc4-wgrad tile range that
// rides in it, the LaunchVariant bits.  The default changes nothing (step_args hands out all F4_TILES tiles).
constexpr int F4_TILES = (NIN4 / 32) * (NFC / 32);
struct LaunchPlan { int xcd_keep = ~0, xcd_bits = 0, variant = 0, f4w_first = 0, f4w_count = F4_TILES; };
// The optimizer tail (run_update_tail): [mode 1: local sums -> g] -> [exchange] -> [mask] -> [clip] -> apply (mode 2, or mode 0 = sums and apply in one
// launch) -> [BatchNorm parameters].  The next step's prep rides in the last update launch of the sequence.
enum Exchange { XCH_NONE = 0, XCH_F32, XCH_HALF, XCH_GROUPED };   // all-reduce of g: fp32 | as half (float16 nets) | overlapped form: the conv and fc5 ranges as one group
struct TailPlan {
  bool reduce_first = false;
  Exchange exchange = XCH_NONE;
  bool noisy = false;                      // --noisy_nets: the sigma launch (g_sigma = g * e, the optimizer on sigma) where the mask sits: behind the sums, in front of the apply launch
  bool mask = false;                       // --dueling: fc5's block mask on g, one launch behind the sums / exchange, in front of the clip
  bool clip = false;                       // --clip_grad_norm: the two clip launches in front of the apply launch
  bool ovf = false;                        // the gradient came through the half payload: the apply launch honours the overflow flag
  int apply_mode = 0;                      // UpdateArgs::mode of the apply launch: 0 | 2 | -1 nothing is applied (grad_only)
  double divisor = 0.0;                    // A9's bsz of the apply launch (and of the clip): B x ranks, or sdqn_net_apply_update's argument
  int skip_fc4 = 0;                        // fc4 is applied elsewhere: in its weight-gradient tiles (fuse_rms) or by the overlapped form's side launch
};
// Everything run_train decides, taken once per step from the handle (sdqn_api_step.hip: step_plan; no HIP call, no side effect)
struct StepPlan {
  StepStructure structure; UpdateForm update;
  int fuse_rms;                            // StepArgs::fuse_rms: fc4's RMSProp rides in its weight-gradient tiles
  int extra_fwd;                           // forward in front of the step (run_extra_forward): 0 none | 1 --munchausen / --advantage_learning (1, 0) | 2 --double_dqn with --batch_norm (0, 1)
  int head_train;                          // HeadArgs::train of the step's head: the HeadMode (launch_route.h) of the option that is on, 0: the caller's
  int nz;                                  // net slots of the step's forward (3: the Double DQN slot rides in it)
  bool side_fc4;                           // overlapped data parallel: fc4's all-reduce + update on g_comm behind bwd3
  LaunchPlan launch[K_WGRADS + 1];         // by kernel id
  TailPlan tail;
};
// ---- functions that cross a file boundary -------------------------------------------------------------------------------
int ensure_stream();
int sample_checked(uint32_t* mt, const uint8_t* terminals, int64_t count, int64_t current, int hist,
                          int batch, int64_t* idx_out, int64_t* draws_out, int nstep = 1);
int sample_checked_lanes(uint32_t* mt, const uint8_t* terminals, int lanes, int64_t lane_len, int64_t fill, int64_t pos, int hist,
                         int batch, int64_t* idx_out, int64_t* draws_out, int nstep);
int replay_sample_uniform(sdqn_replay_s* r, uint32_t* mt, int64_t* idx_out, int64_t* draws_out);   // the ring's own rule: lanes or not
int nstep_match(const sdqn_net_s* h, const sdqn_replay_s* r);       // --n_step: the memory's (n, discount, reward clip) equal the net's
double nstep_gamma_n(int n, double gamma);                         // gamma^n by repeated multiplication (the n-step loop's g)
int replay_free(sdqn_replay_s* r);
int64_t replay_add_meta(sdqn_replay_s* r, int action, int64_t reward, int terminal);
int replay_add_commit(sdqn_replay_s* r, int64_t c);
int replay_flush_pending(sdqn_replay_s* r);
int replay_push_idx(sdqn_replay_s* r, const int64_t* idx, int* slot_out, const int64_t** dev);
int replay_release_idx(sdqn_replay_s* r, int slot);
int replay_release_idx_batched(sdqn_replay_s* r, int slot, bool flush);
GatherArgs gather_args(sdqn_replay_s* r, const int64_t* didx);
int replay_gather_generic(sdqn_replay_s* r, const int64_t* didx);
int rccl_load(const char* path);
int dalloc(sdqn_net_s* h, void** p, size_t bytes, bool zero = true);
int net_free(sdqn_net_s* h);
float* which_buf(sdqn_net_s* h, int which);
bool bn_layer_span(sdqn_net_s* h, int which, int layer, float** base, int64_t* n);
int gen_set(sdqn_net_s* h, int which, int layer, const void* w, int64_t n, bool f64);
int gen_get(sdqn_net_s* h, int which, int layer, void* w, int64_t n, bool f64);
int ensure_slots3(sdqn_net_s* h);                                  // room for a third net slot in a1..a4, slab4, q (first use of --double_dqn / --munchausen / --advantage_learning)
int target_blend(sdqn_net_s* h, double tau);                       // one soft target update now (tau in (0, 1]; the caller has joined g_comm)
int step_blend(sdqn_net_s* h);                                     // the blend of --target_tau behind an applied train step, or nothing
int gen_step_done(sdqn_net_s* h);                                  // generic path: a train step was enqueued ([clip + deferred update,] counter, step_blend)
// the actions a transition may hold (--bootstrap_heads / --quantiles: A is K / N times that; --dueling: one more, the V row)
inline int game_actions(const sdqn_net_s* h) { return game_actions(h->opt, h->A); }
// --noisy_nets: the effective buffers as of xi_{nz_step}, recomposed when stale (nothing on a plain net); the acting weights of the phase
int noisy_fresh(sdqn_net_s* h);
int noisy_compose(sdqn_net_s* h, int64_t step, int nets);
inline bool noisy_acting(const sdqn_net_s* h) { return h->noisy && h->nz_collecting; }
inline bool clip_on(const sdqn_net_s* h) { return h->clip_grad_norm > 0.0; }
// The options of option_table.h that are on, as a mask of option_bit(OptionId); values (may be NULL): [OPT_COUNT], the values the messages
// print
inline unsigned active_options(const sdqn_net_s* h, int* values = nullptr) {
  const TrainOptions& o = h->opt;
  const bool on[OPT_COUNT] = {o.double_dqn, o.munchausen, advantage_on(o), cql_on(o), bootstrap_on(o), quantiles_on(o), o.dueling,
                              h->noisy, h->cfg.batch_norm != 0.0, clip_on(h), h->target_tau > 0.0};
  unsigned mask = 0;
  for (int id = 0; id < OPT_COUNT; ++id) { if (on[id]) mask |= option_bit(id); if (values) values[id] = 0; }
  if (values) { values[OPT_BOOTSTRAP_HEADS] = o.boot_K; values[OPT_QUANTILES] = o.quant_N; }
  return mask;
}
int clip_gradient(sdqn_net_s* h, double bsz);                      // --clip_grad_norm: the two launches on g between update modes 1 and 2 (nothing when off)
StepPlan step_plan(const sdqn_net_s* h);
int run_update_tail(sdqn_net_s* h, UpdateArgs u, const TailPlan& t, const PrepArgs* next = nullptr);
int prof_collect(sdqn_net_s* h);
int prof_event(sdqn_net_s* h, hipEvent_t* e);
hipError_t dp_allreduce(sdqn_net_s* h, void* buf, size_t count, int dtype, void* comm, hipStream_t s);
StepArgs step_args(sdqn_net_s* h);
HeadArgs head_args(sdqn_net_s* h, int train);
int join_comm(sdqn_net_s* h);
BnArgs bn_args(sdqn_net_s* h, const StepArgs& a, int layer, int train);
hipError_t launch_tuned(sdqn_net_s* h, int id, StepArgs a, hipStream_t s, int variant = 0);    // variant: LaunchVariant bits
int run_forward(sdqn_net_s* h, const StepArgs& a, const HeadArgs& hd);
UpdateArgs make_update_args(sdqn_net_s* h, const StepArgs& a);
StepStructure step_structure(const sdqn_net_s* h);
UpdateForm update_form(const sdqn_net_s* h);
int run_train(sdqn_net_s* h, const StepArgs& a, const HeadArgs& hd, const PrepArgs* next = nullptr);
int read_cost(sdqn_net_s* h, float* cost_out);                      // either path; ends with per_check_all
int read_mean_cost(sdqn_net_s* h, int n_steps, float* mean_cost);
// noisy (a --noisy_nets net): the forward reads the effective weights (the caller has run noisy_fresh), else mu
int predict_forward_tuned(sdqn_net_s* h, const uint8_t* states, const HeadArgs& hd, int B = 0, bool noisy = false);   // B = 0: the net's batch
int predict_forward(sdqn_net_s* h, const uint8_t* states, int rows, const void** q, int* q_f64, bool noisy = false);
StepArgs ring_step_args(sdqn_net_s* h, const sdqn_replay_s* r);
int run_ring_step(sdqn_net_s* h, sdqn_replay_s* r, const int64_t* host_idx, const HeadArgs& hd, const PrepArgs* next = nullptr);
int check_replay_geometry(const sdqn_net_s* h, const sdqn_replay_s* r);
// What follows an applied train step of the tuned path (sdqn_api_net.hip: step_applied, the one place that knows the order) and its parts:
// one regulariser launch (fuse: it blends the target net too), one ReDo event, one reset event — each as its *_now entry point runs it
int step_applied(sdqn_net_s* h, bool interval_events);
int regularize_launch(sdqn_net_s* h, double wd, double lambda, bool fuse);      // sdqn_api_regularize.hip
int redo_event(sdqn_net_s* h);                                                  // sdqn_api_redo.hip
int reset_event(sdqn_net_s* h);                                                 // sdqn_api_reset.hip
// sdqn_redo_draw / sdqn_reset_draw: word `index` under an event's key and the initialiser's draw of it in `layer` of 1..layers
inline int keyed_init_draw(uint64_t key, int64_t index, int layer, int layers, uint64_t* word, float* value) {
  ARGCHK(index >= 0 && layer >= 1 && layer <= layers, "bad arguments (index %lld, layer %d of 1..%d)", (long long)index, layer, layers);
  const uint64_t w = stream_keyed(key, (uint64_t)index);
  if (word) *word = w;
  if (value) *value = init_draw(w, layer);
  return SDQN_OK;
}
inline bool redo_on(const sdqn_net_s* h) { return h->redo_interval > 0; }
inline bool reset_on(const sdqn_net_s* h) { return h->reset_interval > 0; }
inline bool regularizer_on(const sdqn_net_s* h) { return h->reg_wd > 0.0 || h->reg_lambda > 0.0; }
// theta (net_slot 0) or theta- (1) was written in [first, last) of the flat buffer: what is derived from it is rebuilt on the library stream
int refresh_derived(sdqn_net_s* h, int net_slot, int64_t first, int64_t last);
// option_table.h's feature rows against this handle: `flag` of `feature` refuses the net | a feature that is on refuses `property`
int refuse_feature(const sdqn_net_s* h, int feature, const char* flag);
int refuse_beside_features(const sdqn_net_s* h, int property, int ranks);
int shift_minibatch(sdqn_net_s* h, sdqn_replay_s* r, const int64_t* didx);   // --random_shift: the launch (the caller has checked shift_P > 0); didx: the step's indexes as the device reads them
bool act_sum_partials(const float* part, int A, float* q_out);
const uint8_t* statebuf_window(sdqn_statebuf_s* s);
int statebuf_advance(sdqn_statebuf_s* s, uint8_t** host_frame, uint8_t** dev_slot);
int predict_state_enqueue(sdqn_net_s* h, sdqn_statebuf_s* sb);
bool act_trace();
int predict_state_collect(sdqn_net_s* h, float* q_out);
PrepArgs prep_args(sdqn_net_s* h, sdqn_replay_s* r, const int64_t* pinned_idx);
int check_ring_actions(sdqn_net_s* h, sdqn_replay_s* r, const int64_t* idx);
// prioritized replay (sdqn_per.hip)
int per_free(PerState* p);
void per_mark(sdqn_replay_s* r, int64_t first, int64_t n);
void per_mark_all(sdqn_replay_s* r);
int per_check(sdqn_replay_s* r);
int per_sample_host(sdqn_replay_s* r, uint32_t* mt, int64_t* idx_out, int64_t* draws_out);
void per_note_gather(sdqn_replay_s* r, const int64_t* idx);
bool per_owns_minibatch(sdqn_replay_s* r);
int per_train_many(sdqn_net_s* h, sdqn_replay_s* r, uint32_t* mt, int n_steps, float* mean_cost);
int per_train_replay(sdqn_net_s* h, sdqn_replay_s* r, const int64_t* idx_host, float* cost_out);
int per_train_host_step(sdqn_net_s* h, sdqn_replay_s* r, const StepArgs& a, HeadArgs hd);
void per_gen_arm(sdqn_net_s* h, sdqn_replay_s* r);
int per_gen_finish(sdqn_net_s* h, sdqn_replay_s* r);
int per_check_all();

inline bool prof_single_kernel(int kid) { return kid != K_ALLREDUCE && kid != K_BN; }
// prof_filter: a kernel id, -1 every launch, PROF_GENERIC_ROWS the rows a generic-path network has (its own launches are not bracketed): the
// soft target update and the update slot's launches of a clipped step
constexpr int PROF_GENERIC_ROWS = -2;
inline bool prof_wants(int filter, int kid) { return filter == -1 || filter == kid || (filter == PROF_GENERIC_ROWS && (kid == K_TARGET || kid == K_UPDATE)); }
#ifdef SDQN_TIMING
namespace sdqn { hipError_t set_wave_timing_buffer(unsigned long long* const* p, const unsigned* nb, hipStream_t s); }
// timing build: sdqn_debug_time_step_waves arms per-wave stamps around ONE launch id of a real train step (h->wt_kid), stream-ordered
#define SDQN_WAVE_TIMING_ARM(STRM, KID) do { if (h->wt_kid == (KID) && h->wt_words) HIPCHK(sdqn::set_wave_timing_buffer((unsigned long long* const*)h->wt_words, (const unsigned*)(h->wt_words + 2), (STRM))); } while (0)
#define SDQN_WAVE_TIMING_DISARM(STRM, KID) do { if (h->wt_kid == (KID) && h->wt_words) HIPCHK(sdqn::set_wave_timing_buffer((unsigned long long* const*)(h->wt_words + 1), (const unsigned*)(h->wt_words + 2), (STRM))); } while (0)
#else
#define SDQN_WAVE_TIMING_ARM(STRM, KID) do {} while (0)
#define SDQN_WAVE_TIMING_DISARM(STRM, KID) do {} while (0)
#endif
#define LAUNCH_ON(STRM, KID, expr) do { \
  const bool pf_ = h->prof_on && prof_wants(h->prof_filter, (KID)) && (h->prof_seen[KID]++ % h->prof_every) == 0; ProfPair pp_; \
  const bool px_ = pf_ && h->prof_mode == 1 && prof_single_kernel(KID); \
  if (pf_) { pp_.id = (KID); int r1_ = prof_event(h, &pp_.a); if (r1_) return r1_; r1_ = prof_event(h, &pp_.b); if (r1_) return r1_; \
             if (px_) { sdqn::LaunchEvents& le = sdqn::launch_events(); le.start = pp_.a; le.stop = pp_.b; le.used = false; } \
             else HIPCHK(hipEventRecord(pp_.a, (STRM))); } \
  SDQN_WAVE_TIMING_ARM(STRM, KID); \
  hipError_t le_ = (expr); \
  SDQN_WAVE_TIMING_DISARM(STRM, KID); \
  bool pu_ = true; \
  if (px_) { sdqn::LaunchEvents& le = sdqn::launch_events(); pu_ = le.used; le.start = le.stop = nullptr; le.used = false; } \
  if (le_ != hipSuccess) { \
    if ((KID) == K_ALLREDUCE && h->nccl_rc != 0) { \
      set_error("ncclAllReduce (rank %d of %d) -> %s", h->rank, h->nranks, g_rccl.GetErrorString ? g_rccl.GetErrorString(h->nccl_rc) : "rccl error"); \
      return SDQN_ERR_RCCL; } \
    set_error("launch %s -> %s", kernel_name(KID), hipGetErrorString(le_)); return SDQN_ERR_HIP; } \
  if (pf_ && !pu_) { h->prof_free.push_back(pp_.a); h->prof_free.push_back(pp_.b); }     /* (a launch path that did not take the events: no sample) */ \
  else if (pf_) { if (!px_) HIPCHK(hipEventRecord(pp_.b, (STRM))); h->prof_pending.push_back(pp_); \
             if (h->prof_pending.size() > 16384) { int r2_ = prof_collect(h); if (r2_) return r2_; } } \
} while (0)
#define LAUNCH(KID, expr) LAUNCH_ON(g_stream, KID, expr)


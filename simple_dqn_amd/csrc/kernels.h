// kernels.h — launch interface between the host orchestration (sdqn_api_*.hip) and the device code: the argument structs of every launch,
// launch_kernel (resolve the route of a GEMM-shaped stage, then run its executor) and the single-purpose launchers.  Kernel ids (launch_route.h)
// double as the profiler's slots.
#pragma once
#include <cstddef>
#include <hip/hip_runtime.h>
#include "problems.h"
#include "launch.h"
#include "launch_route.h"
#include "bootstrap.h"
#include "quantile.h"
#include "dueling.h"

namespace sdqn {

const char* kernel_name(int id);


struct HeadArgs {
  const uint8_t* st_actions;    // minibatch metadata (staged from the host, or gathered by prep_kernel)
  const int64_t* st_rewards;
  const uint8_t* st_terminals;
  float* q;                     // [nz][B][A] q-values of the net slots (problems.h: wslot)
  float* maxq;                  // [B]
  float* dq;                    // [B][A] clipped deltas
  float* cost_terms;            // [B]  0.5 * delta^2 (pre-clip)
  double discount, min_reward, max_reward;
  float clip_error;
  int train;                    // a HeadMode (launch_route.h): HEAD_PREDICT, HEAD_TRAIN, or the train step of an option with a head of its own
  // --munchausen, read when train == HEAD_MUNCHAUSEN: bonus scale alpha, softmax temperature tau, lower clip l0 of tau ln pi.  They lie
  // in the 24 bytes a retired option's fields left: every later field keeps its offset (see StepArgs::reserved_)
  // --advantage_learning, read when train == HEAD_ADVANTAGE: the gap scale alpha in (0, 1) and the persistent (PAL) switch.  The two
  // options are refused together (sdqn_net_set_advantage_learning), so they share mu_alpha's and mu_tau's bytes: no field moves
  // --cql_alpha, read when train == HEAD_CQL: the regulariser's scale alpha > 0.  Refused together with both (sdqn_net_set_cql): the
  // same bytes once more
  union { double mu_alpha; double al_alpha; double cql_alpha; };
  union { double mu_tau; int al_persistent; };
  double mu_clip;
  // --prioritized_replay (sdqn_per.hip): per_w != nullptr selects the PER head — dq = w clip(delta), cost term 0.5 w delta^2, and
  // per_p[n] = (|delta| + per_eps)^per_alpha, the new priority the next per_step launch writes back
  const float* per_w; float* per_p; double per_alpha, per_eps;
  // --n_step: nstep > 1 selects the n-step head — st_rewards holds the returns R as doubles, st_terminals the done flags,
  // the target is R (done) or R + gamma_n * max Q' with gamma_n = discount^n by repeated multiplication, no reward clip
  int nstep; double gamma_n;
};

struct PrepArgs {                // pinned index slot + ring metadata -> device-resident (idx, a, r, t) of this step
  const int64_t* idx_pinned;    // [B] zero-copy view of the pinned slot
  const MetaRec* meta;          // ring metadata mirror
  int64_t* idx;                 // [B] device
  uint8_t* actions;             // [B] device staging shared with the host-minibatch path
  int64_t* rewards;
  uint8_t* terminals;
  int B;
  // B <= 32: the indexes themselves (host data at launch time) ride in the kernel arguments, so the prep block of the update launch
  // starts with a load from the argument segment instead of a zero-copy read of pinned host memory over PCIe (~2 us: it was the longest
  // dependency chain of the whole update launch)
  int idx_in_valid;
  int64_t idx_in[32];
  NStepArgs ns;                 // --n_step: rewards / terminals receive (R, done) (problems.h stage_meta)
};

struct UpdateArgs {
  float* theta;                 // online parameters (flat, internal layout)
  float* state;                 // RMSProp state
  float* g;                     // flat gradient sum
  const float* slab[3];
  int ns[3];
  const float* dq;              // [B][A]
  const float* a4;              // online a4 [B][512]
  const float* cost_terms;
  float* cost_out;              // [1]
  double* cost_accum;           // running sum over steps
  int B, A;
  int mode;                     // 0 fused reduce+apply, 1 reduce only (-> g), 2 apply only (g already reduced)
  int skip_fc4;                 // fc4 already updated inside fc4_wgrad's epilogue (StepArgs::fuse_rms), or by the only_fc4 launch
  int only_fc4;                 // overlapped data parallel: this launch (on the comm stream) applies the fc4 range only
  PrepArgs next;                // next.B > 0: also do the NEXT step's prep (train_many samples one step ahead)
  float bsz;                    // divisor of A9 (B, or R*B under data parallel)
  float rho, one_minus_rho, lr, eps;
  int opt;                      // 0 RMSProp, 1 Adam, 2 Adadelta (deepqnetwork.py:50-59)
  float* state2;                // Adam v / Adadelta E[dx^2]
  float beta1, one_minus_beta1, beta2, one_minus_beta2, lr_t;   // Adam: lr_t = lr*sqrt(1-b2^t)/(1-b1^t), t = epoch+1
  half_t* wh;                   // fp16 mode: half copies of theta refreshed by the update (master layout / transposed)
  half_t* wht;
  unsigned short* w1p;          // conv1's three bf16 planes of the ONLINE net, rewritten with W1 (nullptr: not maintained)
  int arg_preload;              // 1: update_kernel's leading parameter block is live (gemm_engine.h: Lead), 0: it reads this struct
  int reserved_[3];             // (retired options' fields: every other field keeps its offset — update_kernel preloads them by name)
  int wt;                       // 1: the new parameters / optimizer state leave with write-through (sc1) stores
  int reserved2_[3];
  int64_t bn_first;             // --batch_norm: element offset of the [beta|gamma] block (bn_update_kernel); BN_PARAMS elements
  const int* ovf_flag;          // fp16 data parallel (update_kernel<true>): != 0 -> the all-reduced half gradient overflowed, leave theta / state untouched
  int64_t* ovf_count;           //   ... and count the skipped step
  int ovf_dynamic;              //   1: block 0 also moves the payload scale (state[1]) — halve on overflow, double after 200 clean steps
};

// The kernel-argument layouts are part of the tuned kernels (StepArgs::reserved_, problems.h): frozen where a retired field became reserved bytes
static_assert(sizeof(HeadArgs) == 160 && offsetof(HeadArgs, train) == 84 && offsetof(HeadArgs, mu_alpha) == 88 && offsetof(HeadArgs, mu_clip) == 104 &&
              offsetof(HeadArgs, al_alpha) == offsetof(HeadArgs, mu_alpha) && offsetof(HeadArgs, al_persistent) == offsetof(HeadArgs, mu_tau) &&
              offsetof(HeadArgs, cql_alpha) == offsetof(HeadArgs, mu_alpha) &&
              offsetof(HeadArgs, per_w) == 112 && offsetof(HeadArgs, per_eps) == 136 &&
              offsetof(HeadArgs, nstep) == 144 && offsetof(HeadArgs, gamma_n) == 152, "HeadArgs layout");
static_assert(sizeof(PrepArgs) == 344 && offsetof(PrepArgs, idx_in_valid) == 52 && offsetof(PrepArgs, idx_in) == 56 && offsetof(PrepArgs, ns) == 312, "PrepArgs layout");
static_assert(sizeof(UpdateArgs) == 616 && offsetof(UpdateArgs, next) == 128 && offsetof(UpdateArgs, next) + offsetof(PrepArgs, idx_in) == 184 &&
              offsetof(UpdateArgs, bsz) == 472 && offsetof(UpdateArgs, w1p) == 544 && offsetof(UpdateArgs, wt) == 568 && offsetof(UpdateArgs, bn_first) == 584 &&
              offsetof(UpdateArgs, ovf_flag) == 592 && offsetof(UpdateArgs, ovf_count) == 600 && offsetof(UpdateArgs, ovf_dynamic) == 608, "UpdateArgs layout");

struct BnArgs {                  // one BatchNorm layer (bn_kernels.hip); activations NHWC: rows x C, C contiguous
  int layer;                    // 0..3 = after conv1, conv2, conv3, fc4
  int C, rows;                  // features; rows per net (B*P*Q, or B for fc4)
  int nz;                       // nets in this forward pass (2 = online + target, 1 = predict)
  int train;                    // 1: z = 0 normalises with batch statistics and updates the running ones
  const float* x;               // raw linear output [nz][rows][C]; fc4: the split-K slabs [S4][2][B][512]
  int S4, B;                    // fc4 only (S4 > 0)
  float* a;                     // activated output [nz][rows][C]
  float* theta[2];              // flat parameter buffers (BatchNorm block at off_bn)
  int64_t off_bn;
  double* partial;              // [row blocks][C][2]
  float* mean; float* rstd;     // [C] batch statistics of z = 0 (kept for the backward pass)
  float* d;                     // backward: dense delta [rows][C], transformed in place
  float* dpad;                  // optional zero-padded copy [n][PD][PD][C] (operand of the next dgrad)
  int PQ, Qw, PD, pad;
  float* g;                     // flat gradient buffer
};

struct GatherArgs {
  const uint8_t* ring;          // [size][84][84]
  const MetaRec* meta;
  const int64_t* idx;           // [B]
  uint8_t* pre;                 // [B][4][84][84]
  uint8_t* post;
  uint8_t* actions;             // [B]
  int64_t* rewards;
  uint8_t* terminals;
  int B;
  NStepArgs ns;                 // --n_step: the poststate starts ns.n frames after the prestate; rewards / terminals receive (R, done)
};

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------
// one parameter of Neon's optimizers [neon-recalled, SURVEY.md A9/A10 + §8a-bis "non-default branches"];
// every one starts with grad = grad / be.bsz
__device__ inline float opt_apply(float w, float& s1, float& s2, float gsum, const UpdateArgs& u) {
  if (u.opt == 0) return rms_step(w, s1, gsum, u.bsz, u.rho, u.one_minus_rho, u.lr, u.eps);
  const float g = div_bsz(gsum, u.bsz);
  if (u.opt == 1) {                                   // Adam: m, v; bias correction folded into lr_t (t = epoch + 1)
    s1 = s1 * u.beta1 + u.one_minus_beta1 * g;
    s2 = s2 * u.beta2 + (u.one_minus_beta2 * g) * g;
    return w - (u.lr_t * s1) / (sqrtf(s2) + u.eps);
  }
  s1 = s1 * u.rho + (u.one_minus_rho * g) * g;        // Adadelta: E[g^2], E[dx^2]
  const float upd = sqrtf((s2 + u.eps) / (s1 + u.eps)) * g;
  s2 = s2 * u.rho + (u.one_minus_rho * upd) * upd;
  return w - upd;
}
#endif

// Which kernel a stage runs is resolve_route's answer (launch_route.h); launch_kernel resolves once and hands the Route to the executor of the
// translation unit that owns the launch form.  An id that rides in another id's launch (Route::unit == U_NONE) launches nothing.
inline RouteKey route_key(const StepArgs& a, const LaunchTune& t) {
  return RouteKey{a.B, a.nz, a.h16, a.bn, a.f4w_count, a.from_ring, a.tps1, a.src != nullptr, a.w1p[0] && a.w1p[a.nz > 1 ? 1 : 0], t.host_idx != nullptr};
}
hipError_t launch_lat(const Route& r, int id, const StepArgs& a, const LaunchTune& t, hipStream_t s);      // sdqn_kernels.hip: float32 on the latency engine
hipError_t launch_ext(const Route& r, int id, const StepArgs& a, const LaunchTune& t, hipStream_t s);      // sdqn_kernels_ext.hip: float16 on the latency engine
hipError_t launch_r3(const Route& r, int id, const StepArgs& a, const LaunchTune& t, hipStream_t s);       // sdqn_kernels_r3.hip: bf16 conv1 kernels, write-through forms, conv3 on 36-deep chunks
hipError_t launch_bt(const Route& r, int id, const StepArgs& a, const LaunchTune& t, hipStream_t s);       // sdqn_kernels_bt.hip: block tiles and the hand-written kernels beside them
hipError_t launch_ss(const Route& r, int id, const StepArgs& a, const LaunchTune& t, hipStream_t s);       // sdqn_kernels_ss.hip: sample-stationary convolution chains
hipError_t launch_kernel(int id, const StepArgs& a, const LaunchTune& t, hipStream_t s);     // the GEMM-shaped stages (single or multi-problem launches)
// q_system_scope: h.q is mapped host memory (acting path); boot / quant / duel: what h.train == HEAD_BOOTSTRAP / HEAD_QUANTILE / HEAD_DUELING
// needs beside the two structs (refused without it)
hipError_t launch_head(const StepArgs& a, const HeadArgs& h, hipStream_t s, bool q_system_scope = false, const BootArgs* boot = nullptr,
                       const QuantArgs* quant = nullptr, const DuelArgs* duel = nullptr);
hipError_t launch_head_dueling(const StepArgs& a, const HeadArgs& h, const DuelArgs& b, hipStream_t s);     // sdqn_dueling.hip: what launch_head runs for HEAD_DUELING
// sdqn_dueling.hip: fc5's block mask on the [rows][H] fc5 range of a flat vector (float or double): the entries outside the two streams become +0.0
hipError_t launch_dueling_mask(void* w5, bool f64, int rows, int H, hipStream_t s);
// sdqn_dueling.hip: [M][A + 1] rows -> [M][A] action values Q = V + Adv - mean(Adv) (float or double)
hipError_t launch_dueling_q(const void* q, void* out, bool f64, int M, int A, hipStream_t s);
hipError_t launch_head_quantile(const StepArgs& a, const HeadArgs& h, const QuantArgs& b, hipStream_t s);     // sdqn_quantile.hip: what launch_head runs for HEAD_QUANTILE
// sdqn_quantile.hip: [M][N A] Q rows -> [M][A] action values, the mean over the quantiles (float or double)
hipError_t launch_quantile_mean(const void* q, void* out, bool f64, int M, int N, int A, hipStream_t s);
hipError_t launch_head_munchausen(const StepArgs& a, const HeadArgs& h, hipStream_t s);     // sdqn_munchausen.hip: what launch_head runs for HEAD_MUNCHAUSEN
hipError_t launch_head_bootstrap(const StepArgs& a, const HeadArgs& h, const BootArgs& b, hipStream_t s);     // sdqn_bootstrap.hip: what launch_head runs for HEAD_BOOTSTRAP
hipError_t launch_head_advantage(const StepArgs& a, const HeadArgs& h, hipStream_t s);      // sdqn_advantage.hip: what launch_head runs for HEAD_ADVANTAGE
hipError_t launch_head_cql(const StepArgs& a, const HeadArgs& h, hipStream_t s);            // sdqn_cql.hip: what launch_head runs for HEAD_CQL
// sdqn_bootstrap.hip: [N][K A] Q rows -> [N][A] acting rows (float or double); vote = 0: the slice of Q-head k(e, episodes_e), the int64 episode
// counter of copy e at recs + e stride + offset; vote = 1: the vote counts
hipError_t launch_bootstrap_select(const void* q, void* out, bool f64, int N, int K, int A, int vote, uint64_t head_seed,
                                   const void* recs, size_t stride, size_t offset, hipStream_t s);
hipError_t launch_update(const UpdateArgs& u, hipStream_t s);
hipError_t launch_gather(const GatherArgs& g, hipStream_t s, const int64_t* host_idx = nullptr);   // host_idx (B <= 256): indexes inside the kernel arguments
hipError_t launch_bn_forward(const BnArgs& b, hipStream_t s);      // [partial +] apply
hipError_t launch_bn_backward(const BnArgs& b, hipStream_t s);     // partial + apply
hipError_t launch_bn_update(const UpdateArgs& u, hipStream_t s);   // optimizer step of the [beta | gamma] block (g already holds the sums)
hipError_t launch_prep(const PrepArgs& p, hipStream_t s, double* zero8 = nullptr);   // zero8: an 8-byte accumulator the launch also clears
hipError_t launch_grad_to_half(const float* g, half_t* gh, int64_t n, int* state, hipStream_t s);       // fp16 DP payload; state = {flag, log2 scale, good steps}
hipError_t launch_grad_from_half(const half_t* gh, float* g, int64_t n, int* state, hipStream_t s);
// ---- the acting forward as ONE launch (sdqn_act.hip): float32, standard geometry, no batch-norm ---------------------------------------
constexpr int ACT_GRID = 256;                     // workgroups of 256 threads (one per CU when the chip is idle; any placement is correct)
constexpr int ACT_XCC_FLOATS = 21248 + 8 * 32 * 64;  // one XCC's scratch: a1 [400][32] | a2 [81][64] | a3 [49][64] (+ pad) | fc4 partials [8 stripes][32 chunks][64]
constexpr int ACT_KCH = 32;                       // fc4 K-chunks per stripe of 64 hidden units
constexpr int ACT_Q_STRIDE = 32;                  // the launch delivers 8 stripe partials of the Q-vector: q[stripe * 32 + action]; the host adds them in stripe order
constexpr int ACT_CTL_WORDS = 832;                // control block of one launch; 4 rotate (a launch clears the one after next)
constexpr int ACT_STAMPS = 40;                    // (timing build of the kernel: {kind, clock64} pairs per workgroup)
struct ActArgs {
  const uint8_t* state;       // [4][84*84] bytes, oldest frame first (the device state buffer's window)
  const float* theta;         // online parameters
  float* scratch;             // [8][ACT_XCC_FLOATS]
  unsigned* ctl;              // [4][ACT_CTL_WORDS], zero before the first launch
  float* q;                   // [8][ACT_Q_STRIDE] destination: stripe partials
  unsigned long long* stamps; // nullptr, or [ACT_GRID][2 * ACT_STAMPS] (tools/exp/act_stamps.py)
  int A;
  unsigned seq;               // launch number (selects the control block / partial slot)
};
hipError_t launch_act(const ActArgs& a, bool q_system_scope, hipStream_t s);
hipError_t launch_w1_planes(const float* theta, unsigned short* w1p, hipStream_t s);   // conv1's three bf16 weight planes of one net (problems.h: split_bf16x3)
hipError_t launch_refresh16(const float* theta, half_t* wh, half_t* wht, hipStream_t s);   // fp16 mode: rebuild both half copies
// ---- --target_tau: theta- <- theta- + tau (theta - theta-) and the target's derived weight copies, ONE launch (sdqn_target.hip) -------
struct TargetBlendArgs {
  const float* theta;         // online parameters (read only)
  float* theta_t;             // target parameters, blended in place
  int64_t NP;                 // values per flat buffer (weights [+ BatchNorm parameters and running statistics])
  float tau;
  half_t* wh; half_t* wht;    // float16 nets: the TARGET net's half copies (master layout / transposed), else nullptr
  unsigned short* w1p;        // float32 nets: the TARGET net's three bf16 planes of W1, else nullptr
  int tiles;                  // (filled in by launch_target_blend) leading workgroups that take a 64 x 32 tile each
  int64_t flat_first;         // (filled in by launch_target_blend) first element of the element-wise part
};
hipError_t launch_target_blend(TargetBlendArgs a, hipStream_t s);
// ---- --noisy_nets: factorised noise on fc4 and fc5 (sdqn_noisy.hip; the noise itself: noisy.h) ---------------------------------------------
struct NoisyArgs {              // noisy_compose: eff = [conv of mu | mu + sigma * (e_out * e_in) on fc4, fc5] for net slots 0 .. nets - 1
  const float* mu[2];           // flat parameters (theta, theta-)
  const float* sigma[2];        // [NP - OFF4] the fc4 | fc5 range, internal layout
  float* eff[2];                // [NP] effective flat buffers (what the step's kernels read as StepArgs::theta)
  float* eps;                   // [2][NOISY_EPS_NET] the factor vectors of the composed nets, left by workgroup 0 of each
  uint64_t seed, step;          // the counter: (seed, step, net slot, layer, side, index)
  int64_t NP;
  int A, nets;
};
struct NoisyTailArgs {          // noisy_tail: g_sigma = g * (e_out * e_in) on the fc range of g, then the optimizer rule on sigma
  const float* g;               // the flat gradient sums (update mode 1)
  float* sigma; float* state; float* state2;      // [n] the online net's sigma and its optimizer state (state2: Adam / Adadelta)
  const float* eps;             // [NOISY_EPS_NET] the online net's factor vectors of this step
  float* gsig;                  // nullptr, or [n]: g_sigma is kept (option keep_gradients)
  int64_t n;                    // NP - OFF4
  UpdateArgs u;                 // the optimizer's constants, bsz = the apply launch's divisor
};
hipError_t launch_noisy_compose(const NoisyArgs& a, hipStream_t s);
hipError_t launch_noisy_tail(const NoisyTailArgs& a, hipStream_t s);

}  // namespace sdqn

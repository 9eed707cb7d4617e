// step_trace — what the host orchestration of a step sends outward (sdqn_api_step.hip: run_train, predict_forward_tuned; sdqn_api_net.hip:
// sdqn_net_apply_update), printed one line per launch / event / all-reduce, in order, on the host and without a device.  Links the host-only
// objects of those two translation units (and of the ReDo / reset / regulariser / data-parallel ones where the tree has them as files of
// their own) and answers everything they call with the recording stubs below; whatever else they name stays
// unresolved and is never called.  Two trees orchestrate alike iff their outputs are equal: the acceptance check of a refactoring of the
// step's host side (tests/test_step_trace.py holds the tree to tests/golden/step_trace.txt).  Build and use: tools/step_trace.sh.
//   step_trace          the thinned grid (the golden): every launch structure and optimizer tail, the other axes off their default one at a
//                       time; every distinct line once, numbered, then each step as the numbers of its lines
//   step_trace --full   the whole cross product, every step written out (12 MB: compare two trees' outputs, or their checksums)
//   step_trace --quantiles   the steps of a --quantiles 6 net over 3 actions (18 outputs), every datatype-regime cell that has them, written
//                       out (neither golden holds them: tests/test_quantile.py reads the head's line)
//   step_trace --dueling     likewise the steps of a --dueling net over 3 actions (4 outputs), with apply_update's tail (tests/test_dueling.py)
//   step_trace --events      what follows an applied step — the regulariser, the blend of --target_tau, the ReDo and reset events, the derived
//                       copies each rebuilds — written out, then every refusal of the three features in both directions
//                       (tests/golden/step_trace_events.txt; needs sdqn_api_redo / _reset / _regularize / _dp, or whatever holds their code)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <utility>
#include "../simple_dqn_amd/csrc/api_internal.h"

// ---- named dummy addresses: distinct, non-null, never dereferenced ----------------------------------------------------------------------
static std::vector<std::pair<uintptr_t, const char*>> g_names;
static constexpr uintptr_t SPAN = 0x10000000u;
template <class T> static T* dummy(const char* name) { g_names.push_back({SPAN * (g_names.size() + 1), name}); return reinterpret_cast<T*>(g_names.back().first); }
static std::string nm(const void* p) {
  const uintptr_t v = (uintptr_t)p;
  if (!v) return "0";
  for (auto& e : g_names) if (v >= e.first && v < e.first + SPAN) {
    char buf[64]; if (v == e.first) return e.second;
    snprintf(buf, sizeof buf, "%s+%llu", e.second, (unsigned long long)(v - e.first)); return buf; }
  return "?";
}
template <class T> static void named(T*& p, const char* name) { p = dummy<T>(name); }
#define NAMED(field) named(field, &#field[3])     // ("h->theta" -> "theta")

// ---- the library-wide state the two translation units read --------------------------------------------------------------------------------
static FILE* g_out = stdout;
thread_local std::string g_err;
hipStream_t g_stream = (hipStream_t)0x1000, g_side = (hipStream_t)0x2000, g_comm = (hipStream_t)0x3000;
hipEvent_t g_ev[5];
int g_dev = 0;
std::vector<sdqn_replay_s*> g_replays;
__attribute__((weak)) Rccl g_rccl;      // (sdqn_api_dp.hip has the definition where --events links it)
static const char* sname(hipStream_t s) { return s == g_stream ? "main" : s == g_comm ? "comm" : s == g_side ? "side" : "?"; }
void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); fprintf(g_out, "  ERROR "); vfprintf(g_out, fmt, ap); fprintf(g_out, "\n"); va_end(ap); }

static const char* K_NAMES[K_COUNT] = {"conv1_fwd", "conv2_fwd", "conv3_fwd", "fc4_fwd", "head", "fc4_dgrad", "fc4_wgrad", "conv3_dgrad", "conv3_wgrad",
  "conv2_dgrad", "conv2_wgrad", "conv1_wgrad", "update", "allreduce", "gather", "prep", "bwd3", "bwd2", "bwd1", "bn", "-", "-", "-", "-", "wgrads", "act", "collect", "target"};
namespace sdqn {
const char* kernel_name(int id) { return (id >= 0 && id < K_COUNT) ? K_NAMES[id] : "?"; }
LaunchEvents& launch_events() { static LaunchEvents le; return le; }

// ---- recording stubs of the launchers --------------------------------------------------------------------------------------------------
static void step_fields(const StepArgs& a) {
  fprintf(g_out, " B=%d nz=%d bn=%d xcd=%d f4w=%d+%d frms=%d ring=%d a1=%s a2=%s a3=%s th=%s src=%s", a.B, a.nz, a.bn, a.xcd_map, a.f4w_first, a.f4w_count, a.fuse_rms,
         a.from_ring, nm(a.a1).c_str(), nm(a.a2).c_str(), nm(a.a3).c_str(), nm(a.theta[0]).c_str(), nm(a.src).c_str());
}
hipError_t launch_kernel(int id, const StepArgs& a, const LaunchTune& t, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s", sname(s), id, kernel_name(id)); step_fields(a);
  fprintf(g_out, " v=%d hidx=%d\n", t.variant, t.host_idx != nullptr);
  return hipSuccess;
}
hipError_t launch_head(const StepArgs& a, const HeadArgs& h, hipStream_t s, bool q_system_scope, const BootArgs*, const QuantArgs*, const DuelArgs*) {
  fprintf(g_out, "  %s %2d %-11s", sname(s), K_HEAD, "head"); step_fields(a);
  fprintf(g_out, " train=%d nstep=%d q=%s sys=%d\n", h.train, h.nstep, nm(h.q).c_str(), (int)q_system_scope);
  return hipSuccess;
}
static void update_fields(const char* what, int id, const UpdateArgs& u, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s mode=%d bsz=%g skip_fc4=%d only_fc4=%d next.B=%d ovf=%d dyn=%d opt=%d\n", sname(s), id, what, u.mode, (double)u.bsz, u.skip_fc4, u.only_fc4, u.next.B,
         u.ovf_flag != nullptr, u.ovf_dynamic, u.opt);
}
hipError_t launch_update(const UpdateArgs& u, hipStream_t s) { update_fields("update", K_UPDATE, u, s); return hipSuccess; }
hipError_t launch_bn_update(const UpdateArgs& u, hipStream_t s) { update_fields("bn_update", K_BN, u, s); return hipSuccess; }
static hipError_t bn_line(const char* what, const BnArgs& b, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s layer=%d train=%d nz=%d B=%d x=%s a=%s\n", sname(s), K_BN, what, b.layer, b.train, b.nz, b.B, nm(b.x).c_str(), nm(b.a).c_str());
  return hipSuccess;
}
hipError_t launch_bn_forward(const BnArgs& b, hipStream_t s) { return bn_line("bn_fwd", b, s); }
hipError_t launch_bn_backward(const BnArgs& b, hipStream_t s) { return bn_line("bn_bwd", b, s); }
hipError_t launch_grad_to_half(const float* g, half_t* gh, int64_t n, int* state, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s g=%s gh=%s n=%lld state=%s\n", sname(s), K_UPDATE, "to_half", nm(g).c_str(), nm(gh).c_str(), (long long)n, nm(state).c_str()); return hipSuccess;
}
hipError_t launch_grad_from_half(const half_t* gh, float* g, int64_t n, int* state, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s g=%s gh=%s n=%lld state=%s\n", sname(s), K_UPDATE, "from_half", nm(g).c_str(), nm(gh).c_str(), (long long)n, nm(state).c_str()); return hipSuccess;
}
template <> hipError_t launch_grad_sqnorm<float>(const float* g, int64_t n, double* part, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s g=%s n=%lld part=%s\n", sname(s), K_UPDATE, "clip_sqnorm", nm(g).c_str(), (long long)n, nm(part).c_str()); return hipSuccess;
}
template <> hipError_t launch_grad_scale<float>(float* g, int64_t n, const double* part, double bsz, double max_norm, double* rec, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s g=%s n=%lld bsz=%g max_norm=%g rec=%s\n", sname(s), K_UPDATE, "clip_scale", nm(g).c_str(), (long long)n, bsz, max_norm, nm(rec).c_str()); return hipSuccess;
}
hipError_t launch_dueling_mask(void* w5, bool f64, int rows, int H, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s w5=%s f64=%d rows=%d H=%d\n", sname(s), K_UPDATE, "duel_mask", nm(w5).c_str(), (int)f64, rows, H); return hipSuccess;
}
hipError_t launch_noisy_compose(const NoisyArgs& a, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s eff=%s step=%llu nets=%d\n", sname(s), K_UPDATE, "nz_compose", nm(a.eff[0]).c_str(), (unsigned long long)a.step, a.nets); return hipSuccess;
}
hipError_t launch_noisy_tail(const NoisyTailArgs& a, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s g=%s sigma=%s bsz=%g opt=%d keep=%d\n", sname(s), K_UPDATE, "nz_sigma", nm(a.g).c_str(), nm(a.sigma).c_str(), (double)a.u.bsz, a.u.opt, a.gsig != nullptr); return hipSuccess;
}
hipError_t launch_target_blend(TargetBlendArgs a, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s tau=%g\n", sname(s), K_TARGET, "blend", (double)a.tau); return hipSuccess;
}
// (--events) the launches behind an applied step
hipError_t launch_redo_scores(const RedoScoreArgs& a, int stage, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s stage=%d a=%s,%s,%s,%s half123=%d B=%d partial=%s scores=%s\n", sname(s), K_UPDATE, "redo_scores", stage, nm(a.a[0]).c_str(), nm(a.a[1]).c_str(),
         nm(a.a[2]).c_str(), nm(a.a[3]).c_str(), a.half123, a.B, nm(a.partial).c_str(), nm(a.scores).c_str()); return hipSuccess;
}
hipError_t launch_redo_apply(const RedoApplyArgs& a, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s scores=%s theta=%s state=%s state2=%s n=%lld tau=%g seed=%llu event=%llu step=%lld info=%s\n", sname(s), K_UPDATE, "redo_apply", nm(a.scores).c_str(),
         nm(a.theta).c_str(), nm(a.state).c_str(), nm(a.state2).c_str(), (long long)a.n, a.tau, (unsigned long long)a.seed, (unsigned long long)a.event, (long long)a.step, nm(a.info).c_str());
  return hipSuccess;
}
hipError_t launch_reset_apply(const ResetApplyArgs& a, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s theta=%s theta_t=%s state=%s state2=%s n=%lld layers=%d alpha=%g seed=%llu event=%llu step=%lld info=%s\n", sname(s), K_UPDATE, "reset_apply",
         nm(a.theta).c_str(), nm(a.theta_t).c_str(), nm(a.state).c_str(), nm(a.state2).c_str(), (long long)a.n, a.layers, a.alpha, (unsigned long long)a.seed, (unsigned long long)a.event,
         (long long)a.step, nm(a.info).c_str());
  return hipSuccess;
}
hipError_t launch_regularize(RegularizeArgs a, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s theta=%s anchor=%s n=%lld kf=%.9g cf=%.9g wd_on=%d l2_on=%d wh=%s wht=%s w1p=%s | theta_t=%s tau=%g wh_t=%s wht_t=%s w1p_t=%s\n", sname(s), K_UPDATE,
         "regularize", nm(a.theta).c_str(), nm(a.anchor).c_str(), (long long)a.n, (double)a.rule.kf, (double)a.rule.cf, (int)a.rule.wd_on, (int)a.rule.l2_on, nm(a.wh).c_str(),
         nm(a.wht).c_str(), nm(a.w1p).c_str(), nm(a.theta_t).c_str(), (double)a.tau, nm(a.wh_t).c_str(), nm(a.wht_t).c_str(), nm(a.w1p_t).c_str());
  return hipSuccess;
}
hipError_t launch_refresh16(const float* theta, half_t* wh, half_t* wht, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s theta=%s wh=%s wht=%s\n", sname(s), K_UPDATE, "refresh16", nm(theta).c_str(), nm(wh).c_str(), nm(wht).c_str()); return hipSuccess;
}
hipError_t launch_w1_planes(const float* theta, unsigned short* w1p, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s theta=%s w1p=%s\n", sname(s), K_UPDATE, "w1_planes", nm(theta).c_str(), nm(w1p).c_str()); return hipSuccess;
}
}  // namespace sdqn

// ---- the HIP runtime entry points the orchestration uses, and the collective library ----------------------------------------------------
static sdqn_net_s* g_h;
static const char* ename(hipEvent_t e) { return g_h && e == g_h->ev_g4 ? "ev_g4" : g_h && e == g_h->ev_w4 ? "ev_w4" : "?"; }
extern "C" {
hipError_t hipGetLastError() { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "hip error"; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { fprintf(g_out, "  %s    record      %s\n", sname(s), ename(e)); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { fprintf(g_out, "  %s    wait        %s\n", sname(s), ename(e)); return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t s) {
  fprintf(g_out, "  %s    copy        dst=%s src=%s bytes=%zu kind=%d\n", sname(s), nm(dst).c_str(), nm(src).c_str(), n, (int)kind); return hipSuccess;
}
// (--events) dalloc's two calls: a named dummy, one line each
static const char* const ALLOC_NAMES[] = {"alloc1", "alloc2", "alloc3", "alloc4", "alloc5", "alloc6", "alloc7", "alloc8"};
static int g_allocs = 0;
hipError_t hipMalloc(void** p, size_t bytes) {
  *p = dummy<char>(ALLOC_NAMES[g_allocs < 8 ? g_allocs : 7]); ++g_allocs;
  fprintf(g_out, "  -       malloc      %s bytes=%zu\n", nm(*p).c_str(), bytes); return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t s) {
  fprintf(g_out, "  %s    memset      dst=%s value=%d bytes=%zu\n", sname(s), nm(dst).c_str(), value, bytes); return hipSuccess;
}
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
}
static int ar_stub(const void* in, void* out, size_t count, int dtype, int op, void* comm, hipStream_t s) {
  fprintf(g_out, "  %s %2d %-11s buf=%s count=%zu dtype=%d op=%d comm=%s%s\n", sname(s), K_ALLREDUCE, "allreduce", nm(out).c_str(), count, dtype, op, nm(comm).c_str(), in == out ? "" : " NOT-IN-PLACE");
  return 0;
}
static int group_start() { fprintf(g_out, "  -       group_start\n"); return 0; }
static int group_end() { fprintf(g_out, "  -       group_end\n"); return 0; }

// ---- one configuration --------------------------------------------------------------------------------------------------------------------
enum Dp { DP_NONE, DP_SERIAL, DP_SERIAL_F32, DP_OVERLAP, DP_GRAD_ONLY, DP_COUNT };
static const char* DP_NAMES[] = {"none", "serial", "serial_f32payload", "overlap", "grad_only"};
enum Tgt { T_STD, T_DDQN, T_MUNCH };
static const char* T_NAMES[] = {"standard", "double_dqn", "munchausen"};
enum Opt { O_NONE, O_BT_XCD0, O_C1W0, O_C1W2, O_C1WIN0, O_C1WIN2, O_F4_SHARE, O_TUPLE, O_COUNT };     // one option off its default
static const char* O_NAMES[] = {"", " bt_xcd=0", " conv1w_bf16=0", " conv1w_bf16=2", " c1w_in_wgrads=0", " c1w_in_wgrads=2", " f4_share=60,30", " tuple"};
struct Cfg { int B, dt, fused, dp, clip, tgt, next, adam, keep, opt; };      // dt: 0 float32, 1 float32 + batch_norm, 2 float16

static int g_quantiles = 1;      // --quantiles: every net is a quantile net over 18 / g_quantiles actions
static bool g_dueling = false;   // --dueling: every net is a dueling net over 3 actions
static bool refused(const Cfg& c) {
  if (g_dueling && (c.dt == 1 || c.tgt != T_STD)) return true;            // sdqn_net_set_dueling refuses batch_norm, double_dqn and munchausen
  if (g_quantiles > 1 && (c.dt == 1 || c.tgt != T_STD)) return true;      // sdqn_net_set_quantiles refuses batch_norm, double_dqn and munchausen
  if (c.dp == DP_SERIAL_F32 && c.dt != 2) return true;     // dp_half is a float16 option
  if (c.tgt == T_MUNCH && c.dt == 1) return true;          // sdqn_net_set_munchausen refuses batch_norm
  return false;
}
static void fill(sdqn_net_s* h, const Cfg& c) {
  g_names.clear(); g_allocs = 0;
  memset(&h->cfg, 0, sizeof h->cfg);
  h->cfg.batch_size = c.B; h->cfg.num_actions = 4; h->cfg.target_enabled = 1; h->cfg.optimizer = c.adam; h->cfg.datatype = c.dt == 2;
  h->cfg.discount_rate = 0.99; h->cfg.clip_error = 1.0; h->cfg.min_reward = -1.0; h->cfg.max_reward = 1.0; h->cfg.learning_rate = 0.00025;
  h->cfg.decay_rate = 0.95; h->cfg.epsilon = 1e-6; h->cfg.beta_1 = 0.9; h->cfg.beta_2 = 0.999; h->cfg.loss_scale = 128.0;
  h->B = c.B; h->A = 4; h->bn = c.dt == 1; h->NPW = OFF5 + (int64_t)h->A * NFC; h->NP = h->NPW + (h->bn ? 2 * BN_PARAMS : 0);
  h->tps1 = c.B >= 128 ? ((c.dt == 1) ? 50 : 10) : 5; h->tps2 = 8; h->tps3 = 7; h->S4 = (c.B >= 128 && c.dt != 2) ? 1 : 7;
  NAMED(h->theta); NAMED(h->theta_t); NAMED(h->state); NAMED(h->state2); NAMED(h->g); NAMED(h->a1); NAMED(h->a2); NAMED(h->a3); NAMED(h->slab4);
  NAMED(h->a4); NAMED(h->d4); NAMED(h->d3p); NAMED(h->d2p); NAMED(h->d1); NAMED(h->d3); NAMED(h->d2); NAMED(h->slab1); NAMED(h->slab2); NAMED(h->slab3);
  NAMED(h->q); NAMED(h->maxq); NAMED(h->dq); NAMED(h->cost_terms); NAMED(h->cost_out); NAMED(h->cost_accum); NAMED(h->st_states); NAMED(h->st_act);
  NAMED(h->st_term); NAMED(h->st_rew); NAMED(h->d_idx); NAMED(h->w1p[0]); NAMED(h->w1p[1]); NAMED(h->clip_buf);
  if (h->bn) { NAMED(h->x1); NAMED(h->x2); NAMED(h->x3); NAMED(h->bn_mean); NAMED(h->bn_rstd); NAMED(h->bn_partial); }
  if (c.dt == 2) {
    NAMED(h->h_a1); NAMED(h->h_a2); NAMED(h->h_a3); NAMED(h->h_d4); NAMED(h->h_d3p); NAMED(h->h_d3); NAMED(h->h_d2p); NAMED(h->h_d2); NAMED(h->h_d1);
    NAMED(h->wh[0]); NAMED(h->wh[1]); NAMED(h->wht[0]); NAMED(h->wht[1]); NAMED(h->gh); NAMED(h->ovf_flag); NAMED(h->ovf_count);
  }
  if (g_quantiles > 1) { h->cfg.num_actions = h->A = MAX_ACTIONS; h->opt.quant_N = g_quantiles; h->NPW = OFF5 + (int64_t)h->A * NFC; h->NP = h->NPW; }
  if (g_dueling) h->opt.dueling = true;                                         // (A = 4: V and three advantages)
  h->ev_g4 = (hipEvent_t)0x4000; h->ev_w4 = (hipEvent_t)0x5000;
  h->fused_launches = c.fused != 0; h->keep_grads = c.keep != 0; h->target_tau = 0.01;      // (every applied step ends with its blend line)
  if (c.clip) h->clip_grad_norm = 10.0;
  if (c.tgt == T_DDQN) h->opt.double_dqn = h->slots3 = true;
  if (c.tgt == T_MUNCH) h->opt.munchausen = h->slots3 = true;
  if (c.dp == DP_GRAD_ONLY) h->grad_only = true;
  if (c.dp == DP_SERIAL || c.dp == DP_SERIAL_F32 || c.dp == DP_OVERLAP) { NAMED(h->comm); h->nranks = 2; h->rank = 1; }
  if (c.dp == DP_SERIAL_F32) h->dp_half = 0;
  if (c.dp == DP_OVERLAP) { NAMED(h->comm2); h->dp_overlap = true; }
  switch (c.opt) {
    case O_BT_XCD0: h->bt_xcd = false; break;
    case O_C1W0: h->conv1w_bf16 = 0; break;
    case O_C1W2: h->conv1w_bf16 = 2; break;
    case O_C1WIN0: h->c1w_in_wgrads = 0; break;
    case O_C1WIN2: h->c1w_in_wgrads = 2; break;
    case O_F4_SHARE: h->f4_share[0] = 60; h->f4_share[1] = 30; break;
    default: break;
  }
}
static void header(const char* what, const Cfg& c) {
  fprintf(g_out, "%s B=%d %s fused=%d dp=%s clip=%d target=%s next=%d opt=%s keep_grads=%d%s\n", what, c.B, c.dt == 0 ? "float32" : c.dt == 1 ? "float32+bn" : "float16",
         c.fused, DP_NAMES[c.dp], c.clip, T_NAMES[c.tgt], c.next, c.adam ? "adam" : "rmsprop", c.keep, O_NAMES[c.opt]);
}
static void footer(int rc, const sdqn_net_s* h) {
  fprintf(g_out, "  -> rc=%d train_iterations=%lld spec_pending=%d clip_ran=%d w4_pending=%d half_payload_pending=%d\n", rc, (long long)h->train_iterations, (int)h->spec_pending,
         (int)h->clip_ran, (int)h->w4_pending, (int)h->half_payload_pending);
}
static int64_t g_host_idx[512];

static void train(const Cfg& c) {
  if (refused(c)) return;
  sdqn_net_s* h = new sdqn_net_s(); g_h = h;
  fill(h, c);
  header("train", c);
  h->spec_pending = true;
  StepArgs a = step_args(h);
  if (c.opt == O_TUPLE) { a.from_ring = 0; a.src = h->st_states; }
  else { a.from_ring = 1; a.src = dummy<const uint8_t>("ring"); a.idx = h->d_idx; h->host_idx_cur = g_host_idx; }
  PrepArgs next; memset(&next, 0, sizeof next); next.B = c.B;
  footer(run_train(h, a, head_args(h, HEAD_TRAIN), c.next ? &next : nullptr), h);
  delete h; g_h = nullptr;
}
static void predict(const Cfg& c, int B1) {
  sdqn_net_s* h = new sdqn_net_s(); g_h = h;
  fill(h, c);
  header(B1 ? "predict_one" : "predict", c);
  h->w4_pending = c.dp == DP_OVERLAP;        // (the previous step's fc4 update may still be running)
  footer(predict_forward_tuned(h, h->st_states, head_args(h, HEAD_PREDICT), B1), h);
  delete h; g_h = nullptr;
}
static void apply(const Cfg& c, bool half_pending) {
  sdqn_net_s* h = new sdqn_net_s(); g_h = h;
  fill(h, c);
  header(half_pending ? "apply_update(half payload)" : "apply_update", c);
  h->spec_pending = true; h->half_payload_pending = half_pending;
  footer(sdqn_net_apply_update(h, 2.0 * c.B), h);
  delete h; g_h = nullptr;
}

// The thinned grid.  Steps: every (datatype, batch regime, fused, data-parallel form) with the other axes at their defaults (B = 33 and the
// unfused structure where they can differ from B = 32 / fused), then one axis at a time on the fused structure.
static bool thin_train(const Cfg& c) {
  const int off = c.clip + (c.tgt != T_STD) + c.next + c.adam + c.keep;
  const bool b2 = c.B == 32 || c.B == 128;
  if (off == 0) return c.fused ? (b2 || (c.B == 33 && c.dp == DP_NONE)) : (b2 && c.dp <= DP_SERIAL);
  if (!b2 || !c.fused || c.dp == DP_SERIAL_F32) return false;
  if (off == 2) return c.clip && c.next && c.dp == DP_NONE && c.dt == 0 && c.B == 32;
  if (off != 1) return false;
  if (c.clip) return true;                               // in every form (the overlapped one steps back to the serial form)
  if (c.next) return c.B == 32 ? c.dt == 0 : (c.dt == 2 && c.dp == DP_SERIAL);
  return c.dp == DP_NONE && (c.tgt != T_STD || c.keep || c.B == 32);
}
// ... options: where the option reaches, without data parallel
static bool thin_option(const Cfg& c) {
  if (c.dp != DP_NONE || (c.B != 32 && c.B != 128)) return false;
  switch (c.opt) {
    case O_BT_XCD0: return c.tgt == T_STD;
    case O_C1W0: case O_C1W2: return c.tgt == T_STD && c.dt == 0;
    case O_C1WIN0: case O_C1WIN2: return c.tgt == T_STD && c.dt == 2 && c.B == 128;
    case O_F4_SHARE: return c.tgt == T_STD && c.B == 32;
    default: return c.B == 32 && (c.tgt == T_STD || c.dt == 1);      // tuple: the staged minibatch, and the poststates of the forward in front of a batch_norm step
  }
}
// The thinned output names every distinct line once and writes a step as the numbers of its lines: the grid repeats a few hundred lines
static void print_thin(char* text) {
  std::vector<std::string> lines; std::string steps;
  for (char* l = strtok(text, "\n"); l; l = strtok(nullptr, "\n")) {
    if (l[0] != ' ') { steps += steps.empty() ? "" : "\n"; steps += l; steps += " :"; continue; }
    size_t i = 0; while (i < lines.size() && lines[i] != l) ++i;
    if (i == lines.size()) lines.push_back(l);
    steps += " " + std::to_string(i + 1);
  }
  printf("== lines\n");
  for (size_t i = 0; i < lines.size(); ++i) printf("%3zu%s\n", i + 1, lines[i].c_str());
  printf("== steps: the lines each sends out, in order\n%s\n", steps.c_str());
}

// ---- --events: what follows an applied step, and the refusals of the three features that move the weights there ---------------------------
// reg: 0 off | 1 weight_decay | 2 weight_decay and l2_init; redo / reset: the interval (0: off); iters: train_iterations in front of the step
struct Ev { int dt, B, target, dueling, dp, reg; double tau; int redo, reset, layers; double alpha; int64_t iters; };
static void fill_events(sdqn_net_s* h, const Ev& e) {
  fill(h, Cfg{e.B, e.dt, 1, e.dp == DP_OVERLAP ? DP_NONE : e.dp, 0, T_STD, 0, 0, 0, O_NONE});
  NAMED(h->state2);
  if (e.dt == 2) h->w1p[0] = h->w1p[1] = nullptr;                             // (as sdqn_net_create leaves a float16 net)
  if (!e.target) { h->cfg.target_enabled = 0; h->theta_t = h->theta; h->w1p[1] = h->w1p[0]; h->wh[1] = h->wh[0]; h->wht[1] = h->wht[0]; }
  h->opt.dueling = e.dueling != 0;
  if (e.dp == DP_OVERLAP) { NAMED(h->comm); NAMED(h->comm2); h->nranks = 1; h->rank = 0; h->dp_overlap = true; }      // one rank, the overlapped form
  h->target_tau = e.tau;
  if (e.reg) { h->reg_wd = 0.1; if (e.reg == 2) { h->reg_lambda = 0.01; NAMED(h->reg_anchor); } }
  h->redo_interval = e.redo; h->redo_tau = 0.1; h->redo_seed = 7;
  h->reset_interval = e.reset; h->reset_layers = e.layers; h->reset_alpha = e.alpha; h->reset_seed = 9;
  h->train_iterations = e.iters;
}
static void header_events(const char* what, const Ev& e) {
  fprintf(g_out, "%s B=%d %s target_net=%d dueling=%d dp=%s weight_decay=%g l2_init=%g target_tau=%g redo_interval=%d reset_interval=%d reset_layers=%d shrink_perturb=%g train_iterations=%lld\n",
          what, e.B, e.dt == 0 ? "float32" : "float16", e.target, e.dueling, DP_NAMES[e.dp], e.reg ? 0.1 : 0.0, e.reg == 2 ? 0.01 : 0.0, e.tau, e.redo, e.reset, e.layers, e.alpha,
          (long long)e.iters);
}
static void footer_events(int rc, const sdqn_net_s* h) {
  footer(rc, h);
  fprintf(g_out, "  -> redo_events=%lld reset_events=%lld redo_acts_live=%d nz_stale=%d\n", (long long)h->redo_events, (long long)h->reset_events, (int)h->redo_acts_live, (int)h->nz_stale);
}
static void train_events(const Ev& e) {
  sdqn_net_s* h = new sdqn_net_s(); g_h = h;
  fill_events(h, e);
  header_events("train", e);
  h->spec_pending = true;
  StepArgs a = step_args(h);
  a.from_ring = 1; a.src = dummy<const uint8_t>("ring"); a.idx = h->d_idx; h->host_idx_cur = g_host_idx;
  footer_events(run_train(h, a, head_args(h, HEAD_TRAIN), nullptr), h);
  delete h; g_h = nullptr;
}
static void apply_events(const Ev& e) {
  sdqn_net_s* h = new sdqn_net_s(); g_h = h;
  fill_events(h, e);
  header_events("apply_update", e);
  h->spec_pending = true;
  footer_events(sdqn_net_apply_update(h, 2.0 * e.B), h);
  delete h; g_h = nullptr;
}
// the features, alone and together; (interval 3, train_iterations 2): due at this step, (3, 3): not due.  reset_first: (layers 2, alpha 1) fc4,
// between conv2's and fc5's offsets; (1, 1) fc5's; (4, 1) conv2's exactly; (5, .) and alpha < 1: 0
static Ev feature(int f, int dt, int B, int target, int dueling, int dp) {
  Ev e{dt, B, target, dueling, dp, 0, 0.0, 0, 0, 2, 1.0, 2};
  switch (f) {
    case 0: e.reg = 1; break;
    case 1: e.reg = 2; break;
    case 2: e.tau = 0.01; break;
    case 3: e.tau = 1.0; break;
    case 4: e.reg = 2; e.tau = 0.01; break;
    case 5: e.reg = 2; e.tau = 1.0; break;
    case 6: e.redo = 3; break;
    case 7: e.redo = 3; e.iters = 3; break;
    case 8: e.reset = 3; break;
    case 9: e.reset = 3; e.iters = 3; break;
    case 10: e.reset = 3; e.layers = 1; break;
    case 11: e.reset = 3; e.layers = 5; break;
    case 12: e.reset = 3; e.layers = 4; break;
    case 13: e.reset = 3; e.layers = 1; e.alpha = 0.5; break;
    case 14: e.reg = 2; e.tau = 0.01; e.redo = 1; e.reset = 1; break;
    case 15: e.reg = 2; e.tau = 0.01; e.redo = 3; e.reset = 3; e.iters = 3; break;
    default: e.reg = 2; e.tau = 1.0; e.redo = 1; e.reset = 1; break;
  }
  return e;
}
constexpr int EVENT_CASES = 17;
// a refusal: the call's words (set_error's stub has printed them) and its return value
enum Bad { BAD_GEN, BAD_BN, BAD_NOISY, BAD_RANKS, BAD_COUNT };
static const char* BAD_NAMES[] = {"the generic path", "batch_norm", "noisy_nets", "two ranks"};
static sdqn_net_s* plain_handle() {
  sdqn_net_s* h = new sdqn_net_s(); g_h = h;
  fill_events(h, Ev{0, 32, 1, 0, DP_NONE, 0, 0.0, 0, 0, 2, 1.0, 2});
  h->redo_acts_live = true;
  return h;
}
static sdqn_net_s* bad_handle(int bad) {
  sdqn_net_s* h = plain_handle();
  if (bad == BAD_GEN) h->gen = reinterpret_cast<decltype(h->gen)>(SPAN / 2);      // (asked for, never dereferenced)
  if (bad == BAD_BN) h->bn = true;
  if (bad == BAD_NOISY) h->noisy = true;
  if (bad == BAD_RANKS) { NAMED(h->comm); h->nranks = 2; }
  return h;
}
static void drop(sdqn_net_s* h) { h->gen = nullptr; delete h; g_h = nullptr; }
#define CALL(h, expr) do { fprintf(g_out, "%s\n", #expr); const int rc_ = (expr); fprintf(g_out, "  -> rc=%d redo_interval=%d reset_interval=%d weight_decay=%g l2_init=%g noisy=%d comm=%s\n", rc_, \
  (h)->redo_interval, (h)->reset_interval, (h)->reg_wd, (h)->reg_lambda, (int)(h)->noisy, nm((h)->comm).c_str()); } while (0)
static void refusals() {
  static float fbuf[2048]; static double dbuf[16]; static char id[128];
  for (int bad = 0; bad < BAD_COUNT; ++bad) {
    fprintf(g_out, "== on a handle with %s\n", BAD_NAMES[bad]);
    sdqn_net_s* h = bad_handle(bad);
    CALL(h, sdqn_net_set_redo(h, 5, 0.1, 7));
    CALL(h, sdqn_net_redo_now(h));
    CALL(h, sdqn_net_redo_scores(h, fbuf));
    CALL(h, sdqn_net_set_reset(h, 5, 2, 1.0, 9));
    CALL(h, sdqn_net_reset_now(h));
    CALL(h, sdqn_net_set_regularizer(h, 0.1, 0.0));
    CALL(h, sdqn_net_set_regularizer(h, 0.0, 0.01));
    CALL(h, sdqn_net_regularize_now(h));
    CALL(h, sdqn_net_regularize_with(h, 0.1, 0.01));
    CALL(h, sdqn_net_anchor_now(h));
    CALL(h, sdqn_net_get_anchor(h, 0, fbuf, 2048));
    CALL(h, sdqn_net_weight_norms(h, dbuf));
    drop(h);
  }
  for (int f = 0; f < 5; ++f) {
    static const char* ON[] = {"redo_interval 5", "reset_interval 5", "weight_decay 0.1", "l2_init 0.01", "weight_decay 0.1 and l2_init 0.01"};
    fprintf(g_out, "== on a handle with %s\n", ON[f]);
    for (int call = 0; call < 2; ++call) {
      sdqn_net_s* h = plain_handle();
      if (f == 0) h->redo_interval = 5;
      if (f == 1) h->reset_interval = 5;
      if (f == 2 || f == 4) h->reg_wd = 0.1;
      if (f == 3 || f == 4) h->reg_lambda = 0.01;
      if (call == 0) CALL(h, sdqn_net_set_noisy(h, 1, 0.5, 0));
      else CALL(h, sdqn_dp_init(h, nullptr, id, 0, 2));
      drop(h);
    }
  }
  // and what the setters do where nothing refuses them (dalloc's lines, the anchor's copy)
  fprintf(g_out, "== on a plain handle\n");
  sdqn_net_s* h = plain_handle();
  CALL(h, sdqn_net_set_redo(h, 5, 0.1, 7));
  CALL(h, sdqn_net_set_reset(h, 5, 2, 1.0, 9));
  CALL(h, sdqn_net_set_regularizer(h, 0.1, 0.01));
  CALL(h, sdqn_net_anchor_now(h));
  CALL(h, sdqn_net_regularize_now(h));
  CALL(h, sdqn_net_regularize_with(h, 0.0, 0.0));
  h->train_iterations = 4;
  CALL(h, sdqn_net_redo_now(h));
  CALL(h, sdqn_net_reset_now(h));
  CALL(h, sdqn_net_set_reset(h, 0, 0, 1.0, 9));
  CALL(h, sdqn_net_reset_now(h));
  drop(h);
}
static void events() {
  for (int dt : {0, 2}) for (int B : {32, 128}) for (int f = 0; f < EVENT_CASES; ++f)
    if (B == 32 || f == 4 || f == 6 || f == 8 || f == 14 || f == 16) train_events(feature(f, dt, B, 1, 0, DP_NONE));
  for (int dt : {0, 2}) for (int shape = 1; shape < 4; ++shape) for (int f : {4, 6, 8, 10, 11, 14, 16}) train_events(feature(f, dt, 32, !(shape & 1), shape >> 1, DP_NONE));
  for (int dt : {0, 2}) train_events(feature(14, dt, 32, 1, 1, DP_GRAD_ONLY));           // a grad_only step applies nothing: nothing follows it
  for (int f : {1, 4, 6, 8, 14}) train_events(feature(f, 0, 32, 1, 0, DP_OVERLAP));      // join_comm in front of each event
  train_events(feature(14, 2, 32, 1, 1, DP_OVERLAP));
  for (int dt : {0, 2}) for (int shape = 0; shape < 4; ++shape) for (int f : {0, 2, 3, 4, 5, 6, 8, 14, 16}) apply_events(feature(f, dt, 32, !(shape & 1), shape >> 1, DP_GRAD_ONLY));
  refusals();
}

int main(int argc, char** argv) {
  setvbuf(stdout, nullptr, _IOFBF, 1 << 20);
  const bool full = argc > 1 && !strcmp(argv[1], "--full");
  char* text = nullptr; size_t text_len = 0;
  const bool quantiles = argc > 1 && !strcmp(argv[1], "--quantiles");
  if (!full && !quantiles && !(argc > 1 && (!strcmp(argv[1], "--dueling") || !strcmp(argv[1], "--events")))) g_out = open_memstream(&text, &text_len);
  g_rccl.AllReduce = ar_stub; g_rccl.GroupStart = group_start; g_rccl.GroupEnd = group_end;
  for (int i = 0; i < 512; ++i) g_host_idx[i] = 1000 + 37 * i;
  if (quantiles) {
    g_quantiles = 6;
    for (int dt : {0, 2}) for (int B : {32, 128}) for (int clip = 0; clip < 2; ++clip) train(Cfg{B, dt, 1, DP_NONE, clip, T_STD, 0, 0, 0, O_NONE});
    train(Cfg{32, 0, 1, DP_SERIAL, 0, T_STD, 0, 0, 0, O_NONE});
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "--events")) { events(); return 0; }
  if (argc > 1 && !strcmp(argv[1], "--dueling")) {
    g_dueling = true;
    for (int dt : {0, 2}) for (int B : {32, 128}) for (int clip = 0; clip < 2; ++clip) train(Cfg{B, dt, 1, DP_NONE, clip, T_STD, 0, 0, 0, O_NONE});
    for (int dp : {DP_SERIAL, DP_OVERLAP, DP_GRAD_ONLY}) train(Cfg{32, 0, 1, dp, 0, T_STD, 0, 0, 0, O_NONE});
    train(Cfg{32, 2, 1, DP_SERIAL, 0, T_STD, 0, 0, 0, O_NONE});
    apply(Cfg{32, 0, 1, DP_GRAD_ONLY, 0, T_STD, 0, 0, 0, O_NONE}, false);
    apply(Cfg{32, 0, 1, DP_GRAD_ONLY, 1, T_STD, 0, 0, 0, O_NONE}, false);
    return 0;
  }
  static const int BS[] = {32, 33, 127, 128, 256};
  for (int dt = 0; dt < 3; ++dt) for (int B : BS) for (int fused = 1; fused >= 0; --fused) for (int dp = 0; dp < DP_COUNT; ++dp) for (int clip = 0; clip < 2; ++clip)
    for (int tgt = 0; tgt < 3; ++tgt) for (int next = 0; next < 2; ++next) for (int adam = 0; adam < 2; ++adam) for (int keep = 0; keep < 2; ++keep) {
      const Cfg c{B, dt, fused, dp, clip, tgt, next, adam, keep, O_NONE};
      if (full || thin_train(c)) train(c);
    }
  // options, each off its default alone: over datatype x batch regime x the forms whose backward differs
  for (int opt = 1; opt < O_COUNT; ++opt) for (int dt = 0; dt < 3; ++dt) for (int B : BS) for (int dp : {DP_NONE, DP_OVERLAP}) for (int tgt : {T_STD, T_DDQN}) {
    const Cfg c{B, dt, 1, dp, 0, tgt, 0, 0, 0, opt};
    if (full ? (opt == O_TUPLE || tgt == T_STD) : thin_option(c)) train(c);
  }
  for (int dt = 0; dt < 3; ++dt) for (int B : {32, 128}) for (int dp : {DP_NONE, DP_OVERLAP}) {
    const Cfg c{B, dt, 1, dp, 0, T_STD, 0, 0, 0, O_NONE};
    if (full || dp == DP_NONE || (dt == 0 && B == 32)) predict(c, 0);
    if (full || (dp == DP_NONE && B == 32)) predict(c, 1);
  }
  for (int dt = 0; dt < 3; ++dt) for (int B : {32, 128}) for (int clip = 0; clip < 2; ++clip) for (int adam = 0; adam < 2; ++adam) {
    const Cfg c{B, dt, 1, DP_GRAD_ONLY, clip, T_STD, 0, adam, 0, O_NONE};
    if (full || (B == 32 && (!adam || (dt == 0 && !clip)))) apply(c, false);
    if (dt == 2 && (full || (B == 32 && !adam))) apply(c, true);
  }
  if (!full) { fclose(g_out); print_thin(text); free(text); }
  return 0;
}

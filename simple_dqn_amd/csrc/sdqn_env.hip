// sdqn_env.hip — the device-resident game "catch" (env_catch.h): host entry points of the environment handle, the render
// kernel of the fused act step (sdqn_net_act_step_env) and the vectorised on-device evaluation loop (sdqn_env_eval).  The kernels of this
// feature live here only: the train step's translation units are untouched.
#include "api_internal.h"
#include "env_catch.h"

struct sdqn_env_s {
  CatchState s;
  int H = 0, W = 0, bpe = 10;
  std::vector<uint8_t> frame;              // the host-rendered frame of `s` (valid while frame_ok)
  bool frame_ok = false;
};
static_assert(sizeof(sdqn_env_state) == sizeof(CatchState) && sizeof(CatchState) == 32, "sdqn_env_state is CatchState");

static const int ENV_THREADS = 512;        // one 21 KB state window = 1323 16-byte chunks: <= 3 per thread

// 16 bytes of a rendered frame starting at byte `first` (first % 16 == 0, frame % 16 == 0): one division for the chunk, then x / y walk
__device__ inline uint4 render_chunk(const CatchView& v, int first, int W, int ch, int cw) {
  int y = first / W, x = first - y * W;
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      word |= (uint32_t)catch_pixel(v, y, x, ch, cw) << (8 * b);
      if (++x == W) { x = 0; ++y; }
    }
    w[k] = word;
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the frame of `v` into up to two device destinations (state-buffer slot, ring-mirror slot): blockIdx.y picks the destination
__global__ void __launch_bounds__(256) catch_render_kernel(CatchView v, uint8_t* dst0, uint8_t* dst1, int H, int W) {
  uint8_t* dst = blockIdx.y ? dst1 : dst0;
  const int frame = H * W, ch = H / CATCH_CELLS, cw = W / CATCH_CELLS;
  if ((frame & 15) == 0 && aligned16(dst)) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < frame / 16) reinterpret_cast<uint4*>(dst)[i] = render_chunk(v, i * 16, W, ch, cw);
  } else {
    for (int i = (blockIdx.x * 256 + threadIdx.x) * 16, e = min(i + 16, frame); i < e; ++i) dst[i] = catch_pixel(v, i / W, i % W, ch, cw);
  }
}
static hipError_t launch_render(const CatchView& v, uint8_t* dst0, uint8_t* dst1, int H, int W, hipStream_t s) {
  const int chunks = (H * W + 15) / 16;
  hipLaunchKernelGGL(catch_render_kernel, dim3((chunks + 255) / 256, dst1 ? 2 : 1), dim3(256), 0, s, v, dst0, dst1, H, W);
  return hipGetLastError();
}

// ---- vectorised evaluation ---------------------------------------------------------------------------------------------------
struct EvalRec {               // one copy of the game, resident on the device for the whole call
  CatchState s;
  uint64_t act_rng;
  int64_t steps, reward, caught, missed, episodes;
};
struct EvalArgs {
  const void* q; int q_f64;    // [>= N][A] Q-values of the forward that precedes this launch (float, or double on a float64 network)
  int A, N, hist, H, W, bpe, init;
  const uint8_t* src; uint8_t* dst;          // [N][hist][H][W]: the window the forward read / the next step's
  EvalRec* envs;
  uint64_t seed, thresh;
  int64_t t;                   // step number (row of the trace)
  uint8_t* tr_act; int8_t* tr_rew; uint8_t* tr_term; double* tr_q;    // [steps][N] ([A]) or all nullptr
};
// --train_envs: where a lockstep's transitions go — slot e lane_len + pos of the ring mirror and of its metadata
struct CollectArgs { uint8_t* ring; MetaRec* meta; int64_t lane_len, pos; };
// One workgroup per copy.  Thread 0: first-maximum argmax (NaN rule of sdqn_net_act_greedy), epsilon-greedy, game step, tallies, restart;
// the view of the new frame reaches the others through LDS; all threads: shift the window into the other buffer and render the new frame
// (restart: zeroed history in front of the first frame, as StateBuffer.reset), 16 bytes per load / store.  COLLECT: the transition is
// also a replay-memory add — the rendered frame goes to the copy's ring slot as well, (action, reward, terminal) to its MetaRec (at a
// terminal the stored frame is the restarted game's first: no valid sample reads it); a.q == nullptr: no Q row was computed (epsilon
// >= 1, every step explores).  The launch that seeds the copies (a.init) is no transition and writes no slot.
template <bool COLLECT>
__device__ __forceinline__ void catch_lockstep(const EvalArgs& a, const CollectArgs& c) {
  __shared__ int sh[4];
  const int e = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    EvalRec r = a.envs[e];
    int restart = 0;
    if (a.init) {
      catch_init(r.s, catch_stream_seed(a.seed, (uint64_t)e, 0));
      r.act_rng = catch_stream_seed(a.seed, (uint64_t)e, 1);
      r.steps = r.reward = r.caught = r.missed = r.episodes = 0;
      restart = 1;
    } else {
      int best = 0; double qb = 0.0;
      for (int k = 0; k < a.A; ++k) {
        const double qk = !a.q ? 0.0 : a.q_f64 ? reinterpret_cast<const double*>(a.q)[(size_t)e * a.A + k] : (double)reinterpret_cast<const float*>(a.q)[(size_t)e * a.A + k];
        if (k == 0 || qk > qb || (qk != qk && qb == qb)) { best = k; qb = qk; }
        if (a.tr_q) a.tr_q[((size_t)a.t * a.N + e) * a.A + k] = qk;
      }
      const int action = catch_epsilon_greedy(r.act_rng, a.thresh, best, a.A);
      const int reward = catch_step(r.s, action, a.bpe);
      const int terminal = r.s.terminal;
      r.steps += 1; r.reward += reward; r.caught += reward > 0; r.missed += reward < 0;
      if (a.tr_act) { const size_t o = (size_t)a.t * a.N + e; a.tr_act[o] = (uint8_t)action; a.tr_rew[o] = (int8_t)reward; a.tr_term[o] = (uint8_t)terminal; }
      if (COLLECT) {
        MetaRec m; m.reward = reward; m.action = (uint8_t)action; m.terminal = (uint8_t)terminal;
        for (int k = 0; k < 6; ++k) m.pad[k] = 0;
        c.meta[(int64_t)e * c.lane_len + c.pos] = m;
      }
      if (terminal) { r.episodes += 1; catch_restart(r.s); restart = 1; }
    }
    a.envs[e] = r;
    sh[0] = r.s.row; sh[1] = r.s.col; sh[2] = r.s.paddle; sh[3] = restart;
  }
  __syncthreads();
  CatchView v; v.row = sh[0]; v.col = sh[1]; v.paddle = sh[2];
  const int restart = sh[3];
  const int frame = a.H * a.W, ch = a.H / CATCH_CELLS, cw = a.W / CATCH_CELLS;
  const size_t state = (size_t)a.hist * frame;
  const uint8_t* src = a.src + (size_t)e * state; uint8_t* dst = a.dst + (size_t)e * state;
  uint8_t* slot = (COLLECT && !a.init) ? c.ring + ((int64_t)e * c.lane_len + c.pos) * frame : nullptr;
  if ((frame & 15) == 0 && aligned16(a.src) && aligned16(a.dst) && (!COLLECT || aligned16(c.ring))) {
    const int n16 = frame / 16, keep = (a.hist - 1) * n16;
    const uint4* s16 = reinterpret_cast<const uint4*>(src) + n16; uint4* d16 = reinterpret_cast<uint4*>(dst);
    for (int i = tid; i < keep; i += ENV_THREADS) d16[i] = restart ? make_uint4(0, 0, 0, 0) : s16[i];
    for (int i = tid; i < n16; i += ENV_THREADS) {
      const uint4 px = render_chunk(v, i * 16, a.W, ch, cw);
      d16[keep + i] = px;
      if (COLLECT && slot) reinterpret_cast<uint4*>(slot)[i] = px;
    }
  } else {
    const int keep = (a.hist - 1) * frame;
    for (int i = tid; i < keep; i += ENV_THREADS) dst[i] = restart ? (uint8_t)0 : src[frame + i];
    for (int i = tid; i < frame; i += ENV_THREADS) {
      const uint8_t px = catch_pixel(v, i / a.W, i % a.W, ch, cw);
      dst[keep + i] = px;
      if (COLLECT && slot) slot[i] = px;
    }
  }
}
__global__ void __launch_bounds__(ENV_THREADS) catch_eval_kernel(const EvalArgs a) { catch_lockstep<false>(a, CollectArgs()); }
__global__ void __launch_bounds__(ENV_THREADS) catch_collect_kernel(const EvalArgs a, const CollectArgs c) { catch_lockstep<true>(a, c); }
static hipError_t launch_collect(const EvalArgs& a, const CollectArgs& c, hipStream_t s) {
  SDQN_LAUNCH(catch_collect_kernel, dim3(a.N), dim3(ENV_THREADS), 0, s, a, c);
  return hipGetLastError();
}

// ---- environment handle: host only, no device needed ------------------------------------------------------------------------------
static bool state_valid(const CatchState& s) {
  return s.row >= 0 && s.row < CATCH_CELLS && s.col >= 0 && s.col < CATCH_CELLS && s.dx >= -1 && s.dx <= 1 && s.paddle >= 0 &&
         s.paddle <= CATCH_CELLS - CATCH_PADDLE && s.balls >= 0 && (s.terminal == 0 || s.terminal == 1);
}
static const uint8_t* env_frame(sdqn_env_s* e) {
  if (!e->frame_ok) { catch_render(catch_view(e->s), e->frame.data(), e->H, e->W); e->frame_ok = true; }
  return e->frame.data();
}
extern "C" int sdqn_env_create(sdqn_env_t* out, const char* name, int H, int W, uint64_t seed, int balls_per_episode) {
  ARGCHK(out && name, "NULL argument");
  ARGCHK(strcmp(name, "catch") == 0, "unknown environment '%s' (known: catch)", name);
  ARGCHK(H >= CATCH_CELLS && W >= CATCH_CELLS && H <= 4096 && W <= 4096, "catch needs a screen of at least %d x %d pixels (got %d x %d)", CATCH_CELLS, CATCH_CELLS, H, W);
  ARGCHK(balls_per_episode >= 1, "balls_per_episode %d < 1", balls_per_episode);
  sdqn_env_s* e = new sdqn_env_s();
  e->H = H; e->W = W; e->bpe = balls_per_episode; e->frame.assign((size_t)H * W, 0);
  catch_init(e->s, seed);
  *out = e; return SDQN_OK;
}
extern "C" int sdqn_env_destroy(sdqn_env_t e) { delete e; return SDQN_OK; }
extern "C" int sdqn_env_restart(sdqn_env_t e) { ARGCHK(e, "NULL handle"); catch_restart(e->s); e->frame_ok = false; return SDQN_OK; }
extern "C" int sdqn_env_num_actions(sdqn_env_t e, int* n) { ARGCHK(e && n, "NULL argument"); *n = CATCH_ACTIONS; return SDQN_OK; }
extern "C" int sdqn_env_step(sdqn_env_t e, int action, int* reward, int* terminal) {
  ARGCHK(e, "NULL handle");
  ARGCHK(action >= 0 && action < CATCH_ACTIONS, "action %d out of range [0, %d)", action, CATCH_ACTIONS);
  const int r = catch_step(e->s, action, e->bpe); e->frame_ok = false;
  if (reward) *reward = r; if (terminal) *terminal = e->s.terminal;
  return SDQN_OK;
}
extern "C" int sdqn_env_screen(sdqn_env_t e, uint8_t* screen) {
  ARGCHK(e && screen, "NULL argument"); memcpy(screen, env_frame(e), e->frame.size()); return SDQN_OK;
}
extern "C" int sdqn_env_get_state(sdqn_env_t e, sdqn_env_state* st) { ARGCHK(e && st, "NULL argument"); memcpy(st, &e->s, sizeof e->s); return SDQN_OK; }
extern "C" int sdqn_env_set_state(sdqn_env_t e, const sdqn_env_state* st) {
  ARGCHK(e && st, "NULL argument");
  CatchState s; memcpy(&s, st, sizeof s);
  ARGCHK(state_valid(s), "catch state out of range (row %d col %d dx %d paddle %d balls %d terminal %d)", s.row, s.col, s.dx, s.paddle, s.balls, s.terminal);
  e->s = s; e->frame_ok = false; return SDQN_OK;
}
// test hook: the frame of the current state as the KERNEL renders it (device scratch, read back; sync)
extern "C" int sdqn_env_render_device(sdqn_env_t e, uint8_t* screen) {
  ARGCHK(e && screen, "NULL argument");
  STREAMCHK();
  const size_t frame = e->frame.size();
  uint8_t* d = nullptr;
  HIPCHK(hipMalloc((void**)&d, frame));
  hipError_t err = launch_render(catch_view(e->s), d, nullptr, e->H, e->W, g_stream);
  if (err == hipSuccess) err = hipMemcpyAsync(screen, d, frame, hipMemcpyDeviceToHost, g_stream);
  if (err == hipSuccess) err = hipStreamSynchronize(g_stream);
  hipFree(d);
  HIPCHK(err);
  return SDQN_OK;
}

// One environment transition in one call, the sibling of sdqn_net_act_step for an environment that lives in the library: the host advances
// the game and renders the new frame into the host mirrors (state-buffer window, pinned ring slot); ONE launch renders the same frame
// from the same three integers into the state buffer's device slot and the ring mirror's slot.  No frame bytes cross PCIe; everything
// else an add does (metadata, count / current, prioritized bookkeeping, generations, wrap, speculation) is the shared code of the add paths.
extern "C" int sdqn_net_act_step_env(sdqn_net_t h, sdqn_statebuf_t sb, sdqn_replay_t r, sdqn_env_t e, int action, int speculate,
                                     int* reward, int* terminal) {
  ARGCHK(h && sb && e, "NULL argument");
  ARGCHK(action >= 0 && action < CATCH_ACTIONS, "action %d out of range [0, %d)", action, CATCH_ACTIONS);
  ARGCHK(!r || !r->lanes, "a laned replay memory (sdqn_replay_set_lanes) is written by sdqn_env_collect only");
  const int64_t FRAME = (int64_t)e->H * e->W;
  ARGCHK(sb->frame == FRAME, "the state buffer's screens (%lld bytes) and the environment's (%lld) differ", (long long)sb->frame, (long long)FRAME);
  ARGCHK(!r || r->frame == FRAME, "the replay memory's screens (%lld bytes) and the environment's (%lld) differ", (long long)(r ? r->frame : 0), (long long)FRAME);
  const int rew = catch_step(e->s, action, e->bpe), term = e->s.terminal;
  const CatchView v = catch_view(e->s);
  uint8_t *hf, *dv;
  int rc = statebuf_advance(sb, &hf, &dv); if (rc) return rc;
  catch_render(v, hf, e->H, e->W);
  memcpy(e->frame.data(), hf, (size_t)FRAME); e->frame_ok = true;
  int64_t c = -1; uint8_t* ring_slot = nullptr;
  if (r) {
    c = replay_add_meta(r, action, rew, term);
    memcpy(r->screens + c * FRAME, hf, (size_t)FRAME);
    if (!(r->flags & SDQN_REPLAY_ZERO_COPY)) ring_slot = r->d_ring + c * FRAME;      // (zero copy: the pinned ring IS what the kernels read)
  }
  HIPCHK(launch_render(v, dv, ring_slot, e->H, e->W, g_stream));
  if (r) { rc = replay_add_commit(r, c); if (rc) return rc; }
  if (reward) *reward = rew; if (terminal) *terminal = term;
  if (speculate && !term && !h->gen && (size_t)sb->hist * sb->frame == (size_t)STATE) return predict_state_enqueue(h, sb);   // (a terminal step: the episode restarts, nobody wants this state's Q-values)
  return SDQN_OK;
}

// N independent copies of the game played by the online net, epsilon-greedy, entirely on the device: per step the batched forward of
// sdqn_net_predict (the generic path's forward for float64 / other geometries) on the [batch][hist][H][W] window buffer, then ONE launch
// of catch_eval_kernel; two window buffers alternate (read one, write the other).  Nothing returns to the host inside the loop; one
// stream synchronisation at the end.  The environment handle gives the geometry and balls_per_episode; its own state is not touched.
extern "C" int sdqn_env_eval(sdqn_net_t h, sdqn_env_t e, int N, int64_t steps, double epsilon, uint64_t seed,
                             int64_t* out_steps, int64_t* out_reward, int64_t* out_caught, int64_t* out_missed, int64_t* out_episodes,
                             uint8_t* tr_actions, int8_t* tr_rewards, uint8_t* tr_terminals, double* tr_q) {
  ARGCHK(h && e, "NULL argument");
  const int hist = h->gen ? h->cfg.history_length : C0, H = h->gen ? h->cfg.screen_height : H0, W = h->gen ? h->cfg.screen_width : W0;
  ARGCHK(e->H == H && e->W == W, "the environment's screen (%d x %d) and the network's (%d x %d) differ", e->H, e->W, H, W);
  ARGCHK(h->A == CATCH_ACTIONS, "the network has %d actions, catch has %d", h->A, CATCH_ACTIONS);
  ARGCHK(N >= 1 && N <= h->B, "num_envs %d out of range [1, batch_size %d]", N, h->B);
  ARGCHK(steps >= 1, "steps %lld < 1", (long long)steps);
  ARGCHK(epsilon >= 0.0 && epsilon <= 1.0, "epsilon %g out of range [0, 1]", epsilon);
  const bool trace = tr_actions || tr_rewards || tr_terminals || tr_q;
  ARGCHK(!trace || (tr_actions && tr_rewards && tr_terminals && tr_q), "the trace buffers come together: all four or none");
  STREAMCHK();
  const size_t state = (size_t)hist * H * W, half = (size_t)h->B * state;      // (rows N .. batch_size - 1 stay zero: the forward runs the full batch)
  const size_t tn = trace ? (size_t)steps * N : 0;
  uint8_t* win = nullptr; EvalRec* recs = nullptr; uint8_t* tr = nullptr; double* trq = nullptr;
  std::vector<EvalRec> hrec((size_t)N);
  auto body = [&]() -> int {
    HIPCHK(hipMalloc((void**)&win, 2 * half + SRC_PAD));
    HIPCHK(hipMemsetAsync(win, 0, 2 * half + SRC_PAD, g_stream));
    HIPCHK(hipMalloc((void**)&recs, (size_t)N * sizeof(EvalRec)));
    HIPCHK(hipMemsetAsync(recs, 0, (size_t)N * sizeof(EvalRec), g_stream));
    if (trace) { HIPCHK(hipMalloc((void**)&tr, 3 * tn)); HIPCHK(hipMalloc((void**)&trq, tn * h->A * sizeof(double))); }
    EvalArgs a; memset(&a, 0, sizeof a);
    a.q = h->gen ? h->gen->q_dev() : (const void*)h->q; a.q_f64 = (h->gen && h->gen->is_f64()) ? 1 : 0;
    a.A = h->A; a.N = N; a.hist = hist; a.H = H; a.W = W; a.bpe = e->bpe; a.envs = recs; a.seed = seed;
    a.thresh = (uint64_t)ceil(ldexp(epsilon, 53));
    if (trace) { a.tr_act = tr; a.tr_rew = reinterpret_cast<int8_t*>(tr + tn); a.tr_term = tr + 2 * tn; a.tr_q = trq; }
    a.init = 1; a.src = win + half; a.dst = win;
    hipLaunchKernelGGL(catch_eval_kernel, dim3(N), dim3(ENV_THREADS), 0, g_stream, a);
    HIPCHK(hipGetLastError());
    a.init = 0;
    for (int64_t t = 0; t < steps; ++t) {
      const uint8_t* cur = win + (size_t)(t & 1) * half;
      if (h->gen) GENCHK(h->gen->forward_dev(cur, N));
      else {
        StepArgs fa = step_args(h); fa.nz = 1; fa.from_ring = 0; fa.src = cur;     // what sdqn_net_predict launches
        int rc = run_forward(h, fa, head_args(h, 0)); if (rc) return rc;
      }
      a.t = t; a.src = cur; a.dst = win + (size_t)((t + 1) & 1) * half;
      hipLaunchKernelGGL(catch_eval_kernel, dim3(N), dim3(ENV_THREADS), 0, g_stream, a);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(hrec.data(), recs, (size_t)N * sizeof(EvalRec), hipMemcpyDeviceToHost, g_stream));
    if (trace) {
      HIPCHK(hipMemcpyAsync(tr_actions, a.tr_act, tn, hipMemcpyDeviceToHost, g_stream));
      HIPCHK(hipMemcpyAsync(tr_rewards, a.tr_rew, tn, hipMemcpyDeviceToHost, g_stream));
      HIPCHK(hipMemcpyAsync(tr_terminals, a.tr_term, tn, hipMemcpyDeviceToHost, g_stream));
      HIPCHK(hipMemcpyAsync(tr_q, trq, tn * h->A * sizeof(double), hipMemcpyDeviceToHost, g_stream));
    }
    HIPCHK(hipStreamSynchronize(g_stream));
    return SDQN_OK;
  };
  const int rc = body();
  if (rc && g_stream) hipStreamSynchronize(g_stream);
  hipFree(win); hipFree(recs); hipFree(tr); hipFree(trq);
  if (rc) return rc;
  for (int i = 0; i < N; ++i) {
    if (out_steps) out_steps[i] = hrec[i].steps; if (out_reward) out_reward[i] = hrec[i].reward;
    if (out_caught) out_caught[i] = hrec[i].caught; if (out_missed) out_missed[i] = hrec[i].missed;
    if (out_episodes) out_episodes[i] = hrec[i].episodes;
  }
  return SDQN_OK;
}

// --train_envs: `locksteps` locksteps of num_envs copies of the game, each lockstep num_envs transitions written into the
// laned ring r by ONE launch of catch_collect_kernel behind the forward of sdqn_net_predict (no forward while epsilon >= 1: no Q row is
// read).  The copies' records and the two window buffers live on the net handle: seed >= 0 seeds the copies as sdqn_env_eval does and
// renders their first frames, seed < 0 goes on where the last call stopped.  Lockstep t of the call plays with
// epsilon = clamp(epsilon_start + t epsilon_step, 0, 1).  Per lockstep two strided device-to-host copies bring the num_envs frames and
// MetaRecs into the pinned master, which stays a true copy of the mirror; nothing goes host to device and nothing waits until the single
// synchronisation at the end, after which actions / rewards / terminals are unpacked.  Tallies: the copies' running sums since they were seeded.
extern "C" int sdqn_env_collect(sdqn_net_t h, sdqn_env_t e, sdqn_replay_t r, int N, int64_t locksteps, double epsilon_start, double epsilon_step,
                                int64_t seed, int64_t* out_steps, int64_t* out_reward, int64_t* out_caught, int64_t* out_missed,
                                int64_t* out_episodes, uint8_t* tr_actions, int8_t* tr_rewards, uint8_t* tr_terminals, double* tr_q) {
  ARGCHK(h && e && r, "NULL argument");
  const int hist = h->gen ? h->cfg.history_length : C0, H = h->gen ? h->cfg.screen_height : H0, W = h->gen ? h->cfg.screen_width : W0;
  ARGCHK(e->H == H && e->W == W, "the environment's screen (%d x %d) and the network's (%d x %d) differ", e->H, e->W, H, W);
  ARGCHK(r->H == H && r->W == W && r->hist == hist, "the replay memory's geometry (%d x %d, history %d) and the network's (%d x %d, %d) differ", r->H, r->W, r->hist, H, W, hist);
  ARGCHK(h->A == CATCH_ACTIONS, "the network has %d actions, catch has %d", h->A, CATCH_ACTIONS);
  ARGCHK(N >= 1 && N <= h->B, "num_envs %d out of range [1, batch_size %d]", N, h->B);
  ARGCHK(r->lanes == N, "the replay memory has %d lanes, num_envs is %d (sdqn_replay_set_lanes)", r->lanes, N);
  ARGCHK(locksteps >= 0, "locksteps %lld < 0", (long long)locksteps);
  ARGCHK(epsilon_start >= 0.0 && epsilon_start <= 1.0, "epsilon %g out of range [0, 1]", epsilon_start);
  const bool trace = tr_actions || tr_rewards || tr_terminals || tr_q;
  ARGCHK(!trace || (tr_actions && tr_rewards && tr_terminals && tr_q), "the trace buffers come together: all four or none");
  const size_t state = (size_t)hist * H * W, half = (size_t)h->B * state;      // (rows N .. batch_size - 1 stay zero: the forward runs the full batch)
  ARGCHK(seed >= 0 || (h->col_recs && h->col_N == N && h->col_state == state), "nothing to resume: the copies were never seeded for %d environments", N);
  STREAMCHK();
  if (!h->col_win) {
    int rc = dalloc(h, (void**)&h->col_win, 2 * half + SRC_PAD); if (rc) return rc;
    rc = dalloc(h, &h->col_recs, (size_t)h->B * sizeof(EvalRec)); if (rc) return rc;
  }
  EvalRec* recs = static_cast<EvalRec*>(h->col_recs);
  const size_t tn = trace ? (size_t)locksteps * N : 0;
  const int64_t FRAME = r->frame, L = r->lane_len;
  uint8_t* tr = nullptr; double* trq = nullptr;
  std::vector<EvalRec> hrec((size_t)N);
  int64_t p = r->lane_pos, f = r->lane_fill, launched = 0;
  auto body = [&]() -> int {
    if (tn) { HIPCHK(hipMalloc((void**)&tr, 3 * tn)); HIPCHK(hipMalloc((void**)&trq, tn * h->A * sizeof(double))); }
    EvalArgs a; memset(&a, 0, sizeof a);
    a.q_f64 = (h->gen && h->gen->is_f64()) ? 1 : 0;
    a.A = h->A; a.N = N; a.hist = hist; a.H = H; a.W = W; a.bpe = e->bpe; a.envs = recs;
    CollectArgs c; c.ring = r->d_ring; c.meta = r->d_meta; c.lane_len = L; c.pos = p;
    if (tn) { a.tr_act = tr; a.tr_rew = reinterpret_cast<int8_t*>(tr + tn); a.tr_term = tr + 2 * tn; a.tr_q = trq; }
    if (seed >= 0) {
      HIPCHK(hipMemsetAsync(h->col_win, 0, 2 * half + SRC_PAD, g_stream));
      a.seed = (uint64_t)seed; a.init = 1; a.src = h->col_win + half; a.dst = h->col_win;
      hipLaunchKernelGGL(catch_collect_kernel, dim3(N), dim3(ENV_THREADS), 0, g_stream, a, c);
      HIPCHK(hipGetLastError());
      a.init = 0; h->col_t = 0; h->col_N = N; h->col_state = state;
    }
    for (int64_t t = 0; t < locksteps; ++t) {
      const int64_t T = h->col_t;
      const uint8_t* cur = h->col_win + (size_t)(T & 1) * half;
      double eps = epsilon_start + (double)t * epsilon_step;
      eps = eps < 0.0 ? 0.0 : (eps > 1.0 ? 1.0 : eps);
      a.q = nullptr;
      if (eps < 1.0) {
        if (h->gen) GENCHK(h->gen->forward_dev(cur, N));
        else {
          StepArgs fa = step_args(h); fa.nz = 1; fa.from_ring = 0; fa.src = cur;     // what sdqn_net_predict launches
          int rc = run_forward(h, fa, head_args(h, 0)); if (rc) return rc;
        }
        a.q = h->gen ? h->gen->q_dev() : (const void*)h->q;
      }
      a.thresh = (uint64_t)ceil(ldexp(eps, 53));
      a.t = t; a.src = cur; a.dst = h->col_win + (size_t)((T + 1) & 1) * half;
      c.pos = p;
      LAUNCH(K_COLLECT, launch_collect(a, c, g_stream));
      h->col_t = T + 1;
      // the lockstep's N slots, one per lane, L slots apart: one strided copy of the frames and one of the MetaRecs
      HIPCHK(hipMemcpy2DAsync(r->screens + p * FRAME, (size_t)L * FRAME, r->d_ring + p * FRAME, (size_t)L * FRAME, (size_t)FRAME, (size_t)N,
                              hipMemcpyDeviceToHost, g_stream));
      HIPCHK(hipMemcpy2DAsync(r->h_meta + p, (size_t)L * sizeof(MetaRec), r->d_meta + p, (size_t)L * sizeof(MetaRec), sizeof(MetaRec), (size_t)N,
                              hipMemcpyDeviceToHost, g_stream));
      p = (p + 1) % L; if (f < L) ++f;
      ++launched;
    }
    HIPCHK(hipMemcpyAsync(hrec.data(), recs, (size_t)N * sizeof(EvalRec), hipMemcpyDeviceToHost, g_stream));
    if (tn) {
      HIPCHK(hipMemcpyAsync(tr_actions, a.tr_act, tn, hipMemcpyDeviceToHost, g_stream));
      HIPCHK(hipMemcpyAsync(tr_rewards, a.tr_rew, tn, hipMemcpyDeviceToHost, g_stream));
      HIPCHK(hipMemcpyAsync(tr_terminals, a.tr_term, tn, hipMemcpyDeviceToHost, g_stream));
      HIPCHK(hipMemcpyAsync(tr_q, trq, tn * h->A * sizeof(double), hipMemcpyDeviceToHost, g_stream));
    }
    HIPCHK(hipStreamSynchronize(g_stream));
    return SDQN_OK;
  };
  const int rc = body();
  if (rc && g_stream) hipStreamSynchronize(g_stream);
  hipFree(tr); hipFree(trq);
  // the positions written, newest last (a failed call: whatever reached the master is unpacked too, fill and position follow the launches made)
  const int64_t touched = launched < L ? launched : L;
  for (int64_t k = 0; k < touched; ++k) {
    const int64_t q = ((p - 1 - k) % L + L) % L;
    for (int en = 0; en < N; ++en) {
      const int64_t sl = (int64_t)en * L + q; const MetaRec& m = r->h_meta[sl];
      r->actions[sl] = m.action; r->rewards[sl] = m.reward; r->terminals[sl] = m.terminal;
    }
  }
  r->lane_pos = p; r->lane_fill = f;
  if (rc) return rc;
  for (int i = 0; i < N; ++i) {
    if (out_steps) out_steps[i] = hrec[i].steps; if (out_reward) out_reward[i] = hrec[i].reward;
    if (out_caught) out_caught[i] = hrec[i].caught; if (out_missed) out_missed[i] = hrec[i].missed;
    if (out_episodes) out_episodes[i] = hrec[i].episodes;
  }
  return SDQN_OK;
}

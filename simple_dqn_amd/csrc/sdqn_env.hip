// sdqn_env.hip — the device-resident games "catch" (env_catch.h), "breakout" (env_breakout.h; §20) and "freeway"
// (env_freeway.h; §25): host entry points of the environment handle, the render kernel of the fused act step (sdqn_net_act_step_env),
// the vectorised on-device evaluation loop (sdqn_env_eval) and vectorised collection (sdqn_env_collect).  Everything below is written
// once against a game trait G (CatchGame, BreakoutGame, FreewayGame: state, view, init / restart / step, renderer, action count,
// tallies) and instantiated per game: three kernels each and one row of the dispatch at the entry points.  The kernels of this feature live here only: the train step's translation units are untouched.
// Every path that steps a game does so through dynamics_step (env_dynamics.h): frame skip and sticky actions.
#include "api_internal.h"
#include "env_catch.h"
#include "env_breakout.h"
#include "env_freeway.h"
#include "env_dynamics.h"

enum { GAME_CATCH = 0, GAME_BREAKOUT = 1, GAME_FREEWAY = 2 };
struct sdqn_env_s {
  int game = GAME_CATCH;
  CatchState cs;                           // the state of the handle's game: the others are unused
  BreakoutState bs;
  FreewayState fs;
  int H = 0, W = 0, bpe = 10;              // bpe: balls per episode; freeway: game ticks per episode
  int frame_skip = 1;                      // the dynamics: ticks per agent step, repeat_action_probability p and
  double p = 0.0;                          // its integer form ceil(p 2^53)
  uint64_t thresh_p = 0;
  int32_t prev = 0;                        // the action the last tick executed (0 after create / restart)
  uint64_t sticky_rng = 0;                 // the sticky generator: stream_seed(seed, 0, 2) at create
  std::vector<uint8_t> frame;              // the host-rendered frame of the state (valid while frame_ok)
  bool frame_ok = false;
  template <class G> typename G::State& st();
};
template <> inline CatchState& sdqn_env_s::st<CatchGame>() { return cs; }
template <> inline BreakoutState& sdqn_env_s::st<BreakoutGame>() { return bs; }
template <> inline FreewayState& sdqn_env_s::st<FreewayGame>() { return fs; }
static_assert(sizeof(sdqn_env_state) == sizeof(CatchState) && sizeof(CatchState) == 32, "sdqn_env_state is CatchState");
static_assert(sizeof(sdqn_env_state_breakout) == sizeof(BreakoutState) && sizeof(BreakoutState) == 48, "sdqn_env_state_breakout is BreakoutState");
static_assert(sizeof(sdqn_env_state_freeway) == sizeof(FreewayState) && sizeof(FreewayState) == 56, "sdqn_env_state_freeway is FreewayState");
// one row per game: `return GAME_CALL(e, fn, args...)` calls fn<G>(args...) for the handle's game
#define GAME_CALL(e, fn, ...) \
  ((e)->game == GAME_FREEWAY ? fn<FreewayGame>(__VA_ARGS__) : (e)->game == GAME_BREAKOUT ? fn<BreakoutGame>(__VA_ARGS__) : fn<CatchGame>(__VA_ARGS__))

static const int ENV_THREADS = 512;        // one 21 KB state window = 1323 16-byte chunks: <= 3 per thread

// 16 bytes of a rendered frame starting at byte `first` (first % 16 == 0, frame % 16 == 0): one division for the chunk, then the game's
// cursor walks x / y (and whatever else its renderer keeps per pixel)
template <class G>
__device__ inline uint4 render_chunk(const typename G::View& v, int first, int W, int ch, int cw) {
  const int y = first / W;
  typename G::Cursor c = G::cursor(y, first - y * W, ch, cw);
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      word |= (uint32_t)G::pixel(v, c, ch, cw) << (8 * b);
      G::advance(c, W, ch, cw);
    }
    w[k] = word;
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}
// the byte path (a frame that is no multiple of 16 bytes, or a destination that is not aligned): bytes [first, min(first + 16, frame)) of
// the same chunking, stored one by one into dst and, when given, slot
template <class G>
__device__ inline void render_bytes(const typename G::View& v, int first, int frame, int W, int ch, int cw, uint8_t* dst, uint8_t* slot) {
  const int y = first / W;
  typename G::Cursor c = G::cursor(y, first - y * W, ch, cw);
  for (int i = first, e = min(first + 16, frame); i < e; ++i) {
    const uint8_t px = G::pixel(v, c, ch, cw);
    dst[i] = px;
    if (slot) slot[i] = px;
    G::advance(c, W, ch, cw);
  }
}
__device__ inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the frame of `v` into up to two device destinations (state-buffer slot, ring-mirror slot): blockIdx.y picks the destination
template <class G>
__device__ __forceinline__ void render_frame(const typename G::View& v, uint8_t* dst0, uint8_t* dst1, int H, int W) {
  uint8_t* dst = blockIdx.y ? dst1 : dst0;
  const int frame = H * W, ch = H / G::CELLS, cw = W / G::CELLS;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if ((frame & 15) == 0 && aligned16(dst)) {
    if (i < frame / 16) reinterpret_cast<uint4*>(dst)[i] = render_chunk<G>(v, i * 16, W, ch, cw);
  } else if (i * 16 < frame) {
    render_bytes<G>(v, i * 16, frame, W, ch, cw, dst, nullptr);
  }
}
__global__ void __launch_bounds__(256) catch_render_kernel(CatchView v, uint8_t* dst0, uint8_t* dst1, int H, int W) { render_frame<CatchGame>(v, dst0, dst1, H, W); }
__global__ void __launch_bounds__(256) breakout_render_kernel(BreakoutView v, uint8_t* dst0, uint8_t* dst1, int H, int W) { render_frame<BreakoutGame>(v, dst0, dst1, H, W); }
__global__ void __launch_bounds__(256) freeway_render_kernel(FreewayView v, uint8_t* dst0, uint8_t* dst1, int H, int W) { render_frame<FreewayGame>(v, dst0, dst1, H, W); }

// ---- vectorised evaluation ---------------------------------------------------------------------------------------------------
template <class G>
struct EvalRec {               // one copy of the game, resident on the device for the whole call
  typename G::State s;
  uint64_t act_rng;
  int64_t steps, reward, caught, missed, episodes;
  uint64_t sticky_rng;         // the dynamics of the copy (env_dynamics.h): sticky generator, the action its last tick executed
  int32_t prev, pad_;
};
struct EvalArgs {
  const void* q; int q_f64;    // [>= N][A] Q-values of the forward that precedes this launch (float, or double on a float64 network)
  int A, N, hist, H, W, bpe, init;
  int frame_skip; uint64_t thresh_p;         // the dynamics every copy plays under (env_dynamics.h)
  const uint8_t* src; uint8_t* dst;          // [N][hist][H][W]: the window the forward read / the next step's
  void* envs;                  // EvalRec<G>[N]
  uint64_t seed, thresh;
  int64_t t;                   // step number (row of the trace)
  uint8_t* tr_act; int8_t* tr_rew; uint8_t* tr_term; double* tr_q;    // [steps][N] ([A]) or all nullptr
};
// --train_envs: where a lockstep's transitions go — slot e lane_len + pos of the ring mirror and of its metadata
struct CollectArgs { uint8_t* ring; MetaRec* meta; int64_t lane_len, pos; };
// One workgroup per copy.  Thread 0: first-maximum argmax (NaN rule of sdqn_net_act_greedy), epsilon-greedy, agent step (up to frame_skip
// game ticks under sticky actions: dynamics_step; trace and MetaRec carry the chosen action and the summed reward), tallies, restart;
// the view of the new frame reaches the others through LDS; all threads: shift the window into the other buffer and render the new frame
// (restart: zeroed history in front of the first frame, as StateBuffer.reset), 16 bytes per load / store.  COLLECT: the transition is
// also a replay-memory add — the rendered frame goes to the copy's ring slot as well, (action, reward, terminal) to its MetaRec (at a
// terminal the stored frame is the restarted game's first: no valid sample reads it); a.q == nullptr: no Q row was computed (epsilon
// >= 1, every step explores).  The launch that seeds the copies (a.init) is no transition and writes no slot.
template <class G, bool COLLECT>
__device__ __forceinline__ void env_lockstep(const EvalArgs& a, const CollectArgs& c) {
  __shared__ int sh[G::VIEW_WORDS + 1];
  const int e = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    EvalRec<G>* envs = static_cast<EvalRec<G>*>(a.envs);
    EvalRec<G> r = envs[e];
    int restart = 0;
    if (a.init) {
      G::init(r.s, stream_seed(a.seed, (uint64_t)e, 0));
      r.act_rng = stream_seed(a.seed, (uint64_t)e, 1);
      r.sticky_rng = stream_seed(a.seed, (uint64_t)e, DYNAMICS_STICKY_STREAM); r.prev = 0; r.pad_ = 0;
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
      int caught, lost;
      const int reward = dynamics_step<G>(r.s, r.prev, r.sticky_rng, action, a.bpe, a.frame_skip, a.thresh_p, caught, lost);
      const int terminal = r.s.terminal;
      r.steps += 1; r.reward += reward; r.caught += caught; r.missed += lost;
      if (a.tr_act) { const size_t o = (size_t)a.t * a.N + e; a.tr_act[o] = (uint8_t)action; a.tr_rew[o] = (int8_t)reward; a.tr_term[o] = (uint8_t)terminal; }
      if (COLLECT) {
        MetaRec m; m.reward = reward; m.action = (uint8_t)action; m.terminal = (uint8_t)terminal;
        for (int k = 0; k < 6; ++k) m.pad[k] = 0;
        c.meta[(int64_t)e * c.lane_len + c.pos] = m;
      }
      if (terminal) { r.episodes += 1; dynamics_restart<G>(r.s, r.prev); restart = 1; }
    }
    envs[e] = r;
    G::pack(G::view(r.s), sh); sh[G::VIEW_WORDS] = restart;
  }
  __syncthreads();
  const typename G::View v = G::unpack(sh);
  const int restart = sh[G::VIEW_WORDS];
  const int frame = a.H * a.W, ch = a.H / G::CELLS, cw = a.W / G::CELLS;
  const size_t state = (size_t)a.hist * frame;
  const uint8_t* src = a.src + (size_t)e * state; uint8_t* dst = a.dst + (size_t)e * state;
  uint8_t* slot = (COLLECT && !a.init) ? c.ring + ((int64_t)e * c.lane_len + c.pos) * frame : nullptr;
  if ((frame & 15) == 0 && aligned16(a.src) && aligned16(a.dst) && (!COLLECT || aligned16(c.ring))) {
    const int n16 = frame / 16, keep = (a.hist - 1) * n16;
    const uint4* s16 = reinterpret_cast<const uint4*>(src) + n16; uint4* d16 = reinterpret_cast<uint4*>(dst);
    for (int i = tid; i < keep; i += ENV_THREADS) d16[i] = restart ? make_uint4(0, 0, 0, 0) : s16[i];
    for (int i = tid; i < n16; i += ENV_THREADS) {
      const uint4 px = render_chunk<G>(v, i * 16, a.W, ch, cw);
      d16[keep + i] = px;
      if (COLLECT && slot) reinterpret_cast<uint4*>(slot)[i] = px;
    }
  } else {
    const int keep = (a.hist - 1) * frame;
    for (int i = tid; i < keep; i += ENV_THREADS) dst[i] = restart ? (uint8_t)0 : src[frame + i];
    for (int i = tid * 16; i < frame; i += ENV_THREADS * 16) render_bytes<G>(v, i, frame, a.W, ch, cw, dst + keep, COLLECT ? slot : nullptr);
  }
}
__global__ void __launch_bounds__(ENV_THREADS) catch_eval_kernel(const EvalArgs a) { env_lockstep<CatchGame, false>(a, CollectArgs()); }
__global__ void __launch_bounds__(ENV_THREADS) catch_collect_kernel(const EvalArgs a, const CollectArgs c) { env_lockstep<CatchGame, true>(a, c); }
__global__ void __launch_bounds__(ENV_THREADS) breakout_eval_kernel(const EvalArgs a) { env_lockstep<BreakoutGame, false>(a, CollectArgs()); }
__global__ void __launch_bounds__(ENV_THREADS) breakout_collect_kernel(const EvalArgs a, const CollectArgs c) { env_lockstep<BreakoutGame, true>(a, c); }
__global__ void __launch_bounds__(ENV_THREADS) freeway_eval_kernel(const EvalArgs a) { env_lockstep<FreewayGame, false>(a, CollectArgs()); }
__global__ void __launch_bounds__(ENV_THREADS) freeway_collect_kernel(const EvalArgs a, const CollectArgs c) { env_lockstep<FreewayGame, true>(a, c); }

// the three kernels of a game; `timed`: the launch the profile's "catch_collect(lockstep)" row brackets (either game's lockstep)
template <class G> struct Kernels;
#define GAME_KERNELS(G, PREFIX) \
  template <> struct Kernels<G> { \
    static hipError_t render(const G::View& v, uint8_t* dst0, uint8_t* dst1, int H, int W, hipStream_t s) { \
      const int chunks = (H * W + 15) / 16; \
      hipLaunchKernelGGL(PREFIX##_render_kernel, dim3((chunks + 255) / 256, dst1 ? 2 : 1), dim3(256), 0, s, v, dst0, dst1, H, W); \
      return hipGetLastError(); \
    } \
    static hipError_t eval(const EvalArgs& a, hipStream_t s) { \
      hipLaunchKernelGGL(PREFIX##_eval_kernel, dim3(a.N), dim3(ENV_THREADS), 0, s, a); \
      return hipGetLastError(); \
    } \
    static hipError_t collect(const EvalArgs& a, const CollectArgs& c, hipStream_t s, bool timed) { \
      if (timed) SDQN_LAUNCH(PREFIX##_collect_kernel, dim3(a.N), dim3(ENV_THREADS), 0, s, a, c); \
      else hipLaunchKernelGGL(PREFIX##_collect_kernel, dim3(a.N), dim3(ENV_THREADS), 0, s, a, c); \
      return hipGetLastError(); \
    } \
  }
GAME_KERNELS(CatchGame, catch);
GAME_KERNELS(BreakoutGame, breakout);
GAME_KERNELS(FreewayGame, freeway);
#undef GAME_KERNELS

// ---- environment handle: host only, no device needed ------------------------------------------------------------------------------
template <class G> static const uint8_t* env_frame(sdqn_env_s* e) {
  if (!e->frame_ok) { G::render(G::view(e->st<G>()), e->frame.data(), e->H, e->W); e->frame_ok = true; }
  return e->frame.data();
}
template <class G> static int env_init(sdqn_env_s* e, uint64_t seed) { G::init(e->st<G>(), seed); return SDQN_OK; }
template <class G> static int env_restart(sdqn_env_s* e) { dynamics_restart<G>(e->st<G>(), e->prev); e->frame_ok = false; return SDQN_OK; }
// one agent step of the handle's game under its dynamics: the ONE place the host steps a game (sdqn_env_step, act_step_env)
template <class G> static int env_advance(sdqn_env_s* e, int action) {
  int caught, lost;
  const int r = dynamics_step<G>(e->st<G>(), e->prev, e->sticky_rng, action, e->bpe, e->frame_skip, e->thresh_p, caught, lost);
  e->frame_ok = false;
  return r;
}
template <class G> static int env_num_actions(int* n) { *n = G::ACTIONS; return SDQN_OK; }
template <class G> static int env_name(const char** name) { *name = G::NAME; return SDQN_OK; }
template <class G> static int env_step(sdqn_env_s* e, int action, int* reward, int* terminal) {
  ARGCHK(action >= 0 && action < G::ACTIONS, "action %d out of range [0, %d)", action, G::ACTIONS);
  const int r = env_advance<G>(e, action);
  if (reward) *reward = r; if (terminal) *terminal = e->st<G>().terminal;
  return SDQN_OK;
}
template <class G> static int env_screen(sdqn_env_s* e, uint8_t* screen) { memcpy(screen, env_frame<G>(e), e->frame.size()); return SDQN_OK; }
extern "C" int sdqn_env_create(sdqn_env_t* out, const char* name, int H, int W, uint64_t seed, int balls_per_episode) {
  ARGCHK(out && name, "NULL argument");
  const int game = strcmp(name, FreewayGame::NAME) == 0 ? GAME_FREEWAY : strcmp(name, BreakoutGame::NAME) == 0 ? GAME_BREAKOUT : strcmp(name, CatchGame::NAME) == 0 ? GAME_CATCH : -1;
  ARGCHK(game >= 0, "unknown environment '%s' (known: catch, breakout, freeway)", name);
  ARGCHK(H >= CATCH_CELLS && W >= CATCH_CELLS && H <= 4096 && W <= 4096, "%s needs a screen of at least %d x %d pixels (got %d x %d)", name, CATCH_CELLS, CATCH_CELLS, H, W);
  ARGCHK(balls_per_episode >= 1, "%s %d < 1", game == GAME_FREEWAY ? "episode_ticks" : "balls_per_episode", balls_per_episode);
  sdqn_env_s* e = new sdqn_env_s();
  e->game = game;
  e->H = H; e->W = W; e->bpe = balls_per_episode; e->frame.assign((size_t)H * W, 0);
  e->sticky_rng = stream_seed(seed, 0, DYNAMICS_STICKY_STREAM);
  GAME_CALL(e, env_init, e, seed);
  *out = e; return SDQN_OK;
}
extern "C" int sdqn_env_destroy(sdqn_env_t e) { delete e; return SDQN_OK; }
extern "C" int sdqn_env_name(sdqn_env_t e, const char** name) { ARGCHK(e && name, "NULL argument"); return GAME_CALL(e, env_name, name); }
extern "C" int sdqn_env_restart(sdqn_env_t e) { ARGCHK(e, "NULL handle"); return GAME_CALL(e, env_restart, e); }
extern "C" int sdqn_env_num_actions(sdqn_env_t e, int* n) { ARGCHK(e && n, "NULL argument"); return GAME_CALL(e, env_num_actions, n); }
extern "C" int sdqn_env_step(sdqn_env_t e, int action, int* reward, int* terminal) {
  ARGCHK(e, "NULL handle");
  return GAME_CALL(e, env_step, e, action, reward, terminal);
}
extern "C" int sdqn_env_screen(sdqn_env_t e, uint8_t* screen) { ARGCHK(e && screen, "NULL argument"); return GAME_CALL(e, env_screen, e, screen); }
// the state entry points, one pair per game: SDQN_ERR_ARG on another game's handle; a refused set leaves the state untouched
static const char* game_name(int game) { return game == GAME_FREEWAY ? FreewayGame::NAME : game == GAME_BREAKOUT ? BreakoutGame::NAME : CatchGame::NAME; }
template <class G> static int env_get_state(sdqn_env_s* e, int game, void* st, const char* fn) {
  ARGCHK(e && st, "NULL argument");
  ARGCHK(e->game == game, "%s serves %s; this environment is %s", fn, G::NAME, game_name(e->game));
  memcpy(st, &e->st<G>(), sizeof(typename G::State)); return SDQN_OK;
}
template <class G> static int env_state_checked(sdqn_env_s* e, int game, const void* st, typename G::State& s, const char* fn) {
  ARGCHK(e && st, "NULL argument");
  ARGCHK(e->game == game, "%s serves %s; this environment is %s", fn, G::NAME, game_name(e->game));
  memcpy(&s, st, sizeof s); return SDQN_OK;
}
extern "C" int sdqn_env_get_state(sdqn_env_t e, sdqn_env_state* st) { return env_get_state<CatchGame>(e, GAME_CATCH, st, "sdqn_env_get_state"); }
extern "C" int sdqn_env_set_state(sdqn_env_t e, const sdqn_env_state* st) {
  CatchState s; int rc = env_state_checked<CatchGame>(e, GAME_CATCH, st, s, "sdqn_env_set_state"); if (rc) return rc;
  ARGCHK(CatchGame::valid(s), "catch state out of range (row %d col %d dx %d paddle %d balls %d terminal %d)", s.row, s.col, s.dx, s.paddle, s.balls, s.terminal);
  e->cs = s; e->frame_ok = false; return SDQN_OK;
}
extern "C" int sdqn_env_get_state_breakout(sdqn_env_t e, sdqn_env_state_breakout* st) {
  return env_get_state<BreakoutGame>(e, GAME_BREAKOUT, st, "sdqn_env_get_state_breakout");
}
extern "C" int sdqn_env_set_state_breakout(sdqn_env_t e, const sdqn_env_state_breakout* st) {
  BreakoutState s; int rc = env_state_checked<BreakoutGame>(e, GAME_BREAKOUT, st, s, "sdqn_env_set_state_breakout"); if (rc) return rc;
  ARGCHK(BreakoutGame::valid(s), "breakout state out of range (row %d col %d dx %d dy %d paddle %d balls %d terminal %d pad %d bricks 0x%llx)",
         s.row, s.col, s.dx, s.dy, s.paddle, s.balls, s.terminal, s.pad, (unsigned long long)s.bricks);
  e->bs = s; e->frame_ok = false; return SDQN_OK;
}
extern "C" int sdqn_env_get_state_freeway(sdqn_env_t e, sdqn_env_state_freeway* st) {
  return env_get_state<FreewayGame>(e, GAME_FREEWAY, st, "sdqn_env_get_state_freeway");
}
extern "C" int sdqn_env_set_state_freeway(sdqn_env_t e, const sdqn_env_state_freeway* st) {
  FreewayState s; int rc = env_state_checked<FreewayGame>(e, GAME_FREEWAY, st, s, "sdqn_env_set_state_freeway"); if (rc) return rc;
  ARGCHK(FreewayGame::valid(s), "freeway state out of range (row %d ticks %d crossings %d terminal %d pad %d %d cars 0x%llx timers 0x%llx periods 0x%llx)",
         s.row, s.ticks, s.crossings, s.terminal, s.pad0, s.pad1, (unsigned long long)s.cars, (unsigned long long)s.timers, (unsigned long long)s.periods);
  e->fs = s; e->frame_ok = false; return SDQN_OK;
}
// the dynamics of the handle.  sdqn_env_eval / sdqn_env_collect play their copies under the handle's frame_skip and p;
// (get_state, get_dynamics) -> (set_state, set_dynamics_state) reproduces a game exactly.
extern "C" int sdqn_env_set_dynamics(sdqn_env_t e, int frame_skip, double repeat_action_probability) {
  ARGCHK(e, "NULL handle");
  ARGCHK(frame_skip >= 1 && frame_skip <= DYNAMICS_MAX_SKIP, "frame_skip %d out of range [1, %d]", frame_skip, DYNAMICS_MAX_SKIP);
  ARGCHK(repeat_action_probability >= 0.0 && repeat_action_probability < 1.0, "repeat_action_probability %g out of range [0, 1)", repeat_action_probability);   // (a NaN fails both)
  e->frame_skip = frame_skip; e->p = repeat_action_probability; e->thresh_p = (uint64_t)ceil(ldexp(repeat_action_probability, 53));
  return SDQN_OK;
}
extern "C" int sdqn_env_get_dynamics(sdqn_env_t e, int* frame_skip, double* repeat_action_probability, int* prev_action, uint64_t* sticky_rng) {
  ARGCHK(e, "NULL handle");
  if (frame_skip) *frame_skip = e->frame_skip; if (repeat_action_probability) *repeat_action_probability = e->p;
  if (prev_action) *prev_action = e->prev; if (sticky_rng) *sticky_rng = e->sticky_rng;
  return SDQN_OK;
}
template <class G> static int env_set_dynamics_state(sdqn_env_s* e, int prev_action, uint64_t sticky_rng) {
  ARGCHK(prev_action >= 0 && prev_action < G::ACTIONS, "prev_action %d out of range [0, %d)", prev_action, G::ACTIONS);
  e->prev = prev_action; e->sticky_rng = sticky_rng;
  return SDQN_OK;
}
extern "C" int sdqn_env_set_dynamics_state(sdqn_env_t e, int prev_action, uint64_t sticky_rng) {
  ARGCHK(e, "NULL handle");
  return GAME_CALL(e, env_set_dynamics_state, e, prev_action, sticky_rng);
}
// test hook: the frame of the current state as the KERNEL renders it (device scratch, read back; sync)
template <class G> static int env_render_device(sdqn_env_s* e, uint8_t* screen) {
  const size_t frame = e->frame.size();
  uint8_t* d = nullptr;
  HIPCHK(hipMalloc((void**)&d, frame));
  hipError_t err = Kernels<G>::render(G::view(e->st<G>()), d, nullptr, e->H, e->W, g_stream);
  if (err == hipSuccess) err = hipMemcpyAsync(screen, d, frame, hipMemcpyDeviceToHost, g_stream);
  if (err == hipSuccess) err = hipStreamSynchronize(g_stream);
  hipFree(d);
  HIPCHK(err);
  return SDQN_OK;
}
extern "C" int sdqn_env_render_device(sdqn_env_t e, uint8_t* screen) {
  ARGCHK(e && screen, "NULL argument");
  STREAMCHK();
  return GAME_CALL(e, env_render_device, e, screen);
}

// One environment transition in one call, the sibling of sdqn_net_act_step for an environment that lives in the library: the host advances
// the game and renders the new frame into the host mirrors (state-buffer window, pinned ring slot); ONE launch renders the same frame
// from the same view into the state buffer's device slot and the ring mirror's slot.  No frame bytes cross PCIe; everything
// else an add does (metadata, count / current, prioritized bookkeeping, generations, wrap, speculation) is the shared code of the add paths.
template <class G>
static int act_step_env(sdqn_net_t h, sdqn_statebuf_t sb, sdqn_replay_t r, sdqn_env_t e, int action, int speculate, int* reward, int* terminal) {
  ARGCHK(action >= 0 && action < G::ACTIONS, "action %d out of range [0, %d)", action, G::ACTIONS);
  ARGCHK(!r || !r->lanes, "a laned replay memory (sdqn_replay_set_lanes) is written by sdqn_env_collect only");
  const int64_t FRAME = (int64_t)e->H * e->W;
  ARGCHK(sb->frame == FRAME, "the state buffer's screens (%lld bytes) and the environment's (%lld) differ", (long long)sb->frame, (long long)FRAME);
  ARGCHK(!r || r->frame == FRAME, "the replay memory's screens (%lld bytes) and the environment's (%lld) differ", (long long)(r ? r->frame : 0), (long long)FRAME);
  typename G::State& st = e->st<G>();
  const int rew = env_advance<G>(e, action), term = st.terminal;
  const typename G::View v = G::view(st);
  uint8_t *hf, *dv;
  int rc = statebuf_advance(sb, &hf, &dv); if (rc) return rc;
  G::render(v, hf, e->H, e->W);
  memcpy(e->frame.data(), hf, (size_t)FRAME); e->frame_ok = true;
  int64_t c = -1; uint8_t* ring_slot = nullptr;
  if (r) {
    c = replay_add_meta(r, action, rew, term);
    memcpy(r->screens + c * FRAME, hf, (size_t)FRAME);
    if (!(r->flags & SDQN_REPLAY_ZERO_COPY)) ring_slot = r->d_ring + c * FRAME;      // (zero copy: the pinned ring IS what the kernels read)
  }
  HIPCHK(Kernels<G>::render(v, dv, ring_slot, e->H, e->W, g_stream));
  if (r) { rc = replay_add_commit(r, c); if (rc) return rc; }
  if (reward) *reward = rew; if (terminal) *terminal = term;
  if (speculate && !term && !h->gen && (size_t)sb->hist * sb->frame == (size_t)STATE) return predict_state_enqueue(h, sb);   // (a terminal step: the episode restarts, nobody wants this state's Q-values)
  return SDQN_OK;
}
extern "C" int sdqn_net_act_step_env(sdqn_net_t h, sdqn_statebuf_t sb, sdqn_replay_t r, sdqn_env_t e, int action, int speculate,
                                     int* reward, int* terminal) {
  ARGCHK(h && sb && e, "NULL argument");
  return GAME_CALL(e, act_step_env, h, sb, r, e, action, speculate, reward, terminal);
}

// ---- the game loops (sdqn_env_eval, sdqn_env_collect): N copies of the game played by the online net, epsilon-greedy, entirely on the
// device.  Per lockstep the predict forward (predict_forward) on the [batch][hist][H][W] window buffer, then ONE launch of the game's
// kernel; two window buffers alternate (read one, write the other).  Nothing returns to the host inside a loop; one stream synchronisation
// at the end.  Shared: what follows.  Per loop: seeding or resuming, whose buffers the copies live in, ring copies, epsilon schedule.
struct EnvOut {                // the callers' output arrays: five tallies [N] (each optional), the trace [locksteps][N] ([A]) (all four or none)
  int64_t *steps, *reward, *caught, *missed, *episodes;
  uint8_t* tr_actions; int8_t* tr_rewards; uint8_t* tr_terminals; double* tr_q;
  bool trace() const { return tr_actions || tr_rewards || tr_terminals || tr_q; }
};
struct EnvGeom { int hist, H, W; size_t state, half; };      // the network's state geometry; half: one window buffer (rows N .. batch_size - 1 stay zero: the forward runs the full batch)
template <class G>
static int env_check(sdqn_net_t h, sdqn_env_t e, int N, double epsilon, const EnvOut& o, EnvGeom& g) {
  g.hist = h->gen ? h->cfg.history_length : C0; g.H = h->gen ? h->cfg.screen_height : H0; g.W = h->gen ? h->cfg.screen_width : W0;
  g.state = (size_t)g.hist * g.H * g.W; g.half = (size_t)h->B * g.state;
  ARGCHK(e->H == g.H && e->W == g.W, "the environment's screen (%d x %d) and the network's (%d x %d) differ", e->H, e->W, g.H, g.W);
  ARGCHK(h->A == net_outputs(h->opt, G::ACTIONS), "the network has %d actions, %s has %d", game_actions(h), G::NAME, G::ACTIONS);
  ARGCHK(N >= 1 && N <= h->B, "num_envs %d out of range [1, batch_size %d]", N, h->B);
  ARGCHK(epsilon >= 0.0 && epsilon <= 1.0, "epsilon %g out of range [0, 1]", epsilon);
  ARGCHK(!o.trace() || (o.tr_actions && o.tr_rewards && o.tr_terminals && o.tr_q), "the trace buffers come together: all four or none");
  return SDQN_OK;
}
struct DevMem {                // device memory of one call
  void* p = nullptr; ~DevMem() { hipFree(p); }
  int alloc(size_t bytes) { HIPCHK(hipMalloc(&p, bytes)); return SDQN_OK; }
};
// the trace of one call: device buffers for `rows` locksteps of N copies (none when the caller wants no trace), wired into the launch
// arguments, read back into the caller's arrays behind the loop
struct EnvTrace {
  DevMem small, q; size_t tn = 0, qbytes = 0;
  int begin(const EnvOut& o, int64_t rows, int N, int A, EvalArgs& a) {
    tn = o.trace() ? (size_t)rows * N : 0; qbytes = tn * A * sizeof(double);
    if (!tn) return SDQN_OK;
    int rc = small.alloc(3 * tn); if (rc) return rc;
    rc = q.alloc(qbytes); if (rc) return rc;
    a.tr_act = static_cast<uint8_t*>(small.p); a.tr_rew = reinterpret_cast<int8_t*>(a.tr_act + tn); a.tr_term = a.tr_act + 2 * tn; a.tr_q = static_cast<double*>(q.p);
    return SDQN_OK;
  }
  int read_back(const EnvOut& o, const EvalArgs& a) {
    if (!tn) return SDQN_OK;
    HIPCHK(hipMemcpyAsync(o.tr_actions, a.tr_act, tn, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(o.tr_rewards, a.tr_rew, tn, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(o.tr_terminals, a.tr_term, tn, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(o.tr_q, a.tr_q, qbytes, hipMemcpyDeviceToHost, g_stream));
    return SDQN_OK;
  }
};
// --bootstrap_heads K > 1: one launch behind the forward reduces its [N][K A] rows to the [N][A] acting rows the game's
// kernel reads — the episode's Q-head per copy (collecting; the episode counters are read from the records) or the vote counts (evaluating).
// K = 1: nothing is launched, the kernel reads the forward's rows.
template <class G>
static int env_select(sdqn_net_t h, EvalArgs& a, int vote) {
  if (output_multiplier(h->opt) == 1 && !h->opt.dueling) return SDQN_OK;
  if (!h->boot_q) { int rc = dalloc(h, &h->boot_q, (size_t)h->B * MAX_ACTIONS * sizeof(double)); if (rc) return rc; }
  // counted like the game kernel it feeds: collect's lockstep under K_COLLECT, eval's not at all
#define BOOT_SELECT launch_bootstrap_select(a.q, h->boot_q, a.q_f64 != 0, a.N, h->opt.boot_K, a.A, vote, bootstrap_head_seed(h->opt.boot_seed), a.envs, \
                                            sizeof(EvalRec<G>), offsetof(EvalRec<G>, episodes), g_stream)
  // --quantiles N > 1 (refused together with bootstrap heads): the mean over the quantiles, collecting and evaluating alike
#define QUANT_MEAN launch_quantile_mean(a.q, h->boot_q, a.q_f64 != 0, a.N, h->opt.quant_N, a.A, g_stream)
  // --dueling (refused together with both): Q = V + Adv - mean(Adv), collecting and evaluating alike
#define DUEL_Q launch_dueling_q(a.q, h->boot_q, a.q_f64 != 0, a.N, a.A, g_stream)
  if (h->opt.dueling) { if (vote) HIPCHK(DUEL_Q); else LAUNCH(K_COLLECT, DUEL_Q); }
  else if (h->opt.quant_N > 1) { if (vote) HIPCHK(QUANT_MEAN); else LAUNCH(K_COLLECT, QUANT_MEAN); }
#undef DUEL_Q
  else if (vote) HIPCHK(BOOT_SELECT); else LAUNCH(K_COLLECT, BOOT_SELECT);
#undef QUANT_MEAN
#undef BOOT_SELECT
  a.q = h->boot_q;
  return SDQN_OK;
}
static EvalArgs env_args(sdqn_net_t h, sdqn_env_t e, int N, const EnvGeom& g, void* recs) {
  EvalArgs a; memset(&a, 0, sizeof a);
  a.A = game_actions(h); a.N = N; a.hist = g.hist; a.H = g.H; a.W = g.W; a.bpe = e->bpe; a.envs = recs;
  a.frame_skip = e->frame_skip; a.thresh_p = e->thresh_p;
  return a;
}
// the host copy of the records -> the callers' tallies
template <class G>
static void env_tallies(const std::vector<EvalRec<G> >& hrec, const EnvOut& o) {
  for (size_t i = 0; i < hrec.size(); ++i) {
    if (o.steps) o.steps[i] = hrec[i].steps; if (o.reward) o.reward[i] = hrec[i].reward;
    if (o.caught) o.caught[i] = hrec[i].caught; if (o.missed) o.missed[i] = hrec[i].missed;
    if (o.episodes) o.episodes[i] = hrec[i].episodes;
  }
}

// sdqn_env_eval: the copies live in buffers of this call, seeded from `seed`; one epsilon.  The environment handle gives the geometry,
// balls_per_episode and the dynamics (frame_skip, repeat_action_probability); its own state is not touched.
template <class G>
static int env_eval(sdqn_net_t h, sdqn_env_t e, int N, int64_t steps, double epsilon, uint64_t seed, const EnvOut& o) {
  typedef EvalRec<G> Rec;
  EnvGeom g; int rc = env_check<G>(h, e, N, epsilon, o, g); if (rc) return rc;
  ARGCHK(steps >= 1, "steps %lld < 1", (long long)steps);
  STREAMCHK();
  DevMem win_mem, recs; EnvTrace tr;
  std::vector<Rec> hrec((size_t)N);
  auto body = [&]() -> int {
    int rc = win_mem.alloc(2 * g.half + SRC_PAD); if (rc) return rc;
    uint8_t* win = static_cast<uint8_t*>(win_mem.p);
    HIPCHK(hipMemsetAsync(win, 0, 2 * g.half + SRC_PAD, g_stream));
    rc = recs.alloc((size_t)N * sizeof(Rec)); if (rc) return rc;
    HIPCHK(hipMemsetAsync(recs.p, 0, (size_t)N * sizeof(Rec), g_stream));
    EvalArgs a = env_args(h, e, N, g, recs.p);
    rc = tr.begin(o, steps, N, a.A, a); if (rc) return rc;
    a.seed = seed; a.thresh = (uint64_t)ceil(ldexp(epsilon, 53));
    a.init = 1; a.src = win + g.half; a.dst = win;
    HIPCHK(Kernels<G>::eval(a, g_stream));
    a.init = 0;
    for (int64_t t = 0; t < steps; ++t) {
      const uint8_t* cur = win + (size_t)(t & 1) * g.half;
      rc = predict_forward(h, cur, N, &a.q, &a.q_f64); if (rc) return rc;
      rc = env_select<G>(h, a, 1); if (rc) return rc;
      a.t = t; a.src = cur; a.dst = win + (size_t)((t + 1) & 1) * g.half;
      HIPCHK(Kernels<G>::eval(a, g_stream));
    }
    HIPCHK(hipMemcpyAsync(hrec.data(), recs.p, (size_t)N * sizeof(Rec), hipMemcpyDeviceToHost, g_stream));
    rc = tr.read_back(o, a); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g_stream));
    return SDQN_OK;
  };
  rc = body();
  if (rc) { if (g_stream) hipStreamSynchronize(g_stream); return rc; }
  env_tallies<G>(hrec, o);
  return SDQN_OK;
}

extern "C" int sdqn_env_eval(sdqn_net_t h, sdqn_env_t e, int N, int64_t steps, double epsilon, uint64_t seed,
                             int64_t* out_steps, int64_t* out_reward, int64_t* out_caught, int64_t* out_missed, int64_t* out_episodes,
                             uint8_t* tr_actions, int8_t* tr_rewards, uint8_t* tr_terminals, double* tr_q) {
  ARGCHK(h && e, "NULL argument");
  const EnvOut o = {out_steps, out_reward, out_caught, out_missed, out_episodes, tr_actions, tr_rewards, tr_terminals, tr_q};
  return GAME_CALL(e, env_eval, h, e, N, steps, epsilon, seed, o);
}

// --train_envs: `locksteps` locksteps of num_envs copies of the game, each lockstep num_envs transitions written into the
// laned ring r by ONE launch of the game's collect kernel behind the predict forward (no forward while epsilon >= 1: no Q row is
// read).  The copies' records and the two window buffers live on the net handle: seed >= 0 seeds the copies as sdqn_env_eval does and
// renders their first frames, seed < 0 goes on where the last call stopped.  Lockstep t of the call plays with
// epsilon = clamp(epsilon_start + t epsilon_step, 0, 1).  Per lockstep two strided device-to-host copies bring the num_envs frames and
// MetaRecs into the pinned master, which stays a true copy of the mirror; nothing goes host to device and nothing waits until the single
// synchronisation at the end, after which actions / rewards / terminals are unpacked.  Tallies: the copies' running sums since they were seeded.
template <class G>
static int env_collect(sdqn_net_t h, sdqn_env_t e, sdqn_replay_t r, int N, int64_t locksteps, double epsilon_start, double epsilon_step,
                       int64_t seed, const EnvOut& o) {
  typedef EvalRec<G> Rec;
  EnvGeom g; int rc = env_check<G>(h, e, N, epsilon_start, o, g); if (rc) return rc;
  ARGCHK(r->H == g.H && r->W == g.W && r->hist == g.hist, "the replay memory's geometry (%d x %d, history %d) and the network's (%d x %d, %d) differ", r->H, r->W, r->hist, g.H, g.W, g.hist);
  ARGCHK(r->lanes == N, "the replay memory has %d lanes, num_envs is %d (sdqn_replay_set_lanes)", r->lanes, N);
  ARGCHK(locksteps >= 0, "locksteps %lld < 0", (long long)locksteps);
  ARGCHK(seed >= 0 || (h->col_recs && h->col_N == N && h->col_state == g.state && h->col_game == e->game),
         "nothing to resume: the copies were never seeded for %d environments of %s", N, G::NAME);
  STREAMCHK();
  if (!h->col_win) {
    rc = dalloc(h, (void**)&h->col_win, 2 * g.half + SRC_PAD); if (rc) return rc;
    rc = dalloc(h, &h->col_recs, (size_t)h->B * std::max(std::max(sizeof(EvalRec<CatchGame>), sizeof(EvalRec<BreakoutGame>)), sizeof(EvalRec<FreewayGame>))); if (rc) return rc;    // (any game's records)
  }
  const int64_t FRAME = r->frame, L = r->lane_len;
  EnvTrace tr;
  std::vector<Rec> hrec((size_t)N);
  int64_t p = r->lane_pos, f = r->lane_fill, launched = 0;
  auto body = [&]() -> int {
    EvalArgs a = env_args(h, e, N, g, h->col_recs);
    int rc = tr.begin(o, locksteps, N, a.A, a); if (rc) return rc;
    CollectArgs c; c.ring = r->d_ring; c.meta = r->d_meta; c.lane_len = L; c.pos = p;
    if (seed >= 0) {
      HIPCHK(hipMemsetAsync(h->col_win, 0, 2 * g.half + SRC_PAD, g_stream));
      a.seed = (uint64_t)seed; a.init = 1; a.src = h->col_win + g.half; a.dst = h->col_win;
      HIPCHK(Kernels<G>::collect(a, c, g_stream, false));
      a.init = 0; h->col_t = 0; h->col_N = N; h->col_state = g.state; h->col_game = e->game;
    }
    for (int64_t t = 0; t < locksteps; ++t) {
      const int64_t T = h->col_t;
      const uint8_t* cur = h->col_win + (size_t)(T & 1) * g.half;
      double eps = epsilon_start + (double)t * epsilon_step;
      eps = eps < 0.0 ? 0.0 : (eps > 1.0 ? 1.0 : eps);
      a.q = nullptr;
      // (--noisy_nets: collecting reads the effective weights — the current parameters under the last train step's noise; evaluating reads mu)
      if (eps < 1.0) { rc = noisy_fresh(h); if (rc) return rc; rc = predict_forward(h, cur, N, &a.q, &a.q_f64, true); if (rc) return rc; rc = env_select<G>(h, a, 0); if (rc) return rc; }
      a.thresh = (uint64_t)ceil(ldexp(eps, 53));
      a.t = t; a.src = cur; a.dst = h->col_win + (size_t)((T + 1) & 1) * g.half;
      c.pos = p;
      LAUNCH(K_COLLECT, Kernels<G>::collect(a, c, g_stream, true));
      h->col_t = T + 1;
      // the lockstep's N slots, one per lane, L slots apart: one strided copy of the frames and one of the MetaRecs
      HIPCHK(hipMemcpy2DAsync(r->screens + p * FRAME, (size_t)L * FRAME, r->d_ring + p * FRAME, (size_t)L * FRAME, (size_t)FRAME, (size_t)N,
                              hipMemcpyDeviceToHost, g_stream));
      HIPCHK(hipMemcpy2DAsync(r->h_meta + p, (size_t)L * sizeof(MetaRec), r->d_meta + p, (size_t)L * sizeof(MetaRec), sizeof(MetaRec), (size_t)N,
                              hipMemcpyDeviceToHost, g_stream));
      p = (p + 1) % L; if (f < L) ++f;
      ++launched;
    }
    HIPCHK(hipMemcpyAsync(hrec.data(), h->col_recs, (size_t)N * sizeof(Rec), hipMemcpyDeviceToHost, g_stream));
    rc = tr.read_back(o, a); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g_stream));
    return SDQN_OK;
  };
  rc = body();
  if (rc && g_stream) hipStreamSynchronize(g_stream);
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
  env_tallies<G>(hrec, o);
  return SDQN_OK;
}
extern "C" int sdqn_env_collect(sdqn_net_t h, sdqn_env_t e, sdqn_replay_t r, int N, int64_t locksteps, double epsilon_start, double epsilon_step,
                                int64_t seed, int64_t* out_steps, int64_t* out_reward, int64_t* out_caught, int64_t* out_missed,
                                int64_t* out_episodes, uint8_t* tr_actions, int8_t* tr_rewards, uint8_t* tr_terminals, double* tr_q) {
  ARGCHK(h && e && r, "NULL argument");
  const EnvOut o = {out_steps, out_reward, out_caught, out_missed, out_episodes, tr_actions, tr_rewards, tr_terminals, tr_q};
  return GAME_CALL(e, env_collect, h, e, r, N, locksteps, epsilon_start, epsilon_step, seed, o);
}

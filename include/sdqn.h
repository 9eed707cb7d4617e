/* sdqn.h — C ABI of libsdqn_hip.so: the MI355X (gfx950) DQN training-step hot path.
 *
 * The reference (tambetm/simple_dqn) has no FFI of its own: its boundary for this
 * path is the duck-typed Python API of two classes.  Each entry point below names
 * the reference interface (file:line under /root/reference) that it replaces; the
 * ctypes binding that turns them back into those classes is
 * simple_dqn_amd/_lib.py.
 *
 * Conventions
 *   - every function returns 0 on success, a negative sdqn_status on failure;
 *     sdqn_last_error() returns a thread-local message for the last failure.
 *     No exception crosses the boundary.
 *   - handles are opaque, owned by the library, single-owner (not thread-safe),
 *     matching the reference's single-threaded caller (src/agent.py:96-116).
 *   - every device operation is enqueued on ONE library stream per process and is
 *     asynchronous unless the call returns host data (then it synchronises).
 *   - host pointers passed in are borrowed for the duration of the call only;
 *     pointers handed out (sdqn_replay_host_ptrs) live as long as the handle.
 *   - there is NO CPU fallback: without a gfx950 device every device entry point
 *     fails with SDQN_ERR_HIP.
 */
#ifndef SDQN_H
#define SDQN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  SDQN_OK = 0,
  SDQN_ERR_ARG = -1,     /* precondition / shape violation: the reference raises AssertionError */
  SDQN_ERR_HIP = -2,     /* HIP runtime failure (incl. "no device") */
  SDQN_ERR_RCCL = -3,    /* RCCL failure */
  SDQN_ERR_STATE = -4    /* call not valid in the handle's current state */
} sdqn_status;

typedef struct sdqn_replay_s* sdqn_replay_t;
typedef struct sdqn_net_s* sdqn_net_t;

#define SDQN_MT_WORDS 625          /* CPython random.getstate()[1]: 624 state words + position */

/* ---- misc ---------------------------------------------------------------- */
const char* sdqn_last_error(void);
int sdqn_version(void);
int sdqn_device_count(int* n);
/* replaces --device_id (src/main.py:52 -> gen_backend(device_id=...), deepqnetwork.py:29-34).  One device per process:
 * the first device call binds the library; asking for the bound device again is a no-op, any other device afterwards
 * is SDQN_ERR_STATE (never a silent run on the wrong GPU). */
int sdqn_set_device(int dev);
int sdqn_get_device(int* dev);                /* the device the library is bound to (binds the current one if none yet) */
int sdqn_device_sync(void);

/* ---- index sampler: pure host, no device needed ---------------------------
 * replaces the rejection sampler in ReplayMemory.getMinibatch, src/replay_memory.py:54-68,
 * bit-exact against CPython 3.10's random.randint stream (Lib/random.py randint ->
 * _randbelow_with_getrandbits; Modules/_randommodule.c genrand_uint32).               */
int sdqn_mt_seed(uint32_t mt[SDQN_MT_WORDS], uint64_t seed);            /* random.seed(int), src/main.py:89-90 */
int sdqn_mt_randint(uint32_t mt[SDQN_MT_WORDS], int64_t a, int64_t b, int64_t* out);
int sdqn_sample_indices(uint32_t mt[SDQN_MT_WORDS], const uint8_t* terminals, int64_t count,
                        int64_t current, int history_length, int batch,
                        int64_t* idx_out /*[batch]*/, int64_t* draws_out /*nullable*/);
/* --n_step: the same rejection loop for n-step transitions — index = randint(history_length, count - n), rejected when
 * the window [index - history_length, index + n - 1] straddles `current` or terminals[index - history_length : index] holds a terminal;
 * n = 1 is sdqn_sample_indices draw for draw.  count < history_length + n is SDQN_ERR_ARG. */
#define SDQN_MAX_N_STEP 16
int sdqn_sample_indices_n(uint32_t mt[SDQN_MT_WORDS], const uint8_t* terminals, int64_t count, int64_t current,
                          int history_length, int n, int batch, int64_t* idx_out /*[batch]*/, int64_t* draws_out /*nullable*/);
/* --train_envs: the rule for a LANED ring — `lanes` rings of lane_len slots side by side (lane e = slots
 * [e lane_len, (e + 1) lane_len)) that share one fill f and one write position p.  span = f - n - history_length + 1 valid local
 * positions per lane; per attempt ONE draw r = randint(0, lanes span - 1), lane r / span, local l = history_length + r % span,
 * index lane lane_len + l; rejected when l + n - 1 >= p && l - history_length < p (the window straddles the write position) or
 * terminals[index - history_length : index] holds a terminal.  A window never crosses a lane edge.  SDQN_ERR_ARG for lanes < 1,
 * lane_len < history_length + n + 2, f > lane_len, p >= lane_len, span <= 0 and lanes without an admissible index. */
int sdqn_sample_indices_lanes(uint32_t mt[SDQN_MT_WORDS], const uint8_t* terminals, int lanes, int64_t lane_len, int64_t fill, int64_t pos,
                              int history_length, int n, int batch, int64_t* idx_out /*[batch]*/, int64_t* draws_out /*nullable*/);

/* ---- replay memory: src/replay_memory.py ---------------------------------- */
#define SDQN_REPLAY_HBM_MIRROR 1   /* ring master in pinned host DRAM + mirror in HBM (default) */
#define SDQN_REPLAY_ZERO_COPY  2   /* no mirror: kernels read the pinned ring over PCIe */

/* ReplayMemory.__init__, replay_memory.py:7-24 */
int sdqn_replay_create(sdqn_replay_t* h, int64_t size, int screen_height, int screen_width,
                       int history_length, int batch_size, int flags);
int sdqn_replay_destroy(sdqn_replay_t h);
/* the numpy attributes screens/actions/rewards/terminals (replay_memory.py:10-13) are views of these */
int sdqn_replay_host_ptrs(sdqn_replay_t h, uint8_t** screens, uint8_t** actions, int64_t** rewards,
                          uint8_t** terminals);
/* preallocated minibatch outputs prestates/poststates (replay_memory.py:21-22) + a/r/t, pinned host */
int sdqn_replay_minibatch_ptrs(sdqn_replay_t h, uint8_t** pre, uint8_t** post, uint8_t** actions,
                               int64_t** rewards, uint8_t** terminals);
/* ReplayMemory.add, replay_memory.py:26-34 (also enqueues the 7 KB H2D into the mirror) */
int sdqn_replay_add(sdqn_replay_t h, int action, int64_t reward, const uint8_t* screen, int terminal);
int sdqn_replay_get_state(sdqn_replay_t h, int64_t* count, int64_t* current);
int sdqn_replay_set_state(sdqn_replay_t h, int64_t count, int64_t current);
/* after writing the host views directly (bulk fill): copy slots [first, first+n) into the mirror */
int sdqn_replay_upload(sdqn_replay_t h, int64_t first, int64_t n);
/* the same for the packed metadata only (actions / rewards / terminals edited in place: 16 B per slot instead of 7 KB) */
int sdqn_replay_upload_meta(sdqn_replay_t h, int64_t first, int64_t n);
/* replay_memory.py:54-68 on this ring (terminals/count/current of the handle).  On a prioritized handle: the stratified draw by priority
 * (below), 2 x batch MT words per call, draws_out = batch; the sample's importance weights stay on the device for the train step */
int sdqn_replay_sample(sdqn_replay_t h, uint32_t mt[SDQN_MT_WORDS], int64_t* idx_out, int64_t* draws_out);
/* --n_step n (1..16): sampling follows sdqn_sample_indices_n, and every gather of this handle (sdqn_replay_gather and the
 * train paths' own) takes the poststate of sample i from state(i + n - 1) and turns (rewards, terminals)[i .. i + n - 1] into the return
 * R = sum_k gamma^k clip(r_{i+k}) up to and including the first terminal, and done = "a terminal was met".  sdqn_replay_gather leaves R
 * (float64 bits) where the rewards go and done where the terminals go.  A train call refuses a memory whose (n, discount, min_reward,
 * max_reward) differ from the network's (option "n_step" and its configuration).  n = 1: the standard memory. */
int sdqn_replay_set_n_step(sdqn_replay_t h, int n, double discount, double min_reward, double max_reward);
/* --train_envs: cut the ring into `lanes` rings of L = size / lanes slots that sdqn_env_collect fills in lockstep, one
 * episode stream per lane.  Only on an empty memory with the HBM mirror that is not prioritized; lanes must divide size and
 * L >= history_length + n_step + 2 (else SDQN_ERR_ARG).  From then on sampling follows sdqn_sample_indices_lanes; sdqn_replay_add,
 * sdqn_net_act_step*, sdqn_replay_set_state and sdqn_replay_enable_priorities are SDQN_ERR_ARG; sdqn_replay_get_state reports
 * count = lanes x fill and current = the lanes' write position.  sdqn_replay_get_lanes: (lanes, L, fill, position), lanes = 0 for a
 * memory without lanes (any pointer may be NULL). */
int sdqn_replay_set_lanes(sdqn_replay_t h, int lanes);
int sdqn_replay_get_lanes(sdqn_replay_t h, int* lanes, int64_t* lane_len, int64_t* fill, int64_t* pos);

/* ---- prioritized experience replay (Schaul et al. 2016, proportional) -------------------------------------------------
 * P(i) = p_i / sum of p_j over the indexes the reference sampler accepts; sample n of a batch of B draws u_n = random.random() and takes
 * the leaf whose prefix interval holds (n + u_n) S / B.  p_i = (|delta_i| + epsilon)^alpha of the unclipped TD error of the taken
 * action; (re)written ring slots get p_max, the largest priority ever written (initially 1).  The train step weights the taken action's
 * row by w_n = (p_n / min_m p_m)^-beta (batch-max normalised).  train_many / train_many_deferred / train_replay, and train_host on the
 * memory's own minibatch gathered from its last sdqn_replay_sample, train with the weights and write the new priorities back; a foreign
 * tuple trains unweighted.  Every datatype and geometry.  A sampled action out of range or a non-finite TD error is SDQN_ERR_ARG
 * from the next synchronising call (these entry points, a train call returning its cost, sdqn_net_sync, sdqn_net_cost_collect). */
/* switch the handle to prioritized sampling, every priority (and p_max) = 1.0; again: reset.  SDQN_ERR_ARG without the HBM mirror,
 * alpha < 0, epsilon <= 0, batch > 256 */
int sdqn_replay_enable_priorities(sdqn_replay_t h, double alpha, double epsilon);
/* importance-sampling exponent of the following train steps, 0 <= beta <= 1 (default 0.4) */
int sdqn_replay_set_priority_beta(sdqn_replay_t h, double beta);
/* raw priorities of slots [first, first + n) (finite, > 0; p_max follows); sync */
int sdqn_replay_set_priorities(sdqn_replay_t h, int64_t first, int64_t n, const float* values);
/* the tree's leaves of slots [first, first + n): raw priority x valid (0 for an index the sampler cannot return); sync */
int sdqn_replay_get_priorities(sdqn_replay_t h, int64_t first, int64_t n, float* out);
/* p_max; sync */
int sdqn_replay_get_max_priority(sdqn_replay_t h, float* out);
/* the last prioritized batch (sdqn_replay_sample or a train step's own sample): indexes [batch] and weights [batch], either nullable; sync */
int sdqn_replay_last_sample(sdqn_replay_t h, int64_t* idx_out, float* w_out);
/* replay_memory.py:71-78: HIP gather of (s, a, r, s', terminal) by index into device HBM (async) */
int sdqn_replay_gather(sdqn_replay_t h, const int64_t* idx_host /*[batch]*/);
/* replay_memory.py:79: the device minibatch copied into the buffers of sdqn_replay_minibatch_ptrs (sync) */
int sdqn_replay_minibatch_to_host(sdqn_replay_t h);
/* One-shot declaration by the caller of sdqn_net_train_host: "the pinned prestates / poststates buffers of this handle
 * (sdqn_replay_minibatch_ptrs) still hold what the last sdqn_replay_minibatch_to_host wrote — I have not modified them".  If that
 * call is then made on exactly those buffers and no other gather has run since, the step reads the device copy of the minibatch in
 * place and uploads only the 10 x batch_size bytes of (rewards, actions, terminals).  Never required for correctness: without it
 * (C callers that write into the buffers, arrays from elsewhere) the states are uploaded as before.  simple_dqn_amd's
 * ReplayMemory exposes the two buffers as write-tracking numpy views and declares this only while they are untouched. */
int sdqn_replay_declare_minibatch_clean(sdqn_replay_t h);
/* replay_memory.py:79 without the wait (round 5): the reference's getMinibatch() returns arrays; most callers hand them straight back
 * to DeepQNetwork.train (agent.py:112-114) and never read the 1.8 MB of states on the host.  sdqn_replay_minibatch_gen reports the
 * generation of the device minibatch (bumped by every gather launch) and of the host copy (set by sdqn_replay_minibatch_to_host), so a
 * host binding can hand out LAZY state arrays and fetch them only when somebody looks.  sdqn_replay_declare_minibatch_on_device is the
 * one-shot declaration for that case: "the two state arguments of the next sdqn_net_train_host stand for device minibatch `gen` — the
 * host buffers may not hold it yet, and I have not written into them".  Honoured only while `gen` still IS the device minibatch's
 * generation (gen = 0: whatever it holds now — the reference's aliased buffers always show the latest gather); otherwise the call uploads
 * the host buffers as always.  gen = UINT64_MAX names the minibatch of the LAST sdqn_replay_gather and is for a caller that has not
 * fetched it: SDQN_ERR_STATE if another launch has overwritten the device minibatch since (round 6: those states exist nowhere).  rewards / actions / terminals always come from the arguments — compared by value with what that gather
 * left on the device (ring[idx] of the three arrays, snapshotted by sdqn_replay_gather): when they are equal the step reads the device
 * copy and the call uploads nothing; any edit (a clipped reward, another action) is uploaded and used, as before. */
int sdqn_replay_minibatch_gen(sdqn_replay_t h, uint64_t* device_gen, uint64_t* host_gen);
int sdqn_replay_declare_minibatch_on_device(sdqn_replay_t h, uint64_t gen);
/* device-side timing of the last n gather launches, for bench.py (HIP events on the library stream) */
int sdqn_replay_bench_gather(sdqn_replay_t h, const int64_t* idx_host, int iters, float* ms_per_launch);
/* the same with a different index set per launch (idx_host = nsets x batch_size, cycled): a repeated set is served from L2 / MALL
 * after its first launch, getMinibatch() (replay_memory.py:54-79) never gathers the same states twice in a row */
int sdqn_replay_bench_gather_sets(sdqn_replay_t h, const int64_t* idx_host, int nsets, int iters, float* ms_per_launch);

/* ---- Q-network: src/deepqnetwork.py ---------------------------------------- */
typedef struct {
  int batch_size;          /* args.batch_size      deepqnetwork.py:19 */
  int history_length;      /* args.history_length  :21 (main.py:34).  84 x 84 x 4 runs on the tuned kernels; any other    */
  int screen_height;       /* :22 (main.py:28)      geometry the layer stack of :83-91 accepts runs on the generic    */
  int screen_width;        /* :22 (main.py:27)      im2col + GEMM path (csrc/generic_net.hip): float32 / float64 only */
  int num_actions;         /* :18 */
  int target_enabled;      /* bool(args.target_steps) :64 */
  int optimizer;           /* args.optimizer :50-59: 0 rmsprop, 1 adam, 2 adadelta */
  int datatype;            /* args.datatype :33 (main.py:53): 0 float32; 1 float16 = half activations/deltas/MFMA weight operands,
                              fp32 accumulation, master weights and optimizer state (BASELINE.json configs[4]);
                              2 float64 = the whole step in double (generic path) */
  /* Python floats (doubles) exactly as argparse hands them over; the library rounds to fp32
   * where Neon's fp32 backend would (lr, decay, epsilon, clip) and keeps doubles where the
   * reference does host-side float math (discount, reward clip: deepqnetwork.py:136-143).  */
  double discount_rate;    /* :20 */
  double clip_error;       /* :23 (0 disables clipping, :158) */
  double min_reward;       /* :24 */
  double max_reward;       /* :25 */
  double learning_rate;    /* :51 */
  double decay_rate;       /* :52 */
  double epsilon;          /* Neon defaults: RMSProp 1e-6, Adam 1e-8, Adadelta 1e-6 */
  double beta_1;           /* Adam (Neon default 0.9) */
  double beta_2;           /* Adam (Neon default 0.999) */
  double loss_scale;       /* float16 mode: static power-of-two scale of the stored deltas (0 -> 1024) */
  double batch_norm;       /* args.batch_norm :26 (0 / 1): Neon BatchNorm after conv1..3 and fc4 (float32 only) */
} sdqn_net_cfg;

/* DeepQNetwork.__init__, deepqnetwork.py:16-75 (weights start at zero: inject with set_weights) */
int sdqn_net_create(sdqn_net_t* h, const sdqn_net_cfg* cfg);
int sdqn_net_destroy(sdqn_net_t h);
/* which: 0 online theta, 1 target theta-, 2 optimizer state (RMSProp s / Adam m / Adadelta E[g^2]),
 * 3 last gradient sum (get only), 4 second optimizer state (Adam v / Adadelta E[dx^2]).
 * layer: 0..4 = conv1, conv2, conv3, fc4, fc5.  With batch_norm also 5..8 = the BatchNorm layers after conv1, conv2,
 * conv3, fc4: 2*C floats [beta | gamma] (C = 32, 64, 64, 512); for those layers which = 5 / 6 reads or writes the
 * running statistics [gmean | gvar] of the online / target net.  Data in Neon layout:
 * conv (C*R*S, K) rows c*R*S+r*S+s; fc4 (512, 3136) nin in (K,P,Q) order; fc5 (A, 512).  */
int sdqn_net_layer_size(sdqn_net_t h, int layer, int64_t* n);
int sdqn_net_set_weights(sdqn_net_t h, int which, int layer, const float* w, int64_t n);
int sdqn_net_get_weights(sdqn_net_t h, int which, int layer, float* w, int64_t n);   /* sync */
/* the same in double: what a float64 network exchanges without a round trip through float (other networks convert) */
int sdqn_net_set_weights_f64(sdqn_net_t h, int which, int layer, const double* w, int64_t n);
int sdqn_net_get_weights_f64(sdqn_net_t h, int which, int layer, double* w, int64_t n);   /* sync */
/* DeepQNetwork.predict, deepqnetwork.py:174-186: states u8[B,4,84,84] -> q float[B,A] (sync) */
int sdqn_net_predict(sdqn_net_t h, const uint8_t* states, float* q_out);
int sdqn_net_predict_f64(sdqn_net_t h, const uint8_t* states, double* q_out);      /* float64 networks: Q-values in double */
/* acting path: Q-values of ONE state u8[4,84,84] -> float[A].  The reference pads the
 * current state to a full minibatch of zero rows only because Neon cannot change its batch size
 * (src/state_buffer.py:13-24, src/agent.py:55-61) and then uses row 0; this computes exactly that row. */
int sdqn_net_predict_one(sdqn_net_t h, const uint8_t* state, float* q_out);
/* Device-resident StateBuffer (src/state_buffer.py:3-27): the last `hist` screens of the
 * acting agent live in HBM, so each environment step uploads one 7 KB frame instead of a padded minibatch
 * (src/agent.py:55-61 builds u8[B,4,84,84] per step).  A host mirror backs getState()/getStateMinibatch(). */
typedef struct sdqn_statebuf_s* sdqn_statebuf_t;
int sdqn_statebuf_create(sdqn_statebuf_t* out, int screen_height, int screen_width, int history_length);
int sdqn_statebuf_destroy(sdqn_statebuf_t s);
int sdqn_statebuf_add(sdqn_statebuf_t s, const uint8_t* screen);   /* state_buffer.py:15-18: shift left, append */
int sdqn_statebuf_reset(sdqn_statebuf_t s);                         /* state_buffer.py:26-27 */
int sdqn_statebuf_get(sdqn_statebuf_t s, uint8_t* state_out);       /* host mirror copy u8[hist,H,W] (no sync) */
int sdqn_statebuf_read_device(sdqn_statebuf_t s, uint8_t* state_out);   /* test hook: D2H of the device window (sync) */
/* Q-values of the buffered state -> float[A] (sync): sdqn_net_predict_one without the state upload */
int sdqn_net_predict_state(sdqn_net_t h, sdqn_statebuf_t s, float* q_out);
/* agent.py:55-59: greedy action of the buffered state = first index of the maximal Q-value (np.argmax); q_out float[A] nullable */
int sdqn_net_act_greedy(sdqn_net_t h, sdqn_statebuf_t s, int* action, float* q_out);
/* One environment transition in one call (agent.py:48-85: `self.buf.add(screen)` [+ `self.mem.add(action, reward, screen, terminal)`,
 * replay_memory.py:26-34, when `r` is not NULL]); speculate != 0 also enqueues the acting forward of the NEW state, whose Q-values the next
 * sdqn_net_predict_state on the same buffer collects without launching anything (dropped if the buffer or the parameters change first). */
int sdqn_net_act_step(sdqn_net_t h, sdqn_statebuf_t sb, sdqn_replay_t r, const uint8_t* screen, int action, int64_t reward,
                      int terminal, int speculate);
/* Test / measurement hook of the one-launch acting forward (float32, no batch_norm, standard geometry; option "act_kernel"): one blocking
 * forward of the buffered state with per-workgroup phase stamps.  q_out float[A], stamps_out uint64[256][80] ({kind, clock} pairs; the last
 * word of a workgroup's row = its XCC id); either may be NULL. */
int sdqn_net_debug_act(sdqn_net_t h, sdqn_statebuf_t sb, float* q_out, unsigned long long* stamps_out);
/* DeepQNetwork.train, deepqnetwork.py:107-172, minibatch given as host arrays.
 * cost_out nullable: NULL -> the step itself is not waited for.  Buffer contract: when the call returns, all five arrays
 * are free to be overwritten — pageable arrays were copied into a pinned double buffer; pre / post that ARE a
 * ReplayMemory's pinned minibatch buffers (sdqn_replay_minibatch_ptrs) are uploaded in place and the call returns only
 * after that upload has completed (the step's kernels are already enqueued behind it).
 * Threading: handles are created, used and destroyed from ONE host thread (no internal locking). */
int sdqn_net_train_host(sdqn_net_t h, const uint8_t* pre, const uint8_t* actions, const int64_t* rewards,
                        const uint8_t* post, const uint8_t* terminals, float* cost_out);
/* the same step for an n-step tuple (option "n_step" > 1, which sdqn_net_train_host refuses): returns R [batch] float64 (clipped per
 * step already: not clipped again) and dones [batch]; target = R if done else R + discount^n max Q'(post).  The lazy-state and
 * small-array reuse of sdqn_net_train_host apply unchanged (an unedited gather of an n-step memory uploads nothing). */
int sdqn_net_train_host_returns(sdqn_net_t h, const uint8_t* pre, const uint8_t* actions, const double* returns,
                                const uint8_t* post, const uint8_t* dones, float* cost_out);
/* How sdqn_net_train_host has been served on this handle: calls / calls that read the states from the device minibatch in place (no
 * 2 x batch x state H2D) / calls that uploaded nothing at all (small arrays equal to what the gather left on the device).  Any NULL. */
int sdqn_net_tuple_counters(sdqn_net_t h, int64_t* calls, int64_t* states_in_place, int64_t* nothing_uploaded);
/* same step with the minibatch gathered on the device straight from the replay ring:
 * fuses replay_memory.py:71-78 with deepqnetwork.py:94-100 (no u8 minibatch is materialised) */
int sdqn_net_train_replay(sdqn_net_t h, sdqn_replay_t r, const int64_t* idx_host, float* cost_out);
/* n_steps x { sample (replay_memory.py:54-68) ; train } without returning to Python:
 * the loop body of Agent.train, src/agent.py:108-114 */
int sdqn_net_train_many(sdqn_net_t h, sdqn_replay_t r, uint32_t mt[SDQN_MT_WORDS], int n_steps,
                        float* mean_cost /*nullable*/);
/* The same without waiting for the cost (deepqnetwork.py:168-172 when the stats callback can take the cost later): the stream copies the
 * call's cost sum into a pinned ring slot; sdqn_net_cost_collect(ticket) polls it (bounded) and returns the mean cost of the call's steps.
 * A ticket stays valid for 64 further deferred calls. */
int sdqn_net_train_many_deferred(sdqn_net_t h, sdqn_replay_t r, uint32_t mt[SDQN_MT_WORDS], int n_steps, int64_t* ticket);
int sdqn_net_cost_collect(sdqn_net_t h, int64_t ticket, float* mean_cost);
/* 32-bit MT19937 outputs the library has drawn since it was loaded: a caller that handed over a COPY of random.getstate()[1] advances its
 * own generator by the difference (random.getrandbits(32 * words)) instead of importing the 625 words back */
int sdqn_mt_words(uint64_t* words);
/* DeepQNetwork.update_target_network, deepqnetwork.py:102-105 */
int sdqn_net_update_target(sdqn_net_t h);
/* Soft (Polyak) target updates, --target_tau (no reference counterpart).  sdqn_net_soft_update performs ONE blend now,
 * on the library stream:  theta-[e] <- theta-[e] + tau_f * (theta[e] - theta-[e])  with tau_f = (float)tau (the network's precision on
 * the generic path: double for float64), subtraction, product and sum each rounded once, never contracted — numpy reproduces it bit
 * for bit.  It covers everything sdqn_net_update_target copies (with batch_norm: beta / gamma and the running statistics) and leaves
 * the target's derived weight copies what sdqn_net_set_weights(which = 1) would have made them.  tau = 1 is sdqn_net_update_target;
 * tau outside (0, 1] or not finite is SDQN_ERR_ARG; without a target net nothing is launched.
 * sdqn_net_set_target_tau sets the per-step mode: 0 (default) off; tau in (0, 1]: every train step of this net that applies an update
 * — whatever its entry point, sdqn_net_apply_update included, a "grad_only" step excluded — is followed by one such blend, enqueued
 * right behind the step's update launch (+1 launch per step; profile row 27). */
int sdqn_net_soft_update(sdqn_net_t h, double tau);
int sdqn_net_set_target_tau(sdqn_net_t h, double tau);
int sdqn_net_get_target_tau(sdqn_net_t h, double* tau);
/* Global gradient-norm clipping, --clip_grad_norm (no reference counterpart).  max_norm G > 0 switches it on, 0 (default)
 * off; negative, NaN or infinite is SDQN_ERR_ARG and keeps the previous value.  With g the flat gradient SUM buffer the optimizer reads
 * (all layers; with batch_norm also the [beta | gamma] block) and bsz the divisor the optimizer uses (batch_size; batch_size x ranks
 * under data parallel; the argument of sdqn_net_apply_update):
 *     norm = sqrt(sum_i g_i^2) / bsz  (fp64 accumulation of the stored values: the L2 norm of the mean gradient),
 *     scale = min(1, G / (norm + 1e-6))  in fp64, rounded once to the network's precision (float; double for float64);
 * scale < 1: every g_i becomes g_i * scale (one rounded multiply), otherwise — or when norm is not finite — g keeps its bits.  The
 * optimizer, the BatchNorm parameter update and the --target_tau blend then run as always, on the clipped g.  Two launches between the
 * gradient's reduction and its application (update form 4: +3 launches per step; a clipped step never runs the overlapped
 * data-parallel form, and fc4's RMSProp no longer rides its weight-gradient launch).  Every step that applies an update clips,
 * sdqn_net_apply_update included; a "grad_only" step does not.
 * sdqn_net_last_grad_norm: norm and the scale as applied (the rounded value) of the last clipped step (sync); SDQN_ERR_STATE before
 * any such step. */
int sdqn_net_set_clip_grad_norm(sdqn_net_t h, double max_norm);
int sdqn_net_get_clip_grad_norm(sdqn_net_t h, double* max_norm);
int sdqn_net_last_grad_norm(sdqn_net_t h, double* norm, double* scale);
int sdqn_net_sync(sdqn_net_t h);
/* The two halves of a data-parallel step without a communicator (the arithmetic every rank performs
 * around the all-reduce).  With option "grad_only" = 1 a train step ends after the local gradient SUMS are in the flat
 * gradient buffer (readable / writable per layer with which = 3); sdqn_net_apply_update then runs the optimizer on
 * whatever that buffer holds with divisor bsz (A9: grad / be.bsz, deepqnetwork.py:165 — nranks * batch_size under DP). */
int sdqn_net_apply_update(sdqn_net_t h, double bsz);
/* float16 mode, data parallel (no reference counterpart: deepqnetwork.py:46-48 disables Neon's DP; SURVEY.md §8e "fp16
 * config: all-reduce fp16 grads with fp32 accumulation in RMSProp"): the two passes that bracket the half all-reduce, callable
 * on their own so the exchange itself can be done by the caller.  to_half: the flat fp32 gradient sums * 2^k as IEEE half
 * (uint16 bit patterns; k = device-side payload scale).  from_half: a summed half payload back into the fp32 gradient buffer
 * (/ 2^k); a non-finite value raises the overflow flag and the next sdqn_net_apply_update skips the step (parameters and
 * optimizer state untouched), counts it (sdqn_net_overflow_steps) and, in dynamic mode, halves the scale; 200 clean steps
 * double it.  n = number of values of the flat buffer (sum of sdqn_net_layer_size over all layers). */
int sdqn_net_grad_to_half(sdqn_net_t h, uint16_t* half_out, int64_t n);
int sdqn_net_grad_from_half(sdqn_net_t h, const uint16_t* half_in, int64_t n);
/* {overflow flag of the last from-half pass, log2 of the payload scale, clean steps since the scale last moved}; sync */
int sdqn_net_half_payload_state(sdqn_net_t h, int* flag, int* scale_log2, int* clean_steps);
/* q-values of the last train step: preq float[B,A] (online, prestates), maxpostq float[B] = the bootstrap value: max_a Q(theta-, post),
 * or with option "double_dqn" Q(theta-, post)[argmax_a Q(theta, post)] (first maximum on ties), or with sdqn_net_set_munchausen the soft
 * value of the poststate (sync) */
int sdqn_net_last_q(sdqn_net_t h, float* preq, float* maxpostq);
int sdqn_net_train_iterations(sdqn_net_t h, int64_t* n);     /* deepqnetwork.py:168 */
/* float16 mode under data parallel: the gradient is all-reduced as IEEE half with a dynamic power-of-two payload scale
 * (device-side: halved on overflow, doubled after 200 clean steps; fp32 accumulation in the optimizer; options "dp_half",
 * "dp_half_scale_log2" = fixed scale).  A step whose summed half gradient is not finite is skipped on every rank;
 * this returns how many were (sync).  Always 0 in float32 mode. */
int sdqn_net_overflow_steps(sdqn_net_t h, int64_t* n);
/* the `epoch` argument of DeepQNetwork.train (deepqnetwork.py:107,165): Neon's Adam bias-corrects with t = epoch + 1 */
int sdqn_net_set_epoch(sdqn_net_t h, int epoch);

/* Which launches a train step of this handle is made of, and how its optimizer pass runs — a function of (batch regime, datatype,
 * batch_norm, data-parallel form, option fused_launches) only (tests/test_step_structure.py enumerates the combinations):
 *   structure: 0 fused (fc4_dgrad | bwd3 | bwd2 | bwd1)   1 float16 block-tile (fc4_dgrad | conv3_dgrad | conv2_dgrad | wgrads | bwd1)
 *              2 fused with fc4's all-reduce + update overlapped on the second communicator   3 one launch per problem   4 generic path
 *   update:    0 one update launch   1 serial data parallel (local sums, all-reduce, apply)   2 overlapped data parallel   3 grad_only
 *              4 single GPU with clip_grad_norm (local sums, norm, scale, apply); the generic path reports 4 too when it clips, else 0 */
int sdqn_net_step_structure(sdqn_net_t h, int* structure, int* update);
/* Munchausen DQN targets, --munchausen (Vieillard, Pietquin and Geist 2020; no reference counterpart).  With qbar = Q(theta-, .),
 * pi = softmax(qbar / tau) and lse(q) = max q + tau log sum_a exp((q[a] - max q) / tau) (double, sum in action order), a train step's target is
 *   y = r_c + alpha clip(qbar(s)[a] - lse(qbar(s)), clip, 0) + (terminal ? 0 : discount lse(qbar(s')))
 * (with option "n_step": R, the done flag and discount^n in their places; the bonus is that of the first transition and is added on
 * terminal transitions too).  Everything behind y — TD error, error clip, prioritized-replay weighting and priorities, backward, optimizer
 * — is unchanged; alpha = 0 is Soft-DQN.  Each step is preceded by ONE more forward, the target net on the prestates (also without a
 * target net, where theta- aliases theta), and sdqn_net_last_q's maxpostq is the soft value lse(qbar(s')).  on: 0 (default) / 1, any
 * datatype and geometry, switchable between steps; tau > 0, 0 <= alpha <= 1, clip <= 0 (reference values 0.03, 0.9, -1), checked also
 * when on = 0.  SDQN_ERR_ARG together with option "double_dqn" (the target has no argmax for the online net to choose) and with batch_norm
 * (either order: option "double_dqn" is refused on a net whose Munchausen targets are on). */
int sdqn_net_set_munchausen(sdqn_net_t h, int on, double alpha, double tau, double clip);
int sdqn_net_get_munchausen(sdqn_net_t h, int* on, double* alpha, double* tau, double* clip);     /* any pointer may be NULL */
/* Advantage-learning targets, --advantage_learning alpha / --persistent_advantage (Bellemare, Ostrovski, Guez, Thomas and Munos 2016; DESIGN.md 28;
 * no reference counterpart).  With qbar = Q(theta-, .), gap(q, a) = max_k q[k] - q[a] and y_std the standard target of the taken action,
 *   y_AL  = y_std - alpha gap(qbar(s), a)                                       (persistent = 0; on terminal transitions too)
 *   y_PAL = terminal ? y_AL : max(y_AL, y_std - alpha gap(qbar(s'), a))         (persistent = 1)
 * in double from the stored Q-values (with option "n_step": R, the done flag and discount^n inside y_std); everything behind y is the standard
 * step, and sdqn_net_last_q's maxpostq stays max_a qbar(s')[a].  qbar(s) costs one more forward per train step (the target weights on the
 * prestates, also without a target network).  alpha in [0, 1); alpha = 0 (default) is off: no launch, no argument changes.  Every datatype and
 * geometry, switchable between steps.  SDQN_ERR_ARG for persistent = 1 with alpha = 0 or with option "n_step" > 1, and for alpha > 0 together
 * with option "double_dqn", sdqn_net_set_munchausen, sdqn_net_set_bootstrap K > 1 and batch_norm (either order). */
int sdqn_net_set_advantage_learning(sdqn_net_t h, double alpha, int persistent);
int sdqn_net_get_advantage_learning(sdqn_net_t h, double* alpha, int* persistent);     /* any pointer may be NULL */
/* Conservative Q-learning, --cql_alpha alpha (Kumar, Zhou, Tucker and Levine 2020, CQL(H) in its discrete form; no reference
 * counterpart).  With q = Q(theta, s) the online net's row of the prestate, a the taken action, y the standard target and w the importance
 * weight of a prioritized memory (else 1), a train step's loss per sample is w (0.5 delta^2 + alpha (lse(q) - q[a])):
 *   lse = max q + log sum_k exp(q[k] - max q),   pi[k] = exp(q[k] - lse)                  (double from the stored row, sum in action order)
 *   dq[k] = w (T)(alpha (pi[k] - 1[k == a])) + 1[k == a] w clip(delta),   cost term = w 0.5 delta^2 + w (T)(alpha (lse - q[a]))
 * in the network's number type T (option "n_step": R, the done flag and discount^n inside y).  delta, the error clip, the new priority (of
 * the unclipped delta) and sdqn_net_last_q's maxpostq are the standard step's; every fc5 row carries gradient.  The regulariser reads only
 * values the step already holds: no forward of its own and no launch more than the standard step, in every regime.  alpha >= 0, finite;
 * alpha = 0 (default) is off: no launch, no argument changes.  Every datatype, geometry, optimizer and replay memory; usable online and
 * offline; switchable between steps.  SDQN_ERR_ARG for a negative, NaN or infinite alpha, and for alpha > 0 together with option
 * "double_dqn", sdqn_net_set_munchausen, sdqn_net_set_advantage_learning, sdqn_net_set_bootstrap K > 1, sdqn_net_set_quantiles N > 1,
 * sdqn_net_set_dueling, sdqn_net_set_noisy and batch_norm (either order). */
int sdqn_net_set_cql(sdqn_net_t h, double alpha);
int sdqn_net_get_cql(sdqn_net_t h, double* alpha);      /* the pointer may be NULL */
/* the rule on one sample, host side (no device), from its stored row q_row [A] and its target y: clip_error 0 = no clip, weight 1 = no
 * prioritized replay.  dq_out [A] and *cost_out receive what the train step's head writes for that sample */
int sdqn_cql_loss(int A, double alpha, double clip_error, const float* q_row, int action, double y, double weight, float* dq_out, float* cost_out);
/* Which training options combine (csrc/option_table.h), host side (no device).  The options that take part are numbered from 0:
 * sdqn_option_name(id) is the name the refusals print ("double_dqn", "munchausen", "advantage_learning", "cql_alpha", "bootstrap_heads",
 * "quantiles", "dueling", "noisy_nets", "batch_norm", "clip_grad_norm", "target_tau"), NULL past the end.  sdqn_option_conflict returns 1
 * when switching option `setting` on is refused while option `other` is on — msg [cap] (may be NULL) then receives the words the setter's
 * SDQN_ERR_ARG leaves in sdqn_last_error, the two values printed where an option prints one — 0 when the two combine (msg is emptied), and
 * SDQN_ERR_ARG for an id past the end.  The relation is symmetric and no option is refused with itself. */
const char* sdqn_option_name(int id);
int sdqn_option_conflict(int setting, int other, int setting_value, int other_value, char* msg /*[cap], nullable*/, int cap);
/* Bootstrapped DQN, --bootstrap_heads K (Osband, Blundell, Pritzel and Van Roy 2016; no reference counterpart).  The network is
 * created with num_actions = K x A outputs (<= 18); output row k A + a is Q-head k, action a, and actions in transitions are < A.  A train step
 * gives every Q-head its own target y_k = r_c + (terminal ? 0 : discount max_a Q_k(theta-, s')[a]) and sets
 *   dq[k A + a_n] = m_k clip(Q_k(theta, s)[a_n] - y_k) / K,   cost term = (sum_k m_k 0.5 delta_k^2) / K,   maxpostq (sdqn_net_last_q) = mean_k max_a Q_k
 * (option "n_step": R, the done flag and discount^n in their places).  m_k is the bootstrap mask of the sample's RING SLOT: a pure function
 * of (seed, slot index, k) that is 1 with probability P (sdqn_bootstrap_mask), all ones for P = 1.  P < 1 therefore needs steps fed from a replay
 * memory (sdqn_net_train_many, sdqn_net_train_replay); sdqn_net_train_host* are refused by name then.  Acting: the game loops and
 * sdqn_net_act_greedy follow ONE Q-head per episode while collecting — head sdqn_bootstrap_head_of(seed, K, copy, episode number) — and the
 * majority vote of the K greedy actions (ties: lowest action) while evaluating.  K = 1 (default) is the network without any of this: no
 * launch, no argument changes.  K in 1..18 dividing num_actions, P in (0, 1]; K > 1 is SDQN_ERR_ARG together with option "double_dqn",
 * sdqn_net_set_munchausen, batch_norm and a prioritized replay memory (either order). */
int sdqn_net_set_bootstrap(sdqn_net_t h, int K, double P, uint64_t seed);
int sdqn_net_get_bootstrap(sdqn_net_t h, int* K, double* P, uint64_t* seed);     /* any pointer may be NULL */
/* single-environment acting (sdqn_net_act_greedy): vote = 1 the majority vote (testing), 0 the episode's Q-head of copy 0 (collecting);
 * new_episode: 1 a fresh episode starts (the episode number advances), 0 not, -1 the episode number returns to 0 */
int sdqn_net_bootstrap_acting(sdqn_net_t h, int vote, int new_episode);
/* the two pure functions, host side (no device): out[k] = m_k(index), k < K; *k = the Q-head copy `copy` follows in its episode `episode` */
int sdqn_bootstrap_mask(uint64_t seed, double P, int K, int64_t index, uint8_t* out);
int sdqn_bootstrap_head_of(uint64_t seed, int K, int64_t copy, int64_t episode, int* k);
/* the acting rule on one raw Q row q[K A]: vote = 1 the majority vote, 0 the greedy action of Q-head sdqn_bootstrap_head_of(seed, K, copy, episode)
 * (first maximum; a NaN counts as one) */
int sdqn_bootstrap_act(const float* q, int K, int A, int vote, uint64_t seed, int64_t copy, int64_t episode, int* action);
/* Quantile-regression DQN, --quantiles N (Dabney, Rowland, Bellemare and Munos 2018; no reference counterpart).  The network is
 * created with num_actions = N x A outputs (<= 18); output row j A + a is quantile j of action a at the midpoint tau_j = (2 j + 1) / (2 N),
 * and actions in transitions are < A.  With m(a) = (sum_j theta_j(theta-, s')[a]) / N and a* its first maximum, a train step sets
 *   T_j' = r_c + (terminal ? 0 : discount theta_j'(theta-, s')[a*]),   delta_jj' = theta_j(theta, s)[a_n] - T_j',   kappa = clip_error (> 0),
 *   dq[j A + a_n] = (sum_j' |tau_j - 1[delta_jj' > 0]| clip(delta_jj', -kappa, kappa) / kappa) / N^2,
 *   cost term = (sum_jj' |tau_j - 1[delta_jj' > 0]| L_kappa(delta_jj') / kappa) / N^2 (L_kappa: the Huber function),   maxpostq (sdqn_net_last_q) = m(a*)
 * (option "n_step": R, the done flag and discount^n in their places).  The mean over the N^2 pairs divides the paper's loss by N once more,
 * so one learning rate serves every N.  Acting: the game loops and sdqn_net_act_greedy take the first maximum of the action values
 * Q(s, a) = (sum_j theta_j(s)[a]) / N, collecting and evaluating alike.  N = 1 (default) is the network without any of this: no launch,
 * no argument changes.  N in 1..18 dividing num_actions; N > 1 is SDQN_ERR_ARG with clip_error <= 0 and together with option "double_dqn",
 * sdqn_net_set_munchausen, sdqn_net_set_advantage_learning, sdqn_net_set_bootstrap K > 1, batch_norm and a prioritized replay memory (either order). */
int sdqn_net_set_quantiles(sdqn_net_t h, int N);
int sdqn_net_get_quantiles(sdqn_net_t h, int* N);     /* the pointer may be NULL */
/* what the last train step's head left (N > 1; sync): targets [B][N] = T_j' as stored in the network's precision, dq [B][N A]; widened to
 * double on every path; either pointer may be NULL */
int sdqn_net_last_quantile_step(sdqn_net_t h, double* targets, double* dq);
/* the rule on one sample, host side (no device), from its two stored Q rows q_pre_row / q_post_row [N A]: reward is r_c (n_step: R), gamma the
 * discount (discount^n); dq_out [N A] and *cost_out receive what the train step's head writes for that sample, bit for bit */
int sdqn_quantile_loss(int N, int A, double kappa, const float* q_pre_row, const float* q_post_row, int action, double reward, int terminal,
                       double gamma, float* dq_out, float* cost_out);
/* the acting rule on one raw Q row q[N A]: the first maximum of the quantile means (a NaN counts as one) */
int sdqn_quantile_act(const float* q, int N, int A, int* action);
/* The dueling architecture, --dueling (Wang, Schaul, Hessel, van Hasselt, Lanctot and de Freitas 2016; no reference counterpart).
 * The network is created with num_actions = A + 1 outputs (<= 18): output row 0 is V, row 1 + a is Adv_a, and actions in transitions are < A.
 * The two streams are the halves of fc4's 512 hidden units: V reads units j < 256 only, every Adv_a units j >= 256 only.  fc5's other
 * entries are exactly +0.0 in the online and the target weights at every point a forward can read them: the setter zeroes them, and so do
 * sdqn_net_set_weights / _f64 on layer 4 of which 0 / 1 (a caller's non-zero values there are accepted and dropped); the same entries of the
 * flat gradient are set to +0.0 behind its local sums (and the all-reduce), in front of clip_grad_norm's norm and of the optimizer, which
 * moves a weight with gradient 0 by exactly 0.  With Q(s, a) = (float)((V + Adv_a) - (sum_b Adv_b) / A) (double, the sum in action order):
 *   y = r_c + (terminal ? 0 : discount max_a Q(theta-, s', a)),   delta = Q(theta, s, a_n) - (float)y,
 *   c = the standard head's clipped (and, prioritized replay, weighted) error,   dq[0] = c,   dq[1 + b] = c (1[b = a_n] - 1 / A)
 * (option "n_step": R, the done flag and discount^n in their places; the cost term and the new priority are the standard head's on delta).
 * maxpostq (sdqn_net_last_q) = max_a Q(theta-, s', a).  Acting: the game loops and sdqn_net_act_greedy take the first maximum of Q(s, .),
 * collecting and evaluating alike.  Every train step runs the split optimizer tail (local sums, mask, apply).  on = 0 (default) is the
 * network without any of this.  on = 1 is SDQN_ERR_ARG together with option "double_dqn", sdqn_net_set_munchausen,
 * sdqn_net_set_advantage_learning, sdqn_net_set_bootstrap K > 1, sdqn_net_set_quantiles N > 1 and batch_norm (either order). */
int sdqn_net_set_dueling(sdqn_net_t h, int on);
int sdqn_net_get_dueling(sdqn_net_t h, int* on);      /* the pointer may be NULL */
/* what the last train step's head left (dueling on; sync): y [B] and delta [B] as stored in the network's precision, dq [B][A + 1]; widened
 * to double on every path; any pointer may be NULL */
int sdqn_net_last_dueling_step(sdqn_net_t h, double* y, double* delta, double* dq);
/* the rule on one sample, host side (no device), from its two stored rows q_pre_row / q_post_row [A + 1]: reward is r_c (n_step: R), gamma
 * the discount (discount^n), clip_error 0 = no clip; per != 0: per_weight multiplies the cost term and the clipped error and *priority_out
 * receives (|delta| + per_eps)^per_alpha.  dq_out [A + 1] and *cost_out receive what the train step's head writes for that sample;
 * y_out, delta_out, maxq_out, priority_out may be NULL */
int sdqn_dueling_loss(int A, double clip_error, const float* q_pre_row, const float* q_post_row, int action, double reward, int terminal,
                      double gamma, int per, double per_weight, double per_alpha, double per_eps, float* dq_out, float* cost_out,
                      float* y_out, float* delta_out, float* maxq_out, float* priority_out);
/* the acting rule on one raw row q[A + 1]: the first maximum of Q(s, .) (a NaN Q(a) is never chosen over a number, a NaN Q(0) stays);
 * q_out (may be NULL) receives the A action values */
int sdqn_dueling_act(const float* q, int A, int* action, float* q_out);
/* Noisy networks, --noisy_nets (Fortunato et al. 2018, factorised Gaussian noise; no reference counterpart).  fc4 and fc5 become
 * W = mu + sigma * (f(e_out) f(e_in)^T), f(x) = sgn(x) sqrt|x|, e of unit normals; the layers have no bias, the convolutions stay as they are.
 * mu is what sdqn_net_set_weights / _get_weights address (which 0 / 1); sigma starts at sigma0 / sqrt(fan_in) in both nets and is the online
 * net's own learned parameter: d sigma = dW * (f(e_out) f(e_in)^T), applied by the net's optimizer rule with state of its own and mu's
 * learning rate and divisor.  Train step t (1, 2, ...) draws xi_t for the online and an independent xi'_t for the target net, used by the
 * whole step.  The noise is a counter: sdqn_noisy_words / sdqn_noisy_noise restate stream (seed, step, slot 0 online / 1 target, layer 0 fc4 /
 * 1 fc5, side 0 inputs / 1 outputs) on the host — n 64-bit words, or the n unit normals z with e = f(z); fc4's input index is the weights'
 * column index.  sdqn_net_update_target also copies sigma.  Forwards: sdqn_net_predict, sdqn_env_eval and the single-environment acting
 * paths after sdqn_net_noisy_acting(h, 0) read mu alone; sdqn_net_predict_noisy, sdqn_env_collect and the acting paths after
 * sdqn_net_noisy_acting(h, 1) (default) read the online net's current mu and sigma under the last train step's xi_t (xi_0 before the first).
 * A noisy step runs the split optimizer tail plus three launches (compose, sigma, compose).  on = 1 is SDQN_ERR_ARG on float16 / float64 /
 * other geometries, with batch_norm, clip_grad_norm, target_tau, munchausen, advantage_learning, bootstrap_heads > 1, quantiles > 1,
 * dueling and data parallel (either order).  sdqn_net_get / _set_noisy_sigma: layer 3 (fc4, [512][3136]) or 4 (fc5, [A][512]) of net 0 / 1,
 * in the layout of the weights.  sdqn_net_debug_read: "noisy_eps" [2][4192] the factors f(z) last composed per net (e_in4 | e_out4 | e_in5 |
 * e_out5 padded to 32), "noisy_theta" / "noisy_theta_t" the effective flat buffers, "noisy_sigma_grad" (option keep_gradients). */
int sdqn_net_set_noisy(sdqn_net_t h, int on, double sigma0, uint64_t seed);
int sdqn_net_get_noisy(sdqn_net_t h, int* on, double* sigma0, uint64_t* seed, int64_t* step);      /* any pointer may be NULL */
int sdqn_net_noisy_acting(sdqn_net_t h, int collecting);
int sdqn_net_get_noisy_sigma(sdqn_net_t h, int which_net, int layer, float* buf, int64_t n);
int sdqn_net_set_noisy_sigma(sdqn_net_t h, int which_net, int layer, const float* buf, int64_t n);
int sdqn_net_predict_noisy(sdqn_net_t h, const uint8_t* states, float* q_out);
int sdqn_noisy_words(uint64_t seed, uint64_t step, int slot, int layer, int side, int64_t n, uint64_t* out_words);
int sdqn_noisy_noise(uint64_t seed, uint64_t step, int slot, int layer, int side, int64_t n, float* out_z);
/* Random-shift augmentation, --random_shift P (DrQ: Kostrikov, Yarats and Fergus 2020; no reference counterpart).  P in 0..8,
 * 0 (default) off: nothing changes.  P > 0: every train step that samples from a replay memory — sdqn_net_train_many, _train_many_deferred,
 * _train_replay, prioritized or not, any datatype and geometry — trains on shifted states: sample n and state s (0 prestate, 1 poststate)
 * draw (dy, dx) in [-P, P]^2, and output pixel (y, x) of every frame of the state is input pixel (clamp(y + dy, 0, H - 1), clamp(x + dx, 0,
 * W - 1)): replicate-padding by P, then a crop.  The bytes stay exact; every forward of the step (online, target, the Double DQN slot, the
 * Munchausen / advantage-learning forward on the prestates) reads the same shifted state.  One launch in front of the step writes the 2 B
 * shifted states into the memory's device minibatch (what sdqn_replay_gather fills: a pending minibatch there is overwritten), and the step
 * reads it in place, as sdqn_net_train_host does with states_in_place.  The draws are a counter: splitmix64 keyed by (seed, t, n, s), t = 0,
 * 1, ... the shifted steps this handle has enqueued since the setter (which returns t to 0); sdqn_random_shift_draw restates them on the host
 * (no device).  Sampling, indexes, weights and priorities are what they are with P = 0; sdqn_net_train_host / _returns (the caller's own
 * states), predict, acting, sdqn_env_eval and sdqn_env_collect are never shifted.  SDQN_ERR_ARG: P outside 0..8, P > 0 with batch_norm or with
 * P >= min(screen_height, screen_width).  sdqn_net_last_shifts: out [B][2][2] = (dy, dx) per sample and state as the last step's launch
 * drew them (waits for the device; SDQN_ERR_ARG before the first shifted step). */
int sdqn_net_set_random_shift(sdqn_net_t h, int P, uint64_t seed);
int sdqn_net_get_random_shift(sdqn_net_t h, int* P, int64_t* step_counter);      /* any pointer may be NULL */
int sdqn_random_shift_draw(uint64_t seed, uint64_t step, int64_t n, int s, int P, int* dy, int* dx);
int sdqn_net_last_shifts(sdqn_net_t h, int8_t* out);
/* Dormant-neuron recycling, --redo_interval N / --redo_threshold T (ReDo: Sokar, Agarwal, Castro and Evci 2023; no reference
 * counterpart).  The four ReLU layers conv1, conv2, conv3, fc4 have 32, 64, 64, 512 units = 672 scores [s_1 | s_2 | s_3 | s_4].  The score of
 * unit j of layer l is m_l[j] / mean_k m_l[k] (0 when the mean is 0), m_l[j] = the mean of |activation| over the rows of the online net's
 * prestate half of the LAST TRAIN STEP, summed in fp64 in a fixed order (no atomics: the same activations give the same bits); a unit is
 * dormant when its score <= T (T in [0, 1), 0: exactly silent units only).  One recycle EVENT e = 1, 2, ... on the online net: the incoming
 * weights of every dormant unit become fresh draws of the initialiser, (u 2^-23 - 1) sqrt(3 / fan_in) in float with u the top 24 bits of one
 * splitmix64 word keyed by (seed, e, flat internal index) (sdqn_redo_draw restates it); every weight of the next layer that multiplies the
 * unit becomes +0.0 (fc5: that column of all rows; zeroing wins over a draw); the optimizer state(s) of all those entries return to +0.0.
 * The target net, every other weight and the gradient buffer are untouched; the half copies / conv1's bf16 planes follow.
 * sdqn_net_set_redo: interval N > 0: an event follows every applied train step t (sdqn_net_train_iterations) with t % N == 0, on the
 * library stream, inside multi-step calls too, without any wait; 0 (default): nothing runs and nothing is allocated.  SDQN_ERR_ARG: N < 0,
 * T outside [0, 1), N > 0 on a batch_norm or noisy net, on the generic path (float64, other geometries) or with data parallel on more than
 * one rank (sdqn_net_set_noisy and sdqn_dp_init refuse the other way round).  sdqn_net_redo_now: one event now; sdqn_net_redo_scores: out
 * [672], recycles nothing, usable with interval 0 — both SDQN_ERR_ARG before the first train step or once a forward of its own (predict,
 * act) has overwritten that step's activations.  sdqn_net_redo_last: out [6] = the last event's number (0: none yet), the train step it
 * followed and the four dormant counts, as the device left them.  sdqn_redo_apply_host (no device): the same rules on host arrays in the
 * internal layouts, theta / state / state2 (state, state2, counts may be NULL) of 1 683 456 + 512 A floats, in place. */
int sdqn_net_set_redo(sdqn_net_t h, int interval, double tau, uint64_t seed);
int sdqn_net_get_redo(sdqn_net_t h, int* interval, double* tau, uint64_t* seed);      /* any pointer may be NULL */
int sdqn_net_redo_now(sdqn_net_t h);
int sdqn_net_redo_scores(sdqn_net_t h, float* out);
int sdqn_net_redo_last(sdqn_net_t h, int64_t* out);
int sdqn_redo_apply_host(const float* scores, double tau, uint64_t seed, uint64_t event, int A, float* theta, float* state, float* state2,
                         int64_t* counts);
int sdqn_redo_draw(uint64_t seed, uint64_t event, int64_t index, int layer, uint64_t* word, float* value);      /* layer 1..4; either may be NULL */
/* Periodic resets with shrink-and-perturb, --reset_interval N / --reset_layers L / --shrink_perturb ALPHA (Nikishin et al. 2022, Ash and
 * Adams 2020, D'Oro et al. 2023; no reference counterpart).  One reset EVENT e = 1, 2, ... walks the flat weight buffers once:
 * the last L of the five layers conv1, conv2, conv3, fc4, fc5 have factor 0, the others factor ALPHA.  Factor 1: the entry is not written, in
 * any buffer.  Factor 0: theta[i] = phi_i (the old value is not read).  Otherwise theta[i] = fmaf(a, theta[i], b * phi_i) with a =
 * (float)ALPHA, b = (float)(1.0 - ALPHA), the product rounded once.  The target net takes the same formula with the same phi_i; the optimizer
 * state(s) become +0.0 wherever the factor is below 1; the gradient buffer, the replay memory and the step counter are untouched.  phi_i =
 * (u 2^-23 - 1) sqrt(3 / fan_in) in float, fan_in 256, 512, 576, 3136, 512, u the top 24 bits of one splitmix64 word keyed by (seed, e, flat
 * internal index) under a domain constant of its own: under one seed it is never the word sdqn_redo_draw gives for the same (e, index)
 * (sdqn_reset_draw restates it).  The half copies / conv1's bf16 planes of both nets and a dueling net's fc5 mask follow.
 * sdqn_net_set_reset: interval N > 0: an event follows every applied train step t (sdqn_net_train_iterations) with t % N == 0, behind the
 * soft target update and the recycle event of sdqn_net_set_redo, on the library stream, inside multi-step calls too, without any wait; 0
 * (default): nothing runs and nothing is allocated.  SDQN_ERR_ARG: N < 0, L outside 0..5, ALPHA outside [0, 1], N > 0 with L = 0 and ALPHA
 * = 1 (nothing to do), N > 0 on a batch_norm or noisy net, on the generic path (float64, other geometries) or with data parallel on more
 * than one rank (sdqn_net_set_noisy and sdqn_dp_init refuse the other way round).  sdqn_net_reset_now: one event now, numbered like the
 * others, with the L and ALPHA last set.  sdqn_net_reset_last: out [2] = the last event's number (0: none yet) and the train step it
 * followed, as the device left them; the only call here that waits.  sdqn_reset_apply_host (no device): the same event on host arrays in the
 * internal layouts, 1 683 456 + 512 A floats each, in place, A = fc5's rows; theta_t NULL or == theta: one net; state may be NULL; state2 is
 * read for optimizer 1 (adam) and 2 (adadelta) only. */
int sdqn_net_set_reset(sdqn_net_t h, int interval, int layers, double alpha, uint64_t seed);
int sdqn_net_get_reset(sdqn_net_t h, int* interval, int* layers, double* alpha, uint64_t* seed);      /* any pointer may be NULL */
int sdqn_net_reset_now(sdqn_net_t h);
int sdqn_net_reset_last(sdqn_net_t h, int64_t* out);
int sdqn_reset_apply_host(int layers, double alpha, uint64_t seed, uint64_t event, int A, int optimizer, float* theta, float* theta_t,
                          float* state, float* state2);
int sdqn_reset_draw(uint64_t seed, uint64_t event, int64_t index, int layer, uint64_t* word, float* value);      /* layer 1..5; either may be NULL */
/* Decoupled weight decay and L2-init regularisation, --weight_decay WD / --l2_init LAMBDA (Loshchilov and Hutter 2019; Kumar, Marklund and Van
 * Roy 2023; no reference counterpart).  The rule on each of the 1 683 456 + 512 A weights of the online net, after every applied
 * train step, in front of the soft target update, the recycle event and the reset event:
 *     v = theta[e];  WD > 0: v = v * kf;  LAMBDA > 0: v = v + cf * (anchor[e] - v);  theta[e] = v
 * with kf = (float)(1.0 - lr WD), cf = (float)(lr LAMBDA), lr the net's learning_rate, every float operation rounded on its own.  A coefficient
 * of 0 skips its line.  The optimizer state is not touched; the half copies / conv1's bf16 planes follow in the same launch.  With target_tau
 * in (0, 1) and a target net ONE launch regularises theta and blends theta- toward the new theta (bit for bit the two launches it replaces).
 * sdqn_net_set_regularizer: SDQN_ERR_ARG for WD < 0, LAMBDA < 0, lr WD >= 1, lr LAMBDA > 1 (NaN included) and for a coefficient > 0 on a
 * batch_norm or noisy net, on the generic path (float64, other geometries) or with data parallel on more than one rank (sdqn_net_set_noisy and
 * sdqn_dp_init refuse the other way round).  When LAMBDA goes from 0 to > 0 the anchor (a device copy of the online weights) is allocated if
 * need be and taken, in stream order; sdqn_net_anchor_now takes it again (and allocates it on a net that has none); events of
 * sdqn_net_set_redo / sdqn_net_set_reset do not move it, and it is not part of the weights a caller saves.  Both 0 (default): nothing runs,
 * nothing is allocated.  sdqn_net_regularize_now: one launch of the rule now with the coefficients set, outside a step, the target net
 * untouched; sdqn_net_regularize_with: the same with the coefficients given (LAMBDA > 0 needs an anchor).  sdqn_net_get_anchor: layer 0..4 of
 * the anchor in sdqn_net_get_weights' layout; waits.  sdqn_net_weight_norms: out [10] = per layer conv1..fc5 the fp64 sum of theta^2, then
 * of (theta - anchor)^2 (NaN without an anchor), reduced in a fixed order: the same weights give the same bits; two launches and a wait, never
 * part of a step.  sdqn_regularize_apply_host (no device): the rule on n host values in place; anchor is read for LAMBDA > 0 only. */
int sdqn_net_set_regularizer(sdqn_net_t h, double wd, double lambda);
int sdqn_net_get_regularizer(sdqn_net_t h, double* wd, double* lambda);      /* either pointer may be NULL */
int sdqn_net_regularize_now(sdqn_net_t h);
int sdqn_net_regularize_with(sdqn_net_t h, double wd, double lambda);
int sdqn_net_anchor_now(sdqn_net_t h);
int sdqn_net_get_anchor(sdqn_net_t h, int layer, float* buf, int64_t n);
int sdqn_net_weight_norms(sdqn_net_t h, double* out);
int sdqn_regularize_apply_host(double wd, double lambda, double lr, int64_t n, float* theta, const float* anchor);
/* option "double_dqn" (0 default / 1, any configuration, switchable between steps): Double DQN targets (van Hasselt, Guez and Silver
 * 2016): the online net picks each poststate's action, the target net values it (see sdqn_net_last_q).  The online net's forward on
 * the poststates rides as a third net slot in the step's own forward launches (batch_norm: a forward of its own in front of the step,
 * inference mode with the running statistics as they stand before the step); without a target net (target_enabled = 0) it is the
 * standard step.
 * option "n_step" (1 default .. 16, any configuration, between steps): n-step returns — the poststate of sample i is
 * state(i + n - 1) (a run-time frame offset of the forward launches: no added launch), the target R + discount^n max Q' (R only when
 * an episode ended inside the n steps).  Ring-fed train calls need a replay memory set to the same n (sdqn_replay_set_n_step); tuples
 * go through sdqn_net_train_host_returns.  sdqn_net_last_q's maxpostq is then the bootstrap value of state(i + n - 1).
 * options: "grad_only" (see sdqn_net_apply_update), "keep_gradients" (1: the fc4 gradient is materialised and readable with which=3; 0 (default): on one
 * GPU RMSProp of fc4 is fused into the wgrad epilogue), "fused_launches" (1 default:
 * independent backward stages share one grid), "xcd_map" (0 default = only where it wins time: conv1/conv2/fc4 forward; 1: the
 * XCD-contiguous workgroup->tile map for every launch), "dp_overlap" (BEFORE sdqn_dp_init: -1 default = auto — second communicator for
 * nranks >= 2, activated by sdqn_dp_probe + vote + sdqn_dp_set_overlap; 1 forced on; 0 one all-reduce on the library stream), "dp_sync_replicas" (1 default: sdqn_dp_init broadcasts rank 0's online net,
 * target net and optimizer state so every learner starts from — and keeps — the same network; 0 BEFORE sdqn_dp_init: keep own), "profile_every" (N: sdqn_net_profile times every N-th
 * launch), "profile_mode" (1 default: the launch records its own dispatch-packet begin / end timestamps into the event pair through hipExtLaunchKernel —
 * what rocprofv3 --kernel-trace reports, nothing added to the queue; 0: hipEventRecord markers around the launch, ~2.6 us more per launch), "nw:<kernel id>" / "xcd:<kernel id>" / "f4_share3" / "f4_share2" (tuning hooks).
 * Round-3 switches of the default fp32 / float16 step, every one bit-identical to its alternative unless noted (tools/exp/README.md has the
 * measurements): "wt" (bit mask, default 511: write-through epilogue stores per launch), "conv1_bf16" / "conv1w_bf16" (1 default: conv1
 * forward / weight gradient on packed-bf16 MFMA with an exact 3-way split; 0: the fp32-MFMA engine — last bits differ), "conv3_c36" (1 default:
 * conv3 forward on 36-deep K-chunks; last bits differ), "r3_xcd" (tile maps of the two conv1 kernels).  A float64 / non-84x84x4 network
 * (generic path) accepts and ignores the tuning options.
 * Round 4: "bt" (1 default: batch_size >= 128 runs on the block-tile engine, gemm_engine_bt.h; 0: the latency engine's launch forms),
 * "bt:<kernel id>" (menu entry of that launch: 0 built-in block shape, -1 latency engine / previous kernel, n > 0 other shapes — tuning
 * surface of tools/sweep_bt.py), "tps:<layer>" (K chunks per weight-gradient slab), "act_kernel" (1 default where available — float32, no
 * batch_norm, 84x84x4: the acting forward of sdqn_net_predict_state / _predict_one is ONE launch, sdqn_act.hip; 0: the five batched
 * forward kernels at batch 1; test hook "act_inject_failure": the next such launch delivers nothing, which exercises the host's fall-back to the
 * five launches).  The step structures that were built, tested and measured SLOWER — "hoist", "f4w_early", "fuse_upd",
 * "head_f4d", "two_streams", "fwd_rb", "bwd_order", "rb:<id>", "bt_x", "btx:<id>", "bt_planes" — left the library in round 5
 * (tools/exp/experiments_r04.patch re-creates the last tree that contained them, results in tools/exp/README.md); a non-zero value for one of
 * these names is refused with SDQN_ERR_ARG, zero is accepted and does nothing. */
int sdqn_net_set_option(sdqn_net_t h, const char* name, int value);

/* test hook: raw read-back of an internal device buffer ("a1","a2","a3","a4","d4","d3p","d2p","d1","q",
 * "dq","g","theta","cost_terms"; internal layouts documented in simple_dqn_amd/csrc/problems.h) */
int sdqn_net_debug_read(sdqn_net_t h, const char* name, float* out, int64_t n);

/* Filter visualisation (the reference's --visualization_file: src/main.py:119-127 -> visualization.py, Neon's DeconvCallback).  For
 * each of the first F_l = min(K_l, max_fm) maps of conv1 / conv2 / conv3, the state n and output position p (row-major) with the largest
 * PRE-activation z_l[n, f, p] over the n states — ties go to the smallest n / batch_size, then the smallest p, then the smallest
 * n % batch_size (batch_size of the net: the reference's batch loop) — and that activation projected back to the input by guided
 * backpropagation (ReLU-gated transposed convolutions) -> vis float[4][84][84].  States: either ring indexes idx[n] of r (frames
 * (idx - 3 + j) mod count, getState's index math; the caller uploads edited ring slots first) or host states u8[n][4][84][84] with
 * r = idx = NULL.  Records, in order conv1, conv2, conv3 (F_1 + F_2 + F_3 entries): rec_state, rec_pos, rec_value; vis_out
 * float[records][4][84][84] (NULL: the search only); ms_out float[2] nullable: device ms of the search and of the projection launch.
 * Online fp32 parameters (float16 nets: the same fp32 master weights), enqueued after pending work on the library stream (sync).
 * SDQN_ERR_ARG for float64 / non-84x84x4 nets, batch_norm nets, max_fm < 1, n < 1 and an n whose tie key overflows 32 bits. */
int sdqn_net_visualize(sdqn_net_t h, sdqn_replay_t r, const int64_t* idx, const uint8_t* states, int64_t n, int max_fm,
                       int64_t* rec_state, int32_t* rec_pos, float* rec_value, float* vis_out, float* ms_out);

/* ---- device-resident environment: the game "catch" (no reference counterpart; DESIGN.md §18, csrc/env_catch.h) ------------------------
 * A 12 x 12 court of (H / 12) x (W / 12)-pixel cells: a ball falls one row per step (col += dx, reflecting at the side walls), a paddle
 * of 3 cells on row 11 moves with actions 0 stay / 1 left / 2 right.  A ball reaching row 11 gives +1 on the paddle, -1 beside it, and a
 * new ball spawns; every other step gives 0; an episode is balls_per_episode balls.  Frames u8[H][W]: 0 background, 255 ball, 128 paddle.
 * The environment owns a splitmix64 generator (never Python's random nor the sampler's MT19937).  create / destroy / restart / step /
 * screen / get_state / set_state / num_actions run on the HOST and need no device. */
typedef struct sdqn_env_s* sdqn_env_t;
typedef struct {
  int32_t row, col, dx;    /* ball: 0..11, 0..11, -1..1 */
  int32_t paddle;          /* left edge, 0..9 */
  int32_t balls;           /* landed in this episode */
  int32_t terminal;        /* 0 / 1 */
  uint64_t rng;            /* splitmix64 counter */
} sdqn_env_state;
/* The game "breakout" (csrc/env_breakout.h), on the same court with the same paddle and actions: three rows of bricks
 * (rows 1..3, pixel 64) that stay destroyed, a ball that moves diagonally (dx, dy in {-1, +1}), reflects at the side walls and the top
 * wall, turns back from a brick it breaks (reward +1, the only reward) and from the paddle (whose left / right cell also sets dx);
 * a ball that passes the paddle is lost, a new one spawns on row 4, an episode is balls_per_episode lost balls; the last brick
 * broken sets all 36 again. */
typedef struct {
  int32_t row, col, dx, dy;  /* ball: 0..10, 0..11, -1 / +1, -1 / +1; never in a brick cell */
  int32_t paddle;            /* left edge, 0..9 */
  int32_t balls;             /* lost in this episode */
  int32_t terminal;          /* 0 / 1 */
  int32_t pad;               /* 0 */
  uint64_t bricks;           /* bit 12 (r - 1) + c: a brick at row r in {1, 2, 3}, column c; bits 36..63 are 0 */
  uint64_t rng;              /* splitmix64 counter */
} sdqn_env_state_breakout;
/* The game "freeway" (csrc/env_freeway.h), on the same court: a chicken on column 6 starts on row 11 and moves with actions
 * 0 stay / 1 up / 2 down; rows 1..10 carry one car each (pixel 128), odd rows driving right, even rows left, wrapping modulo 12, a car of
 * period p moving one cell every p-th tick.  Reaching row 0 gives +1 (the only reward), puts the chicken back on row 11 and draws new
 * traffic; a hit (the chicken walks into a car, or a car drives into it) puts it back on row 11 without a reward.  An episode is
 * balls_per_episode game TICKS (the `balls_per_episode` argument of sdqn_env_create carries the episode length for this game). */
typedef struct {
  int32_t row;               /* the chicken: 0..11, never in a car's cell */
  int32_t ticks;             /* game ticks played in this episode, >= 0 */
  int32_t crossings;         /* made in this episode, >= 0 */
  int32_t terminal;          /* 0 / 1 */
  int32_t pad0, pad1;        /* 0 */
  uint64_t cars;             /* nibble r - 1: the column (0..11) of the car of row r in 1..10; bits 40..63 are 0 (in all three words) */
  uint64_t timers;           /* nibble r - 1: ticks until that car moves, 1..period */
  uint64_t periods;          /* nibble r - 1: 1..5 */
  uint64_t rng;              /* splitmix64 counter */
} sdqn_env_state_freeway;
/* name = "catch", "breakout" or "freeway"; H, W >= 12 (else SDQN_ERR_ARG); the generator starts at `seed`, the first episode is started.
 * Every sdqn_env_* call below serves all games; the tallies `caught` / `missed` of sdqn_env_eval / sdqn_env_collect count bricks broken /
 * balls lost on breakout and crossings / hits on freeway. */
int sdqn_env_create(sdqn_env_t* h, const char* name, int screen_height, int screen_width, uint64_t seed, int balls_per_episode);
int sdqn_env_destroy(sdqn_env_t e);
int sdqn_env_restart(sdqn_env_t e);                                  /* new episode: balls 0, paddle 4, a new ball; does not reseed */
int sdqn_env_num_actions(sdqn_env_t e, int* n);
int sdqn_env_step(sdqn_env_t e, int action, int* reward, int* terminal);
int sdqn_env_screen(sdqn_env_t e, uint8_t* screen /*[H][W]*/);       /* the host-rendered frame of the current state */
int sdqn_env_get_state(sdqn_env_t e, sdqn_env_state* st);
int sdqn_env_set_state(sdqn_env_t e, const sdqn_env_state* st);      /* SDQN_ERR_ARG for fields out of range; both: SDQN_ERR_ARG on a breakout handle */
int sdqn_env_get_state_breakout(sdqn_env_t e, sdqn_env_state_breakout* st);
int sdqn_env_set_state_breakout(sdqn_env_t e, const sdqn_env_state_breakout* st);   /* SDQN_ERR_ARG for fields out of range; both: SDQN_ERR_ARG on a catch handle */
int sdqn_env_get_state_freeway(sdqn_env_t e, sdqn_env_state_freeway* st);
int sdqn_env_set_state_freeway(sdqn_env_t e, const sdqn_env_state_freeway* st);     /* SDQN_ERR_ARG for fields out of range; both: SDQN_ERR_ARG on another game's handle */
int sdqn_env_name(sdqn_env_t e, const char** name);                  /* "catch" / "breakout" / "freeway": a static string */
/* Dynamics of the game (csrc/env_dynamics.h), honoured by every call that steps it (sdqn_env_step, sdqn_net_act_step_env,
 * and the copies of sdqn_env_eval / sdqn_env_collect, which play under the dynamics of the handle they are given).  frame_skip k in 1..8
 * (default 1): one agent step is up to k game ticks of the same chosen action, the rewards add up, a tick that sets terminal ends it, only
 * the last state is rendered.  repeat_action_probability p in [0, 1) (default 0; ALE's sticky actions): before every tick one draw u of
 * the sticky generator (splitmix64; catch_stream_seed(seed, 0, 2) for a handle created with seed, (seed, e, 2) for copy e), and with
 * (u >> 11) < ceil(p 2^53) the tick executes the action the last tick executed (0 after create and after every restart) instead of the
 * chosen one; p = 0 draws nothing.  Replay memory, traces and statistics record the chosen action.  Out of range: SDQN_ERR_ARG. */
int sdqn_env_set_dynamics(sdqn_env_t e, int frame_skip, double repeat_action_probability);
/* every output optional (NULL); prev_action / sticky_rng complete sdqn_env_get_state*: together they reproduce a game exactly */
int sdqn_env_get_dynamics(sdqn_env_t e, int* frame_skip, double* repeat_action_probability, int* prev_action, uint64_t* sticky_rng);
int sdqn_env_set_dynamics_state(sdqn_env_t e, int prev_action, uint64_t sticky_rng);   /* SDQN_ERR_ARG: prev_action not an action */
/* test hook: the frame of the current state as the render KERNEL produces it (sync) */
int sdqn_env_render_device(sdqn_env_t e, uint8_t* screen);
/* sdqn_net_act_step for an environment of the library: steps the game with `action`, then adds the new frame to the state buffer and,
 * with r, the transition (action, reward, frame, terminal) to the replay memory.  The host renders the frame into the host mirrors, one
 * launch renders it into the state buffer's device slot and the ring mirror's slot: no frame crosses PCIe.  Everything else is
 * sdqn_statebuf_add + sdqn_replay_add (+ the speculative acting forward), bit for bit. */
int sdqn_net_act_step_env(sdqn_net_t h, sdqn_statebuf_t sb, sdqn_replay_t r, sdqn_env_t e, int action, int speculate,
                          int* reward, int* terminal);
/* Vectorised evaluation on the device: num_envs (1 .. batch_size) independent copies of e's game (its geometry and balls_per_episode;
 * e's own state is untouched) played for `steps` steps by the online net, epsilon-greedy.  Copy i: game generator
 * seeded mix(seed + K (2 i + 1)), acting generator mix(seed + K (2 i + 2)) (K = 0xD1B54A32D192ED03, mix = the splitmix64 finaliser); per
 * step ONE draw u of the acting generator, exploring when (u >> 11) < ceil(epsilon 2^53) with a second draw % 3 as the action, else the
 * first maximum of the copy's Q row (NaN rule of sdqn_net_act_greedy).  A terminal step restarts the copy with zeroed history.  Per
 * step the batched forward of sdqn_net_predict and one kernel are enqueued; one synchronisation at the end.  Outputs [num_envs], any
 * NULL: steps, summed reward, balls caught, balls missed, episodes finished.  Trace, all four or none: actions / rewards / terminals
 * [steps][num_envs], q [steps][num_envs][3] (double: exact for every datatype).  Any datatype / geometry sdqn_net_predict serves. */
int sdqn_env_eval(sdqn_net_t h, sdqn_env_t e, int num_envs, int64_t steps, double epsilon, uint64_t seed,
                  int64_t* out_steps, int64_t* out_reward, int64_t* out_caught, int64_t* out_missed, int64_t* out_episodes,
                  uint8_t* actions, int8_t* rewards, uint8_t* terminals, double* q);
/* --train_envs: collect experience the way sdqn_env_eval plays.  `locksteps` locksteps of num_envs copies of e's game;
 * every lockstep is the forward of sdqn_net_predict on the copies' states (skipped while epsilon >= 1, where no Q row is read) and ONE
 * kernel that picks the actions, steps and renders the games and writes the num_envs transitions into slot `position` of each lane of the
 * laned memory r (sdqn_replay_set_lanes(r, num_envs)): frame and (action, reward, terminal) into the HBM mirror, then two strided
 * device-to-host copies into the pinned master, which stays a true copy.  Nothing goes host to device; the call waits once, at its end,
 * advances the memory's fill / position and unpacks actions / rewards / terminals.  The copies live on the net handle between calls:
 * seed >= 0 seeds them as sdqn_env_eval does (their first frames are no transitions), seed < 0 continues the stream of the last call
 * (SDQN_ERR_ARG if there is none for num_envs).  Lockstep t of the call plays with epsilon = clamp(epsilon_start + t epsilon_step, 0, 1).
 * The frame stored with a terminal transition is the restarted game's first frame.  Outputs and trace as sdqn_env_eval ([locksteps]
 * rows; q is 0 where the forward was skipped); the tallies are the copies' running sums since they were seeded. */
int sdqn_env_collect(sdqn_net_t h, sdqn_env_t e, sdqn_replay_t r, int num_envs, int64_t locksteps, double epsilon_start, double epsilon_step,
                     int64_t seed, int64_t* out_steps, int64_t* out_reward, int64_t* out_caught, int64_t* out_missed, int64_t* out_episodes,
                     uint8_t* actions, int8_t* rewards, uint8_t* terminals, double* q);

/* per-kernel device timing (HIP events on the library stream; see option "profile_mode"), for bench.py's roofline leg.
 * kernel < 0 brackets every kernel of the step, otherwise only that kernel id. */
int sdqn_net_profile(sdqn_net_t h, int enable, int kernel);
int sdqn_net_profile_count(int* n_kernels);
int sdqn_net_profile_read(sdqn_net_t h, int kernel, const char** name, double* total_ms, int64_t* launches);
int sdqn_net_profile_reset(sdqn_net_t h);

/* ---- data parallel: one learner per GPU, one RCCL all-reduce of the flat gradient per step ---
 * (no reference counterpart: deepqnetwork.py:46-48 disables Neon's DP) */
int sdqn_dp_unique_id(const char* rccl_path, char id[128]);
int sdqn_dp_init(sdqn_net_t h, const char* rccl_path, const char id[128], int rank, int nranks);
int sdqn_dp_shutdown(sdqn_net_t h);
/* what RCCL reports about the live communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice; -1 without one)
 * and the device the library is bound to: lets a multi-GPU record prove that RCCL spanned N ranks on N devices */
int sdqn_dp_info(sdqn_net_t h, int* comm_ranks, int* comm_rank, int* comm_device, int* bound_device);
/* Overlapped form of the step (fc4's 95 % of the gradient all-reduced + applied on a second communicator / stream under the rest of the
 * step; no reference counterpart, deepqnetwork.py:46-48).  With option "dp_overlap" = -1 (auto, default) sdqn_dp_init creates the second
 * communicator for nranks >= 2 but leaves the form INACTIVE; the caller then
 *   1. runs sdqn_dp_probe on every rank (two rounds of the overlapped collectives with bounded waits; *ok = 1: drained in time here),
 *   2. agrees over its control plane (all ranks' ok AND-ed),
 *   3. calls sdqn_dp_set_overlap(agreed) on EVERY rank: 1 activates the form, 0 tears the second communicator down (ncclCommAbort on a
 *      rank whose probe never drained) and the serial form — one all-reduce on the library stream — runs.
 * sdqn_dp_form reports what runs: 0 no communicator, 1 serial, 2 overlapped; *probe = -1 not probed / 0 timed out / 1 ok;
 * *second_comm = 1 while the second communicator exists. */
int sdqn_dp_probe(sdqn_net_t h, int timeout_ms, int inject_timeout, int* ok);
int sdqn_dp_set_overlap(sdqn_net_t h, int on);
int sdqn_dp_form(sdqn_net_t h, int* form, int* probe, int* second_comm);

#ifdef __cplusplus
}
#endif
#endif /* SDQN_H */

// generic_net.h — the DQN train step for the configurations the tuned path does not cover: `--datatype float64`
// (src/main.py:53 -> deepqnetwork.py:33) and screens / history lengths other than 84 x 84 x 4 (src/main.py:27-28,34 ->
// deepqnetwork.py:21-22,28,83-91: the layer stack is the same, its sizes follow the input).  Same algorithm, same C ABI,
// same Neon layouts at the boundary; every layer is an explicit im2col + a tiled FMA GEMM in the network's own
// precision (generic_net.hip).  Selected by sdqn_net_create from the configuration alone; the 84 x 84 x 4 float32 /
// float16 configurations never come here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/sdqn.h"
#include "problems.h"          // NStepArgs
#include "bootstrap.h"         // BootArgs
#include "quantile.h"          // QuantArgs
#include "dueling.h"           // DuelArgs
#include "train_options.h"

namespace sdqn {

hipError_t launch_dueling_mask(void* w5, bool f64, int rows, int H, hipStream_t s);      // sdqn_dueling.hip (kernels.h)

struct GenericNet {
  virtual ~GenericNet() {}
  virtual bool is_f64() const = 0;
  virtual int64_t layer_size(int layer) const = 0;                       // 0..4 = conv1, conv2, conv3, fc4, fc5 (Neon layouts)
  virtual int64_t param_count() const = 0;
  // which: 0 theta, 1 theta-, 2 optimizer state, 3 last gradient sum (get only), 4 second optimizer state; host data float or double
  virtual hipError_t set_param(int which, int layer, const void* host, bool host_f64) = 0;
  virtual hipError_t get_param(int which, int layer, void* host, bool host_f64) = 0;          // synchronises
  // Q(s; theta) of n <= batch_size states already on the device ([n][hist][H][W] u8); q_host [n][A], synchronises
  virtual hipError_t predict_dev(const uint8_t* states_dev, int n, void* q_host, bool host_f64) = 0;
  // the same forward enqueued only (no read-back, no synchronisation); q_dev() is where it leaves Q [n][A] in the network's precision
  virtual hipError_t forward_dev(const uint8_t* states_dev, int n) = 0;
  virtual const void* q_dev() const = 0;
  virtual hipError_t predict_host(const uint8_t* states_host, int n, void* q_host, bool host_f64) = 0;
  // one train step (deepqnetwork.py:107-172) on a device-resident minibatch; asynchronous on the stream
  virtual hipError_t train_dev(const uint8_t* pre, const uint8_t* post, const uint8_t* act, const int64_t* rew,
                               const uint8_t* term, int epoch) = 0;
  virtual hipError_t train_host(const uint8_t* pre, const uint8_t* act, const int64_t* rew, const uint8_t* post,
                                const uint8_t* term, int epoch) = 0;
  // device-resident states (a ReplayMemory's gathered minibatch) + host metadata: only the 10 x B bytes of (r, a, t) are uploaded
  virtual hipError_t train_dev_host_meta(const uint8_t* pre_dev, const uint8_t* post_dev, const uint8_t* act, const int64_t* rew,
                                         const uint8_t* term, int epoch) = 0;
  virtual hipError_t read_cost(double* cost) = 0;                        // cost of the last step (synchronises)
  virtual hipError_t reset_cost_sum() = 0;                               // running sum over steps (train_many's mean)
  virtual hipError_t read_cost_sum(double* sum) = 0;
  virtual hipError_t last_q(void* preq, void* maxpostq, bool host_f64) = 0;
  virtual hipError_t update_target() = 0;                                // deepqnetwork.py:102-105
  // --target_tau: theta- <- theta- + tau (theta - theta-) in the network's precision, three rounded operations; one
  // launch, none without a target net
  virtual hipError_t soft_update(double tau) = 0;
  virtual bool has_target() const = 0;
  // The target options (train_options.h) are the handle's: the net reads the TrainOptions it was made with where it builds its head's
  // arguments and decides on its extra forwards, and keeps no copy.  prepare(next) allocates what a step under `next` needs that the net
  // does not have yet (the Q rows of --double_dqn's and --munchausen / --advantage_learning's extra forwards, the read-outs of
  // --quantiles and --dueling) and commits nothing: the API setter assigns `next` when it has succeeded (sdqn_api_net.hip) — the
  // counterpart of ensure_slots3 / dalloc on the tuned path.  Which options combine, and their ranges, is the setter's to refuse
  virtual hipError_t prepare(const TrainOptions& next) = 0;
  // --prioritized_replay (sdqn_per.hip): w != nullptr makes the following train steps weight the taken action's row by w[n] and write the
  // new priority (|delta| + eps)^alpha into newp[n]; nullptr: the standard step
  virtual void set_per(const float* w, float* newp, double alpha, double eps) = 0;
  // --bootstrap_heads (bootstrap.h): boot_idx names the [B] ring indexes of the NEXT step's samples (device-readable; copied
  // on the stream) or, nullptr, none (tuple path, P = 1; also what sdqn_net_set_bootstrap leaves)
  virtual hipError_t boot_idx(const int64_t* idx) = 0;
  // --quantiles (quantile.h) / --dueling (dueling.h): what the last train step's head left, as doubles;
  // dueling_mask_weights applies fc5's block mask to W5 of theta (0) or theta_t (1)
  virtual hipError_t last_quantile_step(double* targets, double* dq) = 0;      // [B][N] targets, [B][A] dq row
  virtual hipError_t dueling_mask_weights(int which) = 0;
  virtual hipError_t last_dueling_step(double* y, double* delta, double* dq) = 0;
  // --clip_grad_norm (sdqn_clip.h): set_clip(true) makes train_dev / train_host / train_dev_host_meta stop behind the
  // gradient — the caller then enqueues clip_sqnorm, clip_scale (divisor bsz, max norm G) and apply_deferred (the step's optimizer
  // launch), one launch each; clip_record reads {norm, scale} of the last clip_scale (synchronises)
  virtual hipError_t set_clip(bool on) = 0;
  virtual hipError_t clip_sqnorm() = 0;
  virtual hipError_t clip_scale(double bsz, double max_norm) = 0;
  virtual hipError_t apply_deferred() = 0;
  virtual hipError_t clip_record(double* norm_scale) = 0;
  virtual size_t state_bytes() const = 0;                                // hist * H * W
};

// nullptr + *err on failure (bad geometry, out of memory); opt: the handle's options, which outlive the net
GenericNet* make_generic_net(const sdqn_net_cfg& c, const TrainOptions* opt, hipStream_t stream, std::string* err);

// the standalone replay gather for any geometry (replay_memory.py:71-78): pre[k] = frames idx-hist .. idx-1, post[k] = idx-hist+1 .. idx
struct GatherGenericArgs {
  const uint8_t* ring; const void* meta /*MetaRec[]*/; const int64_t* idx /*device*/;
  uint8_t *pre, *post, *actions; int64_t* rewards; uint8_t* terminals;
  int B, hist; int64_t frame;
  NStepArgs ns;                 // --n_step: poststate = frames idx-hist+n .. idx+n-1; rewards / terminals receive (R, done)
};
hipError_t launch_gather_generic(const GatherGenericArgs& g, hipStream_t s);

}  // namespace sdqn

// train_options.h — the STATE of the target options, once.  Plain C++17 (no HIP include: tests/emul compiles it with g++, as it does
// launch_route.h).  sdqn_net_s holds one TrainOptions (api_internal.h: opt); the tuned path reads it where it plans and launches a step,
// the generic net (generic_net.hip) holds a pointer to the same object and reads it where it builds its head's arguments.  Which options
// combine is option_table.h's; what each one computes is its rule header's (td_rule.h, munchausen.h, ...).
//
// Only the API setters write it (sdqn_api_net.hip), all in one shape: check the ranges, edit a COPY, refuse by the option table, allocate
// what the copy needs (GenericNet::prepare, or ensure_slots3 / dalloc on the tuned path), and only then assign the copy — a refused or
// failed call leaves every field as it was.  The ranges the setters hold, which the readers rely on instead of clamping again:
// al_alpha in [0, 1) with al_persistent only beside al_alpha > 0; cql_alpha finite and >= 0; boot_K, quant_N >= 1 and dividing the net's
// outputs; mu_tau > 0, mu_alpha in [0, 1], mu_clip <= 0; n_step >= 1.
#pragma once
#include <stdint.h>

namespace sdqn {

struct TrainOptions {
  bool double_dqn = false;                                          // --double_dqn (option "double_dqn")
  int n_step = 1; double gamma_n = 0.0;                             // --n_step (option "n_step"); gamma_n: discount^n_step (nstep_gamma_n), set WITH n_step: both paths read it when n_step > 1
  bool munchausen = false; double mu_alpha = 0.9, mu_tau = 0.03, mu_clip = -1.0;      // --munchausen
  double al_alpha = 0.0; bool al_persistent = false;                // --advantage_learning / --persistent_advantage: alpha > 0 is "on"
  double cql_alpha = 0.0;                                           // --cql_alpha: > 0 is "on"
  int boot_K = 1; double boot_P = 1.0; uint64_t boot_seed = 0, boot_thresh = 1ull << 53;   // --bootstrap_heads: thresh = ceil(P 2^53)
  int quant_N = 1;                                                  // --quantiles
  bool dueling = false;                                             // --dueling
};

inline bool advantage_on(const TrainOptions& o) { return o.al_alpha > 0.0; }
inline bool cql_on(const TrainOptions& o) { return o.cql_alpha > 0.0; }
inline bool bootstrap_on(const TrainOptions& o) { return o.boot_K > 1; }
inline bool quantiles_on(const TrainOptions& o) { return o.quant_N > 1; }
// --munchausen / --advantage_learning: the target net runs on the prestates in front of the step (option_table.h refuses the two together)
inline bool prestate_target_forward(const TrainOptions& o) { return o.munchausen || advantage_on(o); }
// A net for a game of GA actions has output_multiplier x GA outputs (K Q-heads or N quantiles per action), --dueling: GA + 1 (the V row)
inline int output_multiplier(const TrainOptions& o) { return o.boot_K * o.quant_N; }
inline int net_outputs(const TrainOptions& o, int game_actions) { return output_multiplier(o) * game_actions + (o.dueling ? 1 : 0); }
inline int game_actions(const TrainOptions& o, int outputs) { return o.dueling ? outputs - 1 : outputs / output_multiplier(o); }

}  // namespace sdqn

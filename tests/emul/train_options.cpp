// train_options.cpp — simple_dqn_amd/csrc/train_options.h on the host, for tests/test_train_options.py: built with g++, no HIP.  Prints the
// default TrainOptions, then one line per setting with the derived predicates and the output arithmetic for a game of 4 actions.
#include <stdio.h>
#include "../../simple_dqn_amd/csrc/train_options.h"

using namespace sdqn;

static void show(const char* name, const TrainOptions& o) {
  const int GA = 4, outputs = net_outputs(o, GA);
  printf("case %s advantage_on=%d cql_on=%d bootstrap_on=%d quantiles_on=%d prestate_target_forward=%d multiplier=%d outputs=%d game_actions=%d\n", name,
         (int)advantage_on(o), (int)cql_on(o), (int)bootstrap_on(o), (int)quantiles_on(o), (int)prestate_target_forward(o), output_multiplier(o), outputs,
         game_actions(o, outputs));
}

int main() {
  const TrainOptions d;
  printf("default double_dqn=%d n_step=%d gamma_n=%.17g munchausen=%d mu_alpha=%.17g mu_tau=%.17g mu_clip=%.17g al_alpha=%.17g al_persistent=%d cql_alpha=%.17g "
         "boot_K=%d boot_P=%.17g boot_seed=%llu boot_thresh=%llu quant_N=%d dueling=%d\n", (int)d.double_dqn, d.n_step, d.gamma_n, (int)d.munchausen, d.mu_alpha,
         d.mu_tau, d.mu_clip, d.al_alpha, (int)d.al_persistent, d.cql_alpha, d.boot_K, d.boot_P, (unsigned long long)d.boot_seed,
         (unsigned long long)d.boot_thresh, d.quant_N, (int)d.dueling);
  TrainOptions o;
  show("off", o);
  o = d; o.double_dqn = true; show("double_dqn", o);
  o = d; o.n_step = 3; o.gamma_n = 0.99 * 0.99 * 0.99; show("n_step", o);
  o = d; o.munchausen = true; show("munchausen", o);
  o = d; o.al_alpha = 0.5; show("advantage_learning", o);
  o = d; o.al_alpha = 0.5; o.al_persistent = true; show("persistent_advantage", o);
  o = d; o.cql_alpha = 1.0; show("cql_alpha", o);
  o = d; o.boot_K = 3; show("bootstrap_heads", o);
  o = d; o.quant_N = 2; show("quantiles", o);
  o = d; o.dueling = true; show("dueling", o);
  return 0;
}

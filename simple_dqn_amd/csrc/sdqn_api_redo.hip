// sdqn_api_redo.hip — dormant-neuron recycling (--redo_interval): the host side.  The rules are redo.h's, the kernels sdqn_redo.hip's.
//   scores   two launches (partial sums, scores) over slot 0 of a1..a4 (h_a1..h_a3 on a float16 net): the online net's prestate activations
//            as the last train step left them
//   event    scores, then one apply launch on theta / state / state2 and the event's record, then the derived copies of the online weights
//            in front of fc5 (refresh_derived)
// Everything is enqueued on the library stream; nothing here waits for the device but the two read-outs.
#include "api_internal.h"

static int redo_buffers(sdqn_net_s* h) {
  if (h->redo_scores) return SDQN_OK;
  int rc = dalloc(h, (void**)&h->redo_partial, (size_t)redo_partial_doubles(h->B) * 8); if (rc) return rc;
  rc = dalloc(h, (void**)&h->redo_scores, (size_t)RELU_UNITS * 4); if (rc) return rc;
  return dalloc(h, (void**)&h->redo_info, 6 * 8);
}
static int redo_scores_enqueue(sdqn_net_s* h) {
  ARGCHK(h->train_iterations > 0, "no train step has run: there are no activations to score");
  ARGCHK(h->redo_acts_live, "a forward of its own (predict, act) has overwritten the last train step's activations: score them before it, or run a train step");
  int rc = redo_buffers(h); if (rc) return rc;
  RedoScoreArgs s; memset(&s, 0, sizeof s);
  const bool half = h->cfg.datatype == 1;
  s.a[0] = half ? (const void*)h->h_a1 : (const void*)h->a1; s.a[1] = half ? (const void*)h->h_a2 : (const void*)h->a2;
  s.a[2] = half ? (const void*)h->h_a3 : (const void*)h->a3; s.a[3] = h->a4;
  s.half123 = half ? 1 : 0; s.B = h->B; s.partial = h->redo_partial; s.scores = h->redo_scores;
  LAUNCH(K_UPDATE, launch_redo_scores(s, 0, g_stream));
  LAUNCH(K_UPDATE, launch_redo_scores(s, 1, g_stream));
  return SDQN_OK;
}
int redo_event(sdqn_net_s* h) {
  { int rc = join_comm(h); if (rc) return rc; }            // (a single rank's overlapped form may still be applying fc4 on the side stream)
  int rc = redo_scores_enqueue(h); if (rc) return rc;
  RedoApplyArgs a; memset(&a, 0, sizeof a);
  a.scores = h->redo_scores; a.theta = h->theta; a.state = h->state; a.state2 = h->state2; a.n = h->NPW;
  a.tau = h->redo_tau; a.seed = h->redo_seed; a.event = (uint64_t)(h->redo_events + 1); a.step = h->train_iterations; a.info = h->redo_info;
  LAUNCH(K_UPDATE, launch_redo_apply(a, g_stream));
  h->redo_events += 1;
  h->spec_pending = false;                 // the online parameters moved under a speculative acting forward
  return refresh_derived(h, 0, 0, OFF5);   // (fc5 gets +0.0 only: its mask has nothing to do)
}

extern "C" int sdqn_net_set_redo(sdqn_net_t h, int interval, double tau, uint64_t seed) {
  ARGCHK(h, "NULL handle");
  ARGCHK(interval >= 0, "redo_interval %d: must be >= 0 (0: off)", interval);
  ARGCHK(tau >= 0.0 && tau < 1.0, "redo_threshold %g: must be in [0, 1)", tau);      // (false for a NaN)
  if (interval > 0) {
    int rc = refuse_feature(h, FEAT_REDO, "redo_interval"); if (rc) return rc;
    rc = redo_buffers(h); if (rc) return rc;
  }
  h->redo_interval = interval; h->redo_tau = tau; h->redo_seed = seed;
  return SDQN_OK;
}
extern "C" int sdqn_net_get_redo(sdqn_net_t h, int* interval, double* tau, uint64_t* seed) {
  ARGCHK(h, "NULL handle");
  if (interval) *interval = h->redo_interval; if (tau) *tau = h->redo_tau; if (seed) *seed = h->redo_seed;
  return SDQN_OK;
}
extern "C" int sdqn_net_redo_now(sdqn_net_t h) {
  ARGCHK(h, "NULL handle");
  int rc = refuse_feature(h, FEAT_REDO, "redo_now"); if (rc) return rc;
  return redo_event(h);
}
extern "C" int sdqn_net_redo_scores(sdqn_net_t h, float* out) {
  ARGCHK(h && out, "NULL argument");
  int rc = refuse_feature(h, FEAT_REDO, "redo_scores"); if (rc) return rc;
  rc = redo_scores_enqueue(h); if (rc) return rc;
  HIPCHK(hipMemcpyAsync(out, h->redo_scores, (size_t)RELU_UNITS * 4, hipMemcpyDeviceToHost, g_stream));
  HIPCHK(hipStreamSynchronize(g_stream));
  return per_check_all();
}
extern "C" int sdqn_net_redo_last(sdqn_net_t h, int64_t* out) {
  ARGCHK(h && out, "NULL argument");
  if (h->redo_events == 0) { for (int i = 0; i < 6; ++i) out[i] = 0; return SDQN_OK; }      // (no event yet: event number 0)
  HIPCHK(hipMemcpyAsync(out, h->redo_info, 6 * 8, hipMemcpyDeviceToHost, g_stream));
  HIPCHK(hipStreamSynchronize(g_stream));
  return per_check_all();
}
// ---- the host restatement (no device) ---------------------------------------------------------------------------------------------------
extern "C" int sdqn_redo_apply_host(const float* scores, double tau, uint64_t seed, uint64_t event, int A, float* theta, float* state, float* state2,
                                    int64_t* counts) {
  ARGCHK(scores && theta, "NULL argument");
  ARGCHK(A >= 1 && A <= MAX_ACTIONS, "num_actions must be in 1..%d (got %d)", MAX_ACTIONS, A);
  ARGCHK(tau >= 0.0 && tau < 1.0, "redo_threshold %g: must be in [0, 1)", tau);
  redo_apply_host(scores, tau, seed, event, OFF5 + (int64_t)A * NFC, theta, state, state2, counts);
  return SDQN_OK;
}
extern "C" int sdqn_redo_draw(uint64_t seed, uint64_t event, int64_t index, int layer, uint64_t* word, float* value) {
  return keyed_init_draw(redo_key(seed, event), index, layer, REDO_LAYERS, word, value);
}

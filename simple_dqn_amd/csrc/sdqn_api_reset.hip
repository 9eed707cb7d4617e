// sdqn_api_reset.hip — periodic resets with shrink-and-perturb (--reset_interval): the host side.  The rules are reset.h's, the
// kernel sdqn_reset.hip's.
//   event    one apply launch on theta / theta_t / state / state2 and the event's record, then both nets' derived copies from the first
//            entry the rule writes (refresh_derived)
// Everything is enqueued on the library stream; nothing here waits for the device but sdqn_net_reset_last.
#include "api_internal.h"

static int reset_rule_check(int layers, double alpha) {
  ARGCHK(layers >= 0 && layers <= RESET_LAYERS, "reset_layers %d: must be in 0..%d", layers, RESET_LAYERS);
  ARGCHK(alpha >= 0.0 && alpha <= 1.0, "shrink_perturb %g: must be in [0, 1]", alpha);      // (false for a NaN)
  return SDQN_OK;
}
int reset_event(sdqn_net_s* h) {
  ARGCHK(!reset_noop(h->reset_layers, h->reset_alpha), "reset_layers 0 with shrink_perturb 1 resets nothing");
  { int rc = join_comm(h); if (rc) return rc; }            // (a single rank's overlapped form may still be applying fc4 on the side stream)
  if (!h->reset_info) { int rc = dalloc(h, (void**)&h->reset_info, 2 * 8); if (rc) return rc; }
  const bool tgt = h->theta_t != h->theta;
  ResetApplyArgs a; memset(&a, 0, sizeof a);
  a.theta = h->theta; a.theta_t = tgt ? h->theta_t : nullptr; a.state = h->state; a.state2 = h->state2; a.n = h->NPW;
  a.layers = h->reset_layers; a.alpha = h->reset_alpha; a.seed = h->reset_seed; a.event = (uint64_t)(h->reset_events + 1);
  a.step = h->train_iterations; a.info = h->reset_info;
  LAUNCH(K_UPDATE, launch_reset_apply(a, g_stream));
  h->reset_events += 1;
  h->spec_pending = false;                 // the online parameters moved under a speculative acting forward
  for (int zz = 0; zz < (tgt ? 2 : 1); ++zz) {      // (fc5 is in every event's tail)
    int rc = refresh_derived(h, zz, reset_first(h->reset_layers, h->reset_alpha), h->NPW); if (rc) return rc;
  }
  return SDQN_OK;
}

extern "C" int sdqn_net_set_reset(sdqn_net_t h, int interval, int layers, double alpha, uint64_t seed) {
  ARGCHK(h, "NULL handle");
  ARGCHK(interval >= 0, "reset_interval %d: must be >= 0 (0: off)", interval);
  int rc = reset_rule_check(layers, alpha); if (rc) return rc;
  if (interval > 0) {
    ARGCHK(!reset_noop(layers, alpha), "reset_interval %d with reset_layers 0 and shrink_perturb 1 would reset nothing", interval);
    rc = refuse_feature(h, FEAT_RESET, "reset_interval"); if (rc) return rc;
    if (!h->reset_info) { rc = dalloc(h, (void**)&h->reset_info, 2 * 8); if (rc) return rc; }
  }
  h->reset_interval = interval; h->reset_layers = layers; h->reset_alpha = alpha; h->reset_seed = seed;
  return SDQN_OK;
}
extern "C" int sdqn_net_get_reset(sdqn_net_t h, int* interval, int* layers, double* alpha, uint64_t* seed) {
  ARGCHK(h, "NULL handle");
  if (interval) *interval = h->reset_interval; if (layers) *layers = h->reset_layers; if (alpha) *alpha = h->reset_alpha; if (seed) *seed = h->reset_seed;
  return SDQN_OK;
}
extern "C" int sdqn_net_reset_now(sdqn_net_t h) {
  ARGCHK(h, "NULL handle");
  int rc = refuse_feature(h, FEAT_RESET, "reset_now"); if (rc) return rc;
  return reset_event(h);
}
extern "C" int sdqn_net_reset_last(sdqn_net_t h, int64_t* out) {
  ARGCHK(h && out, "NULL argument");
  if (h->reset_events == 0) { out[0] = out[1] = 0; return SDQN_OK; }      // (no event yet: event number 0)
  HIPCHK(hipMemcpyAsync(out, h->reset_info, 2 * 8, hipMemcpyDeviceToHost, g_stream));
  HIPCHK(hipStreamSynchronize(g_stream));
  return per_check_all();
}
// ---- the host restatement (no device) ---------------------------------------------------------------------------------------------------
extern "C" int sdqn_reset_apply_host(int layers, double alpha, uint64_t seed, uint64_t event, int A, int optimizer, float* theta, float* theta_t,
                                     float* state, float* state2) {
  ARGCHK(theta, "NULL argument");
  ARGCHK(A >= 1 && A <= MAX_ACTIONS, "fc5 rows must be in 1..%d (got %d)", MAX_ACTIONS, A);
  ARGCHK(optimizer >= 0 && optimizer <= 2, "optimizer %d: 0 rmsprop, 1 adam, 2 adadelta", optimizer);
  int rc = reset_rule_check(layers, alpha); if (rc) return rc;
  ARGCHK(optimizer == 0 || state2, "optimizer %d keeps a second state: state2 is NULL", optimizer);
  reset_apply_host(layers, alpha, seed, event, OFF5 + (int64_t)A * NFC, theta, theta_t, state, optimizer == 0 ? nullptr : state2);
  return SDQN_OK;
}
extern "C" int sdqn_reset_draw(uint64_t seed, uint64_t event, int64_t index, int layer, uint64_t* word, float* value) {
  return keyed_init_draw(reset_key(seed, event), index, layer, RESET_LAYERS, word, value);
}

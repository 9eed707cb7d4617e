// sdqn_api_regularize.hip — decoupled weight decay and L2-init regularisation (--weight_decay, --l2_init): the host side.  The rule
// is regularize.h's, the kernels sdqn_regularize.hip's.
//   step     regularize_launch from step_applied: one launch on the online weights and their derived copies; with --target_tau in (0, 1)
//            and a target net the SAME launch blends theta- and writes the target's derived copies (fuse)
//   now      the same launch outside a step, never fused
//   norms    the read-out: two launches and one 80-byte copy, waited for
// Everything is enqueued on the library stream; nothing here waits for the device but the read-outs.
#include "api_internal.h"

static int regularize_range_check(double wd, double lambda, double lr) {
  const int e = reg_range_error(wd, lambda, lr);
  ARGCHK(e != 1, "weight_decay %g: must be >= 0 (0: off)", wd);
  ARGCHK(e != 2, "l2_init %g: must be >= 0 (0: off)", lambda);
  ARGCHK(e != 3, "weight_decay %g: learning_rate x weight_decay = %g must be below 1", wd, lr * wd);
  ARGCHK(e != 4, "l2_init %g: learning_rate x l2_init = %g must be at most 1", lambda, lr * lambda);
  return SDQN_OK;
}
// the anchor = the online weights as of now, in stream order (allocated on first use)
static int anchor_take(sdqn_net_s* h) {
  { int rc = join_comm(h); if (rc) return rc; }
  if (!h->reg_anchor) { int rc = dalloc(h, (void**)&h->reg_anchor, (size_t)h->NPW * 4, false); if (rc) return rc; }
  HIPCHK(hipMemcpyAsync(h->reg_anchor, h->theta, (size_t)h->NPW * 4, hipMemcpyDeviceToDevice, g_stream));
  return SDQN_OK;
}
// one launch of the rule with (wd, lambda); fuse: blend the target net toward the new weights with h->target_tau in the same launch
int regularize_launch(sdqn_net_s* h, double wd, double lambda, bool fuse) {
  { int rc = join_comm(h); if (rc) return rc; }            // (a single rank's overlapped form may still be applying fc4 on the side stream)
  RegularizeArgs a; memset(&a, 0, sizeof a);
  a.theta = h->theta; a.anchor = h->reg_anchor; a.n = h->NPW; a.rule = reg_rule(wd, lambda, h->cfg.learning_rate);
  if (h->cfg.datatype == 1) { a.wh = h->wh[0]; a.wht = h->wht[0]; }
  else a.w1p = h->w1p[0];
  if (fuse) {
    a.theta_t = h->theta_t; a.tau = (float)h->target_tau;
    if (h->cfg.datatype == 1) { a.wh_t = h->wh[1]; a.wht_t = h->wht[1]; }
    else a.w1p_t = h->w1p[1];
  }
  LAUNCH(K_UPDATE, launch_regularize(a, g_stream));
  h->spec_pending = false;                 // the online parameters moved under a speculative acting forward
  return SDQN_OK;
}

extern "C" int sdqn_net_set_regularizer(sdqn_net_t h, double wd, double lambda) {
  ARGCHK(h, "NULL handle");
  int rc = regularize_range_check(wd, lambda, h->cfg.learning_rate); if (rc) return rc;
  if (wd > 0.0) { rc = refuse_feature(h, FEAT_REGULARIZER, "weight_decay"); if (rc) return rc; }
  if (lambda > 0.0) {
    rc = refuse_feature(h, FEAT_REGULARIZER, "l2_init"); if (rc) return rc;
    if (!(h->reg_lambda > 0.0)) { rc = anchor_take(h); if (rc) return rc; }      // 0 -> on: the anchor is the weights as they are now
  }
  h->reg_wd = wd; h->reg_lambda = lambda;
  return SDQN_OK;
}
extern "C" int sdqn_net_get_regularizer(sdqn_net_t h, double* wd, double* lambda) {
  ARGCHK(h, "NULL handle");
  if (wd) *wd = h->reg_wd; if (lambda) *lambda = h->reg_lambda;
  return SDQN_OK;
}
extern "C" int sdqn_net_regularize_with(sdqn_net_t h, double wd, double lambda) {
  ARGCHK(h, "NULL handle");
  int rc = refuse_feature(h, FEAT_REGULARIZER, "regularize_now"); if (rc) return rc;
  rc = regularize_range_check(wd, lambda, h->cfg.learning_rate); if (rc) return rc;
  ARGCHK(!(lambda > 0.0) || h->reg_anchor, "l2_init %g: this network has no anchor yet (sdqn_net_set_regularizer with l2_init > 0, or sdqn_net_anchor_now)", lambda);
  if (!(wd > 0.0) && !(lambda > 0.0)) return SDQN_OK;      // both lines skipped: no launch
  return regularize_launch(h, wd, lambda, false);
}
extern "C" int sdqn_net_regularize_now(sdqn_net_t h) {
  ARGCHK(h, "NULL handle");
  return sdqn_net_regularize_with(h, h->reg_wd, h->reg_lambda);
}
extern "C" int sdqn_net_anchor_now(sdqn_net_t h) {
  ARGCHK(h, "NULL handle");
  int rc = refuse_feature(h, FEAT_REGULARIZER, "anchor_now"); if (rc) return rc;
  return anchor_take(h);
}
extern "C" int sdqn_net_get_anchor(sdqn_net_t h, int layer, float* buf, int64_t n) {
  ARGCHK(h && buf, "NULL argument");
  int rc = refuse_feature(h, FEAT_REGULARIZER, "get_anchor"); if (rc) return rc;
  ARGCHK(h->reg_anchor, "this network has no anchor (l2_init was never set above 0 and sdqn_net_anchor_now never called)");
  ARGCHK(layer >= 0 && layer < 5, "layer %d: must be in 0..4", layer);
  int64_t rows, cols, off; layer_dims(layer, h->A, rows, cols, off);
  ARGCHK(n == rows * cols, "layer %d holds %lld values, got %lld", layer, (long long)(rows * cols), (long long)n);
  std::vector<float> tmp((size_t)n);
  HIPCHK(hipMemcpyAsync(tmp.data(), h->reg_anchor + off, (size_t)n * 4, hipMemcpyDeviceToHost, g_stream));
  HIPCHK(hipStreamSynchronize(g_stream));
  for (int64_t r = 0; r < rows; ++r) for (int64_t c = 0; c < cols; ++c) buf[r * cols + c] = tmp[(size_t)neon_to_internal(layer, r, c)];
  return per_check_all();
}
extern "C" int sdqn_net_weight_norms(sdqn_net_t h, double* out) {
  ARGCHK(h && out, "NULL argument");
  int rc = refuse_feature(h, FEAT_REGULARIZER, "weight_norms"); if (rc) return rc;
  rc = join_comm(h); if (rc) return rc;
  if (!h->reg_norms) { rc = dalloc(h, (void**)&h->reg_norms, (size_t)REG_NORM_DOUBLES * 8); if (rc) return rc; }
  WeightNormArgs a; a.theta = h->theta; a.anchor = h->reg_anchor; a.n = h->NPW; a.buf = h->reg_norms;
  HIPCHK(launch_weight_norms(a, g_stream));
  HIPCHK(hipMemcpyAsync(out, h->reg_norms + 2 * REG_LAYERS * REG_NORM_BLOCKS, 2 * REG_LAYERS * 8, hipMemcpyDeviceToHost, g_stream));
  HIPCHK(hipStreamSynchronize(g_stream));
  if (!h->reg_anchor) for (int l = 0; l < REG_LAYERS; ++l) out[REG_LAYERS + l] = NAN;
  return per_check_all();
}
// ---- the host restatement (no device) ---------------------------------------------------------------------------------------------------
extern "C" int sdqn_regularize_apply_host(double wd, double lambda, double lr, int64_t n, float* theta, const float* anchor) {
  ARGCHK(theta && n >= 0, "bad arguments");
  int rc = regularize_range_check(wd, lambda, lr); if (rc) return rc;
  ARGCHK(!(lambda > 0.0) || anchor, "l2_init %g: anchor is NULL", lambda);
  reg_apply_host(wd, lambda, lr, n, theta, anchor);
  return SDQN_OK;
}

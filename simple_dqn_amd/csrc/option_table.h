// option_table.h — WHICH training options combine, as data.  Plain C++17 (no HIP include).  One row per option, one entry per refused
// pair; option_conflict() is the only code that reads them.  The setters (sdqn_api_net.hip: refuse_conflicts) ask it before they change
// anything, step_plan (sdqn_api_step.hip) takes the step's head from the row of the option that is on, and sdqn_option_name /
// sdqn_option_conflict show the table to a caller without a device (tests/test_option_table.py holds deepqnetwork.py's table to it;
// DESIGN.md 36 prints the matrix).  A new head option is one row, its entries below, and one refuse_conflicts call in its setter.
#pragma once
#include <stdio.h>
#include "launch_route.h"

namespace sdqn {

enum OptionId {
  OPT_DOUBLE_DQN = 0, OPT_MUNCHAUSEN, OPT_ADVANTAGE_LEARNING, OPT_CQL_ALPHA, OPT_BOOTSTRAP_HEADS, OPT_QUANTILES, OPT_DUELING, OPT_NOISY_NETS,
  OPT_BATCH_NORM, OPT_CLIP_GRAD_NORM, OPT_TARGET_TAU, OPT_COUNT
};
// name: as the messages print it; prints_value: ... followed by its value ("bootstrap_heads 2"); head: the HeadMode of a train step's head
// while the option is on (0: the option has no head of its own)
struct OptionRow { const char* name; bool prints_value; int head; };
constexpr OptionRow OPTIONS[OPT_COUNT] = {
  {"double_dqn", false, HEAD_DOUBLE}, {"munchausen", false, HEAD_MUNCHAUSEN}, {"advantage_learning", false, HEAD_ADVANTAGE}, {"cql_alpha", false, HEAD_CQL},
  {"bootstrap_heads", true, HEAD_BOOTSTRAP}, {"quantiles", true, HEAD_QUANTILE}, {"dueling", false, HEAD_DUELING}, {"noisy_nets", false, 0},
  {"batch_norm", false, 0}, {"clip_grad_norm", false, 0}, {"target_tau", false, 0},
};

// The refused pairs, each once (either order is refused, in the same words); reason: what the message appends after ": ", or nullptr.
// The six options with a head of their own exclude each other, double_dqn, noisy_nets and batch_norm; noisy_nets also excludes batch_norm,
// clip_grad_norm and target_tau.  Every option with a non-zero head excludes every other one: a step has ONE head (option_head).
struct OptionConflict { int a, b; const char* reason; };
constexpr const char* NO_THIRD_SLOT = "the shared head body carries no third slot";
constexpr const char* NO_BN_THIRD_FORWARD = "inference-mode statistics for its third forward are not defined";
constexpr OptionConflict OPTION_CONFLICTS[] = {
  {OPT_MUNCHAUSEN, OPT_DOUBLE_DQN, "the Munchausen target has no argmax for the online net to choose"},
  {OPT_MUNCHAUSEN, OPT_ADVANTAGE_LEARNING, "both targets want q slot 2 for a head of their own"},
  {OPT_MUNCHAUSEN, OPT_CQL_ALPHA, nullptr}, {OPT_MUNCHAUSEN, OPT_BOOTSTRAP_HEADS, nullptr}, {OPT_MUNCHAUSEN, OPT_QUANTILES, nullptr},
  {OPT_MUNCHAUSEN, OPT_DUELING, nullptr}, {OPT_MUNCHAUSEN, OPT_NOISY_NETS, nullptr}, {OPT_MUNCHAUSEN, OPT_BATCH_NORM, NO_BN_THIRD_FORWARD},
  {OPT_ADVANTAGE_LEARNING, OPT_DOUBLE_DQN, "q slot 2 is taken by its third forward"},
  {OPT_ADVANTAGE_LEARNING, OPT_CQL_ALPHA, nullptr}, {OPT_ADVANTAGE_LEARNING, OPT_BOOTSTRAP_HEADS, nullptr}, {OPT_ADVANTAGE_LEARNING, OPT_QUANTILES, nullptr},
  {OPT_ADVANTAGE_LEARNING, OPT_DUELING, nullptr}, {OPT_ADVANTAGE_LEARNING, OPT_NOISY_NETS, nullptr}, {OPT_ADVANTAGE_LEARNING, OPT_BATCH_NORM, NO_BN_THIRD_FORWARD},
  {OPT_CQL_ALPHA, OPT_DOUBLE_DQN, NO_THIRD_SLOT},
  {OPT_CQL_ALPHA, OPT_BOOTSTRAP_HEADS, nullptr}, {OPT_CQL_ALPHA, OPT_QUANTILES, nullptr}, {OPT_CQL_ALPHA, OPT_DUELING, nullptr},
  {OPT_CQL_ALPHA, OPT_NOISY_NETS, nullptr}, {OPT_CQL_ALPHA, OPT_BATCH_NORM, nullptr},
  {OPT_BOOTSTRAP_HEADS, OPT_DOUBLE_DQN, nullptr}, {OPT_BOOTSTRAP_HEADS, OPT_QUANTILES, nullptr}, {OPT_BOOTSTRAP_HEADS, OPT_DUELING, nullptr},
  {OPT_BOOTSTRAP_HEADS, OPT_NOISY_NETS, nullptr}, {OPT_BOOTSTRAP_HEADS, OPT_BATCH_NORM, nullptr},
  {OPT_QUANTILES, OPT_DOUBLE_DQN, nullptr}, {OPT_QUANTILES, OPT_DUELING, nullptr}, {OPT_QUANTILES, OPT_NOISY_NETS, nullptr}, {OPT_QUANTILES, OPT_BATCH_NORM, nullptr},
  {OPT_DUELING, OPT_DOUBLE_DQN, NO_THIRD_SLOT}, {OPT_DUELING, OPT_NOISY_NETS, nullptr}, {OPT_DUELING, OPT_BATCH_NORM, nullptr},
  {OPT_NOISY_NETS, OPT_BATCH_NORM, nullptr},
  {OPT_NOISY_NETS, OPT_CLIP_GRAD_NORM, "the norm would have to include sigma's gradient"},
  {OPT_NOISY_NETS, OPT_TARGET_TAU, "the blend would have to cover sigma"},
};
static_assert(sizeof OPTION_CONFLICTS / sizeof OPTION_CONFLICTS[0] == 36, "36 refused pairs");

constexpr unsigned option_bit(int id) { return 1u << id; }
constexpr bool option_id_ok(int id) { return id >= 0 && id < OPT_COUNT; }
inline const OptionConflict* option_pair(int a, int b) {
  for (const OptionConflict& c : OPTION_CONFLICTS) if ((c.a == a && c.b == b) || (c.a == b && c.b == a)) return &c;
  return nullptr;
}
// the head of a train step with these options on (the table lets at most one option with a head through); 0: none of them has one
inline int option_head(unsigned active_mask) {
  for (int id = 0; id < OPT_COUNT; ++id) if ((active_mask & option_bit(id)) && OPTIONS[id].head) return OPTIONS[id].head;
  return 0;
}
inline void option_label(int id, int value, char* out, size_t cap) {
  if (OPTIONS[id].prints_value) snprintf(out, cap, "%s %d", OPTIONS[id].name, value); else snprintf(out, cap, "%s", OPTIONS[id].name);
}
// Switching `setting` on (with value setting_value, printed where its row says so) beside the options in active_mask (values[id]: theirs):
// the first active option it is refused with, and the refusal's message in buf; -1 and an empty buf when it combines with all of them.
inline int option_conflict(int setting, int setting_value, unsigned active_mask, const int* values, char* buf, int cap) {
  if (buf && cap > 0) buf[0] = 0;
  for (int other = 0; other < OPT_COUNT; ++other) {
    const OptionConflict* c = (active_mask & option_bit(other)) ? option_pair(setting, other) : nullptr;
    if (!c) continue;
    char first[48], second[48];
    option_label(setting, setting_value, first, sizeof first); option_label(other, values ? values[other] : 0, second, sizeof second);
    if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s cannot be combined with %s%s%s", first, second, c->reason ? ": " : "", c->reason ? c->reason : "");
    return other;
  }
  return -1;
}

// ---- the features that move the weights behind an applied step (--redo_interval, --reset_interval, --weight_decay / --l2_init) -----------
// They refuse properties of the NET, not other options, so they have rows of their own: the label the feature's value prints with (one
// int, or two doubles), why it cannot run beside each property, its DESIGN section.  feature_refusal words the refusal from the feature's
// side (its setters and *_now calls), feature_refuses from the property's (sdqn_net_set_noisy, sdqn_dp_init); no reason is written twice.
enum FeatureId { FEAT_REDO = 0, FEAT_RESET, FEAT_REGULARIZER, FEAT_COUNT };
enum NetProperty { NET_BATCH_NORM = 0, NET_NOISY_NETS, NET_DATA_PARALLEL, NET_PROPERTIES };
struct FeatureRow { const char* label; const char* reason[NET_PROPERTIES]; int section; };
constexpr FeatureRow FEATURES[FEAT_COUNT] = {
  {"redo_interval %d", {"the stored planes are not what the next layer reads", "sigma would have to be recycled too", "the ranks' activations differ"}, 37},
  {"reset_interval %d", {"the running statistics would have to be reset too", "sigma would have to be reset too", "every rank would have to run the same event"}, 38},
  {"weight_decay %g / l2_init %g", {"its block of the flat buffer is not weights", "sigma would have to be regularised too",
                                    "every rank would have to hold the same anchor and run the rule behind the overlapped fc4 update"}, 39},
};
// `flag` (a feature's option or entry point) on a net with these properties (ranks: of its communicator, 1 without one): true and the
// message in buf when the feature refuses the net
inline bool feature_refusal(int feature, const char* flag, bool generic, bool batch_norm, bool noisy, int ranks, char* buf, size_t cap) {
  const char* const* why = FEATURES[feature].reason;
  if (generic) snprintf(buf, cap, "%s is implemented for the 84x84x4 float32 / float16 configurations (not datatype float64 or other geometries: the generic path)", flag);
  else if (batch_norm) snprintf(buf, cap, "%s cannot be combined with batch_norm: %s", flag, why[NET_BATCH_NORM]);
  else if (noisy) snprintf(buf, cap, "%s cannot be combined with noisy_nets: %s", flag, why[NET_NOISY_NETS]);
  else if (ranks > 1) snprintf(buf, cap, "%s cannot be combined with data parallel on %d ranks: %s", flag, ranks, why[NET_DATA_PARALLEL]);
  else return false;
  return true;
}
// the reverse question: the net is about to get `property` (NET_NOISY_NETS, or NET_DATA_PARALLEL on `ranks` ranks) while `feature` is on
// with values v (v[1]: the regulariser's second): true and the message in buf when the feature refuses it
inline bool feature_refuses(int feature, int property, int ranks, const double* v, char* buf, size_t cap) {
  if (property == NET_DATA_PARALLEL && ranks <= 1) return false;
  const FeatureRow& f = FEATURES[feature];
  char label[96];
  if (feature == FEAT_REGULARIZER) snprintf(label, sizeof label, f.label, v[0], v[1]); else snprintf(label, sizeof label, f.label, (int)v[0]);
  if (property == NET_NOISY_NETS) snprintf(buf, cap, "noisy_nets cannot be combined with %s: %s", label, f.reason[property]);
  else snprintf(buf, cap, "data parallel with %d ranks cannot be combined with %s: %s (DESIGN.md §%d)", ranks, label, f.reason[property], f.section);
  return true;
}

}  // namespace sdqn

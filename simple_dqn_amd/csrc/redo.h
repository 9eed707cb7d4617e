// redo.h — dormant-neuron recycling (--redo_interval; ReDo: Sokar, Agarwal, Castro, Evci, ICML 2023): the score rule, the
// draw and the index maps, ONE definition in plain C++, compiled for the host (sdqn_redo_apply_host, sdqn_redo_draw: the oracle's source of
// truth) and for the device (sdqn_redo.hip), like noisy.h and shift.h.
//
//   layers   l = 1..4: conv1, conv2, conv3, fc4 with 32, 64, 64, 512 ReLU units; their scores lie in one buffer of 672 values
//            [s_1 | s_2 | s_3 | s_4] at relu_off(l - 1)
//   score    m_l[j] = mean over the rows of |a_l[row][j]| (fp64, fixed order: sdqn_redo.hip), s_l[j] = m_l[j] / mean_k m_l[k] (0 when the layer
//            mean is 0; the layer sum by halving: m[k] += m[k + n/2], n/2 -> n/4 -> .. -> 1), stored as float.  Unit j is dormant when (double)s_l[j] <= tau
//   entry    flat index i of the weight buffer (problems.h: internal layouts) lies in layer L = 1..5; it FEEDS unit `in` of layer L (none for
//            fc5) and MULTIPLIES unit `src` of layer L - 1 (none for conv1):
//              W1i [(c,r,s)][32]   in = i % 32
//              W2i [(r,s,c)][64]   in = i % 64,  src = (i / 64) % 32
//              W3i [(r,s,c)][64]   in = i % 64,  src = (i / 64) % 64
//              W4i [(pix,f)][512]  in = i % 512, src = (i / 512) % 64
//              W5i [A][512]                      src = i % 512
//   rule     src dormant -> +0.0 (zeroing wins) | else in dormant -> redo_draw | else kept.  The optimizer states of a redrawn or zeroed entry
//            go back to +0.0, a fresh network's value
//   draw     key = mix(mix(seed + G) + G (event + 1)), w = mix(key + G (i + 1)) = stream_keyed(key, i) with the flat index i of the WHOLE
//            buffer (mix, G: stream.h); value = init_draw(w, L) = (u * 2^-23 - 1) * k in float, u = w >> 40 (the top 24 bits), k =
//            float(sqrt(3 / fan_in)) of the entry's layer (net_layout.h: the initialiser of deepqnetwork.py); the product by 2^-23 and the
//            difference are exact, the product by k is rounded once
#pragma once
#include <stdint.h>
#include "net_layout.h"
#include "stream.h"

namespace sdqn {

constexpr int REDO_LAYERS = RELU_LAYERS;      // the 672 scores are net_layout.h's per-unit values: relu_units(l) of them at relu_off(l)

SDQN_HD uint64_t redo_key(uint64_t seed, uint64_t event) { return stream_keyed(stream_keyed(seed, 0), event); }
// init_draw of a ReLU layer, L = 1..4.  Written over relu_init_bound, not init_bound: redo_apply_kernel evaluates it for fc5's entries too,
// where the value is never used (they feed no unit), and fc5's case in init_bound would change that kernel's bytes for nothing
SDQN_HD float redo_draw(uint64_t key, uint64_t i, int L) { return stream_unit24(stream_keyed(key, i)) * relu_init_bound(L); }
// what entry i of the flat weight buffer is: its layer L = 1..5, the unit it feeds (index into the 672 scores, -1: none) and the unit it
// multiplies (likewise)
struct RedoEntry { int L, in, src; };
SDQN_HD RedoEntry redo_entry(int64_t i) {
  RedoEntry e;
  if (i < OFF2) { e.L = 1; e.in = relu_off(0) + (int)(i & 31); e.src = -1; }
  else if (i < OFF3) { const int64_t r = i - OFF2; e.L = 2; e.in = relu_off(1) + (int)(r & 63); e.src = relu_off(0) + (int)((r >> 6) & 31); }
  else if (i < OFF4) { const int64_t r = i - OFF3; e.L = 3; e.in = relu_off(2) + (int)(r & 63); e.src = relu_off(1) + (int)((r >> 6) & 63); }
  else if (i < OFF5) { const int64_t r = i - OFF4; e.L = 4; e.in = relu_off(3) + (int)(r & 511); e.src = relu_off(2) + (int)((r >> 9) & 63); }
  else { const int64_t r = i - OFF5; e.L = 5; e.in = -1; e.src = relu_off(3) + (int)(r & 511); }
  return e;
}
SDQN_HD bool redo_dormant(float score, double tau) { return (double)score <= tau; }
// 0 kept | 1 redrawn | 2 zeroed
SDQN_HD int redo_action(const float* scores, double tau, const RedoEntry& e) {
  if (e.src >= 0 && redo_dormant(scores[e.src], tau)) return 2;
  if (e.in >= 0 && redo_dormant(scores[e.in], tau)) return 1;
  return 0;
}
// one event on host arrays: theta / state / state2 (may be NULL) [n] in place, n = OFF5 + 512 A; counts (may be NULL): dormant units per layer
inline void redo_apply_host(const float* scores, double tau, uint64_t seed, uint64_t event, int64_t n, float* theta, float* state, float* state2, int64_t* counts) {
  const uint64_t key = redo_key(seed, event);
  for (int64_t i = 0; i < n; ++i) {
    const RedoEntry e = redo_entry(i);
    const int act = redo_action(scores, tau, e);
    if (!act) continue;
    theta[i] = act == 1 ? redo_draw(key, (uint64_t)i, e.L) : 0.0f;
    if (state) state[i] = 0.0f;
    if (state2) state2[i] = 0.0f;
  }
  if (counts) for (int l = 0; l < REDO_LAYERS; ++l) {
    counts[l] = 0;
    for (int j = relu_off(l); j < relu_off(l + 1); ++j) counts[l] += redo_dormant(scores[j], tau) ? 1 : 0;
  }
}

// sdqn_redo.hip.  The score launches read the online net's prestate half (slot 0) of the last step's activations
struct RedoScoreArgs {
  const void* a[REDO_LAYERS];   // a1 [B*400][32], a2 [B*81][64], a3 [B*49][64] (float, or half when half123), a4 [B][512] (always float)
  int half123;
  int B;
  double* partial;              // redo_partial_doubles(B) doubles: per layer [blocks][units]
  float* scores;                // [672]
};
struct RedoApplyArgs {
  const float* scores;          // [672]
  float* theta; float* state; float* state2;      // [n]; state2 may be NULL
  int64_t n;
  double tau; uint64_t seed, event; int64_t step;
  int64_t* info;                // [6] event, step, dormant counts of the four layers (written by workgroup 0)
};
// rows a workgroup of the first stage reduces, per layer: fixed, so that the order of the sums is a function of the batch size alone
SDQN_HD constexpr int redo_chunk(int l) { return l == 3 ? 32 : 512; }
SDQN_HD constexpr int redo_pix(int l) { return l == 0 ? 400 : l == 1 ? 81 : l == 2 ? 49 : 1; }      // rows per sample
SDQN_HD int redo_blocks(int l, int B) { return (int)(((int64_t)B * redo_pix(l) + redo_chunk(l) - 1) / redo_chunk(l)); }
SDQN_HD int64_t redo_partial_doubles(int B) { int64_t n = 0; for (int l = 0; l < REDO_LAYERS; ++l) n += (int64_t)redo_blocks(l, B) * relu_units(l); return n; }

#if defined(__HIPCC__)
hipError_t launch_redo_scores(const RedoScoreArgs& a, int stage, hipStream_t s);      // stage 0: partial sums, 1: scores
hipError_t launch_redo_apply(const RedoApplyArgs& a, hipStream_t s);
#endif

}  // namespace sdqn

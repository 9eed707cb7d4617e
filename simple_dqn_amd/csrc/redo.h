// redo.h — dormant-neuron recycling (--redo_interval; ReDo: Sokar, Agarwal, Castro, Evci, ICML 2023): the score rule, the
// draw and the index maps, ONE definition in plain C++, compiled for the host (sdqn_redo_apply_host, sdqn_redo_draw: the oracle's source of
// truth) and for the device (sdqn_redo.hip), like noisy.h and shift.h.
//
//   layers   l = 1..4: conv1, conv2, conv3, fc4 with 32, 64, 64, 512 ReLU units; their scores lie in one buffer of 672 values
//            [s_1 | s_2 | s_3 | s_4] at redo_soff(l - 1)
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
//   draw     key = mix(mix(seed + G) + G (event + 1)), w = mix(key + G (i + 1)) with the flat index i of the WHOLE buffer (mix: splitmix64's
//            finaliser, G its increment; integers mod 2^64); u = w >> 40 (the top 24 bits); value = (u * 2^-23 - 1) * k in float, k =
//            float(sqrt(3 / fan_in)) of the entry's layer (fan_in 256, 512, 576, 3136: the initialiser of deepqnetwork.py); the product by
//            2^-23 and the difference are exact, the product by k is rounded once
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define REDO_HD __host__ __device__ inline
#else
#define REDO_HD inline
#endif

namespace sdqn {

constexpr int REDO_LAYERS = 4, REDO_UNITS = 32 + 64 + 64 + 512;      // 672
REDO_HD constexpr int redo_soff(int l) { return l == 0 ? 0 : l == 1 ? 32 : l == 2 ? 96 : l == 3 ? 160 : 672; }      // first score of layer l + 1
// the flat buffer's layer boundaries (problems.h: OFF1..OFF5, restated so that this header stands alone; sdqn_redo.hip asserts they agree)
constexpr int64_t REDO_OFF2 = 256 * 32, REDO_OFF3 = REDO_OFF2 + 512 * 64, REDO_OFF4 = REDO_OFF3 + 576 * 64, REDO_OFF5 = REDO_OFF4 + (int64_t)3136 * 512;
constexpr uint64_t REDO_G = 0x9E3779B97F4A7C15ull;

REDO_HD uint64_t redo_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
REDO_HD uint64_t redo_key(uint64_t seed, uint64_t event) { return redo_mix(redo_mix(seed + REDO_G) + REDO_G * (event + 1)); }
REDO_HD uint64_t redo_word(uint64_t key, uint64_t i) { return redo_mix(key + REDO_G * (i + 1)); }
// k = float(sqrt(3 / fan_in)) of layer L = 1..4 (the doubles, rounded to float once by the compiler)
REDO_HD float redo_bound(int L) {
  return L == 1 ? (float)0.10825317547305482 : L == 2 ? (float)0.07654655446197431 : L == 3 ? (float)0.07216878364870322 : (float)0.030929478706587094;
}
REDO_HD float redo_draw(uint64_t key, uint64_t i, int L) {
  const float u = (float)(uint32_t)(redo_word(key, i) >> 40);      // < 2^24: exact
  const float t = u * 1.1920928955078125e-07f - 1.0f;              // u 2^-23 - 1 in [-1, 1): both operations exact
  return t * redo_bound(L);
}
// what entry i of the flat weight buffer is: its layer L = 1..5, the unit it feeds (index into the 672 scores, -1: none) and the unit it
// multiplies (likewise)
struct RedoEntry { int L, in, src; };
REDO_HD RedoEntry redo_entry(int64_t i) {
  RedoEntry e;
  if (i < REDO_OFF2) { e.L = 1; e.in = redo_soff(0) + (int)(i & 31); e.src = -1; }
  else if (i < REDO_OFF3) { const int64_t r = i - REDO_OFF2; e.L = 2; e.in = redo_soff(1) + (int)(r & 63); e.src = redo_soff(0) + (int)((r >> 6) & 31); }
  else if (i < REDO_OFF4) { const int64_t r = i - REDO_OFF3; e.L = 3; e.in = redo_soff(2) + (int)(r & 63); e.src = redo_soff(1) + (int)((r >> 6) & 63); }
  else if (i < REDO_OFF5) { const int64_t r = i - REDO_OFF4; e.L = 4; e.in = redo_soff(3) + (int)(r & 511); e.src = redo_soff(2) + (int)((r >> 9) & 63); }
  else { const int64_t r = i - REDO_OFF5; e.L = 5; e.in = -1; e.src = redo_soff(3) + (int)(r & 511); }
  return e;
}
REDO_HD bool redo_dormant(float score, double tau) { return (double)score <= tau; }
// 0 kept | 1 redrawn | 2 zeroed
REDO_HD int redo_action(const float* scores, double tau, const RedoEntry& e) {
  if (e.src >= 0 && redo_dormant(scores[e.src], tau)) return 2;
  if (e.in >= 0 && redo_dormant(scores[e.in], tau)) return 1;
  return 0;
}
// one event on host arrays: theta / state / state2 (may be NULL) [n] in place, n = REDO_OFF5 + 512 A; counts (may be NULL): dormant units per layer
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
    for (int j = redo_soff(l); j < redo_soff(l + 1); ++j) counts[l] += redo_dormant(scores[j], tau) ? 1 : 0;
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
REDO_HD constexpr int redo_chunk(int l) { return l == 3 ? 32 : 512; }
REDO_HD constexpr int redo_pix(int l) { return l == 0 ? 400 : l == 1 ? 81 : l == 2 ? 49 : 1; }      // rows per sample
REDO_HD constexpr int redo_n(int l) { return l == 0 ? 32 : l == 3 ? 512 : 64; }                    // units
REDO_HD int redo_blocks(int l, int B) { return (int)(((int64_t)B * redo_pix(l) + redo_chunk(l) - 1) / redo_chunk(l)); }
REDO_HD int64_t redo_partial_doubles(int B) { int64_t n = 0; for (int l = 0; l < REDO_LAYERS; ++l) n += (int64_t)redo_blocks(l, B) * redo_n(l); return n; }

#if defined(__HIPCC__)
hipError_t launch_redo_scores(const RedoScoreArgs& a, int stage, hipStream_t s);      // stage 0: partial sums, 1: scores
hipError_t launch_redo_apply(const RedoApplyArgs& a, hipStream_t s);
#endif

}  // namespace sdqn

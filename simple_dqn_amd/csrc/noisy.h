// noisy.h — the noise of --noisy_nets: ONE definition, compiled for the host (sdqn_noisy_noise / sdqn_noisy_words, the
// oracle's source of truth) and for the device (sdqn_noisy.hip), as env_catch.h is.  Counter-based: every value is a function of
// (seed, step, net slot, layer, side, index) alone, so no workgroup waits for another and any of them can regenerate what it needs.
//
//   stream  k0 = mix(seed + G), k1 = mix(k0 + G (step + 1)), key = mix(k1 + G (4 slot + 2 layer + side + 1))     (integers, mod 2^64)
//   word    w_i = mix(key + G (i + 1))                                            mix: splitmix64's finaliser, G its increment
//   normal  hi = w >> 32, lo = w & (2^32 - 1); u1 = float(hi + 1) / 2^32, u2 = float(lo) / 2^32; z = sqrt(-2 ln u1) cos(2 pi u2), in float
//   factor  e = f(z) = sgn(z) sqrt|z|                                             (Fortunato et al. 2018, factorised Gaussian noise)
//
// slot: 0 online net, 1 target net.  layer: 0 fc4 (3136 inputs, 512 outputs), 1 fc5 (512 inputs, A outputs).  side: 0 inputs, 1 outputs.
// The input index of fc4 is the reference layout's (feature map f, pixel): i = f 49 + pix; the flat buffers hold fc4 pixel-major
// (problems.h: neon_to_internal), noisy_fc4_input maps a row of the internal layout back.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NOISY_HD __host__ __device__ inline
#else
#define NOISY_HD inline
#endif

namespace sdqn {

constexpr int NOISY_IN4 = 3136, NOISY_OUT4 = 512, NOISY_IN5 = 512, NOISY_OUT5_PAD = 32;       // (fc5's outputs: A <= 18, padded)
// one net's four factor vectors in the device buffer ("noisy_eps"): [e_in4 | e_out4 | e_in5 | e_out5 (padded with zeros)]
constexpr int NOISY_EPS_IN4 = 0, NOISY_EPS_OUT4 = NOISY_IN4, NOISY_EPS_IN5 = NOISY_EPS_OUT4 + NOISY_OUT4, NOISY_EPS_OUT5 = NOISY_EPS_IN5 + NOISY_IN5;
constexpr int NOISY_EPS_NET = NOISY_EPS_OUT5 + NOISY_OUT5_PAD;      // 4192 floats per net
constexpr uint64_t NOISY_G = 0x9E3779B97F4A7C15ull;

NOISY_HD uint64_t noisy_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
NOISY_HD uint64_t noisy_key(uint64_t seed, uint64_t step, int slot, int layer, int side) {
  uint64_t k = noisy_mix(seed + NOISY_G);
  k = noisy_mix(k + NOISY_G * (step + 1));
  return noisy_mix(k + NOISY_G * (uint64_t)(4 * slot + 2 * layer + side + 1));
}
NOISY_HD uint64_t noisy_word(uint64_t key, uint64_t i) { return noisy_mix(key + NOISY_G * (i + 1)); }
// the unit normal of one word (Box-Muller, cosine branch), every operation in float and rounded once
NOISY_HD float noisy_normal(uint64_t w) {
  const float u1 = (float)((w >> 32) + 1) * 2.3283064365386963e-10f;       // (hi + 1) / 2^32 in (0, 1]
  const float u2 = (float)(w & 0xFFFFFFFFull) * 2.3283064365386963e-10f;   // lo / 2^32 in [0, 1]
  const float r = sqrtf(-2.0f * logf(u1));
  return r * cosf(6.28318530717958647692f * u2);
}
NOISY_HD float noisy_f(float z) { return copysignf(sqrtf(fabsf(z)), z); }
NOISY_HD float noisy_factor(uint64_t key, uint64_t i) { return noisy_f(noisy_normal(noisy_word(key, i))); }
// row k = pix 64 + f of fc4 in the internal layout -> its input index f 49 + pix in the reference layout (problems.h: neon_to_internal, layer 3)
NOISY_HD int noisy_fc4_input(int k) { return (k & 63) * 49 + (k >> 6); }

}  // namespace sdqn

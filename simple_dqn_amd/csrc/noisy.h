// noisy.h — the noise of --noisy_nets: ONE definition, compiled for the host (sdqn_noisy_noise / sdqn_noisy_words, the
// oracle's source of truth) and for the device (sdqn_noisy.hip), as env_catch.h is.  Counter-based: every value is a function of
// (seed, step, net slot, layer, side, index) alone, so no workgroup waits for another and any of them can regenerate what it needs.
//
//   stream  k0 = mix(seed + G), k1 = mix(k0 + G (step + 1)), key = mix(k1 + G (4 slot + 2 layer + side + 1))     (integers, mod 2^64)
//   word    w_i = mix(key + G (i + 1)) = stream_keyed(key, i)                     mix, G: stream.h (k0 = stream_keyed(seed, 0), and so on)
//   normal  hi = w >> 32, lo = w & (2^32 - 1); u1 = float(hi + 1) / 2^32, u2 = float(lo) / 2^32; z = sqrt(-2 ln u1) cos(2 pi u2), in float
//   factor  e = f(z) = sgn(z) sqrt|z|                                             (Fortunato et al. 2018, factorised Gaussian noise)
//
// slot: 0 online net, 1 target net.  layer: 0 fc4 (3136 inputs, 512 outputs), 1 fc5 (512 inputs, A outputs).  side: 0 inputs, 1 outputs.
// The input index of fc4 is the reference layout's (feature map f, pixel): i = f 49 + pix; the flat buffers hold fc4 pixel-major
// (problems.h: neon_to_internal), noisy_fc4_input maps a row of the internal layout back.
#pragma once
#include <stdint.h>
#include <math.h>
#include "net_layout.h"
#include "stream.h"

namespace sdqn {

constexpr int NOISY_OUT5_PAD = 32;       // fc5's outputs: A <= 18, padded (fc4: NIN4 inputs, NFC outputs; fc5: NFC inputs; net_layout.h)
// one net's four factor vectors in the device buffer ("noisy_eps"): [e_in4 | e_out4 | e_in5 | e_out5 (padded with zeros)]
constexpr int NOISY_EPS_IN4 = 0, NOISY_EPS_OUT4 = NIN4, NOISY_EPS_IN5 = NOISY_EPS_OUT4 + NFC, NOISY_EPS_OUT5 = NOISY_EPS_IN5 + NFC;
constexpr int NOISY_EPS_NET = NOISY_EPS_OUT5 + NOISY_OUT5_PAD;      // 4192 floats per net

SDQN_HD uint64_t noisy_key(uint64_t seed, uint64_t step, int slot, int layer, int side) {
  return stream_mix(stream_keyed(stream_keyed(seed, 0), step) + STREAM_G * (uint64_t)(4 * slot + 2 * layer + side + 1));
}
// the unit normal of one word (Box-Muller, cosine branch), every operation in float and rounded once
SDQN_HD float noisy_normal(uint64_t w) {
  const float u1 = (float)((w >> 32) + 1) * 2.3283064365386963e-10f;       // (hi + 1) / 2^32 in (0, 1]
  const float u2 = (float)(w & 0xFFFFFFFFull) * 2.3283064365386963e-10f;   // lo / 2^32 in [0, 1]
  const float r = sqrtf(-2.0f * logf(u1));
  return r * cosf(6.28318530717958647692f * u2);
}
SDQN_HD float noisy_f(float z) { return copysignf(sqrtf(fabsf(z)), z); }
SDQN_HD float noisy_factor(uint64_t key, uint64_t i) { return noisy_f(noisy_normal(stream_keyed(key, i))); }
// row k = pix 64 + f of fc4 in the internal layout -> its input index f 49 + pix in the reference layout (problems.h: neon_to_internal, layer 3)
SDQN_HD int noisy_fc4_input(int k) { return (k & 63) * 49 + (k >> 6); }

}  // namespace sdqn

// net_layout.h — the geometry of the five layers and of the flat weight buffer, stated once in plain C++ for the host and
// the device: the GEMM problems (problems.h), the noise of fc4 / fc5 (noisy.h) and every pass over the flat buffer (redo.h, reset.h,
// regularize.h) read it here.
//
//   layers   L = 1..5: conv1, conv2, conv3, fc4, fc5.  One net's weights are one flat buffer [W1i | W2i | W3i | W4i | W5i] in the internal
//            layouts (problems.h), layer L at [layer_first(L), layer_first(L + 1)); fc5 ends at n = OFF5 + NFC A, the caller's business
//   units    the ReLU layers 1..4 have 32, 64, 64, 512 units; one value per unit (a score, a statistic) lies at relu_off(L - 1) + j of a
//            buffer of RELU_UNITS
//   init     the initialiser of deepqnetwork.py draws every layer from U(-k, k), k = sqrt(3 / fan_in), fan_in 256, 512, 576, 3136, 512
#pragma once
#include <stdint.h>
#include "hd.h"
#include "stream.h"

namespace sdqn {

constexpr int ST1 = 4, P1 = 20, Q1 = 20, K1 = 32;   // conv 8x8 s4   deepqnetwork.py:83
constexpr int ST2 = 2, P2 = 9, Q2 = 9, K2 = 64;     // conv 4x4 s2   :85
constexpr int P3 = 7, Q3 = 7, K3 = 64;              // conv 3x3 s1   :87
constexpr int PIX1 = P1 * Q1, PIX2 = P2 * Q2, PIX3 = P3 * Q3;
constexpr int CRS1 = 256, CRS2 = 512, CRS3 = 576;
constexpr int NFC = 512, NIN4 = PIX3 * K3;          // Affine 512    :89
constexpr int NW1 = CRS1 * K1, NW2 = CRS2 * K2, NW3 = CRS3 * K3, NW4 = NIN4 * NFC;
constexpr int OFF1 = 0, OFF2 = OFF1 + NW1, OFF3 = OFF2 + NW2, OFF4 = OFF3 + NW3, OFF5 = OFF4 + NW4;
constexpr int NET_LAYERS = 5, RELU_LAYERS = 4, RELU_UNITS = K1 + K2 + K3 + NFC;      // 672

// the layer L = 1..5 that holds flat index i, and the first flat index of layer L (6: one past fc5 is the caller's n)
SDQN_HD int layer_of(int64_t i) { return i < OFF2 ? 1 : i < OFF3 ? 2 : i < OFF4 ? 3 : i < OFF5 ? 4 : 5; }
SDQN_HD constexpr int64_t layer_first(int L) { return L <= 1 ? OFF1 : L == 2 ? OFF2 : L == 3 ? OFF3 : L == 4 ? OFF4 : OFF5; }
// ReLU layer l = 0..3: its units, and where its units' values start (l = 4: RELU_UNITS, one past the last)
SDQN_HD constexpr int relu_units(int l) { return l == 0 ? K1 : l == 3 ? NFC : K2; }
SDQN_HD constexpr int relu_off(int l) { return l == 0 ? 0 : l == 1 ? K1 : l == 2 ? K1 + K2 : l == 3 ? K1 + K2 + K3 : RELU_UNITS; }
static_assert(K2 == K3, "relu_units");

// k = float(sqrt(3 / fan_in)) of layer L (the doubles, rounded to float once by the compiler): the ReLU layers L = 1..4, and all of L = 1..5,
// where fc5's fan_in is fc4's width, 512: conv2's value
SDQN_HD float relu_init_bound(int L) {
  return L == 1 ? (float)0.10825317547305482 : L == 2 ? (float)0.07654655446197431 : L == 3 ? (float)0.07216878364870322 : (float)0.030929478706587094;
}
SDQN_HD float init_bound(int L) { return L == 5 ? relu_init_bound(2) : relu_init_bound(L); }
// the initialiser's draw of layer L from one 64-bit word: (u 2^-23 - 1) k, the product by k rounded once
SDQN_HD float init_draw(uint64_t w, int L) { return stream_unit24(w) * init_bound(L); }

}  // namespace sdqn

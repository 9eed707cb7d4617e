// stream.h — the project's counter-based generator, ONE definition in plain integer C++ for the host and the device: every
// seeded feature (the games, --bootstrap_heads, --noisy_nets, --random_shift, --redo_interval, --reset_interval) derives its words from
// these functions and keeps only its own keying scheme in its own header.  splitmix64 (Steele, Lea and Flood 2014): the state is a counter,
// the output its finalised value; all sums and products modulo 2^64.  No floating point but stream_unit24, no library state.
#pragma once
#include <stdint.h>
#include "hd.h"

namespace sdqn {

constexpr uint64_t STREAM_G = 0x9E3779B97F4A7C15ull;        // the increment: a counter's step
constexpr uint64_t STREAM_MUL = 0xD1B54A32D192ED03ull;      // the stream multiplier: what separates the generators of one seed

SDQN_HD uint64_t stream_mix(uint64_t z) {                   // the finaliser: a bijection of the 64-bit words
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// sequential use: the state moves on by G, the output is its finalised value
SDQN_HD uint64_t stream_next(uint64_t& s) { s += STREAM_G; return stream_mix(s); }
// random access: word i under `key`, the output of a generator started at `key` after i + 1 steps; also how a key is derived from a key
SDQN_HD uint64_t stream_keyed(uint64_t key, uint64_t i) { return stream_mix(key + STREAM_G * (i + 1)); }
// the starting state of generator `stream` (0, 1, 2: what each means is its user's business) of copy `e` under `seed`
SDQN_HD uint64_t stream_seed(uint64_t seed, uint64_t e, uint64_t stream) { return stream_mix(seed + STREAM_MUL * (2 * e + stream + 1)); }
// the top 24 bits of a word as a float in [-1, 1): u 2^-23 - 1, the conversion, the product and the difference all exact
SDQN_HD float stream_unit24(uint64_t w) {
  const float u = (float)(uint32_t)(w >> 40);               // < 2^24: exact
  return u * 1.1920928955078125e-07f - 1.0f;
}

}  // namespace sdqn

// sdqn_regularize.hip — decoupled weight decay and L2-init regularisation, --weight_decay / --l2_init (the rule: regularize.h):
//     v = theta[e];  [v = v * kf;]  [v = v + cf * (anchor[e] - v);]  theta[e] = v          for the n = OFF5 + 512 A weights of the online net,
// plus every derived copy of the online weights that sdqn_net_set_weights(which = 0) would have rebuilt: conv1's three bf16 planes (float32
// nets) or the two half copies wh / wht (float16 nets).  ONE launch, built like target_blend_kernel (sdqn_target.hip), two kinds of workgroups:
//   bid <  tiles : a 64 (k) x 32 (n) tile of a layer whose weights have a TRANSPOSED derived copy.  The rule runs on 16-byte loads / stores along
//                  n, the derived values cross an LDS tile (rows of 66 uint16: off the bank stride) and leave with 16-byte stores along k.
//   bid >= tiles : the rest of the weights, element-wise float4.
// L2 (template): without --l2_init the kernel has no anchor load at all.  A template and not a uniform branch: the branch would keep the
// anchor's address arithmetic and its 16-byte destination registers in every thread of the decay-only kernel; the instantiations are four
// small kernels, and the choice is made once per launch on the host.
// FUSE (template): the fused form with --target_tau.  The same pass then blends theta- toward the NEW theta with blend1's three operations
// (sdqn_target.hip) and writes the target net's derived copies too: bit for bit what this launch followed by target_blend_kernel leaves, with
// theta read once.  No atomics, no scratch, no argument that changes from step to step.
//
// weight_norms: per layer sum theta^2 and sum (theta - anchor)^2 in fp64, two stages in a fixed order (REG_NORM_BLOCKS partials per layer and
// quantity, folded by one wave), as sdqn_clip.hip reduces the gradient: the same weights give the same bits.  A read-out, never part of a step.
#include "kernels.h"
#include "regularize.h"

namespace sdqn {
namespace {

constexpr int TK = 64, TN = 32;                        // tile: k rows x n columns of a layer's [K][N] weights
constexpr int TROW = TK + 2;                           // LDS row of the transposed tile (uint16; 132 B: 4-byte aligned, off the bank stride)
static_assert(CRS1 % TK == 0 && CRS2 % TK == 0 && CRS3 % TK == 0 && NIN4 % TK == 0, "every layer is whole tiles along k");
static_assert(K1 % TN == 0 && K2 % TN == 0 && K3 % TN == 0 && NFC % TN == 0, "every layer is whole tiles along n");
static_assert(OFF2 % 4 == 0 && OFF5 % 4 == 0 && NFC % 4 == 0, "the element-wise part is whole float4s");
constexpr int TILES1 = (CRS1 / TK) * (K1 / TN), TILES2 = (CRS2 / TK) * (K2 / TN), TILES3 = (CRS3 / TK) * (K3 / TN), TILES4 = (NIN4 / TK) * (NFC / TN);

__device__ __forceinline__ float blend1(float w, float wt, float tau) {      // sdqn_target.hip's, restated: three roundings
  const float d = __fsub_rn(w, wt);
  const float m = __fmul_rn(tau, d);
  return __fadd_rn(wt, m);
}
template <bool L2> __device__ __forceinline__ float rule1(const RegRule& r, float v, float an) {
  if (r.wd_on) v = reg_decay(r, v);                    // uniform: a scalar branch around one multiplication
  if (L2) v = reg_pull(r, v, an);
  return v;
}
template <bool L2> __device__ __forceinline__ float4 rule4(const RegularizeArgs& a, int64_t e) {
  const float4 w = *reinterpret_cast<const float4*>(a.theta + e);
  float4 an = make_float4(0.f, 0.f, 0.f, 0.f);
  if (L2) an = *reinterpret_cast<const float4*>(a.anchor + e);
  return make_float4(rule1<L2>(a.rule, w.x, an.x), rule1<L2>(a.rule, w.y, an.y), rule1<L2>(a.rule, w.z, an.z), rule1<L2>(a.rule, w.w, an.w));
}
__device__ __forceinline__ float4 blend4(const float4& w, const float4& wt, float tau) {
  return make_float4(blend1(w.x, wt.x, tau), blend1(w.y, wt.y, tau), blend1(w.z, wt.z, tau), blend1(w.w, wt.w, tau));
}
__device__ __forceinline__ uint16_t half_bits(float f) { const half_t h = (half_t)f; return __builtin_bit_cast(uint16_t, h); }

using Tile = uint16_t[3][TN][TROW];                     // [plane][n][k]: plane 0 = half / bf16 hi, 1 = bf16 mid, 2 = bf16 lo

// the derived values of four consecutive n at row kk: into the LDS tile (and wh in the master layout on a float16 net)
__device__ __forceinline__ void derive4(Tile& tile, const float4& v, int nn, int kk, half_t* wh, int64_t e) {
  const float vv[4] = {v.x, v.y, v.z, v.w};
  if (wh) {
    uint16_t hb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { hb[i] = half_bits(vv[i]); tile[0][nn + i][kk] = hb[i]; }
    uint2 p; p.x = (uint32_t)hb[0] | (uint32_t)hb[1] << 16; p.y = (uint32_t)hb[2] | (uint32_t)hb[3] << 16;
    *reinterpret_cast<uint2*>(wh + e) = p;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint16_t hi, mid, lo; split_bf16x3(vv[i], hi, mid, lo);
      tile[0][nn + i][kk] = hi; tile[1][nn + i][kk] = mid; tile[2][nn + i][kk] = lo;
    }
  }
}
// the transposed side of one net: thread -> row n0 + nr, 8 consecutive k (16 bytes) per plane
__device__ __forceinline__ void store_transposed(const Tile& tile, int t, half_t* wht, unsigned short* w1p, int off, int K, int k0, int n0) {
  const int nr = t >> 3, kc = (t & 7) * 8;
  const int planes = wht ? 1 : 3;
  for (int p = 0; p < planes; ++p) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&tile[p][nr][kc]);
    uint4 o; o.x = src[0]; o.y = src[1]; o.z = src[2]; o.w = src[3];
    const int64_t d = (int64_t)(n0 + nr) * K + k0 + kc;                  // < N * K
    uint16_t* dst = wht ? reinterpret_cast<uint16_t*>(wht) + off + d : w1p + (int64_t)p * W1P_PLANE + d;
    *reinterpret_cast<uint4*>(dst) = o;
  }
}

template <bool L2, bool FUSE>
__global__ void __launch_bounds__(256) regularize_kernel(const RegularizeArgs a) {
  __shared__ __attribute__((aligned(16))) Tile tiles[FUSE ? 2 : 1];      // the online net's tile [, the target net's]
  const int t = threadIdx.x, bid = blockIdx.x;
  if (bid < a.tiles) {
    int ti = bid, off = OFF1, K = CRS1, N = K1;
    if (ti >= TILES1) { ti -= TILES1; off = OFF2; K = CRS2; N = K2;
      if (ti >= TILES2) { ti -= TILES2; off = OFF3; K = CRS3; N = K3;
        if (ti >= TILES3) { ti -= TILES3; off = OFF4; K = NIN4; N = NFC; } } }
    const int ntn = N / TN, k0 = (ti / ntn) * TK, n0 = (ti % ntn) * TN;
    const int nn = (t & 7) * 4;
#pragma unroll
    for (int pass = 0; pass < TK / 32; ++pass) {
      const int kk = pass * 32 + (t >> 3);
      const int64_t e = off + (int64_t)(k0 + kk) * N + n0 + nn;          // < off + K * N <= OFF5 <= n: inside the layer
      const float4 v = rule4<L2>(a, e);
      *reinterpret_cast<float4*>(a.theta + e) = v;
      derive4(tiles[0], v, nn, kk, reinterpret_cast<half_t*>(a.wh), e);
      if (FUSE) {
        const float4 vt = blend4(v, *reinterpret_cast<const float4*>(a.theta_t + e), a.tau);
        *reinterpret_cast<float4*>(a.theta_t + e) = vt;
        derive4(tiles[FUSE ? 1 : 0], vt, nn, kk, reinterpret_cast<half_t*>(a.wh_t), e);
      }
    }
    __syncthreads();
    store_transposed(tiles[0], t, reinterpret_cast<half_t*>(a.wht), a.w1p, off, K, k0, n0);
    if (FUSE) store_transposed(tiles[FUSE ? 1 : 0], t, reinterpret_cast<half_t*>(a.wht_t), a.w1p_t, off, K, k0, n0);
    return;
  }
  const int fb = bid - a.tiles, nfb = (int)gridDim.x - a.tiles;
  const int64_t n4 = (a.n - a.flat_first) >> 2;                          // (n - flat_first is a multiple of 4: launch_regularize)
  for (int64_t i = (int64_t)fb * 256 + t; i < n4; i += (int64_t)nfb * 256) {
    const int64_t e = a.flat_first + 4 * i;                              // e + 3 < n
    const float4 v = rule4<L2>(a, e);
    *reinterpret_cast<float4*>(a.theta + e) = v;
    if (FUSE) *reinterpret_cast<float4*>(a.theta_t + e) = blend4(v, *reinterpret_cast<const float4*>(a.theta_t + e), a.tau);
  }
}

// ---- weight_norms -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double s) {                    // every lane receives the sum (a + b == b + a)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  return s;
}
__device__ __forceinline__ int64_t layer_first(int L, int64_t n) { return L == 0 ? OFF1 : L == 1 ? OFF2 : L == 2 ? OFF3 : L == 3 ? OFF4 : L == 4 ? OFF5 : n; }

// workgroup (L, b) of REG_LAYERS x REG_NORM_BLOCKS: float4s b * 256 + t + k * (REG_NORM_BLOCKS * 256) of layer L
template <bool ANCHOR>
__global__ void __launch_bounds__(256) weight_norms_partial_kernel(const WeightNormArgs a) {
  __shared__ double wsum[2][4];
  const int t = threadIdx.x, L = blockIdx.x / REG_NORM_BLOCKS, b = blockIdx.x % REG_NORM_BLOCKS;
  const int64_t first = layer_first(L, a.n), n4 = (layer_first(L + 1, a.n) - first) >> 2;      // every layer is whole float4s
  double sn = 0.0, sd = 0.0;
  for (int64_t i = (int64_t)b * 256 + t; i < n4; i += (int64_t)REG_NORM_BLOCKS * 256) {
    const int64_t e = first + 4 * i;                                     // e + 3 < first of the next layer <= n
    const float4 w = *reinterpret_cast<const float4*>(a.theta + e);
    const float wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) { const double d = (double)wv[k]; sn += __dmul_rn(d, d); }
    if (ANCHOR) {
      const float4 an = *reinterpret_cast<const float4*>(a.anchor + e);
      const float av[4] = {an.x, an.y, an.z, an.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) { const double d = __dsub_rn((double)wv[k], (double)av[k]); sd += __dmul_rn(d, d); }
    }
  }
  sn = wave_sum(sn); sd = wave_sum(sd);
  if ((t & 63) == 0) { wsum[0][t >> 6] = sn; wsum[1][t >> 6] = sd; }
  __syncthreads();
  if (t < 2) {                                                           // fixed order
    const double s = ((wsum[t][0] + wsum[t][1]) + wsum[t][2]) + wsum[t][3];
    if (t == 0 || ANCHOR) a.buf[(t * REG_LAYERS + L) * REG_NORM_BLOCKS + b] = s;
  }
}
// one wave: result q = lane-wise partial of row q, then the butterfly
__global__ void __launch_bounds__(64) weight_norms_fold_kernel(const WeightNormArgs a, const int rows) {
  static_assert(REG_NORM_BLOCKS == 64, "one partial per lane");
  const int lane = threadIdx.x;
  for (int q = 0; q < rows; ++q) {
    const double s = wave_sum(a.buf[q * REG_NORM_BLOCKS + lane]);
    if (lane == 0) a.buf[2 * REG_LAYERS * REG_NORM_BLOCKS + q] = s;
  }
}

}  // namespace

hipError_t launch_regularize(RegularizeArgs a, hipStream_t s) {
  // which layers go through tiles follows from the derived copies this net keeps; the flat part starts where they end
  a.tiles = a.wh ? TILES1 + TILES2 + TILES3 + TILES4 : (a.w1p ? TILES1 : 0);
  a.flat_first = a.wh ? OFF5 : (a.w1p ? OFF2 : 0);
  const bool fuse = a.theta_t != nullptr;
  if (!a.theta || a.n < OFF5 || ((a.n - OFF5) & 3) || (a.wh && !a.wht) || (a.rule.l2_on && !a.anchor)) return hipErrorInvalidValue;
  if (fuse && (a.theta_t == a.theta || (a.wh && !(a.wh_t && a.wht_t)) || (a.w1p && !a.wh && !a.w1p_t))) return hipErrorInvalidValue;
  const int64_t n4 = (a.n - a.flat_first) >> 2;
  int64_t fblocks = (n4 + 511) / 512;                   // two float4 per thread, at most 1024 workgroups
  fblocks = fblocks < 1 ? 1 : (fblocks > 1024 ? 1024 : fblocks);
  const dim3 grid((unsigned)(a.tiles + fblocks)), block(256);
  if (a.rule.l2_on) {
    if (fuse) SDQN_LAUNCH((regularize_kernel<true, true>), grid, block, 0, s, a); else SDQN_LAUNCH((regularize_kernel<true, false>), grid, block, 0, s, a);
  } else {
    if (fuse) SDQN_LAUNCH((regularize_kernel<false, true>), grid, block, 0, s, a); else SDQN_LAUNCH((regularize_kernel<false, false>), grid, block, 0, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_weight_norms(const WeightNormArgs& a, hipStream_t s) {
  if (!a.theta || !a.buf || a.n < OFF5 || ((a.n - OFF5) & 3)) return hipErrorInvalidValue;
  const dim3 grid(REG_LAYERS * REG_NORM_BLOCKS), block(256);
  if (a.anchor) SDQN_LAUNCH(weight_norms_partial_kernel<true>, grid, block, 0, s, a); else SDQN_LAUNCH(weight_norms_partial_kernel<false>, grid, block, 0, s, a);
  hipError_t e = hipGetLastError(); if (e != hipSuccess) return e;
  SDQN_LAUNCH(weight_norms_fold_kernel, dim3(1), dim3(64), 0, s, a, a.anchor ? 2 * REG_LAYERS : REG_LAYERS);
  return hipGetLastError();
}

}  // namespace sdqn

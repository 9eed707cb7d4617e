// sdqn_target.hip — soft (Polyak) target-network update, --target_tau:
//     theta-[e] <- theta-[e] + tau * (theta[e] - theta-[e])          for all NP values of the flat buffer,
// three separately rounded fp32 operations (numpy float32 reproduces them bit for bit), plus every derived copy of the target's
// weights that sdqn_net_set_weights(which = 1) would have rebuilt: conv1's three bf16 planes (float32 nets) or the two half copies
// wh / wht (float16 nets).  ONE launch, two kinds of workgroups:
//   bid <  tiles : a 64 (k) x 32 (n) tile of a layer whose weights have a TRANSPOSED derived copy (conv1 for the bf16 planes; conv1..fc4
//                  for wht).  The tile is blended with 16-byte loads / stores along n, its derived values cross an LDS tile and leave
//                  with 16-byte stores along k: both global sides are coalesced (the element-wise form of update_body.h scatters
//                  2-byte stores K elements apart — fc4's 1.6 M of them would be the whole cost of this kernel).
//   bid >= tiles : the rest of the flat buffer (fc5, the BatchNorm block; conv2..fc4 too on a float32 net), element-wise float4.
// The kernel reads no argument that changes from step to step, uses no atomics and no scratch and writes to no buffer of the online
// net, so it commutes with nothing but its own stream order (sdqn_api_net.hip: target_blend).
#include "kernels.h"

namespace sdqn {
namespace {

constexpr int TK = 64, TN = 32;                        // tile: k rows x n columns of a layer's [K][N] weights
constexpr int TROW = TK + 2;                           // LDS row of the transposed tile (uint16; 132 B: 4-byte aligned, off the bank stride)
static_assert(CRS1 % TK == 0 && CRS2 % TK == 0 && CRS3 % TK == 0 && NIN4 % TK == 0, "every layer is whole tiles along k");
static_assert(K1 % TN == 0 && K2 % TN == 0 && K3 % TN == 0 && NFC % TN == 0, "every layer is whole tiles along n");
constexpr int TILES1 = (CRS1 / TK) * (K1 / TN), TILES2 = (CRS2 / TK) * (K2 / TN), TILES3 = (CRS3 / TK) * (K3 / TN), TILES4 = (NIN4 / TK) * (NFC / TN);

__device__ __forceinline__ float blend1(float w, float wt, float tau) {
  const float d = __fsub_rn(w, wt);                    // never contracted: d, m and the sum are each rounded once
  const float m = __fmul_rn(tau, d);
  return __fadd_rn(wt, m);
}
__device__ __forceinline__ float4 blend4(const float4& w, const float4& wt, float tau) {
  return make_float4(blend1(w.x, wt.x, tau), blend1(w.y, wt.y, tau), blend1(w.z, wt.z, tau), blend1(w.w, wt.w, tau));
}
__device__ __forceinline__ uint16_t half_bits(float f) { const half_t h = (half_t)f; return __builtin_bit_cast(uint16_t, h); }

__global__ void __launch_bounds__(256) target_blend_kernel(const TargetBlendArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t tile[3][TN][TROW];   // [plane][n][k]: plane 0 = half / bf16 hi, 1 = bf16 mid, 2 = bf16 lo
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
      const int64_t e = off + (int64_t)(k0 + kk) * N + n0 + nn;          // < off + K * N: inside the layer
      const float4 w = *reinterpret_cast<const float4*>(a.theta + e);
      const float4 v = blend4(w, *reinterpret_cast<const float4*>(a.theta_t + e), a.tau);
      *reinterpret_cast<float4*>(a.theta_t + e) = v;
      const float vv[4] = {v.x, v.y, v.z, v.w};
      if (a.wh) {                                       // float16 net: wh in the master layout, wht through the tile
        uint16_t hb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { hb[i] = half_bits(vv[i]); tile[0][nn + i][kk] = hb[i]; }
        uint2 p; p.x = (uint32_t)hb[0] | (uint32_t)hb[1] << 16; p.y = (uint32_t)hb[2] | (uint32_t)hb[3] << 16;
        *reinterpret_cast<uint2*>(a.wh + e) = p;
      } else {                                          // float32 net: conv1's three bf16 planes (problems.h: split_bf16x3)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          uint16_t hi, mid, lo; split_bf16x3(vv[i], hi, mid, lo);
          tile[0][nn + i][kk] = hi; tile[1][nn + i][kk] = mid; tile[2][nn + i][kk] = lo;
        }
      }
    }
    __syncthreads();
    // transposed side: thread -> row n0 + nr, 8 consecutive k (16 bytes)
    const int nr = t >> 3, kc = (t & 7) * 8;
    const int planes = a.wh ? 1 : 3;
    for (int p = 0; p < planes; ++p) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(&tile[p][nr][kc]);
      uint4 o; o.x = src[0]; o.y = src[1]; o.z = src[2]; o.w = src[3];
      const int64_t d = (int64_t)(n0 + nr) * K + k0 + kc;                // < N * K
      uint16_t* dst = a.wh ? reinterpret_cast<uint16_t*>(a.wht) + off + d : a.w1p + (int64_t)p * W1P_PLANE + d;
      *reinterpret_cast<uint4*>(dst) = o;
    }
    return;
  }
  const int fb = bid - a.tiles, nfb = (int)gridDim.x - a.tiles;
  const int64_t n = a.NP - a.flat_first, n4 = n >> 2;
  for (int64_t i = (int64_t)fb * 256 + t; i < n4; i += (int64_t)nfb * 256) {
    const int64_t e = a.flat_first + 4 * i;
    const float4 w = *reinterpret_cast<const float4*>(a.theta + e);
    *reinterpret_cast<float4*>(a.theta_t + e) = blend4(w, *reinterpret_cast<const float4*>(a.theta_t + e), a.tau);
  }
  if (fb == 0 && t < (int)(n & 3)) {                    // tail: the last NP % 4 values, one thread each
    const int64_t e = a.NP - (n & 3) + t;
    a.theta_t[e] = blend1(a.theta[e], a.theta_t[e], a.tau);
  }
}

}  // namespace

hipError_t launch_target_blend(TargetBlendArgs a, hipStream_t s) {
  // which layers go through tiles follows from the derived copies this net keeps; the flat part starts where they end
  a.tiles = a.wh ? TILES1 + TILES2 + TILES3 + TILES4 : (a.w1p ? TILES1 : 0);
  a.flat_first = a.wh ? OFF5 : (a.w1p ? OFF2 : 0);
  if (a.NP < a.flat_first || (a.wh && !a.wht)) return hipErrorInvalidValue;
  const int64_t n4 = (a.NP - a.flat_first) >> 2;
  int64_t fblocks = (n4 + 511) / 512;                   // two float4 per thread, at most 1024 workgroups
  fblocks = fblocks < 1 ? 1 : (fblocks > 1024 ? 1024 : fblocks);
  SDQN_LAUNCH(target_blend_kernel, dim3((unsigned)(a.tiles + fblocks)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace sdqn

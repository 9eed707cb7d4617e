// sdqn_vis.hip — guided-backpropagation filter visualisation (the reference's --visualization_file: src/main.py:119-127 ->
// visualization.py -> Neon's DeconvCallback), fp32 throughout, on the online net's theta (the float16 mode keeps fp32 master weights
// there, so both datatypes are visualised from the same numbers).
//
// Two launches:
//   * vis_search_kernel — persistent grid, one 512-thread workgroup per CU.  A workgroup walks the states n = blockIdx.x, +gridDim.x, ...;
//     per state it stages the four frames (replay ring slots (idx - 3 + j) mod count, getState's index math, or an uploaded state array)
//     into LDS and runs conv1 -> conv2 -> conv3 with the activations in LDS; weights come from L2.  Every output is ONE thread's dot
//     product in one fixed (c, r, s) order — FMA on the vector ALU, not MFMA: on gfx950 an f32-input MFMA runs at the vector FMA rate, and
//     the vector form needs no operand shuffles, keeps every output's summation order independent of the position, state and workgroup
//     it lands in (the tie rule below is only exact because of that) and takes its input operand as an LDS broadcast.  Each thread keeps
//     the best (value, key) of its map in a register; at the end one LDS atomicMax per thread and ONE 64-bit global atomicMax per
//     (layer, map) per workgroup publishes it.  The 64-bit word is [order-preserving u32 of the pre-activation value | ~key] with
//     key = ((n / bsz) * P + p) * bsz + n % bsz, the reference's batch-loop tie order: the maximum word is the largest value, and
//     among equal values the smallest key — whatever order the workgroups finish in.
//   * vis_project_kernel — one workgroup per record.  It recomputes the winning state's conv1 / conv2 with the same code (so the
//     masks are bit-identical to the search's forward pass), keeps [a1 > 0] and [a2 > 0] as bitmasks in LDS and runs the ReLU-gated
//     transposed convolutions as gathers: every input element sums the output positions that cover it in a fixed order (no atomics:
//     deterministic).  The 4 x 84 x 84 result goes straight to global memory.
#include "api_internal.h"

namespace sdqn {
namespace vis {

constexpr int NT = 512;                          // 8 waves
constexpr int NREC = K1 + K2 + K3;               // 160: every map of the three conv layers
// LDS (bytes): state | one channel as float | a1 [400][32] | a2 [81][64] | [a1 > 0] [400] words | [a2 > 0] [81][2] words | reduction [160]
constexpr int L_S = 0, L_XF = L_S + STATE, L_A1 = L_XF + FRAME * 4, L_A2 = L_A1 + PIX1 * K1 * 4;
constexpr int L_M1 = L_A2 + PIX2 * K2 * 4, L_M2 = L_M1 + PIX1 * 4, L_RED = L_M2 + PIX2 * 8, L_END = L_RED + NREC * 8;
static_assert(L_XF % 16 == 0 && L_A1 % 16 == 0 && L_A2 % 16 == 0 && L_RED % 8 == 0 && L_END <= 160 * 1024, "LDS plan");
static_assert(FRAME % 16 == 0 && PIX3 * K3 * 4 <= FRAME * 4, "frame staging / E3 in the channel buffer");

struct VisArgs {
  const uint8_t* ring;        // replay ring [count][84*84] (nullptr: states)
  int64_t count;
  const int64_t* idx;         // [n] ring indexes
  const uint8_t* states;      // [n][4][84*84]
  int64_t n;
  int bsz;                    // the net's batch size (tie rule)
  int F[3], off[3];           // maps searched per layer, their first record
  const float* theta;         // online parameters (internal layout, problems.h)
  unsigned long long* res;    // [records] packed (value, ~key)
  float* vis;                 // [records][4][84*84]
};

__device__ __forceinline__ unsigned long long pack(float v, unsigned key) {
  if (v == 0.f) v = 0.f;                                           // -0 and +0 are one value
  const unsigned u = __float_as_uint(v);
  const unsigned o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // order-preserving float -> u32
  return ((unsigned long long)o << 32) | (unsigned long long)(~key);
}
__device__ __forceinline__ float unpack_value(unsigned long long w) {
  const unsigned o = (unsigned)(w >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__device__ __forceinline__ const uint8_t* frame_ptr(const VisArgs& a, int64_t n, int j) {
  if (a.ring) {
    int64_t slot = (a.idx[n] - (C0 - 1) + j) % a.count;           // replay_memory.py getState: (index - hist + 1 + j) mod count
    if (slot < 0) slot += a.count;
    return a.ring + slot * FRAME;
  }
  return a.states + n * STATE + j * FRAME;
}
__device__ __forceinline__ void stage_state(const VisArgs& a, int64_t n, uint8_t* S) {
  constexpr int Q = FRAME / 16;
  for (int i = threadIdx.x; i < C0 * Q; i += NT) {
    const int j = i / Q, q = i - j * Q;
    reinterpret_cast<uint4*>(S + j * FRAME)[q] = reinterpret_cast<const uint4*>(frame_ptr(a, n, j))[q];
  }
}
__device__ __forceinline__ float fma4(const float4 x, const float* w, float acc) {
  acc = __builtin_fmaf(x.x, w[0], acc); acc = __builtin_fmaf(x.y, w[1], acc);
  acc = __builtin_fmaf(x.z, w[2], acc); return __builtin_fmaf(x.w, w[3], acc);
}

// conv1 (8x8 s4, k = c*64 + r*8 + s): thread = map f (lanes 0..31) x position group g (16); positions g, g + 16, ... (25 each).
// The bytes are convolved as integers 0..255 and the sum divided by 255 (deepqnetwork.py:100 scales the input first: same value to
// fp32 round-off).  Writes a1 = max(z1, 0) [p][32]; TRACK: best[f] over the positions.  Starts with a barrier (S must be staged).
template <bool TRACK>
__device__ void conv1(const float* __restrict__ W, const uint8_t* S, float* XF, float* A1, unsigned kb, unsigned nr, unsigned bsz,
                      unsigned long long& best) {
  const int t = threadIdx.x, f = t & 31, g = t >> 5;
  float acc[25];
#pragma unroll
  for (int j = 0; j < 25; ++j) acc[j] = 0.f;
#pragma unroll 1
  for (int c = 0; c < C0; ++c) {
    __syncthreads();
    for (int i = t; i < FRAME; i += NT) XF[i] = (float)S[c * FRAME + i];
    __syncthreads();
#pragma unroll 1
    for (int r = 0; r < 8; ++r) {
      float w[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) w[s] = W[(c * 64 + r * 8 + s) * K1 + f];
#pragma unroll
      for (int j = 0; j < 25; ++j) {
        const int p = g + 16 * j, oy = p / Q1, ox = p - oy * Q1;
        const float* x = XF + (ST1 * oy + r) * W0 + ST1 * ox;
        acc[j] = fma4(*reinterpret_cast<const float4*>(x), w, acc[j]);
        acc[j] = fma4(*reinterpret_cast<const float4*>(x + 4), w + 4, acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 25; ++j) {
    const int p = g + 16 * j;
    const float z = acc[j] / 255.f;
    A1[p * K1 + f] = fmaxf(z, 0.f);
    if (TRACK) { const unsigned long long w = pack(z, (kb + p) * bsz + nr); best = w > best ? w : best; }
  }
}

// conv2 / conv3 over an NHWC activation in LDS, k = (r, s, c) like W2i / W3i: thread = map f (64 lanes) x group g (the 8 waves);
// positions g, g + 8, ... (<= J).  K is walked in chunks of 4 channels: 4 weights per thread (the next chunk's loaded while this one is
// used) against one 16-byte LDS broadcast per position.  STORE: a = max(z, 0) [p][64]; TRACK: best[f] over the positions.
template <int CIN, int R, int S, int ST, int IW, int OW, int PIX, bool STORE, bool TRACK>
__device__ void conv_nhwc(const float* __restrict__ W, const float* in, float* out, unsigned kb, unsigned nr, unsigned bsz,
                          unsigned long long& best) {
  constexpr int NQ = R * S * CIN / 4, J = (PIX + 7) / 8;
  const int t = threadIdx.x, f = t & 63, g = t >> 6;
  float acc[J], wc[4];
#pragma unroll
  for (int j = 0; j < J; ++j) acc[j] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) wc[i] = W[i * 64 + f];
#pragma unroll 2
  for (int q = 0; q < NQ; ++q) {
    const int nx = q + 1 < NQ ? q + 1 : q, rs = q / (CIN / 4), c0 = (q - rs * (CIN / 4)) * 4, r = rs / S, s = rs - r * S;
    float wn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) wn[i] = W[(nx * 4 + i) * 64 + f];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int p = min(g + 8 * j, PIX - 1), oy = p / OW, ox = p - oy * OW;
      acc[j] = fma4(*reinterpret_cast<const float4*>(in + ((ST * oy + r) * IW + ST * ox + s) * CIN + c0), wc, acc[j]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) wc[i] = wn[i];
  }
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int p = g + 8 * j;
    if (p < PIX) {
      if (STORE) out[p * 64 + f] = fmaxf(acc[j], 0.f);
      if (TRACK) { const unsigned long long w = pack(acc[j], (kb + p) * bsz + nr); best = w > best ? w : best; }
    }
  }
}
template <bool TRACK>
__device__ __forceinline__ void conv2(const float* W, const float* A1, float* A2, unsigned kb, unsigned nr, unsigned bsz, unsigned long long& best) {
  conv_nhwc<K1, 4, 4, ST2, Q1, Q2, PIX2, true, TRACK>(W, A1, A2, kb, nr, bsz, best);
}
__device__ __forceinline__ void conv3_track(const float* W, const float* A2, unsigned kb, unsigned nr, unsigned bsz, unsigned long long& best) {
  conv_nhwc<K2, 3, 3, 1, Q2, Q3, PIX3, false, true>(W, A2, nullptr, kb, nr, bsz, best);
}

__global__ __launch_bounds__(NT) void vis_search_kernel(VisArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[L_END];
  uint8_t* S = lds + L_S; float* XF = reinterpret_cast<float*>(lds + L_XF);
  float* A1 = reinterpret_cast<float*>(lds + L_A1); float* A2 = reinterpret_cast<float*>(lds + L_A2);
  unsigned long long* red = reinterpret_cast<unsigned long long*>(lds + L_RED);
  const float* th = a.theta;
  const unsigned bsz = (unsigned)a.bsz;
  unsigned long long b1 = 0, b2 = 0, b3 = 0;
  for (int64_t n = blockIdx.x; n < a.n; n += gridDim.x) {
    const unsigned nb = (unsigned)(n / bsz), nr = (unsigned)(n % bsz);
    __syncthreads();                                   // the previous state's readers are done with S and A2
    stage_state(a, n, S);
    conv1<true>(th + OFF1, S, XF, A1, nb * PIX1, nr, bsz, b1);
    __syncthreads();
    conv2<true>(th + OFF2, A1, A2, nb * PIX2, nr, bsz, b2);
    __syncthreads();
    conv3_track(th + OFF3, A2, nb * PIX3, nr, bsz, b3);
  }
  const int t = threadIdx.x;
  if (t < NREC) red[t] = 0;
  __syncthreads();
  atomicMax(red + (t & 31), b1);
  atomicMax(red + K1 + (t & 63), b2);
  atomicMax(red + K1 + K2 + (t & 63), b3);
  __syncthreads();
  if (t < NREC) {
    const int l = t < K1 ? 0 : (t < K1 + K2 ? 1 : 2), f = t - (l == 0 ? 0 : (l == 1 ? K1 : K1 + K2));
    if (f < a.F[l] && red[t]) atomicMax(a.res + a.off[l] + f, red[t]);
  }
}

__global__ __launch_bounds__(NT) void vis_project_kernel(VisArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[L_END];
  uint8_t* S = lds + L_S; float* XF = reinterpret_cast<float*>(lds + L_XF);
  float* A1 = reinterpret_cast<float*>(lds + L_A1); float* A2 = reinterpret_cast<float*>(lds + L_A2);
  unsigned* M1 = reinterpret_cast<unsigned*>(lds + L_M1); unsigned* M2 = reinterpret_cast<unsigned*>(lds + L_M2);
  const int t = threadIdx.x, b = blockIdx.x;
  const int L = b < a.off[1] ? 1 : (b < a.off[2] ? 2 : 3), f = b - a.off[L - 1];
  const int P = L == 1 ? PIX1 : (L == 2 ? PIX2 : PIX3);
  float* out = a.vis + (int64_t)b * STATE;
  const unsigned long long rec = a.res[b];
  const unsigned key = ~(unsigned)rec, bsz = (unsigned)a.bsz;
  const unsigned q = key / bsz, p = q % (unsigned)P;
  const int64_t n = (int64_t)(q / (unsigned)P) * bsz + key % bsz;
  if (rec == 0 || n >= a.n) {                            // (no record: cannot happen for n >= 1; never read outside the states)
    for (int i = t; i < STATE; i += NT) out[i] = 0.f;
    return;
  }
  const float e = fmaxf(unpack_value(rec), 0.f);         // E = max(E, 0) of the record's own layer
  const float* th = a.theta;
  unsigned long long unused = 0;
  stage_state(a, n, S);
  if (L >= 2) {                                          // conv1 forward -> [a1 > 0]: word p, bit f
    conv1<false>(th + OFF1, S, XF, A1, 0, 0, 1, unused);
    __syncthreads();
    if (L == 3) conv2<false>(th + OFF2, A1, A2, 0, 0, 1, unused);
    for (int pp = t; pp < PIX1; pp += NT) {
      unsigned m = 0;
      for (int c = 0; c < K1; ++c) m |= (A1[pp * K1 + c] > 0.f ? 1u : 0u) << c;
      M1[pp] = m;
    }
    __syncthreads();
    if (L == 3)                                          // [a2 > 0]: words 2p, 2p + 1
      for (int w = t; w < 2 * PIX2; w += NT) {
        unsigned m = 0;
        for (int c = 0; c < 32; ++c) m |= (A2[w * 32 + c] > 0.f ? 1u : 0u) << c;
        M2[w] = m;
      }
  }
  __syncthreads();
  float* E1 = A1;                                        // [400][32]: the a1 region, free once M1 is built
  float* E2 = A2;                                        // [81][64]
  if (L == 3) {                                          // E3 = one-hot [49][64] in the channel buffer; G3 gathered, masked by [a2 > 0]
    float* E3 = XF;
    for (int i = t; i < PIX3 * K3; i += NT) E3[i] = 0.f;
    __syncthreads();
    if (t == 0) E3[p * K3 + f] = e;
    __syncthreads();
    const float* W = th + OFF3;
    for (int o = t; o < PIX2 * K2; o += NT) {
      const int c = o & 63, pix = o >> 6, y = pix / Q2, x = pix - y * Q2;
      float acc = 0.f;
      for (int r = 0; r < 3; ++r) {
        const int oy = y - r;
        if (oy < 0 || oy >= P3) continue;
        for (int s = 0; s < 3; ++s) {
          const int ox = x - s;
          if (ox < 0 || ox >= Q3) continue;
          const float* w = W + ((r * 3 + s) * K2 + c) * K3;      // W3i[(r, s, c)][f]
          const float* ee = E3 + (oy * Q3 + ox) * K3;
          for (int k = 0; k < K3; k += 4) acc = fma4(*reinterpret_cast<const float4*>(ee + k), w + k, acc);
        }
      }
      E2[o] = (M2[o >> 5] >> (o & 31)) & 1u ? acc : 0.f;
    }
    __syncthreads();
  } else if (L == 2) {
    for (int i = t; i < PIX2 * K2; i += NT) E2[i] = 0.f;
    __syncthreads();
    if (t == 0) E2[p * K2 + f] = e;
    __syncthreads();
  }
  if (L >= 2) {                                          // G2 over a1's grid [20][20][32], masked by [a1 > 0]
    const float* W = th + OFF2;
    for (int o = t; o < PIX1 * K1; o += NT) {
      const int c = o & 31, pix = o >> 5, y = pix / Q1, x = pix - y * Q1;
      float acc = 0.f;
      for (int r = (y & 1); r < 4; r += 2) {
        const int oy = (y - r) >> 1;
        if (y < r || oy >= P2) continue;
        for (int s = (x & 1); s < 4; s += 2) {
          const int ox = (x - s) >> 1;
          if (x < s || ox >= Q2) continue;
          const float* w = W + ((r * 4 + s) * K1 + c) * K2;      // W2i[(r, s, c)][f]
          const float* ee = E2 + (oy * Q2 + ox) * K2;
          for (int k = 0; k < K2; k += 4) {
            const float4 v = *reinterpret_cast<const float4*>(ee + k);
            acc = fma4(make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)), w + k, acc);
          }
        }
      }
      E1[o] = (M1[pix] >> c) & 1u ? acc : 0.f;
    }
    __syncthreads();
  } else {
    for (int i = t; i < PIX1 * K1; i += NT) E1[i] = 0.f;
    __syncthreads();
    if (t == 0) E1[p * K1 + f] = e;
    __syncthreads();
  }
  const float* W = th + OFF1;                            // G1 over the input [4][84][84], masked by [byte > 0]
  for (int o = t; o < STATE; o += NT) {
    const int c = o / FRAME, rem = o - c * FRAME, y = rem / W0, x = rem - y * W0;
    float acc = 0.f;
    for (int r = (y & 3); r < 8; r += 4) {
      const int oy = (y - r) >> 2;
      if (y < r || oy >= P1) continue;
      for (int s = (x & 3); s < 8; s += 4) {
        const int ox = (x - s) >> 2;
        if (x < s || ox >= Q1) continue;
        const float* w = W + (c * 64 + r * 8 + s) * K1;          // W1i[(c, r, s)][f]
        const float* ee = E1 + (oy * Q1 + ox) * K1;
        for (int k = 0; k < K1; k += 4) {
          const float4 v = *reinterpret_cast<const float4*>(ee + k);
          acc = fma4(make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)), w + k, acc);
        }
      }
    }
    out[o] = S[o] ? acc : 0.f;
  }
}

}  // namespace vis
}  // namespace sdqn

using sdqn::vis::VisArgs;

namespace {
struct DevBufs {                                         // temporaries of one call (hipFree waits for the device)
  std::vector<void*> p;
  ~DevBufs() { for (void* q : p) hipFree(q); }
  hipError_t alloc(void** out, size_t bytes) { hipError_t e = hipMalloc(out, bytes); if (e == hipSuccess) p.push_back(*out); return e; }
};
struct Events {
  hipEvent_t e[3] = {nullptr, nullptr, nullptr};
  ~Events() { for (hipEvent_t x : e) if (x) hipEventDestroy(x); }
};
}  // namespace

extern "C" int sdqn_net_visualize(sdqn_net_t h, sdqn_replay_t r, const int64_t* idx, const uint8_t* states, int64_t n, int max_fm,
                                  int64_t* rec_state, int32_t* rec_pos, float* rec_value, float* vis_out, float* ms_out) {
  ARGCHK(h && rec_state && rec_pos && rec_value, "NULL argument");
  ARGCHK((r && idx && !states) || (!r && !idx && states), "give either a replay memory with indexes or a states array, not both");
  ARGCHK(!h->gen, "filter visualisation is implemented for the 84x84x4 float32 / float16 networks (not float64 or other geometries)");
  ARGCHK(!h->bn, "filter visualisation is not implemented for batch_norm networks");
  ARGCHK(max_fm >= 1, "max_fm must be >= 1 (got %d)", max_fm);
  ARGCHK(n >= 1, "no states to visualise (n = %lld)", (long long)n);
  const int64_t bsz = h->B, nbatch = (n + bsz - 1) / bsz;
  ARGCHK(nbatch <= (int64_t)0xFFFFFFFF / (PIX1 * bsz), "%lld states overflow the 32-bit tie key at batch_size %lld", (long long)n, (long long)bsz);
  if (r) {
    ARGCHK(r->tuned_geom, "the replay memory is not 84x84 with history_length 4");
    ARGCHK(!r->lanes, "filter visualisation reads getState's index math, which a laned replay memory (sdqn_replay_set_lanes) does not have");
    ARGCHK(r->count > 0, "the replay memory is empty");
    for (int64_t i = 0; i < n; ++i)
      ARGCHK(idx[i] >= 0 && idx[i] < r->count, "index %lld out of range (count %lld)", (long long)idx[i], (long long)r->count);
  }
  STREAMCHK();
  { int rc = join_comm(h); if (rc) return rc; }
  VisArgs a;
  a.F[0] = max_fm < K1 ? max_fm : K1; a.F[1] = max_fm < K2 ? max_fm : K2; a.F[2] = max_fm < K3 ? max_fm : K3;
  a.off[0] = 0; a.off[1] = a.F[0]; a.off[2] = a.F[0] + a.F[1];
  const int R = a.F[0] + a.F[1] + a.F[2];
  a.n = n; a.bsz = (int)bsz; a.theta = h->theta; a.ring = nullptr; a.count = 0; a.idx = nullptr; a.states = nullptr; a.vis = nullptr;
  DevBufs d;
  if (r) {
    HIPCHK(d.alloc((void**)&a.idx, (size_t)n * 8));
    HIPCHK(hipMemcpyAsync((void*)a.idx, idx, (size_t)n * 8, hipMemcpyHostToDevice, g_stream));
    a.ring = r->d_ring; a.count = r->count;
  } else {
    HIPCHK(d.alloc((void**)&a.states, (size_t)n * STATE));
    HIPCHK(hipMemcpyAsync((void*)a.states, states, (size_t)n * STATE, hipMemcpyHostToDevice, g_stream));
  }
  HIPCHK(d.alloc((void**)&a.res, (size_t)R * 8));
  HIPCHK(hipMemsetAsync(a.res, 0, (size_t)R * 8, g_stream));
  if (vis_out) HIPCHK(d.alloc((void**)&a.vis, (size_t)R * STATE * 4));
  int cus = 0;
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g_dev));
  const int grid = (int)(n < cus ? n : cus);
  Events ev;
  if (ms_out) for (int i = 0; i < 3; ++i) HIPCHK(hipEventCreate(&ev.e[i]));
  if (ms_out) HIPCHK(hipEventRecord(ev.e[0], g_stream));
  hipLaunchKernelGGL(sdqn::vis::vis_search_kernel, dim3(grid), dim3(sdqn::vis::NT), 0, g_stream, a);
  HIPCHK(hipGetLastError());
  if (ms_out) HIPCHK(hipEventRecord(ev.e[1], g_stream));
  if (vis_out) {
    hipLaunchKernelGGL(sdqn::vis::vis_project_kernel, dim3(R), dim3(sdqn::vis::NT), 0, g_stream, a);
    HIPCHK(hipGetLastError());
  }
  if (ms_out) HIPCHK(hipEventRecord(ev.e[2], g_stream));
  std::vector<unsigned long long> res((size_t)R);
  HIPCHK(hipMemcpyAsync(res.data(), a.res, (size_t)R * 8, hipMemcpyDeviceToHost, g_stream));
  if (vis_out) HIPCHK(hipMemcpyAsync(vis_out, a.vis, (size_t)R * STATE * 4, hipMemcpyDeviceToHost, g_stream));
  HIPCHK(hipStreamSynchronize(g_stream));
  if (ms_out) { HIPCHK(hipEventElapsedTime(ms_out, ev.e[0], ev.e[1])); HIPCHK(hipEventElapsedTime(ms_out + 1, ev.e[1], ev.e[2])); }
  for (int i = 0; i < R; ++i) {
    const int L = i < a.off[1] ? 1 : (i < a.off[2] ? 2 : 3);
    const unsigned P = L == 1 ? PIX1 : (L == 2 ? PIX2 : PIX3);
    const unsigned key = ~(unsigned)res[i], q = key / (unsigned)bsz;
    const unsigned o = (unsigned)(res[i] >> 32);
    const unsigned u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float v; memcpy(&v, &u, 4);
    rec_state[i] = (int64_t)(q / P) * bsz + key % (unsigned)bsz;
    rec_pos[i] = (int32_t)(q % P);
    rec_value[i] = v;
    if (res[i] == 0) { set_error("no record for map %d (internal error)", i); return SDQN_ERR_STATE; }
  }
  return SDQN_OK;
}

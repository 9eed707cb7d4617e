// gemm_engine.h — the one tile engine behind every GEMM-shaped stage (problems.h).
//
// Regime: at B=32 every stage is a few hundred MFLOP — far too small to fill 256 CUs with classic
// block-tiled GEMMs, and a per-K-tile __syncthreads pipeline is a serial chain of memory latencies
// (measured: ~10 us per stage for ~1 us of MFMA work).  So the engine is organised for latency:
//
//   * one workgroup = ONE 32x32 fp32 output tile (a single v_mfma_f32_32x32x2_f32 accumulator:
//     exact fp32, bitwise an fmaf chain — needed for the 1e-4 Q-value parity);
//   * its NW wave64s (1..16) split the reduction dimension: wave w owns the 32-deep K-chunks
//     w, w+NW, ... and runs them autonomously — NO workgroup barrier in the main loop, every wave
//     has its next chunk's global loads in flight while it issues the current chunk's 16 MFMAs;
//   * operands whose memory-contiguous dimension is m/n (weights [k][n], deltas [m][f], the wgrad
//     im2col rows) are loaded straight into the MFMA operand layout (lane l <- [kslot][x0 + (l&31)],
//     two coalesced 128-B rows per instruction, no LDS);
//   * operands contiguous along k (im2col patches, activations, dgrad weights) need NO staging either: the MFMA's
//     k-slot <-> logical-k assignment is free as long as A and B agree, and with kslot(t, h) = 8*(t>>2) + 4h + (t&3)
//     a lane's 16 operand values are four 16 B loads of its own row (4 B for the u8 ring);
//   * the NW partial tiles are summed through LDS in a fixed order (deterministic), then P::store.
//   * a staged problem whose N leaves most CUs without a 32-wide tile (fc4_dgrad: 98 of them) runs the same scheme on 32 x 16 tiles and
//     v_mfma_f32_16x16x4_f32 instead (P::N16_WAVES, gemm_tile_n16; maps in n16_map.h).
//   * a direct-operand problem whose 32-row tiles give some CUs two workgroups and the others one (conv2_fwd below B = 128: 324 tiles) runs
//     on 48 x 32 tiles of the same instruction, one workgroup per CU (P::M48_WAVES, gemm_tile_m48; maps in m48_map.h).
//
// MFMA operand maps (guide §3): lane l holds A[i = l&31][k = l>>5], B[k = l>>5][j = l&31];
// D register r of lane l is D[i = (r&3) + 8*(r>>2) + 4*(l>>5)][j = l&31].
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include "problems.h"
#include "n16_map.h"
#include "m48_map.h"
#include "launch.h"

namespace sdqn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// element type of an x-contiguous operand (float unless the problem says otherwise: the fp16-mode wgrads read half)
template <class P, class = void> struct a_elem { typedef float type; };
template <class P> struct a_elem<P, decltype((void)sizeof(typename P::AT))> { typedef typename P::AT type; };
template <class P, class = void> struct b_elem { typedef float type; };
template <class P> struct b_elem<P, decltype((void)sizeof(typename P::BT))> { typedef typename P::BT type; };
// k-contiguous operands: direct (4 x 16 B loads of the lane's own row: 32 cache lines per instruction, no LDS) or
// staged (lanes (k4, x): 8 rows x 128 B per instruction, transposed through a wave-private LDS panel).  Direct wins
// when the rows of a tile are close together and the launch is latency-bound (conv fwd/dgrad at B = 32); staged wins
// for the fc4 GEMMs (rows 2-12 KB apart) and in the throughput regime (B >= 128).  Measured: profiles/README.md.
template <class P, class = void> struct stages_lds { static constexpr bool value = false; };
template <class P> struct stages_lds<P, decltype((void)P::STAGE_LDS)> { static constexpr bool value = P::STAGE_LDS; };
template <class P> struct Staged : P { static constexpr bool STAGE_LDS = true; };      // same problem, staged operands
// A_GROUP4: the irregular (im2col-row) A operand is affine inside every aligned group of 4 consecutive k
// (conv1: 20 x 20 output positions, x fastest, stride 4 bytes in the u8 frame; 20 and 400 are multiples of 4), so a
// lane needs 4 gathered offsets per chunk instead of 16 and fetches its 4 bytes with ONE unaligned 16-byte load
template <class P, class = void> struct a_group4 { static constexpr bool value = false; };
template <class P> struct a_group4<P, decltype((void)P::A_GROUP4)> { static constexpr bool value = P::A_GROUP4; };
template <class P, class = void> struct uses_f16_wgrad { static constexpr bool value = false; };
template <class P> struct uses_f16_wgrad<P, decltype((void)P::F16_WGRAD)> { static constexpr bool value = P::F16_WGRAD; };
// PRELOAD: P::preload(a) runs first thing in the kernel and touches every argument field the problem will read, so that hipcc issues
// ALL their scalar loads in one batch behind one wait.  Left alone it fetches each field of the 464-byte by-value StepArgs where it is
// first used: four or five DEPENDENT round trips to a kernel-argument segment that is cold at every launch (round 3, sdqn_kernels_r3.hip)
template <class P, class = void> struct has_preload { static constexpr bool value = false; };
template <class P> struct has_preload<P, decltype((void)P::PRELOAD)> { static constexpr bool value = P::PRELOAD; };
template <class P, class = void> struct has_preload_multi { static constexpr bool value = false; };
template <class P> struct has_preload_multi<P, decltype((void)P::PRELOAD_MULTI)> { static constexpr bool value = P::PRELOAD_MULTI; };
// LEAD: the launch's hot arguments a second time, as LEADING scalar / pointer kernel parameters in front of the by-value StepArgs.  gfx950's
// command processor can place the first 14 argument dwords in user SGPRs at wave launch (-mllvm -amdgpu-kernarg-preload-count, csrc/Makefile;
// a by-value struct is never preloaded), so a wave forms the addresses of its first vector loads without the scalar round trip to the cold
// kernel-argument segment that P::preload batches.  The block is 16 dwords (the struct keeps its 64-byte phase): five operand pointers the
// problem names (SDQN_LEAD_FIELDS), B, two launch scalars and a control word; the last two dwords are padding.  With the control word's
// LEAD_ON bit clear (option arg_preload = 0) the kernel takes the same values from the struct behind P::preload, as before: same bits.
// What each kernel packs (host) and unpacks (device) — one row per pack / unpack pair:
//   kernel                   p[0..4]                          B slot            s0                        s1            ctl
//   gemm_kernel, gemm36      SDQN_LEAD_FIELDS of the problem  B                 gx | gy << 16 | gz << 24   field X       lead_ctl
//   gemm_multi_kernel        SDQN_LEAD_FIELDS of problem 1    B                 n[0] | n[1] << 16          field X       lead_ctl
//   head_kernel              theta[0], theta[1], slab4, a4, d4  B               A                         -             lead_ctl
//   conv1_bf16_kernel        src, a1, w1p[0], w1p[1], idx     B                 tiles_per_net             wgs_per_net   xcd | pad_ << 1 | from_ring << 2 | tpw << 4 | LEAD_ON | post_off << 16
//   conv1_wgrad_bf16_kernel  src, d1, slab1, idx, -           B                 tps1                      Kt            xcd | pad_ << 1 | from_ring << 2 | LEAD_ON | grid z << 16
//   update_kernel            theta, state, slab[0..2]         ns[0] | ns[1] << 16  ns[2]                  A | mode << 8 | only_fc4 << 12   LEAD_ON
// lead_ctl = xcd_map [0, 8) | LEAD_ON | nz [12, 16) | S4 [16, 24).  Every host pack clears LEAD_ON when a value does not fit its bits or B >= 128.
struct Lead { const void* p[5]; int B, s0, s1, ctl, r0, r1; };
static_assert(sizeof(Lead) == 64, "leading block: 16 dwords");
constexpr int LEAD_ON = 256;                 // ctl: xcd_map [0, 8) | LEAD_ON | nz [12, 16) | S4 [16, 24)
#define SDQN_LEAD_PARAMS const void* lp0, const void* lp1, const void* lp2, const void* lp3, const void* lp4, int lB, int ls0, int ls1, int lctl, int lr0, int lr1
#define SDQN_LEAD_ARGS(L) (L).p[0], (L).p[1], (L).p[2], (L).p[3], (L).p[4], (L).B, (L).s0, (L).s1, (L).ctl, (L).r0, (L).r1
template <class T> struct lead_noref { typedef T type; };
template <class T> struct lead_noref<T&> { typedef T type; };
#define SDQN_LEAD_SET_(f, v) a.f = (typename lead_noref<decltype(a.f)>::type)(v)
// the five pointer fields of StepArgs a problem (or a whole multi-problem launch) wants in SGPRs at wave launch; X = one more int field
#define SDQN_LEAD_FIELDS(f0, f1, f2, f3, f4, X) \
  static void lead_pack(const StepArgs& a, Lead& l) { l.p[0] = a.f0; l.p[1] = a.f1; l.p[2] = a.f2; l.p[3] = a.f3; l.p[4] = a.f4; l.s1 = a.X; } \
  __device__ static void lead_apply(StepArgs& a, const void* q0, const void* q1, const void* q2, const void* q3, const void* q4, int x) { \
    SDQN_LEAD_SET_(f0, q0); SDQN_LEAD_SET_(f1, q1); SDQN_LEAD_SET_(f2, q2); SDQN_LEAD_SET_(f3, q3); SDQN_LEAD_SET_(f4, q4); a.X = x; }
template <class P, class = void> struct has_lead { static constexpr bool value = false; };
template <class P> struct has_lead<P, decltype((void)P::LEAD)> { static constexpr bool value = P::LEAD; };
template <class P, class = void> struct has_lead_multi { static constexpr bool value = false; };
template <class P> struct has_lead_multi<P, decltype((void)P::LEAD_MULTI)> { static constexpr bool value = P::LEAD_MULTI; };
inline int lead_grid(const dim3& g) { return (int)(g.x | g.y << 16 | g.z << 24); }          // s0 of a single-problem launch: gx [0, 16) | gy [16, 24) | gz [24, 31)
inline bool lead_grid_fits(const dim3& g) { return g.x < 65536u && g.y < 256u && g.z < 128u; }
// (the block is for the latency regime, B < 128; a field that does not fit its bits clears LEAD_ON too: the kernel then reads the struct)
inline int lead_ctl(const StepArgs& a, bool on) {
  const bool fits = a.B < 128 && a.xcd_map >= 0 && a.xcd_map < 256 && a.nz >= 0 && a.nz < 16 && a.S4 >= 0 && a.S4 < 256;
  return (a.xcd_map & 255) | (on && fits ? LEAD_ON : 0) | ((a.nz & 15) << 12) | ((a.S4 & 255) << 16);
}
__device__ __forceinline__ void lead_scalars(StepArgs& a, int B, int ctl) { a.B = B; a.xcd_map = ctl & 255; a.nz = (ctl >> 12) & 15; a.S4 = (ctl >> 16) & 255; }
#define SDQN_LEAD_FWD lp0, lp1, lp2, lp3, lp4, lB, ls0, ls1, lctl, lr0, lr1
template <class P, class = void> struct uses_f16_mfma { static constexpr bool value = false; };
template <class P> struct uses_f16_mfma<P, decltype((void)P::F16_MFMA)> { static constexpr bool value = P::F16_MFMA; };
// N16_WAVES: the wave count at which a staged fp32 problem runs on the 32 x 16 tile body (gemm_tile_n16 below) instead of the 32 x 32 one;
// absent or 0: never.  The choice belongs to (problem, waves per tile): the same problem keeps 32 x 32 tiles in its other launch forms.
template <class P, class = void> struct n16_waves { static constexpr int value = 0; };
template <class P> struct n16_waves<P, decltype((void)P::N16_WAVES)> { static constexpr int value = P::N16_WAVES; };
template <class P, int NW> constexpr bool use_n16() {
  return NW > 1 && n16_waves<P>::value == NW && stages_lds<P>::value && !uses_f16_wgrad<P>::value && !uses_f16_mfma<P>::value;
}
// M48_WAVES: the wave count at which a direct-operand fp32 problem (A k-contiguous, B a plain [k][n] matrix) runs on the 48 x 32 tile body
// (gemm_tile_m48 below) instead of the 32 x 32 one; absent or 0: never.  Like N16_WAVES the choice belongs to (problem, waves per tile).
template <class P, class = void> struct m48_waves { static constexpr int value = 0; };
template <class P> struct m48_waves<P, decltype((void)P::M48_WAVES)> { static constexpr int value = P::M48_WAVES; };
template <class P, int NW> constexpr bool use_m48() {
  return NW > 1 && m48_waves<P>::value == NW && !stages_lds<P>::value && !uses_f16_wgrad<P>::value && !uses_f16_mfma<P>::value;
}
// problems whose epilogue gates the result with a stored activation may offer the two halves of store apart (P::GATED: gate_load, store_gated)
template <class P, class = void> struct gated_store { static constexpr bool value = false; };
template <class P> struct gated_store<P, decltype((void)P::GATED)> { static constexpr bool value = P::GATED; };

constexpr int PANEL = 32 * 33;      // one [32 k][32 x] fp32 panel, pitch 33

__device__ __forceinline__ void wave_lds_sync() {
  // wave-private LDS hand-off between lanes of ONE wave: LDS ops of a wave execute in order, so only
  // the compiler has to be kept from reordering the stores past the loads
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}


// value held by lane s (lanes 0-31) / lane s+4 (lanes 32-63): the k-slot of the upper half-wave is 4 further.
// v_readlane (VALU -> SGPR, no LDS round trip) x2 + v_cndmask; s is a compile-time constant after unrolling.
__device__ __forceinline__ int pick_half(int v, int s, bool hi) {
  const int lo = __builtin_amdgcn_readlane(v, s), up = __builtin_amdgcn_readlane(v, s + 4);
  return hi ? up : lo;
}
__device__ __forceinline__ int64_t pick_half(int64_t v, int s, bool hi) {
  const int i = s;
  const int l0 = __builtin_amdgcn_readlane((int)(v & 0xFFFFFFFF), i), l1 = __builtin_amdgcn_readlane((int)(v >> 32), i);
  const int u0 = __builtin_amdgcn_readlane((int)(v & 0xFFFFFFFF), i + 4), u1 = __builtin_amdgcn_readlane((int)(v >> 32), i + 4);
  const int64_t lo = ((int64_t)l1 << 32) | (uint32_t)l0, up = ((int64_t)u1 << 32) | (uint32_t)u0;
  return hi ? up : lo;
}

#ifdef SDQN_TIMING
// phase stamps (s_memtime) of wave 0 of every workgroup: dbg[(block*8 + phase)]; NOT in the product build
__device__ unsigned long long* g_sdqn_dbg = nullptr;
#define SDQN_STAMP(ph) do { if (g_sdqn_dbg && threadIdx.x == 0) g_sdqn_dbg[((size_t)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) * 8) + (ph)] = clock64(); } while (0)
// per-WAVE stamps of the latency engine's tile routine (round 5: which operand lands when, tools/landing_hist.py):
// wdbg[((block * 16 + wave) * 4 + phase)], phase 0 = before the first operand load, 1 = all loads issued, 2 = A landed, 3 = B landed;
// + the XCC the workgroup ran on in wdbg[blocks * 64 + block]
__device__ unsigned long long* g_sdqn_wdbg = nullptr;
__device__ unsigned g_sdqn_wdbg_blocks = 0;
// (the stamps are TAKEN into registers where they belong and WRITTEN at the end of the tile: a store, or the load of the buffer pointer,
//  next to the operand loads would sit in the same in-order vmcnt queue and turn every stamp into "everything before me has landed")
#define SDQN_WSTAMP_DECL unsigned long long wst_[4] = {0, 0, 0, 0}
#define SDQN_WSTAMP(ph) do { if (wst_[ph] == 0) wst_[ph] = clock64(); } while (0)
#define SDQN_WSTAMP_FLUSH do { unsigned long long* wd_ = g_sdqn_wdbg; if (wd_ && (threadIdx.x & 63) == 0) { \
  const size_t b_ = (size_t)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)); const unsigned nb_ = g_sdqn_wdbg_blocks; \
  if (b_ < nb_ && (threadIdx.x >> 6) < 16) { \
    for (int q_ = 0; q_ < 4; ++q_) wd_[(b_ * 16 + (threadIdx.x >> 6)) * 4 + q_] = wst_[q_]; \
    if (threadIdx.x == 0) { unsigned x_; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(x_)); wd_[(size_t)nb_ * 64 + b_] = x_; } } } } while (0)
#else
#define SDQN_STAMP(ph) do {} while (0)
#define SDQN_WSTAMP_DECL do {} while (0)
#define SDQN_WSTAMP(ph) do {} while (0)
#define SDQN_WSTAMP_FLUSH do {} while (0)
#endif

// LDS floats one workgroup of NW waves needs (only the fixed-order combine of the NW partial tiles uses LDS)
template <class P, int NW>
constexpr int tile_lds() {
  return NW * PANEL * (stages_lds<P>::value && (P::A_K || P::B_K) ? ((P::A_K ? 1 : 0) + (P::B_K ? 1 : 0)) : 1);
}

// k-slot assignment shared by BOTH operands of every problem: MFMA step t (0..15) of a 32-deep chunk, half-wave h,
// consumes logical k = kc + kslot(t, h).  Any bijection works as long as A and B agree; this one makes a k-contiguous
// operand exactly four 16-byte loads of the lane's own row (j = t >> 2 selects the load, e = t & 3 the component):
__device__ __forceinline__ constexpr int kslot(int t, int h) { return 8 * (t >> 2) + 4 * h + (t & 3); }

template <class T>
__device__ __forceinline__ T ld_byte_off(const T* base, uint32_t byte_off) {
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off);
}

// One 32x32 output tile (bx, by, bz) of problem P computed by the first NW waves of a workgroup of NT threads
// (waves >= NW idle through the epilogue barrier).  NW == 1 inside a wider workgroup is handled by the caller
// (one tile per wave, no barrier): see gemm_multi_kernel.
template <class P, int NW, int NT>
__device__ __forceinline__ void gemm_tile(const StepArgs& a, int bx, int by, int bz, float* smem) {
  constexpr bool STG = stages_lds<P>::value;
  constexpr bool STG_A = STG && P::A_K, STG_B = STG && P::B_K;
  constexpr int WAVE_LDS = PANEL * ((STG_A || STG_B) ? ((STG_A ? 1 : 0) + (STG_B ? 1 : 0)) : 1);
  typedef typename P::aoff_t aoff_t;

  SDQN_STAMP(0);
  SDQN_WSTAMP_DECL;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // provably wave-uniform -> SGPR index math
  const int m0 = bx * 32, n0 = by * 32;
  int z, ks, kbeg, kend;
  P::ksplit(a, bz, z, ks, kbeg, kend);
  if (NW * 64 < NT && wave >= NW) kend = kbeg;          // surplus waves of a wider workgroup: no chunks
  const int M = P::M(a), N = P::N(a);
  const int hb = lane >> 5;                             // half-wave: which k-slots this lane feeds
  const bool hi = lane >= 32;

  // ---- per-lane operand geometry: lane l always owns row m0 + (l & 31) of A and column n0 + (l & 31) of B ----------
  const int mrow = m0 + (lane & 31), ncol = n0 + (lane & 31);
  const aoff_t arow = P::a_row(a, z, mrow < M ? mrow : M - 1);
  const int bcol = P::b_col(a, z, ncol < N ? ncol : N - 1);
  typedef typename a_elem<P>::type AT; typedef typename b_elem<P>::type BT;
  const AT* abase = P::a_ptr(a, z);
  const BT* bbase = P::b_ptr(a, z);
  // plain row-major [k][x] operands: per-lane pointer fixed for the whole tile (row 0 / row 4 for the two half-waves)
  const AT* areg = nullptr; const BT* breg = nullptr;
  if constexpr (!P::A_K && P::A_REG) areg = abase + (uint32_t)arow + (hi ? 4 * P::A_LD : 0);
  if constexpr (!P::B_K && P::B_REG) breg = bbase + (uint32_t)bcol + (hi ? 4 * P::B_LD : 0);
  // the same per-lane position as a 32-bit BYTE offset from the (uniform) base pointer: `global_load v, v_off, s[base]`
  // instead of three VALU instructions of 64-bit pointer arithmetic per load (all operand buffers are < 4 GB)
  uint32_t aoffb = 0, boffb = 0;
  if constexpr (!P::A_K && P::A_REG) aoffb = (uint32_t)sizeof(AT) * ((uint32_t)arow + (hi ? 4u * P::A_LD : 0u));
  if constexpr (!P::B_K && P::B_REG) boffb = (uint32_t)sizeof(BT) * ((uint32_t)bcol + (hi ? 4u * P::B_LD : 0u));
  (void)abase; (void)bbase; (void)areg; (void)breg; (void)aoffb; (void)boffb;

  // staged operands: lane -> (k4 = l & 7, rows (l >> 3) + 8j) for the loads, wave-private panels [k][x] (pitch 33)
  float* pan_a = smem + (wave < NW ? wave : 0) * WAVE_LDS;
  float* pan_b = pan_a + (STG_A ? PANEL : 0);
  aoff_t srow[STG_A ? 4 : 1]; int scol[STG_B ? 4 : 1];
  if constexpr (STG_A) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int m = m0 + (lane >> 3) + 8 * j; srow[j] = P::a_row(a, z, m < M ? m : M - 1); }
  }
  if constexpr (STG_B) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int n = n0 + (lane >> 3) + 8 * j; scol[j] = P::b_col(a, z, n < N ? n : N - 1); }
  }
  (void)pan_a; (void)pan_b; (void)srow; (void)scol;

  typename P::Epi epi;
  if constexpr (NW == 1) P::epi_begin(a, m0, n0, lane, epi);

  // One chunk's 16 MFMA operand values of this lane, straight from global memory into registers (no LDS staging):
  //   k-contiguous operand : 4 x 16-byte loads (4 bytes for the u8 ring) of the lane's own row at k = kc + 8j + 4h
  //   x-contiguous, regular: 16 dword loads off the per-lane pointer at immediate row offsets kslot(t, 0) * LD
  //   x-contiguous, im2col : one index decomposition per lane per chunk (lane <-> k = kc + (l & 31)), distributed with
  //                          v_readlane; offsets of out-of-range k are clamped in bounds, loads are UNconditional and the
  //                          value is selected afterwards (a conditional load costs a branch + vmcnt(0) per element)
  auto load_a = [&](int kc, float* dst) {
    if constexpr (P::A_K) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f4 v = P::a_load4(a, z, arow + P::a_col(a, z, kc + 8 * j + 4 * hb));
        dst[4 * j] = v.x; dst[4 * j + 1] = v.y; dst[4 * j + 2] = v.z; dst[4 * j + 3] = v.w;
      }
    } else if constexpr (P::A_REG) {
      if (kc + 32 <= kend) {
        if constexpr (sizeof(AT) * P::A_LD >= 2048) {          // every row offset beyond the 12-bit immediate: 32-bit offsets
          const uint32_t kcb = (uint32_t)sizeof(AT) * (uint32_t)kc * (uint32_t)P::A_LD;          // wave-uniform
#pragma unroll
          for (int t = 0; t < 16; ++t) dst[t] = (float)ld_byte_off(abase, aoffb + kcb + (uint32_t)(sizeof(AT) * kslot(t, 0) * P::A_LD));
        } else {
          const AT* p = areg + (size_t)kc * P::A_LD;
#pragma unroll
          for (int t = 0; t < 16; ++t) dst[t] = (float)p[(size_t)kslot(t, 0) * P::A_LD];
        }
      } else {
#pragma unroll
        for (int t = 0; t < 16; ++t) { const int k = kc + kslot(t, hb); dst[t] = k < kend ? (float)areg[(size_t)(kc + kslot(t, 0)) * P::A_LD] : 0.0f; }
      }
    } else if constexpr (a_group4<P>::value) {
      const int kl = kc + (lane & 31);
      const aoff_t cv = P::a_col(a, z, kl < kend ? kl : kbeg);
#pragma unroll
      for (int j = 0; j < 4; ++j) {                                         // k = kc + 8j + 4h + e, e = 0..3
        const aoff_t c = pick_half(cv, 8 * j, hi);
        const bool ok = kc + 8 * j + 4 * hb < kend;                         // Kt is a multiple of 4: whole groups
        const f4 v = P::a_load_group4(a, z, arow + c);
        dst[4 * j] = ok ? v.x : 0.0f; dst[4 * j + 1] = ok ? v.y : 0.0f; dst[4 * j + 2] = ok ? v.z : 0.0f; dst[4 * j + 3] = ok ? v.w : 0.0f;
      }
    } else {
      const int kl = kc + (lane & 31);
      const aoff_t cv = P::a_col(a, z, kl < kend ? kl : kbeg);
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const aoff_t c = pick_half(cv, kslot(t, 0), hi);
        const bool ok = kc + kslot(t, hb) < kend;
        float v;
        if constexpr (P::A_U8) v = P::a_load(a, z, arow + c);
        else v = (float)abase[(uint32_t)(arow + c)];                      // uniform base + 32-bit lane offset
        dst[t] = ok ? v : 0.0f;
      }
    }
  };
  auto load_b = [&](int kc, float* dst) {
    if constexpr (P::B_K) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f4 v = P::b_load4(a, z, bcol + P::b_row(a, z, kc + 8 * j + 4 * hb));
        dst[4 * j] = v.x; dst[4 * j + 1] = v.y; dst[4 * j + 2] = v.z; dst[4 * j + 3] = v.w;
      }
    } else if constexpr (P::B_REG) {
      if (kc + 32 <= kend) {
        if constexpr (sizeof(BT) * P::B_LD >= 2048) {
          const uint32_t kcb = (uint32_t)sizeof(BT) * (uint32_t)kc * (uint32_t)P::B_LD;
#pragma unroll
          for (int t = 0; t < 16; ++t) dst[t] = (float)ld_byte_off(bbase, boffb + kcb + (uint32_t)(sizeof(BT) * kslot(t, 0) * P::B_LD));
        } else {
          const BT* p = breg + (size_t)kc * P::B_LD;
#pragma unroll
          for (int t = 0; t < 16; ++t) dst[t] = (float)p[(size_t)kslot(t, 0) * P::B_LD];
        }
      } else {
#pragma unroll
        for (int t = 0; t < 16; ++t) { const int k = kc + kslot(t, hb); dst[t] = k < kend ? (float)breg[(size_t)(kc + kslot(t, 0)) * P::B_LD] : 0.0f; }
      }
    } else {
      const int kl = kc + (lane & 31);
      const int rv = P::b_row(a, z, kl < kend ? kl : kbeg);
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int r = pick_half(rv, kslot(t, 0), hi);
        const float v = (float)bbase[(uint32_t)(r + bcol)];               // always in bounds (clamped k)
        dst[t] = kc + kslot(t, hb) < kend ? v : 0.0f;
      }
    }
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;

  int kc = kbeg + (wave < NW ? wave : 0) * 32;            // wave-uniform
  SDQN_STAMP(1);
  SDQN_STAMP(2);
  // No software prefetch across chunks: one register set keeps the kernels at ~64 VGPRs, so 7-8 waves per SIMD are
  // resident and hide each other's load latency (most waves own a single chunk at B = 32 anyway).
  // staged operands are software-prefetched one chunk ahead (4 x f4 per operand): registers -> panel -> fragment
  f4 pra[STG_A ? 4 : 1], prb[STG_B ? 4 : 1];
  auto stage_load = [&](int kk) {
    if constexpr (STG_A) {
      const aoff_t c = P::a_col(a, z, kk + 4 * (lane & 7));
#pragma unroll
      for (int j = 0; j < 4; ++j) pra[j] = P::a_load4(a, z, srow[j] + c);
    }
    if constexpr (STG_B) {
      const int r = P::b_row(a, z, kk + 4 * (lane & 7));
#pragma unroll
      for (int j = 0; j < 4; ++j) prb[j] = P::b_load4(a, z, r + scol[j]);
    }
  };
  (void)pra; (void)prb;
  if constexpr (STG_A || STG_B) { SDQN_WSTAMP(0); if (kc < kend) stage_load(kc); SDQN_WSTAMP(1); }
  while (kc < kend) {
    float fa[16], fb[16];
    SDQN_WSTAMP(0);
    if constexpr (!STG_A) load_a(kc, fa);
    if constexpr (!STG_B) load_b(kc, fb);
    if constexpr (STG_A || STG_B) {
      if constexpr (STG_A) {
        float* d = pan_a + (4 * (lane & 7)) * 33 + (lane >> 3);
#pragma unroll
        for (int j = 0; j < 4; ++j) { d[8 * j] = pra[j].x; d[33 + 8 * j] = pra[j].y; d[66 + 8 * j] = pra[j].z; d[99 + 8 * j] = pra[j].w; }
      }
      if constexpr (STG_B) {
        float* d = pan_b + (4 * (lane & 7)) * 33 + (lane >> 3);
#pragma unroll
        for (int j = 0; j < 4; ++j) { d[8 * j] = prb[j].x; d[33 + 8 * j] = prb[j].y; d[66 + 8 * j] = prb[j].z; d[99 + 8 * j] = prb[j].w; }
      }
      if (kc + NW * 32 < kend) stage_load(kc + NW * 32);   // next chunk's loads fly under this chunk's MFMAs
      wave_lds_sync();
      if constexpr (STG_A) {
#pragma unroll
        for (int t = 0; t < 16; ++t) fa[t] = pan_a[kslot(t, 0) * 33 + hb * (4 * 33) + (lane & 31)];
      }
      if constexpr (STG_B) {
#pragma unroll
        for (int t = 0; t < 16; ++t) fb[t] = pan_b[kslot(t, 0) * 33 + hb * (4 * 33) + (lane & 31)];
      }
      wave_lds_sync();                                     // panel reads issued before the next chunk's stores
    }
#ifdef SDQN_TIMING
    SDQN_WSTAMP(1);
    asm volatile("" :: "v"(fa[0]), "v"(fa[3]), "v"(fa[4]), "v"(fa[8]), "v"(fa[12]), "v"(fa[15]));      // A landed (its loads were issued first: in-order return)
    SDQN_WSTAMP(2);
    asm volatile("" :: "v"(fa[0]), "v"(fb[0]), "v"(fa[15]), "v"(fb[15]));      // operands landed
    SDQN_WSTAMP(3);
    SDQN_STAMP(3);
#endif
#pragma unroll
    for (int t = 0; t < 16; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[t], fb[t], acc, 0, 0, 0);
    kc += NW * 32;
  }

  // ---- epilogue: NW partial tiles -> LDS -> summed in fixed order -> P::store (lanes along n) ----
#ifdef SDQN_TIMING
  asm volatile("" :: "v"(acc[0]), "v"(acc[15]));
  SDQN_STAMP(4);
#endif
  if constexpr (NW > 1) {
    if (wave < NW) {
      float* cw = smem + wave * WAVE_LDS;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        cw[row * 33 + (lane & 31)] = acc[r];
      }
    }
    __syncthreads();
    SDQN_STAMP(5);
    for (int e = threadIdx.x; e < 1024; e += NT) {
      const int ml = e >> 5, nl = e & 31;
      float v = smem[ml * 33 + nl];
#pragma unroll
      for (int w = 1; w < NW; ++w) v += smem[w * WAVE_LDS + ml * 33 + nl];
      if (m0 + ml < M && n0 + nl < N) P::store(a, z, ks, m0 + ml, n0 + nl, v);
    }
  } else {
    float v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = acc[r];
    P::store16(a, z, ks, m0, n0, lane, M, N, v, epi);     // lane holds rows (r&3)+8(r>>2)+4(l>>5), column l&31
  }
  SDQN_STAMP(6);
  SDQN_WSTAMP_FLUSH;
}

// ---- 32 x 16 tile body: v_mfma_f32_16x16x4_f32 ----------------------------------------------------------------------------------
// For staged problems (both operands k-contiguous) whose N leaves most CUs without a 32-wide tile: half the columns per workgroup, twice
// the workgroups, half the matrix time and half the B panel on every CU.  Same structure as gemm_tile — wave w owns the 32-deep chunks
// w, w + NW, ..., runs them without a workgroup barrier with the next chunk's loads in flight, and the NW partial tiles are summed through
// LDS in wave order — on the maps of n16_map.h: a chunk is 8 k-steps x 2 row halves of the 16 x 16 x 4 instruction (32 cycles each, two
// independent accumulators: the 40-cycle dependent latency never shows), both halves on the same B fragment.  Exact fp32 like the
// 32 x 32 x 2 form, and the k-slot map feeds every element's fmaf chain the same k in the same order: bit-identical to gemm_tile.
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <class P, int NW, int NT>
__device__ __forceinline__ void gemm_tile_n16(const StepArgs& a, int bx, int by, int bz, float* smem) {
  static_assert(P::A_K && P::B_K && NW > 1, "32 x 16 body: both operands staged, K split over the waves");
  typedef typename P::aoff_t aoff_t;
  SDQN_STAMP(0);
  SDQN_WSTAMP_DECL;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = bx * n16::TM, n0 = by * n16::TN;
  int z, ks, kbeg, kend;
  P::ksplit(a, bz, z, ks, kbeg, kend);
  if (NW * 64 < NT && wave >= NW) kend = kbeg;          // surplus waves of a wider workgroup: no chunks
  const int M = P::M(a), N = P::N(a);

  float* pan_a = smem + (wave < NW ? wave : 0) * n16::WAVE_LDS;
  float* pan_b = pan_a + n16::PANEL_A;
  aoff_t srow[4]; int scol[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) { const int m = m0 + n16::ld_x(lane, j); srow[j] = P::a_row(a, z, m < M ? m : M - 1); }
#pragma unroll
  for (int j = 0; j < 2; ++j) { const int n = n0 + n16::ld_x(lane, j); scol[j] = P::b_col(a, z, n < N ? n : N - 1); }

  f4 pra[4], prb[2];
  auto stage_load = [&](int kk) {
    const aoff_t c = P::a_col(a, z, kk + n16::ld_k(lane));
#pragma unroll
    for (int j = 0; j < 4; ++j) pra[j] = P::a_load4(a, z, srow[j] + c);
    const int r = P::b_row(a, z, kk + n16::ld_k(lane));
#pragma unroll
    for (int j = 0; j < 2; ++j) prb[j] = P::b_load4(a, z, r + scol[j]);
  };
  int kc = kbeg + (wave < NW ? wave : 0) * 32;            // wave-uniform
  SDQN_STAMP(1);
  SDQN_STAMP(2);
  SDQN_WSTAMP(0);
  if (kc < kend) stage_load(kc);
  SDQN_WSTAMP(1);
  // the epilogue's element of this thread: known now, so a gating activation is fetched behind the operand loads instead of as a
  // dependent load after the combine (unconditional with clamped indexes: a guarded load costs a branch and a full vmcnt wait)
  const int el = threadIdx.x & (n16::TM * n16::TN - 1);
  const int ml = n16::epi_row(el), nl = n16::epi_col(el);
  const bool mine = threadIdx.x < n16::TM * n16::TN && m0 + ml < M && n0 + nl < N;
  float gate = 0.0f;
  if constexpr (gated_store<P>::value) gate = P::gate_load(a, z, m0 + ml < M ? m0 + ml : M - 1, n0 + nl < N ? n0 + nl : N - 1);
  (void)gate;

  f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
  while (kc < kend) {
    float fa0[8], fa1[8], fb[8];
    // registers -> panels: logical k = ld_k + e goes to panel row krow(k) (n16_map.h), columns as loaded
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = n16::ld_x(lane, j), k = n16::ld_k(lane);
      pan_a[n16::pan_off(n16::PA, k, x)] = pra[j].x; pan_a[n16::pan_off(n16::PA, k + 1, x)] = pra[j].y;
      pan_a[n16::pan_off(n16::PA, k + 2, x)] = pra[j].z; pan_a[n16::pan_off(n16::PA, k + 3, x)] = pra[j].w;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int x = n16::ld_x(lane, j), k = n16::ld_k(lane);
      pan_b[n16::pan_off(n16::PB, k, x)] = prb[j].x; pan_b[n16::pan_off(n16::PB, k + 1, x)] = prb[j].y;
      pan_b[n16::pan_off(n16::PB, k + 2, x)] = prb[j].z; pan_b[n16::pan_off(n16::PB, k + 3, x)] = prb[j].w;
    }
    if (kc + NW * 32 < kend) stage_load(kc + NW * 32);     // next chunk's loads fly under this chunk's MFMAs
    wave_lds_sync();
#pragma unroll
    for (int t = 0; t < 8; ++t) { fa0[t] = pan_a[n16::frag_a(lane, t, 0)]; fa1[t] = pan_a[n16::frag_a(lane, t, 1)]; fb[t] = pan_b[n16::frag_b(lane, t)]; }
    wave_lds_sync();                                       // panel reads issued before the next chunk's stores
#ifdef SDQN_TIMING
    asm volatile("" :: "v"(fa0[0]), "v"(fa1[7]));          // A landed (its loads were issued first: in-order return)
    SDQN_WSTAMP(2);
    asm volatile("" :: "v"(fb[0]), "v"(fb[7]));            // operands landed
    SDQN_WSTAMP(3);
    SDQN_STAMP(3);
#endif
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(fa0[t], fb[t], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(fa1[t], fb[t], acc1, 0, 0, 0);
    }
    kc += NW * 32;
  }

  // ---- epilogue: NW partial tiles -> LDS (the wave's own panels, done with) -> summed in wave order -> store ----
#ifdef SDQN_TIMING
  asm volatile("" :: "v"(acc0[0]), "v"(acc1[3]));
  SDQN_STAMP(4);
#endif
  if (wave < NW) {
    float* cw = smem + wave * n16::WAVE_LDS;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      cw[n16::comb_off(n16::acc_row(0, lane, r), n16::acc_col(lane))] = acc0[r];
      cw[n16::comb_off(n16::acc_row(1, lane, r), n16::acc_col(lane))] = acc1[r];
    }
  }
  __syncthreads();
  SDQN_STAMP(5);
  static_assert(NT >= n16::TM * n16::TN, "one thread per element of the tile");
  if (mine) {
    float v = smem[n16::comb_off(ml, nl)];
#pragma unroll
    for (int w = 1; w < NW; ++w) v += smem[w * n16::WAVE_LDS + n16::comb_off(ml, nl)];
    if constexpr (gated_store<P>::value) P::store_gated(a, z, ks, m0 + ml, n0 + nl, v, gate);
    else P::store(a, z, ks, m0 + ml, n0 + nl, v);
  }
  SDQN_STAMP(6);
  SDQN_WSTAMP_FLUSH;
}

// ---- 48 x 32 tile body: v_mfma_f32_16x16x4_f32 --------------------------------------------------------------------------------------
// For a direct-operand problem (A k-contiguous, B a plain [k][n] matrix, K a whole number of 32-deep chunks) whose 32-row tiles land two
// to a CU on part of the chip: 1.5 x the rows per workgroup, two thirds of the workgroups, one per CU.  Wave w owns the 32-deep chunks
// w, w + NW, ... as in gemm_tile; a chunk is 8 k-steps x 3 row groups x 2 column halves of the 16 x 16 x 4 instruction on six accumulators
// (m48_map.h).  The k-slot map is n16_map.h's, so every element's fmaf chain takes the same k in the same order as the 32 x 32 body's;
// the NW partial tiles pass through LDS in two halves of NW / 2 panels with the running sum carried in registers, in wave order:
// bit-identical to gemm_tile.
template <class P, int NW, int NT>
__device__ __forceinline__ void gemm_tile_m48(const StepArgs& a, int bx, int by, int bz, float* smem) {
  static_assert(P::A_K && !P::B_K && P::B_REG && !P::A_U8, "48 x 32 body: A k-contiguous floats, B a plain [k][n] matrix");
  static_assert(NW == 2 * m48::HALF_WAVES && NT == NW * 64, "two combine halves of 8 waves, no surplus waves");
  static_assert(sizeof(typename a_elem<P>::type) == 4 && sizeof(typename b_elem<P>::type) == 4, "fp32 operands");
  typedef typename P::aoff_t aoff_t;
  SDQN_STAMP(0);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = bx * m48::TM, n0 = by * m48::TN;
  int z, ks, kbeg, kend;
  P::ksplit(a, bz, z, ks, kbeg, kend);
  const int M = P::M(a), N = P::N(a);
  const float* bbase = P::b_ptr(a, z);
  // A: loader lane (k4 = l & 7, x = n16::ld_x(l, j)) fetches 16 bytes of row 16 rg + x — the 8 lanes of a k4 run read the 128 contiguous
  // bytes of one row's chunk — and the wave-private panel turns them into fragments, one row group at a time.  B: lane l owns columns
  // 16 h + (l & 15) at the k of its slot l >> 4.  (Clamped in bounds: rows past M are computed and not stored.)
  aoff_t srow[m48::RG][2]; int bcol[m48::CH];
#pragma unroll
  for (int rg = 0; rg < m48::RG; ++rg)
#pragma unroll
    for (int j = 0; j < 2; ++j) { const int m = m0 + m48::ld_row(lane, rg, j); srow[rg][j] = P::a_row(a, z, m < M ? m : M - 1); }
#pragma unroll
  for (int h = 0; h < m48::CH; ++h) { const int n = n0 + m48::frag_col(lane, h); bcol[h] = P::b_col(a, z, n < N ? n : N - 1); }
  const int klane = m48::kslot_lane(lane >> 4);
  float* pan = smem + m48::opnd_off(wave);

  f32x4 acc[m48::RG][m48::CH];
#pragma unroll
  for (int rg = 0; rg < m48::RG; ++rg)
#pragma unroll
    for (int h = 0; h < m48::CH; ++h) acc[rg][h] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  SDQN_STAMP(1);
  SDQN_STAMP(2);
  for (int kc = kbeg + wave * 32; kc < kend; kc += NW * 32) {      // wave-uniform
    f4 pra[m48::RG][2]; float fb[m48::CH][m48::STEPS];
    const aoff_t c = P::a_col(a, z, kc + n16::ld_k(lane));
    // (the last row group's two loads are issued behind the first group's panel stores and land under 32 MFMAs: 8 VGPRs less at the peak)
#pragma unroll
    for (int rg = 0; rg < m48::RG - 1; ++rg)
#pragma unroll
      for (int j = 0; j < 2; ++j) pra[rg][j] = P::a_load4(a, z, srow[rg][j] + c);
#pragma unroll
    for (int t = 0; t < m48::STEPS; ++t) {
      const int r = P::b_row(a, z, kc + m48::kslot_step(t) + klane);
#pragma unroll
      for (int h = 0; h < m48::CH; ++h) fb[h][t] = bbase[(uint32_t)(r + bcol[h])];
    }
#ifdef SDQN_TIMING
    asm volatile("" :: "v"(pra[0][0].x), "v"(pra[1][1].w), "v"(fb[0][0]), "v"(fb[1][7]));      // operands landed
    SDQN_STAMP(3);
#endif
    // row group by row group through the one panel: registers -> panel (logical k in row n16::krow(k)) -> fragments -> 16 MFMAs.  An
    // accumulator pair starts to live when its group begins, which keeps the kernel inside 64 VGPRs; the two column halves alternate,
    // so a dependent MFMA is 64 cycles behind its predecessor
#pragma unroll
    for (int rg = 0; rg < m48::RG; ++rg) {
      float fa[m48::STEPS];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int x = n16::ld_x(lane, j), k = n16::ld_k(lane);
        pan[m48::pan_off(k, x)] = pra[rg][j].x; pan[m48::pan_off(k + 1, x)] = pra[rg][j].y;
        pan[m48::pan_off(k + 2, x)] = pra[rg][j].z; pan[m48::pan_off(k + 3, x)] = pra[rg][j].w;
      }
      if (rg == 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) pra[m48::RG - 1][j] = P::a_load4(a, z, srow[m48::RG - 1][j] + c);
      }
      wave_lds_sync();
#pragma unroll
      for (int t = 0; t < m48::STEPS; ++t) fa[t] = pan[m48::frag_a(lane, t)];
      wave_lds_sync();                                     // panel reads issued before the next group's stores
#pragma unroll
      for (int t = 0; t < m48::STEPS; ++t)
#pragma unroll
        for (int h = 0; h < m48::CH; ++h) acc[rg][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[t], fb[h][t], acc[rg][h], 0, 0, 0);
    }
  }

  // ---- epilogue: NW partial tiles -> 8 panels, twice -> running sums in wave order -> P::store (32 consecutive lanes = one row) ----
#ifdef SDQN_TIMING
  asm volatile("" :: "v"(acc[0][0][0]), "v"(acc[2][1][3]));
  SDQN_STAMP(4);
#endif
  const int e0 = threadIdx.x, e1 = threadIdx.x + NT;
  const bool two = e1 < m48::TM * m48::TN;                 // waves 0-7: a second element (wave-uniform)
  const int o0 = m48::comb_off(m48::epi_row(e0), m48::epi_col(e0)), o1 = two ? m48::comb_off(m48::epi_row(e1), m48::epi_col(e1)) : o0;
  float v0 = 0.0f, v1 = 0.0f;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    if (half) __syncthreads();                             // the first half's panels are read before the second half's stores
    if (m48::comb_half(wave) == half) {
      float* cw = smem + m48::comb_panel(wave) * m48::PANEL_C;
#pragma unroll
      for (int rg = 0; rg < m48::RG; ++rg)
#pragma unroll
        for (int h = 0; h < m48::CH; ++h)
#pragma unroll
          for (int r = 0; r < 4; ++r) cw[m48::comb_off(m48::acc_row(rg, lane, r), m48::acc_col(h, lane))] = acc[rg][h][r];
    }
    __syncthreads();
    if (half) SDQN_STAMP(5);
#pragma unroll
    for (int w = 0; w < m48::HALF_WAVES; ++w) {
      const float p0 = smem[w * m48::PANEL_C + o0];
      v0 = (half == 0 && w == 0) ? p0 : v0 + p0;
      if (two) { const float p1 = smem[w * m48::PANEL_C + o1]; v1 = (half == 0 && w == 0) ? p1 : v1 + p1; }
    }
  }
  { const int m = m0 + m48::epi_row(e0), n = n0 + m48::epi_col(e0); if (m < M && n < N) P::store(a, z, ks, m, n, v0); }
  if (two) { const int m = m0 + m48::epi_row(e1), n = n0 + m48::epi_col(e1); if (m < M && n < N) P::store(a, z, ks, m, n, v1); }
  SDQN_STAMP(6);
}

// ---- fp16-mode tile body: packed-fp16 MFMA -------------------------------------------------------------------
// v_mfma_f32_32x32x16_f16: lane (i = l & 31, h = l >> 5) feeds 8 consecutive k (one 16-B load) of row i of A and of
// column i of B into k-slots 8h..8h+7; both operands of these problems are k-contiguous in memory (NHWC activations /
// padded deltas; TRANSPOSED half weight copies for forward, master-layout half copies for dgrad), so there is no LDS
// staging at all: 2 loads + 1 MFMA per 16 k.  A and B use the same slot <-> k assignment, so the result does not
// depend on the hardware's internal k numbering.  fp32 accumulation, same K-split / fixed-order combine as above.
template <class P, int NW, int NT>
__device__ __forceinline__ void gemm_tile_h(const StepArgs& a, int bx, int by, int bz, float* smem) {
  constexpr int WAVE_LDS = PANEL;
  typedef typename P::aoff_t aoff_t;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = bx * 32, n0 = by * 32;
  int z, ks, kbeg, kend;
  P::ksplit(a, bz, z, ks, kbeg, kend);
  if (NW * 64 < NT && wave >= NW) kend = kbeg;
  const int M = P::M(a), N = P::N(a);
  const int i = lane & 31, h8 = (lane >> 5) * 8;
  const aoff_t arow = P::a_row(a, z, m0 + i < M ? m0 + i : M - 1);
  const int bcol = P::b_col(a, z, n0 + i < N ? n0 + i : N - 1);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  for (int kc = kbeg + (wave < NW ? wave : 0) * 32; kc < kend; kc += NW * 32) {
    const half8 fa0 = P::a_load8(a, z, arow + P::a_col(a, z, kc + h8));
    const half8 fb0 = P::b_load8(a, z, bcol + P::b_row(a, z, kc + h8));
    const half8 fa1 = P::a_load8(a, z, arow + P::a_col(a, z, kc + 16 + h8));
    const half8 fb1 = P::b_load8(a, z, bcol + P::b_row(a, z, kc + 16 + h8));
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa0, fb0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa1, fb1, acc, 0, 0, 0);
  }
  if constexpr (NW > 1) {
    if (wave < NW) {
      float* cw = smem + wave * WAVE_LDS;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        cw[row * 33 + (lane & 31)] = acc[r];
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 1024; e += NT) {
      const int ml = e >> 5, nl = e & 31;
      float v = smem[ml * 33 + nl];
#pragma unroll
      for (int w = 1; w < NW; ++w) v += smem[w * WAVE_LDS + ml * 33 + nl];
      if (m0 + ml < M && n0 + nl < N) P::store(a, z, ks, m0 + ml, n0 + nl, v);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ml = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), nl = lane & 31;
      if (m0 + ml < M && n0 + nl < N) P::store(a, z, ks, m0 + ml, n0 + nl, acc[r]);
    }
  }
}



// ---- fp16-mode weight gradients on packed-fp16 MFMA ---------------------------------------------------------------
// C(m, n) = sum_k A(k, m) B(k, n) with k = (sample, output position): BOTH operands are contiguous along m / n in memory
// (NHWC activations, dense deltas), while v_mfma_f32_32x32x16_f16 wants 8 consecutive k per lane.  So every 32-deep
// K-chunk goes through a wave-private LDS transpose: lane (k = l & 31, part = l >> 5) fetches 16 consecutive halves
// (32 B, two 16-byte loads) of row k of each operand and stores them as [k][x] rows (pitch 40 halves: 16-byte aligned,
// conflict-free for the 8-lane groups of ds_write_b128); lane (i = l & 31, h = l >> 5) then reads its 8 k-values of
// column i with 8 ds_read_u16 (lanes along x: 64 contiguous bytes per half-wave, no conflicts) per MFMA operand.
// 4 loads + 4 wide stores + 32 narrow reads + 2 MFMAs per chunk instead of 32 loads + 16 fp32 MFMAs (1024 pipe cycles).
// conv1's A operand needs no transpose: the 4 output positions of an aligned k-group are 4 bytes apart in the u8 frame
// (A_GROUP4), so a lane builds its 8 k-values from two unaligned 16-byte ring loads, normalised and rounded to half like
// the forward pass does.  fp32 accumulation, K split over NW waves and combined in fixed order, same epilogues as the
// fp32-MFMA wgrads (loss scale divided out, fused RMSProp + half-copy refresh for fc4).
constexpr int HW_PITCH = 40;                                   // halves per staged k-row
constexpr int HW_TILE = 32 * HW_PITCH;                         // one [32 k][32 x] half tile: 2560 B
constexpr int HW_WAVE_LDS = (2 * HW_TILE * 2 + 3) / 4 > PANEL ? (2 * HW_TILE * 2 + 3) / 4 : PANEL;   // floats per wave: two half tiles, later one fp32 combine panel
static_assert(2 * HW_TILE * 2 <= HW_WAVE_LDS * 4 && PANEL <= HW_WAVE_LDS, "staging tiles / combine panel fit the per-wave region");
__device__ __forceinline__ half8 ld_half8(const half_t* p) { return *reinterpret_cast<const half8*>(p); }

template <class P, int NW, int NT>
__device__ __forceinline__ void gemm_tile_hw(const StepArgs& a, int bx, int by, int bz, float* smem) {
  typedef typename P::aoff_t aoff_t;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m0 = bx * 32, n0 = by * 32;
  int z, ks, kbeg, kend;
  P::ksplit(a, bz, z, ks, kbeg, kend);
  if (NW * 64 < NT && wave >= NW) kend = kbeg;
  const int M = P::M(a), N = P::N(a);
  const int i = lane & 31, hb = lane >> 5;
  const bool hi = lane >= 32;
  // NW == 1 inside a wider workgroup (one tile per wave, gemm_multi_kernel): every wave stages in its own region
  half_t* sa = reinterpret_cast<half_t*>(smem + (NW == 1 ? wave : (wave < NW ? wave : 0)) * HW_WAVE_LDS);
  half_t* sb = sa + HW_TILE;
  const half_t* bbase = P::b_ptr(a, z);
  // staging role: this lane fetches halves [16 * hb, 16 * hb + 16) of row k = kc + i of the chunk
  const int bcol16 = P::b_col(a, z, n0 + 16 * hb);
  aoff_t arow16 = 0, arow_own = 0;
  if constexpr (P::A_U8) arow_own = P::a_row(a, z, m0 + i < M ? m0 + i : M - 1);          // conv1: own row, direct
  else arow16 = P::a_row(a, z, m0 + 16 * hb);
  (void)arow16; (void)arow_own;

  typename P::Epi epi;
  if constexpr (NW == 1) P::epi_begin(a, m0, n0, lane, epi);

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;

  half8 pa0, pa1, pb0, pb1;                                    // staged rows of the NEXT chunk (prefetched)
  aoff_t cvn = 0;                                             // conv1: patch origin of k = kc + i of the next chunk
  auto stage_load = [&](int kc) {
    const int kl = kc + i;
    const int kk = kl < kend ? kl : kbeg;
    const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    const half_t* pb = bbase + (size_t)kk * P::B_LD + bcol16;
    pb0 = ld_half8(pb); pb1 = ld_half8(pb + 8);
    if (kl >= kend) { pb0 = zero; pb1 = zero; }
    if constexpr (P::A_U8) cvn = P::a_col(a, z, kk);
    else {
      const half_t* pa;
      if constexpr (P::A_REG) pa = P::a_ptr(a, z) + (size_t)kk * P::A_LD + (size_t)arow16;
      else pa = P::a_ptr(a, z) + (uint32_t)(arow16 + P::a_col(a, z, kk));
      pa0 = ld_half8(pa); pa1 = ld_half8(pa + 8);
      if (kl >= kend) { pa0 = zero; pa1 = zero; }
    }
  };
  int kc = kbeg + (wave < NW ? wave : 0) * 32;
  if (kc < kend) stage_load(kc);
  while (kc < kend) {
    // staged rows -> LDS ([k][x], pitch 40 halves)
    *reinterpret_cast<half8*>(sb + i * HW_PITCH + 16 * hb) = pb0;
    *reinterpret_cast<half8*>(sb + i * HW_PITCH + 16 * hb + 8) = pb1;
    if constexpr (!P::A_U8) {
      *reinterpret_cast<half8*>(sa + i * HW_PITCH + 16 * hb) = pa0;
      *reinterpret_cast<half8*>(sa + i * HW_PITCH + 16 * hb + 8) = pa1;
    }
    const aoff_t cv = cvn;
    const int kcur = kc;
    kc += NW * 32;
    if (kc < kend) stage_load(kc);                              // next chunk's loads fly under the transposes + MFMAs
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      half8 fa, fb;
#pragma unroll
      for (int j = 0; j < 8; ++j) fb[j] = sb[(16 * s + 8 * hb + j) * HW_PITCH + i];
      if constexpr (P::A_U8) {
        // k = kcur + 16 s + 8 h + 4 g + e: patch origins of the two aligned k-groups from lanes 16 s + 4 g (+ 8 for h = 1)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const int src = 16 * s + 4 * g;
          const int l0 = __builtin_amdgcn_readlane((int)(cv & 0xFFFFFFFF), src), l1 = __builtin_amdgcn_readlane((int)((int64_t)cv >> 32), src);
          const int u0 = __builtin_amdgcn_readlane((int)(cv & 0xFFFFFFFF), src + 8), u1 = __builtin_amdgcn_readlane((int)((int64_t)cv >> 32), src + 8);
          const int64_t lo = ((int64_t)l1 << 32) | (uint32_t)l0, up = ((int64_t)u1 << 32) | (uint32_t)u0;
          const int64_t c = hi ? up : lo;
          const bool ok = kcur + 16 * s + 8 * hb + 4 * g < kend;
          const f4 v = P::a_load_group4(a, z, arow_own + c);
          fa[4 * g] = ok ? (half_t)v.x : (half_t)0.0f; fa[4 * g + 1] = ok ? (half_t)v.y : (half_t)0.0f;
          fa[4 * g + 2] = ok ? (half_t)v.z : (half_t)0.0f; fa[4 * g + 3] = ok ? (half_t)v.w : (half_t)0.0f;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) fa[j] = sa[(16 * s + 8 * hb + j) * HW_PITCH + i];
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, acc, 0, 0, 0);
    }
    wave_lds_sync();                                            // tile reads issued before the next chunk's stores
  }

  if constexpr (NW > 1) {
    if (wave < NW) {                                            // the wave's own staging region becomes its combine panel
      float* cw = smem + wave * HW_WAVE_LDS;
#pragma unroll
      for (int r = 0; r < 16; ++r) cw[((r & 3) + 8 * (r >> 2) + 4 * hb) * 33 + i] = acc[r];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 1024; e += NT) {
      const int ml = e >> 5, nl = e & 31;
      float v = smem[ml * 33 + nl];
#pragma unroll
      for (int w = 1; w < NW; ++w) v += smem[w * HW_WAVE_LDS + ml * 33 + nl];
      if (m0 + ml < M && n0 + nl < N) P::store(a, z, ks, m0 + ml, n0 + nl, v);
    }
  } else {
    float v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = acc[r];
    P::store16(a, z, ks, m0, n0, lane, M, N, v, epi);
  }
}

template <class P, int NW, int NT>
__device__ __forceinline__ void run_tile(const StepArgs& a, int bx, int by, int bz, float* smem) {
  if constexpr (use_n16<P, NW>()) gemm_tile_n16<P, NW, NT>(a, bx, by, bz, smem);
  else if constexpr (use_m48<P, NW>()) gemm_tile_m48<P, NW, NT>(a, bx, by, bz, smem);
  else if constexpr (uses_f16_wgrad<P>::value) gemm_tile_hw<P, NW, NT>(a, bx, by, bz, smem);
  else if constexpr (uses_f16_mfma<P>::value) gemm_tile_h<P, NW, NT>(a, bx, by, bz, smem);
  else gemm_tile<P, NW, NT>(a, bx, by, bz, smem);
}
template <class P, int NW>
constexpr int tile_lds_any() {
  if constexpr (use_n16<P, NW>()) return NW * n16::WAVE_LDS;          // operand panels, reused as combine panels
  else if constexpr (use_m48<P, NW>()) return m48::LDS_FLOATS;      // the combine panels of one half of the waves + the A panels of the other half
  else if constexpr (uses_f16_wgrad<P>::value) return NW * HW_WAVE_LDS;   // staging tiles, reused as combine panels
  else return uses_f16_mfma<P>::value ? NW * PANEL : tile_lds<P, NW>();
}
// rows / columns of C one tile covers (NW: waves per tile of the launch form; 0 = a form without a narrow body)
template <class P, int NW = 0> constexpr int tile_m() { return use_m48<P, NW>() ? m48::TM : 32; }
template <class P, int NW = 0> constexpr int tile_n() { return use_n16<P, NW>() ? n16::TN : 32; }

// (xcd_tile_id / xcd_tile_id_range, the XCD-aware workgroup -> tile maps: problems.h — host + device, tests/emul executes them)

// a single-problem launch's arguments: a = the struct patched from the leading block and the tile grid from s0 (LEAD_ON), or the struct
// behind P::preload and the launch grid
template <class P>
__device__ __forceinline__ void lead_take(StepArgs& a, int& gx, int& gy, int& gz, const StepArgs& a_, SDQN_LEAD_PARAMS) {
  (void)lr0; (void)lr1;
  if (lctl & LEAD_ON) { lead_scalars(a, lB, lctl); P::lead_apply(a, lp0, lp1, lp2, lp3, lp4, ls1); gx = ls0 & 0xFFFF; gy = (ls0 >> 16) & 255; gz = ls0 >> 24; }
  else { if constexpr (has_preload<P>::value) P::preload(a_, gridDim.x, gridDim.y, gridDim.z); gx = gridDim.x; gy = gridDim.y; gz = gridDim.z; }
}
template <class P, int NW>
__device__ __forceinline__ void gemm_kernel_body(const StepArgs& a, int gx, int gy, int gz, float* smem) {
  const int lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
  const int t = (a.xcd_map & 1) ? xcd_tile_id(lin, gx * gy * gz) : lin;
  const int bz = t / (gx * gy), r = t - bz * (gx * gy);
  run_tile<P, NW, NW * 64>(a, r % gx, r / gx, bz, smem);
}
template <class P, int NW>
__global__ void __launch_bounds__(NW * 64) gemm_kernel(SDQN_LEAD_PARAMS, const StepArgs a_) {
  __shared__ float smem[tile_lds_any<P, NW>()];
  (void)lr0; (void)lr1;
  if constexpr (has_lead<P>::value) {
    StepArgs a = a_;
    int gx, gy, gz;
    lead_take<P>(a, gx, gy, gz, a_, SDQN_LEAD_FWD);
    gemm_kernel_body<P, NW>(a, gx, gy, gz, smem);
  } else {
    if constexpr (has_preload<P>::value) P::preload(a_, gridDim.x, gridDim.y, gridDim.z);
    gemm_kernel_body<P, NW>(a_, gridDim.x, gridDim.y, gridDim.z, smem);
  }
}

// ---- several independent problems in ONE launch -------------------------------------------------------
// Stages that depend on the same producer (e.g. conv3_dgrad, conv3_wgrad and fc4_wgrad all wait for
// fc4_dgrad only) run as one grid: workgroup ranges dispatch to different problem structs, so their latency
// chains overlap without cross-stream event waits and two launch ramps disappear.  A problem with NW == 1
// (fc4_wgrad at B <= 32) gets one TILE PER WAVE of the 1024-thread workgroup.
struct MultiDims { int n[3]; int gx[3], gy[3]; };       // workgroups per problem and its (x, y) tile grid

template <class P, int NW, int NT>
__device__ __forceinline__ void multi_dispatch(const StepArgs& a, const MultiDims& d, int which, int local, float* smem) {
  static_assert(!use_n16<P, NW>() && !use_m48<P, NW>(), "multi-problem launches size their tile grids for 32 x 32 tiles");
  if constexpr (NW == 1) {
    // one tile per wave; the launch owns the tile range [a.f4w_first, a.f4w_first + a.f4w_count)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = local * (NT / 64) + wave;
    const int per_z = d.gx[which] * d.gy[which];
    if (t < a.f4w_count) {
      const int tile = a.f4w_first + t;
      const int bz = tile / per_z, r = tile - bz * per_z;
      run_tile<P, 1, 64>(a, r % d.gx[which], r / d.gx[which], bz, smem);    // (n-fastest tile order measured: -0.4 %)
    }
  } else {
    const int per_z = d.gx[which] * d.gy[which];
    const int bz = local / per_z, r = local - bz * per_z;
    run_tile<P, NW, NT>(a, r % d.gx[which], r / d.gx[which], bz, smem);
  }
}

template <int NT, class P0, int NW0, class P1, int NW1, class P2, int NW2>
__device__ __forceinline__ void gemm_multi_body(const StepArgs& a, const MultiDims& d, float* smem) {
  const int b = blockIdx.x;                               // problem choice is workgroup-uniform; XCD-contiguous runs per problem
  const int xm = a.xcd_map;                               // bit i: problem i of the launch uses the XCD-contiguous map
  if (b < d.n[0]) multi_dispatch<P0, NW0, NT>(a, d, 0, (xm & 1) ? xcd_tile_id_range(b, 0, d.n[0]) : b, smem);
  else if (b < d.n[0] + d.n[1]) multi_dispatch<P1, NW1, NT>(a, d, 1, (xm & 2) ? xcd_tile_id_range(b, d.n[0], d.n[1]) : b - d.n[0], smem);
  else multi_dispatch<P2, NW2, NT>(a, d, 2, (xm & 4) ? xcd_tile_id_range(b, d.n[0] + d.n[1], d.n[2]) : b - d.n[0] - d.n[1], smem);
}
template <int NT, class P0, int NW0, class P1, int NW1, class P2, int NW2>
__global__ void __launch_bounds__(NT) gemm_multi_kernel(SDQN_LEAD_PARAMS, const StepArgs a_, const MultiDims d_) {
  // (a one-tile-per-wave problem needs one region per wave of the workgroup)
  constexpr int L0 = tile_lds_any<P0, NW0>() * (NW0 == 1 ? NT / 64 : 1), L1 = tile_lds_any<P1, NW1>() * (NW1 == 1 ? NT / 64 : 1),
                L2 = tile_lds_any<P2, NW2>() * (NW2 == 1 ? NT / 64 : 1);
  constexpr int L = L0 > L1 ? (L0 > L2 ? L0 : L2) : (L1 > L2 ? L1 : L2);
  __shared__ float smem[L];
  (void)lr0; (void)lr1;
  if constexpr (has_lead_multi<P1>::value) {
    // leading block of a multi-problem launch: s0 = workgroups of problem 0 | problem 1 << 16; the tile grids follow from B
    StepArgs a = a_; MultiDims d = d_;
    if (lctl & LEAD_ON) {
      lead_scalars(a, lB, lctl); P1::lead_apply(a, lp0, lp1, lp2, lp3, lp4, ls1);
      d.n[0] = ls0 & 0xFFFF; d.n[1] = (int)((unsigned)ls0 >> 16);
      // (multi_fill's formulas.  d.n[2] stays the struct's: its one reader is xcd_tile_id_range in problem 2's branch of gemm_multi_body — the
      //  choice of the problem compares b with n[0] and n[0] + n[1] only — and problem 2's workgroups wait for their own scalars anyway)
      d.gx[0] = (P0::M(a) + tile_m<P0>() - 1) / tile_m<P0>(); d.gy[0] = (P0::N(a) + tile_n<P0>() - 1) / tile_n<P0>();
      d.gx[1] = (P1::M(a) + tile_m<P1>() - 1) / tile_m<P1>(); d.gy[1] = (P1::N(a) + tile_n<P1>() - 1) / tile_n<P1>();
      d.gx[2] = (P2::M(a) + tile_m<P2>() - 1) / tile_m<P2>(); d.gy[2] = (P2::N(a) + tile_n<P2>() - 1) / tile_n<P2>();
    } else { if constexpr (has_preload_multi<P1>::value) P1::preload_multi(a_, d_); }
    gemm_multi_body<NT, P0, NW0, P1, NW1, P2, NW2>(a, d, smem);
  } else {
    if constexpr (has_preload_multi<P1>::value) P1::preload_multi(a_, d_);      // (one statement for the whole launch: every field of all its problems)
    gemm_multi_body<NT, P0, NW0, P1, NW1, P2, NW2>(a_, d_, smem);
  }
}

struct NoProblem {            // placeholder third problem for two-problem launches (never dispatched: n[2] = 0)
  static constexpr bool A_K = false, B_K = false; typedef int aoff_t; struct Epi {};
  static constexpr bool A_REG = false, A_U8 = false, B_REG = false; static constexpr int A_LD = 0, B_LD = 0;
  SDQN_HD static const float* a_ptr(const StepArgs&, int) { return nullptr; }
  SDQN_HD static const float* b_ptr(const StepArgs&, int) { return nullptr; }
  SDQN_HD static int M(const StepArgs&) { return 0; }
  SDQN_HD static int N(const StepArgs&) { return 0; }
  SDQN_HD static int nbz(const StepArgs&) { return 0; }
  SDQN_HD static void ksplit(const StepArgs&, int, int& z, int& ks, int& kb, int& ke) { z = ks = kb = ke = 0; }
  SDQN_HD static int a_row(const StepArgs&, int, int) { return 0; }
  SDQN_HD static int a_col(const StepArgs&, int, int) { return 0; }
  SDQN_HD static float a_load(const StepArgs&, int, int) { return 0.f; }
  SDQN_HD static f4 a_load4(const StepArgs&, int, int) { f4 o; o.x = o.y = o.z = o.w = 0.f; return o; }
  SDQN_HD static f4 b_load4(const StepArgs&, int, int) { f4 o; o.x = o.y = o.z = o.w = 0.f; return o; }
  SDQN_HD static int b_row(const StepArgs&, int, int) { return 0; }
  SDQN_HD static int b_col(const StepArgs&, int, int) { return 0; }
  SDQN_HD static float b_load(const StepArgs&, int, int) { return 0.f; }
  SDQN_HD static void store(const StepArgs&, int, int, int, int, float) {}
  __device__ static void epi_begin(const StepArgs&, int, int, int, Epi&) {}
  __device__ static void store16(const StepArgs&, int, int, int, int, int, int, int, const float*, Epi&) {}
};

template <class P, int NW>
inline hipError_t launch_gemm(const StepArgs& a, hipStream_t stream) {
  dim3 grid((P::M(a) + tile_m<P, NW>() - 1) / tile_m<P, NW>(), (P::N(a) + tile_n<P, NW>() - 1) / tile_n<P, NW>(), P::nbz(a));
  Lead l; memset(&l, 0, sizeof l);
  if constexpr (has_lead<P>::value) {                       // (the tile grid rides packed in one dword: a larger grid reads the struct)
    P::lead_pack(a, l); l.B = a.B; l.s0 = lead_grid(grid);
    l.ctl = lead_ctl(a, a.arg_preload && lead_grid_fits(grid));
  }
  SDQN_LAUNCH((gemm_kernel<P, NW>), grid, dim3(NW * 64), 0, stream, SDQN_LEAD_ARGS(l), a);
  return hipGetLastError();
}

template <int NT, class P, int NW>
inline void multi_fill(const StepArgs& a, MultiDims& d, int i) {
  d.gx[i] = (P::M(a) + tile_m<P>() - 1) / tile_m<P>(); d.gy[i] = (P::N(a) + tile_n<P>() - 1) / tile_n<P>();
  const int tiles = d.gx[i] * d.gy[i] * P::nbz(a);
  d.n[i] = NW == 1 ? (a.f4w_count + NT / 64 - 1) / (NT / 64) : tiles;    // NW == 1: one tile per wave, range from StepArgs
}
template <int NT, class P0, int NW0, class P1, int NW1, class P2, int NW2>
inline hipError_t launch_multi(const StepArgs& a, bool has1, bool has2, hipStream_t stream) {
  static_assert(NW0 * 64 <= NT && NW1 * 64 <= NT && NW2 * 64 <= NT, "waves per tile exceed the workgroup");
  MultiDims d; memset(&d, 0, sizeof d);
  multi_fill<NT, P0, NW0>(a, d, 0);
  if (has1) multi_fill<NT, P1, NW1>(a, d, 1);
  if (has2) multi_fill<NT, P2, NW2>(a, d, 2);
  if (d.n[0] + d.n[1] + d.n[2] == 0) return hipSuccess;
  Lead l; memset(&l, 0, sizeof l);
  if constexpr (has_lead_multi<P1>::value) {
    P1::lead_pack(a, l); l.B = a.B; l.s0 = (int)((unsigned)d.n[0] | (unsigned)d.n[1] << 16);
    l.ctl = lead_ctl(a, a.arg_preload && has1 && has2 && d.n[0] < 65536 && d.n[1] < 65536);
  }
  SDQN_LAUNCH((gemm_multi_kernel<NT, P0, NW0, P1, NW1, P2, NW2>), dim3(d.n[0] + d.n[1] + d.n[2]), dim3(NT), 0, stream, SDQN_LEAD_ARGS(l), a, d);
  return hipGetLastError();
}

}  // namespace sdqn

// m48_map.h — index maps of the latency engine's 48 x 32 tile body (gemm_engine.h: gemm_tile_m48), the routine of a direct-operand problem
// whose 32-row tiles leave some CUs with two workgroups and the rest with one (conv2_fwd below B = 128: at B = 32, 2 nets x 2 592 rows
// x 64 maps = 324 tiles of 32 x 32 on 256 CUs, but 216 tiles of 48 x 32: one per CU).  Host + device: tests/emul/emul_m48.cpp executes the
// very same maps on the CPU, so fragment coverage, the k-slot agreement of A and B, the accumulator rows, the order of the K sum, the
// two-half combine and the LDS banking are checked without a GPU.
//
// One wave owns one 32-deep K-chunk of a 48 (m) x 32 (n) tile: 8 steps of v_mfma_f32_16x16x4_f32 for each of 3 row groups x 2 column
// halves, six accumulators; an A fragment serves both column halves, a B fragment all three row groups.  MFMA maps (16 x 16 x 4, f32) as
// in n16_map.h: lane l feeds A[i = l & 15][k-slot l >> 4] and B[k-slot l >> 4][j = l & 15]; register r of lane l is D[4 (l >> 4) + r][l & 15].
// B is n-contiguous and goes straight from global memory into that layout with dword loads (16 lanes read 64 contiguous bytes of one k
// row).  A is k-contiguous: whole 128-byte rows of the chunk are fetched with 16-byte loads and transposed through a wave-private LDS
// panel, one row group at a time (dword loads of A straight into the layout — 16 rows x 32 bytes per instruction, 24 per lane —
// measured 7.5 us per step slower than the 32 x 32 body: DESIGN.md 30).
//
// SAME SUM, SAME ORDER as the 32 x 32 body: step t, slot g consumes k = kc + n16::kslot(t, g) — n16_map.h derives why that reproduces
// the 32 x 32 x 2 body's fmaf chain — and the formula is not repeated here: kslot splits into a step part and a lane part (checked
// below for every (t, g)), so a lane adds its own constant once and the steps are compile-time offsets.
//
// Combine: 16 partial tiles of 48 x 32 floats are 96 KB; the launch keeps to 80 KB of LDS, so the partials pass through 8 panels in two
// barrier-separated halves — waves 0-7, then waves 8-15 — and every thread carries the running sum of its elements across the halves:
// p0 + p1 + ... + p15 in wave order, as the 32 x 32 body adds them.  Banking (ds_write_b32 / ds_read_b32: two groups of 32 lanes, bank =
// dword address mod 32): a store group holds two k-slot quarters = rows 4 apart x 16 consecutive columns, so the pitch PC must put rows
// 4 apart 16 banks apart: PC = 36 (4 x 36 = 144 = 16 mod 32); a read group is 32 consecutive columns of one row.  The emulator counts
// the extra LDS cycles of both: 0.
#pragma once
#include "n16_map.h"

namespace sdqn {
namespace m48 {

constexpr int TM = 48, TN = 32, KC = 32;      // tile rows, tile columns, chunk depth
constexpr int RG = TM / 16, CH = TN / 16;     // row groups, column halves of the 16 x 16 instruction
constexpr int STEPS = KC / 4;                 // MFMA steps per (row group, column half)
constexpr int PC = 36;                        // floats per row of a combine panel
constexpr int PANEL_C = TM * PC;              // 6 912 B
constexpr int HALF_WAVES = 8;                 // waves per combine half: 8 panels = 55 296 B

// k of MFMA step t, slot g (= lane >> 4), relative to the chunk: n16::kslot(t, g) = kslot_step(t) + kslot_lane(g)
SDQN_HD constexpr int kslot_step(int t) { return n16::kslot(t, 0); }
SDQN_HD constexpr int kslot_lane(int g) { return n16::kslot(0, g); }
constexpr bool kslot_splits() {
  for (int t = 0; t < STEPS; ++t) for (int g = 0; g < 4; ++g) if (n16::kslot(t, g) != kslot_step(t) + kslot_lane(g)) return false;
  return true;
}
static_assert(kslot_splits(), "the k-slot map is a step part plus a lane part");
// A: one row group (16 rows x 32 k) at a time through a wave-private panel that is n16_map.h's B panel with rows for columns — its loader
// items (n16::ld_k, n16::ld_x, j < 2), its row permutation n16::krow and pitch n16::PB, its fragment read: conflict-free there, so here
constexpr int PANEL_A = n16::PANEL_B;         // 2 176 B
SDQN_HD constexpr int ld_row(int lane, int rg, int j) { return 16 * rg + n16::ld_x(lane, j); }
SDQN_HD constexpr int pan_off(int k, int x) { return n16::pan_off(n16::PB, k, x); }
SDQN_HD constexpr int frag_a(int lane, int t) { return n16::frag_b(lane, t); }      // row lane & 15 at k = n16::kslot(t, lane >> 4)
// fragment of lane l: row of row group rg (A), column of column half h (B)
SDQN_HD constexpr int frag_row(int lane, int rg) { return 16 * rg + (lane & 15); }
SDQN_HD constexpr int frag_col(int lane, int h) { return 16 * h + (lane & 15); }
// register r (0..3) of accumulator (rg, h) of lane l
SDQN_HD constexpr int acc_row(int rg, int lane, int r) { return 16 * rg + 4 * (lane >> 4) + r; }
SDQN_HD constexpr int acc_col(int h, int lane) { return 16 * h + (lane & 15); }
SDQN_HD constexpr int comb_off(int row, int col) { return row * PC + col; }
// combine half of wave w and its panel there
SDQN_HD constexpr int comb_half(int wave) { return wave / HALF_WAVES; }
SDQN_HD constexpr int comb_panel(int wave) { return wave % HALF_WAVES; }
// LDS of the workgroup, in floats: the 8 combine panels, then the A panels of waves 8-15.  The A panel of a wave of the first half lies
// inside its own combine panel, the only one written before the first barrier — by that wave, when its chunks are done; the second
// half's stores come after a barrier that every wave reaches with its A panel done with.  72 704 B
SDQN_HD constexpr int opnd_off(int wave) { return wave < HALF_WAVES ? wave * PANEL_C : HALF_WAVES * PANEL_C + (wave - HALF_WAVES) * PANEL_A; }
constexpr int LDS_FLOATS = HALF_WAVES * PANEL_C + HALF_WAVES * PANEL_A;
static_assert(PANEL_A <= PANEL_C && LDS_FLOATS * 4 <= 80 * 1024, "A panels inside the owner's combine panel; the launch keeps to 80 KB");
// epilogue: thread tid of NT sums elements tid and tid + NT (the second only where it exists) and stores them
SDQN_HD constexpr int epi_row(int e) { return e >> 5; }
SDQN_HD constexpr int epi_col(int e) { return e & 31; }

}  // namespace m48
}  // namespace sdqn

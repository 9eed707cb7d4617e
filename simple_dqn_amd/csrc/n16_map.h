// n16_map.h — index maps of the latency engine's 32 x 16 tile body (gemm_engine.h: gemm_tile_n16), the routine of staged problems whose
// 32-wide tiles leave CUs idle (fc4_dgrad below B = 128: N = 3136 = 98 x 32 = 196 x 16).  Host + device: tests/emul/emul_n16.cpp executes
// the very same maps on the CPU (simulated panels, simulated MFMA lanes), so loader coverage, the k-slot agreement of A and B, the
// accumulator rows, the order of the K sum and the LDS banking are checked without a GPU.
//
// One wave owns one 32-deep K-chunk of a 32 (m) x 16 (n) tile.  Both operands are k-contiguous in memory and go through wave-private LDS
// panels like the 32 x 32 body's: A 32 k x 32 rows, B 32 k x 16 columns.  The chunk is 8 steps of v_mfma_f32_16x16x4_f32 for each
// of the two row halves (accumulator 0: rows 0-15, accumulator 1: rows 16-31); both halves use the same B fragment.
// MFMA maps (16 x 16 x 4, f32): lane l feeds A[i = l & 15][k-slot l >> 4] and B[k-slot l >> 4][j = l & 15]; register r of lane l is
// D[4 (l >> 4) + r][l & 15].
//
// SAME SUM, SAME ORDER as the 32 x 32 body.  An f32 MFMA is an fmaf chain over its k-slots in slot order, so an element of the 32 x 32
// body's partial tile is the chain over k = kc + 8 (t >> 2) + 4 h + (t & 3) for t = 0..15, h = 0, 1 (gemm_engine.h: kslot).  Here
// position 4 t + g of the chain (step t = 0..7, slot g = 0..3) takes exactly the k of that chain's position 2 t' + h with t' = 2 t + (g >> 1),
// h = g & 1: kslot(t, g) below.  The partial tiles are then summed in wave order as before, so every element is bit-identical to the
// 32 x 32 body's (tests/test_emul_n16.py on the fmaf model; tests/test_gpu_fc4_dgrad_tiles.py against the 32 x 32 instantiation).
//
// Banking (ds_read_b32 / ds_write_b32: two groups of 32 lanes, bank = dword address mod 32): a read group holds two k-slots x 16
// consecutive x, so the two slots' panel rows must lie 16 banks apart, while kslot puts them 4 k apart.  So logical k lives in panel row
// krow(k) — the row the read at (t, g) wants is 16 (g & 1) + 8 (g >> 1) + t — at odd pitches (33 / 17): reads are conflict-free.  Stores:
// lane (k4 = l & 7, c = (l >> 3) & 3) writes k = 4 k4 + e, whose rows are {0, 2, 4, 6} + {0, 16} + const(e) over k4, at columns
// {0, 1, 8, 9}[c] + const: 32 distinct banks per group.  The emulator counts the extra LDS cycles of every access: 0.
#pragma once
#include "problems.h"

namespace sdqn {
namespace n16 {

constexpr int TM = 32, TN = 16, KC = 32;      // tile rows, tile columns, chunk depth
constexpr int PA = 33, PB = 17;               // floats per k-row of the A / B panel
constexpr int PC = 16;                        // floats per row of a wave's combine panel (read by 32 consecutive lanes: two whole rows)
constexpr int PANEL_A = KC * PA, PANEL_B = KC * PB;
constexpr int WAVE_LDS = PANEL_A + PANEL_B;   // floats per wave: 6 400 B (16 waves: 100 KB, one workgroup per CU)
static_assert(TM * PC <= WAVE_LDS, "a wave's combine panel reuses its operand panels");

// loader: lane l fetches 4 consecutive k (one 16-byte load) at k = ld_k(l) of row / column ld_x(l, j), j < TM / 8 (A) or TN / 8 (B):
// the 8 lanes of a k4 run read 128 contiguous bytes of one row; which rows share an instruction is chosen for the stores' banks (above)
SDQN_HD constexpr int ld_k(int lane) { return 4 * (lane & 7); }
SDQN_HD constexpr int ld_x(int lane, int j) {
  const int c = (lane >> 3) & 3, q = 2 * j + (lane >> 5);
  return (c & 1) + 8 * (c >> 1) + 2 * (q & 3) + 16 * (q >> 2);
}
// panel row of logical k (a permutation of 0..31) and the panel offset of (k, x)
SDQN_HD constexpr int krow(int k) { return 16 * ((k >> 2) & 1) + 8 * (k & 1) + 2 * (k >> 3) + ((k >> 1) & 1); }
SDQN_HD constexpr int pan_off(int pitch, int k, int x) { return krow(k) * pitch + x; }
// MFMA step t (0..7) of the chunk, slot g = l >> 4, consumes logical k = kc + kslot(t, g) — the same for A and B; krow(kslot(t, g)) =
// 16 (g & 1) + 8 (g >> 1) + t
SDQN_HD constexpr int kslot(int t, int g) { return 8 * ((2 * t + (g >> 1)) >> 2) + 4 * (g & 1) + ((2 * t + (g >> 1)) & 3); }
// fragment of lane l at step t: row half h of A, the 16 columns of B
SDQN_HD constexpr int frag_a(int lane, int t, int h) { return pan_off(PA, kslot(t, lane >> 4), 16 * h + (lane & 15)); }
SDQN_HD constexpr int frag_b(int lane, int t) { return pan_off(PB, kslot(t, lane >> 4), lane & 15); }
// register r (0..3) of accumulator h of lane l
SDQN_HD constexpr int acc_row(int h, int lane, int r) { return 16 * h + 4 * (lane >> 4) + r; }
SDQN_HD constexpr int acc_col(int lane) { return lane & 15; }
SDQN_HD constexpr int comb_off(int row, int col) { return row * PC + col; }
// epilogue: thread e < TM * TN sums element (e >> 4, e & 15) of the waves' panels in wave order and stores it
SDQN_HD constexpr int epi_row(int e) { return e >> 4; }
SDQN_HD constexpr int epi_col(int e) { return e & 15; }

}  // namespace n16
}  // namespace sdqn

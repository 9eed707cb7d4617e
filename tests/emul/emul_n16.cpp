// emul_n16.cpp — TEST-ONLY host executor of the latency engine's 32 x 16 tile body (simple_dqn_amd/csrc/gemm_engine.h: gemm_tile_n16)
// on the maps of n16_map.h.  A simulated workgroup — 16 waves x 64 lanes, wave-private LDS panels, the documented lane semantics of
// v_mfma_f32_16x16x4_f32 (lane l feeds A[l & 15][k-slot l >> 4] and B[k-slot l >> 4][l & 15]; register r of lane l is
// D[4 (l >> 4) + r][l & 15]) — runs fc4_dgrad through Fc4Dgrad's own index functions and its own store, so a hole in the loader
// coverage, a disagreement of the A and B k-slot maps, a wrong accumulator row or a wrong epilogue element shows on the CPU.
// It is NOT part of the product: nothing under simple_dqn_amd/ links or loads it.
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <set>
#include <vector>
#include "../../simple_dqn_amd/csrc/n16_map.h"

using namespace sdqn;

// extra LDS cycles of one ds_read_b32 / ds_write_b32: two groups of 32 lanes, bank = dword address mod 32, equal addresses broadcast
static int conflict_cycles(const int* addr /*[64]*/) {
  int extra = 0;
  for (int g = 0; g < 2; ++g) {
    std::set<int> per_bank[32];
    for (int l = 32 * g; l < 32 * g + 32; ++l) per_bank[addr[l] & 31].insert(addr[l]);
    int worst = 1;
    for (auto& s : per_bank) worst = (int)s.size() > worst ? (int)s.size() : worst;
    extra += worst - 1;
  }
  return extra;
}

// One wave's chunk with TAGS instead of numbers: panel slots hold (x, k) ids, the MFMA lane semantics pair them up.
// count[(row * 16 + col) * 32 + k] += 1 for every product the 16 instructions form; returns the number of products whose A and B k
// differ or that land in an accumulator register claiming another (row, col).  conflicts[0..2] = extra LDS cycles of the A-panel stores,
// the B-panel stores and the fragment reads.
extern "C" int n16_chunk_cover(int* count, int* conflicts) {
  using namespace n16;
  std::vector<int> pa(PANEL_A, -1), pb(PANEL_B, -1);
  int addr[64];
  conflicts[0] = conflicts[1] = conflicts[2] = 0;
  for (int j = 0; j < TM / 8; ++j) for (int e = 0; e < 4; ++e) {
    for (int l = 0; l < 64; ++l) { const int k = ld_k(l) + e, x = ld_x(l, j); addr[l] = pan_off(PA, k, x); pa[addr[l]] = x * KC + k; }
    conflicts[0] += conflict_cycles(addr);
  }
  for (int j = 0; j < TN / 8; ++j) for (int e = 0; e < 4; ++e) {
    for (int l = 0; l < 64; ++l) { const int k = ld_k(l) + e, x = ld_x(l, j); addr[l] = pan_off(PB, k, x); pb[addr[l]] = x * KC + k; }
    conflicts[1] += conflict_cycles(addr);
  }
  int bad = 0;
  for (int t = 0; t < 8; ++t) {
    for (int h = 0; h < 2; ++h) { for (int l = 0; l < 64; ++l) addr[l] = frag_a(l, t, h); conflicts[2] += conflict_cycles(addr); }
    for (int l = 0; l < 64; ++l) addr[l] = frag_b(l, t);
    conflicts[2] += conflict_cycles(addr);
    for (int h = 0; h < 2; ++h)
      for (int l = 0; l < 64; ++l) for (int r = 0; r < 4; ++r) {       // register r of lane l: D[i][jn]
        const int i = 4 * (l >> 4) + r, jn = l & 15;
        for (int s = 0; s < 4; ++s) {
          const int ta = pa[frag_a(16 * s + i, t, h)], tb = pb[frag_b(16 * s + jn, t)];
          if (ta < 0 || tb < 0) { ++bad; continue; }
          const int row = ta / KC, ka = ta % KC, col = tb / KC, kb = tb % KC;
          if (ka != kb || row != acc_row(h, l, r) || col != acc_col(l)) { ++bad; continue; }
          count[(row * TN + col) * KC + ka] += 1;
        }
      }
  }
  return bad;
}

// fc4_dgrad of a whole batch on the simulated workgroups: d3 / d3p through Fc4Dgrad::store.  ids != 0: the value stored for (m, n) is
// m * 3136 + n + 1 instead of the sum (exact in fp32), so the caller sees which element went to which address.
// mn_count[m * 3136 + n] += 1 per store the epilogue issues; conflicts[0] / [1] = extra LDS cycles of the combine stores / reads.
extern "C" int n16_fc4_dgrad(int B, const float* d4, const float* w4i, const float* a3, float* d3, float* d3p, int ids, int* mn_count, int* conflicts) {
  using namespace n16;
  typedef Fc4Dgrad P;
  constexpr int NW = 16;
  std::vector<float> theta((size_t)OFF4 + NW4);
  memcpy(theta.data() + OFF4, w4i, (size_t)NW4 * sizeof(float));
  StepArgs a; memset(&a, 0, sizeof a);
  a.B = B; a.nz = 2; a.theta[0] = theta.data(); a.theta[1] = theta.data();
  a.d4 = const_cast<float*>(d4); a.a3 = const_cast<float*>(a3); a.d3 = d3; a.d3p = d3p;
  const int M = P::M(a), N = P::N(a);
  const int gx = (M + TM - 1) / TM, gy = (N + TN - 1) / TN;
  int z, ks, kbeg, kend; P::ksplit(a, 0, z, ks, kbeg, kend);
  conflicts[0] = conflicts[1] = 0;
  std::vector<float> smem((size_t)NW * WAVE_LDS);
  int addr[64];
  for (int by = 0; by < gy; ++by) for (int bx = 0; bx < gx; ++bx) {
    const int m0 = bx * TM, n0 = by * TN;
    std::vector<float> acc((size_t)NW * 2 * 64 * 4, 0.f);            // [wave][h][lane][r]
    for (int wave = 0; wave < NW; ++wave) {
      float* pan_a = smem.data() + (size_t)wave * WAVE_LDS; float* pan_b = pan_a + PANEL_A;
      for (int kc = kbeg + wave * KC; kc < kend; kc += NW * KC) {
        for (int i = 0; i < WAVE_LDS; ++i) pan_a[i] = -1e30f;        // a missed slot poisons the result
        for (int l = 0; l < 64; ++l) {
          for (int j = 0; j < TM / 8; ++j) {
            const int m = m0 + ld_x(l, j);
            const f4 v = P::a_load4(a, z, P::a_row(a, z, m < M ? m : M - 1) + P::a_col(a, z, kc + ld_k(l)));
            const float e4[4] = {v.x, v.y, v.z, v.w};
            for (int e = 0; e < 4; ++e) pan_a[pan_off(PA, ld_k(l) + e, ld_x(l, j))] = e4[e];
          }
          for (int j = 0; j < TN / 8; ++j) {
            const int n = n0 + ld_x(l, j);
            const f4 v = P::b_load4(a, z, P::b_row(a, z, kc + ld_k(l)) + P::b_col(a, z, n < N ? n : N - 1));
            const float e4[4] = {v.x, v.y, v.z, v.w};
            for (int e = 0; e < 4; ++e) pan_b[pan_off(PB, ld_k(l) + e, ld_x(l, j))] = e4[e];
          }
        }
        for (int t = 0; t < 8; ++t) for (int h = 0; h < 2; ++h)
          for (int l = 0; l < 64; ++l) for (int r = 0; r < 4; ++r) {
            const int i = 4 * (l >> 4) + r, jn = l & 15;
            float d = acc[(((size_t)wave * 2 + h) * 64 + l) * 4 + r];
            for (int s = 0; s < 4; ++s) d = fmaf(pan_a[frag_a(16 * s + i, t, h)], pan_b[frag_b(16 * s + jn, t)], d);      // an fmaf chain in slot order
            acc[(((size_t)wave * 2 + h) * 64 + l) * 4 + r] = d;
          }
      }
    }
    for (int wave = 0; wave < NW; ++wave) {                          // partial tiles -> the waves' combine panels
      float* cw = smem.data() + (size_t)wave * WAVE_LDS;
      for (int i = 0; i < TM * PC; ++i) cw[i] = -1e30f;
      for (int h = 0; h < 2; ++h) for (int r = 0; r < 4; ++r) {
        for (int l = 0; l < 64; ++l) { addr[l] = comb_off(acc_row(h, l, r), acc_col(l)); cw[addr[l]] = acc[(((size_t)wave * 2 + h) * 64 + l) * 4 + r]; }
        if (wave == 0 && bx == 0 && by == 0) conflicts[0] += conflict_cycles(addr);
      }
    }
    for (int e0 = 0; e0 < TM * TN; e0 += 64) {                       // the epilogue's threads, one wave of them at a time
      for (int l = 0; l < 64; ++l) addr[l] = comb_off(epi_row(e0 + l), epi_col(e0 + l));
      if (bx == 0 && by == 0) conflicts[1] += conflict_cycles(addr);
      for (int l = 0; l < 64; ++l) {
        const int ml = epi_row(e0 + l), nl = epi_col(e0 + l);
        if (m0 + ml >= M || n0 + nl >= N) continue;
        float v = smem[comb_off(ml, nl)];
        for (int w = 1; w < NW; ++w) v += smem[(size_t)w * WAVE_LDS + comb_off(ml, nl)];
        if (ids) v = (float)((m0 + ml) * NIN4 + n0 + nl + 1);
        mn_count[(m0 + ml) * NIN4 + n0 + nl] += 1;
        P::store(a, z, ks, m0 + ml, n0 + nl, v);
      }
    }
  }
  return 0;
}

// The 32 x 32 body's sum of the same product on the same model (gemm_engine.h: gemm_tile): wave w's partial is the fmaf chain over
// k = 32 w + 8 (t >> 2) + 4 h + (t & 3), t = 0..15, h = 0, 1 (v_mfma_f32_32x32x2_f32: two k-slots per step), the 16 partials are added in
// wave order, the mask is a3 > 0.  out[m * 3136 + n]
extern "C" void n32_fc4_dgrad_ref(int B, const float* d4, const float* w4i, const float* a3, float* out) {
  for (int m = 0; m < B; ++m) for (int n = 0; n < NIN4; ++n) {
    float v = 0.f;
    for (int w = 0; w < 16; ++w) {
      float p = 0.f;
      for (int t = 0; t < 16; ++t) for (int h = 0; h < 2; ++h) {
        const int k = 32 * w + 8 * (t >> 2) + 4 * h + (t & 3);
        p = fmaf(d4[(size_t)m * NFC + k], w4i[(size_t)n * NFC + k], p);
      }
      v = w == 0 ? p : v + p;
    }
    out[(size_t)m * NIN4 + n] = a3[(size_t)m * NIN4 + n] > 0.0f ? v : 0.0f;
  }
}

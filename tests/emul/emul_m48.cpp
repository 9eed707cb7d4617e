// emul_m48.cpp — TEST-ONLY host executor of the latency engine's 48 x 32 tile body (simple_dqn_amd/csrc/gemm_engine.h: gemm_tile_m48)
// on the maps of m48_map.h.  A simulated workgroup — 16 waves x 64 lanes, the documented lane semantics of v_mfma_f32_16x16x4_f32 (lane l
// feeds A[l & 15][k-slot l >> 4] and B[k-slot l >> 4][l & 15]; register r of lane l is D[4 (l >> 4) + r][l & 15]), eight combine panels
// used twice — runs conv2_fwd through Conv2Fwd's own index functions and its own store, so a hole in the fragment coverage, a
// disagreement of the A and B k-slots, a wrong accumulator row, a wrong combine order or a wrong epilogue element shows on the CPU.
// It is NOT part of the product: nothing under simple_dqn_amd/ links or loads it.
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <set>
#include <vector>
#include "../../simple_dqn_amd/csrc/m48_map.h"

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

// One wave's chunk with TAGS instead of numbers: every lane's fragment is (row or column, k); the MFMA lane semantics pair them up.
// count[(row * 32 + col) * 32 + k] += 1 for every product the 48 instructions form; returns the number of products whose A and B k differ
// or that land in an accumulator register claiming another (row, col).
extern "C" int m48_chunk_cover(int* count) {
  using namespace m48;
  int bad = 0;
  for (int rg = 0; rg < RG; ++rg) for (int t = 0; t < STEPS; ++t) for (int h = 0; h < CH; ++h)
    for (int l = 0; l < 64; ++l) for (int r = 0; r < 4; ++r) {           // register r of lane l: D[i][jn]
      const int i = 4 * (l >> 4) + r, jn = l & 15;
      for (int s = 0; s < 4; ++s) {
        const int la = 16 * s + i, lb = 16 * s + jn;                     // the lanes that feed slot s of A row i / B column jn
        const int row = frag_row(la, rg), ka = kslot_step(t) + kslot_lane(la >> 4);
        const int col = frag_col(lb, h), kb = kslot_step(t) + kslot_lane(lb >> 4);
        if (ka != kb || ka != n16::kslot(t, s) || row != acc_row(rg, l, r) || col != acc_col(h, l)) { ++bad; continue; }
        count[(row * TN + col) * KC + ka] += 1;
      }
    }
  return bad;
}

// conv2_fwd of both nets of a batch on the simulated workgroups: a2 through Conv2Fwd::store.  a1 [2][B * 400][32], w2 [2][512][64],
// a2 [2][B * 81][64].  ids != 0: the value stored for (z, m, n) is (z * M + m) * 64 + n + 1 instead of the sum (exact in fp32 at the
// tested sizes), so the caller sees which element went to which address.  mn_count[(z * M + m) * 64 + n] += 1 per store the epilogue
// issues; conflicts[0] / [1] = extra LDS cycles of one wave's combine stores / of the epilogue's combine reads, [2] / [3] = of one wave's
// A-panel stores / fragment reads (all three row groups); order[16] = the waves
// whose partials thread 0 of the first workgroup added, in the order it added them; returns the number of threads of that workgroup
// whose order differs from thread 0's, plus the number of poisoned (never written) panel slots any thread read.
extern "C" int m48_conv2_fwd(int B, const float* a1, const float* w2, float* a2, int ids, int* mn_count, int* conflicts, int* order) {
  using namespace m48;
  typedef Conv2Fwd P;
  constexpr int NW = 16, NT = NW * 64;
  std::vector<float> th0((size_t)OFF2 + NW2), th1((size_t)OFF2 + NW2);
  memcpy(th0.data() + OFF2, w2, (size_t)NW2 * sizeof(float));
  memcpy(th1.data() + OFF2, w2 + NW2, (size_t)NW2 * sizeof(float));
  StepArgs a; memset(&a, 0, sizeof a);
  a.B = B; a.nz = 2; a.theta[0] = th0.data(); a.theta[1] = th1.data();
  a.a1 = const_cast<float*>(a1); a.a2 = a2;
  const int M = P::M(a), N = P::N(a);
  const int gx = (M + TM - 1) / TM, gy = (N + TN - 1) / TN, gz = P::nbz(a);
  conflicts[0] = conflicts[1] = conflicts[2] = conflicts[3] = 0;
  const float POISON = -1e30f;
  std::vector<float> lds((size_t)LDS_FLOATS);              // the workgroup's LDS: combine panels first (smem), A panels by opnd_off
  float* const smem = lds.data();
  int addr[64], bad = 0;
  for (int bz = 0; bz < gz; ++bz) for (int by = 0; by < gy; ++by) for (int bx = 0; bx < gx; ++bx) {
    const bool first = bx == 0 && by == 0 && bz == 0;
    const int m0 = bx * TM, n0 = by * TN;
    int z, ks, kbeg, kend; P::ksplit(a, bz, z, ks, kbeg, kend);
    const float* bbase = P::b_ptr(a, z);
    std::vector<float> acc((size_t)NW * RG * CH * 64 * 4, 0.f);          // [wave][rg][h][lane][r]
    auto A = [&](size_t wave, int rg, int h, int l, int r) -> float& { return acc[((((wave * RG + rg) * CH + h) * 64) + l) * 4 + r]; };
    for (int wave = 0; wave < NW; ++wave)
      for (int kc = kbeg + wave * KC; kc < kend; kc += NW * KC) {
        // every lane's fragments, as the kernel gets them: B straight from memory, A one row group at a time through the wave's panel
        float fa[RG][STEPS][64], fb[CH][STEPS][64];
        for (int l = 0; l < 64; ++l) for (int t = 0; t < STEPS; ++t) {
          const int k = kc + kslot_step(t) + kslot_lane(l >> 4);
          for (int h = 0; h < CH; ++h) { const int n = n0 + frag_col(l, h); fb[h][t][l] = bbase[P::b_row(a, z, k) + P::b_col(a, z, n < N ? n : N - 1)]; }
        }
        float* pan = lds.data() + opnd_off(wave);
        for (int rg = 0; rg < RG; ++rg) {
          for (int i = 0; i < PANEL_A; ++i) pan[i] = POISON;               // a missed slot poisons the result
          for (int j = 0; j < 2; ++j) {
            f4 v[64];
            for (int l = 0; l < 64; ++l) { const int m = m0 + ld_row(l, rg, j); v[l] = P::a_load4(a, z, P::a_row(a, z, m < M ? m : M - 1) + P::a_col(a, z, kc + n16::ld_k(l))); }
            for (int e = 0; e < 4; ++e) {
              for (int l = 0; l < 64; ++l) { addr[l] = pan_off(n16::ld_k(l) + e, n16::ld_x(l, j)); pan[addr[l]] = e == 0 ? v[l].x : e == 1 ? v[l].y : e == 2 ? v[l].z : v[l].w; }
              if (first && wave == 0) conflicts[2] += conflict_cycles(addr);
            }
          }
          for (int t = 0; t < STEPS; ++t) {
            for (int l = 0; l < 64; ++l) { addr[l] = frag_a(l, t); fa[rg][t][l] = pan[addr[l]]; if (fa[rg][t][l] == POISON) ++bad; }
            if (first && wave == 0) conflicts[3] += conflict_cycles(addr);
          }
        }
        for (int rg = 0; rg < RG; ++rg) for (int t = 0; t < STEPS; ++t) for (int h = 0; h < CH; ++h)
          for (int l = 0; l < 64; ++l) for (int r = 0; r < 4; ++r) {
            const int i = 4 * (l >> 4) + r, jn = l & 15;
            float d = A(wave, rg, h, l, r);
            for (int s = 0; s < 4; ++s) d = fmaf(fa[rg][t][16 * s + i], fb[h][t][16 * s + jn], d);      // an fmaf chain in slot order
            A(wave, rg, h, l, r) = d;
          }
      }
    // the two-half combine: every thread's running sums and the waves it added, in order
    std::vector<float> v0(NT, 0.f), v1(NT, 0.f);
    std::vector<std::vector<int>> added(NT);
    for (int half = 0; half < 2; ++half) {
      int owner[HALF_WAVES];
      for (int i = 0; i < HALF_WAVES * PANEL_C; ++i) smem[i] = POISON;
      for (int wave = 0; wave < NW; ++wave) {
        if (comb_half(wave) != half) continue;
        float* cw = smem + (size_t)comb_panel(wave) * PANEL_C;
        owner[comb_panel(wave)] = wave;
        for (int rg = 0; rg < RG; ++rg) for (int h = 0; h < CH; ++h) for (int r = 0; r < 4; ++r) {
          for (int l = 0; l < 64; ++l) { addr[l] = comb_off(acc_row(rg, l, r), acc_col(h, l)); cw[addr[l]] = A(wave, rg, h, l, r); }
          if (first && wave == 0) conflicts[0] += conflict_cycles(addr);
        }
      }
      for (int w = 0; w < HALF_WAVES; ++w)
        for (int t0 = 0; t0 < NT; t0 += 64) {                            // the epilogue's threads, one wave of them at a time
          const bool two = t0 + NT < TM * TN;
          for (int e = 0; e < (two ? 2 : 1); ++e) {
            for (int l = 0; l < 64; ++l) addr[l] = comb_off(epi_row(t0 + l + e * NT), epi_col(t0 + l + e * NT));
            if (first && w == 0 && half == 0) conflicts[1] += conflict_cycles(addr);
            for (int l = 0; l < 64; ++l) {
              const float p = smem[(size_t)w * PANEL_C + addr[l]];
              if (p == POISON) ++bad;
              float& v = e ? v1[t0 + l] : v0[t0 + l];
              v = (half == 0 && w == 0) ? p : v + p;
              if (e == 0) added[t0 + l].push_back(owner[w]);
            }
          }
        }
    }
    if (first) {
      for (int i = 0; i < NW; ++i) order[i] = i < (int)added[0].size() ? added[0][i] : -1;
      for (int t = 1; t < NT; ++t) if (added[t] != added[0]) ++bad;
    }
    for (int t = 0; t < NT; ++t) for (int e = 0; e < 2; ++e) {
      const int el = t + e * NT;
      if (el >= TM * TN) continue;
      const int m = m0 + epi_row(el), n = n0 + epi_col(el);
      if (m >= M || n >= N) continue;
      float v = e ? v1[t] : v0[t];
      if (ids) v = (float)(((int64_t)z * M + m) * K2 + n + 1);
      mn_count[((int64_t)z * M + m) * K2 + n] += 1;
      P::store(a, z, ks, m, n, v);
    }
  }
  return bad;
}

// The 32 x 32 body's sum of the same product on the same model (gemm_engine.h: gemm_tile): wave w's partial is the fmaf chain over
// k = 32 w + 8 (t >> 2) + 4 h + (t & 3), t = 0..15, h = 0, 1 (v_mfma_f32_32x32x2_f32: two k-slots per step), the 16 partials are added in
// wave order, then Rectlin.  out[(z * M + m) * 64 + n]
extern "C" void n32_conv2_fwd_ref(int B, const float* a1, const float* w2, float* out) {
  typedef Conv2Fwd P;
  StepArgs a; memset(&a, 0, sizeof a);
  a.B = B; a.nz = 2;
  const int M = P::M(a);
  for (int z = 0; z < 2; ++z) for (int m = 0; m < M; ++m) for (int n = 0; n < K2; ++n) {
    const int arow = P::a_row(a, z, m);
    float v = 0.f;
    for (int w = 0; w < 16; ++w) {
      float p = 0.f;
      for (int t = 0; t < 16; ++t) for (int h = 0; h < 2; ++h) {
        const int k = 32 * w + 8 * (t >> 2) + 4 * h + (t & 3);
        p = fmaf(a1[arow + P::a_col(a, z, k)], w2[(size_t)wslot(z) * NW2 + (size_t)k * K2 + n], p);
      }
      v = w == 0 ? p : v + p;
    }
    out[((size_t)z * M + m) * K2 + n] = fmaxf(v, 0.0f);
  }
}

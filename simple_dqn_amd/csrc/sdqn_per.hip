// sdqn_per.hip — prioritized experience replay (Schaul et al. 2016, proportional variant).
//
// A prioritized replay handle owns, in HBM: raw priorities (float32), leaves = raw x valid (float32) and a 64-ary sum-tree over the
// leaves with fp64 internal sums.  An index is valid exactly when replay_memory.py:54-68 would accept it, so the sampler never rejects.
// Internal nodes are always recomputed from their 64 children by one wavefront (a fixed butterfly order), never updated by deltas.
//
// Launches:
//   per_step_kernel    ONE workgroup: [refresh rewritten slot ranges] -> [write back the last step's priorities + recompute their
//                      ancestors, level by level] -> [stratified sample of the next batch, IS weights, (a, r, t) gather].  It takes the
//                      place of prep_kernel in front of a train_many call and runs once after every PER step.
//   per_leaves_kernel  grid: raw = p_max over a rewritten range and/or leaf = raw x valid over a slot range (full rebuilds)
//   per_level_kernel   grid: recompute every node of one level (full rebuilds; one launch per level)
#include "api_internal.h"

namespace sdqn {

__device__ inline bool per_valid(const PerRing& r, int64_t i) {
  const int n = r.ns.n > 1 ? r.ns.n : 1;                                  // --n_step: window [i - hist, i + n - 1] (sampler.h)
  if (i < r.hist || i > r.count - n) return false;                        // randint(hist, count - n), :59
  if (i + n - 1 >= r.current && i - r.hist < r.current) return false;     // :61
  for (int64_t k = i - r.hist; k < i; ++k) if (r.meta[k].terminal) return false;   // :65
  return true;
}
__device__ inline double per_entry(const PerTree& t, int L, int64_t k) {          // entry k of level L, 0 beyond its end
  if (k >= t.n[L]) return 0.0;
  return L == 0 ? (double)t.leaf[k] : t.lvl[L][k];
}
// the sum of 64 entries in one fixed order: lane i after the butterfly holds ((x_i + x_i^32) + ...) — the same value on every lane
// (fp addition commutes), numpy: while len(x) > 1: x = x[:len/2] + x[len/2:]
__device__ inline double per_fold(double x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}
__device__ inline void per_recompute(const PerTree& t, int L, int64_t j, int lane) {   // whole wavefront; L >= 1
  const double s = per_fold(per_entry(t, L - 1, j * PER_FAN + lane));
  if (lane == 0) t.lvl[L][j] = s;
}
// descent: the leaf whose prefix interval contains x.  At every level the children are scanned in order with an fp64 running prefix
// (numpy: np.cumsum); the first child with c > 0 and x < prefix + c is taken and x becomes x - prefix.  When rounding leaves x at the
// right edge, the last non-zero child is taken: a zero-priority leaf is never returned.
__device__ inline int64_t per_descend(const PerTree& t, double x) {
  int L = t.nlev - 1;
  int64_t base = 0, cnt = t.n[L];
  for (;;) {
    int64_t chosen = -1, last_nz = -1; double prefix = 0.0, last_pre = 0.0;
    for (int64_t k0 = 0; k0 < cnt && chosen < 0; k0 += 16) {
      double c[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {                                      // 16 loads in flight, then the scan
        const int64_t k = base + (k0 + q < cnt ? k0 + q : cnt - 1);
        const double v = L == 0 ? (double)t.leaf[k] : t.lvl[L][k];
        c[q] = k0 + q < cnt ? v : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        if (chosen >= 0) break;
        if (c[q] > 0.0) {
          if (x < prefix + c[q]) { chosen = base + k0 + q; x -= prefix; break; }
          last_nz = base + k0 + q; last_pre = prefix;
        }
        prefix += c[q];
      }
    }
    if (chosen < 0) { chosen = last_nz; x -= last_pre; }
    if (L == 0 || chosen < 0) return chosen;
    base = chosen * PER_FAN; --L;
    cnt = t.n[L] - base < PER_FAN ? t.n[L] - base : PER_FAN;
  }
}
__device__ inline void per_flag(const PerTree& t, int code) {
  __hip_atomic_store(t.err, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <int CAP>
__global__ void __launch_bounds__(256) per_step_kernel(const PerStepArgsU<CAP> a) {
  const PerStepArgs& p = a.p;
  const PerTree& t = p.t;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ int64_t sh_idx[PER_MAX_B];
  __shared__ float sh_p[PER_MAX_B];
  __shared__ float sh_red[4];
  __shared__ double sh_S;
  if (p.zero8 && tid == 0) *p.zero8 = 0.0;                    // the cost accumulator of a train_many call (prep_kernel's job)
  // ---- 1. slots (re)written since the last sampling launch: raw = p_max, then validity of [first - back, end + hist) re-evaluated, where
  // back = n - 1 (--n_step: a write moves `current`, which decides the validity of indexes whose window ends up to n - 1 slots later)
  if (p.nseg > 0) {
    const int back = p.ring.ns.n > 1 ? p.ring.ns.n - 1 : 0;
    const float pm = *t.pmax;
    for (int s = 0; s < p.nseg; ++s)
      for (int64_t i = p.seg[s].first + tid; i < p.seg[s].end; i += 256) t.raw[i] = pm;
    __syncthreads();
    for (int s = 0; s < p.nseg; ++s) {
      const int64_t span = p.seg[s].end - p.seg[s].first + p.ring.hist + back;
      for (int64_t k = tid; k < span; k += 256) {
        int64_t i = p.seg[s].first - back + k; if (i < 0) i += t.size; if (i >= t.size) i -= t.size;
        t.leaf[i] = per_valid(p.ring, i) ? t.raw[i] : 0.0f;
      }
    }
    __syncthreads();
    for (int L = 1; L < t.nlev; ++L) {
      const int sh = 6 * L;
      for (int s = 0; s < p.nseg; ++s) {
        const int64_t f = p.seg[s].first - back, last = p.seg[s].end + p.ring.hist - 1;
        const int64_t lo0 = f < 0 ? 0 : f, hi0 = last < t.size ? last : t.size - 1;
        for (int64_t j = (lo0 >> sh) + wave; j <= (hi0 >> sh); j += 4) per_recompute(t, L, j, lane);
        if (last >= t.size)
          for (int64_t j = wave; j <= ((last - t.size) >> sh); j += 4) per_recompute(t, L, j, lane);
        if (f < 0)                                                 // (the widened window wrapped below slot 0: its tail at the ring's end)
          for (int64_t j = ((f + t.size) >> sh) + wave; j <= ((t.size - 1) >> sh); j += 4) per_recompute(t, L, j, lane);
      }
      __syncthreads();
    }
  }
  // ---- 2. write-back of the last step: leaf = (|delta| + eps)^alpha x valid, the last occurrence of an index in batch order wins
  if (p.wb_B > 0) {
    for (int n = tid; n < p.wb_B; n += 256) { sh_idx[n] = p.wb_idx[n]; sh_p[n] = p.wb_p[n]; }
    __syncthreads();
    float mx = 0.0f;
    for (int n = tid; n < p.wb_B; n += 256) {
      const int64_t i = sh_idx[n]; const float v = sh_p[n];
      if (!(v >= 0.0f && v <= 3.0e38f)) { per_flag(t, 2); continue; }    // non-finite (or negative) priority: refused, tree untouched
      bool later = false;
      for (int m = n + 1; m < p.wb_B; ++m) later |= sh_idx[m] == i;
      if (!later) { t.raw[i] = v; t.leaf[i] = per_valid(p.ring, i) ? v : 0.0f; }
      mx = fmaxf(mx, v);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) sh_red[wave] = mx;
    __syncthreads();
    if (tid == 0) *t.pmax = fmaxf(fmaxf(*t.pmax, fmaxf(sh_red[0], sh_red[1])), fmaxf(sh_red[2], sh_red[3]));
    for (int L = 1; L < t.nlev; ++L) {                        // ancestors, level by level (a node two samples share is written twice, same value)
      for (int n0 = wave; n0 < p.wb_B; n0 += 4 * 8) {        // 8 nodes per wave with their children's loads in flight together
        double x[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int n = n0 + 4 * q;
          x[q] = n < p.wb_B ? per_entry(t, L - 1, (sh_idx[n] >> (6 * L)) * PER_FAN + lane) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int n = n0 + 4 * q;
          const double s = per_fold(x[q]);
          if (n < p.wb_B && lane == 0) t.lvl[L][sh_idx[n] >> (6 * L)] = s;
        }
      }
      __syncthreads();
    }
  }
  if (p.mode == 0) return;
  // ---- 3. the next batch: stratified by priority (t_n = (n + u_n) S / B) or the given indexes; weights (p_n / min_m p_m)^-beta
  __syncthreads();
  if (p.mode == 1) {
    if (wave == 0) { const double s = per_fold(per_entry(t, t.nlev - 1, lane)); if (lane == 0) sh_S = s; }
    __syncthreads();
    const double S = sh_S;
    for (int n = tid; n < p.B; n += 256) {
      int64_t i = -1;
      if (S > 0.0) i = per_descend(t, ((double)n + a.u[n]) * S / (double)p.B);
      if (i < 0) { per_flag(t, 3); i = p.ring.hist; }        // nothing valid to sample (memory safety; reported by the host)
      sh_idx[n] = i; sh_p[n] = t.leaf[i];
    }
  } else {
    for (int n = tid; n < p.B; n += 256) { const int64_t i = a.gidx[n]; sh_idx[n] = i; sh_p[n] = t.raw[i]; }
  }
  __syncthreads();
  float mn = 3.4e38f;
  for (int n = tid; n < p.B; n += 256) mn = fminf(mn, sh_p[n]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mn = fminf(mn, __shfl_xor(mn, off, 64));
  if (lane == 0) sh_red[wave] = mn;
  __syncthreads();
  const double pmin = (double)fminf(fminf(sh_red[0], sh_red[1]), fminf(sh_red[2], sh_red[3]));
  for (int n = tid; n < p.B; n += 256) {
    const int64_t i = sh_idx[n];
    const float w = pmin > 0.0 ? (float)pow((double)sh_p[n] / pmin, -p.beta) : 1.0f;
    p.sidx[n] = i; p.w[n] = w;
    if (p.idx_out) p.idx_out[n] = i;
    if (p.actions) {
      stage_meta(p.ring.meta, i, p.ring.ns, p.actions, p.rewards, p.terminals, n);
      if (p.ring.meta[i].action >= p.A) per_flag(t, 1);       // check_ring_actions, on the device
    }
  }
}

__global__ void __launch_bounds__(256) per_leaves_kernel(const PerTree t, const PerRing r, int64_t lo, int64_t hi, int64_t rw_end) {
  const float pm = *t.pmax;
  for (int64_t i = lo + (int64_t)blockIdx.x * 256 + threadIdx.x; i < hi; i += (int64_t)gridDim.x * 256) {
    float v = t.raw[i];
    if (i < rw_end) { v = pm; t.raw[i] = v; }
    t.leaf[i] = per_valid(r, i) ? v : 0.0f;
  }
}
__global__ void __launch_bounds__(256) per_level_kernel(const PerTree t, int L) {
  const int lane = threadIdx.x & 63;
  for (int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < t.n[L]; j += (int64_t)gridDim.x * 4) per_recompute(t, L, j, lane);
}

hipError_t per_launch_step(const PerStepArgs& p, const double* u_or_gidx, hipStream_t s) {
  const int n = p.mode ? p.B : 0;
  if (n > PER_MAX_B || p.wb_B > PER_MAX_B) return hipErrorInvalidValue;
  if (n <= 32) {
    PerStepArgsU<32> a; memset(&a, 0, sizeof a); a.p = p;
    if (n) memcpy(a.u, u_or_gidx, (size_t)n * 8);
    SDQN_LAUNCH(per_step_kernel<32>, dim3(1), dim3(256), 0, s, a);
  } else {
    PerStepArgsU<PER_MAX_B> a; memset(&a, 0, sizeof a); a.p = p;
    memcpy(a.u, u_or_gidx, (size_t)n * 8);
    SDQN_LAUNCH(per_step_kernel<PER_MAX_B>, dim3(1), dim3(256), 0, s, a);
  }
  return hipGetLastError();
}
hipError_t per_launch_leaves(const PerTree& t, const PerRing& r, int64_t lo, int64_t hi, int64_t rw_end, hipStream_t s) {
  if (hi <= lo) return hipSuccess;
  int64_t blocks = (hi - lo + 255) / 256; if (blocks > 2048) blocks = 2048;
  SDQN_LAUNCH(per_leaves_kernel, dim3((unsigned)blocks), dim3(256), 0, s, t, r, lo, hi, rw_end);
  return hipGetLastError();
}
hipError_t per_launch_level(const PerTree& t, int L, hipStream_t s) {
  int64_t blocks = (t.n[L] + 3) / 4; if (blocks > 2048) blocks = 2048;
  SDQN_LAUNCH(per_level_kernel, dim3((unsigned)blocks), dim3(256), 0, s, t, L);
  return hipGetLastError();
}
hipError_t per_launch_levels(const PerTree& t, hipStream_t s) {
  for (int L = 1; L < t.nlev; ++L) { hipError_t e = per_launch_level(t, L, s); if (e != hipSuccess) return e; }
  return hipSuccess;
}

}  // namespace sdqn

// ---- host side -------------------------------------------------------------------------------------------------------------

static PerRing per_ring(sdqn_replay_s* r) { PerRing g; g.meta = r->d_meta; g.count = r->count; g.current = r->current; g.hist = r->hist; g.ns = r->ns; return g; }

int per_free(PerState* p) {
  if (!p) return SDQN_OK;
  hipFree(p->t.raw); hipFree(p->t.leaf); hipFree(p->t.pmax); hipFree(p->newp); hipFree(p->sidx); hipFree(p->w);
  for (int L = 1; L < PER_MAX_LEVELS; ++L) hipFree(p->t.lvl[L]);
  hipHostFree(p->t.err);
  delete p;
  return SDQN_OK;
}
// slots [first, first + n) of the ring were (re)written: kept as a sorted list of disjoint ranges
void per_mark(sdqn_replay_s* r, int64_t first, int64_t n) {
  PerState* p = r->per;
  if (!p || n <= 0) return;
  int64_t f = first, e = first + n;
  std::vector<PerSeg> out;
  for (const PerSeg& s : p->rw) {
    if (s.end < f || s.first > e) out.push_back(s);
    else { f = s.first < f ? s.first : f; e = s.end > e ? s.end : e; }
  }
  PerSeg ns; ns.first = f; ns.end = e;
  size_t k = 0; while (k < out.size() && out[k].first < f) ++k;
  out.insert(out.begin() + k, ns);
  p->rw.swap(out);
}
void per_mark_all(sdqn_replay_s* r) { if (r->per) r->per->full = true; }

// the arguments every per_step launch of this handle shares, without the pending ring changes
static void per_base(sdqn_replay_s* r, PerStepArgs& a) {
  PerState* p = r->per;
  memset(&a, 0, sizeof a);
  a.t = p->t; a.ring = per_ring(r); a.beta = p->beta; a.sidx = p->sidx; a.w = p->w; a.A = 256; a.B = r->B;
}
// ... and with them: they go into the launch built from `a`, or are applied now by grid launches (counted in h's profile, if given)
#define PER_LAUNCH(expr) do { if (h) LAUNCH(K_PREP, (expr)); else HIPCHK(expr); } while (0)
static int per_begin(sdqn_replay_s* r, PerStepArgs& a, sdqn_net_s* h = nullptr) {
  PerState* p = r->per;
  per_base(r, a);
  int64_t span = 0;
  for (const PerSeg& s : p->rw) span += s.end - s.first + r->hist + (r->ns.n > 1 ? r->ns.n - 1 : 0);
  const bool big = p->full || (int)p->rw.size() > PER_SEGS || span > PER_SEG_SPAN || span > r->size;
  if (big) {
    for (const PerSeg& s : p->rw) PER_LAUNCH(per_launch_leaves(p->t, a.ring, s.first, s.end, s.end, g_stream));
    PER_LAUNCH(per_launch_leaves(p->t, a.ring, 0, r->size, 0, g_stream));
    for (int L = 1; L < p->t.nlev; ++L) PER_LAUNCH(per_launch_level(p->t, L, g_stream));
  } else {
    a.nseg = (int)p->rw.size();
    for (int i = 0; i < a.nseg; ++i) a.seg[i] = p->rw[i];
  }
  p->rw.clear(); p->full = false;
  return SDQN_OK;
}
// CPython random.random(): two 32-bit words, (a >> 5, b >> 6) -> 53 bits
static void per_draw(uint32_t* mt, int B, double* u) {
  MT g(mt);
  for (int n = 0; n < B; ++n) {
    const uint32_t x = g.genrand() >> 5, y = g.genrand() >> 6;
    u[n] = ((double)x * 67108864.0 + (double)y) * (1.0 / 9007199254740992.0);
  }
}
// after a synchronisation: the device's error word (sticky until reported)
int per_check(sdqn_replay_s* r) {
  if (!r->per) return SDQN_OK;
  volatile int* e = r->per->t.err;
  const int code = *e;
  if (!code) return SDQN_OK;
  *e = 0;
  if (code == 1) { set_error("prioritized replay: a sampled ring slot holds an action the network has no output for"); return SDQN_ERR_ARG; }
  if (code == 2) { set_error("prioritized replay: a non-finite TD error (priority) was refused"); return SDQN_ERR_ARG; }
  set_error("prioritized replay: no valid index to sample (count %lld, history %d)", (long long)r->count, r->hist);
  return SDQN_ERR_ARG;
}
static int per_sync_check(sdqn_replay_s* r) { HIPCHK(hipStreamSynchronize(g_stream)); return per_check(r); }
// apply pending ring changes without sampling (get / set / last_sample)
static int per_flush(sdqn_replay_s* r) {
  PerStepArgs a; int rc = per_begin(r, a); if (rc) return rc;
  if (a.nseg) { a.mode = 0; HIPCHK(per_launch_step(a, nullptr, g_stream)); }
  return SDQN_OK;
}

extern "C" int sdqn_replay_enable_priorities(sdqn_replay_t r, double alpha, double epsilon) {
  ARGCHK(r, "NULL handle");
  ARGCHK(!(r->flags & SDQN_REPLAY_ZERO_COPY), "prioritized replay needs the HBM mirror (SDQN_REPLAY_HBM_MIRROR)");
  ARGCHK(!r->lanes, "a laned replay memory (sdqn_replay_set_lanes) cannot be prioritized: the sum-tree refresh takes 4 slot ranges per launch, a lockstep writes one per lane");
  ARGCHK(alpha >= 0.0 && alpha <= 1e6, "priority alpha %g must be >= 0", alpha);
  ARGCHK(epsilon > 0.0 && epsilon <= 1e30, "priority epsilon %g must be > 0", epsilon);
  ARGCHK(r->B <= PER_MAX_B, "prioritized replay supports batch sizes up to %d (got %d)", PER_MAX_B, r->B);
  STREAMCHK();
  if (!r->per) {
    PerState* p = new PerState();
    memset(&p->t, 0, sizeof p->t);
    p->t.size = r->size;
    int64_t n = r->size; int L = 0;
    p->t.n[0] = n;
    while (n > PER_FAN) { n = (n + PER_FAN - 1) / PER_FAN; ++L; ARGCHK(L < PER_MAX_LEVELS, "ring too large for the sum-tree"); p->t.n[L] = n; }
    p->t.nlev = L + 1;
#define PCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_error("%s -> %s", #x, hipGetErrorString(e_)); per_free(p); return SDQN_ERR_HIP; } } while (0)
    PCHK(hipMalloc((void**)&p->t.raw, (size_t)r->size * 4));
    PCHK(hipMalloc((void**)&p->t.leaf, (size_t)r->size * 4));
    for (int l = 1; l < p->t.nlev; ++l) PCHK(hipMalloc((void**)&p->t.lvl[l], (size_t)p->t.n[l] * 8));
    PCHK(hipMalloc((void**)&p->t.pmax, 4));
    PCHK(hipMalloc((void**)&p->newp, (size_t)r->B * 4));
    PCHK(hipMalloc((void**)&p->sidx, (size_t)r->B * 8));
    PCHK(hipMalloc((void**)&p->w, (size_t)r->B * 4));
    PCHK(hipHostMalloc((void**)&p->t.err, 4, hipHostMallocMapped | hipHostMallocPortable));
#undef PCHK
    *p->t.err = 0;
    r->per = p;
  }
  PerState* p = r->per;
  p->alpha = alpha; p->eps = epsilon;
  std::vector<float> ones((size_t)r->size, 1.0f);                      // every priority (and p_max) back to 1.0
  HIPCHK(hipMemcpyAsync(p->t.raw, ones.data(), (size_t)r->size * 4, hipMemcpyHostToDevice, g_stream));
  HIPCHK(hipMemcpyAsync(p->t.pmax, ones.data(), 4, hipMemcpyHostToDevice, g_stream));
  HIPCHK(hipMemsetAsync(p->sidx, 0, (size_t)r->B * 8, g_stream));
  HIPCHK(hipMemsetAsync(p->w, 0, (size_t)r->B * 4, g_stream));
  p->rw.clear(); p->full = true; p->sample_live = p->gathered = false;
  HIPCHK(hipStreamSynchronize(g_stream));                             // (the staging vector dies here)
  return SDQN_OK;
}
extern "C" int sdqn_replay_set_priority_beta(sdqn_replay_t r, double beta) {
  ARGCHK(r, "NULL handle");
  ARGCHK(r->per, "the replay memory is not prioritized (sdqn_replay_enable_priorities)");
  ARGCHK(beta >= 0.0 && beta <= 1.0, "priority beta %g outside [0, 1]", beta);
  r->per->beta = beta;
  return SDQN_OK;
}
extern "C" int sdqn_replay_set_priorities(sdqn_replay_t r, int64_t first, int64_t n, const float* values) {
  ARGCHK(r && (values || n == 0), "NULL argument");
  ARGCHK(r->per, "the replay memory is not prioritized (sdqn_replay_enable_priorities)");
  ARGCHK(first >= 0 && n >= 0 && first + n <= r->size, "bad priority range");
  float mx = 0.0f;
  for (int64_t i = 0; i < n; ++i) {
    ARGCHK(values[i] > 0.0f && values[i] <= 3.0e38f, "priority %g at slot %lld must be finite and > 0", (double)values[i], (long long)(first + i));
    mx = values[i] > mx ? values[i] : mx;
  }
  if (n == 0) return SDQN_OK;
  int rc = per_flush(r); if (rc) return rc;                            // pending (re)writes first: they would overwrite these values
  PerState* p = r->per;
  float pm = 0.0f;
  HIPCHK(hipMemcpyAsync(&pm, p->t.pmax, 4, hipMemcpyDeviceToHost, g_stream));
  HIPCHK(hipStreamSynchronize(g_stream));
  pm = mx > pm ? mx : pm;
  HIPCHK(hipMemcpyAsync(p->t.raw + first, values, (size_t)n * 4, hipMemcpyHostToDevice, g_stream));
  HIPCHK(hipMemcpyAsync(p->t.pmax, &pm, 4, hipMemcpyHostToDevice, g_stream));
  const PerRing g = per_ring(r);
  HIPCHK(per_launch_leaves(p->t, g, first, first + n, 0, g_stream));
  HIPCHK(per_launch_levels(p->t, g_stream));
  HIPCHK(hipStreamSynchronize(g_stream));                              // (values and pm are borrowed)
  p->sample_live = p->gathered = false;
  return SDQN_OK;
}
extern "C" int sdqn_replay_get_priorities(sdqn_replay_t r, int64_t first, int64_t n, float* out) {
  ARGCHK(r && (out || n == 0), "NULL argument");
  ARGCHK(r->per, "the replay memory is not prioritized (sdqn_replay_enable_priorities)");
  ARGCHK(first >= 0 && n >= 0 && first + n <= r->size, "bad priority range");
  int rc = per_flush(r); if (rc) return rc;
  if (n) HIPCHK(hipMemcpyAsync(out, r->per->t.leaf + first, (size_t)n * 4, hipMemcpyDeviceToHost, g_stream));
  return per_sync_check(r);
}
extern "C" int sdqn_replay_get_max_priority(sdqn_replay_t r, float* out) {
  ARGCHK(r && out, "NULL argument");
  ARGCHK(r->per, "the replay memory is not prioritized (sdqn_replay_enable_priorities)");
  HIPCHK(hipMemcpyAsync(out, r->per->t.pmax, 4, hipMemcpyDeviceToHost, g_stream));
  return per_sync_check(r);
}
extern "C" int sdqn_replay_last_sample(sdqn_replay_t r, int64_t* idx_out, float* w_out) {
  ARGCHK(r, "NULL handle");
  ARGCHK(r->per, "the replay memory is not prioritized (sdqn_replay_enable_priorities)");
  if (idx_out) HIPCHK(hipMemcpyAsync(idx_out, r->per->sidx, (size_t)r->B * 8, hipMemcpyDeviceToHost, g_stream));
  if (w_out) HIPCHK(hipMemcpyAsync(w_out, r->per->w, (size_t)r->B * 4, hipMemcpyDeviceToHost, g_stream));
  return per_sync_check(r);
}

// sdqn_replay_sample on a prioritized handle: refresh, sample, weights; indexes to the host
int per_sample_host(sdqn_replay_s* r, uint32_t* mt, int64_t* idx_out, int64_t* draws_out) {
  ARGCHK(mt && idx_out, "NULL argument");
  ARGCHK(r->count >= r->hist + r->ns.n, "replay memory holds %lld screens: at least history_length + n_step = %d needed", (long long)r->count, r->hist + r->ns.n);
  PerStepArgs a; int rc = per_begin(r, a); if (rc) return rc;
  std::vector<double> u((size_t)r->B); per_draw(mt, r->B, u.data());
  a.mode = 1;
  HIPCHK(per_launch_step(a, u.data(), g_stream));
  HIPCHK(hipMemcpyAsync(idx_out, r->per->sidx, (size_t)r->B * 8, hipMemcpyDeviceToHost, g_stream));
  rc = per_sync_check(r); if (rc) return rc;
  r->per->h_sidx.assign(idx_out, idx_out + r->B); r->per->sample_live = true; r->per->gathered = false;
  if (draws_out) *draws_out = r->B;
  return SDQN_OK;
}

// ---- the train step with priorities ------------------------------------------------------------------------------------------------
// Tuned 84 x 84 x 4 path: the head's PER form reads the weights and writes the new priorities, conv1 reads the device-sampled indexes
// from HBM.  Generic path (float64, other geometries; generic_net.hip): the same per_step launches, the gather of the sampled indexes,
// then the generic step with its head in the weighted form (GenericNet::set_per).
static HeadArgs per_head(sdqn_net_s* h, PerState* p) {
  HeadArgs hd = head_args(h, HEAD_TRAIN);
  hd.per_w = p->w; hd.per_p = p->newp; hd.per_alpha = p->alpha; hd.per_eps = p->eps;
  return hd;
}
static PerStepArgs per_writeback(PerStepArgs a, PerState* p) {
  a.nseg = 0; a.zero8 = nullptr; a.mode = 0; a.wb_B = a.B; a.wb_idx = p->sidx; a.wb_p = p->newp;
  return a;
}
// the step's (a, r, t) destination: the tuned step's staging, or the generic path's gathered minibatch (the gather writes the same values)
static void per_targets(sdqn_net_s* h, sdqn_replay_s* r, PerStepArgs& a) {
  a.A = h->A;
  if (h->gen) { a.idx_out = nullptr; a.actions = r->d_act; a.rewards = r->d_rew; a.terminals = r->d_term; }
  else { a.idx_out = h->d_idx; a.actions = h->st_act; a.rewards = h->st_rew; a.terminals = h->st_term; }
}
// generic path: gather the sampled minibatch and run one weighted step on it
static int per_gen_step(sdqn_net_s* h, sdqn_replay_s* r) {
  PerState* p = r->per;
  int rc = replay_gather_generic(r, p->sidx); if (rc) return rc;
  if (h->shift_P > 0) { rc = shift_minibatch(h, r, p->sidx); if (rc) return rc; }      // --random_shift: the states again, shifted; (a, r, t) stay
  h->gen->set_per(p->w, p->newp, p->alpha, p->eps);
  const hipError_t e = h->gen->train_dev(r->d_pre, r->d_post, r->d_act, r->d_rew, r->d_term, h->epoch);
  h->gen->set_per(nullptr, nullptr, 0.0, 0.0);
  GENCHK(e);
  return gen_step_done(h);
}
// one step on the minibatch the last sampling launch left (host_idx: run_ring_step)
static int per_train_step(sdqn_net_s* h, sdqn_replay_s* r, const int64_t* host_idx) {
  return h->gen ? per_gen_step(h, r) : run_ring_step(h, r, host_idx, per_head(h, r->per));
}
// (sdqn_net_train_many / sdqn_net_train_replay have checked batch size, n-step settings and geometry; the former has cleared the cost sum)
// n steps: [refresh + sample 0] | step 0 | [write-back 0 + sample 1] | step 1 | ... | step n-1 | [write-back n-1]
int per_train_many(sdqn_net_s* h, sdqn_replay_s* r, uint32_t* mt, int n_steps, float* mean_cost) {
  PerState* p = r->per;
  if (n_steps > 0) {
    ARGCHK(r->count >= r->hist + r->ns.n, "replay memory holds %lld screens: at least history_length + n_step = %d needed", (long long)r->count, r->hist + r->ns.n);
    std::vector<double> u((size_t)r->B);
    PerStepArgs a; int rc = per_begin(r, a, h); if (rc) return rc;
    per_targets(h, r, a);
    PerStepArgs s0 = a; s0.mode = 1; s0.zero8 = h->gen ? nullptr : h->cost_accum;
    per_draw(mt, r->B, u.data());
    LAUNCH(K_PREP, per_launch_step(s0, u.data(), g_stream));
    for (int i = 0; i < n_steps; ++i) {
      rc = per_train_step(h, r, nullptr); if (rc) return rc;
      PerStepArgs wb = per_writeback(a, p);
      if (i + 1 < n_steps) { wb.mode = 1; per_draw(mt, r->B, u.data()); }
      LAUNCH(K_PREP, per_launch_step(wb, u.data(), g_stream));
    }
    p->sample_live = p->gathered = false;
  }
  return mean_cost ? read_mean_cost(h, n_steps, mean_cost) : SDQN_OK;
}
// given indexes (sdqn_net_train_replay): weights from their raw priorities, then the step, then the write-back
int per_train_replay(sdqn_net_s* h, sdqn_replay_s* r, const int64_t* idx_host, float* cost_out) {
  int rc = check_ring_actions(h, r, idx_host); if (rc) return rc;
  for (int i = 0; i < r->B; ++i)
    ARGCHK(idx_host[i] >= r->hist && idx_host[i] + r->ns.n - 1 < r->count, "index %lld out of range (count %lld, n_step %d)", (long long)idx_host[i], (long long)r->count, r->ns.n);
  PerState* p = r->per;
  PerStepArgs a; rc = per_begin(r, a, h); if (rc) return rc;
  per_targets(h, r, a);
  PerStepArgs s0 = a; s0.mode = 2;
  LAUNCH(K_PREP, per_launch_step(s0, reinterpret_cast<const double*>(idx_host), g_stream));
  rc = per_train_step(h, r, idx_host); if (rc) return rc;
  LAUNCH(K_PREP, per_launch_step(per_writeback(a, p), nullptr, g_stream));
  p->sample_live = p->gathered = false;
  if (cost_out) { rc = read_cost(h, cost_out); if (rc) return rc; }
  return per_sync_check(r);
}
// sdqn_net_train_host on the memory's own device minibatch, gathered from its last prioritized sample: the weights of that sample.  The
// write-back leaves ring changes made since the sample pending (an add between getMinibatch() and train()): the next sampling launch
// applies them after it, so a slot rewritten in between ends at p_max and the validity of its window is re-evaluated.
bool per_owns_minibatch(sdqn_replay_s* r) { return r && r->per && r->per->gathered; }
static int per_host_writeback(sdqn_net_s* h, sdqn_replay_s* r) {
  PerState* p = r->per;
  PerStepArgs b; per_base(r, b);
  LAUNCH(K_PREP, per_launch_step(per_writeback(b, p), nullptr, g_stream));
  p->sample_live = p->gathered = false;
  return SDQN_OK;
}
int per_train_host_step(sdqn_net_s* h, sdqn_replay_s* r, const StepArgs& a, HeadArgs hd) {
  PerState* p = r->per;
  HeadArgs ph = per_head(h, p);
  ph.st_actions = hd.st_actions; ph.st_rewards = hd.st_rewards; ph.st_terminals = hd.st_terminals;
  int rc = run_train(h, a, ph, nullptr); if (rc) return rc;
  return per_host_writeback(h, r);
}
// generic path: the caller runs the step between these two
void per_gen_arm(sdqn_net_s* h, sdqn_replay_s* r) { PerState* p = r->per; h->gen->set_per(p->w, p->newp, p->alpha, p->eps); }
int per_gen_finish(sdqn_net_s* h, sdqn_replay_s* r) { h->gen->set_per(nullptr, nullptr, 0.0, 0.0); return per_host_writeback(h, r); }
// net-level synchronising calls (sdqn_net_sync, read_cost, sdqn_net_cost_collect): the device flags of every prioritized memory
int per_check_all() {
  for (sdqn_replay_s* r : g_replays) { int rc = per_check(r); if (rc) return rc; }
  return SDQN_OK;
}
// sdqn_replay_gather: is this the last prioritized sample?
void per_note_gather(sdqn_replay_s* r, const int64_t* idx) {
  if (!r->per) return;
  PerState* p = r->per;
  p->gathered = p->sample_live && p->h_sidx.size() == (size_t)r->B && !memcmp(p->h_sidx.data(), idx, (size_t)r->B * 8);
}

// sdqn_per.h — prioritized experience replay (Schaul et al. 2016, proportional variant) on the device: the priority arrays and
// the 64-ary sum-tree a replay handle owns, and the launches that keep it, sample from it and write priorities back (sdqn_per.hip).
// DESIGN.md §16.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "problems.h"

namespace sdqn {

constexpr int PER_FAN = 64;            // children per node: one wavefront folds a node with one load per lane
constexpr int PER_MAX_LEVELS = 8;      // leaves + internal levels (64^7 slots)
constexpr int PER_MAX_B = 256;         // batch sizes the sampling launch carries its uniform draws for (kernel arguments)
constexpr int PER_SEGS = 4;            // rewritten slot ranges a sampling launch refreshes itself (more: the grid rebuild)
constexpr int PER_SEG_SPAN = 8192;     // ... and their total length

// device view of the tree.  Level 0 = the leaves (float32, raw x valid), level l >= 1 = fp64 sums of PER_FAN children of level l - 1,
// ALWAYS recomputed from the children (never updated by deltas): after any update the tree equals a fresh build.  The top level has
// at most PER_FAN entries; S = their fold.
struct PerTree {
  float* raw;                  // [size] raw priorities (|delta| + eps)^alpha, or p_max for (re)written slots
  float* leaf;                 // [size] raw x valid (replay_memory.py:54-68's acceptance rule); level 0 of the tree
  double* lvl[PER_MAX_LEVELS]; // lvl[l], l >= 1: [n[l]] node sums (lvl[0] unused)
  int64_t n[PER_MAX_LEVELS];   // entries per level (n[0] = size)
  int nlev;                    // levels including the leaves; top = nlev - 1
  float* pmax;                 // [1] largest leaf value ever written
  int* err;                    // [1] mapped host word: 1 = action out of range, 2 = non-finite priority, 3 = no valid index (sticky)
  int64_t size;
};

struct PerRing {               // what the validity rule reads
  const MetaRec* meta;
  int64_t count, current;
  int hist;
  NStepArgs ns;                // --n_step: ns.n > 1 widens the rule to the window [i - hist, i + n - 1]; the gather's returns
};

struct PerSeg { int64_t first, end; };       // slots [first, end) were (re)written: raw = p_max, validity of [first - n + 1, end + hist) re-evaluated

struct PerStepArgs {
  PerTree t; PerRing ring;
  int nseg; PerSeg seg[PER_SEGS];
  // write-back of the last step: wb_idx[n] gets wb_p[n] (last occurrence in batch order wins)
  int wb_B; const int64_t* wb_idx; const float* wb_p;
  // sample: mode 1 stratified by priority (u[n] = the draws), 2 the given indexes (gidx); 0 none
  int mode, B, A; double beta;
  int64_t* idx_out;            // [B] the net's device index array (nullable)
  int64_t* sidx;               // [B] the handle's last sample
  float* w;                    // [B] importance weights
  uint8_t* actions; int64_t* rewards; uint8_t* terminals;   // (a, r, t)[idx] (nullable: no metadata gather)
  double* zero8;               // nullable: an 8-byte accumulator this launch clears (the first launch of a train_many call)
};
template <int CAP> struct PerStepArgsU { PerStepArgs p; union { double u[CAP]; int64_t gidx[CAP]; }; };

hipError_t per_launch_step(const PerStepArgs& p, const double* u_or_gidx, hipStream_t s);
hipError_t per_launch_leaves(const PerTree& t, const PerRing& r, int64_t lo, int64_t hi, int64_t rw_end, hipStream_t s);
hipError_t per_launch_level(const PerTree& t, int L, hipStream_t s);
hipError_t per_launch_levels(const PerTree& t, hipStream_t s);

}  // namespace sdqn

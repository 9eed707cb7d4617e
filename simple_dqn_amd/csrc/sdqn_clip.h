// sdqn_clip.h — global gradient-norm clipping, --clip_grad_norm (kernels in sdqn_clip.hip).  Two launches between the
// reduction of the flat gradient sums g (update mode 1) and their application (update mode 2):
//   grad_sqnorm : CLIP_GRID partial sums of g[i]^2 in fp64, one per workgroup, no atomics — grid and order are fixed: same bits every run
//   grad_scale  : every workgroup folds the partials in the same order, norm = sqrt(sum) / bsz, scale = min(1, G / (norm + 1e-6)) in fp64,
//                 rounded once to T; scale < 1: g[i] <- g[i] * scale in place (one rounded multiply); otherwise, or when the norm is not
//                 finite, g is not written.  Workgroup 0 leaves {norm, scale} in the 16-byte record.
// Plain HIP, no other project header: the tuned path (float) and generic_net.hip (float / double) both include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdqn {

constexpr int CLIP_GRID = 256;                   // workgroups of both launches: about one per CU
constexpr int CLIP_WORDS = CLIP_GRID + 2;        // doubles of a net's clip buffer: [CLIP_GRID] partials | norm | scale
constexpr double CLIP_EPS = 1e-6;

// g: n values, 16-byte aligned; part: [CLIP_GRID]; rec: {norm, scale as applied (the rounded T, widened)}
template <typename T> hipError_t launch_grad_sqnorm(const T* g, int64_t n, double* part, hipStream_t s);
template <typename T> hipError_t launch_grad_scale(T* g, int64_t n, const double* part, double bsz, double max_norm, double* rec, hipStream_t s);

}  // namespace sdqn

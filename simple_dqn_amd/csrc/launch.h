// launch.h — the one way step kernels are launched.  Normally a plain launch; when the host orchestration has armed a
// pair of events (sdqn_net_profile), the launch hands them to hipExtLaunchKernel, which stores the DISPATCH PACKET's own
// begin / end timestamps in them — the same two timestamps `rocprofv3 --kernel-trace` reports for the launch, with no
// marker packets added to the queue (an hipEventRecord pair around a launch adds ~2.6 us of packet processing to what it
// measures and perturbs the dependent chain it sits in).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

namespace sdqn {
struct LaunchEvents { hipEvent_t start = nullptr, stop = nullptr; bool used = false; };
LaunchEvents& launch_events();             // thread-local (sdqn_kernels.hip); armed by api_internal.h's LAUNCH_ON for ONE launch
}

#ifdef SDQN_LAUNCH_TRACE
// Trace build (tools/route_trace.cpp; never part of the library): a launch becomes one record naming the kernel instantiation — the enclosing
// launcher's signature with its template arguments, the kernel expression, the launch dimensions and a hash of every argument's bytes — so
// two trees' launch decisions can be compared on the host, without a device.
namespace sdqn { namespace trace {
void emit(const char* launcher, const char* kernel, dim3 grid, dim3 block, unsigned long long arg_hash);      // defined by the trace program
inline unsigned long long hash_args(unsigned long long h) { return h; }
template <class T, class... R>
inline unsigned long long hash_args(unsigned long long h, const T& v, const R&... rest) {      // FNV-1a over the object representation
  const unsigned char* p = reinterpret_cast<const unsigned char*>(&v);
  for (size_t i = 0; i < sizeof(T); ++i) h = (h ^ p[i]) * 1099511628211ull;
  return hash_args(h, rest...);
}
} }
#define SDQN_LAUNCH(kernel, grid, block, shmem, stream, ...) \
  sdqn::trace::emit(__PRETTY_FUNCTION__, #kernel, (grid), (block), sdqn::trace::hash_args(14695981039346656037ull, __VA_ARGS__))
#else
#define SDQN_LAUNCH(kernel, grid, block, shmem, stream, ...) do { \
  sdqn::LaunchEvents& le__ = sdqn::launch_events(); \
  if (le__.start) { \
    hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, le__.start, le__.stop, 0, __VA_ARGS__); \
    le__.start = le__.stop = nullptr; le__.used = true; \
  } else hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__); \
} while (0)
#endif

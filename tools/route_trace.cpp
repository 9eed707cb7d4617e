// route_trace — which kernel instantiation launch_kernel picks for every (id, key, options) of a grid, printed one record per call, on the
// host and without a device.  Links the five kernel translation units built with -DSDQN_LAUNCH_TRACE (launch.h: a launch becomes a record
// instead of a launch).  Two trees route alike iff their outputs are equal: the acceptance check of a refactoring of the dispatch, and the
// way to see what an option does before running it.  Build and use: tools/route_trace.sh.
//   route_trace            the whole grid (default options, then one option off its default at a time)
//   route_trace --default  the default-options grid only
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../simple_dqn_amd/csrc/kernels.h"

using namespace sdqn;

// what the kernel TUs' host code expects of the HIP runtime, answered here: the program links no runtime library and reaches no device
// (the code-object registration of a host-only build has nothing to register; a real launch in a trace build is a bug)
extern "C" {
hipError_t hipGetLastError() { return hipSuccess; }
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
hipError_t __hipPushCallConfiguration(dim3, dim3, size_t, hipStream_t) { fprintf(stderr, "route_trace: a launch outside SDQN_LAUNCH\n"); abort(); }
hipError_t __hipPopCallConfiguration(dim3*, dim3*, size_t*, hipStream_t*) { abort(); }
hipError_t hipLaunchKernel(const void*, dim3, dim3, void**, size_t, hipStream_t) { abort(); }
}
namespace sdqn {
namespace trace {
static std::string g_rec;
void emit(const char* launcher, const char* kernel, dim3 grid, dim3 block, unsigned long long h) {
  char buf[160];
  snprintf(buf, sizeof buf, " g=%u,%u,%u b=%u,%u,%u args=%016llx", grid.x, grid.y, grid.z, block.x, block.y, block.z, h);
  g_rec += " | "; g_rec += launcher; g_rec += " | "; g_rec += kernel; g_rec += buf;
}
} }

static const int IDS[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16, 17, 18, 24};
static const int BS[] = {1, 32, 33, 47, 48, 64, 127, 128, 160, 204, 205, 208, 256, 257, 512};
static int64_t g_host_idx[32];

template <class T> static T* dummy(int n) { return reinterpret_cast<T*>((uintptr_t)0x10000000u * (unsigned)n); }      // distinct, non-null, never dereferenced

static StepArgs base_args() {
  StepArgs a; memset(&a, 0, sizeof a);
  int n = 1;
  a.src = dummy<const uint8_t>(n++); a.idx = dummy<const int64_t>(n++); a.theta[0] = dummy<const float>(n++); a.theta[1] = dummy<const float>(n++);
  a.a1 = dummy<float>(n++); a.a2 = dummy<float>(n++); a.a3 = dummy<float>(n++); a.slab4 = dummy<float>(n++); a.a4 = dummy<float>(n++); a.d4 = dummy<float>(n++);
  a.d3p = dummy<float>(n++); a.d2p = dummy<float>(n++); a.d3 = dummy<float>(n++); a.d2 = dummy<float>(n++); a.d1 = dummy<float>(n++); a.g = dummy<float>(n++);
  a.slab1 = dummy<float>(n++); a.slab2 = dummy<float>(n++); a.slab3 = dummy<float>(n++);
  a.h_a1 = dummy<half_t>(n++); a.h_a2 = dummy<half_t>(n++); a.h_a3 = dummy<half_t>(n++); a.h_d4 = dummy<half_t>(n++); a.h_d3p = dummy<half_t>(n++);
  a.h_d3 = dummy<half_t>(n++); a.h_d2p = dummy<half_t>(n++); a.h_d2 = dummy<half_t>(n++); a.h_d1 = dummy<half_t>(n++);
  a.wh[0] = dummy<const half_t>(n++); a.wh[1] = dummy<const half_t>(n++); a.wht[0] = dummy<const half_t>(n++); a.wht[1] = dummy<const half_t>(n++);
  a.wh_w = dummy<half_t>(n++); a.wht_w = dummy<half_t>(n++); a.theta_w = dummy<float>(n++); a.state = dummy<float>(n++);
  a.w1p[0] = dummy<const unsigned short>(n++); a.w1p[1] = dummy<const unsigned short>(n++);
  a.A = 4; a.S4 = 7; a.tps1 = 5; a.tps2 = 9; a.tps3 = 7; a.fuse_rms = 1; a.loss_scale = 128.0f; a.inv_loss_scale = 1.0f / 128.0f;
  a.post_off = 1; a.arg_preload = 1; a.bsz = 32.0f; a.rho = 0.95f; a.one_minus_rho = 0.05f; a.lr = 0.00025f; a.eps = 1e-6f;
  return a;
}

// a call's frames reuse whatever earlier calls left on the stack, and launchers leave struct padding unwritten: start every call from zeroes
static __attribute__((noinline)) void scrub_stack() {
  volatile unsigned char pad[1 << 16];
  for (size_t i = 0; i < sizeof pad; ++i) pad[i] = 0;
}

static void one(const char* dev, int id, const StepArgs& a, const LaunchTune& t) {
  trace::g_rec.clear();
  scrub_stack();
  const hipError_t e = launch_kernel(id, a, t, nullptr);
  printf("%s id=%d B=%d h16=%d bn=%d nz=%d f4w=%d ring=%d hidx=%d :%s%s\n", dev, id, a.B, a.h16, a.bn, a.nz, a.f4w_count > 0, a.from_ring, t.host_idx != nullptr,
         e == hipSuccess ? (trace::g_rec.empty() ? " NONE" : "") : (e == hipErrorInvalidValue ? " INVALID" : " ERROR"), trace::g_rec.c_str());
}

// the default-options cross product; `patch` applies the deviation under test, `want(id)` thins the ids to those the deviation can reach
template <class Patch, class Want>
static void grid(const char* dev, Patch patch, Want want) {
  for (int dt = 0; dt < 4; ++dt)            // float32, float32 + batch_norm, h16 = 1, h16 = 2
    for (int B : BS) for (int nz = 1; nz <= 3; ++nz) for (int f4w = 0; f4w < 2; ++f4w) for (int ring = 0; ring < 2; ++ring) for (int hidx = 0; hidx < 2; ++hidx) {
      StepArgs a = base_args();
      a.B = B; a.nz = nz; a.bn = dt == 1; a.h16 = dt >= 2 ? dt - 1 : 0; a.f4w_first = 0; a.f4w_count = f4w ? (NIN4 / 32) * (NFC / 32) : 0; a.from_ring = ring;
      LaunchTune t; memset(&t, 0, sizeof t);
      t.host_idx = hidx ? g_host_idx : nullptr;
      patch(a, t);
      for (int id : IDS) if (want(id)) one(dev, id, a, t);
    }
}
// ids whose route reads bt / nw of id j: j itself and the members of its chain (conv1..3 forward, the two dgrads, bwd1 / wgrads)
static bool reaches(int j, int id) {
  auto group = [](int i) { return i <= 2 ? 1 : (i == K_CONV3_DGRAD || i == K_CONV2_DGRAD) ? 2 : (i == K_BWD1 || i == K_WGRADS) ? 3 : 0; };
  return id == j || (group(j) && group(j) == group(id));
}

int main(int argc, char** argv) {
  for (int i = 0; i < 32; ++i) g_host_idx[i] = 1000 + 37 * i;
  char dev[64];
  auto all = [](int) { return true; };
  grid("default", [](StepArgs&, LaunchTune&) {}, all);
  if (argc > 1 && !strcmp(argv[1], "--default")) return 0;
  for (int v : {-1, 1, 2, 3, 6, 7, 8}) {
    for (int j : IDS) { snprintf(dev, sizeof dev, "bt[%d]=%d", j, v); grid(dev, [=](StepArgs&, LaunchTune& t) { t.bt[j] = v; }, [=](int id) { return reaches(j, id); }); }
    snprintf(dev, sizeof dev, "bt[*]=%d", v); grid(dev, [=](StepArgs&, LaunchTune& t) { for (int& b : t.bt) b = v; }, all);     // (-1: option bt = 0 turns every entry off)
  }
  for (int v : {1, 2, 4, 8, 9, 16})
    for (int j = 0; j < 12; ++j) { snprintf(dev, sizeof dev, "nw[%d]=%d", j, v); grid(dev, [=](StepArgs&, LaunchTune& t) { t.nw_override[j] = v; }, [=](int id) { return reaches(j, id); }); }
  for (int v : {511, 1, 2, 4, 8, 16, 32, 64, 128, 256}) { snprintf(dev, sizeof dev, "wt=%d", v); grid(dev, [=](StepArgs&, LaunchTune& t) { t.wt = v; }, all); }
  for (int v : {(int)LV_CONV3_C36, (int)LV_CONV1_FWD_BF16, (int)LV_CONV1_WGRAD_BF16, (int)LV_C1W_IN_WGRADS, (int)LV_C1W_FIRST, LV_C1W_IN_WGRADS | LV_C1W_FIRST}) {
    snprintf(dev, sizeof dev, "variant=%d", v); grid(dev, [=](StepArgs&, LaunchTune& t) { t.variant = v; }, all);
  }
  for (int v : {4, 7, 10}) { snprintf(dev, sizeof dev, "tps1=%d", v); grid(dev, [=](StepArgs& a, LaunchTune&) { a.tps1 = v; }, [](int id) { return id == K_CONV1_WGRAD || id == K_BWD1 || id == K_WGRADS; }); }
  // operands a route asks for: no state source (conv1 cannot ride in the float16 chain), conv1's bf16 planes missing
  grid("src=0", [](StepArgs& a, LaunchTune&) { a.src = nullptr; }, [](int id) { return id <= 2; });
  grid("variant=4,w1p[1]=0", [](StepArgs& a, LaunchTune& t) { t.variant = LV_CONV1_FWD_BF16; a.w1p[1] = nullptr; }, [](int id) { return id == K_CONV1_FWD; });
  grid("variant=4,w1p=0", [](StepArgs& a, LaunchTune& t) { t.variant = LV_CONV1_FWD_BF16; a.w1p[0] = a.w1p[1] = nullptr; }, [](int id) { return id == K_CONV1_FWD; });
  // write-through and a variant together (bwd1's write-through form steps aside for the bf16 kernel)
  grid("wt=511,variant=8", [](StepArgs&, LaunchTune& t) { t.wt = 511; t.variant = LV_CONV1_WGRAD_BF16; }, [](int id) { return id == K_CONV1_WGRAD || id == K_BWD1; });
  grid("wt=511,variant=2", [](StepArgs&, LaunchTune& t) { t.wt = 511; t.variant = LV_CONV3_C36; }, [](int id) { return id == K_CONV3_FWD; });
  return 0;
}

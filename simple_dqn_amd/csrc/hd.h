// hd.h — the one qualifier of a function that is compiled for the host and for the device from the same text (plain `inline` when no
// device compiler reads the header: tests/emul and the tools run that text on the CPU).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDQN_HD __host__ __device__ inline
#else
#define SDQN_HD inline
#endif

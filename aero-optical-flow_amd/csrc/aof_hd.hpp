// The qualifiers of what is written once and runs on both sides.  AOF_HD_INLINE: a rule (aof_imu_step.hpp,
// aof_mavlink_rx_step.hpp, aof_exposure_step.hpp, aof_mavlink.hpp): inlined into a kernel under hipcc, a plain inline
// function for a host compiler.  AOF_HD: the form without the inlining, for members of the argument structs.
#pragma once

#include "aof.h"

#if defined(__HIPCC__)
#define AOF_HD __host__ __device__
#else
#define AOF_HD
#endif

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AOF_HD_INLINE __host__ __device__ __forceinline__
#else
#define AOF_HD_INLINE inline
#endif

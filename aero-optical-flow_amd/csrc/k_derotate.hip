// Gyro de-rotation of a batch of flow records (include/aof.h).  The arithmetic of one
// record is derotate_flow (aof_derotate.hpp), which the stream bank's tail lane runs as well.
#include "aof_derotate.hpp"
#include "aof_engine_args.hpp"

namespace aof {

namespace {

__global__ __launch_bounds__(256) void k_derotate(aof_derotate_params p, const aof_flow *flows,
                                                  const aof_gyro *gyro, int64_t n, float *out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const aof_flow f = flows[i];
    const aof_gyro g = gyro[i];
    float x, y;
    derotate_flow(p, f, g, &x, &y);
    out[2 * i + 0] = x;
    out[2 * i + 1] = y;
}

}  // namespace

int launch_derotate(const aof_derotate_params &p, const aof_flow *flows, const aof_gyro *gyro, int64_t n,
                    float *out, void *stream)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_derotate, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), p, flows, gyro, n, out);
    return (int)hipGetLastError();
}

}  // namespace aof

// conv_stats.hip — k_conv_stats: the instance-norm statistics of the maps a convolution of csrc/conv_tile.hpp wrote, from
// the per-tile partials of tile_store_stats.  One thread per (map, frame, channel) adds its tiles' partials in tile order and
// stores mean and rstd as floats (tile_order_stats).  A launch of its own for the stem (one map, 64 channels) and the trunk
// (a block's maps): at 192 x 256 a frame has 384 tiles, and every workgroup re-reducing them would read more than it stages.
#include "conv_tile.hpp"

namespace bt {

// part [maps][F][tiles][C][2]; mean, rstd [maps][F][C]; thread i is (map, frame, channel) i
__global__ __launch_bounds__(64) void k_conv_stats(const double *__restrict__ part, int tiles, int C, long long count, double n,
                                                   float *__restrict__ mean, float *__restrict__ rstd) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const long long mf = i / C;
    const int c = (int)(i - mf * C);
    float m, r;
    tile_order_stats(part + (mf * tiles * C + c) * 2, (long long)C * 2, tiles, n, m, r);
    mean[i] = m;
    rstd[i] = r;
}

bool conv_stats_launch(hipStream_t st, const double *part, long long tiles, long long C, long long count, long long n, float *mean, float *rstd) {
    hipLaunchKernelGGL(k_conv_stats, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, st, part, (int)tiles, (int)C, count, (double)n, mean, rstd);
    return hipGetLastError() == hipSuccess;
}

}  // namespace bt

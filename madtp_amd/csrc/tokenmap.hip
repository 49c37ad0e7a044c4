// Token maps on the device (csrc/madtp_tokenmap.h): the five kernels.  Everything the lanes do is in tokenmap_device.h, which the
// host emulation (madtp_tokenmap_*_host) runs as well; this file checks the arguments and launches.
//
// Visibility.  Lanes of a workgroup hand data to each other through LDS only, with a barrier between the write and the read
// (sync_lanes).  The build kernel reads back from global memory only what the SAME lane wrote (the previous layer's row of the map
// and depth: program order of one thread).  No workgroup waits for another, there are no atomics, and every loop is bounded by a
// launch argument or a checked table value: identical calls give identical bits.
#include "common.h"

#include "tokenmap_device.h"

namespace {

using namespace madtp_tokenmap;

__global__ __launch_bounds__(kLanes) void tokenmap_build_kernel(const int64_t* __restrict__ table, int L, int n0, int32_t* slot, float* coef,
                                                                int32_t* depth, int32_t* __restrict__ status) {
    __shared__ BuildShared sh;
    build_sample(sh, table, L, n0, (int)blockIdx.x, slot, coef, depth, status);
}

template <int V>
__global__ __launch_bounds__(kLanes) void tokenmap_push_kernel(const float* __restrict__ x, int64_t x_sb, int64_t x_sp,
                                                               const int32_t* __restrict__ slot, const float* __restrict__ coef,
                                                               int64_t map_sb, float* __restrict__ y, int n0, int n_out, int C) {
    __shared__ PushShared sh;
    push_sample<V>(sh, x, x_sb, x_sp, slot, coef, map_sb, y, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y, n0, n_out, C);
}

template <int V>
__global__ __launch_bounds__(kLanes) void tokenmap_pull_kernel(const float* __restrict__ v, const int32_t* __restrict__ slot,
                                                               const float* __restrict__ coef, int64_t map_sb, float* __restrict__ out,
                                                               int n0, int n_l, int C, bool weighted) {
    pull_cell<V>(v, slot, coef, map_sb, out, (int)blockIdx.y, (int64_t)blockIdx.x * kLanes + threadIdx.x, n0, n_l, C, weighted);
}

__global__ __launch_bounds__(kLanes) void tokenmap_agree_kernel(const int32_t* __restrict__ depth_a, const int32_t* __restrict__ depth_b,
                                                                int32_t* __restrict__ out, int n0, int L) {
    __shared__ AgreeShared sh;
    agree_sample(sh, depth_a, depth_b, out, (int)blockIdx.x, n0, L);
}

__global__ __launch_bounds__(kLanes) void tokenmap_shade_kernel(const uint8_t* __restrict__ images, const int32_t* __restrict__ depth,
                                                                const uint8_t* __restrict__ level, uint8_t* __restrict__ out, int gh,
                                                                int gw, int ph, int pw, int L) {
    shade_group(images, depth, level, out, (int)blockIdx.y, (int64_t)blockIdx.x * kLanes + threadIdx.x, gh, gw, ph, pw, L);
}

}  // namespace

extern "C" int madtp_tokenmap_abi_version(void) { return MADTP_TOKENMAP_ABI_VERSION; }

extern "C" const char* madtp_tokenmap_strerror(int code) {
    const char* s = madtp_tokenmap::strerror_tokenmap(code);
    return s ? s : madtp_strerror(code);
}

extern "C" int madtp_tokenmap_build(const int64_t* table, int L, int B, int n0, int32_t* slot, float* coef, int32_t* depth,
                                    int32_t* status, void* stream) {
    if (int rc = build_args(table, L, B, n0, slot, coef, depth, status)) return rc;
    hipLaunchKernelGGL(tokenmap_build_kernel, dim3(B), dim3(kLanes), 0, (hipStream_t)stream, table, L, n0, slot, coef, depth, status);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" int madtp_tokenmap_push(const float* x, int64_t x_sb, int64_t x_sp, const int32_t* slot, const float* coef, int64_t map_sb,
                                   float* y, int B, int n0, int n_out, int C, void* stream) {
    if (int rc = push_args(x, x_sb, x_sp, slot, coef, map_sb, y, B, n0, n_out, C)) return rc;
    if (push_vec4(x, x_sb, x_sp, y, C))
        hipLaunchKernelGGL(tokenmap_push_kernel<4>, dim3(B, push_groups(n_out, C, 4)), dim3(kLanes), 0, (hipStream_t)stream, x, x_sb, x_sp,
                           slot, coef, map_sb, y, n0, n_out, C);
    else
        hipLaunchKernelGGL(tokenmap_push_kernel<1>, dim3(B, push_groups(n_out, C, 1)), dim3(kLanes), 0, (hipStream_t)stream, x, x_sb, x_sp,
                           slot, coef, map_sb, y, n0, n_out, C);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" int madtp_tokenmap_pull(const float* v, const int32_t* slot, const float* coef, int64_t map_sb, float* out, int B, int n0,
                                   int n_l, int C, int weighted, void* stream) {
    if (int rc = pull_args(v, slot, coef, map_sb, out, B, n0, n_l, C, weighted)) return rc;
    const bool v4 = pull_vec4(v, out, C);
    const int64_t cells = (int64_t)n0 * (v4 ? C / 4 : C);
    const dim3 grid((unsigned)((cells + kLanes - 1) / kLanes), B);
    if (v4)
        hipLaunchKernelGGL(tokenmap_pull_kernel<4>, grid, dim3(kLanes), 0, (hipStream_t)stream, v, slot, coef, map_sb, out, n0, n_l, C, weighted != 0);
    else
        hipLaunchKernelGGL(tokenmap_pull_kernel<1>, grid, dim3(kLanes), 0, (hipStream_t)stream, v, slot, coef, map_sb, out, n0, n_l, C, weighted != 0);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" int madtp_tokenmap_agree(const int32_t* depth_a, const int32_t* depth_b, int32_t* out, int B, int n0, int L, void* stream) {
    if (int rc = agree_args(depth_a, depth_b, out, B, n0, L)) return rc;
    hipLaunchKernelGGL(tokenmap_agree_kernel, dim3(B), dim3(kLanes), 0, (hipStream_t)stream, depth_a, depth_b, out, n0, L);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" int madtp_tokenmap_shade(const void* images, const int32_t* depth, const void* level, void* out, int B, int gh, int gw, int ph,
                                    int pw, int L, void* stream) {
    if (int rc = shade_args(images, depth, level, out, B, gh, gw, ph, pw, L)) return rc;
    const int64_t groups = (int64_t)gh * ph * gw * pw * 3 / 16;
    hipLaunchKernelGGL(tokenmap_shade_kernel, dim3((unsigned)((groups + kLanes - 1) / kLanes), B), dim3(kLanes), 0, (hipStream_t)stream,
                       (const uint8_t*)images, depth, (const uint8_t*)level, (uint8_t*)out, gh, gw, ph, pw, L);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" int madtp_tokenmap_build_host(const int64_t* table, int L, int B, int n0, int32_t* slot, float* coef, int32_t* depth,
                                         int32_t* status) {
    return madtp_tokenmap::build_host(table, L, B, n0, slot, coef, depth, status);
}

extern "C" int madtp_tokenmap_push_host(const float* x, int64_t x_sb, int64_t x_sp, const int32_t* slot, const float* coef, int64_t map_sb,
                                        float* y, int B, int n0, int n_out, int C) {
    return madtp_tokenmap::push_host(x, x_sb, x_sp, slot, coef, map_sb, y, B, n0, n_out, C);
}

extern "C" int madtp_tokenmap_pull_host(const float* v, const int32_t* slot, const float* coef, int64_t map_sb, float* out, int B, int n0,
                                        int n_l, int C, int weighted) {
    return madtp_tokenmap::pull_host(v, slot, coef, map_sb, out, B, n0, n_l, C, weighted);
}

extern "C" int madtp_tokenmap_agree_host(const int32_t* depth_a, const int32_t* depth_b, int32_t* out, int B, int n0, int L) {
    return madtp_tokenmap::agree_host(depth_a, depth_b, out, B, n0, L);
}

extern "C" int madtp_tokenmap_shade_host(const void* images, const int32_t* depth, const void* level, void* out, int B, int gh, int gw,
                                         int ph, int pw, int L) {
    return madtp_tokenmap::shade_host(images, depth, level, out, B, gh, gw, ph, pw, L);
}

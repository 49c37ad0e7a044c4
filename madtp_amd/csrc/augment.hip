// The training transform of the data loader (include/madtp_augment.h): the resize tile of image.hip stored as bytes, then per
// RandAugment stage a histogram pass (Equalize, AutoContrast) and an apply pass (copy, byte table, fixed-point affine warp) over
// uint8 planes [B,3,Sh,Sw]; the last apply writes f32 through the 3 x 256 normalisation table.  Every image has its own op per
// stage (one plan row each), so a batch is at most 1 + 2 N launches.  Fixed grids; the only atomics are integer LDS atomics of
// the histogram; doubles are evaluated operation by operation: identical calls give identical bits.
#include "image_device.h"

#include "../../include/madtp_augment.h"

namespace {

struct StoreBytes {
    uint8_t* __restrict__ out;
    __device__ __forceinline__ void prepare() const {}
    __device__ __forceinline__ void put(size_t index, size_t plane, int r, int g, int b) const {
        uint8_t* oy = out + index;  // 64 contiguous bytes per wave and plane
        oy[0] = (uint8_t)r;
        oy[plane] = (uint8_t)g;
        oy[2 * plane] = (uint8_t)b;
    }
};

__global__ __launch_bounds__(IMG_THREADS) void augment_resize_u8_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ table,
                                                                         uint8_t* __restrict__ out, int B, int Sh, int Sw) {
    image_resize_tile(src, table, B, Sh, Sw, StoreBytes{out});
}

constexpr int AUG_THREADS = 256;
constexpr int AUG_WAVES = AUG_THREADS / 64;
constexpr int AUG_PX = 4;  // consecutive pixels of a plane per thread: one dword of bytes in, one dword or one float4 out

// ---- stats: one workgroup per (image, channel) --------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void augment_stats_kernel(const uint8_t* __restrict__ in, const int64_t* __restrict__ plan,
                                                                     const double* __restrict__ scale255, uint8_t* __restrict__ lut_u8,
                                                                     int plane) {
    __shared__ unsigned part[AUG_WAVES][256];  // a histogram per wave: a flat image is 64-way contention, not 256-way
    __shared__ unsigned hist[256];
    const int c = blockIdx.x, b = blockIdx.y;
    const int op = (int)plan[(size_t)b * MADTP_AUGMENT_FIELDS + MADTP_AUGMENT_F_OP];
    if (op != MADTP_AUGMENT_OP_EQUALIZE && op != MADTP_AUGMENT_OP_AUTOCONTRAST) return;  // (uniform: before any barrier)
    const int tid = threadIdx.x;
    for (int w = 0; w < AUG_WAVES; ++w) part[w][tid] = 0;
    __syncthreads();
    unsigned* mine = part[tid / 64];
    const uint8_t* p = in + ((size_t)b * 3 + c) * plane;
    const int head = min(plane, (int)((4 - ((uintptr_t)p & 3)) & 3));  // bytes before the first aligned dword
    const int words = (plane - head) / 4;
    if (tid < head) atomicAdd(&mine[p[tid]], 1u);
    const uint32_t* pw = (const uint32_t*)(p + head);
    for (int i = tid; i < words; i += AUG_THREADS) {
        const uint32_t v = pw[i];
        atomicAdd(&mine[v & 255], 1u);
        atomicAdd(&mine[(v >> 8) & 255], 1u);
        atomicAdd(&mine[(v >> 16) & 255], 1u);
        atomicAdd(&mine[v >> 24], 1u);
    }
    const int tail = head + 4 * words + tid;  // at most three bytes
    if (tail < plane) atomicAdd(&mine[p[tail]], 1u);
    __syncthreads();
    unsigned sum = 0;
    for (int w = 0; w < AUG_WAVES; ++w) sum += part[w][tid];
    hist[tid] = sum;
    __syncthreads();
    // every thread walks the 256 bins (one LDS address per step for the whole wave: a broadcast): the first and last non-empty
    // bin, and the pixels below its own bin
    int lo = 256, hi = 0;
    unsigned below = 0;
    for (int i = 0; i < 256; ++i) {
        const unsigned h = hist[i];
        if (h) {
            lo = min(lo, i);
            hi = i;
        }
        if (i < tid) below += h;
    }
    int v = tid;
    if (op == MADTP_AUGMENT_OP_EQUALIZE) {
        const unsigned step = ((unsigned)plane - hist[hi]) / 255u;
        if (step) v = (int)min(255u, (step / 2 + below) / step);
    } else if (hi > lo) {
#pragma clang fp contract(off)
        const double scale = scale255[hi - lo];
        const double offset = (double)((256 - lo) & 255) * scale;
        double t = (double)tid * scale;
        t = t + offset;
        t = fmin(fmax(t, 0.0), 255.0);
        v = (int)t;
    }
    lut_u8[((size_t)b * 3 + c) * 256 + tid] = (uint8_t)v;
}

// ---- apply --------------------------------------------------------------------------------------------------------------------
// one source coordinate in 1/32 pixel: (rint((ay * y + ac) * 1024) + 16 + rint(ax * x * 1024)) >> 5.  A value beyond +-2^30 is
// far outside any image (sides stay below 2^24) and is clamped there, where all four taps are the fill.
__device__ __forceinline__ int warp_coord(double ax, double ay, double ac, int x, int y) {
#pragma clang fp contract(off)
    double t = ay * (double)y;
    t = t + ac;
    t = t * 1024.0;
    double u = ax * (double)x;
    u = u * 1024.0;
    const double lim = 35184372088832.0;  // 2^45
    t = fmin(fmax(__builtin_rint(t), -lim), lim);
    u = fmin(fmax(__builtin_rint(u), -lim), lim);
    const long long X = ((long long)t + 16 + (long long)u) >> 5;
    return (int)min(max(X, -(1LL << 30)), 1LL << 30);
}

__global__ __launch_bounds__(AUG_THREADS) void augment_apply_kernel(const uint8_t* __restrict__ in, const int64_t* __restrict__ plan,
                                                                     const uint8_t* __restrict__ lut_u8, const float* __restrict__ norm,
                                                                     void* __restrict__ out, int Sh, int Sw, int vec) {
    __shared__ uint8_t stab[3 * 256];
    __shared__ float snorm[3 * 256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t* row = plan + (size_t)b * MADTP_AUGMENT_FIELDS;
    const int op = (int)row[MADTP_AUGMENT_F_OP];
    if (op < 0 || op >= MADTP_AUGMENT_OPS) return;  // (uniform, as everything up to the barrier)
    const bool tabled = op == MADTP_AUGMENT_OP_TABLE || op == MADTP_AUGMENT_OP_EQUALIZE || op == MADTP_AUGMENT_OP_AUTOCONTRAST;
    if (op == MADTP_AUGMENT_OP_TABLE) {
        const uint8_t* t = (const uint8_t*)row[MADTP_AUGMENT_F_TABLE];
        if (!t) return;
        for (int i = tid; i < 3 * 256; i += AUG_THREADS) stab[i] = t[i & 255];
    } else if (tabled) {
        const uint8_t* t = lut_u8 + (size_t)b * 3 * 256;
        for (int i = tid; i < 3 * 256; i += AUG_THREADS) stab[i] = t[i];
    }
    if (norm)
        for (int i = tid; i < 3 * 256; i += AUG_THREADS) snorm[i] = norm[i];
    __syncthreads();

    const int plane = Sh * Sw;
    const int i0 = (blockIdx.x * AUG_THREADS + tid) * AUG_PX;
    if (i0 >= plane) return;
    const int n = min(AUG_PX, plane - i0);  // (AUG_PX whenever vec: the plane is then a multiple of it)
    const uint8_t* src = in + (size_t)b * 3 * plane;
    int v[3][AUG_PX];
    if (op == MADTP_AUGMENT_OP_WARP) {
        double a[6];
        for (int k = 0; k < 6; ++k) a[k] = __longlong_as_double(row[MADTP_AUGMENT_F_A0 + k]);
        int x = i0 % Sw, y = i0 / Sw;
        for (int j = 0; j < n; ++j) {
            const int X = warp_coord(a[0], a[1], a[2], x, y), Y = warp_coord(a[3], a[4], a[5], x, y);
            const int fx = X & 31, fy = Y & 31;
            const int sx = min(max(X >> 5, -2), Sw), sy = min(max(Y >> 5, -2), Sh);  // (-2 and the side: both taps outside, as beyond)
            const int w00 = 32 * (32 - fx) * (32 - fy), w01 = 32 * fx * (32 - fy), w10 = 32 * (32 - fx) * fy, w11 = 32 * fx * fy;
            const bool x0 = sx >= 0 && sx < Sw, x1 = sx + 1 >= 0 && sx + 1 < Sw, y0 = sy >= 0 && sy < Sh, y1 = sy + 1 >= 0 && sy + 1 < Sh;
            const int at = sy * Sw + sx;  // (read only where the tap is inside)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint8_t* p = src + (size_t)c * plane;
                const int p00 = y0 && x0 ? p[at] : MADTP_AUGMENT_FILL, p01 = y0 && x1 ? p[at + 1] : MADTP_AUGMENT_FILL;
                const int p10 = y1 && x0 ? p[at + Sw] : MADTP_AUGMENT_FILL, p11 = y1 && x1 ? p[at + Sw + 1] : MADTP_AUGMENT_FILL;
                v[c][j] = (w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 16384) >> 15;
            }
            if (++x == Sw) {
                x = 0;
                ++y;
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint8_t* p = src + (size_t)c * plane + i0;
            if (vec) {
                const uint32_t w = *(const uint32_t*)p;
#pragma unroll
                for (int j = 0; j < AUG_PX; ++j) v[c][j] = (w >> (8 * j)) & 255;
            } else {
#pragma unroll
                for (int j = 0; j < AUG_PX; ++j) v[c][j] = j < n ? p[j] : 0;
            }
            if (tabled) {
#pragma unroll
                for (int j = 0; j < AUG_PX; ++j) v[c][j] = stab[c * 256 + v[c][j]];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t o = ((size_t)b * 3 + c) * plane + i0;
        if (norm) {
            float* q = (float*)out + o;
            if (vec) {
                *(float4*)q = make_float4(snorm[c * 256 + v[c][0]], snorm[c * 256 + v[c][1]], snorm[c * 256 + v[c][2]], snorm[c * 256 + v[c][3]]);
            } else {
#pragma unroll
                for (int j = 0; j < AUG_PX; ++j)
                    if (j < n) q[j] = snorm[c * 256 + v[c][j]];
            }
        } else {
            uint8_t* q = (uint8_t*)out + o;
            if (vec) {
                *(uint32_t*)q = (uint32_t)v[c][0] | (uint32_t)v[c][1] << 8 | (uint32_t)v[c][2] << 16 | (uint32_t)v[c][3] << 24;
            } else {
#pragma unroll
                for (int j = 0; j < AUG_PX; ++j)
                    if (j < n) q[j] = (uint8_t)v[c][j];
            }
        }
    }
}

constexpr int AUG_STATS_MASK = 1 << MADTP_AUGMENT_OP_EQUALIZE | 1 << MADTP_AUGMENT_OP_AUTOCONTRAST;

int augment_args(const void* in, const int64_t* plan, const void* out, int B, int Sh, int Sw, int op_mask) {
    if (!in || !plan || !out || B < 1 || op_mask < 1 || op_mask >= 1 << MADTP_AUGMENT_OPS) return MADTP_E_BADARG;
    if (Sh < 1 || Sw < 1 || (int64_t)Sh * Sw >= MADTP_AUGMENT_MAX_PIXELS) return MADTP_E_SHAPE;
    return 0;
}

}  // namespace

extern "C" int madtp_augment_abi_version(void) { return MADTP_AUGMENT_ABI_VERSION; }

extern "C" int madtp_augment_resize_u8(const void* src, const int64_t* table, void* out_u8, int B, int Sh, int Sw, int n_blocks,
                                       int max_ksize, void* stream) {
    if (!src || !table || !out_u8 || B < 1 || n_blocks < 1) return MADTP_E_BADARG;
    if (Sh < 1 || Sw < 1 || max_ksize < 1 || max_ksize > MADTP_IMAGE_MAX_KSIZE) return MADTP_E_SHAPE;
    hipLaunchKernelGGL(augment_resize_u8_kernel, dim3(n_blocks), dim3(IMG_THREADS), 0, (hipStream_t)stream, (const uint8_t*)src, table,
                       (uint8_t*)out_u8, B, Sh, Sw);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" int madtp_augment_stats(const void* in, const int64_t* plan, const double* scale255, void* lut_u8, int B, int Sh, int Sw,
                                   int op_mask, void* stream) {
    if (!scale255) return MADTP_E_BADARG;
    const int bad = augment_args(in, plan, lut_u8, B, Sh, Sw, op_mask);
    if (bad) return bad;
    if (B > 65535) return MADTP_E_SHAPE;
    if (!(op_mask & AUG_STATS_MASK)) return 0;
    hipLaunchKernelGGL(augment_stats_kernel, dim3(3, B), dim3(AUG_THREADS), 0, (hipStream_t)stream, (const uint8_t*)in, plan, scale255,
                       (uint8_t*)lut_u8, Sh * Sw);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" int madtp_augment_apply(const void* in, const int64_t* plan, const void* lut_u8, const float* norm, void* out, int B, int Sh,
                                   int Sw, int op_mask, void* stream) {
    if (!lut_u8) return MADTP_E_BADARG;
    const int bad = augment_args(in, plan, out, B, Sh, Sw, op_mask);
    if (bad) return bad;
    if (B > 65535) return MADTP_E_SHAPE;
    const int plane = Sh * Sw;
    // dwords in, dwords or float4 out: when every plane starts at a multiple of four pixels from aligned bases
    const int vec = plane % AUG_PX == 0 && (uintptr_t)in % 4 == 0 && (uintptr_t)out % 16 == 0;
    const int per_block = AUG_THREADS * AUG_PX;
    hipLaunchKernelGGL(augment_apply_kernel, dim3((plane + per_block - 1) / per_block, B), dim3(AUG_THREADS), 0, (hipStream_t)stream,
                       (const uint8_t*)in, plan, (const uint8_t*)lut_u8, norm, out, Sh, Sw, vec);
    MADTP_LAUNCH_CHECK();
    return 0;
}

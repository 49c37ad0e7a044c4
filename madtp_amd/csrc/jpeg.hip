// The device stage of the JPEG decode (include/madtp_jpeg.h): coefficient blocks as the host's entropy decoder wrote them -> uint8
// sample planes (dequantise, libjpeg's jpeg_idct_islow, range limit) -> packed RGB [h, w, 3] (fancy chroma upsampling on the fly,
// fixed-point colour conversion), two launches for a batch of images of different sizes and subsamplings.  Everything is integer
// VALU work, so nothing can be contracted, and all of it is 32-bit two's complement that wraps (computed in uint32_t; only the
// arithmetic shifts are signed).  No atomics, fixed grids: identical calls give identical bits.
#include "common.h"

#include "jpeg_entropy.h"

namespace {

constexpr int JPEG_THREADS = 256;
constexpr int IDCT_BLOCKS = MADTP_JPEG_IDCT_BLOCKS;
constexpr int WS_ROW = 9, WS_BLOCK = 8 * WS_ROW;  // a padded 8x8 of int32 per block: lanes of a block read rows 9 words apart
static_assert(IDCT_BLOCKS * 8 == JPEG_THREADS, "eight lanes per block");
static_assert(MADTP_JPEG_RGB_PIXELS == 4 * JPEG_THREADS, "four pixels per lane");

struct Geometry {
    int w, h, components, hs, vs, bx, by;
    int64_t luma, chroma;  // blocks of the luma plane and of one chroma plane
    __device__ __forceinline__ bool read(const int64_t* t) {
        w = (int)t[MADTP_JPEG_F_W], h = (int)t[MADTP_JPEG_F_H], components = (int)t[MADTP_JPEG_F_COMPONENTS];
        hs = (int)t[MADTP_JPEG_F_HS], vs = (int)t[MADTP_JPEG_F_VS];
        bx = (int)t[MADTP_JPEG_F_BLOCKS_X], by = (int)t[MADTP_JPEG_F_BLOCKS_Y];
        if (w < 1 || w > MADTP_JPEG_MAX_SIDE || h < 1 || h > MADTP_JPEG_MAX_SIDE) return false;
        if (components != 1 && components != 3) return false;
        if (!((hs == 1 && vs == 1) || (components == 3 && hs == 2 && (vs == 1 || vs == 2)))) return false;
        if (bx < 1 || by < 1 || bx > MADTP_JPEG_MAX_SIDE / 8 + 1 || by > MADTP_JPEG_MAX_SIDE / 8 + 1) return false;
        if (bx % hs || by % vs || 8 * bx < w || 8 * by < h) return false;
        luma = (int64_t)bx * by;
        chroma = components == 3 ? luma / (hs * vs) : 0;
        return true;
    }
};

// the image a workgroup belongs to: last b with table[b][field] <= blockIdx.x (image_device.h's search)
__device__ __forceinline__ int find_image(const int64_t* __restrict__ table, int B, int field) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(size_t)mid * MADTP_JPEG_FIELDS + field] <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One pass of jpeg_idct_islow (jidctint.c) over eight values; SHIFT = 11 for the column pass, 18 for the row pass.
template <int SHIFT>
__device__ __forceinline__ void idct8(const uint32_t (&in)[8], int32_t (&out)[8]) {
    uint32_t z1, z2, z3, z4, z5, tmp0, tmp1, tmp2, tmp3;
    z2 = in[2], z3 = in[6];
    z1 = (z2 + z3) * 4433u;
    tmp2 = z1 - z3 * 15137u;
    tmp3 = z1 + z2 * 6270u;
    z2 = in[0], z3 = in[4];
    tmp0 = (z2 + z3) << 13;
    tmp1 = (z2 - z3) << 13;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7], tmp1 = in[5], tmp2 = in[3], tmp3 = in[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
    z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u, tmp1 *= 16819u, tmp2 *= 25172u, tmp3 *= 12299u;
    z1 = 0u - z1 * 7373u, z2 = 0u - z2 * 20995u, z3 = 0u - z3 * 16069u, z4 = 0u - z4 * 3196u;
    z3 += z5, z4 += z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    constexpr uint32_t half = 1u << (SHIFT - 1);
    out[0] = (int32_t)(tmp10 + tmp3 + half) >> SHIFT;
    out[7] = (int32_t)(tmp10 - tmp3 + half) >> SHIFT;
    out[1] = (int32_t)(tmp11 + tmp2 + half) >> SHIFT;
    out[6] = (int32_t)(tmp11 - tmp2 + half) >> SHIFT;
    out[2] = (int32_t)(tmp12 + tmp1 + half) >> SHIFT;
    out[5] = (int32_t)(tmp12 - tmp1 + half) >> SHIFT;
    out[3] = (int32_t)(tmp13 + tmp0 + half) >> SHIFT;
    out[4] = (int32_t)(tmp13 - tmp0 + half) >> SHIFT;
}

// libjpeg's range-limit table read at x & 1023: the wrap into -512 .. 511, the level shift, the clamp
__device__ __forceinline__ uint32_t range_limit(int32_t x) {
    const int v = (int)(((uint32_t)x + 512u) & 1023u) - 512 + 128;
    return (uint32_t)min(max(v, 0), 255);
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_idct_kernel(const uint8_t* __restrict__ coef, const uint8_t* __restrict__ qtables,
                                                                 const int64_t* __restrict__ table, uint8_t* __restrict__ planes, int B) {
    __shared__ int32_t ws[IDCT_BLOCKS * WS_BLOCK];
    const int64_t* t = table + (size_t)find_image(table, B, MADTP_JPEG_F_FIRST_IDCT) * MADTP_JPEG_FIELDS;
    const int64_t local = (int64_t)blockIdx.x - t[MADTP_JPEG_F_FIRST_IDCT];
    Geometry g;
    if (!g.read(t) || local < 0) return;  // (uniform: before the barrier)
    const int64_t coef_at = t[MADTP_JPEG_F_COEF], q_at = t[MADTP_JPEG_F_QTABLE], planes_at = t[MADTP_JPEG_F_PLANES];
    if (coef_at < 0 || (coef_at & 15) || q_at < 0 || (q_at & 15) || planes_at < 0 || (planes_at & 7)) return;
    const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
    const int64_t k = local * IDCT_BLOCKS + slot;  // block of the image, component after component
    const bool live = k < g.luma + 2 * g.chroma;
    int comp = 0, pbx = g.bx;
    int64_t kk = k, plane_at = 0;
    if (k >= g.luma) {
        comp = k - g.luma >= g.chroma ? 2 : 1;
        kk = k - g.luma - (comp - 1) * g.chroma;
        pbx = g.bx / g.hs;
        plane_at = 64 * (g.luma + (comp - 1) * g.chroma);
    }
    // column j of the block: one 16-byte vector of coefficients, one of the (column-major) quantisation table
    uint32_t v[8];
    int32_t o[8];
    if (live) {
        const int4 c4 = *(const int4*)(coef + coef_at + k * 128 + j * 16);
        const int4 q4 = *(const int4*)(qtables + q_at + comp * 128 + j * 16);
        const int cw[4] = {c4.x, c4.y, c4.z, c4.w}, qw[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = (uint32_t)(int32_t)(int16_t)(cw[i] & 0xffff) * (uint32_t)(qw[i] & 0xffff);
            v[2 * i + 1] = (uint32_t)(cw[i] >> 16) * ((uint32_t)qw[i] >> 16);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = 0;
    }
    idct8<11>(v, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[slot * WS_BLOCK + r * WS_ROW + j] = o[r];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = (uint32_t)ws[slot * WS_BLOCK + j * WS_ROW + c];
    idct8<18>(v, o);
    if (!live) return;
    uint2 px;
    px.x = range_limit(o[0]) | range_limit(o[1]) << 8 | range_limit(o[2]) << 16 | range_limit(o[3]) << 24;
    px.y = range_limit(o[4]) | range_limit(o[5]) << 8 | range_limit(o[6]) << 16 | range_limit(o[7]) << 24;
    const int64_t brow = kk / pbx, bcol = kk - brow * pbx;
    *(uint2*)(planes + planes_at + plane_at + (brow * 8 + j) * (int64_t)(pbx * 8) + bcol * 8) = px;  // row j of the block
}

// the chroma sample of output pixel (x, y): libjpeg's h2v1 / h2v2 fancy upsampling, one output at a time.  A neighbour that does not
// exist is the sample itself, which turns the filter into libjpeg's edge rules ((3 s + s + 1) >> 2 = s, (3 c + c + 8) >> 4).
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ C, int stride, int x, int y, int hs, int vs, int dw, int dh) {
    if (hs == 1) return C[(int64_t)y * stride + x];
    const int cx = x >> 1, odd = x & 1;
    const int nx = odd ? min(cx + 1, dw - 1) : max(cx - 1, 0);
    if (vs == 1) {
        const uint8_t* row = C + (int64_t)y * stride;
        if (dw <= 2) return row[cx];
        return (3 * row[cx] + row[nx] + 1 + odd) >> 2;
    }
    const int cy = y >> 1;
    const uint8_t* near = C + (int64_t)cy * stride;
    if (dw <= 2) return near[cx];
    const uint8_t* far = C + (int64_t)((y & 1) ? min(cy + 1, dh - 1) : max(cy - 1, 0)) * stride;
    const int c0 = 3 * near[cx] + far[cx], c1 = 3 * near[nx] + far[nx];
    return (3 * c0 + c1 + 8 - odd) >> 4;
}

__device__ __forceinline__ uint32_t clamp8(int v) { return (uint32_t)min(max(v, 0), 255); }

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_rgb_kernel(const uint8_t* __restrict__ planes, const int64_t* __restrict__ table,
                                                                uint8_t* __restrict__ out, int B) {
    const int64_t* t = table + (size_t)find_image(table, B, MADTP_JPEG_F_FIRST_RGB) * MADTP_JPEG_FIELDS;
    const int64_t local = (int64_t)blockIdx.x - t[MADTP_JPEG_F_FIRST_RGB];
    Geometry g;
    if (!g.read(t) || local < 0) return;
    const int64_t planes_at = t[MADTP_JPEG_F_PLANES], out_at = t[MADTP_JPEG_F_OUT];
    if (planes_at < 0 || out_at < 0 || (out_at & 3)) return;
    const int npix = g.w * g.h;  // at most 2^26
    const int64_t p0 = (local * JPEG_THREADS + threadIdx.x) * 4;
    if (p0 >= npix) return;
    const uint8_t* Y = planes + planes_at;
    const uint8_t* Cb = Y + 64 * g.luma;
    const uint8_t* Cr = Cb + 64 * g.chroma;
    const int ystride = 8 * g.bx, cstride = 8 * (g.bx / g.hs);
    const int dw = (g.w + g.hs - 1) / g.hs, dh = (g.h + g.vs - 1) / g.vs;
    int y = (int)(p0 / g.w), x = (int)(p0 - (int64_t)y * g.w);
    uint32_t bytes[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int lum = Y[(int64_t)y * ystride + x];
        uint32_t r, gr, b;
        if (g.components == 1) {
            r = gr = b = (uint32_t)lum;
        } else {
            const int cb = chroma_at(Cb, cstride, x, y, g.hs, g.vs, dw, dh) - 128;
            const int cr = chroma_at(Cr, cstride, x, y, g.hs, g.vs, dw, dh) - 128;
            r = clamp8(lum + ((91881 * cr + 32768) >> 16));
            gr = clamp8(lum + ((-22554 * cb - 46802 * cr + 32768) >> 16));
            b = clamp8(lum + ((116130 * cb + 32768) >> 16));
        }
        bytes[3 * i] = r, bytes[3 * i + 1] = gr, bytes[3 * i + 2] = b;
        if (p0 + i + 1 < npix && ++x == g.w) x = 0, ++y;  // (past the last pixel the group repeats it: the bytes are padding)
    }
    uint32_t* dst = (uint32_t*)(out + out_at + p0 * 3);
    dst[0] = bytes[0] | bytes[1] << 8 | bytes[2] << 16 | bytes[3] << 24;
    dst[1] = bytes[4] | bytes[5] << 8 | bytes[6] << 16 | bytes[7] << 24;
    dst[2] = bytes[8] | bytes[9] << 8 | bytes[10] << 16 | bytes[11] << 24;
}

bool geometry_ok(int components, int hs, int vs, int blocks_x, int blocks_y) {
    if (components != 1 && components != 3) return false;
    if (!((hs == 1 && vs == 1) || (components == 3 && hs == 2 && (vs == 1 || vs == 2)))) return false;
    const int most = MADTP_JPEG_MAX_SIDE / 8 + 1;
    return blocks_x >= 1 && blocks_y >= 1 && blocks_x <= most && blocks_y <= most && blocks_x % hs == 0 && blocks_y % vs == 0;
}

}  // namespace

extern "C" int madtp_jpeg_abi_version(void) { return MADTP_JPEG_ABI_VERSION; }

extern "C" const char* madtp_jpeg_strerror(int code) {
    const char* s = madtp_jpeg::strerror_jpeg(code);
    return s ? s : madtp_strerror(code);
}

extern "C" int madtp_jpeg_inspect(const void* data, int64_t size, int32_t* info, void* qtables) {
    return madtp_jpeg::inspect((const uint8_t*)data, size, info, (uint16_t*)qtables);
}

extern "C" int madtp_jpeg_entropy_decode(const void* data, int64_t size, void* coef, int64_t coef_capacity) {
    return madtp_jpeg::entropy_decode((const uint8_t*)data, size, (int16_t*)coef, coef_capacity);
}

extern "C" int64_t madtp_jpeg_blocks(int components, int hs, int vs, int blocks_x, int blocks_y) {
    if (!geometry_ok(components, hs, vs, blocks_x, blocks_y)) return 0;
    const int64_t luma = (int64_t)blocks_x * blocks_y;
    return components == 1 ? luma : luma + 2 * (luma / (hs * vs));
}

extern "C" int64_t madtp_jpeg_plane_bytes(int components, int hs, int vs, int blocks_x, int blocks_y) {
    return 64 * madtp_jpeg_blocks(components, hs, vs, blocks_x, blocks_y);
}

extern "C" int64_t madtp_jpeg_out_bytes(int w, int h) {
    if (w < 1 || h < 1 || w > MADTP_JPEG_MAX_SIDE || h > MADTP_JPEG_MAX_SIDE) return 0;
    return 12 * (((int64_t)w * h + 3) / 4);
}

extern "C" int madtp_jpeg_idct_groups(int64_t blocks) {
    if (blocks < 1 || blocks > ((int64_t)1 << 36)) return 0;
    const int64_t n = (blocks + MADTP_JPEG_IDCT_BLOCKS - 1) / MADTP_JPEG_IDCT_BLOCKS;
    return n > 0x7fffffff ? 0 : (int)n;
}

extern "C" int madtp_jpeg_rgb_groups(int w, int h) {
    if (w < 1 || h < 1 || w > MADTP_JPEG_MAX_SIDE || h > MADTP_JPEG_MAX_SIDE) return 0;
    return (int)(((int64_t)w * h + MADTP_JPEG_RGB_PIXELS - 1) / MADTP_JPEG_RGB_PIXELS);
}

extern "C" int64_t madtp_jpeg_workspace(int B, int64_t plane_bytes_sum) {
    if (B < 1 || plane_bytes_sum < 1) return 0;
    return plane_bytes_sum + 256 * (int64_t)B;
}

extern "C" int madtp_jpeg_idct_batch(const void* coef, const void* qtables, const int64_t* table, void* planes, int B, int n_groups,
                                     void* stream) {
    if (!coef || !qtables || !table || !planes || B < 1 || n_groups < 1) return MADTP_E_BADARG;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(n_groups), dim3(JPEG_THREADS), 0, (hipStream_t)stream, (const uint8_t*)coef,
                       (const uint8_t*)qtables, table, (uint8_t*)planes, B);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" int madtp_jpeg_rgb_batch(const void* planes, const int64_t* table, void* out, int B, int n_groups, void* stream) {
    if (!planes || !table || !out || B < 1 || n_groups < 1) return MADTP_E_BADARG;
    hipLaunchKernelGGL(jpeg_rgb_kernel, dim3(n_groups), dim3(JPEG_THREADS), 0, (hipStream_t)stream, (const uint8_t*)planes, table,
                       (uint8_t*)out, B);
    MADTP_LAUNCH_CHECK();
    return 0;
}

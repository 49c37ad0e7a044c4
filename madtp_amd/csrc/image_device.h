// The resize tile of the image stage (include/madtp_image.h), shared by its two kernels: image.hip stores the tile through the
// 3 x 256 normalisation table into f32 planes, augment.hip stores the three clip8 bytes into uint8 planes for the augmentation
// stages.  One workgroup owns IMG_TW output columns x TILE_H output rows of one image: horizontal pass of the source rows the tile
// needs into LDS (rounded to uint8, as Pillow's first pass is), vertical pass from LDS, three coalesced plane stores.
//
// A Store has   __device__ void prepare()                                        every thread, before the tile's one barrier
//               __device__ void put(size_t index, size_t plane, int r, int g, int b)   index = offset of (image, channel 0, y, x)
#pragma once
#include "common.h"

#include "../../include/madtp_image.h"

namespace {

constexpr int IMG_THREADS = 256;
constexpr int IMG_TW = MADTP_IMAGE_TILE_W;
constexpr int IMG_ROWS = MADTP_IMAGE_LDS_ROWS;
constexpr int IMG_ROW_BYTES = IMG_TW * 3;  // the intermediate keeps the source's interleaved RGB
constexpr int IMG_MAX_TILE_H = 32;
static_assert(IMG_THREADS % IMG_TW == 0, "a thread keeps one tile column through both passes");
constexpr int IMG_ROW_STEP = IMG_THREADS / IMG_TW;
constexpr int IMG_HROWS = 4;  // source rows a thread carries through one step of the horizontal pass (0.81-0.85 of one row's time)

// (the table's addresses are device memory: global_load rather than the flat forms a plain pointer compiles to)
typedef __attribute__((address_space(1))) const uint8_t gu8;
typedef __attribute__((address_space(1))) const int32_t gi32;

// Pillow's clip8 (ImagingUtils.h): arithmetic shift by the 22 coefficient bits, then the clamp
__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> 22, 0), 255); }

template <class Store>
__device__ __forceinline__ void image_resize_tile(const uint8_t* __restrict__ src, const int64_t* __restrict__ table, int B, int Sh,
                                                  int Sw, Store store) {
    __shared__ uint8_t inter[IMG_ROWS * IMG_ROW_BYTES];
    // the image this block belongs to: last b with first_block[b] <= blockIdx.x (madtp_adamw_step's search)
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(size_t)mid * MADTP_IMAGE_FIELDS + MADTP_IMAGE_F_FIRST] <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const int b = lo;
    const int64_t* t = table + (size_t)b * MADTP_IMAGE_FIELDS;
    const int tile_h = (int)t[MADTP_IMAGE_F_TILE_H];
    const int local = (int)((int64_t)blockIdx.x - t[MADTP_IMAGE_F_FIRST]);
    const int tiles_x = (Sw + IMG_TW - 1) / IMG_TW;
    if (tile_h < 1 || tile_h > IMG_MAX_TILE_H || local < 0) return;
    const int x0 = (local % tiles_x) * IMG_TW, y0 = (local / tiles_x) * tile_h;
    if (y0 >= Sh) return;
    const int rows = min(tile_h, Sh - y0);
    gi32* by = (gi32*)t[MADTP_IMAGE_F_BY];
    const int ybase = by[2 * y0];
    const int span = by[2 * (y0 + rows - 1)] + by[2 * (y0 + rows - 1) + 1] - ybase;  // source rows [ybase, ybase + span)
    if (ybase < 0 || span < 0 || span > IMG_ROWS || ybase + span > (int)t[MADTP_IMAGE_F_H]) return;  // (uniform: before any barrier)

    store.prepare();

    const int c = threadIdx.x % IMG_TW;  // this thread's tile column in both passes
    const int x = x0 + c;
    const bool live = x < Sw;
    const int xt = t[MADTP_IMAGE_F_FLIP] ? Sw - 1 - x : x;  // the column of the resize this output column shows
    if (live) {
        const int ksx = (int)t[MADTP_IMAGE_F_KSX];
        gi32* bx = (gi32*)t[MADTP_IMAGE_F_BX];
        gi32* kx = (gi32*)t[MADTP_IMAGE_F_KX] + (size_t)xt * ksx;
        const int xmin = bx[2 * xt], n = min(bx[2 * xt + 1], ksx);
        const int64_t stride = t[MADTP_IMAGE_F_STRIDE];
        gu8* p0 = (gu8*)(src + t[MADTP_IMAGE_F_OFFSET]) + (int64_t)ybase * stride + (int64_t)xmin * 3;
        if (xmin >= 0 && xmin + n <= (int)t[MADTP_IMAGE_F_W]) {
            // IMG_HROWS rows per step: one coefficient load serves them all, and their byte loads are in flight together (a row
            // past the span re-reads the span's last row and is not stored)
            for (int r = threadIdx.x / IMG_TW; r < span; r += IMG_HROWS * IMG_ROW_STEP) {
                gu8* p[IMG_HROWS];
                int a[IMG_HROWS][3];
#pragma unroll
                for (int j = 0; j < IMG_HROWS; ++j) {
                    p[j] = p0 + (int64_t)min(r + j * IMG_ROW_STEP, span - 1) * stride;
                    a[j][0] = a[j][1] = a[j][2] = 1 << 21;
                }
                for (int i = 0; i < n; ++i) {
                    const int k = kx[i];
#pragma unroll
                    for (int j = 0; j < IMG_HROWS; ++j) {
                        a[j][0] += (int)p[j][3 * i] * k;
                        a[j][1] += (int)p[j][3 * i + 1] * k;
                        a[j][2] += (int)p[j][3 * i + 2] * k;
                    }
                }
#pragma unroll
                for (int j = 0; j < IMG_HROWS; ++j) {
                    const int rj = r + j * IMG_ROW_STEP;
                    if (rj < span) {
                        uint8_t* q = inter + rj * IMG_ROW_BYTES + c * 3;
                        q[0] = (uint8_t)clip8(a[j][0]);
                        q[1] = (uint8_t)clip8(a[j][1]);
                        q[2] = (uint8_t)clip8(a[j][2]);
                    }
                }
            }
        }
    }
    __syncthreads();
    if (!live) return;
    const int ksy = (int)t[MADTP_IMAGE_F_KSY];
    gi32* ky = (gi32*)t[MADTP_IMAGE_F_KY];
    const size_t plane = (size_t)Sh * Sw;
    const size_t o = (size_t)b * 3 * plane + x;
    for (int r = threadIdx.x / IMG_TW; r < rows; r += IMG_ROW_STEP) {
        const int y = y0 + r;
        const int first = by[2 * y] - ybase;
        const int n = min(min(by[2 * y + 1], ksy), span - first);
        if (first < 0) continue;
        gi32* k = ky + (size_t)y * ksy;
        const uint8_t* q = inter + first * IMG_ROW_BYTES + c * 3;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int i = 0; i < n; ++i) {
            const int kk = k[i];
            a0 += (int)q[i * IMG_ROW_BYTES] * kk;
            a1 += (int)q[i * IMG_ROW_BYTES + 1] * kk;
            a2 += (int)q[i * IMG_ROW_BYTES + 2] * kk;
        }
        // lanes = consecutive columns: contiguous bytes per wave and plane
        store.put(o + (size_t)y * Sw, plane, clip8(a0), clip8(a1), clip8(a2));
    }
}

}  // namespace

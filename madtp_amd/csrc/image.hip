// The image stage of the data loader (include/madtp_image.h): uint8 RGB images of different sizes -> normalised f32 [B,3,Sh,Sw]
// in one launch.  Pillow's bicubic resize (Resample.c) is integer arithmetic on host-made fixed-point coefficient tables, so the
// result has the bits of the reference's PIL Resize + ToTensor + Normalize.  One workgroup owns IMG_TW output columns x TILE_H
// output rows of one image: horizontal pass of the source rows the tile needs into LDS (rounded to uint8, as Pillow's first pass
// is), vertical pass from LDS (image_device.h, shared with augment.hip), three coalesced f32 plane stores through the 3 x 256
// normalisation table (the store below).  No atomics, no intermediate in global memory, fixed grid: identical calls give
// identical bits.
#include "image_device.h"

namespace {

// the store of this kernel: ToTensor + Normalize of a byte is one of 3 x 256 f32 values, kept in LDS
struct StoreNormalized {
    const float* __restrict__ lut;
    float* slut;
    float* __restrict__ out;
    __device__ __forceinline__ void prepare() const {
        for (int i = threadIdx.x; i < 3 * 256; i += IMG_THREADS) slut[i] = lut[i];
    }
    __device__ __forceinline__ void put(size_t index, size_t plane, int r, int g, int b) const {
        float* oy = out + index;  // 256 contiguous bytes per wave and plane
        oy[0] = slut[r];
        oy[plane] = slut[256 + g];
        oy[2 * plane] = slut[512 + b];
    }
};

__global__ __launch_bounds__(IMG_THREADS) void image_resize_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ table,
                                                                    const float* __restrict__ lut, float* __restrict__ out, int B,
                                                                    int Sh, int Sw) {
    __shared__ float slut[3 * 256];
    image_resize_tile(src, table, B, Sh, Sw, StoreNormalized{lut, slut, out});
}

}  // namespace

extern "C" int madtp_image_abi_version(void) { return MADTP_IMAGE_ABI_VERSION; }

extern "C" int madtp_image_tile_rows(double ratio, int ksize) {
    // rows of a tile of T output rows: yend(last) - ymin(first) <= (T - 1) * ratio + 2 * support + 1 <= (T - 1) * ratio + ksize
    if (!(ratio > 0.0) || ksize < 1 || ksize > MADTP_IMAGE_MAX_KSIZE) return 0;
    for (int T = IMG_MAX_TILE_H; T >= 1; T >>= 1)
        if ((T - 1) * ratio + ksize <= (double)IMG_ROWS) return T;
    return 0;
}

extern "C" int madtp_image_blocks(int Sh, int Sw, int tile_h) {
    if (Sh < 1 || Sw < 1 || tile_h < 1) return 0;
    const int64_t n = (int64_t)((Sw + IMG_TW - 1) / IMG_TW) * ((Sh + tile_h - 1) / tile_h);
    return n > 0x7fffffff ? 0 : (int)n;
}

extern "C" int madtp_image_resize_batch(const void* src, const int64_t* table, const float* lut, float* out, int B, int Sh, int Sw,
                                        int n_blocks, int max_ksize, void* stream) {
    if (!src || !table || !lut || !out || B < 1 || n_blocks < 1) return MADTP_E_BADARG;
    if (Sh < 1 || Sw < 1 || max_ksize < 1 || max_ksize > MADTP_IMAGE_MAX_KSIZE) return MADTP_E_SHAPE;
    hipLaunchKernelGGL(image_resize_kernel, dim3(n_blocks), dim3(IMG_THREADS), 0, (hipStream_t)stream, (const uint8_t*)src, table,
                       lut, out, B, Sh, Sw);
    MADTP_LAUNCH_CHECK();
    return 0;
}

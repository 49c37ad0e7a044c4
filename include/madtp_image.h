/* madtp_image.h - the image stage of the data loader on the device: uint8 RGB images of different sizes -> the normalised f32
 * [B, 3, Sh, Sw] batch a model takes, in one launch (csrc/image.hip, linked into libmadtp_hip.so).
 *
 * It mirrors what the reference's DataLoader workers do per image (data/__init__.py:29-33, clip/clip.py:80-88): PIL bicubic
 * Resize, ToTensor, Normalize - bit for bit, since Pillow's resampling is integer arithmetic on fixed-point coefficients
 * (Resample.c): the horizontal pass first, rounded to uint8, then the vertical pass on those bytes,
 *     acc = 2^21 + sum_i px[xmin + i] * k[i]   (int32),    result = clamp(acc >> 22, 0, 255)   (arithmetic shift),
 * and ToTensor + Normalize of a byte is one of 3 x 256 f32 values.  The coefficient tables k (22 fractional bits) and the bounds
 * (xmin, n) come from the HOST (madtp_amd/preprocess.py resample_tables: IEEE double, operation by operation as Pillow's C);
 * computed on the device, FMA contraction would change bits.
 *
 * Conventions of madtp_hip.h: plain pointers and sizes, nothing allocates, frees or synchronises, the launch goes to `stream`
 * (a hipStream_t passed as void*); 0 on success, a negative MADTP_E_* code on a rejected argument before any launch, a positive
 * hipError_t if the runtime refuses the launch.  This header has its own version number: MADTP_ABI_VERSION and the entry
 * points of madtp_hip.h (the op sequence of the models) do not change with it. */
#ifndef MADTP_IMAGE_H
#define MADTP_IMAGE_H

#include "madtp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MADTP_IMAGE_ABI_VERSION 1
int madtp_image_abi_version(void);

/* One int64 row of MADTP_IMAGE_FIELDS entries per image (device memory, the pointer-table scheme of madtp_ema_update and
 * madtp_adamw_step).  Unused entries are 0. */
#define MADTP_IMAGE_FIELDS 16
#define MADTP_IMAGE_F_OFFSET 0   /* byte offset from src to the first pixel of the (cropped) source image                    */
#define MADTP_IMAGE_F_STRIDE 1   /* bytes from one source row to the next (>= 3 * w; a crop keeps the stride of its image)  */
#define MADTP_IMAGE_F_W 2        /* source width in pixels (of the crop box, when there is one), 1 .. 8192                  */
#define MADTP_IMAGE_F_H 3        /* source height                                                                            */
#define MADTP_IMAGE_F_KX 4       /* address of int32 [Sw, ksx]: coefficients of output column x (of the FIRST column of an   */
#define MADTP_IMAGE_F_BX 5       /* output window into a larger resize); address of int32 [Sw, 2]: (xmin, n) of column x     */
#define MADTP_IMAGE_F_KSX 6      /* row width of the KX table, 1 .. MADTP_IMAGE_MAX_KSIZE                                    */
#define MADTP_IMAGE_F_KY 7       /* the same three for the rows: int32 [Sh, ksy]                                             */
#define MADTP_IMAGE_F_BY 8       /* int32 [Sh, 2]: (ymin, n) of output row y; ymin and ymin + n must not decrease with y     */
#define MADTP_IMAGE_F_KSY 9
#define MADTP_IMAGE_F_FLIP 10    /* != 0: output column x shows column Sw - 1 - x (the resize, then a horizontal flip)       */
#define MADTP_IMAGE_F_TILE_H 11  /* output rows per workgroup, >= 1: the source rows [ymin(first), ymin + n (last)) of every  */
/*                                  tile of this image must number at most MADTP_IMAGE_LDS_ROWS (madtp_image_tile_rows)      */
#define MADTP_IMAGE_F_FIRST 12   /* first workgroup of the image: prefix sum of madtp_image_blocks                           */

#define MADTP_IMAGE_TILE_W 64    /* output columns per workgroup                                                             */
#define MADTP_IMAGE_LDS_ROWS 128 /* rows of the horizontally resized intermediate a workgroup keeps in LDS                   */
#define MADTP_IMAGE_MAX_KSIZE 65 /* ksize = 2 * ceil(2 * max(ratio, 1)) + 1 of a downscale ratio of 16                       */

/* Largest tile height (a power of two, at most 32) with which every tile of an axis of `in` source rows resized by `ratio` =
 * in / out with rows of `ksize` coefficients surely fits MADTP_IMAGE_LDS_ROWS; 0 if none does (ksize > MADTP_IMAGE_MAX_KSIZE). */
int madtp_image_tile_rows(double ratio, int ksize);
/* Workgroups of one image: ceil(Sw / MADTP_IMAGE_TILE_W) * ceil(Sh / tile_h); 0 for a non-positive argument. */
int madtp_image_blocks(int Sh, int Sw, int tile_h);

/* madtp_image_resize_batch: B uint8 RGB images (3-byte pixels, rows at any alignment) -> out f32 [B, 3, Sh, Sw].
 *   src        the packed source bytes; image b starts at src + table[b][OFFSET]
 *   table      int64 [B, MADTP_IMAGE_FIELDS], see above
 *   lut        f32 [3, 256]: lut[c][v] = what ToTensor + Normalize make of byte v in channel c
 *   n_blocks   sum of madtp_image_blocks over the images (table[b][FIRST] is its prefix sum)
 *   max_ksize  the largest KSX / KSY of the batch
 * One workgroup owns MADTP_IMAGE_TILE_W columns x TILE_H rows of one image: it forms the intermediate rows its tile needs in
 * LDS (no intermediate in global memory), runs the vertical pass on them and stores the three planes.  No atomics, fixed grid:
 * identical calls give identical bits.  A workgroup whose table row breaks the TILE_H rule writes nothing.
 * MADTP_E_BADARG: a null pointer, B < 1 or n_blocks < 1.  MADTP_E_SHAPE: Sh < 1, Sw < 1, or max_ksize outside
 * 1 .. MADTP_IMAGE_MAX_KSIZE (a downscale ratio beyond 16) - there is no fallback. */
int madtp_image_resize_batch(const void* src, const int64_t* table, const float* lut, float* out, int B, int Sh, int Sw,
                             int n_blocks, int max_ksize, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MADTP_IMAGE_H */

/* madtp_augment.h - the TRAINING transform of the data loader on the device: uint8 RGB images of different sizes -> the
 * normalised f32 [B, 3, Sh, Sw] batch, with the reference's RandAugment between the resize and the normalise
 * (data/__init__.py:21-28, transform/randaugment.py; csrc/augment.hip, linked into libmadtp_hip.so).
 *
 *   madtp_augment_resize_u8       crop box -> Pillow-exact bicubic resize -> flip, as madtp_image_resize_batch does it (the same
 *                                 table rows, the same tile), stored as the three clip8 BYTES: uint8 planes [B, 3, Sh, Sw]
 *   per augmentation stage:
 *   madtp_augment_stats           256-bin histogram of every (image, channel) whose op needs the whole image -> a 256-byte table
 *   madtp_augment_apply           next planes from the current ones: copy, byte table, or affine warp with constant fill; the
 *                                 last stage writes f32 planes through the 3 x 256 normalisation table instead of bytes
 *
 * Every image of a batch has its own op in every stage: one int64 row of MADTP_AUGMENT_FIELDS entries per image (device memory,
 * the pointer-table scheme of madtp_adamw_step).  Conventions of madtp_hip.h and madtp_image.h: nothing allocates, frees or
 * synchronises, launches go to `stream`; 0 on success, a negative MADTP_E_* code on a rejected argument before any launch, a
 * positive hipError_t if the runtime refuses the launch.  All grids are fixed, the only atomics are integer LDS atomics of the
 * histogram, and every double expression is evaluated operation by operation (no FMA contraction): identical calls give
 * identical bits.  This header has its own version number; madtp_hip.h and madtp_image.h do not change with it. */
#ifndef MADTP_AUGMENT_H
#define MADTP_AUGMENT_H

#include "madtp_image.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MADTP_AUGMENT_ABI_VERSION 1
int madtp_augment_abi_version(void);

#define MADTP_AUGMENT_FIELDS 8
#define MADTP_AUGMENT_F_OP 0     /* one of MADTP_AUGMENT_OP_*                                                                 */
#define MADTP_AUGMENT_F_TABLE 1  /* OP_TABLE: address of the host-made uint8 [256] table (all three channels use it)          */
#define MADTP_AUGMENT_F_A0 2     /* OP_WARP: entries 2 .. 7 hold the bits of six doubles a0 .. a5, the INVERSE map             */
/*                                  source x = a0 * x + a1 * y + a2,  source y = a3 * x + a4 * y + a5                          */

#define MADTP_AUGMENT_OP_COPY 0          /* Identity, an op that was not drawn, an op that is the identity at its level       */
#define MADTP_AUGMENT_OP_TABLE 1         /* Brightness: out = table[in]                                                       */
#define MADTP_AUGMENT_OP_EQUALIZE 2      /* per channel, from the histogram h of the Sh * Sw bytes:                           */
/*     step = (Sh * Sw - h[last non-empty bin]) / 255;  step == 0: identity;  else table[i] = min(255, (step / 2 + sum_{j<i} h[j]) / step)  */
#define MADTP_AUGMENT_OP_AUTOCONTRAST 3  /* per channel lo = min, hi = max;  hi <= lo: identity;  else scale = scale255[hi - lo], */
/*     offset = ((256 - lo) mod 256) * scale (the reference negates a uint8),  table[i] = trunc(clip(i * scale + offset, 0, 255)) */
#define MADTP_AUGMENT_OP_WARP 4          /* TranslateX/Y, ShearX/Y, Rotate: fixed-point bilinear, a tap outside the image is 128 */
#define MADTP_AUGMENT_OPS 5
#define MADTP_AUGMENT_FILL 128

/* The warp, for output pixel (x, y), rint = round half to even, >> arithmetic:
 *     X = (rint((a1 * y + a2) * 1024) + 16 + rint(a0 * x * 1024)) >> 5,   Y likewise from a3, a4, a5
 *     sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31
 *     out = (32 (32 - fx)(32 - fy) p[sy][sx] + 32 fx (32 - fy) p[sy][sx + 1] + 32 (32 - fx) fy p[sy + 1][sx] + 32 fx fy p[sy + 1][sx + 1]
 *            + 16384) >> 15
 * modelled on OpenCV's fixed-point warpAffine (10 coordinate bits, 5 interpolation bits, 15 coefficient bits). */

#define MADTP_AUGMENT_MAX_PIXELS 16777216 /* Sh * Sw must stay BELOW 2^24: there the integer Equalize equals the reference's f32 */

/* op_mask: OR of (1 << op) over the rows of `plan` - what the host knows of the stage.  A bit outside MADTP_AUGMENT_OPS is
 * MADTP_E_BADARG; a row whose op the mask does not announce is not looked at by madtp_augment_stats. */

/* madtp_augment_resize_u8: the arguments of madtp_image_resize_batch without the normalisation table; out_u8 is uint8
 * [B, 3, Sh, Sw].  The same refusals. */
int madtp_augment_resize_u8(const void* src, const int64_t* table, void* out_u8, int B, int Sh, int Sw, int n_blocks, int max_ksize,
                            void* stream);

/* madtp_augment_stats: in uint8 [B, 3, Sh, Sw], plan int64 [B, MADTP_AUGMENT_FIELDS], scale255 f64 [256] with scale255[d] =
 * 255 / d for d >= 1 (made on the HOST: the device does not divide doubles), lut_u8 uint8 [B, 3, 256].  One workgroup per (image,
 * channel); those of rows that are neither OP_EQUALIZE nor OP_AUTOCONTRAST exit at once and leave their table untouched.  No
 * launch at all when op_mask holds neither.  MADTP_E_BADARG: a null pointer, B < 1, a bad op_mask.  MADTP_E_SHAPE: Sh < 1, Sw < 1
 * or Sh * Sw >= MADTP_AUGMENT_MAX_PIXELS. */
int madtp_augment_stats(const void* in, const int64_t* plan, const double* scale255, void* lut_u8, int B, int Sh, int Sw, int op_mask,
                        void* stream);

/* madtp_augment_apply: out = op(in) per image.  norm == NULL: out is uint8 [B, 3, Sh, Sw] (must not overlap `in`); else norm is
 * f32 [3, 256] (madtp_image_resize_batch's lut) and out is f32 [B, 3, Sh, Sw].  lut_u8 is what madtp_augment_stats wrote for this
 * stage.  A row with an op code outside MADTP_AUGMENT_OPS writes nothing.  The same refusals as madtp_augment_stats. */
int madtp_augment_apply(const void* in, const int64_t* plan, const void* lut_u8, const float* norm, void* out, int B, int Sh, int Sw,
                        int op_mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MADTP_AUGMENT_H */

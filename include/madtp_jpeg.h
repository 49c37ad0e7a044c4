/* madtp_jpeg.h - baseline JPEG decode for the data loader: Huffman entropy decoding on the host (csrc/jpeg_entropy.h), dequantisation,
 * the 8x8 inverse DCT, chroma upsampling and YCbCr -> RGB on the device (csrc/jpeg.hip, linked into libmadtp_hip.so).  The result
 * is the packed uint8 [h, w, 3] image that madtp_image.h / madtp_augment.h start from.
 *
 * It mirrors the `Image.open(path).convert('RGB')` of the reference's datasets (its data/ dataset classes) bit for bit.  Pillow's JPEG
 * library is libjpeg-turbo, whose default decode is defined operation by operation in integers:
 *   - jpeg_idct_islow: coef * q, a column pass into 32-bit values (CONST_BITS 13, PASS1_BITS 2, descaled by 11), a row pass
 *     descaled by 18, DESCALE(x, n) = (x + (1 << (n - 1))) >> n with an arithmetic shift, and the range-limit table read at
 *     x & 1023, which is clamp((((x + 512) mod 1024) - 512) + 128, 0, 255): a wrap, then a clamp;
 *   - "fancy" triangle upsampling of the chroma planes (h2v1, h2v2), plain replication where a plane has at most two columns;
 *   - the fixed-point colour conversion with 16 fractional bits.
 * All device arithmetic is 32-bit two's complement and wraps; no file a baseline encoder writes comes near the wrap.
 *
 * Conventions of madtp_hip.h / madtp_image.h: plain pointers and sizes, nothing allocates, frees or synchronises, launches go to
 * `stream` (a hipStream_t passed as void*); 0 on success, a negative code on a rejected argument before any launch, a positive
 * hipError_t if the runtime refuses a launch.  The two host calls touch no GPU state: a DataLoader worker process may call them.
 * This header has its own version number; madtp_hip.h, madtp_image.h and madtp_augment.h do not change with it. */
#ifndef MADTP_JPEG_H
#define MADTP_JPEG_H

#include "madtp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MADTP_JPEG_ABI_VERSION 1
int madtp_jpeg_abi_version(void);

#define MADTP_JPEG_MAX_SIDE 8192

/* ---- host stage: codes ------------------------------------------------------------------------------------------------------------
 * -100 .. -199: a valid file of a kind this decoder refuses (there is no fallback); -200 .. -299: a malformed stream.  A malformed
 * stream is never an out-of-bounds access and never a partial image; libjpeg's "warn and fill" recovery is not reproduced. */
#define MADTP_JPEG_E_PROGRESSIVE (-101) /* SOF2 and up: progressive, lossless or arithmetic coding (also a DAC segment)       */
#define MADTP_JPEG_E_PRECISION (-102)   /* sample precision other than 8 bits                                                 */
#define MADTP_JPEG_E_COMPONENTS (-103)  /* a component count other than 1 or 3 (CMYK / YCCK)                                  */
#define MADTP_JPEG_E_ADOBE_RGB (-104)   /* three components with an Adobe APP14 segment of transform 0: RGB, not YCbCr         */
#define MADTP_JPEG_E_RGB_IDS (-105)     /* component ids 'R', 'G', 'B': RGB, not YCbCr                                         */
#define MADTP_JPEG_E_CHROMA (-106)      /* chroma sampling other than 1x1                                                     */
#define MADTP_JPEG_E_LUMA (-107)        /* luma sampling other than 1x1, 2x1 or 2x2                                           */
#define MADTP_JPEG_E_SCANS (-108)       /* more than one scan, or a scan that does not hold every component in frame order    */
#define MADTP_JPEG_E_DNL (-109)         /* a DNL segment or a frame height of 0                                               */
#define MADTP_JPEG_E_SIDE (-110)        /* a side over MADTP_JPEG_MAX_SIDE                                                    */
#define MADTP_JPEG_E_SCAN_PARAMS (-111) /* Ss, Se, Ah, Al other than 0, 63, 0, 0                                              */

#define MADTP_JPEG_E_TRUNCATED (-201)   /* the data ends before the image does                                                */
#define MADTP_JPEG_E_CODE (-202)        /* a bit pattern that is no code of its Huffman table                                 */
#define MADTP_JPEG_E_INDEX (-203)       /* a run that carries a coefficient index beyond 63                                   */
#define MADTP_JPEG_E_NO_TABLE (-204)    /* a quantisation or Huffman table that a component names was never defined           */
#define MADTP_JPEG_E_RESTART (-205)     /* a restart marker is missing, out of sequence or preceded by extra bytes            */
#define MADTP_JPEG_E_SEGMENT (-206)     /* a segment length beyond the buffer, or shorter than its own content                */
#define MADTP_JPEG_E_NOT_JPEG (-207)    /* the data does not begin with SOI                                                   */
#define MADTP_JPEG_E_HEADER (-208)      /* a frame, scan or table segment with impossible content, a missing or repeated SOF  */
#define MADTP_JPEG_E_MARKER (-209)      /* the scan is not followed by EOI                                                    */

/* Human-readable name of one of the codes above (of a MADTP_E_* code: madtp_strerror's). */
const char* madtp_jpeg_strerror(int code);

/* ---- host stage: inspect and entropy-decode ---------------------------------------------------------------------------------------
 * madtp_jpeg_inspect: the header of the `size` bytes at `data` -> info (int32 [MADTP_JPEG_INFO_FIELDS]) and qtables (uint16
 * [3][64]: the table of each component in natural, row-major order; rows of absent components are 0).  Reads up to the scan header.
 * A one-component file is 1x1 sampled whatever its sampling bytes say.  Block counts are padded to whole MCUs (8 x HS by 8 x VS
 * luma pixels of an interleaved scan; one block of a grayscale file). */
#define MADTP_JPEG_INFO_FIELDS 16
#define MADTP_JPEG_I_WIDTH 0
#define MADTP_JPEG_I_HEIGHT 1
#define MADTP_JPEG_I_COMPONENTS 2 /* 1 or 3                                                                                    */
#define MADTP_JPEG_I_HS 3         /* luma sampling: (HS, VS) = (1, 1), (2, 1) or (2, 2)                                         */
#define MADTP_JPEG_I_VS 4
#define MADTP_JPEG_I_BLOCKS_X 5   /* blocks per row of the luma plane; chroma planes have BLOCKS_X / HS                         */
#define MADTP_JPEG_I_BLOCKS_Y 6   /* block rows of the luma plane; chroma planes have BLOCKS_Y / VS                             */
#define MADTP_JPEG_I_RESTART 7    /* restart interval in MCUs, 0 = none                                                         */
#define MADTP_JPEG_I_BLOCKS 8     /* blocks of all components: BLOCKS_X * BLOCKS_Y * (1 + 2 / (HS * VS)), or the luma's alone    */
int madtp_jpeg_inspect(const void* data, int64_t size, int32_t* info, void* qtables);

/* madtp_jpeg_entropy_decode: the same bytes -> coef, int16 [BLOCKS][64]: component after component, each [blocks_y][blocks_x][64],
 * de-zigzagged and NOT dequantised.  Within a block the coefficient of row r and column c is element c * 8 + r (column-major), so
 * that the device stage loads one column as one 16-byte vector; its column pass runs first.  coef_capacity: int16 elements that
 * coef can take, at least 64 * BLOCKS (MADTP_E_BADARG otherwise; nothing is written then).  On an error the content of coef is
 * unspecified, nothing outside coef[0 .. 64 * BLOCKS) is ever written. */
int madtp_jpeg_entropy_decode(const void* data, int64_t size, void* coef, int64_t coef_capacity);

/* ---- device stage -----------------------------------------------------------------------------------------------------------------
 * One int64 row of MADTP_JPEG_FIELDS entries per image (device memory, the table scheme of madtp_image_resize_batch). */
#define MADTP_JPEG_FIELDS 16
#define MADTP_JPEG_F_COEF 0       /* byte offset from `coef` to the image's coefficients (as entropy_decode wrote them), % 16 == 0 */
#define MADTP_JPEG_F_QTABLE 1     /* byte offset from `qtables` to uint16 [3][64] of the image, each table COLUMN-major, % 16 == 0 */
#define MADTP_JPEG_F_PLANES 2     /* byte offset from `planes` to the image's sample planes, % 8 == 0: Y [8 BLOCKS_Y][8 BLOCKS_X], */
/*                                   then Cb and Cr [8 BLOCKS_Y / VS][8 BLOCKS_X / HS]; madtp_jpeg_plane_bytes of scratch          */
#define MADTP_JPEG_F_OUT 3        /* byte offset from `out` to the image's packed RGB [H, W, 3], % 4 == 0; the kernel writes whole */
/*                                   12-byte groups: madtp_jpeg_out_bytes(W, H) bytes belong to the image                           */
#define MADTP_JPEG_F_W 4          /* 1 .. MADTP_JPEG_MAX_SIDE                                                                     */
#define MADTP_JPEG_F_H 5
#define MADTP_JPEG_F_COMPONENTS 6 /* 1 or 3                                                                                       */
#define MADTP_JPEG_F_HS 7
#define MADTP_JPEG_F_VS 8
#define MADTP_JPEG_F_BLOCKS_X 9   /* of the luma plane, a multiple of HS, 8 * BLOCKS_X >= W                                        */
#define MADTP_JPEG_F_BLOCKS_Y 10  /* of the luma plane, a multiple of VS, 8 * BLOCKS_Y >= H                                        */
#define MADTP_JPEG_F_FIRST_IDCT 11 /* first workgroup of the image in idct_batch: prefix sum of madtp_jpeg_idct_groups             */
#define MADTP_JPEG_F_FIRST_RGB 12  /* first workgroup of the image in rgb_batch: prefix sum of madtp_jpeg_rgb_groups               */

#define MADTP_JPEG_IDCT_BLOCKS 32   /* 8x8 blocks per workgroup of idct_batch (eight lanes per block)                             */
#define MADTP_JPEG_RGB_PIXELS 1024  /* pixels per workgroup of rgb_batch (four per lane)                                          */

/* Sizes the caller needs (host arithmetic, no GPU): 0 for an argument outside the ranges above. */
int64_t madtp_jpeg_blocks(int components, int hs, int vs, int blocks_x, int blocks_y); /* the I_BLOCKS of such an image          */
int64_t madtp_jpeg_plane_bytes(int components, int hs, int vs, int blocks_x, int blocks_y); /* 64 * blocks: one byte per sample  */
int64_t madtp_jpeg_out_bytes(int w, int h);                                            /* 12 * ceil(w * h / 4)                   */
int madtp_jpeg_idct_groups(int64_t blocks);                                            /* ceil(blocks / MADTP_JPEG_IDCT_BLOCKS)  */
int madtp_jpeg_rgb_groups(int w, int h);                                               /* ceil(w * h / MADTP_JPEG_RGB_PIXELS)    */
/* madtp_jpeg_workspace: bytes of `planes` for a batch whose images take plane_bytes_sum in all, each placed at a multiple of 256. */
int64_t madtp_jpeg_workspace(int B, int64_t plane_bytes_sum);

/* madtp_jpeg_idct_batch: coefficients -> uint8 sample planes (dequantise, jpeg_idct_islow, range limit).  Eight lanes per block:
 * each runs one column, the 8x8 values cross through LDS, each runs one row and stores its 8 bytes.  n_groups: the sum of
 * madtp_jpeg_idct_groups over the images.  No atomics, fixed grid: identical calls give identical bits.
 * madtp_jpeg_rgb_batch: planes -> packed RGB.  A lane owns four consecutive pixels of the flattened [H * W] image (12 bytes, three
 * dword stores); chroma is upsampled on the fly from up to four samples per pixel, no upsampled plane reaches global memory,
 * padding rows and columns beyond ceil(H / VS), ceil(W / HS) are never read.  n_groups: the sum of madtp_jpeg_rgb_groups.
 * MADTP_E_BADARG: a null pointer, B < 1 or n_groups < 1.  A workgroup whose table row breaks a rule above writes nothing. */
int madtp_jpeg_idct_batch(const void* coef, const void* qtables, const int64_t* table, void* planes, int B, int n_groups, void* stream);
int madtp_jpeg_rgb_batch(const void* planes, const int64_t* table, void* out, int B, int n_groups, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MADTP_JPEG_H */

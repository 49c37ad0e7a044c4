/* madtp_png.h - PNG decode for the data loader: chunk parsing on the host (csrc/png_device.h, madtp_png_prepare), zlib inflate and
 * the per-row unfilter on the device (csrc/png.hip, linked into libmadtp_hip.so).  The result is the packed uint8 [h, w, 3] image
 * that madtp_image.h / madtp_augment.h start from, with the bytes of the `Image.open(path).convert('RGB')` of the reference's
 * datasets (Pillow 12.2.0), which for a PNG is:
 *   RGB 8-bit: the three bytes; RGBA 8-bit: R, G, B (alpha dropped, no compositing); gray 8-bit: the value three times; gray +
 *   alpha 8-bit: the gray value three times; gray 1 / 2 / 4-bit: v * 255 / 85 / 17; palette 1 / 2 / 4 / 8-bit: PLTE[v], and black
 *   for an index beyond PLTE; RGB / RGBA 16-bit: the high byte of each sample.  tRNS, gAMA, sRGB, iCCP, pHYs, text and unknown
 *   ancillary chunks change nothing.  Chunk CRCs are not verified (Pillow does not verify those of IDAT).
 *
 * Conventions of madtp_hip.h / madtp_jpeg.h: plain pointers and sizes, nothing allocates, frees or synchronises, launches go to
 * `stream` (a hipStream_t passed as void*); 0 on success, a negative code on a rejected argument before any launch, a positive
 * hipError_t if the runtime refuses a launch.  The host calls touch no GPU state: a DataLoader worker process may call them.
 * This header has its own version number; the other headers do not change with it.  It lives next to the sources that implement
 * it: the file list of include/ is pinned by a test of the candidate lists. */
#ifndef MADTP_PNG_H
#define MADTP_PNG_H

#include "../../include/madtp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MADTP_PNG_ABI_VERSION 1
int madtp_png_abi_version(void);

#define MADTP_PNG_MAX_SIDE 8192

/* ---- codes ------------------------------------------------------------------------------------------------------------------------
 * -100 .. -199: a valid file of a kind this decoder refuses; -200 .. -299: a malformed file or stream.  A malformed stream is never
 * an out-of-bounds access and never a partial image. */
#define MADTP_PNG_E_INTERLACE (-101)   /* Adam7 interlace                                                                       */
#define MADTP_PNG_E_GRAY16 (-102)      /* 16-bit gray or gray + alpha (Pillow opens them as I;16 and clips)                     */
#define MADTP_PNG_E_APNG (-103)        /* an animation: acTL with more than one frame, or an fdAT chunk                         */
#define MADTP_PNG_E_SIDE (-104)        /* a side over MADTP_PNG_MAX_SIDE                                                        */
#define MADTP_PNG_E_COLOR_DEPTH (-105) /* a colour type / bit depth pair the PNG specification forbids                          */

#define MADTP_PNG_E_SIGNATURE (-201)   /* the data does not begin with the PNG signature                                        */
#define MADTP_PNG_E_NO_IHDR (-202)     /* the first chunk is not a 13-byte IHDR                                                 */
#define MADTP_PNG_E_NO_PLTE (-203)     /* a palette image without a PLTE chunk before its IDAT                                  */
#define MADTP_PNG_E_NO_IDAT (-204)     /* no IDAT chunk                                                                         */
#define MADTP_PNG_E_CHUNK (-205)       /* a chunk running past the end of the data, or the data ending without IEND            */
#define MADTP_PNG_E_HEADER (-206)      /* IHDR or PLTE with impossible content: a side of 0, an unknown method, a second one    */
#define MADTP_PNG_E_IDAT_ORDER (-207)  /* IDAT chunks that are not consecutive (Pillow stops at the chunk between them)         */
#define MADTP_PNG_E_ZLIB_HEADER (-208) /* a zlib header that is not deflate, has a window above 32 KiB or fails its check       */
#define MADTP_PNG_E_DICT (-209)        /* a preset dictionary                                                                   */
#define MADTP_PNG_E_BLOCK_TYPE (-210)  /* block type 3                                                                          */
#define MADTP_PNG_E_STORED (-211)      /* a stored block whose LEN and NLEN disagree                                            */
#define MADTP_PNG_E_LENGTHS (-212)     /* a code-length set that is over-subscribed, incomplete where zlib refuses it, repeats  */
/*                                        nothing or past the end, counts above 286 / 30, or has no end-of-block code           */
#define MADTP_PNG_E_SYMBOL (-213)      /* a bit pattern that is no code, or a length / distance symbol that stands for nothing  */
#define MADTP_PNG_E_DISTANCE (-214)    /* a distance beyond the bytes produced so far                                           */
#define MADTP_PNG_E_SIZE (-215)        /* output that is not exactly RAW_BYTES bytes                                            */
#define MADTP_PNG_E_TRUNCATED (-216)   /* the stream ends before its final block and checksum do                                */
#define MADTP_PNG_E_ADLER (-217)       /* the Adler-32 of the output is not the stream's                                        */
#define MADTP_PNG_E_FILTER (-218)      /* a filter byte above 4                                                                 */

/* Human-readable name of one of the codes above (of a MADTP_E_* code: madtp_strerror's). */
const char* madtp_png_strerror(int code);

/* ---- host stage -------------------------------------------------------------------------------------------------------------------
 * madtp_png_prepare: the chunks of the `size` bytes at `data` -> info (int32 [MADTP_PNG_INFO_FIELDS]), palette (768 bytes: PLTE,
 * zero beyond it and for other colour types) and, where `stream` is not null, the payloads of the IDAT chunks one behind the other
 * as ONE contiguous zlib stream of STREAM_BYTES bytes (the device never sees chunk framing).  stream_capacity: bytes that `stream`
 * can take, at least STREAM_BYTES (MADTP_E_BADARG otherwise, info and palette are filled, nothing is written to stream).  With a
 * null `stream` the call only inspects.  Nothing outside the three buffers is written. */
#define MADTP_PNG_INFO_FIELDS 16
#define MADTP_PNG_I_WIDTH 0
#define MADTP_PNG_I_HEIGHT 1
#define MADTP_PNG_I_DEPTH 2        /* bits per sample: 1, 2, 4, 8, 16                                                            */
#define MADTP_PNG_I_COLOR 3        /* PNG colour type: 0 gray, 2 RGB, 3 palette, 4 gray + alpha, 6 RGBA                          */
#define MADTP_PNG_I_CHANNELS 4     /* samples per pixel: 1, 3, 1, 2, 4                                                           */
#define MADTP_PNG_I_ROWBYTES 5     /* ceil(WIDTH * CHANNELS * DEPTH / 8), without the filter byte                                */
#define MADTP_PNG_I_BPP 6          /* the distance in bytes the filters look back: max(1, CHANNELS * DEPTH / 8)                  */
#define MADTP_PNG_I_RAW_BYTES 7    /* HEIGHT * (1 + ROWBYTES): the filtered scanlines the zlib stream must hold                  */
#define MADTP_PNG_I_STREAM_BYTES 8 /* bytes of all IDAT payloads                                                                 */
#define MADTP_PNG_I_PALETTE 9      /* entries of PLTE, 0 without one                                                             */
int madtp_png_prepare(const void* data, int64_t size, int32_t* info, void* palette, void* stream, int64_t stream_capacity);

/* ---- device stage -----------------------------------------------------------------------------------------------------------------
 * One int64 row of MADTP_PNG_FIELDS entries per image (device memory).  Both kernels run one workgroup of MADTP_PNG_LANES lanes
 * (one wave) per image and read row blockIdx.x. */
#define MADTP_PNG_FIELDS 16
#define MADTP_PNG_F_STREAM 0       /* byte offset from `bytes` to the image's zlib stream                                        */
#define MADTP_PNG_F_STREAM_BYTES 1 /* 0 .. 2^31 - 1                                                                              */
#define MADTP_PNG_F_RAW 2          /* byte offset from `raw` to the image's filtered scanlines, % 4 == 0; RAW_BYTES belong to it  */
#define MADTP_PNG_F_RAW_BYTES 3    /* H * (1 + ROWBYTES)                                                                         */
#define MADTP_PNG_F_OUT 4          /* byte offset from `out` to the image's packed RGB [H, W, 3]; 3 * W * H bytes belong to it     */
#define MADTP_PNG_F_W 5            /* 1 .. MADTP_PNG_MAX_SIDE                                                                    */
#define MADTP_PNG_F_H 6
#define MADTP_PNG_F_DEPTH 7
#define MADTP_PNG_F_COLOR 8
#define MADTP_PNG_F_PALETTE 9      /* byte offset from `palette` to the image's 768 bytes                                        */
#define MADTP_PNG_F_CARRY 10       /* byte offset from `out` to 16 * H bytes of scratch of the unfilter kernel, % 16 == 0         */

#define MADTP_PNG_LANES 64
#define MADTP_PNG_WINDOW 32768     /* the inflate kernel's window in LDS                                                         */
#define MADTP_PNG_FLUSH 16384      /* ... which goes to global memory in halves                                                  */
#define MADTP_PNG_BAND 64          /* rows the unfilter kernel runs as one skewed wavefront (one lane per row)                   */
#define MADTP_PNG_TILE 384         /* bytes of a row it stages at a time: a multiple of every BPP                                */

/* Sizes the caller needs (host arithmetic, no GPU): 0 for an argument outside the ranges above. */
int64_t madtp_png_rowbytes(int w, int depth, int color);
int64_t madtp_png_raw_bytes(int w, int h, int depth, int color); /* h * (1 + rowbytes) */
int64_t madtp_png_carry_bytes(int h);                            /* 16 * h             */

/* Status of one image after madtp_png_inflate_batch (int32 [MADTP_PNG_STATUS_FIELDS] per image). */
#define MADTP_PNG_STATUS_FIELDS 4
#define MADTP_PNG_S_CODE 0   /* 0, one of MADTP_PNG_E_* (-208 .. -218), or MADTP_E_BADARG for a table row that breaks a rule above */
#define MADTP_PNG_S_BLOCKS 1 /* deflate blocks begun                                                                              */
#define MADTP_PNG_S_BYTES 2  /* bytes written to raw                                                                              */
#define MADTP_PNG_S_ADLER 3  /* Adler-32 of those bytes (the bits of a uint32)                                                    */

/* madtp_png_inflate_batch: zlib streams -> filtered scanlines.  The wave decodes a stream's symbols uniformly (every lane holds the
 * same bit position and takes the same branch), writes literals and copies LZ77 matches - overlapping ones included - into a
 * MADTP_PNG_WINDOW-byte ring in LDS, takes every match from that ring, and stores the ring to `raw` in halves of MADTP_PNG_FLUSH
 * bytes with all lanes, which is also where the Adler-32 is summed and the filter bytes are checked.  It accepts exactly the
 * streams that zlib's inflate accepts (trailing bytes behind the checksum are ignored, as there) with exactly RAW_BYTES of
 * output.  Every loop is bounded by the stream's bits and the output's bytes, every read is checked against STREAM_BYTES and every
 * write against RAW_BYTES.  No workgroup waits for another, no atomics: identical calls give identical bits.  On a non-zero code
 * the image's raw bytes are unspecified; nothing outside them is written.
 * madtp_png_unfilter_batch: filtered scanlines -> packed RGB.  Lane r of the wave owns row r of a band of MADTP_PNG_BAND rows and
 * runs the filter recurrence along it one pixel behind the lane above (row r at column x while row r - 1 is at x + 1), on a tile
 * of MADTP_PNG_TILE bytes per row staged in LDS; the finished tile is expanded to RGB by all lanes.  `raw` is not modified.  A
 * filter byte above 4 is treated as 0: the caller checks the inflate status (or the bytes) first.
 * MADTP_E_BADARG: a null pointer or B < 1.  A workgroup whose table row breaks a rule above writes nothing (but its status). */
int madtp_png_inflate_batch(const void* bytes, const int64_t* table, void* raw, int32_t* status, int B, void* stream);
int madtp_png_unfilter_batch(const void* raw, const int64_t* table, const void* palette, void* out, int B, void* stream);

/* ---- host emulation ---------------------------------------------------------------------------------------------------------------
 * The routines of the two kernels with the lanes in a `for` loop; no GPU call.  For checking without a GPU - the host's inflate is
 * zlib's.  madtp_png_inflate_host: `stream` -> raw (raw_bytes of capacity, the expected size), status as above; returns the code.
 * madtp_png_unfilter_host: raw (h * (1 + rowbytes) bytes) -> out (3 * w * h bytes); MADTP_PNG_E_FILTER for a filter byte above 4,
 * MADTP_E_BADARG for a geometry outside the ranges. */
int madtp_png_inflate_host(const void* stream, int64_t stream_bytes, void* raw, int64_t raw_bytes, int rowbytes, int32_t* status);
int madtp_png_unfilter_host(const void* raw, int w, int h, int depth, int color, const void* palette, void* out);

#ifdef __cplusplus
}
#endif
#endif /* MADTP_PNG_H */

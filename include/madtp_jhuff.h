/* madtp_jhuff.h - the Huffman entropy stage of the baseline JPEG decode on the device (csrc/jpeg_huff.hip, csrc/jpeg_huff_device.h,
 * linked into libmadtp_hip.so).  The host only parses the header (madtp_jhuff_prepare, microseconds); the compressed bytes cross to
 * the device, one launch decodes every scan of the batch into the int16 coefficient layout of madtp_jpeg_entropy_decode, bit for
 * bit, and madtp_jpeg_idct_batch / madtp_jpeg_rgb_batch (madtp_jpeg.h) read coefficients that never left device memory.
 *
 * A baseline Huffman stream self-synchronises: a decoder started at a wrong bit falls into step with the true symbol sequence after
 * a few symbols (Weissenberger and Schmidt, "Massively Parallel Huffman Decoding on GPUs", ICPP 2018).  One workgroup of
 * MADTP_JHUFF_LANES lanes owns an image from the first pass to the last write:
 *   1. the scan is cut into subsequences of subseq_bytes bytes, one lane each; every lane decodes from the first bit of its
 *      subsequence as if a MCU began there, up to the first symbol that begins in the next subsequence, and keeps that end state
 *      (bit position, block of the MCU, zigzag index) and the number of blocks it completed;
 *   2. synchronisation passes: a lane whose start state differs from its predecessor's end state decodes again from that state;
 *      the passes end when no lane had to, after at most as many passes as there are subsequences (lane i is right after pass i + 1);
 *   3. a prefix sum of the block counts gives every lane the block it starts in;
 *   4. every lane decodes once more, now with the host decoder's exact rules (it knows its MCU number: restart markers are demanded
 *      where the interval puts them and nowhere else, the scan ends after the last MCU) and writes its coefficients, the DC values
 *      still as differences.  The lanes' results are checked as a chain: the first lane, in stream order, that ends in a code gives
 *      the image's code; a lane whose exact end state is not the state its successor started from (only a malformed stream can do
 *      that) sends the image to one lane that decodes it serially, so the answer never rests on a guess;
 *   5. a segmented scan per component in scan order, restarted at every restart interval, turns the differences into DC values,
 *      accumulated in 32 bits, the low 16 stored - the host's (int16_t)pred.
 * An image of more than MADTP_JHUFF_LANES subsequences runs steps 1 - 4 for MADTP_JHUFF_LANES subsequences at a time, each round
 * starting from the exact end state of the round before.  No workgroup waits for another, every loop is bounded by a count known
 * at launch (subsequences, bits of a subsequence, MCUs per lane), every read is checked against the file's size and every write
 * against the image's 64 * BLOCKS coefficients.  No global atomics: identical calls give identical bits.
 *
 * Conventions of madtp_jpeg.h: plain pointers and sizes, nothing allocates, frees or synchronises, launches go to `stream`; 0 on
 * success, a negative code on a rejected argument before any launch, a positive hipError_t if the runtime refuses a launch.  The
 * MADTP_JPEG_E_* codes and MADTP_JPEG_I_* fields are madtp_jpeg.h's.  This header has its own version number; the other headers do
 * not change with it. */
#ifndef MADTP_JHUFF_H
#define MADTP_JHUFF_H

#include "madtp_jpeg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MADTP_JHUFF_ABI_VERSION 1
int madtp_jhuff_abi_version(void);

#define MADTP_JHUFF_LANES 1024          /* lanes of the workgroup that owns an image = subsequences of one round                  */
#define MADTP_JHUFF_MAX_BYTES 268435455 /* largest file (2^28 - 1 bytes): bit positions are 32-bit                               */

/* ---- host stage -------------------------------------------------------------------------------------------------------------------
 * The Huffman record of a file: six tables, [component 0 .. 2][DC, AC], each MADTP_JHUFF_TABLE_BYTES:
 *   uint16 look[512]      (length << 8) | symbol of the code that begins these 9 bits, 0 = longer than 9 bits or none
 *   int32  maxcode[18]    largest code of each length 1 .. 16, -1 = none; [17] = 0x7fffffff
 *   int32  valoffset[18]  index of a code's symbol = code + valoffset[length]
 *   uint8  vals[256]
 * Tables of absent components are 0. */
#define MADTP_JHUFF_TABLE_BYTES 1424
#define MADTP_JHUFF_RECORD_BYTES 8544

/* madtp_jhuff_prepare: the header of the `size` bytes at `data` -> info (int32 [MADTP_JPEG_INFO_FIELDS]) and qtables (uint16
 * [3][64]), both exactly as madtp_jpeg_inspect fills them, with its codes; tables: the MADTP_JHUFF_RECORD_BYTES of the record above
 * (4-byte aligned); scan_begin: offset of the first byte of entropy-coded data.  Touches no GPU state and does not allocate: a
 * loader worker may call it.  MADTP_E_BADARG: a null pointer, a negative size or a size over MADTP_JHUFF_MAX_BYTES. */
int madtp_jhuff_prepare(const void* data, int64_t size, int32_t* info, void* qtables, void* tables, int64_t* scan_begin);

/* ---- device stage -----------------------------------------------------------------------------------------------------------------
 * One int64 row of MADTP_JHUFF_FIELDS entries per image (device memory, the table scheme of madtp_jpeg_idct_batch). */
#define MADTP_JHUFF_FIELDS 16
#define MADTP_JHUFF_F_FILE 0       /* byte offset from `bytes` to the first byte of the file                                      */
#define MADTP_JHUFF_F_SIZE 1       /* bytes of the file, 0 .. MADTP_JHUFF_MAX_BYTES; nothing at or beyond FILE + SIZE is read      */
#define MADTP_JHUFF_F_SCAN 2       /* scan_begin of madtp_jhuff_prepare, 0 .. SIZE                                               */
#define MADTP_JHUFF_F_RECORD 3     /* byte offset from `bytes` to the file's Huffman record, % 4 == 0                             */
#define MADTP_JHUFF_F_COEF 4       /* byte offset from `coef` to the image's coefficients, % 4 == 0 (% 16 for madtp_jpeg_idct_batch) */
#define MADTP_JHUFF_F_COMPONENTS 5 /* 1 or 3                                                                                      */
#define MADTP_JHUFF_F_HS 6
#define MADTP_JHUFF_F_VS 7
#define MADTP_JHUFF_F_BLOCKS_X 8   /* of the luma plane, a multiple of HS                                                         */
#define MADTP_JHUFF_F_BLOCKS_Y 9   /* of the luma plane, a multiple of VS                                                         */
#define MADTP_JHUFF_F_RESTART 10   /* restart interval in MCUs, 0 = none                                                          */

/* status: int32 [B][MADTP_JHUFF_STATUS_FIELDS] */
#define MADTP_JHUFF_STATUS_FIELDS 4
#define MADTP_JHUFF_S_CODE 0       /* 0, or the MADTP_JPEG_E_* that madtp_jpeg_entropy_decode returns for the file; MADTP_E_BADARG */
/*                                    for a table row that breaks a rule above (nothing of the image is read or written then)     */
#define MADTP_JHUFF_S_PASSES 1     /* decoding passes of steps 1 and 2 over all rounds, at most SUBSEQS                           */
#define MADTP_JHUFF_S_SUBSEQS 2    /* subsequences: max(1, ceil((SIZE - SCAN) / subsequence bytes))                               */
#define MADTP_JHUFF_S_SERIAL 3     /* 1 if the chain check sent the image to the serial lane                                      */

/* The subsequence size the library chooses for a scan of scan_bytes bytes (subseq_bytes = 0): the smallest multiple of 4 that is
 * at least 32 bytes (a lane should hold a few dozen symbols, or the passes cost more than they spread) and leaves the image at most
 * MADTP_JHUFF_LANES subsequences, so that it is decoded in one round.  0 for a negative argument. */
int madtp_jhuff_subseq_bytes(int64_t scan_bytes);

/* madtp_jhuff_decode_batch: one workgroup per image.  coef receives exactly what madtp_jpeg_entropy_decode writes: component after
 * component, each [blocks_y][blocks_x][64], de-zigzagged, column-major within a block, not dequantised; blocks that the stream
 * leaves at zero are zero.  On a code other than 0 the content of the image's coefficients is unspecified; nothing outside its
 * 64 * BLOCKS elements is ever written.  subseq_bytes: 0 for the library's choice per image, else a multiple of 4, at least 4.
 * MADTP_E_BADARG: a null pointer, B < 1, or such a subseq_bytes. */
int madtp_jhuff_decode_batch(const void* bytes, const int64_t* table, void* coef, int32_t* status, int B, int subseq_bytes, void* stream);

/* madtp_jhuff_decode_host: the same lane routines and the same passes with the lanes in a loop, on the host, for one file: no GPU
 * call.  status: int32 [MADTP_JHUFF_STATUS_FIELDS].  Returns status[0] (a header code of madtp_jhuff_prepare likewise), or
 * MADTP_E_BADARG for a null pointer, such a subseq_bytes, or a coef_capacity (int16 elements) under 64 * BLOCKS; nothing is
 * written to coef then. */
int madtp_jhuff_decode_host(const void* data, int64_t size, int subseq_bytes, void* coef, int64_t coef_capacity, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* MADTP_JHUFF_H */

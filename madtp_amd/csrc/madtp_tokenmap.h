/* madtp_tokenmap.h - token maps: what every layer's output slots stand for in the coordinates of the encoder's INPUT (patches, or
 * the text tokens behind row 0), composed on the device from the prune records a forward leaves behind (csrc/tokenmap.hip, linked
 * into libmadtp_hip.so; the lane routines of csrc/tokenmap_device.h, which the host emulation below runs as well).
 *
 * An encoder run has L layers over n0 prunable positions; row 0 (CLS / [ENC]) is never pruned and is not part of the map.  A pruned
 * layer with input length n_in and k kept tokens has k + 1 output slots: slot i < k holds input position indices[b, i], slot k is
 * the merged token over indices_sort[b, k .. n_in) with the weights w_j = score_j / (sum of the pruned scores + 1e-8) - the merge_w
 * of madtp_token_select, summed in its order.  An unpruned layer is the identity.  After every layer the original positions form a
 * partition over the slots, so one (slot, coef) pair per position describes a layer, and every position's chain is independent:
 *   slot  int32 [B, L, n0]  in [0, n_l): row slot + 1 of the layer's output
 *   coef  f32   [B, L, n0]  the product of the merge weights the position has passed through; exactly 1.0 while it owns its slot
 *   depth int32 [B, n0]     the number of leading layers after which the position still owned a slot alone, 0 .. L; the position
 *                           is "kept at layer l" iff depth > l
 *
 * Conventions of madtp_hip.h: plain pointers and sizes, nothing allocates, frees or synchronises, launches go to `stream` (a
 * hipStream_t passed as void*); 0 on success, a negative code on a rejected argument before any launch, a positive hipError_t if the
 * runtime refuses a launch.  No float or global atomics and no workgroup that waits for another: identical calls give identical
 * bits.  Every index read from a record or a map is checked before it addresses anything, and every loop is bounded by a count
 * known at launch.  This header has its own version number; the other headers do not change with it.  It lives next to the sources
 * that implement it: the file list of include/ is pinned by a test of the candidate lists. */
#ifndef MADTP_TOKENMAP_H
#define MADTP_TOKENMAP_H

#include "../../include/madtp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MADTP_TOKENMAP_ABI_VERSION 1
int madtp_tokenmap_abi_version(void);

#define MADTP_TOKENMAP_MAX_N 4096     /* positions of a sample: n0, and so every n_in                                          */
#define MADTP_TOKENMAP_MAX_LAYERS 48
#define MADTP_TOKENMAP_MAX_BATCH 65535
#define MADTP_TOKENMAP_MAX_C 65536    /* channels of a pushed / pulled tensor                                                  */
#define MADTP_TOKENMAP_LANES 256      /* of every workgroup here                                                               */

/* ---- codes of a record the build refuses (in the status word) ------------------------------------------------------------------- */
#define MADTP_TOKENMAP_E_RANGE (-301)  /* an index of indices[:k] / indices_sort[k:n_in] outside [0, n_in)                      */
#define MADTP_TOKENMAP_E_REPEAT (-302) /* an index that occurs twice in indices[:k] + indices_sort[k:n_in]                      */
#define MADTP_TOKENMAP_E_K (-303)      /* k outside 1 .. n_in - 1 (and not -1)                                                  */
#define MADTP_TOKENMAP_E_CHAIN (-304)  /* n_in is not what the layer before left (n0 for the first, k + 1 after a pruned one)   */
#define MADTP_TOKENMAP_E_TABLE (-305)  /* a null pointer in the row of a pruned layer, or a row stride below what is read       */
const char* madtp_tokenmap_strerror(int code);

/* status word of a sample: 0, or -((-code << 6) | layer) with one of the codes above and the first layer that breaks a rule */
#define MADTP_TOKENMAP_STATUS_LAYER_BITS 6

/* ---- build -----------------------------------------------------------------------------------------------------------------------
 * table: L rows of MADTP_TOKENMAP_FIELDS int64 (device memory; the host emulation: host memory), one per layer.  The record tensors
 * are buffers of at least the row stride given: indices' first K columns count, indices_sort's and score's first N_IN. */
#define MADTP_TOKENMAP_FIELDS 8
#define MADTP_TOKENMAP_F_N_IN 0           /* prunable positions entering the layer                                              */
#define MADTP_TOKENMAP_F_K 1              /* kept tokens, or -1: the layer did not prune (the pointers are not read)            */
#define MADTP_TOKENMAP_F_INDICES 2        /* const int64_t*: [B, stride] kept positions, slot order                             */
#define MADTP_TOKENMAP_F_INDICES_STRIDE 3 /* elements between samples, >= K                                                     */
#define MADTP_TOKENMAP_F_SORT 4           /* const int64_t*: [B, stride] every position in descending order of score            */
#define MADTP_TOKENMAP_F_SORT_STRIDE 5    /* >= N_IN                                                                            */
#define MADTP_TOKENMAP_F_SCORE 6          /* const float*: [B, stride] the scores the layer pruned by                           */
#define MADTP_TOKENMAP_F_SCORE_STRIDE 7   /* >= N_IN                                                                            */

/* One workgroup per sample walks the layers twice: first checking every record (the first broken rule goes to status[b] and the
 * sample's slot / coef / depth are NOT written), then composing.  Per pruned layer the lanes invert indices[:k] + indices_sort[k:]
 * into a position table in LDS (a range check before the write, a read-back that finds repeats), sum the pruned scores as
 * madtp_token_select does (lane t adds positions t, t + 256, ... in that order, then its butterfly and the four wave sums in
 * order) and advance their own positions p, p + 256, ... from the previous layer's row of the map, which the same lane wrote.
 * MADTP_E_BADARG: a null pointer, L outside 1 .. MAX_LAYERS, B outside 1 .. MAX_BATCH, n0 outside 1 .. MAX_N. */
int madtp_tokenmap_build(const int64_t* table, int L, int B, int n0, int32_t* slot, float* coef, int32_t* depth, int32_t* status,
                         void* stream);

/* ---- push: the pruning replayed on any per-position tensor ------------------------------------------------------------------------
 * y[b, s, :] = sum over the positions p with slot[b, p] == s, in ascending p, of coef[b, p] * x[b, p, :] (one fused multiply-add per
 * cell), zero for a slot nothing maps to.  x: f32, element (b, p, c) at x[b * x_sb + p * x_sp + c]; slot / coef: one layer's rows
 * of a map, sample b's at + b * map_sb; y: f32 [B, n_out, C] contiguous.  A workgroup sorts its sample's (slot, p) pairs with a
 * stable counting sort (4-bit digits) in LDS; a wave then owns a (slot, 64-lane column block) unit and walks the slot's cells in
 * order.  A position whose slot is outside [0, n_out) contributes nothing.  C % 4 == 0 with x_sb, x_sp % 4 == 0 and 16-byte aligned
 * x, y takes the 16-byte path.  MADTP_E_BADARG: a null pointer or a size outside the ranges above (n_out: 1 .. MAX_N). */
int madtp_tokenmap_push(const float* x, int64_t x_sb, int64_t x_sp, const int32_t* slot, const float* coef, int64_t map_sb, float* y,
                        int B, int n0, int n_out, int C, void* stream);

/* ---- pull: the transpose, a gather ----------------------------------------------------------------------------------------------
 * out[b, p, :] = v[b, slot[b, p], :], times coef[b, p] when weighted; v f32 [B, n_l, C], out f32 [B, n0, C], both contiguous.  A
 * slot outside [0, n_l) gives a row of zeros. */
int madtp_tokenmap_pull(const float* v, const int32_t* slot, const float* coef, int64_t map_sb, float* out, int B, int n0, int n_l,
                        int C, int weighted, void* stream);

/* ---- agree: two maps' kept sets in original coordinates ---------------------------------------------------------------------------
 * depth_a, depth_b: int32 [B, n0] (values outside 0 .. L are clamped).  out: int32 [B, L, 2]: per layer the size of the
 * intersection and of the union of {p: depth > l}, from the histograms of min / max depth and their suffix sums. */
int madtp_tokenmap_agree(const int32_t* depth_a, const int32_t* depth_b, int32_t* out, int B, int n0, int L, void* stream);

/* ---- shade: the kept-patch figure ---------------------------------------------------------------------------------------------------
 * images, out: uint8 [B, gh * ph, gw * pw, 3], 16-byte aligned, (gh * ph * gw * pw * 3) % 16 == 0 (MADTP_E_ALIGN otherwise); depth:
 * int32 [B, gh * gw]; level: uint8 [L + 1].  out = (pix * level[clamp(depth[patch], 0, L)] + 127) / 255 in integer arithmetic; each
 * lane loads and stores 16 bytes.  Sides up to 16384. */
int madtp_tokenmap_shade(const void* images, const int32_t* depth, const void* level, void* out, int B, int gh, int gw, int ph, int pw,
                         int L, void* stream);

/* ---- host emulation -----------------------------------------------------------------------------------------------------------------
 * The same lane routines with the lanes (and the workgroups) in `for` loops; every pointer is host memory, the table's included; no
 * GPU call.  For checking without a GPU. */
int madtp_tokenmap_build_host(const int64_t* table, int L, int B, int n0, int32_t* slot, float* coef, int32_t* depth, int32_t* status);
int madtp_tokenmap_push_host(const float* x, int64_t x_sb, int64_t x_sp, const int32_t* slot, const float* coef, int64_t map_sb,
                             float* y, int B, int n0, int n_out, int C);
int madtp_tokenmap_pull_host(const float* v, const int32_t* slot, const float* coef, int64_t map_sb, float* out, int B, int n0,
                             int n_l, int C, int weighted);
int madtp_tokenmap_agree_host(const int32_t* depth_a, const int32_t* depth_b, int32_t* out, int B, int n0, int L);
int madtp_tokenmap_shade_host(const void* images, const int32_t* depth, const void* level, void* out, int B, int gh, int gw, int ph,
                              int pw, int L);

#ifdef __cplusplus
}
#endif
#endif /* MADTP_TOKENMAP_H */

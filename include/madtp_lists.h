/* madtp_lists.h - re-ranked candidate lists on the device (csrc/lists.hip, linked into libmadtp_hip.so): what stage 2 of BLIP's
 * two-stage retrieval leaves behind, ranked and ordered without the dense [n, nk] score matrix it stands for.
 *
 * A CANDIDATE LIST of a row is k slots (1 <= k <= MADTP_LISTS_MAX_K): idx int64 [n, k] and val f32 [n, k], each with a row stride
 * in elements (>= k).  A slot with idx == -1 is empty and its value is ignored (so is a slot whose index lies outside [0, nk):
 * the kernels never read or write through an index).  A filled slot has 0 <= idx < nk, and no key occurs twice in a row - the
 * caller's precondition.  The list stands for the dense row
 *       s_j = val of the slot that holds j,    s_j = fill for every key j in no slot.
 *
 *   madtp_lists_rank   the ranks of the ground-truth keys of every row, exactly as madtp_rank_scores writes them for that dense
 *                      row:  rank(t) = #{j != t : s_j > s_t} + #{j > t : s_j == s_t}, floats compared as IEEE floats (a NaN
 *                      beats nothing and is beaten by nothing, -0 ties with +0).  Same CSR targets (tgt_ptr int32 [n + 1],
 *                      tgt_idx int32, at most MADTP_LISTS_MAX_TARGETS per row, later ones ignored), same outputs: rank_tgt per
 *                      target (nk for a target outside [0, nk)), rank_row the minimum of the row (nk for a row without targets).
 *                      The keys in no slot are counted, not visited: the work per row is O(k * targets), whatever nk is.
 *   madtp_lists_sort   every row in the order of madtp_search.h: value descending, equal values by key index DESCENDING, -0 and
 *                      +0 tie, NaN below every number (among NaNs by index descending), empty slots last as idx -1, val -inf.
 *                      Values come out as madtp_topk_embeds reports them: a zero as +0, a NaN as the canonical quiet NaN, every
 *                      other value with its bits.  out_idx int64 [n, k] and out_val f32 [n, k] are contiguous and must not
 *                      overlap the inputs.  For a row without NaN values, a target held in a slot whose value is above `fill`
 *                      sits at position madtp_lists_rank gives it.
 *
 * Conventions of madtp_hip.h: nothing allocates, frees or synchronises, launches go to `stream`; 0 on success, a negative MADTP_E_*
 * code on a rejected argument before any launch, a positive hipError_t if the runtime refuses the launch.  No float atomics, no
 * global atomics and no atomics at all: integer counts summed over the lanes of one wave, a sorting network on 64-bit words that
 * are a total order.  Identical calls give identical bits.  This header has its own version number; no other header changes with
 * it. */
#ifndef MADTP_LISTS_H
#define MADTP_LISTS_H

#include "madtp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MADTP_LISTS_ABI_VERSION 1
int madtp_lists_abi_version(void);

#define MADTP_LISTS_MAX_K 256
#define MADTP_LISTS_MAX_TARGETS 16

/* rank_row int32 [n], rank_tgt int32 [tgt_ptr[n]].  MADTP_E_BADARG: a null pointer, k outside [1, MADTP_LISTS_MAX_K].
 * MADTP_E_SHAPE: n < 1, nk < 1, ld_idx or ld_val below k. */
int madtp_lists_rank(const int64_t* idx, int64_t ld_idx, const float* val, int64_t ld_val, int n, int k, int nk, float fill,
                     const int32_t* tgt_ptr, const int32_t* tgt_idx, int32_t* rank_row, int32_t* rank_tgt, void* stream);

/* MADTP_E_BADARG: a null pointer, k outside [1, MADTP_LISTS_MAX_K], an output that overlaps an input.  MADTP_E_SHAPE: n < 1,
 * nk < 1, ld_idx or ld_val below k. */
int madtp_lists_sort(const int64_t* idx, int64_t ld_idx, const float* val, int64_t ld_val, int n, int k, int nk, int64_t* out_idx,
                     float* out_val, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MADTP_LISTS_H */

/* madtp_search.h - retrieval search on the device: the top-k gallery items of every query, from the embeddings
 * (csrc/search.hip, linked into libmadtp_hip.so).  It is what a retrieval model does after training, and stage 1 of BLIP's
 * two-stage evaluate() (compress_retrieval_dtp.py:155-198: sims_matrix[i].topk(k_test) per row).
 *
 *   madtp_topk_embeds   q f32 [nq, ldq], keys f32 [nk, ldk] -> the k keys with the largest <q_r, keys_j> of every row r.  No
 *                       [nq, nk] matrix is written anywhere: the selection runs in the epilogue of the products.
 *   madtp_topk_scores   the same selection on a given dense f32 matrix [nq, ld >= nk] (the counterpart of madtp_rank_scores)
 *
 * THE CONTRACT
 *   scores  madtp_topk_embeds forms <q_r, keys_j> with the product routine of madtp_rank_embeds (csrc/eval_device.h, exact f32
 *           products on v_mfma_f32_16x16x4_f32, a function of the two rows alone): the value reported for (r, j) has the bits of
 *           the score_tgt that madtp_rank_embeds reports for that pair.
 *   order   score descending, equal scores by key index DESCENDING: position p of a row is element p of
 *           np.argsort(s, kind="stable")[::-1], the rule of madtp_rank_embeds.  So for a row without NaN scores a target whose
 *           rank from madtp_rank_embeds is rho < k sits at position rho, and a target with rho >= k is absent.
 *   ties    scores compare as IEEE floats: -0 and +0 tie (and are ordered by index).
 *   NaN     a NaN score ranks below every number, -inf included; among NaNs the order is by index descending.  madtp_topk_embeds
 *           reports such a value as the canonical quiet NaN, madtp_topk_scores as the matrix holds it.
 *   fill    when k > nk, positions nk .. k - 1 of every row hold index -1 and value -inf.
 *
 * Conventions of madtp_hip.h: nothing allocates, frees or synchronises, launches go to `stream`; 0 on success, a negative MADTP_E_*
 * code on a rejected argument before any launch, a positive hipError_t if the runtime refuses the launch.  No float atomics and no
 * global atomics; the integer LDS atomics hand out slots of a candidate buffer that is then cut by the total order (score, index),
 * which no arrival order can change: identical calls give identical bits.  This header has its own version number; madtp_hip.h,
 * madtp_image.h, madtp_augment.h and madtp_jpeg.h do not change with it. */
#ifndef MADTP_SEARCH_H
#define MADTP_SEARCH_H

#include "madtp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MADTP_SEARCH_ABI_VERSION 1
int madtp_search_abi_version(void);

#define MADTP_TOPK_MAX_K 256

/* Bytes of workspace madtp_topk_embeds needs (the sorted candidate lists of the key splits, merged by a second launch); 0 for
 * arguments the call would refuse.  Monotone in nq, nk and k. */
size_t madtp_topk_workspace(int nq, int nk, int D, int k);

/* values f32 [nq, k], indices int32 [nq, k], best first.  MADTP_E_BADARG: a null pointer, k outside [1, MADTP_TOPK_MAX_K], a base
 * of q or keys that is not 16-byte aligned, ws_bytes < madtp_topk_workspace(nq, nk, D, k).  MADTP_E_SHAPE: nq < 1, nk < 1,
 * D % 64 != 0, D outside [64, 1024], ldq or ldk below D or not a multiple of 4. */
int madtp_topk_embeds(const float* q, int ldq, const float* keys, int ldk, int nq, int nk, int D, int k, float* values, int32_t* indices,
                      void* ws, size_t ws_bytes, void* stream);

/* scores f32 [nq, ld] row-major, the first nk entries of a row are its scores; one workgroup per row, the row read once.
 * MADTP_E_BADARG: a null pointer, k outside [1, MADTP_TOPK_MAX_K].  MADTP_E_SHAPE: nq < 1, nk < 1, ld < nk. */
int madtp_topk_scores(const float* scores, int ld, int nq, int nk, int k, float* values, int32_t* indices, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MADTP_SEARCH_H */

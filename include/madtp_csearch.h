/* madtp_csearch.h - retrieval search through a bf16 shortlist with an exactness certificate (csrc/search_coarse.hip, linked into
 * libmadtp_hip.so).  madtp_ctopk_embeds returns, for EVERY input, the values and indices madtp_topk_embeds (madtp_search.h)
 * returns: same order, same value bits.  What changes is the route:
 *
 *   prepare   f32 rows -> bf16 rows (round to nearest even) and four f32 statistics per row (madtp_coarse_prepare); the gallery's
 *             statistics reduce to a summary of four words (madtp_coarse_summary).  Once per gallery, every call for the queries.
 *   coarse    <q16_r, y16_j> on v_mfma_f32_16x16x32_bf16 (16x the rate of the exact f32 products); the selection of madtp_search.h
 *             keeps the m best coarse scores of every row: the shortlist.
 *   row       the m shortlisted keys are scored again with the exact route's arithmetic (the fmaf chain of csrc/eval_device.h, so
 *             the bits are those madtp_topk_embeds reports for the pair), sorted by the contract's order, and the row's
 *             certificate is evaluated.
 *   fallback  rows without a certificate are listed (ordered scan, no atomics) and go through the kernels of madtp_topk_embeds in
 *             the same call.  No answer rests on a guess.
 *
 * THE CERTIFICATE
 *   Write c(j) for the coarse score of key j as the coarse stage computed it, s(j) for the exact route's score, c_m for the m-th
 *   best coarse score of the row and s_k for the k-th best exact score among the shortlisted.  Every key j outside the shortlist
 *   has c(j) <= c_m (the selection's order: a key with a smaller word lost to m others).  If |s(j) - c(j)| <= E_r for every key j,
 *   such a key has s(j) <= c_m + E_r, so when
 *
 *       s_k > c_m + E_r                     (strictly)
 *
 *   k shortlisted keys beat every key outside in the exact order - strictly, so no tie-break by index is involved - and the exact
 *   top-k is the top-k of the shortlist.  The row is then CERTIFIED.  A tie across the shortlist's boundary is never certified.
 *
 * THE BOUND  (u = 2^-24; x16 the bf16 rounding of x; norms Euclidean; Y = max_j |y_j|, dY = max_j |y_j - y16_j|,
 *             Y16 = max_j |y16_j|; for row r: a_r = |q_r - q16_r|, b_r = |q16_r|)
 *   Proof, for finite operands without overflow (see "never certified" below).  With <.,.> the real inner product:
 *     (1) <q, y> - <q16, y16> = <q - q16, y> + <q16, y - y16>, so by Cauchy-Schwarz |(1)| <= a_r Y + b_r dY.
 *     (2) the exact route forms s(j) as a chain of D fmaf, one rounding each (eval_device.h): the standard bound for recursive
 *         summation of D exactly formed products gives |s(j) - <q, y>| <= gamma_D sum_i |q_i y_i| <= (D + 2) u |q_r| Y
 *         (gamma_D = D u / (1 - D u) <= (D + 2) u for D <= 1024; Cauchy-Schwarz again).
 *     (3) a product of two bf16 numbers is exact in f32 (8 + 8 significand bits); the matrix unit adds D of them to an f32
 *         accumulator in an order and with intermediate roundings that are not documented.  Any summation of D terms that rounds
 *         every intermediate to no fewer than 24 bits satisfies |c(j) - <q16, y16>| <= (D - 1) u' sum |.| with u' <= 2 u; A = 4
 *         leaves a factor of two on top of that:  |c(j) - <q16, y16>| <= A D u b_r Y16.  It is measured, not derived:
 *         tests/test_search_coarse_gpu.py asserts it for every shortlisted pair and README.md records the largest ratio seen.
 *     (4) results below the normal range: every rounding of (2) and (3) may also lose up to 2^-126 absolutely (a flushed or
 *         gradually underflowed intermediate): U = 3 D 2^-126 covers the D roundings of (2) and 2 D of (3).
 *   Hence
 *       E_r = (a_r Y + b_r dY + (D + 2) u |q_r| Y + A D u b_r Y16) (1 + 2^-10) + U .
 *   The factor (1 + 2^-10) pays for the roundings of evaluating E_r in f32 and of the comparison, which is made in f64; the
 *   statistics themselves are rounded UP by madtp_coarse_prepare.
 *
 * NEVER CERTIFIED (the row goes to the fallback)
 *   - a row whose statistics carry the flag, or a gallery whose summary carries it.  The flag is set for a row that holds a
 *     non-finite element, an element whose bf16 rounding overflows, or a non-zero element below the normal range 2^-126 (the
 *     matrix unit may read such an operand as zero, which no term above covers);
 *   - |q_r| Y >= 2^126 or b_r Y16 >= 2^126 (or NaN): below that no partial sum of either route can overflow;
 *   - s_k or c_m NaN; s_k <= c_m + E_r.
 *   When nk <= m every key is shortlisted and a row without the flag is certified.
 *
 * Conventions of madtp_hip.h: nothing allocates, frees or synchronises, launches go to `stream`; 0 on success, a negative MADTP_E_*
 * code on a rejected argument before any launch, a positive hipError_t if the runtime refuses the launch.  No float atomics and no
 * global atomics (the integer LDS atomics of madtp_search.h's selection only): identical calls give identical bits.  This header
 * has its own version number; madtp_hip.h, madtp_search.h and the other side headers do not change with it. */
#ifndef MADTP_CSEARCH_H
#define MADTP_CSEARCH_H

#include "madtp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MADTP_CSEARCH_ABI_VERSION 1
int madtp_csearch_abi_version(void);

#define MADTP_CTOPK_MAX_K 128
/* the constant A of term (3) */
#define MADTP_CTOPK_ACC_FACTOR 4
/* f32 words of a row's statistics {|x|, |x - x16|, |x16|, flag (0 or 1)} and of a summary {Y, dY, Y16, flag} */
#define MADTP_COARSE_STATS 4
/* int32 / f32 words of a row of `info`: {certified (int32 0 / 1), c_m (f32), E_r (f32), position in the fallback list or -1} */
#define MADTP_CTOPK_INFO 4

/* x f32 [n, ldx] -> x16 bf16 [n, D] (dense rows) and stats f32 [n, MADTP_COARSE_STATS].  Every norm is rounded so that it is an
 * upper bound of the real one (it is computed on the row scaled by a power of two, so neither 1e-30 nor 1e+30 rows lose it).
 * MADTP_E_BADARG: a null pointer, a base of x or x16 that is not 16-byte aligned.  MADTP_E_SHAPE: n < 1, D % 64 != 0, D outside
 * [64, 1024], ldx below D or not a multiple of 4. */
int madtp_coarse_prepare(const float* x, int ldx, int n, int D, void* x16, float* stats, void* stream);

/* summary[i] = max over the n rows of stats[., i] (one workgroup, a fixed order; max is associative, so it does not matter).
 * fold != 0: the maximum also runs over the summary's own four words, which is how rows appended to a gallery are taken in.
 * MADTP_E_BADARG: a null pointer.  MADTP_E_SHAPE: n < 1. */
int madtp_coarse_summary(const float* stats, int n, float* summary, int fold, void* stream);

/* Bytes of workspace madtp_ctopk_embeds needs; 0 for arguments the call would refuse.  Monotone in nq, nk and k. */
size_t madtp_ctopk_workspace(int nq, int nk, int D, int k, int m);

/* values f32 [nq, k], indices int32 [nq, k], best first, equal to madtp_topk_embeds' for the same q, keys and k.
 *   keys16              bf16 [nk, D] and
 *   key_stats_summary   f32 [MADTP_COARSE_STATS], both from madtp_coarse_prepare / madtp_coarse_summary on `keys`
 *   m                   the shortlist: 64, 128 or 256, and m >= 2 k
 *   info                [nq, MADTP_CTOPK_INFO] words, see above
 *   shortlist_indices   optional int32 [nq, m] and
 *   shortlist_coarse    optional f32 [nq, m] (both or neither): the shortlist, best coarse score first; -1 / -inf past nk keys
 * After the call the first int32 of ws holds the number of uncertified rows and is followed, at byte 16, by their ascending list.
 * MADTP_E_BADARG: a null pointer among the required ones, one shortlist pointer without the other, k outside
 * [1, MADTP_CTOPK_MAX_K], m not one of 64 / 128 / 256 or m < 2 k, a base of q, keys, keys16 or ws that is not 16-byte aligned,
 * ws_bytes < madtp_ctopk_workspace(nq, nk, D, k, m).  MADTP_E_SHAPE: as madtp_topk_embeds. */
int madtp_ctopk_embeds(const float* q, int ldq, const float* keys, int ldk, const void* keys16, const float* key_stats_summary, int nq,
                       int nk, int D, int k, int m, float* values, int32_t* indices, int32_t* info, int32_t* shortlist_indices,
                       float* shortlist_coarse, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MADTP_CSEARCH_H */

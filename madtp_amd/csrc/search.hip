// Retrieval search (include/madtp_search.h): the top-k keys of every query row, selected on the device.
//
// The selection itself - the candidate words, the sort, both kernels - is csrc/search_device.h, shared with search_coarse.hip.
//
// A candidate is ONE 64-bit word: (order-preserving image of the f32 score) << 32 | key index.  Comparing the words as unsigned
// integers is the contract's total order - score descending, equal scores by index descending, NaN below every number, 0 = "no
// candidate" below everything - and no two candidates of a row are equal, so "the k largest words, sorted" has one answer,
// whatever order the candidates arrived in.
//
//   topk_tile_kernel   workgroup (32 query rows, key split): rank_tile_products (csrc/eval_device.h, the product routine of
//                      madtp_rank_embeds) forms a 32 x 64 score tile; a score above its row's threshold (the k-th best so far)
//                      takes a slot of the row's candidate buffer in LDS (integer LDS atomic).  When a buffer could overflow in
//                      the next tile, every row is sorted (bitonic, in LDS), cut to its best k, and the threshold moves up.
//                      The split's sorted k words per row go to the workspace.
//   topk_row_kernel    one workgroup per row streams words through the same threshold / buffer / sort-and-cut scheme: the
//                      splits' lists of a row (the merge of madtp_topk_embeds) or a row of a dense score matrix
//                      (madtp_topk_scores), and writes values and indices.
#include "search_device.h"

#include "../../include/madtp_search.h"

extern "C" int madtp_search_abi_version(void) { return MADTP_SEARCH_ABI_VERSION; }

extern "C" size_t madtp_topk_workspace(int nq, int nk, int D, int k) {
    if (!topk_shape_ok(nq, nk, D) || k < 1 || k > MADTP_TOPK_MAX_K) return 0;
    return sizeof(u64) * (size_t)k * topk_geometry(nq, nk).ws_rows;
}

extern "C" int madtp_topk_embeds(const float* q, int ldq, const float* keys, int ldk, int nq, int nk, int D, int k, float* values,
                                 int32_t* indices, void* ws, size_t ws_bytes, void* stream) {
    if (!q || !keys || !values || !indices || !ws) return MADTP_E_BADARG;
    if (k < 1 || k > MADTP_TOPK_MAX_K) return MADTP_E_BADARG;
    if (!topk_shape_ok(nq, nk, D) || ldq < D || ldk < D || ldq % 4 != 0 || ldk % 4 != 0) return MADTP_E_SHAPE;
    if (!aligned16(q) || !aligned16(keys) || ((uintptr_t)ws & 7u) != 0) return MADTP_E_BADARG;
    if (ws_bytes < madtp_topk_workspace(nq, nk, D, k)) return MADTP_E_BADARG;
    const TopkGeometry g = topk_geometry(nq, nk);
    RankArgs a = {};
    a.q = q; a.keys = keys; a.ldq = ldq; a.ldk = ldk; a.nq = nq; a.nk = nk; a.D = D;
    a.splits = g.splits; a.tiles_per_split = g.tiles_per_split;
    hipStream_t s = (hipStream_t)stream;
    u64* part = (u64*)ws;
    int rc;
    if (k <= 64) rc = launch_topk_tiles<128>(a, k, g, part, s);
    else if (k <= 128) rc = launch_topk_tiles<256>(a, k, g, part, s);
    else rc = launch_topk_tiles<512>(a, k, g, part, s);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(topk_row_kernel<false>, dim3(nq), dim3(RK_THREADS), 0, s, (const float*)nullptr, (size_t)0, part, nq,
                       g.splits * k, k, values, indices);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" int madtp_topk_scores(const float* scores, int ld, int nq, int nk, int k, float* values, int32_t* indices, void* stream) {
    if (!scores || !values || !indices) return MADTP_E_BADARG;
    if (k < 1 || k > MADTP_TOPK_MAX_K) return MADTP_E_BADARG;
    if (nq <= 0 || nk <= 0 || ld < nk) return MADTP_E_SHAPE;
    hipLaunchKernelGGL(topk_row_kernel<true>, dim3(nq), dim3(RK_THREADS), 0, (hipStream_t)stream, scores, (size_t)ld, (const u64*)nullptr,
                       nq, nk, k, values, indices);
    MADTP_LAUNCH_CHECK();
    return 0;
}

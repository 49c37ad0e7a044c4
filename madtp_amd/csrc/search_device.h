// The selection routines of the retrieval search, shared by search.hip (the exact route of include/madtp_search.h) and
// search_coarse.hip (the bf16 shortlist of include/madtp_csearch.h, whose fallback runs the exact kernels over a list of rows).
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
//
// MAPPED (the fallback of madtp_ctopk_embeds): the kernels run over the rows a device-side list names - RankArgs.row_map /
// row_count (eval_device.h).  Position p of the list is query row row_map[p]; the grid is sized for nq rows and a workgroup past
// *row_count returns at once; the lists of the splits are indexed by p and the results go to row row_map[p].  A row's result is a
// function of that row and the keys alone, so which rows share a workgroup changes nothing.
#pragma once
#include <algorithm>

#include "eval_device.h"

namespace {

typedef unsigned long long u64;

constexpr int TK_MAX_SPLITS = 256;
constexpr int TK_MIN_TILES = 4;      // key tiles a split holds at least: 256 keys behind every list of k words
constexpr int TK_WORKGROUPS = 1024;  // row tiles x splits aimed at: 4 per CU
constexpr int TK_ROW_CAP = 512;      // candidate words of topk_row_kernel: k <= 256 kept + a chunk of 256 new ones

__device__ __forceinline__ uint32_t score_bits(float s) {
    if (s != s) return 1u;  // below -inf (0x007fffff), above "no candidate" (0)
    const uint32_t u = s == 0.f ? 0u : __float_as_uint(s);  // -0 ties with +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bits_score(uint32_t b) {
    if (b == 1u) return __builtin_nanf("");
    return __uint_as_float((b & 0x80000000u) ? (b & 0x7fffffffu) : ~b);
}
__device__ __forceinline__ u64 candidate(float s, int index) { return ((u64)score_bits(s) << 32) | (uint32_t)index; }

// One stage (k2, j) of the bitonic network on PPR pairs of every row, the pairs of the words [OFF, OFF + 2 PPR) of a row.  A thread
// takes its pairs eight at a time: the sixteen LDS reads are in flight together (one wave per SIMD is all the k = 256 kernel has
// to hide their latency with), then the exchanges.
template <int CAP, int ROWS, int PPR, int OFF> __device__ __forceinline__ void sort_stage(u64* buf, int k2, int j) {
    constexpr int PER = ROWS * PPR / RK_THREADS, U = PER < 8 ? PER : 8;
    static_assert(ROWS * PPR % RK_THREADS == 0 && PER % U == 0, "every thread has the same whole number of batches");
    for (int b = 0; b < PER; b += U) {
        int lo[U];
        u64 x[U], y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = (b + u) * RK_THREADS + threadIdx.x, i = p % PPR;
            lo[u] = (p / PPR) * CAP + OFF + (((i & ~(j - 1)) << 1) | (i & (j - 1)));
            x[u] = buf[lo[u]];
            y[u] = buf[lo[u] + j];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool desc = (lo[u] & k2) == 0 || k2 == CAP;  // (row * CAP has no bit below CAP; the last merge is descending)
            if ((x[u] < y[u]) == desc) {
                buf[lo[u]] = y[u];
                buf[lo[u] + j] = x[u];
            }
        }
    }
    __syncthreads();
}

// ROWS x CAP words in LDS, every row sorted descending by all RK_THREADS threads (CAP a power of two).  NEWHALF: the first half
// of every row is sorted descending already, which is what the network makes of it before its last merge: the stages before
// that merge run on the second half alone (27 instead of 45 full stages at CAP = 512).
template <int CAP, int ROWS, bool NEWHALF> __device__ __forceinline__ void sort_rows_desc(u64* buf) {
    for (int k2 = 2; k2 < CAP; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            if constexpr (NEWHALF) sort_stage<CAP, ROWS, CAP / 4, CAP / 2>(buf, k2, j);
            else sort_stage<CAP, ROWS, CAP / 2, 0>(buf, k2, j);
        }
    for (int j = CAP >> 1; j > 0; j >>= 1) sort_stage<CAP, ROWS, CAP / 2, 0>(buf, CAP, j);
}

// sort and cut.  Called by all threads, after a barrier that settled count and buf; ends with a barrier.  The words past
// count[row] are cleared and the rows sorted; thresh = the k-th word (0 while a row holds fewer than k).
//   NEWHALF (k <= CAP / 2): the first half of a row holds what earlier cuts kept, sorted, new words go to the second half from
//   slot CAP / 2 on: count = CAP / 2 afterwards (the words that rank k .. CAP / 2 - 1 stay where they are: the half is sorted).
//   Otherwise new words follow the k kept ones: count = min(count, k) afterwards.
template <int CAP, int ROWS, bool NEWHALF> __device__ __forceinline__ void sort_and_cut(u64* buf, int* count, u64* thresh, int k) {
    for (int e = threadIdx.x; e < ROWS * CAP; e += RK_THREADS)
        if (e % CAP >= count[e / CAP]) buf[e] = 0;
    __syncthreads();
    sort_rows_desc<CAP, ROWS, NEWHALF>(buf);
    if ((int)threadIdx.x < ROWS) {
        const int r = threadIdx.x;
        thresh[r] = buf[r * CAP + k - 1];  // (0 = no candidate)
        count[r] = NEWHALF ? CAP / 2 : min(count[r], k);
    }
    __syncthreads();
}

// ---- the selection in the epilogue of a 32 x 64 score tile, whichever routine formed the scores ----------------------------------
// cand [RK_RT][CAP] words, count / thresh [RK_RT].  A tile adds at most RK_CT words to a row, and a row holds at most CAP - RK_CT
// when a tile starts: CAP = 128 keeps k <= 64 words and new ones behind them; CAP = 256 / 512 keep k <= CAP / 2 in the first half
// (see sort_and_cut)
template <int CAP> __device__ __forceinline__ void tile_select_init(u64* cand, int* count, u64* thresh) {
    constexpr bool NEWHALF = CAP >= 256;
    const int t = threadIdx.x;
    if (t < RK_RT) {
        thresh[t] = 0;
        count[t] = NEWHALF ? CAP / 2 : 0;
    }
    if (NEWHALF)
        for (int e = t; e < RK_RT * CAP / 2; e += RK_THREADS) cand[(e / (CAP / 2)) * CAP + e % (CAP / 2)] = 0;
    __syncthreads();
}

// the scores of key tile `tile` in the accumulator layout of rank_tile_products: lane (c, g) of wave w holds
// [row 4 g + i][column 16 w + c] of the two 16-row blocks in acc0[i] / acc1[i].  Called by all threads; ends with a barrier.
template <int CAP> __device__ __forceinline__ void tile_select_add(const f32x4& acc0, const f32x4& acc1, int tile, int nk, u64* cand,
                                                                   int* count, u64* thresh, int k) {
    constexpr bool NEWHALF = CAP >= 256;
    const int t = threadIdx.x, w = t >> 6, c = t & 15, g = (t >> 4) & 3;
    const int col = tile * RK_CT + 16 * w + c;
    int full = 0;
    if (col < nk) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int rl = (i < 4 ? 0 : 16) + 4 * g + (i & 3);
            const u64 word = candidate(i < 4 ? acc0[i & 3] : acc1[i & 3], col);
            if (word > thresh[rl]) {
                const int slot = atomicAdd(&count[rl], 1);  // < CAP: see above
                cand[rl * CAP + slot] = word;
                full |= slot >= CAP - RK_CT;  // the lane whose word took a row past the mark sees it
            }
        }
    }
    if (__syncthreads_or(full)) sort_and_cut<CAP, RK_RT, NEWHALF>(cand, count, thresh, k);
}

// the last cut, and the split's sorted k words of the rows [r0, r0 + RK_RT) below nrows to part[(split * nq + row) * k + i]
template <int CAP> __device__ __forceinline__ void tile_select_finish(u64* cand, int* count, u64* thresh, int k, int r0, int nrows,
                                                                      int nq, int split, u64* part) {
    constexpr bool NEWHALF = CAP >= 256;
    sort_and_cut<CAP, RK_RT, NEWHALF>(cand, count, thresh, k);
    for (int e = threadIdx.x; e < RK_RT * k; e += RK_THREADS) {
        const int rl = e / k, i = e % k;
        if (r0 + rl < nrows) part[((size_t)split * nq + r0 + rl) * k + i] = cand[rl * CAP + i];
    }
}

template <int CAP, bool MAPPED = false> __global__ __launch_bounds__(RK_THREADS) void topk_tile_kernel(RankArgs a, int k, u64* part) {
    __shared__ __attribute__((aligned(16))) float Qs[RK_RT][RK_LD];
    __shared__ __attribute__((aligned(16))) float Ks[RK_CT][RK_LD];
    __shared__ u64 thresh[RK_RT];
    __shared__ int count[RK_RT];
    extern __shared__ __attribute__((aligned(16))) u64 cand[];  // [RK_RT][CAP]
    const int t = threadIdx.x;
    const int r0 = blockIdx.x * RK_RT, split = blockIdx.y;
    const int nrows = MAPPED ? *a.row_count : a.nq;
    if (MAPPED && r0 >= nrows) return;  // (uniform over the workgroup, before any barrier)
    tile_select_init<CAP>(cand, count, thresh);
    const int ntiles = (a.nk + RK_CT - 1) / RK_CT;
    const int tile0 = split * a.tiles_per_split, tile1 = min(ntiles, tile0 + a.tiles_per_split);
    for (int tile = tile0; tile < tile1; ++tile) {
        int krow[4];
        for (int i = 0; i < 4; ++i) {
            const int kr = tile * RK_CT + (t >> 4) + 16 * i;
            krow[i] = kr < a.nk ? kr : -1;
        }
        f32x4 acc0, acc1;
        rank_tile_products<MAPPED>(a, r0, krow, Qs, Ks, acc0, acc1, nrows);
        tile_select_add<CAP>(acc0, acc1, tile, a.nk, cand, count, thresh, k);
    }
    tile_select_finish<CAP>(cand, count, thresh, k, r0, nrows, a.nq, split, part);
}

// The merge of a row's lists: the words part[(s * nq + r) * k + i], e = s * k + i < n = splits * k (0 = no candidate, never above
// the threshold) - or, DENSE, candidate(row[e], e), e < n - through the threshold / buffer / sort-and-cut scheme.  Called by all
// threads of a workgroup; afterwards buf [TK_ROW_CAP] holds the k best words sorted descending and zeros behind them.
template <bool DENSE> __device__ __forceinline__ void row_select(const float* row, const u64* part, int nq, int r, int n, int k, u64* buf,
                                                                 int* count, u64* thresh) {
    const int t = threadIdx.x;
    if (t == 0) {
        *thresh = 0;
        *count = 0;
    }
    __syncthreads();
    for (int base = 0; base < n; base += 4 * RK_THREADS) {
        u64 word[4];  // four chunks' loads in flight at once
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = base + u * RK_THREADS + t;
            word[u] = 0;
            if (e < n) word[u] = DENSE ? candidate(row[e], e) : part[((size_t)(e / k) * nq + r) * k + e % k];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int full = 0;
            if (word[u] > *thresh) {
                const int slot = atomicAdd(count, 1);  // < TK_ROW_CAP: at most 256 when the chunk starts, 256 threads
                buf[slot] = word[u];
                full = slot >= TK_ROW_CAP - RK_THREADS;
            }
            if (__syncthreads_or(full)) sort_and_cut<TK_ROW_CAP, 1, false>(buf, count, thresh, k);
        }
    }
    sort_and_cut<TK_ROW_CAP, 1, false>(buf, count, thresh, k);
}

// DENSE: the words of row r are candidate(scores[r][e], e), e < n.  Otherwise they are the lists of the splits (row_select).
// MAPPED (never DENSE): workgroup p merges the lists at position p and writes row row_map[p].
template <bool DENSE, bool MAPPED = false>
__global__ __launch_bounds__(RK_THREADS) void topk_row_kernel(const float* scores, size_t ld, const u64* part, int nq, int n, int k,
                                                              float* values, int32_t* indices, const int32_t* row_map = nullptr,
                                                              const int32_t* row_count = nullptr) {
    __shared__ u64 buf[TK_ROW_CAP];
    __shared__ u64 thresh;
    __shared__ int count;
    const int t = threadIdx.x, r = blockIdx.x;
    if (MAPPED && r >= *row_count) return;
    const int out = MAPPED ? row_map[r] : r;
    const float* row = scores + (size_t)r * ld;
    row_select<DENSE>(row, part, nq, r, n, k, buf, &count, &thresh);
    if (t < k) {
        const u64 word = buf[t];
        const int idx = word ? (int)(uint32_t)word : -1;
        float v = -INFINITY;
        if (word) v = DENSE ? row[idx] : bits_score((uint32_t)(word >> 32));
        values[(size_t)out * k + t] = v;
        indices[(size_t)out * k + t] = idx;
    }
}

struct TopkGeometry {
    int rowtiles, splits, tiles_per_split;
    size_t ws_rows;  // rows of k words the workspace holds: >= nq * splits, and monotone in nq and nk (splits itself is not)
};

inline TopkGeometry topk_geometry(int nq, int nk) {
    TopkGeometry g;
    const int ntiles = (nk + RK_CT - 1) / RK_CT;
    g.rowtiles = (nq + RK_RT - 1) / RK_RT;
    const int by_keys = std::min(TK_MAX_SPLITS, (ntiles + TK_MIN_TILES - 1) / TK_MIN_TILES);
    const int by_rows = (TK_WORKGROUPS + g.rowtiles - 1) / g.rowtiles;
    const int want = std::max(1, std::min(by_keys, by_rows));
    g.tiles_per_split = (ntiles + want - 1) / want;
    g.splits = (ntiles + g.tiles_per_split - 1) / g.tiles_per_split;  // <= want
    // rowtiles * splits <= rowtiles * by_keys and <= rowtiles * ceil(1024 / rowtiles) <= 1023 + rowtiles
    g.ws_rows = (size_t)RK_RT * std::min((size_t)g.rowtiles * (size_t)by_keys, (size_t)(TK_WORKGROUPS - 1) + (size_t)g.rowtiles);
    return g;
}

inline bool topk_shape_ok(int nq, int nk, int D) { return nq > 0 && nk > 0 && D % RK_DC == 0 && D >= 64 && D <= 1024; }

template <int CAP, bool MAPPED = false> int launch_topk_tiles(const RankArgs& a, int k, const TopkGeometry& g, u64* part, hipStream_t s) {
    constexpr size_t lds = sizeof(u64) * RK_RT * CAP;
    MADTP_ENSURE_MAX_LDS((topk_tile_kernel<CAP, MAPPED>), lds);
    hipLaunchKernelGGL((topk_tile_kernel<CAP, MAPPED>), dim3(g.rowtiles, g.splits), dim3(RK_THREADS), lds, s, a, k, part);
    return 0;
}

}  // namespace

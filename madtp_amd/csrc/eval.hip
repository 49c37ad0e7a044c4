// Retrieval evaluation (compress_retrieval_*_dtp.py itm_eval): the rank of every ground-truth key among a query's scores, counted
// on the device.  "How many keys score above the target" is all recall@K needs, so no similarity matrix is formed, copied or
// sorted.  Exact f32 products on v_mfma_f32_16x16x4_f32, integer counts, fixed-order sums, no atomics: identical calls give
// identical bits.
//   rank(t) = #{j != t : s_j > s_t} + #{j > t : s_j == s_t}       (the position of t in argsort(s, kind="stable")[::-1])
#include <algorithm>
#include <limits.h>

#include "eval_device.h"  // the constants, RankArgs and rank_tile_products, the one product routine (shared with search.hip)

namespace {

// targets of row r: first CSR position and count.  Pointers that leave [0, min(tgt_ptr[nq], cap)] or run backwards give an
// empty row; targets past the 16th are ignored.
__device__ __forceinline__ void rank_row_span(const RankArgs& a, int r, int& lo, int& n) {
    lo = a.tgt_ptr[r];
    const int hi = a.tgt_ptr[r + 1];
    n = (lo < 0 || hi > min(a.tgt_ptr[a.nq], a.cap) || hi < lo) ? 0 : min(hi - lo, RK_MAXT);
}

// ---- pass 1: the target scores.  One workgroup per row tile; its rows' targets are gathered as key columns, slot
// (local row) * ntmax + k, 64 slots per tile, and go through rank_tile_products.
__global__ __launch_bounds__(RK_THREADS) void rank_target_scores_kernel(RankArgs a) {
    __shared__ __attribute__((aligned(16))) float Qs[RK_RT][RK_LD];
    __shared__ __attribute__((aligned(16))) float Ks[RK_CT][RK_LD];
    __shared__ int lo_s[RK_RT], n_s[RK_RT], ntmax_s;
    const int t = threadIdx.x, w = t >> 6, c = t & 15, g = (t >> 4) & 3;
    const int r0 = blockIdx.x * RK_RT;
    if (t < RK_RT) {
        int lo = 0, n = 0;
        if (r0 + t < a.nq) rank_row_span(a, r0 + t, lo, n);
        lo_s[t] = lo;
        n_s[t] = n;
    }
    __syncthreads();
    if (t == 0) {
        int m = 0;
        for (int r = 0; r < RK_RT; ++r) m = max(m, n_s[r]);
        ntmax_s = m;
    }
    __syncthreads();
    const int ntmax = ntmax_s;
    if (ntmax == 0) return;
    const int ntiles = (RK_RT * ntmax + RK_CT - 1) / RK_CT;
    for (int tile = 0; tile < ntiles; ++tile) {
        // CSR position of slot s, or -1
        auto slot_pos = [&](int s) {
            const int rl = s / ntmax, k = s % ntmax;
            return (rl < RK_RT && k < n_s[rl]) ? lo_s[rl] + k : -1;
        };
        int krow[4];
        for (int i = 0; i < 4; ++i) {
            const int pos = slot_pos(tile * RK_CT + (t >> 4) + 16 * i);
            int kr = -1;
            if (pos >= 0) {
                kr = a.tgt_idx[pos];
                if (kr < 0 || kr >= a.nk) kr = -1;
            }
            krow[i] = kr;
        }
        f32x4 acc0, acc1;
        rank_tile_products(a, r0, krow, Qs, Ks, acc0, acc1);
        const int s = tile * RK_CT + 16 * w + c, rl = s / ntmax, pos = slot_pos(s);
        if (pos >= 0) {
            const int kr = a.tgt_idx[pos];
            const bool ok = kr >= 0 && kr < a.nk;
            for (int i = 0; i < 4; ++i) {
                if (rl == 4 * g + i) a.score_tgt[pos] = ok ? acc0[i] : __builtin_nanf("");
                if (rl == 16 + 4 * g + i) a.score_tgt[pos] = ok ? acc1[i] : __builtin_nanf("");
            }
        }
    }
}

// ---- pass 2: the counts.  Workgroup (row tile, split) walks its key tiles; every accumulator is compared with the targets of
// its row and each lane keeps integer counts, summed over the lanes and waves at the end (integers: any order is exact).
// (rank_beats, the comparison, is in eval_device.h: lists.hip counts with it too)

__global__ __launch_bounds__(RK_THREADS) void rank_count_kernel(RankArgs a) {
    __shared__ __attribute__((aligned(16))) float Qs[RK_RT][RK_LD];
    __shared__ __attribute__((aligned(16))) float Ks[RK_CT][RK_LD];
    __shared__ float St[RK_RT][RK_MAXT];
    __shared__ int Tc[RK_RT][RK_MAXT];
    __shared__ int lo_s[RK_RT], n_s[RK_RT], ntmax_s;
    __shared__ int red[4][RK_RT][RK_MAXT];
    const int t = threadIdx.x, w = t >> 6, c = t & 15, g = (t >> 4) & 3;
    const int r0 = blockIdx.x * RK_RT, split = blockIdx.y;
    if (t < RK_RT) {
        int lo = 0, n = 0;
        if (r0 + t < a.nq) rank_row_span(a, r0 + t, lo, n);
        lo_s[t] = lo;
        n_s[t] = n;
    }
    __syncthreads();
    for (int e = t; e < RK_RT * RK_MAXT; e += RK_THREADS) {
        const int rl = e / RK_MAXT, k = e % RK_MAXT;
        // an absent or out-of-range target: nothing beats it (and its counts are never read)
        float st = INFINITY;
        int tc = INT_MAX;
        if (k < n_s[rl]) {
            const int kr = a.tgt_idx[lo_s[rl] + k];
            if (kr >= 0 && kr < a.nk) {
                st = a.score_tgt[lo_s[rl] + k];
                tc = kr;
            }
        }
        St[rl][k] = st;
        Tc[rl][k] = tc;
    }
    if (t == 0) {
        int m = 0;
        for (int r = 0; r < RK_RT; ++r) m = max(m, n_s[r]);
        ntmax_s = m;
    }
    __syncthreads();
    const int ntmax = ntmax_s;
    if (ntmax == 0) return;
    int cnt[8][RK_MAXT];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int k = 0; k < RK_MAXT; ++k) cnt[i][k] = 0;
    const int ntiles = (a.nk + RK_CT - 1) / RK_CT;
    const int tile0 = split * a.tiles_per_split, tile1 = min(ntiles, tile0 + a.tiles_per_split);
    for (int tile = tile0; tile < tile1; ++tile) {
        int krow[4];
        for (int i = 0; i < 4; ++i) {
            const int kr = tile * RK_CT + (t >> 4) + 16 * i;
            krow[i] = kr < a.nk ? kr : -1;
        }
        f32x4 acc0, acc1;
        rank_tile_products(a, r0, krow, Qs, Ks, acc0, acc1);
        const int col = tile * RK_CT + 16 * w + c;
        const bool colok = col < a.nk;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int rl = (i < 4 ? 0 : 16) + 4 * g + (i & 3);
            const float s = colok ? (i < 4 ? acc0[i & 3] : acc1[i & 3]) : __builtin_nanf("");  // NaN compares false
#pragma unroll
            for (int k = 0; k < RK_MAXT; ++k)
                if (k < ntmax) cnt[i][k] += rank_beats(s, col, St[rl][k], Tc[rl][k]);
        }
    }
    // the 16 column lanes of a wave, then the four waves
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int rl = (i < 4 ? 0 : 16) + 4 * g + (i & 3);
#pragma unroll
        for (int k = 0; k < RK_MAXT; ++k) {
            if (k < ntmax) {
                int v = cnt[i][k];
                for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m);
                if (c == 0) red[w][rl][k] = v;
            }
        }
    }
    __syncthreads();
    for (int e = t; e < RK_RT * RK_MAXT; e += RK_THREADS) {
        const int rl = e / RK_MAXT, k = e % RK_MAXT;
        if (k < n_s[rl]) a.part[(size_t)split * a.cap + lo_s[rl] + k] = red[0][rl][k] + red[1][rl][k] + red[2][rl][k] + red[3][rl][k];
    }
}

// ---- combine: one thread per row sums the splits of each target and takes the row minimum
constexpr int RK_CB_THREADS = 256;
__global__ __launch_bounds__(RK_CB_THREADS) void rank_combine_kernel(RankArgs a) {
    const int r = blockIdx.x * RK_CB_THREADS + threadIdx.x;
    if (r >= a.nq) return;
    int lo, n;
    rank_row_span(a, r, lo, n);
    int best = a.nk;
    for (int k = 0; k < n; ++k) {
        const int kr = a.tgt_idx[lo + k];
        int rank = a.nk;
        if (kr >= 0 && kr < a.nk) {
            rank = 0;
            for (int sp = 0; sp < a.splits; ++sp) rank += a.part[(size_t)sp * a.cap + lo + k];
            best = min(best, rank);
        }
        a.rank_tgt[lo + k] = rank;
    }
    a.rank_row[r] = best;
}

void rank_geometry(int nq, int nk, int& rowtiles, int& splits, int& tiles_per_split) {
    const int ntiles = (nk + RK_CT - 1) / RK_CT;
    rowtiles = (nq + RK_RT - 1) / RK_RT;
    const int want = std::max(1, std::min(RK_MAX_SPLITS, 4096 / rowtiles));  // ~16 workgroups per CU in all
    tiles_per_split = (ntiles + want - 1) / want;
    splits = (ntiles + tiles_per_split - 1) / tiles_per_split;
}

// ---- dense score matrices (BLIP's re-ranked score_matrix_i2t / _t2i): one workgroup per row, the row streamed once
constexpr int RS_THREADS = 256;

__global__ __launch_bounds__(RS_THREADS) void rank_scores_kernel(const float* scores, size_t ld, int nk, const int32_t* tgt_ptr,
                                                                 const int32_t* tgt_idx, int32_t* rank_row, int32_t* rank_tgt) {
    __shared__ int red[RS_THREADS / 64][RK_MAXT];
    const int r = blockIdx.x, t = threadIdx.x;
    const float* row = scores + (size_t)r * ld;
    // the row's span as in rank_row_span (gridDim.x = nq): outside [0, tgt_ptr[nq]] or backwards = an empty row
    const int lo = tgt_ptr[r], hi = tgt_ptr[r + 1];
    const int n = (lo < 0 || hi > tgt_ptr[gridDim.x] || hi < lo) ? 0 : min(hi - lo, RK_MAXT);
    if (n == 0) {
        if (t == 0) rank_row[r] = nk;
        return;
    }
    float st[RK_MAXT];
    int tc[RK_MAXT], cnt[RK_MAXT];
#pragma unroll
    for (int k = 0; k < RK_MAXT; ++k) {
        st[k] = INFINITY;
        tc[k] = INT_MAX;
        cnt[k] = 0;
        if (k < n) {
            const int kr = tgt_idx[lo + k];
            if (kr >= 0 && kr < nk) {
                st[k] = row[kr];
                tc[k] = kr;
            }
        }
    }
    auto one = [&](float s, int col) {
#pragma unroll
        for (int k = 0; k < RK_MAXT; ++k)
            if (k < n) cnt[k] += rank_beats(s, col, st[k], tc[k]);
    };
    // scalar head up to the first 16-byte boundary of the row, 16-byte loads, scalar tail
    const int head = min(nk, (int)((4 - (((uintptr_t)row >> 2) & 3)) & 3));
    const int nvec = (nk - head) / 4;
    if (t < head) one(row[t], t);
    for (int v = t; v < nvec; v += RS_THREADS) {
        const f32x4 x = *(const f32x4*)(row + head + 4 * v);
        for (int e = 0; e < 4; ++e) one(x[e], head + 4 * v + e);
    }
    const int tail0 = head + 4 * nvec;
    if (tail0 + t < nk) one(row[tail0 + t], tail0 + t);
#pragma unroll
    for (int k = 0; k < RK_MAXT; ++k) {
        if (k < n) {
            int v = cnt[k];
            for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
            if ((t & 63) == 0) red[t >> 6][k] = v;
        }
    }
    __syncthreads();
    if (t == 0) {
        int best = nk;
        for (int k = 0; k < n; ++k) {
            const int kr = tgt_idx[lo + k];
            int rank = nk;
            if (kr >= 0 && kr < nk) {
                rank = 0;
                for (int w = 0; w < RS_THREADS / 64; ++w) rank += red[w][k];
                best = min(best, rank);
            }
            rank_tgt[lo + k] = rank;
        }
        rank_row[r] = best;
    }
}

}  // namespace

extern "C" size_t madtp_rank_workspace(int nq, int nk, int D, int n_targets) {
    if (nq <= 0 || nk <= 0 || D <= 0 || n_targets < 0) return 0;
    int rowtiles, splits, tps;
    rank_geometry(nq, nk, rowtiles, splits, tps);
    return sizeof(int32_t) * (size_t)splits * (size_t)std::max(n_targets, 1);
}

extern "C" int madtp_rank_embeds(const float* q, int ldq, const float* keys, int ldk, int nq, int nk, int D, const int32_t* tgt_ptr,
                                 const int32_t* tgt_idx, int32_t* rank_row, int32_t* rank_tgt, float* score_tgt, void* ws,
                                 size_t ws_bytes, void* stream) {
    if (!q || !keys || !tgt_ptr || !tgt_idx || !rank_row || !rank_tgt || !score_tgt || !ws) return MADTP_E_BADARG;
    if (nq <= 0 || nk <= 0 || D % RK_DC != 0 || D < 64 || D > 1024 || ldq < D || ldk < D) return MADTP_E_SHAPE;
    if (!aligned16(q) || !aligned16(keys) || ldq % 4 != 0 || ldk % 4 != 0) return MADTP_E_ALIGN;
    RankArgs a;
    a.q = q; a.keys = keys; a.ldq = ldq; a.ldk = ldk; a.nq = nq; a.nk = nk; a.D = D;
    a.tgt_ptr = tgt_ptr; a.tgt_idx = tgt_idx; a.rank_row = rank_row; a.rank_tgt = rank_tgt; a.score_tgt = score_tgt;
    int rowtiles;
    rank_geometry(nq, nk, rowtiles, a.splits, a.tiles_per_split);
    const size_t per_split = ws_bytes / sizeof(int32_t) / (size_t)a.splits;
    if (per_split == 0) return MADTP_E_BADARG;
    a.cap = (int)std::min(per_split, (size_t)nq * RK_MAXT);  // the number of targets itself is tgt_ptr[nq], read on the device
    a.part = (int32_t*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(rank_target_scores_kernel, dim3(rowtiles), dim3(RK_THREADS), 0, s, a);
    hipLaunchKernelGGL(rank_count_kernel, dim3(rowtiles, a.splits), dim3(RK_THREADS), 0, s, a);
    hipLaunchKernelGGL(rank_combine_kernel, dim3((nq + RK_CB_THREADS - 1) / RK_CB_THREADS), dim3(RK_CB_THREADS), 0, s, a);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" int madtp_rank_scores(const float* scores, int ld, int nq, int nk, const int32_t* tgt_ptr, const int32_t* tgt_idx,
                                 int32_t* rank_row, int32_t* rank_tgt, void* stream) {
    if (!scores || !tgt_ptr || !tgt_idx || !rank_row || !rank_tgt) return MADTP_E_BADARG;
    if (nq <= 0 || nk <= 0 || ld < nk) return MADTP_E_SHAPE;
    hipLaunchKernelGGL(rank_scores_kernel, dim3(nq), dim3(RS_THREADS), 0, (hipStream_t)stream, scores, (size_t)ld, nk, tgt_ptr, tgt_idx,
                       rank_row, rank_tgt);
    MADTP_LAUNCH_CHECK();
    return 0;
}

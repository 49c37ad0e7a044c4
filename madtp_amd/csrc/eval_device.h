// The exact-f32 product routine of the retrieval kernels, shared by eval.hip (ranks of known targets: a count in the epilogue)
// and search.hip (top-k candidates: a selection in the epilogue).  Both form every score <q_r, keys_j> here, so the score of a
// (row, key) pair is the same bits whichever of them reports it.
#pragma once
#include "common.h"

namespace {

constexpr int RK_RT = 32;        // query rows per workgroup: two 16-row MFMA blocks that share every key fragment
constexpr int RK_CT = 64;        // key columns per tile, 16 per wave
constexpr int RK_DC = 64;        // features per staged chunk
constexpr int RK_LD = 68;        // floats per LDS row: 16-byte aligned rows, 68 r mod 64 = 4 r
constexpr int RK_THREADS = 256;
constexpr int RK_MAXT = 16;      // targets per row
constexpr int RK_MAX_SPLITS = 1024;

struct RankArgs {
    const float *q, *keys;
    int ldq, ldk, nq, nk, D;
    int cap;  // targets the workspace holds per split = the stride of part
    const int32_t *tgt_ptr, *tgt_idx;
    int32_t *rank_row, *rank_tgt;
    float* score_tgt;
    int32_t* part;  // [splits, cap] counts
    int splits, tiles_per_split;
    // the optional row map (the MAPPED kernels of search_device.h): query row p of the launch is row row_map[p] of q, and
    // *row_count rows are listed, both read on the device
    const int32_t* row_map = nullptr;
    const int32_t* row_count = nullptr;
};

// The one comparison of the rank rule, rank(t) = #{j != t : s_j > s_t} + #{j > t : s_j == s_t}: does key `col` with score s stand
// before target tc with score st?  IEEE comparisons: a NaN on either side beats nothing, -0 ties with +0.  Shared by eval.hip
// (dense rows and embeddings) and lists.hip (candidate lists).
__device__ __forceinline__ int rank_beats(float s, int col, float st, int tc) {
    return ((s > st) & (col != tc)) | ((s == st) & (col > tc));
}

// The one product routine of the retrieval kernels: acc0 / acc1 = rows [r0, r0 + 16) / [r0 + 16, r0 + 32) of q against the 64 key
// rows krow[] that the caller names (thread t stages feature quad 4 (t % 16) of the tile's columns t / 16 + 16 i; -1 = a column of
// zeros).  Lane (c, g) = (l & 15, l >> 4) of wave w holds [row 4 g + i][column 16 w + c] in register i.  Every element is the
// fmaf chain over the features in the order chunk, j, e, g of feature 64 chunk + 16 j + 4 g + e - a function of the two rows
// alone, not of the column's place in a tile - so a score computed for a gathered target column and the score the counting
// pass forms for the same key row (or a byte copy of it) are the same bits.
// The next chunk's global loads are issued before the products of the current one.
// MAPPED: the rows are those of the row map, nrows = *a.row_count of them (read by the caller).
template <bool MAPPED = false>
__device__ __forceinline__ void rank_tile_products(const RankArgs& a, int r0, const int (&krow)[4], float (*Qs)[RK_LD],
                                                   float (*Ks)[RK_LD], f32x4& acc0, f32x4& acc1, int nrows = 0) {
    const int t = threadIdx.x, w = t >> 6, c = t & 15, g = (t >> 4) & 3;
    const int sr = t >> 4, d4 = (t & 15) * 4;
    const int ndc = a.D / RK_DC;
    f32x4 qreg[2], kreg[4];
    int qrow[2];
    for (int i = 0; i < 2; ++i) {
        const int row = r0 + sr + 16 * i;
        if constexpr (MAPPED) qrow[i] = row < nrows ? a.row_map[row] : -1;
        else qrow[i] = row < a.nq ? row : -1;
    }
    auto fetch = [&](int dc) {
        for (int i = 0; i < 2; ++i) {
            qreg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (qrow[i] >= 0) qreg[i] = *(const f32x4*)(a.q + (size_t)qrow[i] * a.ldq + dc * RK_DC + d4);
        }
        for (int i = 0; i < 4; ++i) {
            kreg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (krow[i] >= 0) kreg[i] = *(const f32x4*)(a.keys + (size_t)krow[i] * a.ldk + dc * RK_DC + d4);
        }
    };
    acc0 = f32x4{0.f, 0.f, 0.f, 0.f};
    acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
    fetch(0);
    for (int dc = 0; dc < ndc; ++dc) {
        for (int i = 0; i < 2; ++i) *(f32x4*)&Qs[sr + 16 * i][d4] = qreg[i];
        for (int i = 0; i < 4; ++i) *(f32x4*)&Ks[sr + 16 * i][d4] = kreg[i];
        __syncthreads();
        if (dc + 1 < ndc) fetch(dc + 1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 qa0 = *(const f32x4*)&Qs[c][16 * j + 4 * g], qa1 = *(const f32x4*)&Qs[16 + c][16 * j + 4 * g];
            const f32x4 kb = *(const f32x4*)&Ks[16 * w + c][16 * j + 4 * g];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa0[e], kb[e], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa1[e], kb[e], acc1, 0, 0, 0);
            }
        }
        lds_barrier();  // the tiles are free again; the loads in flight stay in flight
    }
}

}  // namespace

// Retrieval training step (models/blip_retrieval.py:99-322): the contrastive loss over the feature queues with its gradient,
// the EMA of the momentum encoders, and the in-batch hard-negative draw of ITM.  All arithmetic is f32 with exact products
// (FMA); every reduction runs in a fixed order and nothing uses atomics, so two identical calls are bit-identical.
#include <algorithm>

#include "common.h"

namespace {

// ================================ ITC: contrastive loss over [in-batch | queue] ===============================================
// One direction per call: query rows q (student) and q_m (momentum) [B,D] against the N = B + Q key columns
//   k_j = kb[j, :] (the other modality's in-batch momentum features, j < B),   k_{B+i} = queue[:, i] (the [D, Q] buffer).
// s = q k / temp, s_m = q_m k / temp,  t = alpha softmax(s_m) + (1 - alpha) pos / n_pos,  loss = -sum_j t_j log softmax(s)_j
//   = logZ(s) - alpha sum_j softmax(s_m)_j s_j - (1 - alpha) sum_pos s_j / n_pos
// Pass 1 streams the keys once: online max / sum-exp of s and s_m, online sum softmax(s_m) s, sum over positives, n_pos.
// Pass 2 streams them again:   dq = sum_j (p_j - t_j) k_j / (B temp),   dtemp = -sum_j (p_j - t_j) s_j / (B temp).
constexpr int ITC_RT = 32;       // query rows per workgroup
constexpr int ITC_CT = 64;       // key columns per tile
constexpr int ITC_DC = 64;       // feature dimensions per staged chunk
constexpr int ITC_THREADS = 256;
constexpr int ITC_NSTAT = 8;     // ms, ls, mm, lm, am, possum, npos, pad
constexpr int ITC_MAX_SPLITS = 1024;  // ~4 workgroups per CU at B <= 32 (one 64-column tile each at Q = 57 600)

struct ItcArgs {
    const float *q, *qm, *kb, *queue;
    const int64_t *idx, *idxq;
    const float* temp;
    float alpha;
    int B, D, Q, N, splits, tiles_per_split;
    float* stats;    // [splits, B, ITC_NSTAT]
    float* rowinfo;  // [B, 4]: logZ, logZm, (1 - alpha) / n_pos
    float* dqpart;   // [splits, B, D]
    float* dtpart;   // [splits, B]
    float *loss, *dq, *dtemp;
};

__device__ __forceinline__ void online_add(float& m, float& l, float x) {
    const float mn = fmaxf(m, x);
    l = l * expf(m - mn) + expf(x - mn);
    m = mn;
}

// stages q / q_m rows [r0, r0 + 32) and key columns [c0, c0 + 64) of feature chunk dc into LDS (zeros outside the problem)
__device__ __forceinline__ void itc_stage_keys(const ItcArgs& a, float (*Ks)[ITC_CT + 1], int c0, int dc) {
    for (int e = threadIdx.x; e < ITC_DC * ITC_CT; e += ITC_THREADS) {
        const int dd = e / ITC_CT, cc = e % ITC_CT, col = c0 + cc, d = dc * ITC_DC + dd;
        float v = 0.f;
        if (col < a.B) v = a.kb[(size_t)col * a.D + d];
        else if (col < a.N) v = a.queue[(size_t)d * a.Q + (col - a.B)];
        Ks[dd][cc] = v;
    }
}

__device__ __forceinline__ void itc_stage_rows(const ItcArgs& a, float (*Qs)[ITC_DC + 1], float (*Qms)[ITC_DC + 1], int r0, int dc) {
    for (int e = threadIdx.x; e < ITC_RT * ITC_DC; e += ITC_THREADS) {
        const int r = e / ITC_DC, dd = e % ITC_DC, row = r0 + r;
        const bool ok = row < a.B;
        Qs[r][dd] = ok ? a.q[(size_t)row * a.D + dc * ITC_DC + dd] : 0.f;
        Qms[r][dd] = ok ? a.qm[(size_t)row * a.D + dc * ITC_DC + dd] : 0.f;
    }
}

__device__ __forceinline__ int64_t itc_col_id(const ItcArgs& a, int col) { return col < a.B ? a.idx[col] : a.idxq[col - a.B]; }

// thread (tr, tc) = (t / 16, t % 16) owns rows 2 tr, 2 tr + 1 and columns 4 tc .. 4 tc + 3 of every tile
template <int NDC, bool PASS2>
__global__ __launch_bounds__(ITC_THREADS) void itc_pass_kernel(ItcArgs a) {
    __shared__ float Qs[ITC_RT][ITC_DC + 1];
    __shared__ float Qms[ITC_RT][ITC_DC + 1];
    __shared__ float Ks[ITC_DC][ITC_CT + 1];
    __shared__ float Ws[ITC_RT][ITC_CT + 1];
    __shared__ float red[ITC_RT][16][7];
    const int t = threadIdx.x, tr = t >> 4, tc = t & 15;
    const int r0 = blockIdx.x * ITC_RT, split = blockIdx.y;
    const float temp = *a.temp;
    const int tile0 = split * a.tiles_per_split;
    const int ntiles = (a.N + ITC_CT - 1) / ITC_CT;
    const int tile1 = min(ntiles, tile0 + a.tiles_per_split);
    int64_t my_id[2];
    float rinfo[2][3];
    for (int i = 0; i < 2; ++i) {
        const int row = r0 + 2 * tr + i;
        my_id[i] = row < a.B ? a.idx[row] : INT64_MIN;
        for (int k = 0; k < 3; ++k) rinfo[i][k] = (PASS2 && row < a.B) ? a.rowinfo[row * 4 + k] : 0.f;
    }
    // pass 1 state per owned row
    float ms[2] = {-INFINITY, -INFINITY}, ls[2] = {0.f, 0.f}, mm[2] = {-INFINITY, -INFINITY}, lm[2] = {0.f, 0.f};
    float am[2] = {0.f, 0.f}, ps[2] = {0.f, 0.f}, np_[2] = {0.f, 0.f};
    // pass 2 state: dq rows (t / 8) and feature lanes (t % 8) + 8 k of every chunk; sum (p - t) s of the owned rows
    const int qr = t >> 3, qd = t & 7;
    float dacc[NDC][8];
    if (PASS2)
        for (int c = 0; c < NDC; ++c)
            for (int k = 0; k < 8; ++k) dacc[c][k] = 0.f;
    float wsum[2] = {0.f, 0.f};

    for (int tile = tile0; tile < tile1; ++tile) {
        const int c0 = tile * ITC_CT;
        float s[2][4], sm[2][4];
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 4; ++j) s[i][j] = sm[i][j] = 0.f;
        for (int dc = 0; dc < NDC; ++dc) {
            itc_stage_rows(a, Qs, Qms, r0, dc);
            itc_stage_keys(a, Ks, c0, dc);
            __syncthreads();
#pragma unroll 8
            for (int dd = 0; dd < ITC_DC; ++dd) {
                float kv[4];
                for (int j = 0; j < 4; ++j) kv[j] = Ks[dd][4 * tc + j];
                for (int i = 0; i < 2; ++i) {
                    const float qv = Qs[2 * tr + i][dd], qmv = Qms[2 * tr + i][dd];
                    for (int j = 0; j < 4; ++j) {
                        s[i][j] = fmaf(qv, kv[j], s[i][j]);
                        sm[i][j] = fmaf(qmv, kv[j], sm[i][j]);
                    }
                }
            }
            __syncthreads();
        }
        for (int i = 0; i < 2; ++i) {
            const int row = r0 + 2 * tr + i;
            for (int j = 0; j < 4; ++j) {
                const int col = c0 + 4 * tc + j;
                const bool ok = row < a.B && col < a.N;
                const float sv = s[i][j] / temp, smv = sm[i][j] / temp;
                const bool pos = ok && itc_col_id(a, col) == my_id[i];
                if (!PASS2) {
                    if (ok) {
                        online_add(ms[i], ls[i], sv);
                        const float mn = fmaxf(mm[i], smv), sc = expf(mm[i] - mn), e = expf(smv - mn);
                        lm[i] = lm[i] * sc + e;
                        am[i] = fmaf(e, sv, am[i] * sc);
                        mm[i] = mn;
                        if (pos) { ps[i] += sv; np_[i] += 1.f; }
                    }
                } else {
                    float w = 0.f;
                    if (ok) {
                        const float tgt = a.alpha * expf(smv - rinfo[i][1]) + (pos ? rinfo[i][2] : 0.f);
                        w = expf(sv - rinfo[i][0]) - tgt;
                        wsum[i] = fmaf(w, sv, wsum[i]);
                    }
                    Ws[2 * tr + i][4 * tc + j] = w / temp;
                }
            }
        }
        if (PASS2) {
            for (int dc = 0; dc < NDC; ++dc) {
                itc_stage_keys(a, Ks, c0, dc);
                __syncthreads();
#pragma unroll 4
                for (int cc = 0; cc < ITC_CT; ++cc) {
                    const float wv = Ws[qr][cc];
                    for (int k = 0; k < 8; ++k) dacc[dc][k] = fmaf(wv, Ks[qd + 8 * k][cc], dacc[dc][k]);
                }
                __syncthreads();
            }
        }
    }
    // fixed-order combine of the 16 column lanes of each row
    for (int i = 0; i < 2; ++i) {
        float* r = red[2 * tr + i][tc];
        if (!PASS2) { r[0] = ms[i]; r[1] = ls[i]; r[2] = mm[i]; r[3] = lm[i]; r[4] = am[i]; r[5] = ps[i]; r[6] = np_[i]; }
        else r[0] = wsum[i];
    }
    __syncthreads();
    if (t < ITC_RT && r0 + t < a.B) {
        const int row = r0 + t;
        if (!PASS2) {
            float M = -INFINITY, L = 0.f, MM = -INFINITY, LM = 0.f, AM = 0.f, P = 0.f, NP = 0.f;
            for (int c = 0; c < 16; ++c) {
                const float* r = red[t][c];
                if (r[1] > 0.f) {
                    const float mn = fmaxf(M, r[0]);
                    L = L * expf(M - mn) + r[1] * expf(r[0] - mn);
                    M = mn;
                    const float mn2 = fmaxf(MM, r[2]), s1 = expf(MM - mn2), s2 = expf(r[2] - mn2);
                    LM = LM * s1 + r[3] * s2;
                    AM = AM * s1 + r[4] * s2;
                    MM = mn2;
                }
                P += r[5];
                NP += r[6];
            }
            float* o = a.stats + ((size_t)split * a.B + row) * ITC_NSTAT;
            o[0] = M; o[1] = L; o[2] = MM; o[3] = LM; o[4] = AM; o[5] = P; o[6] = NP; o[7] = 0.f;
        } else {
            float sum = 0.f;
            for (int c = 0; c < 16; ++c) sum += red[t][c][0];
            a.dtpart[(size_t)split * a.B + row] = -sum / temp;
        }
    }
    if (PASS2 && r0 + qr < a.B) {
        float* o = a.dqpart + ((size_t)split * a.B + r0 + qr) * a.D;
        for (int dc = 0; dc < NDC; ++dc)
            for (int k = 0; k < 8; ++k) o[dc * ITC_DC + qd + 8 * k] = dacc[dc][k];
    }
}

// split statistics (max, sum-exp of s; max, sum-exp, sum e*s of s_m; sum over positives; n_pos) and their merge
struct ItcStat {
    float M, L, MM, LM, AM, P, NP;
};
__device__ __forceinline__ ItcStat itc_stat_empty() { return {-INFINITY, 0.f, -INFINITY, 0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ void itc_stat_merge(ItcStat& x, const ItcStat& y) {
    if (y.L > 0.f) {
        if (x.L > 0.f) {
            const float mn = fmaxf(x.M, y.M);
            x.L = x.L * expf(x.M - mn) + y.L * expf(y.M - mn);
            x.M = mn;
            const float mn2 = fmaxf(x.MM, y.MM), s1 = expf(x.MM - mn2), s2 = expf(y.MM - mn2);
            x.LM = x.LM * s1 + y.LM * s2;
            x.AM = x.AM * s1 + y.AM * s2;
            x.MM = mn2;
        } else {
            x.M = y.M; x.L = y.L; x.MM = y.MM; x.LM = y.LM; x.AM = y.AM;
        }
    }
    x.P += y.P;
    x.NP += y.NP;
}

// ================================ ITC, wide features (512 < D <= 1024): the same two passes on the exact-f32 MFMA =============
// v_mfma_f32_16x16x4_f32 forms every product: bitwise an fmaf chain, at the vector FP32 rate, with one LDS read per operand per
// 16 x 16 x 4 block instead of one per FMA.  A workgroup owns 16 query rows (the CLIP driver's batch) and walks 64-column key
// tiles; wave w owns columns 16 w .. 16 w + 15 of the tile and its s and s_m accumulators share every key fragment.  Tiles
// never straddle the in-batch keys and the queue: the first ceil(B / 64) tiles are rows of kb, the rest columns of the queue
// from its column 0, so a queue tile chunk is 64 rows of 256 contiguous bytes and is staged with 16-byte loads.
// Lane l = (c, g) = (l & 15, l >> 4).  Operands: A[row c][k = g], B[k = g][col c]; result register i: [row 4 g + i][col c].
// Pass 1 / the scores of pass 2: the four k of step (j, e) are the features 16 j + 4 g + e of the chunk, so the lane's q values
//   of four steps are one 16-byte LDS read and, with the 68-float rows of Ks, the four key rows of a step start 16 banks apart.
// Pass 2: dq[16, D] += W K^T with W = (p - t) / temp through LDS; the k of a step are the tile columns 16 j + 4 g + e (16-byte
//   reads of both operands) and wave w owns features 16 w .. 16 w + 15 of every chunk: NDC accumulator tiles per lane.
constexpr int ITCW_RT = 16;
constexpr int ITCW_LD = 68;  // floats per LDS row: 16-byte aligned rows, 68 r mod 64 = 4 r
constexpr int ITCW_MAX_SPLITS = 1024;  // one key tile per workgroup at Q = 57 600 (901 tiles): ~3.5 workgroups per CU per row tile

__device__ __forceinline__ void itcw_stage_keys(const ItcArgs& a, float (*Ks)[ITCW_LD], int tile, int nbt, int dc, bool vec) {
    if (tile < nbt) {  // in-batch keys: rows of kb
        for (int e = threadIdx.x; e < ITC_CT * ITC_DC; e += ITC_THREADS) {
            const int cc = e / ITC_DC, dd = e % ITC_DC, col = tile * ITC_CT + cc;
            Ks[dd][cc] = col < a.B ? a.kb[(size_t)col * a.D + dc * ITC_DC + dd] : 0.f;
        }
        return;
    }
    const int q0 = (tile - nbt) * ITC_CT;
    if (vec) {  // Q % 4 == 0 and a 16-byte aligned queue: whole float4 are inside or outside
        for (int e = threadIdx.x; e < ITC_DC * (ITC_CT / 4); e += ITC_THREADS) {
            const int dd = e / (ITC_CT / 4), c4 = (e % (ITC_CT / 4)) * 4, qi = q0 + c4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (qi < a.Q) v = *(const f32x4*)(a.queue + (size_t)(dc * ITC_DC + dd) * a.Q + qi);
            *(f32x4*)&Ks[dd][c4] = v;
        }
    } else {
        for (int e = threadIdx.x; e < ITC_DC * ITC_CT; e += ITC_THREADS) {
            const int dd = e / ITC_CT, cc = e % ITC_CT, qi = q0 + cc;
            Ks[dd][cc] = qi < a.Q ? a.queue[(size_t)(dc * ITC_DC + dd) * a.Q + qi] : 0.f;
        }
    }
}

__device__ __forceinline__ void itcw_stage_rows(const ItcArgs& a, float (*Qs)[ITCW_LD], float (*Qms)[ITCW_LD], int r0, int dc) {
    for (int e = threadIdx.x; e < ITCW_RT * ITC_DC; e += ITC_THREADS) {
        const int r = e / ITC_DC, dd = e % ITC_DC, row = r0 + r;
        const bool ok = row < a.B;
        Qs[r][dd] = ok ? a.q[(size_t)row * a.D + dc * ITC_DC + dd] : 0.f;
        Qms[r][dd] = ok ? a.qm[(size_t)row * a.D + dc * ITC_DC + dd] : 0.f;
    }
}

__device__ __forceinline__ ItcStat itc_stat_shfl_xor(const ItcStat& x, int m) {
    return {__shfl_xor(x.M, m), __shfl_xor(x.L, m), __shfl_xor(x.MM, m), __shfl_xor(x.LM, m),
            __shfl_xor(x.AM, m), __shfl_xor(x.P, m), __shfl_xor(x.NP, m)};
}

template <int NDC, bool PASS2>
__global__ __launch_bounds__(ITC_THREADS) void itc_wide_kernel(ItcArgs a) {
    __shared__ __attribute__((aligned(16))) float Qs[ITCW_RT][ITCW_LD];
    __shared__ __attribute__((aligned(16))) float Qms[ITCW_RT][ITCW_LD];
    __shared__ __attribute__((aligned(16))) float Ks[ITC_DC][ITCW_LD];
    __shared__ __attribute__((aligned(16))) float Ws[PASS2 ? ITCW_RT : 1][ITCW_LD];
    __shared__ float red[ITCW_RT][4][PASS2 ? 1 : 7];
    const int t = threadIdx.x, w = t >> 6, c = t & 15, g = (t >> 4) & 3;
    const int r0 = blockIdx.x * ITCW_RT, split = blockIdx.y;
    const float temp = *a.temp;
    const int nbt = (a.B + ITC_CT - 1) / ITC_CT, ntiles = nbt + (a.Q + ITC_CT - 1) / ITC_CT;
    const int tile0 = split * a.tiles_per_split, tile1 = min(ntiles, tile0 + a.tiles_per_split);
    const bool vec = (a.Q & 3) == 0 && (((uintptr_t)a.queue) & 15u) == 0;
    // result register i of this lane is row 4 g + i
    int64_t my_id[4];
    float rinfo[4][3];
    for (int i = 0; i < 4; ++i) {
        const int row = r0 + 4 * g + i;
        my_id[i] = row < a.B ? a.idx[row] : INT64_MIN;
        for (int k = 0; k < 3; ++k) rinfo[i][k] = (PASS2 && row < a.B) ? a.rowinfo[row * 4 + k] : 0.f;
    }
    ItcStat st[4];
    for (int i = 0; i < 4; ++i) st[i] = itc_stat_empty();
    f32x4 dacc[NDC];
    for (int dc = 0; dc < NDC; ++dc) dacc[dc] = f32x4{0.f, 0.f, 0.f, 0.f};
    float wsum[4] = {0.f, 0.f, 0.f, 0.f};

    for (int tile = tile0; tile < tile1; ++tile) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f}, sm = {0.f, 0.f, 0.f, 0.f};
        for (int dc = 0; dc < NDC; ++dc) {
            itcw_stage_rows(a, Qs, Qms, r0, dc);
            itcw_stage_keys(a, Ks, tile, nbt, dc, vec);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 qa = *(const f32x4*)&Qs[c][16 * j + 4 * g], qma = *(const f32x4*)&Qms[c][16 * j + 4 * g];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float kv = Ks[16 * j + 4 * g + e][16 * w + c];
                    s = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[e], kv, s, 0, 0, 0);
                    sm = __builtin_amdgcn_mfma_f32_16x16x4f32(qma[e], kv, sm, 0, 0, 0);
                }
            }
            __syncthreads();
        }
        // this lane's column of the tile, its validity and id
        const int cc = 16 * w + c;
        bool colok;
        int64_t cid = 0;
        if (tile < nbt) {
            const int col = tile * ITC_CT + cc;
            colok = col < a.B;
            if (colok) cid = a.idx[col];
        } else {
            const int qi = (tile - nbt) * ITC_CT + cc;
            colok = qi < a.Q;
            if (colok) cid = a.idxq[qi];
        }
        for (int i = 0; i < 4; ++i) {
            const bool ok = colok && r0 + 4 * g + i < a.B;
            const float sv = s[i] / temp, smv = sm[i] / temp;
            const bool pos = ok && cid == my_id[i];
            if constexpr (!PASS2) {
                if (ok) {
                    ItcStat& x = st[i];
                    online_add(x.M, x.L, sv);
                    const float mn = fmaxf(x.MM, smv), sc = expf(x.MM - mn), ex = expf(smv - mn);
                    x.LM = x.LM * sc + ex;
                    x.AM = fmaf(ex, sv, x.AM * sc);
                    x.MM = mn;
                    if (pos) { x.P += sv; x.NP += 1.f; }
                }
            } else {
                float wv = 0.f;
                if (ok) {
                    const float tgt = a.alpha * expf(smv - rinfo[i][1]) + (pos ? rinfo[i][2] : 0.f);
                    wv = expf(sv - rinfo[i][0]) - tgt;
                    wsum[i] = fmaf(wv, sv, wsum[i]);
                }
                Ws[4 * g + i][cc] = wv / temp;
            }
        }
        if constexpr (PASS2) {
            __syncthreads();
            f32x4 wa[4];
            for (int j = 0; j < 4; ++j) wa[j] = *(const f32x4*)&Ws[c][16 * j + 4 * g];
#pragma unroll
            for (int dc = 0; dc < NDC; ++dc) {
                itcw_stage_keys(a, Ks, tile, nbt, dc, vec);
                __syncthreads();
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 kv = *(const f32x4*)&Ks[16 * w + c][16 * j + 4 * g];
#pragma unroll
                    for (int e = 0; e < 4; ++e) dacc[dc] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[j][e], kv[e], dacc[dc], 0, 0, 0);
                }
                __syncthreads();
            }
        }
    }
    // the 16 column lanes of a wave by a fixed xor tree, then the four waves in order
    for (int i = 0; i < 4; ++i) {
        for (int m = 1; m < 16; m <<= 1) {
            if constexpr (!PASS2) {
                const ItcStat y = itc_stat_shfl_xor(st[i], m);
                itc_stat_merge(st[i], y);
            } else {
                wsum[i] += __shfl_xor(wsum[i], m);
            }
        }
        if (c == 0) {
            float* r = red[4 * g + i][w];
            if constexpr (!PASS2) {
                const ItcStat& x = st[i];
                r[0] = x.M; r[1] = x.L; r[2] = x.MM; r[3] = x.LM; r[4] = x.AM; r[5] = x.P; r[6] = x.NP;
            } else {
                r[0] = wsum[i];
            }
        }
    }
    __syncthreads();
    if (t < ITCW_RT && r0 + t < a.B) {
        const int row = r0 + t;
        if constexpr (!PASS2) {
            ItcStat x = itc_stat_empty();
            for (int k = 0; k < 4; ++k) {
                const float* r = red[t][k];
                const ItcStat y = {r[0], r[1], r[2], r[3], r[4], r[5], r[6]};
                itc_stat_merge(x, y);
            }
            float* o = a.stats + ((size_t)split * a.B + row) * ITC_NSTAT;
            o[0] = x.M; o[1] = x.L; o[2] = x.MM; o[3] = x.LM; o[4] = x.AM; o[5] = x.P; o[6] = x.NP; o[7] = 0.f;
        } else {
            float sum = 0.f;
            for (int k = 0; k < 4; ++k) sum += red[t][k][0];
            a.dtpart[(size_t)split * a.B + row] = -sum / temp;
        }
    }
    if constexpr (PASS2) {
        for (int i = 0; i < 4; ++i) {
            const int row = r0 + 4 * g + i;
            if (row >= a.B) continue;
            float* o = a.dqpart + ((size_t)split * a.B + row) * a.D + 16 * w + c;
            for (int dc = 0; dc < NDC; ++dc) o[dc * ITC_DC] = dacc[dc][i];
        }
    }
}

// one wave per row: lane l merges splits l, l + 64, ... in order, then a fixed pairwise tree over the lanes
// -> loss, logZ, logZm, (1 - alpha) / n_pos
constexpr int ITC_C1_THREADS = 64;
__global__ __launch_bounds__(ITC_C1_THREADS) void itc_combine1_kernel(ItcArgs a) {
    __shared__ ItcStat st[ITC_C1_THREADS];
    const int row = blockIdx.x, lane = threadIdx.x;
    ItcStat acc = itc_stat_empty();
    for (int sp = lane; sp < a.splits; sp += ITC_C1_THREADS) {
        const float* r = a.stats + ((size_t)sp * a.B + row) * ITC_NSTAT;
        const ItcStat y = {r[0], r[1], r[2], r[3], r[4], r[5], r[6]};
        itc_stat_merge(acc, y);
    }
    st[lane] = acc;
    __syncthreads();
    for (int w = ITC_C1_THREADS / 2; w > 0; w >>= 1) {
        if (lane < w) itc_stat_merge(st[lane], st[lane + w]);
        __syncthreads();
    }
    if (lane == 0) {
        const ItcStat x = st[0];
        const float logZ = x.M + logf(x.L), logZm = x.MM + logf(x.LM), cpos = (1.f - a.alpha) / x.NP;
        a.loss[row] = logZ - a.alpha * (x.AM / x.LM) - cpos * x.P;
        a.rowinfo[row * 4 + 0] = logZ;
        a.rowinfo[row * 4 + 1] = logZm;
        a.rowinfo[row * 4 + 2] = cpos;
        a.rowinfo[row * 4 + 3] = 0.f;
    }
}

// blocks (b, c) with b < B: dq[b, 64 c .. 64 c + 63] = sum over splits / B - wave w sums splits w, w + 16, ..., then the 16
// wave sums are added in order.  Block (B, 0): dtemp = sum of all [splits, B] partials / B, thread t summing entries t,
// t + 256, ... and a fixed pairwise tree over the threads.
constexpr int ITC_C2_THREADS = 1024;
__global__ __launch_bounds__(ITC_C2_THREADS) void itc_combine2_kernel(ItcArgs a) {
    __shared__ float part[ITC_C2_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const float invB = 1.f / (float)a.B;
    if (b < a.B) {
        const int w = t >> 6, d = blockIdx.y * 64 + (t & 63);
        float s = 0.f;
        for (int sp = w; sp < a.splits; sp += ITC_C2_THREADS / 64) s += a.dqpart[((size_t)sp * a.B + b) * a.D + d];
        part[t] = s;
        __syncthreads();
        if (t < 64) {
            float acc = part[t];
            for (int k = 1; k < ITC_C2_THREADS / 64; ++k) acc += part[t + 64 * k];
            a.dq[(size_t)b * a.D + d] = acc * invB;
        }
        return;
    }
    if (blockIdx.y != 0) return;
    float s = 0.f;
    const int n = a.splits * a.B;
    for (int i = t; i < n; i += ITC_C2_THREADS) s += a.dtpart[i];
    part[t] = s;
    __syncthreads();
    for (int w = ITC_C2_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) part[t] += part[t + w];
        __syncthreads();
    }
    if (t == 0) *a.dtemp = part[0] * invB;
}

void itc_geometry(int B, int D, int Q, int& rowtiles, int& splits, int& tiles_per_split) {
    if (D > 512) {  // the wide kernel: 16-row tiles, key tiles that do not straddle the in-batch keys and the queue
        const int ntiles = (B + ITC_CT - 1) / ITC_CT + (Q + ITC_CT - 1) / ITC_CT;
        rowtiles = (B + ITCW_RT - 1) / ITCW_RT;
        const int want = std::max(1, std::min(ITCW_MAX_SPLITS, 2048 / rowtiles));
        tiles_per_split = (ntiles + want - 1) / want;
        splits = (ntiles + tiles_per_split - 1) / tiles_per_split;
        return;
    }
    const int N = B + Q, ntiles = (N + ITC_CT - 1) / ITC_CT;
    rowtiles = (B + ITC_RT - 1) / ITC_RT;
    int want = std::max(1, std::min(ITC_MAX_SPLITS, 2048 / rowtiles));
    tiles_per_split = (ntiles + want - 1) / want;
    splits = (ntiles + tiles_per_split - 1) / tiles_per_split;
}

template <int NDC>
void itc_launch(const ItcArgs& a, int rowtiles, hipStream_t s) {
    hipLaunchKernelGGL((itc_pass_kernel<NDC, false>), dim3(rowtiles, a.splits), dim3(ITC_THREADS), 0, s, a);
    hipLaunchKernelGGL(itc_combine1_kernel, dim3(a.B), dim3(ITC_C1_THREADS), 0, s, a);
    hipLaunchKernelGGL((itc_pass_kernel<NDC, true>), dim3(rowtiles, a.splits), dim3(ITC_THREADS), 0, s, a);
    hipLaunchKernelGGL(itc_combine2_kernel, dim3(a.B + 1, a.D / ITC_DC), dim3(ITC_C2_THREADS), 0, s, a);
}

template <int NDC>
void itc_wide_launch(const ItcArgs& a, int rowtiles, hipStream_t s) {
    hipLaunchKernelGGL((itc_wide_kernel<NDC, false>), dim3(rowtiles, a.splits), dim3(ITC_THREADS), 0, s, a);
    hipLaunchKernelGGL(itc_combine1_kernel, dim3(a.B), dim3(ITC_C1_THREADS), 0, s, a);
    hipLaunchKernelGGL((itc_wide_kernel<NDC, true>), dim3(rowtiles, a.splits), dim3(ITC_THREADS), 0, s, a);
    hipLaunchKernelGGL(itc_combine2_kernel, dim3(a.B + 1, a.D / ITC_DC), dim3(ITC_C2_THREADS), 0, s, a);
}

// ================================ EMA of the momentum encoders ===============================================================
// table: int64 [4, n]: rows = momentum pointer, source pointer, numel, first block of the tensor (prefix sum)
constexpr int EMA_THREADS = 256;
constexpr int EMA_PER_BLOCK = EMA_THREADS * 4 * 4;  // 4 float4 per thread

// p_m m + p (1 - m) with three roundings: hipcc contracts a*b + c*d into an FMA by default (also through the inlined __fmul_rn /
// __fadd_rn of the HIP headers), so the expression is written here with contraction off
__device__ __forceinline__ float ema1(float pm, float p, float m, float om) {
#pragma clang fp contract(off)
    return pm * m + p * om;
}

__global__ __launch_bounds__(EMA_THREADS) void ema_kernel(const int64_t* table, int n, float m, float om) {
    // the tensor this block belongs to: last t with first_block[t] <= blockIdx.x
    const int64_t* first = table + 3 * (size_t)n;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    float* pm = (float*)table[lo];
    const float* p = (const float*)table[n + lo];
    const int64_t numel = table[2 * (size_t)n + lo];
    const int64_t base = ((int64_t)blockIdx.x - first[lo]) * EMA_PER_BLOCK;
    const int64_t end = min(numel, base + (int64_t)EMA_PER_BLOCK);
    if (((((uintptr_t)pm) | ((uintptr_t)p)) & 15u) == 0) {
        const int64_t vend = base + ((end - base) & ~(int64_t)3);
        for (int64_t i = base + 4 * (int64_t)threadIdx.x; i < vend; i += 4 * EMA_THREADS) {
            f32x4 a = *(const f32x4*)(pm + i), b = *(const f32x4*)(p + i), r;
            for (int k = 0; k < 4; ++k) r[k] = ema1(a[k], b[k], m, om);
            *(f32x4*)(pm + i) = r;
        }
        for (int64_t i = vend + threadIdx.x; i < end; i += EMA_THREADS) pm[i] = ema1(pm[i], p[i], m, om);
    } else {
        for (int64_t i = base + threadIdx.x; i < end; i += EMA_THREADS) pm[i] = ema1(pm[i], p[i], m, om);
    }
}

// ================================ ITM hard negatives ===========================================================================
// blockIdx.y = direction (0: t2i, a negative image per text; 1: i2t, a negative text per image), blockIdx.x = row b.
constexpr int NEG_THREADS = 256;
constexpr int NEG_MAX_COLS = 8192;

__global__ __launch_bounds__(NEG_THREADS) void itm_neg_kernel(const float* img, const float* txt, const float* img_w, const float* txt_w,
                                                              const int64_t* idx, const int64_t* idx_w, const float* temp_p, const float* u,
                                                              int64_t* neg, int* flag, int B, int Bw, int D) {
    extern __shared__ float sm[];  // [D] query row, [Bw] weights
    float* f = sm;
    float* w = sm + D;
    __shared__ float red[NEG_THREADS];
    const int b = blockIdx.x, dir = blockIdx.y, t = threadIdx.x;
    const float* qrow = (dir == 0 ? txt : img) + (size_t)b * D;
    const float* keys = dir == 0 ? img_w : txt_w;
    const float temp = *temp_p;
    for (int d = t; d < D; d += NEG_THREADS) f[d] = qrow[d];
    __syncthreads();
    float mx = -INFINITY;
    for (int j = t; j < Bw; j += NEG_THREADS) {
        float acc = 0.f;
        for (int d = 0; d < D; ++d) acc = fmaf(f[d], keys[(size_t)j * D + d], acc);
        w[j] = acc / temp;
        mx = fmaxf(mx, w[j]);
    }
    red[t] = mx;
    __syncthreads();
    if (t == 0) {
        float m = -INFINITY;
        for (int i = 0; i < NEG_THREADS; ++i) m = fmaxf(m, red[i]);
        red[0] = m;
    }
    __syncthreads();
    mx = red[0];
    __syncthreads();
    float sum = 0.f;
    for (int j = t; j < Bw; j += NEG_THREADS) {
        w[j] = expf(w[j] - mx);
        sum += w[j];
    }
    red[t] = sum;
    __syncthreads();
    if (t == 0) {
        float s = 0.f;
        for (int i = 0; i < NEG_THREADS; ++i) s += red[i];
        const int64_t me = idx[b];
        float c = 0.f;
        for (int j = 0; j < Bw; ++j) {  // softmax, then the same-id columns set to 0 (blip_retrieval.py:234-238)
            w[j] = idx_w[j] == me ? 0.f : w[j] / s;
            c += w[j];
        }
        int64_t pick = -1;
        if (c > 0.f) {  // inverse CDF: the first column whose running sum exceeds u * total
            const float thr = u[dir * B + b] * c;
            float run = 0.f;
            for (int j = 0; j < Bw; ++j) {
                if (w[j] > 0.f) pick = j;  // fallback: the last non-zero column (u * total rounded to the total)
                run += w[j];
                if (w[j] > 0.f && run > thr) break;
            }
        } else {
            *flag = 1;
        }
        neg[dir * B + b] = pick;
    }
}

}  // namespace

extern "C" size_t madtp_itc_workspace(int B, int D, int Q) {
    if (B <= 0 || D <= 0 || Q < 0) return 0;
    int rowtiles, splits, tps;
    itc_geometry(B, D, Q, rowtiles, splits, tps);
    return sizeof(float) * ((size_t)splits * B * ITC_NSTAT + (size_t)B * 4 + (size_t)splits * B * D + (size_t)splits * B);
}

extern "C" int madtp_itc_loss(const float* q, const float* q_m, const float* keys_batch, const float* queue, const int64_t* idx,
                              const int64_t* idx_queue, const float* temp, float alpha, float* loss, float* dq, float* dtemp, void* ws,
                              size_t ws_bytes, int B, int D, int Q, void* stream) {
    if (!q || !q_m || !keys_batch || !idx || !temp || !loss || !dq || !dtemp || !ws || B <= 0 || D <= 0 || Q < 0)
        return MADTP_E_BADARG;
    if (Q > 0 && (!queue || !idx_queue)) return MADTP_E_BADARG;
    if (D % ITC_DC != 0 || D > 1024 || B > 256) return MADTP_E_SHAPE;
    if (ws_bytes < madtp_itc_workspace(B, D, Q)) return MADTP_E_BADARG;
    ItcArgs a;
    a.q = q; a.qm = q_m; a.kb = keys_batch; a.queue = queue; a.idx = idx; a.idxq = idx_queue; a.temp = temp; a.alpha = alpha;
    a.B = B; a.D = D; a.Q = Q; a.N = B + Q;
    int rowtiles;
    itc_geometry(B, D, Q, rowtiles, a.splits, a.tiles_per_split);
    float* w = (float*)ws;
    a.stats = w; w += (size_t)a.splits * B * ITC_NSTAT;
    a.rowinfo = w; w += (size_t)B * 4;
    a.dqpart = w; w += (size_t)a.splits * B * D;
    a.dtpart = w;
    a.loss = loss; a.dq = dq; a.dtemp = dtemp;
    hipStream_t s = (hipStream_t)stream;
    switch (D / ITC_DC) {
        case 1: itc_launch<1>(a, rowtiles, s); break;
        case 2: itc_launch<2>(a, rowtiles, s); break;
        case 3: itc_launch<3>(a, rowtiles, s); break;
        case 4: itc_launch<4>(a, rowtiles, s); break;
        case 5: itc_launch<5>(a, rowtiles, s); break;
        case 6: itc_launch<6>(a, rowtiles, s); break;
        case 7: itc_launch<7>(a, rowtiles, s); break;
        case 8: itc_launch<8>(a, rowtiles, s); break;
        case 9: itc_wide_launch<9>(a, rowtiles, s); break;
        case 10: itc_wide_launch<10>(a, rowtiles, s); break;
        case 11: itc_wide_launch<11>(a, rowtiles, s); break;
        case 12: itc_wide_launch<12>(a, rowtiles, s); break;
        case 13: itc_wide_launch<13>(a, rowtiles, s); break;
        case 14: itc_wide_launch<14>(a, rowtiles, s); break;
        case 15: itc_wide_launch<15>(a, rowtiles, s); break;
        default: itc_wide_launch<16>(a, rowtiles, s); break;
    }
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" int madtp_ema_update(const int64_t* table, int n_tensors, int n_blocks, float m, float one_minus_m, void* stream) {
    if (!table || n_tensors <= 0 || n_blocks <= 0) return MADTP_E_BADARG;
    hipLaunchKernelGGL(ema_kernel, dim3(n_blocks), dim3(EMA_THREADS), 0, (hipStream_t)stream, table, n_tensors, m, one_minus_m);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" int madtp_ema_blocks(int64_t numel) { return (int)((numel + EMA_PER_BLOCK - 1) / EMA_PER_BLOCK); }

extern "C" int madtp_itm_negatives(const float* image_feat, const float* text_feat, const float* image_feat_world,
                                   const float* text_feat_world, const int64_t* idx, const int64_t* idx_world, const float* temp,
                                   const float* u, int64_t* neg, int* flag, int B, int Bw, int D, void* stream) {
    if (!image_feat || !text_feat || !image_feat_world || !text_feat_world || !idx || !idx_world || !temp || !u || !neg || !flag ||
        B <= 0 || Bw <= 0 || D <= 0)
        return MADTP_E_BADARG;
    if (D % 64 != 0 || D > 512 || Bw < B || Bw > NEG_MAX_COLS) return MADTP_E_SHAPE;
    const size_t lds = (size_t)(D + Bw) * sizeof(float);
    MADTP_ENSURE_MAX_LDS(itm_neg_kernel, 40 * 1024);
    hipLaunchKernelGGL(itm_neg_kernel, dim3(B, 2), dim3(NEG_THREADS), lds, (hipStream_t)stream, image_feat, text_feat, image_feat_world,
                       text_feat_world, idx, idx_world, temp, u, neg, flag, B, Bw, D);
    MADTP_LAUNCH_CHECK();
    return 0;
}

// Retrieval search through a bf16 shortlist with an exactness certificate (include/madtp_csearch.h, which states and proves the
// bound).  Five stages on the caller's stream, no host round trip:
//
//   coarse_prepare_kernel   one wave per row: f32 -> bf16 (round to nearest even) and the row's statistics, rounded up
//   ctopk_tile_kernel       workgroup (32 query rows, key split): 32 x 64 coarse score tiles on v_mfma_f32_16x16x32_bf16 from bf16
//                           rows staged by 16-byte loads (the next chunk's loads are issued before the products of the current
//                           one); the epilogue is the selection of search_device.h, keeping the m best coarse words per row
//   ctopk_row_kernel        one workgroup per row: merges the splits' lists to the m best coarse words, scores those m keys again
//                           with the fmaf chain of eval_device.h (the bits of the exact route), sorts them by the contract's
//                           order, evaluates the certificate, writes the top k and the row's info
//   ctopk_compact_kernel    one workgroup: an ordered scan over the certified flags -> the ascending list of uncertified rows
//   fallback                topk_tile_kernel / topk_row_kernel of search_device.h, MAPPED over that list (a grid for nq rows,
//                           workgroups past the device-side count return at once)
#include "search_device.h"

#include "../../include/madtp_csearch.h"

namespace {

constexpr int CT_LD = 72;            // bf16 per LDS row of a 64-feature chunk: 144 bytes, 16-byte aligned rows
constexpr float CT_TWO_M126 = 1.17549435e-38f;  // 2^-126, the smallest normal f32 (and bf16)
constexpr float CT_TWO_P126 = 8.50705917e37f;   // 2^126

// ---- prepare ----------------------------------------------------------------------------------------------------------------------
// sqrt of a sum of squares formed on the row scaled by 2^-e, as an upper bound of the real norm: the f32 sum of <= 1024
// non-negative terms is low by less than 2^-13 relatively, and terms that underflowed after the scaling (below 2^-126 of the
// row's largest element) are covered by the floor 2^-100; sqrt and the product round by 2^-24 each; scaling back may round once
// more in the subnormal range, hence the last step up.
__device__ __forceinline__ float norm_up(float sum, int e) {
    const float n = ldexpf(sqrtf(sum * (1.0f + 0x1p-12f) + 0x1p-100f) * (1.0f + 0x1p-11f), e);
    return n < INFINITY ? __uint_as_float(__float_as_uint(n) + 1u) : n;  // (n > 0; NaN stays NaN)
}

__global__ __launch_bounds__(RK_THREADS) void coarse_prepare_kernel(const float* x, size_t ldx, int n, int D, bf16_t* x16, float* stats) {
    const int row = blockIdx.x * (RK_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;  // (a whole wave)
    const float* xr = x + (size_t)row * ldx;
    f32x4 v[4];
    float mx = 0.f;
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int col = (lane + 64 * c) * 4;
        v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (col < D) v[c] = *(const f32x4*)(xr + col);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float av = fabsf(v[c][i]);
            mx = fmaxf(mx, av);
            bad |= !(av < INFINITY) || (av != 0.f && av < CT_TWO_M126);
        }
    }
    mx = wave_max(mx);
    const int e = (mx > 0.f && mx < INFINITY) ? ilogbf(mx) : 0;
    float sx = 0.f, sd = 0.f, sh = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int col = (lane + 64 * c) * 4;
        if (col >= D) continue;
        const bf16x4 h = pack_bf16x4(v[c]);
        *(bf16x4*)(x16 + (size_t)row * D + col) = h;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float xh = bf16_to_f32((bf16_t)h[i]);
            bad |= !(fabsf(xh) < INFINITY);
            const float a = ldexpf(v[c][i], -e), d = ldexpf(v[c][i] - xh, -e), b = ldexpf(xh, -e);  // (x - x16 is exact in f32)
            sx = fmaf(a, a, sx);
            sd = fmaf(d, d, sd);
            sh = fmaf(b, b, sh);
        }
    }
    sx = wave_sum(sx);
    sd = wave_sum(sd);
    sh = wave_sum(sh);
    const bool flag = __any(bad);
    if (lane == 0) {
        f32x4 st = {0.f, 0.f, 0.f, flag ? 1.f : 0.f};
        if (mx != 0.f) {  // (an all-zero row has exact zeros)
            st[0] = norm_up(sx, e);
            st[1] = sd == 0.f ? 0.f : norm_up(sd, e);  // a row of bf16 numbers has no operand error
            st[2] = norm_up(sh, e);
        }
        *(f32x4*)(stats + (size_t)row * MADTP_COARSE_STATS) = st;
    }
}

__global__ __launch_bounds__(RK_THREADS) void coarse_summary_kernel(const float* stats, int n, float* summary, int fold) {
    __shared__ f32x4 part[RK_THREADS];
    const int t = threadIdx.x;
    f32x4 m = {0.f, 0.f, 0.f, 0.f};
    for (int r = t; r < n; r += RK_THREADS) {
        const f32x4 s = *(const f32x4*)(stats + (size_t)r * MADTP_COARSE_STATS);
        for (int i = 0; i < 4; ++i) m[i] = fmaxf(m[i], s[i]);  // (a NaN norm belongs to a flagged row: the flag carries it)
    }
    part[t] = m;
    __syncthreads();
    for (int o = RK_THREADS / 2; o > 0; o >>= 1) {
        if (t < o)
            for (int i = 0; i < 4; ++i) part[t][i] = fmaxf(part[t][i], part[t + o][i]);
        __syncthreads();
    }
    if (t == 0) {
        m = part[0];
        if (fold)
            for (int i = 0; i < 4; ++i) m[i] = fmaxf(m[i], summary[i]);
        *(f32x4*)summary = m;
    }
}

// ---- coarse tiles -----------------------------------------------------------------------------------------------------------------
// acc0 / acc1 = rows [r0, r0 + 16) / [r0 + 16, r0 + 32) of q16 against the keys [64 tile, 64 tile + 64) of k16, in the accumulator
// layout of rank_tile_products: for v_mfma_f32_16x16x32_bf16 lane l holds A[l & 15][8 (l >> 4) + j] and B[8 (l >> 4) + j][l & 15],
// j < 8, and C[row 4 (l >> 4) + i][col l & 15] in register i.  A = the query rows, B = the key rows of wave w's 16 columns.
__device__ __forceinline__ void coarse_tile_products(const bf16_t* q16, const bf16_t* k16, int nq, int nk, int D, int r0, int tile,
                                                     bf16_t (*Qs)[CT_LD], bf16_t (*Ks)[CT_LD], f32x4& acc0, f32x4& acc1) {
    const int t = threadIdx.x, w = t >> 6, c = t & 15, g = (t >> 4) & 3;
    const int sr = t >> 3, d8 = (t & 7) * 8;  // thread t stages 8 features of q row sr and of key rows sr, sr + 32
    const int ndc = D / RK_DC;
    const int qrow = r0 + sr < nq ? r0 + sr : -1;
    int krow[2];
    for (int i = 0; i < 2; ++i) {
        const int kr = tile * RK_CT + sr + 32 * i;
        krow[i] = kr < nk ? kr : -1;
    }
    u32x4 qreg, kreg[2];
    auto fetch = [&](int dc) {
        qreg = u32x4{0u, 0u, 0u, 0u};
        if (qrow >= 0) qreg = *(const u32x4*)(q16 + (size_t)qrow * D + dc * RK_DC + d8);
        for (int i = 0; i < 2; ++i) {
            kreg[i] = u32x4{0u, 0u, 0u, 0u};
            if (krow[i] >= 0) kreg[i] = *(const u32x4*)(k16 + (size_t)krow[i] * D + dc * RK_DC + d8);
        }
    };
    acc0 = f32x4{0.f, 0.f, 0.f, 0.f};
    acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
    fetch(0);
    for (int dc = 0; dc < ndc; ++dc) {
        *(u32x4*)&Qs[sr][d8] = qreg;
        for (int i = 0; i < 2; ++i) *(u32x4*)&Ks[sr + 32 * i][d8] = kreg[i];
        __syncthreads();
        if (dc + 1 < ndc) fetch(dc + 1);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const bf16x8 qa0 = *(const bf16x8*)&Qs[c][32 * s + 8 * g], qa1 = *(const bf16x8*)&Qs[16 + c][32 * s + 8 * g];
            const bf16x8 kb = *(const bf16x8*)&Ks[16 * w + c][32 * s + 8 * g];
            acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa0, kb, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa1, kb, acc1, 0, 0, 0);
        }
        lds_barrier();  // the tiles are free again; the loads in flight stay in flight
    }
}

template <int CAP> __global__ __launch_bounds__(RK_THREADS)
void ctopk_tile_kernel(const bf16_t* q16, const bf16_t* k16, int nq, int nk, int D, int tiles_per_split, int m, u64* part) {
    __shared__ __attribute__((aligned(16))) bf16_t Qs[RK_RT][CT_LD];
    __shared__ __attribute__((aligned(16))) bf16_t Ks[RK_CT][CT_LD];
    __shared__ u64 thresh[RK_RT];
    __shared__ int count[RK_RT];
    extern __shared__ __attribute__((aligned(16))) u64 cand[];  // [RK_RT][CAP]
    const int r0 = blockIdx.x * RK_RT, split = blockIdx.y;
    tile_select_init<CAP>(cand, count, thresh);
    const int ntiles = (nk + RK_CT - 1) / RK_CT;
    const int tile0 = split * tiles_per_split, tile1 = min(ntiles, tile0 + tiles_per_split);
    for (int tile = tile0; tile < tile1; ++tile) {
        f32x4 acc0, acc1;
        coarse_tile_products(q16, k16, nq, nk, D, r0, tile, Qs, Ks, acc0, acc1);
        tile_select_add<CAP>(acc0, acc1, tile, nk, cand, count, thresh, m);
    }
    tile_select_finish<CAP>(cand, count, thresh, m, r0, nq, nq, split, part);
}

// ---- the row kernel ---------------------------------------------------------------------------------------------------------------
struct CRowArgs {
    const float *q, *keys;
    size_t ldq, ldk;
    const float *qstats, *summary;
    const u64* part;
    int nq, nk, D, k, m, splits;
    float* values;
    int32_t *indices, *info, *sl_idx;
    float* sl_coarse;
};

// <q, key> with the bits of rank_tile_products: the fmaf chain over the features in the order chunk, j, e, g of feature
// 64 chunk + 16 j + 4 g + e (v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain, one rounding per product, g its k index).
__device__ __forceinline__ float exact_score(const float* qs, const float* key, int D) {
    float acc = 0.f;
    for (int ch = 0; ch < D / RK_DC; ++ch) {
        f32x4 kv[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) kv[i] = *(const f32x4*)(key + ch * RK_DC + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int g = 0; g < 4; ++g) acc = __builtin_fmaf(qs[ch * RK_DC + 16 * j + 4 * g + e], kv[4 * j + g][e], acc);
    }
    return acc;
}

__global__ __launch_bounds__(RK_THREADS) void ctopk_row_kernel(CRowArgs a) {
    __shared__ u64 buf[TK_ROW_CAP];
    __shared__ u64 thresh;
    __shared__ int count;
    __shared__ __attribute__((aligned(16))) float qs[1024];
    const int t = threadIdx.x, r = blockIdx.x, m = a.m, k = a.k;
    if (4 * t < a.D) *(f32x4*)&qs[4 * t] = *(const f32x4*)(a.q + (size_t)r * a.ldq + 4 * t);
    row_select<false>(nullptr, a.part, a.nq, r, a.splits * m, m, buf, &count, &thresh);  // (its barriers settle qs too)
    const u64 cw = t < m ? buf[t] : 0;  // the shortlist, best coarse word first
    const u64 cm_word = buf[m - 1];
    __syncthreads();
    if (t < m) {
        u64 word = 0;
        if (cw) {
            const int idx = (int)(uint32_t)cw;
            word = candidate(exact_score(qs, a.keys + (size_t)idx * a.ldk, a.D), idx);
        }
        buf[t] = word;
    }
    if (t == 0) count = m;
    __syncthreads();
    sort_and_cut<TK_ROW_CAP, 1, false>(buf, &count, &thresh, k);
    if (t < k) {
        const u64 word = buf[t];
        a.values[(size_t)r * k + t] = word ? bits_score((uint32_t)(word >> 32)) : -INFINITY;
        a.indices[(size_t)r * k + t] = word ? (int)(uint32_t)word : -1;
    }
    if (a.sl_idx && t < m) {
        a.sl_idx[(size_t)r * m + t] = cw ? (int)(uint32_t)cw : -1;
        a.sl_coarse[(size_t)r * m + t] = cw ? bits_score((uint32_t)(cw >> 32)) : -INFINITY;
    }
    if (t == 0) {  // the certificate (madtp_csearch.h)
        const f32x4 qst = *(const f32x4*)(a.qstats + (size_t)r * MADTP_COARSE_STATS), sm = *(const f32x4*)a.summary;
        const float u = 0x1p-24f, Df = (float)a.D;
        const float p1 = qst[0] * sm[0], p3 = qst[2] * sm[2];
        const float E = ((qst[1] * sm[0] + qst[2] * sm[1]) + (Df + 2.f) * u * p1 + (float)MADTP_CTOPK_ACC_FACTOR * Df * u * p3) *
                            (1.0f + 0x1p-10f) + (3.f * Df + 8.f) * CT_TWO_M126;
        const float c_m = cm_word ? bits_score((uint32_t)(cm_word >> 32)) : -INFINITY;
        bool ok = qst[3] == 0.f && sm[3] == 0.f && p1 < CT_TWO_P126 && p3 < CT_TWO_P126;  // (a NaN fails every comparison)
        if (ok && a.nk > m) {
            const float s_k = bits_score((uint32_t)(thresh >> 32));  // thresh = the k-th word: m >= 2 k of nk > m keys are listed
            ok = (double)s_k > (double)c_m + (double)E;
        }
        a.info[(size_t)r * MADTP_CTOPK_INFO + 0] = ok ? 1 : 0;
        a.info[(size_t)r * MADTP_CTOPK_INFO + 1] = (int32_t)__float_as_uint(c_m);
        a.info[(size_t)r * MADTP_CTOPK_INFO + 2] = (int32_t)__float_as_uint(E);
    }
}

// ---- compaction -------------------------------------------------------------------------------------------------------------------
// thread t owns the rows [t per, (t + 1) per): counts its uncertified ones, an exclusive scan over the 256 counts gives its first
// position, and it writes its rows in order.  head[0] = the count, list = head + 4 (byte 16).
__global__ __launch_bounds__(RK_THREADS) void ctopk_compact_kernel(int32_t* info, int nq, int32_t* head) {
    __shared__ int sc[RK_THREADS];
    const int t = threadIdx.x, per = (nq + RK_THREADS - 1) / RK_THREADS;
    const int lo = min(nq, t * per), hi = min(nq, lo + per);
    int n = 0;
    for (int r = lo; r < hi; ++r) n += info[(size_t)r * MADTP_CTOPK_INFO] == 0;
    sc[t] = n;
    __syncthreads();
    for (int o = 1; o < RK_THREADS; o <<= 1) {  // inclusive scan
        const int add = t >= o ? sc[t - o] : 0;
        __syncthreads();
        sc[t] += add;
        __syncthreads();
    }
    int pos = sc[t] - n;
    int32_t* list = head + 4;
    for (int r = lo; r < hi; ++r) {
        const bool un = info[(size_t)r * MADTP_CTOPK_INFO] == 0;
        info[(size_t)r * MADTP_CTOPK_INFO + 3] = un ? pos : -1;
        if (un) list[pos++] = r;
    }
    if (t == RK_THREADS - 1) head[0] = sc[t];
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

struct CtopkLayout {
    size_t list, qstats, q16, cpart, xpart, total;  // byte offsets into ws (the count is at 0)
};

CtopkLayout ctopk_layout(int nq, int nk, int D, int k, int m) {
    const size_t rows = topk_geometry(nq, nk).ws_rows;
    CtopkLayout l;
    l.list = 16;
    l.qstats = l.list + up16(sizeof(int32_t) * (size_t)nq);
    l.q16 = l.qstats + sizeof(float) * MADTP_COARSE_STATS * (size_t)nq;
    l.cpart = l.q16 + sizeof(bf16_t) * (size_t)D * (size_t)nq;
    l.xpart = l.cpart + sizeof(u64) * (size_t)m * rows;
    l.total = l.xpart + sizeof(u64) * (size_t)k * rows;
    return l;
}

bool ctopk_km_ok(int k, int m) { return k >= 1 && k <= MADTP_CTOPK_MAX_K && (m == 64 || m == 128 || m == 256) && m >= 2 * k; }

template <int CAP> int launch_ctopk_tiles(const bf16_t* q16, const bf16_t* k16, int nq, int nk, int D, int m, const TopkGeometry& g,
                                          u64* part, hipStream_t s) {
    constexpr size_t lds = sizeof(u64) * RK_RT * CAP;
    MADTP_ENSURE_MAX_LDS(ctopk_tile_kernel<CAP>, lds);
    hipLaunchKernelGGL(ctopk_tile_kernel<CAP>, dim3(g.rowtiles, g.splits), dim3(RK_THREADS), lds, s, q16, k16, nq, nk, D,
                       g.tiles_per_split, m, part);
    return 0;
}

int launch_prepare(const float* x, int ldx, int n, int D, bf16_t* x16, float* stats, hipStream_t s) {
    constexpr int rows = RK_THREADS / 64;
    hipLaunchKernelGGL(coarse_prepare_kernel, dim3((n + rows - 1) / rows), dim3(RK_THREADS), 0, s, x, (size_t)ldx, n, D, x16, stats);
    return 0;
}

}  // namespace

extern "C" int madtp_csearch_abi_version(void) { return MADTP_CSEARCH_ABI_VERSION; }

extern "C" int madtp_coarse_prepare(const float* x, int ldx, int n, int D, void* x16, float* stats, void* stream) {
    if (!x || !x16 || !stats) return MADTP_E_BADARG;
    if (n <= 0 || D % RK_DC != 0 || D < 64 || D > 1024 || ldx < D || ldx % 4 != 0) return MADTP_E_SHAPE;
    if (!aligned16(x) || !aligned16(x16) || !aligned16(stats)) return MADTP_E_BADARG;
    launch_prepare(x, ldx, n, D, (bf16_t*)x16, stats, (hipStream_t)stream);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" int madtp_coarse_summary(const float* stats, int n, float* summary, int fold, void* stream) {
    if (!stats || !summary || !aligned16(stats) || !aligned16(summary)) return MADTP_E_BADARG;
    if (n <= 0) return MADTP_E_SHAPE;
    hipLaunchKernelGGL(coarse_summary_kernel, dim3(1), dim3(RK_THREADS), 0, (hipStream_t)stream, stats, n, summary, fold);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t madtp_ctopk_workspace(int nq, int nk, int D, int k, int m) {
    if (!topk_shape_ok(nq, nk, D) || !ctopk_km_ok(k, m)) return 0;
    return ctopk_layout(nq, nk, D, k, m).total;
}

extern "C" int madtp_ctopk_embeds(const float* q, int ldq, const float* keys, int ldk, const void* keys16, const float* key_stats_summary,
                                  int nq, int nk, int D, int k, int m, float* values, int32_t* indices, int32_t* info,
                                  int32_t* shortlist_indices, float* shortlist_coarse, void* ws, size_t ws_bytes, void* stream) {
    if (!q || !keys || !keys16 || !key_stats_summary || !values || !indices || !info || !ws) return MADTP_E_BADARG;
    if ((shortlist_indices == nullptr) != (shortlist_coarse == nullptr)) return MADTP_E_BADARG;
    if (!ctopk_km_ok(k, m)) return MADTP_E_BADARG;
    if (!topk_shape_ok(nq, nk, D) || ldq < D || ldk < D || ldq % 4 != 0 || ldk % 4 != 0) return MADTP_E_SHAPE;
    if (!aligned16(q) || !aligned16(keys) || !aligned16(keys16) || !aligned16(key_stats_summary) || !aligned16(ws)) return MADTP_E_BADARG;
    if (ws_bytes < madtp_ctopk_workspace(nq, nk, D, k, m)) return MADTP_E_BADARG;
    const TopkGeometry g = topk_geometry(nq, nk);
    const CtopkLayout l = ctopk_layout(nq, nk, D, k, m);
    char* base = (char*)ws;
    int32_t* head = (int32_t*)base;
    float* qstats = (float*)(base + l.qstats);
    bf16_t* q16 = (bf16_t*)(base + l.q16);
    u64 *cpart = (u64*)(base + l.cpart), *xpart = (u64*)(base + l.xpart);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    // 1. the queries' bf16 rows and statistics
    launch_prepare(q, ldq, nq, D, q16, qstats, s);
    // 2. coarse tiles: the m best coarse words per row and split
    const bf16_t* k16 = (const bf16_t*)keys16;
    if (m == 64) rc = launch_ctopk_tiles<128>(q16, k16, nq, nk, D, m, g, cpart, s);
    else if (m == 128) rc = launch_ctopk_tiles<256>(q16, k16, nq, nk, D, m, g, cpart, s);
    else rc = launch_ctopk_tiles<512>(q16, k16, nq, nk, D, m, g, cpart, s);
    if (rc != 0) return rc;
    // 3. merge, exact scores of the shortlist, certificate
    CRowArgs ra = {};
    ra.q = q; ra.keys = keys; ra.ldq = (size_t)ldq; ra.ldk = (size_t)ldk; ra.qstats = qstats; ra.summary = key_stats_summary;
    ra.part = cpart; ra.nq = nq; ra.nk = nk; ra.D = D; ra.k = k; ra.m = m; ra.splits = g.splits;
    ra.values = values; ra.indices = indices; ra.info = info; ra.sl_idx = shortlist_indices; ra.sl_coarse = shortlist_coarse;
    hipLaunchKernelGGL(ctopk_row_kernel, dim3(nq), dim3(RK_THREADS), 0, s, ra);
    // 4. the list of uncertified rows
    hipLaunchKernelGGL(ctopk_compact_kernel, dim3(1), dim3(RK_THREADS), 0, s, info, nq, head);
    // 5. the exact route over the listed rows
    RankArgs a = {};
    a.q = q; a.keys = keys; a.ldq = ldq; a.ldk = ldk; a.nq = nq; a.nk = nk; a.D = D;
    a.splits = g.splits; a.tiles_per_split = g.tiles_per_split;
    a.row_map = head + 4; a.row_count = head;
    if (k <= 64) rc = launch_topk_tiles<128, true>(a, k, g, xpart, s);
    else rc = launch_topk_tiles<256, true>(a, k, g, xpart, s);
    if (rc != 0) return rc;
    hipLaunchKernelGGL((topk_row_kernel<false, true>), dim3(nq), dim3(RK_THREADS), 0, s, (const float*)nullptr, (size_t)0, xpart, nq,
                       g.splits * k, k, values, indices, (const int32_t*)(head + 4), (const int32_t*)head);
    MADTP_LAUNCH_CHECK();
    return 0;
}

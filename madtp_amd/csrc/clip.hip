// The two ends of CLIP's text tower under autograd (clip/model.py:486-488):
//   clip_embed      x[b,l,:] = table[ids[b,l],:] + pos[l,:]               one pass, one wave per row, float4 lanes
//   embedding_grad  dtable[v,:] = sum over the occurrences of v in ids of dx[b,l,:], in ascending flat position b*L + l
// The gradient is a segmented sum over the ids in sorted order instead of a scatter of atomic adds:
//   1. embed_rank_kernel: rank-by-counting (the rule of token_select): rank(i) = #{j : (ids[j], j) < (ids[i], i)} - a stable
//      sort of the n <= 19712 positions in one pass, O(n^2) integer compares spread over n/64 workgroups.  It writes the sorted
//      ids and the permutation to the workspace.
//   2. embed_grad_kernel: one wave per (16 consecutive table rows, 256-column slice): one binary search of the first row in the
//      sorted ids, then for each row the sequential f32 sum of its occurrences in sorted (= ascending position) order, or a row
//      of zeros when it does not occur; a segment of 64 or more occurrences is shared by the four waves of its workgroup.
//      Every element of dtable is written exactly once by a vector store, so there is no memset, no atomic and no dependence on
//      the prior contents; the order of the additions is fixed by the data alone (bit-identical across calls).
// The hand-over between the two kernels is the kernel boundary of one stream: no cross-workgroup traffic inside a launch.
// Roofline: HBM writes of V*D*4 bytes (101 MB at 49408 x 512) plus n*D*4 bytes read; the long segment of the padding id (about
// 60 of every 77 positions) is one dependent chain per column, fed by 64 row loads in flight in each of D / 64 waves.
#include "common.h"
#include "internal.h"

namespace {

__global__ __launch_bounds__(256) void clip_embed_kernel(const int64_t* __restrict__ ids, const float* __restrict__ table,
                                                         const float* __restrict__ pos, float* __restrict__ x, int rows, int L,
                                                         int dim) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* tr = table + (size_t)ids[row] * dim;
    const float* pr = pos + (size_t)(row % L) * dim;
    float* xr = x + (size_t)row * dim;
    for (int col = lane * 4; col < dim; col += 256) {
        const float4 a = *(const float4*)(tr + col), b = *(const float4*)(pr + col);
        *(float4*)(xr + col) = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
}

constexpr int RANK_TILE = 1024;  // ids staged in LDS per step (8 KiB)

// 64 positions per workgroup; wave q of the four counts over the q-th quarter of every staged tile, the counts meet in LDS
__global__ __launch_bounds__(256) void embed_rank_kernel(const int64_t* __restrict__ ids, int64_t* __restrict__ skeys,
                                                         int32_t* __restrict__ order, int n) {
    __shared__ int64_t tile[RANK_TILE];
    __shared__ int part[4][64];
    const int il = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + il;
    const int64_t key = i < n ? ids[i] : 0;
    int cnt = 0;
    for (int base = 0; base < n; base += RANK_TILE) {
        const int m = min(RANK_TILE, n - base);
        __syncthreads();
        for (int t = threadIdx.x; t < m; t += 256) tile[t] = ids[base + t];
        __syncthreads();
        const int j0 = q * (RANK_TILE / 4), j1 = min(m, j0 + RANK_TILE / 4);
        for (int j = j0; j < j1; ++j) {
            const int64_t kj = tile[j];  // (one address per wave: an LDS broadcast)
            cnt += (kj < key || (kj == key && base + j < i)) ? 1 : 0;
        }
    }
    part[q][il] = cnt;
    __syncthreads();
    if (q == 0 && i < n) {
        const int r = (part[0][il] + part[1][il]) + (part[2][il] + part[3][il]);  // a permutation of [0, n): (id, position) is a total order
        skeys[r] = key;
        order[r] = i;
    }
}

__device__ __forceinline__ int lower_bound_i64(const int64_t* __restrict__ a, int n, int64_t v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

constexpr int GRAD_UNROLL = 8;
constexpr int GRAD_LONG = 64;  // occurrences from which the four waves of a workgroup share one segment
constexpr int GRAD_ROWS = 16;  // consecutive table rows per wave: one binary search finds the first, the rest follow in order

// Wave w of a workgroup owns unit 4 * blockIdx.x + w = (256-column slice, chunk of GRAD_ROWS table rows).  It finds its first row
// in the sorted ids once and walks on from there; most rows do not occur and are written as zeros.  A short segment (fewer than
// GRAD_LONG occurrences) is summed by the wave alone, a float4 per lane.  A long one - the padding id's - is one dependent chain
// per column whatever is done, so what counts is the number of row loads in flight: it is left on a list in LDS, and the four
// waves then take 64 columns of its slice each, a float per lane, with 64 rows in flight per wave (their positions fetched one
// batch ahead by one coalesced load and handed out with readlane).  Either way every column's additions run in sorted order.
__global__ __launch_bounds__(256) void embed_grad_kernel(const float* __restrict__ dx, const int64_t* __restrict__ skeys,
                                                         const int32_t* __restrict__ order, float* __restrict__ dtable, int n,
                                                         int dim, int V, int n_chunks, long long n_units) {
    __shared__ int longs[4][GRAD_ROWS][3];  // (row, first, end) of the long segments each wave met
    __shared__ int n_long[4], slice_of[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long unit = (long long)blockIdx.x * 4 + wv;
    const bool live = unit < n_units;
    const int slice = live ? (int)(unit / n_chunks) : 0;  // (slice-major: the slices of one row run in different workgroups)
    const int v0 = live ? (int)(unit % n_chunks) * GRAD_ROWS : 0;
    const int v1 = live ? min(V, v0 + GRAD_ROWS) : 0;
    const int col = slice * 256 + lane * 4;
    int r = live ? lower_bound_i64(skeys, n, v0) : 0;
    int nl = 0;
    for (int v = v0; v < v1; ++v) {
        const int lo = r;
        if (r < n && skeys[r] == v) r = lower_bound_i64(skeys, n, (int64_t)v + 1);
        const int hi = r;
        if (hi - lo >= GRAD_LONG) {
            if (lane == 0) { longs[wv][nl][0] = v; longs[wv][nl][1] = lo; longs[wv][nl][2] = hi; }
            ++nl;
            continue;
        }
        if (col >= dim) continue;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        int k = lo;
        for (; k + GRAD_UNROLL <= hi; k += GRAD_UNROLL) {
            float4 t[GRAD_UNROLL];
#pragma unroll
            for (int u = 0; u < GRAD_UNROLL; ++u) t[u] = *(const float4*)(dx + (size_t)order[k + u] * dim + col);
#pragma unroll
            for (int u = 0; u < GRAD_UNROLL; ++u) { acc.x += t[u].x; acc.y += t[u].y; acc.z += t[u].z; acc.w += t[u].w; }
        }
        for (; k < hi; ++k) {
            const float4 t = *(const float4*)(dx + (size_t)order[k] * dim + col);
            acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
        }
        *(float4*)(dtable + (size_t)v * dim + col) = acc;
    }
    if (lane == 0) { n_long[wv] = nl; slice_of[wv] = slice; }
    __syncthreads();
    for (int p = 0; p < 4; ++p) {
        for (int q = 0; q < n_long[p]; ++q) {  // (the same trip counts in all four waves)
            const int v = longs[p][q][0], plo = longs[p][q][1], phi = longs[p][q][2];
            const int c = slice_of[p] * 256 + wv * 64 + lane;
            const bool ok = c < dim;
            const float* src = dx + (ok ? c : 0);
            float acc = 0.f;
            int mine = plo + lane < phi ? order[plo + lane] : 0;
            for (int k = plo; k < phi; k += 64) {
                const int cnt = min(64, phi - k);
                const int cur = mine;
                mine = k + 64 + lane < phi ? order[k + 64 + lane] : 0;  // the next batch's positions
                float t[64];
#pragma unroll
                for (int u = 0; u < 64; ++u) {
                    const int o = __shfl(cur, u, 64);  // (lanes past cnt hold position 0: a valid row, loaded and not added)
                    t[u] = src[(size_t)o * dim];
                }
#pragma unroll
                for (int u = 0; u < 64; ++u)
                    if (u < cnt) acc += t[u];
            }
            if (ok) dtable[(size_t)v * dim + c] = acc;
        }
    }
}

constexpr int EMBED_GRAD_MAX_N = 256 * 77;

}  // namespace

extern "C" int madtp_clip_embed(const int64_t* ids, const float* table, const float* pos, float* x, int B, int L, int D, int V,
                                void* stream) {
    if (!ids || !table || !pos || !x || B <= 0 || L <= 0 || V <= 0) return MADTP_E_BADARG;
    if (D <= 0 || D % 4 != 0 || (long long)B * L > 0x7fffffffLL / 4) return MADTP_E_SHAPE;
    const int rows = B * L;
    hipLaunchKernelGGL(clip_embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, ids, table, pos, x, rows, L, D);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t madtp_embedding_grad_workspace(int n) {
    if (n <= 0 || n > EMBED_GRAD_MAX_N) return 0;
    return (size_t)n * (sizeof(int64_t) + sizeof(int32_t));
}

extern "C" int madtp_embedding_grad(const int64_t* ids, const float* dx, float* dtable, void* ws, size_t ws_bytes, int n, int D,
                                    int V, void* stream) {
    if (!ids || !dx || !dtable || !ws || n <= 0 || V <= 0) return MADTP_E_BADARG;
    if (n > EMBED_GRAD_MAX_N || D <= 0 || D % 64 != 0 || D > 1024) return MADTP_E_SHAPE;
    if (ws_bytes < madtp_embedding_grad_workspace(n) || (((uintptr_t)ws) & 7u)) return MADTP_E_BADARG;
    int64_t* skeys = (int64_t*)ws;
    int32_t* order = (int32_t*)(skeys + n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(embed_rank_kernel, dim3((n + 63) / 64), dim3(256), 0, s, ids, skeys, order, n);
    MADTP_LAUNCH_CHECK();
    const int slices = (D + 255) / 256;
    const int n_chunks = (V + GRAD_ROWS - 1) / GRAD_ROWS;
    const long long n_units = (long long)n_chunks * slices;
    if ((n_units + 3) / 4 > 0x7fffffffLL) return MADTP_E_SHAPE;
    hipLaunchKernelGGL(embed_grad_kernel, dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, s, dx, skeys, order, dtable, n, D, V, n_chunks,
                       n_units);
    MADTP_LAUNCH_CHECK();
    return 0;
}

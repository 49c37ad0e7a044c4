// Re-ranked candidate lists (include/madtp_lists.h): idx int64 [n, k] / val f32 [n, k] stand for the dense row "val of the slot that
// holds j, `fill` for a key in no slot".  Two kernels that never form that row:
//
//   lists_rank_kernel   one wave per row.  Lane l keeps the slots l, l + 64, l + 128, l + 192 in registers.  Per target: a ballot finds
//                       the slot that holds it (s_t = its value, else `fill`), every lane counts its filled slots that stand before
//                       the target (rank_beats of eval_device.h, the comparison of madtp_rank_scores) and those with a larger key
//                       index, both <= 256 and packed into one int, summed over the wave.  The keys in no slot all score `fill`:
//                       they stand before the target either all (fill > s_t), or those above it (fill == s_t), or not at all, and
//                       how many those are follows from nk, the number of filled slots and the second count.
//   lists_sort_kernel   a workgroup sorts LS_ROWS rows as the 64-bit candidate words of search_device.h with its LDS bitonic network:
//                       the words' unsigned order is the contract order of madtp_search.h, an empty slot is the word 0, last.
//
// Integer counts and a total order: identical calls give identical bits.  No atomics.
#include <limits.h>

#include "search_device.h"  // candidate words and sort_rows_desc; eval_device.h (rank_beats, RK_MAXT, RK_THREADS) through it

#include "../../include/madtp_lists.h"

namespace {

static_assert(RK_MAXT == MADTP_LISTS_MAX_TARGETS, "the target limit of madtp_rank_scores");
static_assert(MADTP_LISTS_MAX_K == 256, "four slots per lane of a wave");

constexpr int LR_THREADS = 256;  // four waves = four rows per workgroup
constexpr int LR_SLOTS = MADTP_LISTS_MAX_K / 64;

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(LR_THREADS) void lists_rank_kernel(const int64_t* idx, size_t ld_idx, const float* val, size_t ld_val, int n,
                                                                int k, int nk, float fill, const int32_t* tgt_ptr,
                                                                const int32_t* tgt_idx, int32_t* rank_row, int32_t* rank_tgt) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (LR_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= n) return;  // (uniform over the wave; the kernel has no workgroup barrier)
    // the row's span as madtp_rank_scores reads it: outside [0, tgt_ptr[n]] or backwards = an empty row, 16 targets at most
    const int lo = tgt_ptr[r], hi = tgt_ptr[r + 1];
    const int nt = (lo < 0 || hi > tgt_ptr[n] || hi < lo) ? 0 : min(hi - lo, RK_MAXT);
    if (nt == 0) {
        if (lane == 0) rank_row[r] = nk;
        return;
    }
    // this lane's slots; an empty one is key -1 with a NaN, which rank_beats never counts
    int key[LR_SLOTS];
    float s[LR_SLOTS];
    int filled = 0;
#pragma unroll
    for (int i = 0; i < LR_SLOTS; ++i) {
        const int slot = lane + 64 * i;
        key[i] = -1;
        s[i] = __builtin_nanf("");
        if (slot < k) {
            const int64_t j = idx[(size_t)r * ld_idx + slot];
            if (j >= 0 && j < (int64_t)nk) {
                key[i] = (int)j;
                s[i] = val[(size_t)r * ld_val + slot];
                ++filled;
            }
        }
    }
    filled = wave_sum_int(filled);
    int best = nk;
    for (int t = 0; t < nt; ++t) {
        const int tc = tgt_idx[lo + t];
        int rank = nk;
        if (tc >= 0 && tc < nk) {
            // the slot that holds the target, if one does (no key occurs twice)
            bool mine = false;
            float sm = 0.f;
#pragma unroll
            for (int i = 0; i < LR_SLOTS; ++i)
                if (key[i] == tc) {
                    mine = true;
                    sm = s[i];
                }
            const unsigned long long held = __ballot(mine);
            const bool present = held != 0ull;
            const float from = __shfl(sm, present ? __ffsll((long long)held) - 1 : 0, 64);
            const float st = present ? from : fill;
            int c = 0;  // (slots before the target) | (filled slots with a larger key) << 16
#pragma unroll
            for (int i = 0; i < LR_SLOTS; ++i) c += rank_beats(s[i], key[i], st, tc) + ((key[i] > tc) << 16);
            c = wave_sum_int(c);
            const int before = c & 0xffff, larger = c >> 16;
            // the keys in no slot, the target itself left out: all of them score `fill`
            const int absent = nk - filled - (present ? 0 : 1);
            const int absent_larger = (nk - 1 - tc) - larger;
            rank = before + (fill > st ? absent : fill == st ? absent_larger : 0);
            best = min(best, rank);
        }
        if (lane == 0) rank_tgt[lo + t] = rank;
    }
    if (lane == 0) rank_row[r] = best;
}

constexpr int LS_ROWS = 8;  // rows per workgroup: every thread of sort_stage has a whole number of pairs at CAP 64, 128 and 256

template <int CAP> __global__ __launch_bounds__(RK_THREADS) void lists_sort_kernel(const int64_t* idx, size_t ld_idx, const float* val,
                                                                                  size_t ld_val, int n, int k, int nk, int64_t* out_idx,
                                                                                  float* out_val) {
    __shared__ u64 buf[LS_ROWS * CAP];
    const int r0 = blockIdx.x * LS_ROWS;
    for (int e = threadIdx.x; e < LS_ROWS * CAP; e += RK_THREADS) {
        const int r = r0 + e / CAP, slot = e % CAP;
        u64 word = 0;
        if (r < n && slot < k) {
            const int64_t j = idx[(size_t)r * ld_idx + slot];
            if (j >= 0 && j < (int64_t)nk) word = candidate(val[(size_t)r * ld_val + slot], (int)j);
        }
        buf[e] = word;
    }
    __syncthreads();
    sort_rows_desc<CAP, LS_ROWS, false>(buf);  // (ends with a barrier)
    for (int e = threadIdx.x; e < LS_ROWS * CAP; e += RK_THREADS) {
        const int r = r0 + e / CAP, slot = e % CAP;
        if (r < n && slot < k) {
            const u64 word = buf[e];
            out_idx[(size_t)r * k + slot] = word ? (int64_t)(uint32_t)word : -1;
            out_val[(size_t)r * k + slot] = word ? bits_score((uint32_t)(word >> 32)) : -INFINITY;
        }
    }
}

bool lists_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace

extern "C" int madtp_lists_abi_version(void) { return MADTP_LISTS_ABI_VERSION; }

extern "C" int madtp_lists_rank(const int64_t* idx, int64_t ld_idx, const float* val, int64_t ld_val, int n, int k, int nk, float fill,
                                const int32_t* tgt_ptr, const int32_t* tgt_idx, int32_t* rank_row, int32_t* rank_tgt, void* stream) {
    if (!idx || !val || !tgt_ptr || !tgt_idx || !rank_row || !rank_tgt) return MADTP_E_BADARG;
    if (k < 1 || k > MADTP_LISTS_MAX_K) return MADTP_E_BADARG;
    if (n <= 0 || nk <= 0 || ld_idx < k || ld_val < k) return MADTP_E_SHAPE;
    constexpr int rows = LR_THREADS / 64;
    hipLaunchKernelGGL(lists_rank_kernel, dim3((n + rows - 1) / rows), dim3(LR_THREADS), 0, (hipStream_t)stream, idx, (size_t)ld_idx, val,
                       (size_t)ld_val, n, k, nk, fill, tgt_ptr, tgt_idx, rank_row, rank_tgt);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" int madtp_lists_sort(const int64_t* idx, int64_t ld_idx, const float* val, int64_t ld_val, int n, int k, int nk,
                                int64_t* out_idx, float* out_val, void* stream) {
    if (!idx || !val || !out_idx || !out_val) return MADTP_E_BADARG;
    if (k < 1 || k > MADTP_LISTS_MAX_K) return MADTP_E_BADARG;
    if (n <= 0 || nk <= 0 || ld_idx < k || ld_val < k) return MADTP_E_SHAPE;
    const size_t in_idx = sizeof(int64_t) * ((size_t)(n - 1) * (size_t)ld_idx + k), in_val = sizeof(float) * ((size_t)(n - 1) * (size_t)ld_val + k);
    const size_t o_idx = sizeof(int64_t) * (size_t)n * k, o_val = sizeof(float) * (size_t)n * k;
    if (lists_overlap(out_idx, o_idx, idx, in_idx) || lists_overlap(out_idx, o_idx, val, in_val) ||
        lists_overlap(out_val, o_val, idx, in_idx) || lists_overlap(out_val, o_val, val, in_val) ||
        lists_overlap(out_idx, o_idx, out_val, o_val))
        return MADTP_E_BADARG;
    const dim3 grid((n + LS_ROWS - 1) / LS_ROWS), block(RK_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (k <= 64) hipLaunchKernelGGL(lists_sort_kernel<64>, grid, block, 0, s, idx, (size_t)ld_idx, val, (size_t)ld_val, n, k, nk, out_idx, out_val);
    else if (k <= 128) hipLaunchKernelGGL(lists_sort_kernel<128>, grid, block, 0, s, idx, (size_t)ld_idx, val, (size_t)ld_val, n, k, nk, out_idx, out_val);
    else hipLaunchKernelGGL(lists_sort_kernel<256>, grid, block, 0, s, idx, (size_t)ld_idx, val, (size_t)ld_val, n, k, nk, out_idx, out_val);
    MADTP_LAUNCH_CHECK();
    return 0;
}

// The optimizer step of the training loops (compress_*_dtp.py / train_*.py: optimizer.step() of torch.optim.AdamW): every f32
// parameter of a step in one launch over a device pointer table - the scheme of madtp_ema_update (retrieval.hip).  No atomics and
// one workgroup per fixed slice of one tensor, so identical calls give identical bits.
#include "common.h"

namespace {

// table: int64 [6, n]: rows = p, g, m (exp_avg), v (exp_avg_sq) pointers, numel, first workgroup of the tensor (prefix sum)
constexpr int ADAMW_THREADS = 256;
constexpr int ADAMW_VECS = 4;  // float4 per thread and stream: 16 independent 16-byte loads (4 KiB per wave) before the first use
constexpr int ADAMW_PER_BLOCK = ADAMW_THREADS * 4 * ADAMW_VECS;

struct AdamwScalars { float decay, w1, beta2, w2, step_size, bc2_sqrt, eps; };

// torch/optim/adam.py _single_tensor_adam (decoupled_weight_decay), one rounding where the kernels torch runs for it round:
// p.mul_(decay); lerp_ (self + weight * diff, one FMA); exp_avg_sq.mul_(beta2), then addcmul_ (a + alpha * (b * c), one FMA);
// sqrt, / bc2_sqrt, add_(eps); addcdiv_ (a + alpha * (b / c), one FMA).  Explicit FMAs with contraction off, so the compiler fuses
// nothing else: exp_avg and exp_avg_sq come out bit for bit as torch's device kernels write them (measured on 4 M elements over
// five steps).  p does not always: aten divides by the HOST scalar bc2_sqrt as a product with the f32 value of its double
// reciprocal, this kernel divides by the f32 bc2_sqrt it is given (torch's CPU kernels do the same) - one rounding apart in a few
// per cent of the elements.  The division and the square root are the correctly rounded ones (hipcc's default).
__device__ __forceinline__ void adamw1(float& p, float g, float& m, float& v, const AdamwScalars& s) {
#pragma clang fp contract(off)
    const float p1 = p * s.decay;
    m = __builtin_fmaf(s.w1, g - m, m);
    const float vb = v * s.beta2;
    v = __builtin_fmaf(s.w2, g * g, vb);
    const float root = sqrtf(v) / s.bc2_sqrt;
    const float denom = root + s.eps;
    p = __builtin_fmaf(-s.step_size, m / denom, p1);
}

// (the table's pointers are device memory: global_load / global_store rather than the flat forms a plain pointer compiles to)
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

__device__ __forceinline__ void adamw4(f32x4& p, const f32x4& g, f32x4& m, f32x4& v, const AdamwScalars& s) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float pk = p[k], mk = m[k], vk = v[k];
        adamw1(pk, g[k], mk, vk, s);
        p[k] = pk; m[k] = mk; v[k] = vk;
    }
}

__device__ __forceinline__ void adamw_scalar(gfloat* p, const gfloat* g, gfloat* m, gfloat* v, int64_t i, const AdamwScalars& s) {
    float pk = p[i], mk = m[i], vk = v[i];
    adamw1(pk, g[i], mk, vk, s);
    p[i] = pk; m[i] = mk; v[i] = vk;
}

__global__ __launch_bounds__(ADAMW_THREADS) void adamw_kernel(const int64_t* table, int n, AdamwScalars s) {
    // the tensor this block belongs to: last t with first_block[t] <= blockIdx.x (a zero-element tensor owns no block)
    const int64_t* first = table + 5 * (size_t)n;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    gfloat* p = (gfloat*)table[lo];
    const gfloat* g = (const gfloat*)table[n + lo];
    gfloat* m = (gfloat*)table[2 * (size_t)n + lo];
    gfloat* v = (gfloat*)table[3 * (size_t)n + lo];
    const int64_t numel = table[4 * (size_t)n + lo];
    const int64_t base = ((int64_t)blockIdx.x - first[lo]) * ADAMW_PER_BLOCK;
    const int64_t end = min(numel, base + (int64_t)ADAMW_PER_BLOCK);
    if (base >= end) return;
    const bool aligned = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15u) == 0;  // (base % 4 == 0)
    if (aligned && end - base == ADAMW_PER_BLOCK) {
        // a whole slice (nearly every byte of a model): all 16 loads issued, without a branch between them, before the first use
        f32x4 vp[ADAMW_VECS], vg[ADAMW_VECS], vm[ADAMW_VECS], vv[ADAMW_VECS];
        const int64_t i0 = base + 4 * (int64_t)threadIdx.x;
#pragma unroll
        for (int c = 0; c < ADAMW_VECS; ++c) {
            const int64_t i = i0 + 4 * c * ADAMW_THREADS;
            vp[c] = *(const gf32x4*)(p + i);
            vg[c] = *(const gf32x4*)(g + i);
            vm[c] = *(const gf32x4*)(m + i);
            vv[c] = *(const gf32x4*)(v + i);
        }
#pragma unroll
        for (int c = 0; c < ADAMW_VECS; ++c) {
            const int64_t i = i0 + 4 * c * ADAMW_THREADS;
            adamw4(vp[c], vg[c], vm[c], vv[c], s);
            *(gf32x4*)(p + i) = vp[c];
            *(gf32x4*)(m + i) = vm[c];
            *(gf32x4*)(v + i) = vv[c];
        }
    } else if (aligned) {  // the last slice of a tensor: 16-byte pieces, then the numel % 4 tail element by element
        const int64_t vend = base + ((end - base) & ~(int64_t)3);
        for (int64_t i = base + 4 * (int64_t)threadIdx.x; i < vend; i += 4 * ADAMW_THREADS) {
            f32x4 a = *(const gf32x4*)(p + i), b = *(const gf32x4*)(g + i), c = *(const gf32x4*)(m + i), d = *(const gf32x4*)(v + i);
            adamw4(a, b, c, d, s);
            *(gf32x4*)(p + i) = a;
            *(gf32x4*)(m + i) = c;
            *(gf32x4*)(v + i) = d;
        }
        for (int64_t i = vend + threadIdx.x; i < end; i += ADAMW_THREADS) adamw_scalar(p, g, m, v, i, s);
    } else {  // a 4-byte aligned view: the same values element by element
        for (int64_t i = base + threadIdx.x; i < end; i += ADAMW_THREADS) adamw_scalar(p, g, m, v, i, s);
    }
}

}  // namespace

extern "C" int madtp_adamw_blocks(int64_t numel) {
    return numel <= 0 ? 0 : (int)((numel + ADAMW_PER_BLOCK - 1) / ADAMW_PER_BLOCK);
}

extern "C" int madtp_adamw_step(const int64_t* table, int n_tensors, int n_blocks, float decay, float w1, float beta2, float w2,
                                float step_size, float bc2_sqrt, float eps, void* stream) {
    if (!table || n_tensors < 1 || n_blocks < 0) return MADTP_E_BADARG;
    if (n_blocks == 0) return 0;
    const AdamwScalars s = {decay, w1, beta2, w2, step_size, bc2_sqrt, eps};
    hipLaunchKernelGGL(adamw_kernel, dim3(n_blocks), dim3(ADAMW_THREADS), 0, (hipStream_t)stream, table, n_tensors, s);
    MADTP_LAUNCH_CHECK();
    return 0;
}

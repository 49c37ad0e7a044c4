// The attention dispatch policy as a pure function: attn_plan(problem, switches, resources) -> which kernel instantiation, grid,
// block and LDS bytes a madtp_attention* / madtp_attention_pair launch gets.  Host-only and free of HIP (it compiles with a plain
// C++17 compiler): no getenv, no statics, no allocation - attention.hip gathers the inputs, calls it, fetches the resources the
// plan names and launches what it says; madtp_attention_plan (include/madtp_hip.h) returns the same plan without launching, which
// is how tests/test_attn_plan_cpu.py pins the policy down without a GPU.  The rules and their measurements: DESIGN.md section 5.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/madtp_hip.h"

namespace {

// ---- inputs ----------------------------------------------------------------------------------------------------------------
struct AttnProblem {
    int B, H, Nq, Nk, ldq, ldk, ldv, ldo;
    int io_dtype;       // MADTP_F32 / BF16 / F16S / F16
    bool pair;          // madtp_attention_pair: two problems of this shape
    bool ptrs;          // q, k, v and out present (both problems of a pair)
    bool scores;        // the score side outputs are requested (colsum_part), with
    bool p0, onorm;     // their companions present
    bool mask_qk;       // additive [Nq, Nk] mask, row stride
    int ld_mask_qk;
    bool add_mask;      // additive key mask [B, Nk]
    bool kv_index;      // K/V batch index
    int kv_block_rows;  // rows from one sample's K/V block to the next, 0 = dense
    bool n_dev;         // the token count is read on the device (sync-free encoder path), the host sizes are the worst case;
    bool dev_q_only;    // it counts the query tokens only
    int split_req;      // column offset of the second f16-split plane of the context, 0 = no planes
    // alignment of the pointers: q, k and v to 16 bytes; out to 16 and to 8 bytes; of a pair, the second problem's q, k and v to 16
    // bytes, and whether both problems have an additive mask or neither
    bool qkv_aligned, out_aligned16, out_aligned8, pair_aligned, pair_masks_alike;
};

// Process switches, with their defaults (attention.hip attn_switches() reads each from the environment variable of its name, once).
struct AttnSwitches {
    int head_split = 1;   // 0 = a launch with scores never splits its heads over workgroups
    int hv = 1;           // 0 = 641..1024 keys with scores keep the one-sweep order
    int head_groups = 0;  // 2..4 forces the head split of attn_bf16_large_kernel to that many groups (A/B runs)
    int f16s = 1;         // 0 = the f16x3 mode keeps its attention on the exact-f32 MFMA kernels (A/B runs)
    int large_f32 = 0;    // 1 = bf16 storage beyond 256 keys on the exact-f32 MFMA kernel (A/B runs)
    int pair = 1;         // 0 = a pair always runs as two launches (A/B runs)
};

// What the launcher can allocate.  It plans with both true, and again with the one false whose allocation failed.
struct AttnResources {
    bool hm = true;     // the head-max exchange area of the head split
    bool opart = true;  // the f32 scratch of the three-sweep order
};

// ---- result ----------------------------------------------------------------------------------------------------------------
enum {
    ATTN_KERNEL = 0,        // attn_kernel<T, NT, SCORES>: exact-f32 MFMA, <= 256 keys
    ATTN_F16S_KERNEL,       // attn_f16s_kernel<NT, SCORES>: f16x3, <= 256 keys
    ATTN_BF16_KERNEL,       // attn_bf16_kernel<NT, SCORES, HS, RB, F16>: bf16 / f16 MFMA, <= 256 keys
    ATTN_BF16_SMALL_KERNEL, // attn_bf16_small_kernel<F16>: <= 32 keys with scores, one sample per workgroup
    ATTN_LARGE_KERNEL,      // attn_large_kernel<T, NCH, SCORES>: exact-f32 MFMA, 257..1024 keys
    ATTN_LARGE_F16S_KERNEL, // attn_large_f16s_kernel<NCH, SCORES>: f16x3, 257..1024 keys
    ATTN_BF16_LARGE_KERNEL, // attn_bf16_large_kernel<NCH, SCORES, 2, F16, HV>: bf16 / f16 MFMA, 257..1024 keys
};
constexpr int ATTN_PAIR_TWO_LAUNCHES = 1000;  // status: this pair does not run as one launch (madtp_attention_pair then launches twice)

struct AttnPlan {
    int status;      // 0, a MADTP_E_* code or ATTN_PAIR_TWO_LAUNCHES; every other field is 0 (family -1) unless status == 0
    int family;      // ATTN_*_KERNEL
    int nt;          // the instantiation's key capacity: NT 16-key tiles (<= 256 keys) or NCH 128-key chunks (beyond); 0 for the small kernel
    int storage;     // element type T of attn_kernel / attn_large_kernel: 0 float, 1 bf16_t (0 for the other families)
    int scores;      // SCORES
    int f16;         // F16 of the bf16 families: operands are IEEE f16
    int hs, rb, hv;  // attn_bf16_kernel: head-parity split, 64-row blocks per workgroup; attn_bf16_large_kernel: 2 = three-sweep order (else 1)
    int gx, gy, gz, block;  // grid and workgroup size
    int lds;         // dynamic LDS bytes of the launch, and
    int lds_optin;   // the bytes the instantiation is opted in to (>= lds: the one-head-per-workgroup cross launch runs on half a ring)
    int need_hm, need_opart;  // the launch reads AttnArgs::hm_ws / hm_tick, AttnArgs::o_part
    int split_dim;   // AttnArgs::split_dim
};
static_assert(sizeof(AttnPlan) == MADTP_ATTN_PLAN_FIELDS * sizeof(int32_t), "madtp_attention_plan hands the plan out field by field, in this order");

// Exchange area of the head split: up to HM_MAX_WGS row blocks, HM_MAX_GZ head groups, 2 * HM_MAX_NT dwords per lane.
constexpr int HM_MAX_WGS = 384, HM_MAX_NT = 40, HM_MAX_GZ = 4;
constexpr int ATTN_SMALL_NW = 12;  // waves per workgroup of attn_bf16_small_kernel (attention.hip SMALL_NW)

inline AttnPlan attn_plan_refused(int status) {
    AttnPlan r{};
    r.status = status; r.family = -1;
    return r;
}

// ---- the rules, once each ---------------------------------------------------------------------------------------------------
// The smallest instantiated key capacity that holds n tiles / chunks (the last rung holds every n that reaches the ladder).
template <size_t N>
inline int attn_rung(const int (&ladder)[N], int n) {
    for (size_t i = 0; i + 1 < N; ++i)
        if (n <= ladder[i]) return ladder[i];
    return ladder[N - 1];
}
constexpr int kAttnNT[] = {2, 4, 6, 8, 10, 12, 13, 16};  // attn_kernel: 2 = the text encoder's 20-35 tokens, 6 = 81-96 keys of the pruned ViT layers
constexpr int kAttnF16sNT[] = {2, 4, 6, 8, 10, 13, 16};
constexpr int kAttnBf16NT[] = {4, 6, 8, 10, 12, 13, 16};
constexpr int kAttnLargeNCH[] = {5, 8};                  // attn_large_kernel, attn_large_f16s_kernel
constexpr int kAttnBf16LargeNCH[] = {3, 5, 8};

// attn_bf16_kernel with scores: the head-parity split where 4 rings fit the 160 KiB of LDS, else two 64-row blocks per workgroup
// (only one ring fits a CU).  The launcher names its instantiations by the same two functions.
constexpr int attn_bf16_hs(bool scores, int nt) { return (scores && nt <= 8) ? 2 : 1; }
constexpr int attn_bf16_rb(bool scores, int nt) { return (scores && nt > 8) ? 2 : 1; }

// Launches without scores (cross-attention: few query rows per sample) spread the heads over gridDim.z workgroups.
inline int attn_head_spread(int wgs, int H) {
    const int gz = wgs >= 512 ? 1 : (wgs >= 128 ? 4 : H);
    return gz > H ? H : gz;
}

// Launches with scores: a row block walks all heads (the head-max), so a launch that leaves most SIMDs with one wave or none runs
// 2..4 workgroups per row block, a share of the heads each, which merge their head-max through the exchange area.  hm_dwords: the
// dwords per lane a workgroup parks there (4 per key tile in f32, 2 per key tile as packed f16 pairs in attn_bf16_large_kernel).
inline bool attn_head_split_ok(const AttnSwitches& sw, const AttnResources& res, int hm_dwords, int wgs, int H) {
    return hm_dwords <= 2 * HM_MAX_NT && wgs <= HM_MAX_WGS && H % 2 == 0 && sw.head_split && res.hm;
}

// attn_bf16_large_kernel: the split that minimises rounds x heads per workgroup (512 workgroup slots at two per CU, 256 at one),
// e.g. 32 samples x 605 keys = 320 row blocks: 2 groups = 640 workgroups = 2 rounds x 6 heads, 3 groups = 960 = 2 rounds x 4 heads.
inline int attn_head_groups(const AttnSwitches& sw, int nch, int wgs, int H) {
    const int cap = 256 * (nch <= 5 ? 2 : 1);
    int best = 2, best_cost = 1 << 30;
    for (int z = 2; z <= HM_MAX_GZ; ++z) {
        if (H % z) continue;
        const int cost = ((wgs * z + cap - 1) / cap) * (H / z);
        if (cost < best_cost) { best_cost = cost; best = z; }
    }
    if (sw.head_groups >= 2 && sw.head_groups <= HM_MAX_GZ && H % sw.head_groups == 0) best = sw.head_groups;
    return best;
}

// ---- the policy ------------------------------------------------------------------------------------------------------------
inline AttnPlan attn_plan(const AttnProblem& p, const AttnSwitches& sw, const AttnResources& res) {
    const int B = p.B, H = p.H, Nq = p.Nq, Nk = p.Nk;
    const bool f16 = p.io_dtype == MADTP_F16;  // plain f16 operands: the bf16 kernels on the f16 MFMA
    const bool lp = p.io_dtype == MADTP_BF16 || f16;
    bool f16s = false;
    int split_dim = 0;
    if (p.pair) {
        // One launch when the two problems run on the bf16 kernel for <= 256 keys (no planes there), two launches otherwise.
        if (p.n_dev && (Nk > 256 || Nq > 256)) return attn_plan_refused(MADTP_E_SHAPE);
        if (!p.ptrs || B <= 0 || H <= 0 || Nq <= 0 || Nk <= 0) return attn_plan_refused(MADTP_E_BADARG);
        const bool one = sw.pair && lp && Nk <= 256 && p.pair_masks_alike && p.qkv_aligned && p.pair_aligned && (p.ldq * 2) % 16 == 0 &&
                         (p.ldk * 2) % 16 == 0 && (p.ldv * 2) % 16 == 0;
        if (!one) return attn_plan_refused(ATTN_PAIR_TWO_LAUNCHES);
        if (p.split_req) return attn_plan_refused(MADTP_E_BADARG);
    } else {
        if (!p.ptrs || B <= 0 || H <= 0 || Nq <= 0 || Nk <= 0) return attn_plan_refused(MADTP_E_BADARG);
        if (p.mask_qk && (p.ld_mask_qk < Nk || Nk > 256)) return attn_plan_refused(MADTP_E_SHAPE);  // the <= 256-key kernels carry the [Nq,Nk] mask
        const int split_req = p.split_req < 0 ? 0 : p.split_req;
        if (p.kv_block_rows && (p.kv_block_rows < Nk || Nk > 256 || p.scores)) return attn_plan_refused(MADTP_E_SHAPE);  // (the <= 256-key kernels without scores)
        if (p.kv_index && p.scores) return attn_plan_refused(MADTP_E_BADARG);  // indexed K/V is a cross-attention feature
        if (p.io_dtype != MADTP_F32 && p.io_dtype != MADTP_BF16 && p.io_dtype != MADTP_F16S && p.io_dtype != MADTP_F16) return attn_plan_refused(MADTP_E_DTYPE);
        // MADTP_F16S: f32 storage, products as three f16 MFMA products of f16-split operands (the f16x3 precision mode).  A request
        // for split planes cannot fall back to a kernel that writes f32, so it is an error unless the f16s kernels are on.
        if (p.io_dtype == MADTP_F16S) {
            f16s = sw.f16s != 0;
            split_dim = f16s ? split_req : 0;
            if (split_req && !f16s) return attn_plan_refused(MADTP_E_BADARG);
        } else if (split_req) {
            return attn_plan_refused(MADTP_E_BADARG);
        }
        if (p.scores && (!p.p0 || !p.onorm || Nq != Nk)) return attn_plan_refused(MADTP_E_BADARG);
        const int esz = lp ? 2 : 4;
        if (!p.qkv_aligned || (p.ldq * esz) % 16 || (p.ldk * esz) % 16 || (p.ldv * esz) % 16) return attn_plan_refused(MADTP_E_ALIGN);
        if (Nk > 1024) return attn_plan_refused(MADTP_E_SHAPE);
        if (split_dim && ((p.ldo % 4) || (split_dim % 4) || !p.out_aligned8)) return attn_plan_refused(MADTP_E_ALIGN);  // planes: 8-byte stores at f16 offsets
        if (!split_dim) f16s = f16s && (p.ldo * 4) % 16 == 0 && p.out_aligned16;  // (f32 context: 16-byte stores, else the exact-f32 kernel)
    }

    AttnPlan r{};
    r.scores = p.scores && !p.pair;
    r.f16 = f16;
    r.hs = r.rb = r.hv = 1;
    r.split_dim = split_dim;
    r.gx = (Nq + 63) / 64; r.gy = B; r.gz = 1; r.block = 256;
    const int wgs = r.gx * B;  // 64-row blocks of the launch (of one problem of a pair)
    const bool scores = r.scores != 0;
    const int nt = (Nk + 15) / 16, nch = (Nk + 127) / 128;
    const int pitch = 64 * (lp ? 2 : 4) + 16;  // K/V row pitch of the exact-f32 MFMA kernels
    bool hm_split = false;                     // the two-group head split of the <= 256-key kernels with scores
    if (Nk > 256) {  // long sequences (384^2 / 480^2 images): two-pass kernels, 128-key chunks
        if (f16s) {
            r.family = ATTN_LARGE_F16S_KERNEL;
            r.nt = attn_rung(kAttnLargeNCH, nch);
            r.lds = 4 * 128 * 160;
        } else if (lp && (f16 || !sw.large_f32)) {
            // fast mode: bf16 MFMA, two stages of K|V chunk images + the waves' Q rows.  The three-stage ring (STG = 3: two chunks in
            // flight behind counted vmcnt waits, 104 KiB, one workgroup per CU) was measured 4-8 % SLOWER at one workgroup per CU and
            // 40 % slower where two would fit (tools/attn_large_bench.py): a chunk step of a lone wave is bound by its own dependent
            // instruction stream (~1.85 us against ~1.2 us with two waves per SIMD), not by the DMA round trip.
            r.family = ATTN_BF16_LARGE_KERNEL;
            r.nt = attn_rung(kAttnBf16LargeNCH, nch);
            r.lds = 2 * 2 * 128 * 128 + 4 * 2048;
            if (scores && r.nt == 8 && sw.hv && H <= 16 && nch > r.nt / 2 && res.opart) {
                // 641..1024 keys with scores: the three-sweep order, two workgroups per CU; the row statistics of every head in LDS
                r.hv = 2;
                r.need_opart = 1;
                r.lds += H * 128 * (int)sizeof(float);
            } else if (scores && attn_head_split_ok(sw, res, 2 * r.nt * 8, wgs, H)) {
                r.gz = attn_head_groups(sw, r.nt, wgs, H);
                r.need_hm = 1;
            }
        } else {
            r.family = ATTN_LARGE_KERNEL;
            r.storage = lp;
            r.nt = attn_rung(kAttnLargeNCH, nch);
            r.lds = 2 * 128 * pitch;
        }
        if (!scores) r.gz = attn_head_spread(wgs, H);
    } else if (f16s) {
        r.family = ATTN_F16S_KERNEL;
        r.nt = attn_rung(kAttnF16sNT, nt);
        r.lds = (2 * r.nt * 16 + 2 * ((r.nt + 1) / 2) * 32) * (r.nt <= 15 ? 160 : 144);
        hm_split = true;
    } else if (!lp) {
        r.family = ATTN_KERNEL;
        r.nt = attn_rung(kAttnNT, nt);
        r.lds = 2 * r.nt * 16 * pitch;
        hm_split = true;
    } else if (scores && Nk <= 32 && !p.mask_qk && !p.n_dev) {  // short text sequences: one sample per workgroup, heads spread over the waves
        r.family = ATTN_BF16_SMALL_KERNEL;
        r.gx = B; r.gy = 1; r.block = 64 * ATTN_SMALL_NW;
    } else {
        r.family = ATTN_BF16_KERNEL;
        r.nt = attn_rung(kAttnBf16NT, nt);
        r.hs = attn_bf16_hs(scores, r.nt);
        r.rb = attn_bf16_rb(scores, r.nt);
        r.lds = 2 * r.hs * (r.nt * 16 + (r.nt + 1) / 2 * 32) * 128;
        r.lds_optin = r.lds;
        r.gx = (Nq + 64 * r.rb - 1) / (64 * r.rb);
        r.gy = p.pair ? 2 * B : B;
        r.block = 256 * r.hs * r.rb;
        if (!scores) {
            // below 512 workgroups every head gets its own workgroup - no head loop, so ONE ring stage is allocated and 2-6
            // workgroups share a CU (the two-stage ring of a 190-key problem is 98 KiB, one 4-wave workgroup per CU)
            r.gz = wgs >= 512 ? 1 : H;
            if (r.gz == H) r.lds /= 2;
        }
    }
    if (hm_split) {
        if (!scores) {
            r.gz = attn_head_spread(wgs, H);
        } else if (attn_head_split_ok(sw, res, 4 * r.nt, wgs, H)) {  // (128 images x 2 row blocks in the parity modes, 64 text samples)
            r.gz = 2;
            r.need_hm = 1;
        }
    }
    if (r.family != ATTN_BF16_KERNEL) r.lds_optin = r.lds;
    return r;
}

}  // namespace

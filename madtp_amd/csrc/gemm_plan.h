// The GEMM dispatch policy as a pure function: gemm_plan(problem, switches, stream attributes) -> which kernel, tile, grid and
// tile order a madtp_gemm / madtp_gemm_pair / madtp_gemm_splitk launch gets.  Host-only and free of HIP (it compiles with a
// plain C++17 compiler): no getenv, no statics, no atomics, no lock, no allocation - gemm.hip gathers the inputs, calls it and
// launches what it says; madtp_gemm_plan (include/madtp_hip.h) returns the same plan without launching, which is how the tests
// pin the policy down without a GPU.  The rules and their measurements: DESIGN.md section 5, profiles/r0*_gemm_*.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/madtp_hip.h"
#include "gemm_table.h"  // per-shape kernel choice of the big problems, measured (tools/gemm_autotune.py)

#if defined(__HIPCC__)
#define MADTP_PLAN_HD __host__ __device__ __forceinline__
#else
#define MADTP_PLAN_HD inline
#endif

namespace {

constexpr int GEMM_ROWB = 128;  // bytes per operand row slab (gemm_device.h ROWB)

// ---- inputs ----------------------------------------------------------------------------------------------------------------
struct GemmProblem {
    int M, N, K, lda, ldw, ldc, ldr;
    int ab_dtype, c_dtype;  // MADTP_F32 / BF16 / F16S / F16
    int splitk;             // K ranges of a madtp_gemm_splitk launch, else 1
    bool pair;              // madtp_gemm_pair: two problems of this shape in one launch
    bool bias, residual;    // epilogue operands present
    bool m_dev;             // M is an upper bound, the kernel reads the row count from device memory (sync-free encoder path)
    // 16-byte alignment of the pointers: A and W; C; bias / residual (true when absent); the second problem of a pair
    bool ab_aligned, c_aligned, bias_aligned, res_aligned, pair_aligned;
};

// Process switches (environment, read once by gemm.hip) plus the forced configuration of madtp_gemm_set_config.
struct GemmSwitches {
    int force_cfg = 0;        // MADTP_GEMM_CFG / madtp_gemm_set_config: 0 automatic, 1..4 a gemm_kernel variant, 5 / 7 wave-specialised
                              // with / without the stream-K tail, 6 lockstep 256x256, 9 / 10 ping-pong 256x256 / 192x256
    int desc = 1;             // MADTP_GEMM_DESC: 0 = gemm_kernel builds its LDS-DMA addresses per instruction (A/B runs)
    int big_min_m = 4096;     // MADTP_GEMM_BIG_MIN_M (>= 256) and
    int big_min_tiles = 200;  // MADTP_GEMM_BIG_MIN_TILES (>= 1): thresholds of the big-tile kernels
    int pair = 1;             // MADTP_GEMM_PAIR: 0 = a pair always runs as two launches
    int sq = 1;               // MADTP_GEMM_SQ: 0 = no 256-column tile in the automatic choice
    int pp = 1;               // MADTP_GEMM_PP: 0 = keep the lockstep 256x256 kernel
    int table = 1;            // MADTP_GEMM_TABLE: 0 = cost model only, 2 = the table also while a hint is in force
    int ngrp = -1;            // MADTP_GEMM_NGRP: column-group width of the tile order, -1 automatic, 0 off, n > 0 forced
    int sk = 0;               // MADTP_GEMM_SK: 1 = stream-K tail of the wave-specialised kernel on automatic launches
    int wg_per_xcd = 32;      // MADTP_GEMM_WG_PER_XCD: workgroups per XCD of the persistent kernels
    int small_cfg = -1;       // MADTP_GEMM_SMALL_CFG: process default of the small-tile hint, -1 = the automatic rule
    float sq_cost = 1.7f;     // MADTP_GEMM_SQ_COST: process default of the 256x256 tile's per-round cost
    bool sk_workspace = true; // the stream-K workspace can be had (gemm.hip plans again with false when its allocation fails)
};

// Per-stream scheduling attributes (madtp_stream_set_sched): the CUs per XCD the stream owns and its two dispatch hints
// (sq_cost <= 0 / small_tile -2 = the process default).
struct StreamSched { int cus_per_xcd; float sq_cost; int small_tile; };

// ---- result ----------------------------------------------------------------------------------------------------------------
enum { GEMM_KERNEL = 0, GEMM_WS_KERNEL = 1, GEMM_SQ_KERNEL = 2, GEMM_PP_KERNEL = 3 };
constexpr int GEMM_PAIR_UNSUPPORTED = 1000;  // status: this pair does not run as one launch (madtp_gemm_pair then launches twice)

struct GemmPlan {
    int status;      // 0, a MADTP_E_* code or GEMM_PAIR_UNSUPPORTED; every other field is 0 (kernel -1) unless status == 0
    int kernel;      // GEMM_KERNEL / GEMM_WS_KERNEL / GEMM_SQ_KERNEL / GEMM_PP_KERNEL
    int variant;     // gemm_kernel: 0 128x128 2 stages, 1 64x128 2 stages, 2 64x128 3 stages, 3 64x64 3 stages
    int rows, cols;  // tile
    int ntm, ntn, ngrp, grid, lds;  // row / column tiles, column-group width of the tile order (0 = row-panel major), workgroups, LDS bytes
    int sk;          // stream-K tail of the wave-specialised kernel
    int desc, fast_epi;  // GemmArgs::desc / fast_epi
    int om;          // output mode of the epilogue: 0 f32, 1 bf16, 2 f16-split, 3 f16 (gemm_device.h OM_*)
    int mode;        // operand format: 0 bf16, 1 f16, 2 f16-split, 3 f32
};
static_assert(sizeof(GemmPlan) == MADTP_PLAN_FIELDS * sizeof(int32_t), "madtp_gemm_plan hands the plan out field by field, in this order");

// ---- helpers ---------------------------------------------------------------------------------------------------------------
// Stream-K tail of a persistent kernel (the wave-specialised 256x128 one): an XCD's `nslots` tiles are `rounds` full rounds of
// its `gl` workgroups plus `rem` tiles.  With rem <= gl/2 the last round would leave most CUs idle for a whole tile time (the
// N = 768 GEMMs of the ViT layers at 11-14 k rows are 1.03-1.3 rounds), so each of the rem tiles is cut along K into `parts`
// pieces run by `parts` workgroups; every consumer wave parks its 64x64 partial in the workspace and the LAST wave to arrive
// (ticket per tile and wave position) sums the pieces in piece order - deterministic - and runs the epilogue.
constexpr int SK_MAX_PARTS = 8;
MADTP_PLAN_HD int sk_parts(int rem, int gl, int nk) {
    if (rem <= 0) return 0;
    int p = gl / rem;
    if (p > SK_MAX_PARTS) p = SK_MAX_PARTS;
    if (p > nk / 2) p = nk / 2;  // at least two slabs per piece
    return p >= 2 ? p : 0;
}

// Cost (in rounds of 256x128 tiles) of the wave-specialised kernel on t256 tiles.  The stream-K tail pays for K >= 2048 only
// (measured, tools/gemm_bench.py ab / profiles/r02_gemm_sk_ab.txt): parking and re-reading the partials costs ~16 us per
// launch, while the few tiles of a plain last round run ~25 % faster than in a full round (no contention), so with K = 768
// (12 slabs, ~13 us per lone tile) the split loses 4-10 us and with K = 3072 it wins 6-14 us (M = 11-14 k rows, N = 768).
constexpr int SK_MIN_SLABS = 32;
inline float ws_cost(int t256, int nk, bool sk, int cpx) {
    const int nsl = (t256 + 7) / 8, rounds = nsl / cpx, rem = nsl - rounds * cpx;
    if (rem == 0) return (float)rounds;
    const int parts = (sk && cpx == 32 && nk >= SK_MIN_SLABS) ? sk_parts(rem, 32, nk) : 0;
    return (float)rounds + (parts ? 0.65f : 1.0f);
}

// Workgroups per XCD of a persistent big-GEMM launch (default 32 = one workgroup per CU walking its share of the tiles): the
// process setting scaled to the CUs the stream owns.  A larger cap gives every workgroup fewer tiles (>= tiles / 8: one tile
// each) - the launch then frees CUs tile by tile, which lets the small kernels of ANOTHER stream in between
// (madtp_amd/pipeline.py) at the price of the cross-tile pipelining.
inline int gemm_wg_per_xcd(const GemmSwitches& sw, const StreamSched& ss) {
    int v = sw.wg_per_xcd < 1 ? 32 : sw.wg_per_xcd;
    if (ss.cus_per_xcd < 32) { v = v * ss.cus_per_xcd / 32; if (v < 1) v = 1; }
    return v;
}
// Grid of a launch whose workgroups walk tile slots XCD by XCD: `slots` per XCD, at most `cap` workgroups per XCD.
inline int gemm_grid(int slots, int cap) { return 8 * (slots < cap ? slots : cap); }

// the four gemm_kernel variants (GemmPlan::variant)
struct GemmSmallTile { int bm, bn, stages, wg_per_cu; };
constexpr GemmSmallTile kGemmSmallTiles[4] = {{128, 128, 2, 2}, {64, 128, 2, 3}, {64, 128, 3, 2}, {64, 64, 3, 3}};

inline GemmPlan gemm_plan_refused(int status) {
    GemmPlan r{};
    r.status = status; r.kernel = -1;
    return r;
}

// ---- the policy ------------------------------------------------------------------------------------------------------------
inline GemmPlan gemm_plan(const GemmProblem& p, const GemmSwitches& sw, const StreamSched& ss) {
    const int M = p.M, N = p.N, K = p.K, ab_dtype = p.ab_dtype, c_dtype = p.c_dtype, splitk = p.splitk, force_cfg = sw.force_cfg;
    if (M <= 0 || N <= 0 || K <= 0) return gemm_plan_refused(MADTP_E_BADARG);
    if (ab_dtype != MADTP_F32 && ab_dtype != MADTP_BF16 && ab_dtype != MADTP_F16S && ab_dtype != MADTP_F16) return gemm_plan_refused(MADTP_E_DTYPE);
    if (c_dtype != MADTP_F32 && c_dtype != MADTP_BF16 && c_dtype != MADTP_F16S && c_dtype != MADTP_F16) return gemm_plan_refused(MADTP_E_DTYPE);
    const bool x3 = ab_dtype == MADTP_F16S;
    const bool f16 = ab_dtype == MADTP_F16;  // plain f16 operands: the bf16 kernels' instantiations on the f16 MFMA
    if (c_dtype == MADTP_F16S && !x3) return gemm_plan_refused(MADTP_E_DTYPE);  // the split epilogue exists on the f16-split kernels only
    if (c_dtype == MADTP_BF16 && (x3 || f16)) return gemm_plan_refused(MADTP_E_DTYPE);  // a 2-byte output of 2-byte operands has their element format
    if (c_dtype == MADTP_F16 && !f16) return gemm_plan_refused(MADTP_E_DTYPE);
    const int esz = ab_dtype == MADTP_F32 ? 4 : 2;
    if ((K * esz) % GEMM_ROWB != 0) return gemm_plan_refused(MADTP_E_SHAPE);
    if (!p.ab_aligned || (p.lda * esz) % 16 || (p.ldw * esz) % 16) return gemm_plan_refused(MADTP_E_ALIGN);
    // f16-split operands: leading dimensions count f16 elements (2 planes of K per activation row and per weight row)
    if (p.lda < (x3 ? 2 : 1) * K || p.ldw < (x3 ? 2 : 1) * K || p.ldc < (c_dtype == MADTP_F16S ? 2 : 1) * N || (p.residual && p.ldr < N))
        return gemm_plan_refused(MADTP_E_SHAPE);
    if (p.m_dev && (M >= 4096 || p.pair || splitk != 1)) return gemm_plan_refused(MADTP_E_SHAPE);  // device-side M: the small-tile kernels only

    GemmPlan r{};
    r.om = c_dtype == MADTP_F32 ? 0 : (c_dtype == MADTP_BF16 ? 1 : (c_dtype == MADTP_F16S ? 2 : 3));
    r.mode = x3 ? 2 : (f16 ? 1 : (ab_dtype == MADTP_BF16 ? 0 : 3));
    {
        const size_t a_bytes = ((size_t)M + 127) * (size_t)p.lda * esz, w_bytes = ((size_t)N + 255) * (size_t)p.ldw * esz;
        r.desc = sw.desc && a_bytes < ((size_t)1 << 31) && w_bytes < ((size_t)1 << 31);
    }
    // vector epilogue needs 16-byte aligned rows on every epilogue operand
    // (and, for the descriptor-bounded stores, a 256-row block of C below 2 GiB; bf16 output with an f32 residual has no
    // caller on the path and takes the scalar epilogue; so does an f16-split output with a residual, but gemm_launch sees to
    // that one: this rule is pinned as recorded, tests/test_gemm_plan_cpu.py)
    r.fast_epi = (N % 8 == 0) && (p.ldc % 8 == 0) && p.c_aligned && (!p.bias || p.bias_aligned) &&
                 (!p.residual || (p.res_aligned && p.ldr % 4 == 0 && c_dtype != MADTP_BF16 && c_dtype != MADTP_F16)) &&
                 (size_t)p.ldc * 256 * 4 < ((size_t)1 << 31);
    // tile configuration of gemm_kernel (MADTP_GEMM_CFG=1..4 forces one of them for A/B measurements):
    //   0: 128x128, 2-stage ring, 2 workgroups/CU  - default, and the f32 path
    //   1: 64x128, 2 stages, 3 WG/CU   2: 64x128, 3 stages, 2 WG/CU   3: 64x64, 3 stages, 3 WG/CU
    // Small bf16 problems (the 1280-row GEMMs of the text encoder) are bound by the LDS-DMA rate of a CU (~40 GB/s with one
    // resident workgroup): what counts is spreading the operand bytes over ALL CUs in one round, so they take the
    // smallest tile whose grid still fits one round of 3 workgroups per CU (measured: 64x64 beats 128x128 by 20-45 % on
    // M=1280, N<=2304; 64x128 wins for N=3072).
    // The wave-specialised 256x128 kernel takes a problem once its tiles fill most of the chip (>= 200 of 256 CUs) - e.g. not
    // the 4480 x 768 GEMMs of a 128-pair re-ranking batch (108 tiles), which run better on 420 64x128 tiles.
    int cfg = 0;
    const int cpx = ss.cus_per_xcd, ncu = 8 * cpx;  // the CUs this stream owns (32 per XCD unless the caller said otherwise)
    const int t256 = ((M + 255) / 256) * ((N + 127) / 128);
    // Thresholds of the big-tile kernels (persistent 256-row tiles): M >= 4096 and most of the chip covered - what a lone launch
    // wants (latency).  MADTP_GEMM_BIG_MIN_M / _TILES lower them (experiments with several forwards in flight, where a launch's
    // CU time counts and a 1280-row problem on 45 efficient tiles costs a third of the CU time of 720 small ones).
    const int big_min_m = sw.big_min_m;
    const int big_min_tiles = cpx == 32 ? sw.big_min_tiles : (sw.big_min_tiles * ncu + 255) / 256;  // "most of the chip" = most of the stream's CUs
    const bool big = !p.m_dev && M >= big_min_m && t256 >= big_min_tiles;
    const bool lp16 = ab_dtype != MADTP_F32;  // 2-byte operand planes: bf16, f16, or f16-split (three times the slab stream)
    if (lp16 && !big) {
        const int t64 = ((M + 63) / 64) * ((N + 63) / 64) * splitk, t64x128 = ((M + 63) / 64) * ((N + 127) / 128) * splitk;
        if (t64 <= 3 * ncu) cfg = 3;
        else if (t64x128 <= 3 * ncu) cfg = 1;
    }
    const int auto_cfg = cfg;  // the kernel choice below follows the AUTOMATIC tile rule; the hint only picks among the small tiles
    if (lp16 && !big) {
        const int small = ss.small_tile > -2 ? ss.small_tile : sw.small_cfg;  // scheduling hint (per stream, else the process default), -1 = the rule above
        if (small >= 0 && small <= 3) cfg = small;
    }
    // MADTP_GEMM_CFG=5 forces the wave-specialised kernel, 1..4 force a gemm_kernel variant (A/B measurements)
    bool ws_ok = lp16 && splitk == 1 &&
                 (force_cfg == 5 || force_cfg == 7 || (force_cfg == 0 && !p.m_dev && M >= big_min_m && (big || (auto_cfg == 0 && M >= 4096))));
    if (p.pair) {
        ws_ok = sw.pair && lp16 && force_cfg == 0 && M >= big_min_m && 2 * t256 >= big_min_tiles && r.fast_epi && p.pair_aligned;
        if (!ws_ok) return gemm_plan_refused(GEMM_PAIR_UNSUPPORTED);
    }
    if (force_cfg > 0 && force_cfg <= 4) cfg = force_cfg - 1;
    // (round 5, measured and dropped: "deep ring" variants of the small tiles - 64x64 x 6 stages / 64x128 x 5, one workgroup per CU,
    //  five / four slabs in flight - are no faster on the text encoder's 1280-row problems (768x768: 11.7 vs 11.8 us, and 24 vs 13.5 us
    //  where the tiles need three rounds): their ~10 us are launch ramp, first-touch latency and drain, not the K loop)
    if (x3 && cfg == 0) cfg = 1;  // f16-split: 64x128 tiles (the 128x128 variant would spill the kept P0 fragments)

    // 256x256 kernel: 2-byte operands, no split-K / pair.  Chosen when its round count times its per-tile cost (measured ~1.7x a
    // 256x128 tile) beats the wave-specialised kernel's; MADTP_GEMM_CFG=6 forces it, MADTP_GEMM_SQ=0 turns it off (A/B runs).
    bool sq_ok = false, pp_ok = false;
    int pp_rows = 256;  // tile height of the ping-pong kernel: 256, or 192 (gemm_pp.hip FA = 3)
    // stream-K tail: off by default, configuration 5 always uses it (gemm.hip sk_workspace has the measurements)
    const bool sk_on = ws_ok && !x3 && ab_dtype == MADTP_BF16 && (force_cfg == 5 || (force_cfg == 0 && sw.sk != 0 && K / 64 >= SK_MIN_SLABS)) &&
                       sw.sk_workspace;
    if (lp16 && splitk == 1 && !p.pair && (K % 64) == 0 &&
        ((size_t)M + 255) * (size_t)p.lda * 2 < ((size_t)1 << 32) && ((size_t)N + 255) * (size_t)p.ldw * 2 < ((size_t)1 << 32)) {
        const int t_sq = ((M + 255) / 256) * ((N + 255) / 256), t_192 = ((M + 191) / 192) * ((N + 255) / 256);
        // the ping-pong main loop (gemm_pp_kernel, gemm_pp.hip) needs an even slab count; MADTP_GEMM_PP=0 keeps the lockstep kernel
        // (A/B runs), cfg 9 forces its 256-row tile, cfg 10 its 192-row tile, cfg 6 forces the lockstep kernel.  Its tile costs
        // ~1.5 tiles of 256x128 (lockstep: 1.7) - profiles/r04_gemm_pp_ab.txt; a caller's sq_cost hint (several forwards in flight)
        // applies to both.  Plain f16 and f16-split operands: the 256-column tile exists as the ping-pong kernel only.
        const bool pp_can = (K % 128) == 0;
        pp_ok = pp_can && (force_cfg == 9 || force_cfg == 10 || (force_cfg == 0 && sw.pp));
        const bool sq_allowed = sw.sq && ((!f16 && !x3) || pp_ok);
        // Per-round cost of a 256x256 tile relative to a 256x128 tile.  1.7 is what an isolated launch measures (the rule then
        // counts rounds).  With several forwards in flight on one GPU the tail of a sparse last round is filled by the other
        // streams' kernels, so the round count matters less than the per-flop efficiency of the tile (the 256x256 tile reads half
        // the LDS bytes per MFMA): madtp_amd/pipeline.py lowers the cost to 0.9 on its workers' streams - measured NLVR
        // 25.2 -> 25.7 k images/s with four in flight, but 20.1 -> 19.2 k on the serial loop, which keeps 1.7.
        float unit = ss.sq_cost > 0.f ? ss.sq_cost : sw.sq_cost;
        if (pp_ok && unit > 1.5f) unit = 1.5f;
        const bool hinted = ss.sq_cost > 0.f || cpx != 32;  // (the table was measured on the whole idle chip; a process default is no hint)
        // Choice for an automatic launch: (1) the measured table (gemm_table.h: per (operand class, N, K, output) and 64-row bucket
        // of M the fastest of {wave-specialised 256x128, ping-pong 256x256, ping-pong 192x256} on an idle MI355X; MADTP_GEMM_TABLE=0
        // turns it off; it steps aside while a caller's in-flight hint is in force), else (2) the round-count cost model.
        int choice = -1;  // 0 wave-specialised, 1 ping-pong / lockstep 256x256, 2 ping-pong 192x256
        if (force_cfg == 6 && !f16 && !x3) choice = 1;
        else if (force_cfg == 9 && pp_can) choice = 1;
        else if (force_cfg == 10 && pp_can) choice = 2;
        else if (force_cfg == 0 && sq_allowed && ws_ok) {
            if (pp_ok && sw.table && cpx == 32 && (sw.table == 2 || !hinted))
                choice = gemm_table_lookup(x3, M, N, K, c_dtype == MADTP_F32);
            if (choice < 0) {
                const float cost_ws = ws_cost(t256, K / 64, sk_on, cpx);
                const float cost_sq = 2 * t_sq >= big_min_tiles ? unit * (float)((t_sq + ncu - 1) / ncu) : 1e9f;
                // a 192-row tile: 3/4 of the MFMAs of a 256-row one behind the same barriers and 7/8 of its DMA stream (measured ~0.8)
                const float cost_192 = (pp_ok && 2 * t_192 >= big_min_tiles) ? 0.8f * unit * (float)((t_192 + ncu - 1) / ncu) : 1e9f;
                choice = (cost_192 < cost_sq && cost_192 < cost_ws) ? 2 : (cost_sq < cost_ws ? 1 : 0);
            }
        }
        sq_ok = choice >= 1;
        pp_ok = pp_ok && sq_ok;
        if (choice == 2) pp_rows = 192;
        if (sq_ok && !pp_ok && (f16 || x3)) sq_ok = false;  // (no lockstep instantiation for these operand formats)
    }
    const int cap = gemm_wg_per_xcd(sw, ss);
    if (sq_ok) {
        r.kernel = pp_ok ? GEMM_PP_KERNEL : GEMM_SQ_KERNEL;
        r.rows = pp_rows; r.cols = 256;
        r.ntm = (M + pp_rows - 1) / pp_rows;
        r.ntn = (N + 255) / 256;
        // MADTP_GEMM_NGRP: column-group width of the tile order (0 = row-panel major; unset = row-panel major up to 15 column
        // tiles - every shape of the forward - and groups of 8 beyond: with 32 column tiles (8192^3) an XCD's 32 concurrent
        // tiles then share 4 A panels and 8 W panels instead of 1 + 32: 1.32 -> 1.53-1.55 PF, profiles/r04_gemm_pp_ab.txt)
        const int grp = sw.ngrp >= 0 ? sw.ngrp : (r.ntn >= 16 ? 8 : 0);
        r.ngrp = (grp > 0 && grp < r.ntn) ? grp : 0;
        r.grid = gemm_grid((r.ntm * r.ntn + 7) / 8, cap);
        r.lds = 2 * (256 + 256) * GEMM_ROWB;
    } else if (ws_ok) {
        // wave-specialised 256x128 kernel (one 12-wave workgroup per CU, 144 KiB LDS ring)
        r.kernel = GEMM_WS_KERNEL;
        r.rows = 256; r.cols = 128;
        r.ntm = (M + 255) / 256;
        r.ntn = (N + 127) / 128;
        // column groups (tile_mn): keep one group's W rows (~2.4 MB) L2-resident when W as a whole is far larger than L2
        int G = sw.ngrp > 0 ? sw.ngrp : (12 * 768) / K;
        if (G < 1) G = 1;
        const bool on = sw.ngrp > 0 || (sw.ngrp == -1 && r.ntn >= 4 * G);
        r.ngrp = (on && G < r.ntn) ? G : 0;
        r.grid = gemm_grid((r.ntm * r.ntn * (p.pair ? 2 : 1) + 7) / 8, cap);
        r.sk = sk_on && r.grid == 256;
        r.lds = 3 * (256 + 128) * GEMM_ROWB;
    } else {
        const GemmSmallTile& t = kGemmSmallTiles[cfg];
        r.kernel = GEMM_KERNEL;
        r.variant = cfg;
        r.rows = t.bm; r.cols = t.bn;
        r.ntm = (M + t.bm - 1) / t.bm;
        r.ntn = (N + t.bn - 1) / t.bn;
        r.grid = gemm_grid(((r.ntm * r.ntn + 7) / 8) * splitk, cpx * t.wg_per_cu);
        r.lds = (t.bm + t.bn) * GEMM_ROWB * t.stages;
    }
    return r;
}

}  // namespace

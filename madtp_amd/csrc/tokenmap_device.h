// Token maps as both sides run them (csrc/madtp_tokenmap.h): the lane routines of the five kernels of tokenmap.hip.  They are
// __host__ __device__ text: a kernel runs them with one thread per lane, madtp_tokenmap_*_host (and tools/tokenmap_host_check.cpp
// under the host compiler's sanitizers) with the lanes of a workgroup, and the workgroups, in `for` loops.
//
// How the 256 lanes of a workgroup work together:
//   - control is UNIFORM: the layer loop, the pass loop of the sort and every early return depend only on launch arguments, table
//     rows and LDS words read behind a barrier, so every lane takes the same branches and reaches the same barriers;
//   - what lanes do side by side is an each_lane() body: the kernel runs it once with its own lane number, the host for lane
//     0 .. 255 in turn.  A body keeps nothing from one each_lane() to the next except in LDS or in the outputs;
//   - sync_lanes() (a barrier on the device, nothing on the host) stands between a write to LDS and a read of it by another lane.
//     What a lane reads back from GLOBAL memory (the previous layer's row of the map, depth) it wrote itself: program order of one
//     thread, no fence needed.
// No allocation, no mutable static, no atomics.  Two lanes write one LDS word only where the outcome does not depend on the winner:
// the flags (both store 1) and the position table under a repeat (the read-back finds the loser, whoever it is).
#pragma once
#include <stdint.h>

#include "madtp_tokenmap.h"

#if defined(__HIPCC__)
#define TM_HD __host__ __device__ inline
#else
#define TM_HD inline
#endif

namespace madtp_tokenmap {

constexpr int kLanes = MADTP_TOKENMAP_LANES, kMaxN = MADTP_TOKENMAP_MAX_N, kMaxL = MADTP_TOKENMAP_MAX_LAYERS, kFields = MADTP_TOKENMAP_FIELDS;
constexpr int kWaves = kLanes / 64;
constexpr int kPBits = 12;  // a sort key is slot << 12 | position
static_assert(kLanes == 256 && kWaves == 4, "the pruned sum restates madtp_token_select's: 256 partial sums, four wave sums");
static_assert(kMaxN == 1 << kPBits && kLanes * 16 == kMaxN, "a position fits the low bits of a key; 16 digits x 256 lanes of counts fill hist");
static_assert(kMaxL < 1 << MADTP_TOKENMAP_STATUS_LAYER_BITS, "a layer fits the status word");

template <class F>
TM_HD void each_lane(F body) {
#if defined(__HIP_DEVICE_COMPILE__)
    body((int)threadIdx.x);
#else
    for (int lane = 0; lane < kLanes; ++lane) body(lane);
#endif
}

TM_HD void sync_lanes() {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

TM_HD bool first_lane() {
#if defined(__HIP_DEVICE_COMPILE__)
    return threadIdx.x == 0;
#else
    return true;
#endif
}

inline const char* strerror_tokenmap(int code) {
    switch (code) {
        case MADTP_TOKENMAP_E_RANGE: return "a record's index is outside [0, n_in)";
        case MADTP_TOKENMAP_E_REPEAT: return "a record's index occurs twice";
        case MADTP_TOKENMAP_E_K: return "a record's k is outside 1 .. n_in - 1";
        case MADTP_TOKENMAP_E_CHAIN: return "a record's n_in is not what the layer before left";
        case MADTP_TOKENMAP_E_TABLE: return "a null pointer or a short row stride in the row of a pruned layer";
    }
    return nullptr;
}

TM_HD int32_t status_word(int code, int layer) { return -(int32_t)(((uint32_t)(-code) << MADTP_TOKENMAP_STATUS_LAYER_BITS) | (uint32_t)layer); }

// ---- build -----------------------------------------------------------------------------------------------------------------------------
struct BuildShared {
    int32_t inv[kMaxN];  // input position of the layer -> its place in indices[:k] + indices_sort[k:n_in]
    float part[kLanes];
    int32_t flag[2];     // a range error, a repeat
};

// The layers of sample b: kWrite == false checks every record and writes nothing, kWrite == true composes (the same checks stand
// in front of every access again).  -> 0 or the status word of the first broken rule; uniform.
template <bool kWrite>
TM_HD int32_t walk(BuildShared& sh, const int64_t* table, int L, int n0, int b, int32_t* slot, float* coef, int32_t* depth) {
    if (kWrite) {
        each_lane([&](int lane) {
            for (int p = lane; p < n0; p += kLanes) depth[p] = 0;
        });
    }
    int n = n0;
    for (int l = 0; l < L; ++l) {
        const int64_t* t = table + (size_t)l * kFields;
        const int64_t n_in = t[MADTP_TOKENMAP_F_N_IN], k64 = t[MADTP_TOKENMAP_F_K];
        if (n_in != n) return status_word(MADTP_TOKENMAP_E_CHAIN, l);
        int32_t* slot_l = slot + (size_t)l * n0;
        float* coef_l = coef + (size_t)l * n0;
        if (k64 == -1) {
            if (kWrite) {
                each_lane([&](int lane) {
                    for (int p = lane; p < n0; p += kLanes) {
                        slot_l[p] = l ? slot_l[p - n0] : p;
                        coef_l[p] = l ? coef_l[p - n0] : 1.0f;
                        if (depth[p] == l) depth[p] = l + 1;
                    }
                });
            }
            continue;
        }
        if (k64 < 1 || k64 >= n) return status_word(MADTP_TOKENMAP_E_K, l);
        const int k = (int)k64;
        const int64_t si = t[MADTP_TOKENMAP_F_INDICES_STRIDE], ss = t[MADTP_TOKENMAP_F_SORT_STRIDE], sc = t[MADTP_TOKENMAP_F_SCORE_STRIDE];
        if (!t[MADTP_TOKENMAP_F_INDICES] || !t[MADTP_TOKENMAP_F_SORT] || !t[MADTP_TOKENMAP_F_SCORE] || si < k || ss < n || sc < n)
            return status_word(MADTP_TOKENMAP_E_TABLE, l);
        const int64_t* ind = (const int64_t*)(uintptr_t)t[MADTP_TOKENMAP_F_INDICES] + (size_t)b * si;
        const int64_t* srt = (const int64_t*)(uintptr_t)t[MADTP_TOKENMAP_F_SORT] + (size_t)b * ss;
        const float* scr = (const float*)(uintptr_t)t[MADTP_TOKENMAP_F_SCORE] + (size_t)b * sc;
        sync_lanes();  // (nobody still reads the table or the flags of the layer before)
        each_lane([&](int lane) {
            for (int i = lane; i < n; i += kLanes) sh.inv[i] = -1;
            if (lane < 2) sh.flag[lane] = 0;
        });
        sync_lanes();
        each_lane([&](int lane) {
            for (int i = lane; i < n; i += kLanes) {
                const int64_t idx = i < k ? ind[i] : srt[i];
                if (idx < 0 || idx >= n) sh.flag[0] = 1;
                else sh.inv[idx] = i;
            }
        });
        sync_lanes();
        each_lane([&](int lane) {
            for (int i = lane; i < n; i += kLanes) {
                const int64_t idx = i < k ? ind[i] : srt[i];
                if (idx >= 0 && idx < n && sh.inv[idx] != i) sh.flag[1] = 1;
            }
        });
        sync_lanes();
        if (sh.flag[0]) return status_word(MADTP_TOKENMAP_E_RANGE, l);
        if (sh.flag[1]) return status_word(MADTP_TOKENMAP_E_REPEAT, l);
        // n places, every index in range, none twice: a permutation, every inv[] is set
        if (kWrite) {
            each_lane([&](int lane) {
                float a = 0.f;
                for (int pos = lane; pos < n; pos += kLanes)
                    if (sh.inv[pos] >= k) a += scr[pos];
                sh.part[lane] = a;
            });
            sync_lanes();
            for (int o = 32; o > 0; o >>= 1) {  // lane 0 of each wave of the butterfly: (v[i] + v[i + 32]) + ..., xor 32 first
                each_lane([&](int lane) {
                    if ((lane & 63) < o) sh.part[lane] = sh.part[lane] + sh.part[lane + o];
                });
                sync_lanes();
            }
            float dsum = 0.f;
            for (int w = 0; w < kWaves; ++w) dsum += sh.part[64 * w];
            const float den = dsum + 1e-8f;
            each_lane([&](int lane) {
                for (int p = lane; p < n0; p += kLanes) {
                    const int s_old = l ? slot_l[p - n0] : p;  // < n: what the layer before wrote
                    const float c_old = l ? coef_l[p - n0] : 1.0f;
                    const int i = sh.inv[s_old];
                    if (i < k) {
                        slot_l[p] = i;
                        coef_l[p] = c_old;
                        if (depth[p] == l) depth[p] = l + 1;
                    } else {
                        slot_l[p] = k;
                        coef_l[p] = c_old * (scr[s_old] / den);
                    }
                }
            });
        }
        n = k + 1;
    }
    return 0;
}

TM_HD void build_sample(BuildShared& sh, const int64_t* table, int L, int n0, int b, int32_t* slot, float* coef, int32_t* depth,
                        int32_t* status) {
    int32_t* slot_b = slot + (size_t)b * L * n0;
    float* coef_b = coef + (size_t)b * L * n0;
    int32_t* depth_b = depth + (size_t)b * n0;
    int32_t w = walk<false>(sh, table, L, n0, b, slot_b, coef_b, depth_b);
    sync_lanes();
    if (w == 0) w = walk<true>(sh, table, L, n0, b, slot_b, coef_b, depth_b);
    if (first_lane()) status[b] = w;
}

// ---- push ------------------------------------------------------------------------------------------------------------------------------
struct alignas(16) F4 {
    float v[4];
};
template <int V> struct Vec;
template <> struct Vec<1> { typedef float type; };
template <> struct Vec<4> { typedef F4 type; };

struct PushShared {
    uint32_t key[2][kMaxN];  // the (slot, position) pairs, ping and pong; behind the sort the free one holds each slot's first place
    int32_t hist[kMaxN];     // [digit][lane] counts, then offsets; behind the sort each slot's end
    int32_t tot[kLanes];
};

TM_HD int bits_of(int v) {
    int n = 0;
    while (v > 0) ++n, v >>= 1;
    return n;
}

// sample b's pairs sorted by slot, positions ascending inside a slot -> the buffer of sh.key that holds them (0 / 1); the other one
// holds start[], sh.hist holds end[].  A slot outside [0, n_out) sorts as n_out, behind every unit.
TM_HD int sort_slots(PushShared& sh, const int32_t* slot_b, int n0, int n_out) {
    const int m = (n0 + kLanes - 1) / kLanes;  // a lane owns positions [lane m, lane m + m): its chunk, ascending
    each_lane([&](int lane) {
        for (int p = lane * m; p < n0 && p < lane * m + m; ++p) {
            const int s = slot_b[p];
            sh.key[0][p] = ((uint32_t)(s < 0 || s >= n_out ? n_out : s) << kPBits) | (uint32_t)p;
        }
    });
    sync_lanes();
    int cur = 0;
    const int passes = (bits_of(n_out) + 3) / 4;  // digits of 4 bits that hold 0 .. n_out
    for (int pass = 0; pass < passes; ++pass) {
        const int shift = kPBits + 4 * pass;
        const uint32_t* src = sh.key[cur];
        uint32_t* dst = sh.key[cur ^ 1];
        each_lane([&](int lane) {
            int c[16];
            for (int d = 0; d < 16; ++d) c[d] = 0;
            for (int p = lane * m; p < n0 && p < lane * m + m; ++p) c[(src[p] >> shift) & 15]++;
            for (int d = 0; d < 16; ++d) sh.hist[d * kLanes + lane] = c[d];
        });
        sync_lanes();
        each_lane([&](int lane) {  // exclusive scan in [digit][lane] order: the lane's own 16 entries first ...
            int s = 0;
            for (int j = 0; j < 16; ++j) {
                const int v = sh.hist[lane * 16 + j];
                sh.hist[lane * 16 + j] = s;
                s += v;
            }
            sh.tot[lane] = s;
        });
        sync_lanes();
        each_lane([&](int lane) {  // ... then the sum of the lanes before it
            int base = 0;
            for (int j = 0; j < lane; ++j) base += sh.tot[j];
            for (int j = 0; j < 16; ++j) sh.hist[lane * 16 + j] += base;
        });
        sync_lanes();
        each_lane([&](int lane) {
            for (int p = lane * m; p < n0 && p < lane * m + m; ++p) {
                const uint32_t key = src[p];
                const int d = (key >> shift) & 15;
                const int at = sh.hist[d * kLanes + lane];
                sh.hist[d * kLanes + lane] = at + 1;
                if (at >= 0 && at < n0) dst[at] = key;
            }
        });
        sync_lanes();
        cur ^= 1;
    }
    const uint32_t* sorted = sh.key[cur];
    int32_t* start = (int32_t*)sh.key[cur ^ 1];
    each_lane([&](int lane) {
        for (int s = lane; s < n_out; s += kLanes) start[s] = 0, sh.hist[s] = 0;
    });
    sync_lanes();
    each_lane([&](int lane) {
        for (int i = lane; i < n0; i += kLanes) {
            const int s = (int)(sorted[i] >> kPBits);
            if (s >= n_out) continue;
            if (i == 0 || (int)(sorted[i - 1] >> kPBits) != s) start[s] = i;
            if (i == n0 - 1 || (int)(sorted[i + 1] >> kPBits) != s) sh.hist[s] = i + 1;
        }
    });
    sync_lanes();
    return cur;
}

// workgroup g of G of sample b: wave w takes the units (g * 4 + w) + j * 4 G, a unit being (slot, 64-lane column block), the LAST
// slot first (the merged token is the long one)
template <int V>
TM_HD void push_sample(PushShared& sh, const float* x, int64_t x_sb, int64_t x_sp, const int32_t* slot, const float* coef,
                       int64_t map_sb, float* y, int b, int g, int G, int n0, int n_out, int C) {
    typedef typename Vec<V>::type T;
    const int cur = sort_slots(sh, slot + (size_t)b * map_sb, n0, n_out);
    const uint32_t* sorted = sh.key[cur];
    const int32_t* start = (const int32_t*)sh.key[cur ^ 1];
    const float* coef_b = coef + (size_t)b * map_sb;
    const float* xb = x + (size_t)b * x_sb;
    const int blocks = (C + 64 * V - 1) / (64 * V);
    const int64_t units = (int64_t)n_out * blocks;
    each_lane([&](int lane) {
        const int wave = lane >> 6, wl = lane & 63;
        for (int64_t u = (int64_t)g * kWaves + wave; u < units; u += (int64_t)G * kWaves) {
            const int s = n_out - 1 - (int)(u / blocks), col = ((int)(u % blocks) * 64 + wl) * V;
            if (col >= C) continue;
            int i0 = start[s], i1 = sh.hist[s];
            if (i0 < 0 || i1 > n0 || i0 > i1) i0 = i1 = 0;
            float acc[V];
            for (int e = 0; e < V; ++e) acc[e] = 0.f;
            for (int i = i0; i < i1; i += 8) {  // eight cells' loads in flight, their sums in order
                T xs[8];
                float cs[8];
                for (int j = 0; j < 8; ++j) {
                    if (i + j < i1) {
                        const int p = (int)(sorted[i + j] & (kMaxN - 1));
                        cs[j] = coef_b[p];
                        xs[j] = *(const T*)(xb + (size_t)p * x_sp + col);
                    }
                }
                for (int j = 0; j < 8; ++j) {
                    if (i + j < i1) {
                        const float* xv = (const float*)&xs[j];
                        for (int e = 0; e < V; ++e) acc[e] = __builtin_fmaf(cs[j], xv[e], acc[e]);
                    }
                }
            }
            T out;
            for (int e = 0; e < V; ++e) ((float*)&out)[e] = acc[e];
            *(T*)(y + ((size_t)b * n_out + s) * C + col) = out;
        }
    });
}

// ---- pull ------------------------------------------------------------------------------------------------------------------------------
// cell e of sample b: position e / (C / V), columns (e % (C / V)) V ..
template <int V>
TM_HD void pull_cell(const float* v, const int32_t* slot, const float* coef, int64_t map_sb, float* out, int b, int64_t e, int n0,
                     int n_l, int C, bool weighted) {
    typedef typename Vec<V>::type T;
    const int cv = C / V;
    if (e >= (int64_t)n0 * cv) return;
    const int p = (int)(e / cv), col = (int)(e % cv) * V;
    const int s = slot[(size_t)b * map_sb + p];
    T r;
    for (int j = 0; j < V; ++j) ((float*)&r)[j] = 0.f;
    if (s >= 0 && s < n_l) {
        r = *(const T*)(v + ((size_t)b * n_l + s) * C + col);
        if (weighted) {
            const float c = coef[(size_t)b * map_sb + p];
            for (int j = 0; j < V; ++j) ((float*)&r)[j] *= c;
        }
    }
    *(T*)(out + ((size_t)b * n0 + p) * C + col) = r;
}

// ---- agree -----------------------------------------------------------------------------------------------------------------------------
struct AgreeShared {
    uint8_t cnt[2 * (kMaxL + 1) * kLanes];  // [min / max][depth][lane]: a lane counts its 16 positions at the most
    int32_t tot[2 * (kMaxL + 1)];
};

TM_HD void agree_sample(AgreeShared& sh, const int32_t* depth_a, const int32_t* depth_b, int32_t* out, int b, int n0, int L) {
    const int bins = L + 1;
    each_lane([&](int lane) {
        for (int j = 0; j < 2 * bins; ++j) sh.cnt[j * kLanes + lane] = 0;
        for (int p = lane; p < n0; p += kLanes) {
            int a = depth_a[(size_t)b * n0 + p], c = depth_b[(size_t)b * n0 + p];
            a = a < 0 ? 0 : a > L ? L : a;
            c = c < 0 ? 0 : c > L ? L : c;
            sh.cnt[(a < c ? a : c) * kLanes + lane]++;
            sh.cnt[(bins + (a < c ? c : a)) * kLanes + lane]++;
        }
    });
    sync_lanes();
    each_lane([&](int lane) {
        if (lane < 2 * bins) {
            int s = 0;
            for (int j = 0; j < kLanes; ++j) s += sh.cnt[lane * kLanes + j];
            sh.tot[lane] = s;
        }
    });
    sync_lanes();
    each_lane([&](int lane) {  // suffix sums: kept at layer l <=> depth > l
        if (lane < 2 * L) {
            const int l = lane >> 1, which = lane & 1;
            int s = 0;
            for (int d = l + 1; d <= L; ++d) s += sh.tot[which * bins + d];
            out[((size_t)b * L + l) * 2 + which] = s;
        }
    });
}

// ---- shade -----------------------------------------------------------------------------------------------------------------------------
struct alignas(16) B16 {
    uint8_t v[16];
};

// 16-byte group q of image b (the image's bytes are a multiple of 16)
TM_HD void shade_group(const uint8_t* images, const int32_t* depth, const uint8_t* level, uint8_t* out, int b, int64_t q, int gh, int gw,
                       int ph, int pw, int L) {
    const int64_t rowbytes = (int64_t)gw * pw * 3, bytes = rowbytes * gh * ph;
    if (q * 16 >= bytes) return;
    const size_t at = (size_t)b * bytes + (size_t)q * 16;
    const B16 in = *(const B16*)(images + at);
    B16 o;
    int row = (int)(q * 16 / rowbytes), col = (int)(q * 16 % rowbytes);
    for (int j = 0; j < 16; ++j) {
        int d = depth[(size_t)b * gh * gw + (size_t)(row / ph) * gw + col / 3 / pw];
        d = d < 0 ? 0 : d > L ? L : d;
        o.v[j] = (uint8_t)(((unsigned)in.v[j] * level[d] + 127u) / 255u);
        if (++col == rowbytes) col = 0, ++row;
    }
    *(B16*)(out + at) = o;
}

// ---- argument checks shared by the launches and the host emulation -----------------------------------------------------------------
inline bool sizes_ok(int B, int n0) { return B >= 1 && B <= MADTP_TOKENMAP_MAX_BATCH && n0 >= 1 && n0 <= kMaxN; }

inline int build_args(const int64_t* table, int L, int B, int n0, const int32_t* slot, const float* coef, const int32_t* depth,
                      const int32_t* status) {
    return (!table || !slot || !coef || !depth || !status || L < 1 || L > kMaxL || !sizes_ok(B, n0)) ? MADTP_E_BADARG : 0;
}

inline int push_args(const float* x, int64_t x_sb, int64_t x_sp, const int32_t* slot, const float* coef, int64_t map_sb, const float* y,
                     int B, int n0, int n_out, int C) {
    if (!x || !slot || !coef || !y || !sizes_ok(B, n0) || n_out < 1 || n_out > kMaxN || C < 1 || C > MADTP_TOKENMAP_MAX_C) return MADTP_E_BADARG;
    if (x_sp < C || x_sb < 0 || map_sb < 0 || (B > 1 && (x_sb < (int64_t)(n0 - 1) * x_sp + C || map_sb < n0))) return MADTP_E_BADARG;
    return 0;
}

inline bool push_vec4(const float* x, int64_t x_sb, int64_t x_sp, const float* y, int C) {
    return C % 4 == 0 && x_sb % 4 == 0 && x_sp % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0;
}

inline int pull_args(const float* v, const int32_t* slot, const float* coef, int64_t map_sb, const float* out, int B, int n0, int n_l,
                     int C, int weighted) {
    if (!v || !slot || (weighted && !coef) || !out || !sizes_ok(B, n0) || n_l < 1 || n_l > kMaxN || C < 1 || C > MADTP_TOKENMAP_MAX_C) return MADTP_E_BADARG;
    if (map_sb < 0 || (B > 1 && map_sb < n0) || (weighted != 0 && weighted != 1)) return MADTP_E_BADARG;
    return 0;
}

inline int agree_args(const int32_t* a, const int32_t* c, const int32_t* out, int B, int n0, int L) {
    return (!a || !c || !out || L < 1 || L > kMaxL || !sizes_ok(B, n0)) ? MADTP_E_BADARG : 0;
}

inline int shade_args(const void* images, const int32_t* depth, const void* level, const void* out, int B, int gh, int gw, int ph, int pw,
                      int L) {
    if (!images || !depth || !level || !out || L < 1 || L > kMaxL || gh < 1 || gw < 1 || ph < 1 || pw < 1) return MADTP_E_BADARG;
    if ((int64_t)gh * ph > 16384 || (int64_t)gw * pw > 16384 || !sizes_ok(B, 1) || (int64_t)gh * gw > kMaxN) return MADTP_E_BADARG;
    if ((uintptr_t)images % 16 || (uintptr_t)out % 16 || ((int64_t)gh * ph * gw * pw * 3) % 16) return MADTP_E_ALIGN;
    return 0;
}

// workgroups per sample of a push: enough for every unit to have a wave, eight at the most (each sorts the sample again)
inline int push_groups(int n_out, int C, int V) {
    const int64_t units = (int64_t)n_out * ((C + 64 * V - 1) / (64 * V));
    const int64_t g = (units + kWaves - 1) / kWaves;
    return (int)(g < 1 ? 1 : g > 8 ? 8 : g);
}

// ---- the host emulation ---------------------------------------------------------------------------------------------------------------
inline int build_host(const int64_t* table, int L, int B, int n0, int32_t* slot, float* coef, int32_t* depth, int32_t* status) {
    if (int rc = build_args(table, L, B, n0, slot, coef, depth, status)) return rc;
    BuildShared sh;
    for (int b = 0; b < B; ++b) build_sample(sh, table, L, n0, b, slot, coef, depth, status);
    return 0;
}

inline int push_host(const float* x, int64_t x_sb, int64_t x_sp, const int32_t* slot, const float* coef, int64_t map_sb, float* y, int B,
                     int n0, int n_out, int C) {
    if (int rc = push_args(x, x_sb, x_sp, slot, coef, map_sb, y, B, n0, n_out, C)) return rc;
    const bool v4 = push_vec4(x, x_sb, x_sp, y, C);
    const int G = push_groups(n_out, C, v4 ? 4 : 1);
    PushShared sh;
    for (int b = 0; b < B; ++b)
        for (int g = 0; g < G; ++g) {
            if (v4) push_sample<4>(sh, x, x_sb, x_sp, slot, coef, map_sb, y, b, g, G, n0, n_out, C);
            else push_sample<1>(sh, x, x_sb, x_sp, slot, coef, map_sb, y, b, g, G, n0, n_out, C);
        }
    return 0;
}

inline bool pull_vec4(const float* v, const float* out, int C) { return C % 4 == 0 && (uintptr_t)v % 16 == 0 && (uintptr_t)out % 16 == 0; }

inline int pull_host(const float* v, const int32_t* slot, const float* coef, int64_t map_sb, float* out, int B, int n0, int n_l, int C,
                     int weighted) {
    if (int rc = pull_args(v, slot, coef, map_sb, out, B, n0, n_l, C, weighted)) return rc;
    const bool v4 = pull_vec4(v, out, C);
    const int64_t cells = (int64_t)n0 * (v4 ? C / 4 : C);
    for (int b = 0; b < B; ++b)
        for (int64_t e = 0; e < cells; ++e) {
            if (v4) pull_cell<4>(v, slot, coef, map_sb, out, b, e, n0, n_l, C, weighted != 0);
            else pull_cell<1>(v, slot, coef, map_sb, out, b, e, n0, n_l, C, weighted != 0);
        }
    return 0;
}

inline int agree_host(const int32_t* a, const int32_t* c, int32_t* out, int B, int n0, int L) {
    if (int rc = agree_args(a, c, out, B, n0, L)) return rc;
    AgreeShared sh;
    for (int b = 0; b < B; ++b) agree_sample(sh, a, c, out, b, n0, L);
    return 0;
}

inline int shade_host(const void* images, const int32_t* depth, const void* level, void* out, int B, int gh, int gw, int ph, int pw, int L) {
    if (int rc = shade_args(images, depth, level, out, B, gh, gw, ph, pw, L)) return rc;
    const int64_t groups = (int64_t)gh * ph * gw * pw * 3 / 16;
    for (int b = 0; b < B; ++b)
        for (int64_t q = 0; q < groups; ++q) shade_group((const uint8_t*)images, depth, (const uint8_t*)level, (uint8_t*)out, b, q, gh, gw, ph, pw, L);
    return 0;
}

}  // namespace madtp_tokenmap

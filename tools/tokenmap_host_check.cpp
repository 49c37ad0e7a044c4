// Stand-alone check of the host emulation of the token map kernels (madtp_amd/csrc/tokenmap_device.h) under the host compiler's
// sanitizers:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/tokenmap_host_check.cpp -o tokenmap_host_check
//     ./tokenmap_host_check [rounds]
//
// Every round draws a seeded chain of layers (n0 up to 1100, up to 12 layers, some unpruned, record rows sometimes wider than what is
// read) into heap buffers of EXACTLY the sizes the table claims (a read or write past one is the sanitizer's to catch; the replayed
// tensors alone carry 16 bytes of slack, for their alignment), builds the map, replays it with push / pull / agree / shade, and
// checks the invariants that need no second implementation: every slot in range, a kept position alone in its slot with coef 1.0,
// every coef in [0, 1], push of ones equal to the coef sums, pull of the slot numbers equal to the slots.  Then the same records are
// damaged at seeded places - an index equal to n_in, a negative or far one, a repeat, a k that does not fit, a broken chain, a short
// stride, a null pointer - and every damaged build must give its code and leave the sample's outputs alone.  CPU only.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../madtp_amd/csrc/tokenmap_device.h"

using namespace madtp_tokenmap;

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t& s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

struct Layer {
    int n_in, k;  // k == -1: unpruned
    int64_t si, ss, sc;
    std::vector<int64_t> indices, sort;
    std::vector<float> score;
};

static int failures = 0;
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) {                       \
            printf(__VA_ARGS__), printf("\n"); \
            ++failures;                      \
        }                                    \
    } while (0)

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 200;
    long builds = 0, damaged = 0, coded = 0, replays = 0;
    uint32_t seed = 20240611u;
    for (int round = 0; round < rounds; ++round) {
        const int B = 1 + lcg(seed) % 3, L = 1 + lcg(seed) % 12;
        const int n0 = round % 7 == 0 ? 3 + lcg(seed) % 6 : 8 + lcg(seed) % 1093;
        std::vector<Layer> layers(L);
        int n = n0;
        for (int l = 0; l < L; ++l) {
            Layer& y = layers[l];
            y.n_in = n;
            y.k = (n < 3 || lcg(seed) % 5 == 0) && l > 0 ? -1 : 1 + (int)(lcg(seed) % (uint32_t)(n - 1));
            if (n < 2) y.k = -1;
            if (y.k < 0) continue;
            const int extra = lcg(seed) % 3 == 0 ? (int)(lcg(seed) % 9) : 0;
            y.si = y.k + extra, y.ss = n + extra, y.sc = n + extra;
            y.indices.assign((size_t)B * y.si, -99), y.sort.assign((size_t)B * y.ss, (int64_t)1 << 41), y.score.assign((size_t)B * y.sc, NAN);
            for (int b = 0; b < B; ++b) {
                std::vector<int64_t> perm(n);
                for (int i = 0; i < n; ++i) perm[i] = i;
                for (int i = n - 1; i > 0; --i) std::swap(perm[i], perm[lcg(seed) % (uint32_t)(i + 1)]);
                for (int i = 0; i < n; ++i) y.sort[(size_t)b * y.ss + i] = perm[i];
                for (int i = 0; i < y.k; ++i) y.indices[(size_t)b * y.si + i] = perm[(i + 3) % y.k];  // the kept ones, rotated
                const bool zeros = lcg(seed) % 9 == 0;
                for (int i = 0; i < n; ++i) y.score[(size_t)b * y.sc + i] = zeros && i % 2 ? 0.f : unit(seed) + 0.01f;
                if (zeros)
                    for (int i = y.k; i < n; ++i) y.score[(size_t)b * y.sc + perm[i]] = 0.f;
            }
            n = y.k + 1;
        }
        const int n_last = n;
        auto table_of = [&](std::vector<Layer>& ls) {
            std::vector<int64_t> t((size_t)L * kFields, 0);
            for (int l = 0; l < L; ++l) {
                int64_t* r = t.data() + (size_t)l * kFields;
                r[MADTP_TOKENMAP_F_N_IN] = ls[l].n_in, r[MADTP_TOKENMAP_F_K] = ls[l].k;
                if (ls[l].k < 0) continue;
                r[MADTP_TOKENMAP_F_INDICES] = (int64_t)(uintptr_t)ls[l].indices.data(), r[MADTP_TOKENMAP_F_INDICES_STRIDE] = ls[l].si;
                r[MADTP_TOKENMAP_F_SORT] = (int64_t)(uintptr_t)ls[l].sort.data(), r[MADTP_TOKENMAP_F_SORT_STRIDE] = ls[l].ss;
                r[MADTP_TOKENMAP_F_SCORE] = (int64_t)(uintptr_t)ls[l].score.data(), r[MADTP_TOKENMAP_F_SCORE_STRIDE] = ls[l].sc;
            }
            return t;
        };
        std::vector<int64_t> table = table_of(layers);
        const size_t cells = (size_t)B * L * n0;
        std::vector<int32_t> slot(cells, -7), depth((size_t)B * n0, -7), status(B, 1);
        std::vector<float> coef(cells, -7.f);
        int rc = build_host(table.data(), L, B, n0, slot.data(), coef.data(), depth.data(), status.data());
        ++builds;
        CHECK(rc == 0, "round %d: build -> %d", round, rc);
        for (int b = 0; b < B; ++b) CHECK(status[b] == 0, "round %d sample %d: a whole record gave status %d", round, b, status[b]);
        // invariants of the map, layer by layer
        for (int b = 0; b < B && !failures; ++b)
            for (int l = 0; l < L; ++l) {
                const int n_out = layers[l].k < 0 ? layers[l].n_in : layers[l].k + 1;
                std::vector<int> owners(n_out, 0), alone(n_out, 0);
                for (int p = 0; p < n0; ++p) {
                    const size_t at = ((size_t)b * L + l) * n0 + p;
                    CHECK(slot[at] >= 0 && slot[at] < n_out, "round %d: slot %d outside [0, %d)", round, slot[at], n_out);
                    if (slot[at] < 0 || slot[at] >= n_out) continue;
                    owners[slot[at]]++;
                    const bool kept = depth[(size_t)b * n0 + p] > l;
                    alone[slot[at]] += kept;
                    CHECK(!kept || coef[at] == 1.0f, "round %d: a kept position with coef %g", round, coef[at]);
                    CHECK(coef[at] >= 0.f && coef[at] <= 1.0f + 1e-5f, "round %d: coef %g", round, coef[at]);
                }
                for (int s = 0; s < n_out; ++s) CHECK(alone[s] == 0 || owners[s] == 1, "round %d layer %d: slot %d kept and shared", round, l, s);
            }
        // replay: push of ones gives the coef sums, pull of the slot numbers gives the slots, agree with itself is exact
        {
            const int C = round % 2 ? 4 : 3, l = L - 1;
            const size_t xn = (size_t)B * n0 * C + 4;
            std::vector<float> xraw(xn, 1.0f), yraw((size_t)B * n_last * C + 4, -1.f), vraw((size_t)B * n_last * C + 4), oraw(xn, -1.f);
            float* x = xraw.data() + ((16 - (uintptr_t)xraw.data() % 16) % 16) / 4;  // 16-byte aligned for C = 4, the exact size behind it
            float* yv = yraw.data() + ((16 - (uintptr_t)yraw.data() % 16) % 16) / 4;
            float* v = vraw.data() + ((16 - (uintptr_t)vraw.data() % 16) % 16) / 4;
            float* o = oraw.data() + ((16 - (uintptr_t)oraw.data() % 16) % 16) / 4;
            const int32_t* sl = slot.data() + (size_t)l * n0;
            const float* cf = coef.data() + (size_t)l * n0;
            rc = push_host(x, (int64_t)n0 * C, C, sl, cf, (int64_t)L * n0, yv, B, n0, n_last, C);
            CHECK(rc == 0, "round %d: push -> %d", round, rc);
            for (int b = 0; b < B; ++b)
                for (int s = 0; s < n_last; ++s) {
                    double want = 0;
                    for (int p = 0; p < n0; ++p)
                        if (sl[(size_t)b * L * n0 + p] == s) want += cf[(size_t)b * L * n0 + p];
                    for (int c = 0; c < C; ++c)
                        CHECK(std::fabs(yv[((size_t)b * n_last + s) * C + c] - want) <= 1e-4 * (1 + want), "round %d: push of ones %g, coef sum %g",
                              round, yv[((size_t)b * n_last + s) * C + c], want);
                }
            for (int b = 0; b < B; ++b)
                for (int s = 0; s < n_last; ++s)
                    for (int c = 0; c < C; ++c) v[((size_t)b * n_last + s) * C + c] = (float)s;
            rc = pull_host(v, sl, cf, (int64_t)L * n0, o, B, n0, n_last, C, round % 3 == 0);
            CHECK(rc == 0, "round %d: pull -> %d", round, rc);
            for (int b = 0; b < B; ++b)
                for (int p = 0; p < n0; ++p) {
                    const float w = round % 3 == 0 ? cf[(size_t)b * L * n0 + p] : 1.0f;
                    CHECK(o[((size_t)b * n0 + p) * C] == (float)sl[(size_t)b * L * n0 + p] * w, "round %d: pull", round);
                }
            std::vector<int32_t> ag((size_t)B * L * 2, -1);
            rc = agree_host(depth.data(), depth.data(), ag.data(), B, n0, L);
            CHECK(rc == 0, "round %d: agree -> %d", round, rc);
            for (size_t i = 0; i < ag.size(); i += 2) CHECK(ag[i] == ag[i + 1] && ag[i] >= 0 && ag[i] <= n0, "round %d: agree %d %d", round, ag[i], ag[i + 1]);
            if (n0 <= 64) {  // one patch of 4 x 4 pixels per position in a row: 48 n0 bytes per image
                std::vector<uint8_t> img((size_t)B * 48 * n0 + 16, 200), out((size_t)B * 48 * n0 + 16, 1), level(L + 1);
                for (int d = 0; d <= L; ++d) level[d] = (uint8_t)(255 * d / L);
                uint8_t* im = img.data() + (16 - (uintptr_t)img.data() % 16) % 16;
                uint8_t* ou = out.data() + (16 - (uintptr_t)out.data() % 16) % 16;
                rc = shade_host(im, depth.data(), level.data(), ou, B, 1, n0, 4, 4, L);
                CHECK(rc == 0, "round %d: shade -> %d", round, rc);
                for (int b = 0; b < B; ++b)
                    for (int p = 0; p < n0; ++p)
                        CHECK(ou[(size_t)b * 48 * n0 + 12 * p] == (200 * level[depth[(size_t)b * n0 + p]] + 127) / 255, "round %d: shade", round);
            }
            replays += 4;
        }
        // damage: one place per try, in sample B - 1
        for (int t = 0; t < 24; ++t) {
            std::vector<Layer> bad(layers);
            std::vector<int> pruned;
            for (int l = 0; l < L; ++l)
                if (bad[l].k > 0) pruned.push_back(l);
            if (pruned.empty()) break;
            const int l = pruned[lcg(seed) % pruned.size()], b = B - 1, kind = t % 8;
            Layer& y = bad[l];
            int want = 0;
            bool whole_batch = false, null_score = false;
            const size_t ki = (size_t)b * y.si + lcg(seed) % (uint32_t)y.k;
            const size_t mi = (size_t)b * y.ss + y.k + lcg(seed) % (uint32_t)(y.n_in - y.k);
            if (kind == 0) y.indices[ki] = y.n_in, want = MADTP_TOKENMAP_E_RANGE;
            if (kind == 1) y.sort[mi] = -1 - (int64_t)(lcg(seed) % 5), want = MADTP_TOKENMAP_E_RANGE;
            if (kind == 2) y.indices[ki] = ((int64_t)1 << 33) + 1, want = MADTP_TOKENMAP_E_RANGE;
            if (kind == 3) y.indices[ki] = y.sort[mi], want = MADTP_TOKENMAP_E_REPEAT;
            if (kind == 4) {
                if (y.k < 2) continue;
                y.indices[(size_t)b * y.si] = y.indices[(size_t)b * y.si + y.k - 1], want = MADTP_TOKENMAP_E_REPEAT;
            }
            if (kind == 5) y.k = lcg(seed) % 2 ? y.n_in + (int)(lcg(seed) % 3) : 0, want = MADTP_TOKENMAP_E_K, whole_batch = true;
            if (kind == 6) y.n_in += 1, want = MADTP_TOKENMAP_E_CHAIN, whole_batch = true;
            if (kind == 7) {
                if (lcg(seed) % 2) y.ss = y.n_in - 1;
                else null_score = true;
                want = MADTP_TOKENMAP_E_TABLE, whole_batch = true;
            }
            std::vector<int64_t> tb = table_of(bad);
            if (null_score) tb[(size_t)l * kFields + MADTP_TOKENMAP_F_SCORE] = 0;
            std::fill(slot.begin(), slot.end(), -7), std::fill(coef.begin(), coef.end(), -7.f), std::fill(depth.begin(), depth.end(), -7);
            rc = build_host(tb.data(), L, B, n0, slot.data(), coef.data(), depth.data(), status.data());
            ++damaged;
            CHECK(rc == 0, "round %d: damaged build -> %d", round, rc);
            CHECK(status[b] == status_word(want, l), "round %d kind %d layer %d: status %d, expected %d", round, kind, l, status[b], status_word(want, l));
            coded += status[b] != 0;
            for (int s = 0; s < B; ++s) {
                const bool untouched = slot[(size_t)s * L * n0] == -7 && coef[(size_t)s * L * n0 + (size_t)L * n0 - 1] == -7.f && depth[(size_t)s * n0] == -7;
                CHECK((status[s] != 0) == untouched, "round %d kind %d: sample %d status %d, outputs %s", round, kind, s, status[s], untouched ? "untouched" : "written");
                CHECK(whole_batch || s == b || status[s] == 0, "round %d kind %d: the undamaged sample %d gave %d", round, kind, s, status[s]);
            }
        }
    }
    printf("%d rounds: %ld whole builds, %ld replays, %ld damaged builds of which %ld gave their code; %d failures\n", rounds, builds, replays, damaged,
           coded, failures);
    return failures ? 1 : 0;
}

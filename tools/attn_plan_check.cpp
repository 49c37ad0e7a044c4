// attn_plan.h on its own, with the host compiler alone (no HIP): plans the boundary shapes of the dispatch and prints a checksum.
//   c++ -std=c++17 -Wall -Wextra -fsanitize=address,undefined tools/attn_plan_check.cpp -o attn_plan_check && ./attn_plan_check
#include <stdio.h>

#include "../madtp_amd/csrc/attn_plan.h"

int main() {
    unsigned long sum = 0, plans = 0;
    const int keys[] = {-1, 0, 1, 16, 32, 33, 64, 65, 96, 97, 128, 160, 161, 192, 193, 208, 209, 256, 257, 384, 385, 640, 641, 1024, 1025};
    const int batches[] = {0, 1, 2, 127, 128, 129, 383, 384, 385, 511, 512, 513}, heads[] = {1, 2, 3, 12, 16, 20};
    for (int dt = -1; dt <= 4; ++dt)
        for (int Nk : keys)
            for (int B : batches)
                for (int H : heads)
                    for (int flags = 0; flags < 64; ++flags) {  // pair, scores, [Nq,Nk] mask, device-side length, K/V block, planes
                        AttnProblem p{};
                        p.B = B; p.H = H; p.Nk = Nk; p.Nq = (flags & 2) ? Nk : 20; p.ldq = p.ldk = p.ldv = 3 * H * 64; p.ldo = 2 * H * 64;
                        p.io_dtype = dt; p.pair = flags & 1; p.scores = flags & 2; p.mask_qk = flags & 4; p.ld_mask_qk = Nk; p.n_dev = flags & 8;
                        p.kv_block_rows = (flags & 16) ? Nk + 1 : 0; p.split_req = (flags & 32) ? H * 64 : 0;
                        p.ptrs = p.p0 = p.onorm = p.qkv_aligned = p.out_aligned16 = p.out_aligned8 = p.pair_aligned = p.pair_masks_alike = true;
                        for (int res = 0; res < 4; ++res) {
                            AttnResources r; r.hm = res & 1; r.opart = res & 2;
                            const AttnPlan pl = attn_plan(p, AttnSwitches{}, r);
                            sum = sum * 31 + (unsigned long)(pl.status * 7 + pl.family * 5 + pl.nt * 3 + pl.gz + pl.lds + pl.block);
                            ++plans;
                        }
                    }
    printf("%lu plans, checksum %lx\n", plans, sum);
    return 0;
}

#!/usr/bin/env python
"""A/B of the candidate stage of retrieval: the dense routes against search.topk_embeds, on one GPU.

    python tools/topk_ab.py [--nq N --nk N --dim D --k K] [--rounds R] [--iters N] [--out FILE]

  leg A   what blip_retrieval.evaluate(candidates="dense") does before it re-ranks: the [nq, nk] f32 sims_matrix by a matmul, then
          sims_matrix[i].topk(k) once per row in a Python loop, and the same over the transposed view: nq + nk launches (the index
          gathers that follow each of them in evaluate() are not part of the leg);
  leg A'  the same product, then ONE batched torch.topk per direction;
  leg B   search.topk_embeds in both directions: no matrix.
Every leg answers both directions (nq queries over nk keys, and the transpose).  Leg B must return the index SETS of leg A' on
every row whose k-th gap (the f32 scores at positions k - 1 and k) is at least 2e-6, or the tool fails.
Inputs: unit-norm rows from torch.Generator(seed).  Defaults: COCO 5000 x 25010 at D 256 / k 256 and at D 512, 768 / k 10;
Flickr 1000 x 5000 at D 256 / k 128.
Timing: device events around each leg; the legs alternate inside every round, leg A runs once per round and the others --iters
times; each figure is the median over the rounds of the per-round median, with the min and max.  Peak memory: the allocator's
peak above what is live before the leg (the embeddings).  The kernel figures (registers, LDS, waves) are the compiler's, copied
here from -Rpass-analysis=kernel-resource-usage: see KERNELS.

    python tools/topk_ab.py --coarse [--kernels-only] [--out FILE]

  leg E   search.topk_embeds, the exact route (leg B above);
  leg A'  as above;
  leg C   search.EmbeddingIndex(keys, coarse="bf16").search: the certified bf16 shortlist over a gallery prepared once (the
          gallery's prepare + summary are timed on their own, and so is the one-shot search.topk_embeds(coarse="bf16")).
The outputs of legs C and E are asserted EQUAL (indices, and the values' bits), on unit-norm Gaussian rows and on "CLIP-like" rows
(a common mean direction of weight 0.8).  Per shape: the certified share, the bytes the exact re-scoring gathers (nq m rows of
4 D bytes) and the compiler's figures for the new kernels (COARSE_KERNELS, from tools/kernel_resources.py).  The time of each
of the five stages comes from a kernel trace of `--coarse --kernels-only` (tools/rocpd_stats.py): that run makes ten coarse
searches per shape and direction and nothing else."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from madtp_amd import hip, search  # noqa: E402

F32_PEAK = 157.3e12  # v_mfma_f32_16x16x4_f32 = the f32 vector rate
GAP = 2e-6
# topk_tile_kernel<CAP>: (largest k, candidate words per row, VGPRs + AGPRs, LDS bytes per workgroup = 26 752 static + 256 CAP,
#                         workgroups per CU by LDS (160 KiB) = waves per SIMD, 4 waves per workgroup)
KERNELS = [(64, 128, "159 + 8", 26752 + 256 * 128, 2), (128, 256, "230 + 8", 26752 + 256 * 256, 1), (256, 512, "114 + 8", 26752 + 256 * 512, 1)]


# search_coarse.hip: kernel, VGPRs, AGPRs, LDS bytes per workgroup (static + dynamic), waves per SIMD (registers / LDS)
COARSE_KERNELS = [("coarse_prepare_kernel", 50, 0, 0, 8), ("ctopk_tile_kernel<128> (m 64)", 168, 0, 14464 + 256 * 128, 3),
                  ("ctopk_tile_kernel<256> (m 128)", 228, 0, 14464 + 256 * 256, 2), ("ctopk_tile_kernel<512> (m 256)", 136, 0, 14464 + 256 * 512, 1),
                  ("ctopk_row_kernel", 74, 0, 8464, 6), ("ctopk_compact_kernel", 18, 0, 1024, 8),
                  ("topk_tile_kernel<128, mapped> (fallback, k <= 64)", 164, 0, 26752 + 256 * 128, 2),
                  ("topk_tile_kernel<256, mapped> (fallback, k <= 128)", 244, 0, 26752 + 256 * 256, 1),
                  ("topk_row_kernel<mapped>", 46, 0, 4368, 8)]
COARSE_CASES = [(5000, 25010, 256, 128), (5000, 25010, 512, 10), (5000, 25010, 768, 10), (1000, 5000, 256, 128)]


def clip_like(n, D, seed, dev, mean=0.8):
    """unit rows around one common direction (seed-independent, so queries and keys share it): mean mu + sqrt(1 - mean^2) noise"""
    mu = features(1, D, 77, dev).double()
    noise = features(n, D, seed, dev).double()
    x = mean * mu + (1 - mean * mean) ** 0.5 * noise
    return (x / x.norm(dim=1, keepdim=True)).float().contiguous()


def features(n, D, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(n, D, generator=g, device=dev, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float().contiguous()


def leg_loop(q, keys, k):
    sims = q @ keys.t()
    for i in range(sims.shape[0]):
        sims[i].topk(k=k, dim=0)
    sims_t = sims.t()
    for i in range(sims_t.shape[0]):
        sims_t[i].topk(k=k, dim=0)


def leg_batched(q, keys, k):
    sims = q @ keys.t()
    return sims.topk(k, dim=1), sims.t().topk(k, dim=1)


def leg_device(q, keys, k):
    return search.topk_embeds(q, keys, k), search.topk_embeds(keys, q, k)


def events(fn, n):
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(ts)


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def same_sets(q, keys, k):
    """rows compared, rows in all: leg B's index sets against the batched dense route's where the k-th gap is >= GAP"""
    sims = q @ keys.t()
    kk = min(k + 1, sims.shape[1])
    v, i = sims.topk(kk, dim=1)
    clear = (v[:, k - 1] - v[:, k] >= GAP) if kk > k else torch.ones(sims.shape[0], dtype=torch.bool, device=q.device)
    _, mine = search.topk_embeds(q, keys, k)
    a, b = i[:, :k].sort(dim=1).values, mine.sort(dim=1).values
    bad = ((a != b).any(dim=1) & clear).sum().item()
    return bad, int(clear.sum().item()), sims.shape[0]


def summary(v):
    return f"{statistics.median(v) * 1e3:10.3f} ms (min {min(v) * 1e3:.3f}, max {max(v) * 1e3:.3f})"


def case(nq, nk, D, k, a, dev, out):
    q, keys = features(nq, D, 1000 + D, dev), features(nk, D, 2000 + D, dev)
    for _ in range(2):
        leg_batched(q, keys, k)
        leg_device(q, keys, k)
    checks = [same_sets(q, keys, k), same_sets(keys, q, k)]
    ok = all(c[0] == 0 for c in checks)
    per = {"A": [], "A'": [], "B": [], "B1": [], "B2": []}
    for _ in range(a.rounds):
        if not a.no_loop:
            per["A"].append(events(lambda: leg_loop(q, keys, k), 1))
        per["A'"].append(events(lambda: leg_batched(q, keys, k), a.iters))
        per["B"].append(events(lambda: leg_device(q, keys, k), a.iters))
        per["B1"].append(events(lambda: search.topk_embeds(q, keys, k), a.iters))
        per["B2"].append(events(lambda: search.topk_embeds(keys, q, k), a.iters))
    mem = {name: peak_bytes(lambda fn=fn: fn(q, keys, k)) for name, fn in (("A'", leg_batched), ("B", leg_device))}
    ws = [int(search.lib().madtp_topk_workspace(n1, n2, D, k)) for n1, n2 in ((nq, nk), (nk, nq))]
    batched, mem_dense = per["A'"], mem["A'"]
    b, ab = statistics.median(per["B"]), statistics.median(batched)
    flops = 2 * 2.0 * nq * nk * D
    kmax, cap, regs, lds, waves = next(row for row in KERNELS if k <= row[0])
    lines = [f"nq {nq} nk {nk} D {D} k {k}: index sets {'equal' if ok else 'DIFFER'} on the "
             f"{checks[0][1]} of {checks[0][2]} + {checks[1][1]} of {checks[1][2]} rows with a k-th gap >= {GAP:g}"]
    if per["A"]:
        r = statistics.median(per["A"]) / b
        lines.append(f"  leg A  dense + topk per row ({nq + nk} launches) {summary(per['A'])}   A / B = {r:.1f}x{'' if r > 1 else '   LOSES'}")
    lines += [f"  leg A' dense + one batched topk per direction {summary(batched)}   A' / B = {ab / b:.2f}x"
              f"{'' if ab > b else '   topk_embeds LOSES'}",
              f"  leg B  topk_embeds, both directions           {summary(per['B'])}",
              f"      {nq} x {nk}: {summary(per['B1'])}   {nk} x {nq}: {summary(per['B2'])}",
              f"      {flops / 1e9:.1f} GFLOP -> {flops / b / 1e12:.1f} TFLOP/s = {100 * flops / b / F32_PEAK:.1f} % of the f32 matrix peak "
              f"({F32_PEAK / 1e12:.1f} TF)",
              f"  peak memory above the embeddings: leg A / A' {mem_dense / 1e6:.1f} MB, leg B {mem['B'] / 1e6:.1f} MB "
              f"(workspaces {ws[0] / 1e6:.1f} + {ws[1] / 1e6:.1f} MB, one live at a time; the f32 matrix alone is {4e-6 * nq * nk:.1f} MB)",
              f"  topk_tile_kernel<{cap}> (k <= {kmax}): {regs} VGPRs + AGPRs, {lds} B of LDS per workgroup -> {waves} workgroup(s) per CU = "
              f"{waves} wave(s) per SIMD; topk_row_kernel: 46 VGPRs, 4368 B, 8 waves per SIMD"]
    for line in lines:
        print(line, flush=True)
        out.append(line)
    return ok


def equal(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def coarse_case(nq, nk, D, k, family, a, dev, out):
    gen = features if family == "gaussian" else clip_like
    q, keys = gen(nq, D, 1000 + D, dev), gen(nk, D, 2000 + D, dev)
    m = search.check_coarse("bf16", k, "topk_ab")
    idx_k, idx_q = search.EmbeddingIndex(keys, coarse="bf16"), search.EmbeddingIndex(q, coarse="bf16")
    leg_c = lambda: (idx_k.search(q, k), idx_q.search(keys, k))
    if a.kernels_only:
        for _ in range(10):
            leg_c()
        torch.cuda.synchronize()
        return True
    for _ in range(2):
        leg_batched(q, keys, k)
        leg_device(q, keys, k)
        leg_c()
    ok, shares = True, []
    for index, qq, kk in ((idx_k, q, keys), (idx_q, keys, q)):
        v, i, info = index.search(qq, k, return_info=True)
        ok &= equal((v, i), search.topk_embeds(qq, kk, k)) and equal((v, i), search.topk_embeds(qq, kk, k, coarse="bf16"))
        shares.append((1.0 - info.n_fallback / qq.shape[0], qq.shape[0]))
    per = {"A'": [], "E": [], "C": [], "C1": [], "C2": [], "P": [], "O": []}
    for _ in range(a.rounds):
        per["A'"].append(events(lambda: leg_batched(q, keys, k), a.iters))
        per["E"].append(events(lambda: leg_device(q, keys, k), a.iters))
        per["C"].append(events(leg_c, a.iters))
        per["C1"].append(events(lambda: idx_k.search(q, k), a.iters))
        per["C2"].append(events(lambda: idx_q.search(keys, k), a.iters))
        per["P"].append(events(lambda: (search.summary(search.prepare(keys)[1]), search.summary(search.prepare(q)[1])), a.iters))
        per["O"].append(events(lambda: (search.topk_embeds(q, keys, k, coarse="bf16"), search.topk_embeds(keys, q, k, coarse="bf16")), a.iters))
    dense = per["A'"]
    c, e, ab = (statistics.median(per[x]) for x in ("C", "E", "A'"))
    ws = [int(search.clib().madtp_ctopk_workspace(n1, n2, D, k, m)) for n1, n2 in ((nq, nk), (nk, nq))]
    lines = [f"{family}: nq {nq} nk {nk} D {D} k {k} m {m}: coarse and exact outputs {'EQUAL' if ok else 'DIFFER'}; certified "
             f"{100 * shares[0][0]:.2f} % of {shares[0][1]} rows, {100 * shares[1][0]:.2f} % of {shares[1][1]} rows",
             f"  leg E  exact route, both directions               {summary(per['E'])}",
             f"  leg A' dense + one batched topk per direction     {summary(dense)}",
             f"  leg C  coarse route over a prepared gallery       {summary(per['C'])}   E / C = {e / c:.2f}x{'' if e > c else '   COARSE LOSES'}"
             f"   A' / C = {ab / c:.2f}x{'' if ab > c else '   COARSE LOSES'}",
             f"      {nq} x {nk}: {summary(per['C1'])}   {nk} x {nq}: {summary(per['C2'])}",
             f"  gallery prepare + summary, both galleries         {summary(per['P'])}",
             f"  one-shot topk_embeds(coarse='bf16'), both (= C + P) {summary(per['O'])}",
             f"  re-scoring gathers {nq} x {m} + {nk} x {m} rows of {4 * D} B = {(nq + nk) * m * 4 * D / 1e6:.1f} MB; workspaces "
             f"{ws[0] / 1e6:.1f} + {ws[1] / 1e6:.1f} MB"]
    for line in lines:
        print(line, flush=True)
        out.append(line)
    return ok


def coarse_main(a):
    out = [f"tools/topk_ab.py --coarse on {torch.cuda.get_device_name(0)}: {a.rounds} alternating rounds, {a.iters} calls per leg and round, "
           "device events, medians of per-round medians"]
    cases = [(a.nq, a.nk, a.dim, a.k)] if a.nq and a.nk else COARSE_CASES
    ok = True
    for nq, nk, D, k in cases:
        for family in ("gaussian", "clip_like")[:1 if a.kernels_only else 2]:
            ok &= coarse_case(nq, nk, D, k, family, a, "cuda", out)
    if a.kernels_only:
        return
    out.append("kernels of search_coarse.hip (tools/kernel_resources.py): VGPRs, AGPRs, LDS bytes per workgroup, waves per SIMD")
    out += [f"  {name}: {v} VGPRs, {g} AGPRs, {lds} B, {w}" for name, v, g, lds, w in COARSE_KERNELS]
    path = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "topk_coarse_ab.txt")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(out) + "\n")
    if not ok:
        raise SystemExit("topk_ab: the coarse and the exact route returned different outputs")


DEFAULT_OUT = os.path.join(ROOT, "profiles", "topk_ab.txt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coarse", action="store_true", help="the certified bf16 shortlist against the exact and the dense route")
    ap.add_argument("--kernels-only", action="store_true", help="with --coarse: ten coarse searches per shape, for a kernel trace")
    ap.add_argument("--nq", type=int, default=0)
    ap.add_argument("--nk", type=int, default=0)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-loop", action="store_true", help="skip leg A (nq + nk launches per round)")
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_ab: needs the GPU (a CPU run measures nothing)")
    hip.load()
    if a.coarse:
        return coarse_main(a)
    cases = [(a.nq, a.nk, a.dim, a.k)] if a.nq and a.nk else [(5000, 25010, 256, 256), (5000, 25010, 512, 10), (5000, 25010, 768, 10),
                                                               (1000, 5000, 256, 128)]
    out = [f"tools/topk_ab.py on {torch.cuda.get_device_name(0)}: {a.rounds} alternating rounds, leg A once and the others {a.iters} calls "
           "per round, device events, medians of per-round medians"]
    ok = True
    for nq, nk, D, k in cases:
        ok &= case(nq, nk, D, k, a, "cuda", out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    if not ok:
        raise SystemExit("topk_ab: topk_embeds and the dense route returned different index sets on rows with a clear k-th gap")


if __name__ == "__main__":
    main()

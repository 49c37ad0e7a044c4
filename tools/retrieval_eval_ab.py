#!/usr/bin/env python
"""A/B of retrieval evaluation: the reference's host route against ranking on the device, on one GPU.

    python tools/retrieval_eval_ab.py [--nq N --nk N] [--dim D] [--rounds R] [--iters N] [--out FILE] [--kernels-only]

  leg A  the route of compress_retrieval_clip_dtp.py evaluate() :121-124 + itm_eval() :127-171, restated here: the [nq, nk] f32
         similarity matrix by a matmul on the device, the matrix and its transpose copied to the host as numpy arrays, then one
         argsort per row and a search for each ground-truth column in the sorted order.  The sort is kind="stable" so that ties
         fall as the kernel's rule says (the reference's default leaves them open);
  leg B  what ClipEval.metrics() does: retrieval_eval.target_lists (the ground truth validated on the host, built as CSR and
         uploaded - a Python loop over the nq + nk rows), rank_embeds in both directions, recall_metrics: no matrix, the per-row
         ranks (nq + nk int32) are all that comes back.  target_lists alone is also timed on its own: a caller that evaluates
         the same dataset every epoch can keep its result.
Both legs must return the same nine-key dict, or the tool fails.  Features: entries k / 8 with k in -4 .. 4, caption j copying
its image on a random 0.05 (1 + j % 4) share of the features - every dot product is exact in f32 in any summation order, so the
two legs see the same scores; ties are frequent.  5 captions per image (the captions past 5 nq go to the first images).
Defaults: COCO 5000 x 25010 and Flickr 1000 x 5000 at D 512 and 768.
Timing: a host clock around each leg, ending in a device synchronise; the legs alternate inside every round and each figure is
the median over the rounds of its per-round median (leg A runs once per round, leg B --iters times), with the min and max.
rank_embeds alone (its three launches, both directions) is timed with device events; the operations and bytes below it are
computed from the shapes.  --kernels-only runs leg B alone, for a kernel trace under rocprofv3."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from madtp_amd import hip, retrieval_eval as re  # noqa: E402

F32_PEAK = 157.3e12  # v_mfma_f32_16x16x4_f32 = the f32 vector rate
HBM_PEAK = 8.0e12
ROW_TILE, COL_TILE = 32, 64  # csrc/eval.hip


def features(nq, nk, D, dev):
    g = torch.Generator(device=dev).manual_seed(nq + D)
    img = torch.randint(-4, 5, (nq, D), generator=g, device=dev).float() / 8
    txt = torch.randint(-4, 5, (nk, D), generator=g, device=dev).float() / 8
    j = torch.arange(nk, device=dev)
    txt2img = torch.where(j < 5 * nq, j // 5, (j - 5 * nq) % nq)
    copy = torch.rand(nk, D, generator=g, device=dev) < (0.05 * (1 + j % 4)).float()[:, None]
    txt = torch.where(copy, img[txt2img], txt)
    txt2img = txt2img.tolist()
    img2txt = [[] for _ in range(nq)]
    for t, i in enumerate(txt2img):
        img2txt[i].append(t)
    return img, txt, txt2img, img2txt


def host_route(img, txt, txt2img, img2txt):
    sims = img @ txt.t()
    s_i2t, s_t2i = sims.cpu().numpy(), sims.t().cpu().numpy()
    ranks_i = np.zeros(s_i2t.shape[0])
    for r, row in enumerate(s_i2t):
        order = np.argsort(row, kind="stable")[::-1]
        ranks_i[r] = min(np.where(order == t)[0][0] for t in img2txt[r])
    ranks_t = np.zeros(s_t2i.shape[0])
    for r, row in enumerate(s_t2i):
        order = np.argsort(row, kind="stable")[::-1]
        ranks_t[r] = np.where(order == txt2img[r])[0][0]
    return re.recall_metrics(ranks_i, ranks_t)


def device_route(img, txt, txt2img, img2txt):
    targets = re.target_lists(txt2img, img2txt, img.shape[0], txt.shape[0], device=img.device)
    ri, _, _ = re.rank_embeds(img, txt, targets.i2t_ptr, targets.i2t_idx)
    rt, _, _ = re.rank_embeds(txt, img, targets.t2i_ptr, targets.t2i_idx)
    return re.recall_metrics(ri, rt)


def clocked(fn, n):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def kernel_events(img, txt, targets, n):
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        re.rank_embeds(img, txt, targets.i2t_ptr, targets.i2t_idx)
        re.rank_embeds(txt, img, targets.t2i_ptr, targets.t2i_idx)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(ts)


def summary(v):
    return f"{statistics.median(v) * 1e3:10.3f} ms (min {min(v) * 1e3:.3f}, max {max(v) * 1e3:.3f})"


def case(nq, nk, D, a, dev, out):
    img, txt, txt2img, img2txt = features(nq, nk, D, dev)
    targets = re.target_lists(txt2img, img2txt, nq, nk, device=dev)
    for _ in range(3):
        got_b = device_route(img, txt, txt2img, img2txt)
    if a.kernels_only:
        for _ in range(a.iters):
            device_route(img, txt, txt2img, img2txt)
        torch.cuda.synchronize()
        return True
    got_a = host_route(img, txt, txt2img, img2txt)
    same = got_a == got_b
    per = {"A": [], "B": [], "T": [], "K": []}
    for _ in range(a.rounds):
        per["A"].append(clocked(lambda: host_route(img, txt, txt2img, img2txt), 1))
        per["B"].append(clocked(lambda: device_route(img, txt, txt2img, img2txt), a.iters))
        per["T"].append(clocked(lambda: re.target_lists(txt2img, img2txt, nq, nk, device=dev), a.iters))
        per["K"].append(kernel_events(img, txt, targets, a.iters))
    k = statistics.median(per["K"])
    flops = 2 * 2.0 * nq * nk * D                      # both directions, 2 per multiply-add
    compulsory = 2 * 4.0 * (nq + nk) * D               # every feature row once per direction
    tiles = lambda n, t: (n + t - 1) // t              # noqa: E731
    streamed = 4.0 * D * (tiles(nq, ROW_TILE) * nk + tiles(nk, COL_TILE) * nq + tiles(nk, ROW_TILE) * nq + tiles(nq, COL_TILE) * nk)
    ratio = statistics.median(per["A"]) / statistics.median(per["B"])
    lines = [f"nq {nq} nk {nk} D {D}: dicts {'equal' if same else 'DIFFER'}  R@1 i2t {got_b['txt_r1']:.2f} t2i {got_b['img_r1']:.2f}",
             f"  leg A host route     {summary(per['A'])}",
             f"  leg B device ranking {summary(per['B'])}   A / B = {ratio:.0f}x{'' if ratio > 1 else '   LOSES'}",
             f"    of which target_lists  {summary(per['T'])}",
             f"  rank_embeds x 2, device events {summary(per['K'])}",
             f"    {flops / 1e9:.1f} GFLOP -> {flops / k / 1e12:.1f} TFLOP/s = {100 * flops / k / F32_PEAK:.1f} % of the f32 matrix peak "
             f"({F32_PEAK / 1e12:.1f} TF)",
             f"    bytes: {compulsory / 1e6:.1f} MB compulsory = {100 * compulsory / k / HBM_PEAK:.2f} % of HBM peak "
             f"({HBM_PEAK / 1e12:.0f} TB/s); {streamed / 1e9:.2f} GB streamed through the tiles = {streamed / k / 1e12:.2f} TB/s "
             "(served by the caches)"]
    for line in lines:
        print(line, flush=True)
        out.append(line)
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=0)
    ap.add_argument("--nk", type=int, default=0)
    ap.add_argument("--dim", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_eval_ab.txt"))
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_eval_ab: needs the GPU (a CPU run measures nothing)")
    hip.load()
    sizes = [(a.nq, a.nk)] if a.nq and a.nk else [(5000, 25010), (1000, 5000)]
    dims = [a.dim] if a.dim else [512, 768]
    out = [f"tools/retrieval_eval_ab.py on {torch.cuda.get_device_name(0)}: {a.rounds} alternating rounds, leg B and the events "
           f"{a.iters} calls per round, medians of per-round medians"]
    ok = True
    for nq, nk in sizes:
        for D in dims:
            ok &= case(nq, nk, D, a, "cuda", out)
    if not a.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(out) + "\n")
    if not ok:
        raise SystemExit("retrieval_eval_ab: the two legs returned different metrics")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""A/B of the tail of a BLIP retrieval evaluation: dense score matrices against re-ranked candidate lists, on one GPU.

    python tools/lists_ab.py [--n-img N --n-txt N --k-test K] [--rounds R] [--iters N] [--out FILE]

What is measured is everything evaluate() and itm_eval() do with the re-ranked values once they exist - not the re-ranking, which
is the same calls in both routes and dominates an evaluation either way.  The values are synthetic (no model): every query row
has k_test distinct candidate keys, its ground truth among them with probability 0.7, and integer-valued scores so that ties occur.
  leg A  the dense route: two matrices [n_img, n_txt] and [n_txt, n_img] filled with -100, the k_test values of every row
         scattered into them (one scatter per matrix, not one per row: the cheapest form of what the loops do), both copied to
         the host as numpy arrays, retrieval_eval.itm_eval on the arrays (which uploads them and runs madtp_rank_scores);
  leg B  the lists route: the values in [n, k_test] tensors next to the indices, retrieval_eval.itm_eval on two CandidateLists
         (madtp_lists_rank); nothing leaves the device but the per-row ranks.
Both legs must return the same nine-key dict, or the tool fails.  Both include retrieval_eval.target_lists (a host loop over the
rows), which is also timed alone.  Defaults: COCO 5000 x 25010 at k_test 256 and Flickr 1000 x 5000 at k_test 128.
Timing: a host clock around each leg, ending in a device synchronise; the legs alternate inside every round and each figure is
the median over the rounds of its per-round median (leg A runs once per round, leg B --iters times), with the min and max.
Memory: torch.cuda.max_memory_allocated of one run of each leg above what the inputs occupy.  madtp_lists_rank and madtp_lists_sort
alone (both directions) are timed with device events; their bytes are computed from the shapes."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from madtp_amd import hip, retrieval_eval as re  # noqa: E402
from madtp_amd import lists  # noqa: E402
from madtp_amd.lists import CandidateLists  # noqa: E402

HBM_PEAK = 8.0e12


def synthetic(n_img, n_txt, k, dev):
    """-> ((idx, val) image -> text, (idx, val) text -> image, txt2img, img2txt)"""
    g = torch.Generator(device=dev).manual_seed(n_img + k)
    j = torch.arange(n_txt, device=dev)
    txt2img = torch.where(j < 5 * n_img, j // 5, (j - 5 * n_img) % n_img)

    def side(n, nk, truth):
        # k distinct random keys per row (the k largest of nk random numbers), the ground truth in a random slot of 70 % of the rows
        idx = torch.rand(n, nk, generator=g, device=dev).topk(k, dim=1).indices
        hit = torch.rand(n, generator=g, device=dev) < 0.7
        slot = torch.randint(0, k, (n,), generator=g, device=dev)
        rows = torch.arange(n, device=dev)
        clash = (idx == truth[:, None]).any(dim=1)
        put = hit & ~clash
        idx[rows[put], slot[put]] = truth[put]
        val = torch.randint(-8, 9, (n, k), generator=g, device=dev).float()
        return idx.contiguous(), val
    i2t = side(n_img, n_txt, torch.arange(n_img, device=dev) * 5 % n_txt)
    t2i = side(n_txt, n_img, txt2img)
    txt2img = txt2img.tolist()
    img2txt = [[] for _ in range(n_img)]
    for t, i in enumerate(txt2img):
        img2txt[i].append(t)
    return i2t, t2i, txt2img, img2txt


def dense_route(i2t, t2i, n_img, n_txt, txt2img, img2txt):
    mats = []
    for (idx, val), shape in ((i2t, (n_img, n_txt)), (t2i, (n_txt, n_img))):
        m = torch.full(shape, -100.0, device=idx.device)
        m.scatter_(1, idx, val)
        mats.append(m)
    a, b = mats[0].cpu().numpy(), mats[1].cpu().numpy()
    del mats
    return re.itm_eval(a, b, txt2img, img2txt)


def lists_route(i2t, t2i, n_img, n_txt, txt2img, img2txt):
    out = []
    for (idx, val), nk in ((i2t, n_txt), (t2i, n_img)):
        v = torch.full(val.shape, -100.0, device=val.device)
        v.copy_(val)
        out.append(CandidateLists(idx, v, nk))
    return re.itm_eval(out[0], out[1], txt2img, img2txt)


def clocked(fn, n):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


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


def kernel_calls(cl, ptr, tgt):
    """-> (rank, sort): the two entry points on preallocated outputs, nothing else between the events"""
    n, k = cl.shape
    rank_row = torch.empty(n, dtype=torch.int32, device=cl.device)
    rank_tgt = torch.empty(tgt.numel(), dtype=torch.int32, device=cl.device)
    out_idx, out_val = torch.empty_like(cl.idx), torch.empty_like(cl.val)
    h, stream = lists.lib(), hip._stream()

    def rank():
        hip._check(h.madtp_lists_rank(cl.idx.data_ptr(), k, cl.val.data_ptr(), k, n, k, cl.nk, cl.fill, ptr.data_ptr(), tgt.data_ptr(),
                                      rank_row.data_ptr(), rank_tgt.data_ptr(), stream), "madtp_lists_rank")

    def sort():
        hip._check(h.madtp_lists_sort(cl.idx.data_ptr(), k, cl.val.data_ptr(), k, n, k, cl.nk, out_idx.data_ptr(), out_val.data_ptr(),
                                      stream), "madtp_lists_sort")
    return rank, sort


def summary(v, unit=1e3, name="ms"):
    return f"{statistics.median(v) * unit:10.3f} {name} (min {min(v) * unit:.3f}, max {max(v) * unit:.3f})"


def case(n_img, n_txt, k, a, dev, out):
    i2t, t2i, txt2img, img2txt = synthetic(n_img, n_txt, k, dev)
    args = (i2t, t2i, n_img, n_txt, txt2img, img2txt)
    li, lt = CandidateLists(*i2t, n_txt).validate(), CandidateLists(*t2i, n_img).validate()
    targets = re.target_lists(txt2img, img2txt, n_img, n_txt, device=dev)
    (rank_i, sort_i), (rank_t, sort_t) = kernel_calls(li, targets.i2t_ptr, targets.i2t_idx), kernel_calls(lt, targets.t2i_ptr, targets.t2i_idx)
    got_b = lists_route(*args)
    got_a = dense_route(*args)
    same = got_a == got_b
    per = {"A": [], "B": [], "T": [], "R": [], "S": []}
    for _ in range(a.rounds):
        per["A"].append(clocked(lambda: dense_route(*args), 1))
        per["B"].append(clocked(lambda: lists_route(*args), a.iters))
        per["T"].append(clocked(lambda: re.target_lists(txt2img, img2txt, n_img, n_txt, device=dev), a.iters))
        per["R"].append(events(lambda: (rank_i(), rank_t()), a.iters))
        per["S"].append(events(lambda: (sort_i(), sort_t()), a.iters))
    mem_a, mem_b = peak_above_inputs(lambda: dense_route(*args)), peak_above_inputs(lambda: lists_route(*args))
    slots = (n_img + n_txt) * k
    rank_bytes = 12.0 * slots + 4.0 * (2 * (n_img + n_txt) + 2 + 2 * len(txt2img)) + 4.0 * (n_img + n_txt + 2 * len(txt2img))
    sort_bytes = 24.0 * slots
    r, s = statistics.median(per["R"]), statistics.median(per["S"])
    ratio = statistics.median(per["A"]) / statistics.median(per["B"])
    lines = [f"n_img {n_img} n_txt {n_txt} k_test {k}: dicts {'equal' if same else 'DIFFER'}  R@1 i2t {got_b['txt_r1']:.2f} t2i {got_b['img_r1']:.2f}",
             f"  leg A dense matrices  {summary(per['A'])}",
             f"  leg B candidate lists {summary(per['B'])}   A / B = {ratio:.1f}x{'' if ratio > 1 else '   LOSES'}",
             f"    of which target_lists (both legs) {summary(per['T'])}",
             f"  peak memory above the inputs: leg A {mem_a / 1e6:.1f} MB, leg B {mem_b / 1e6:.1f} MB "
             f"(the lists themselves: {li.nbytes / 1e6 + lt.nbytes / 1e6:.1f} MB; one dense matrix: {4.0 * n_img * n_txt / 1e6:.1f} MB)",
             f"  madtp_lists_rank x 2, device events {summary(per['R'], 1e6, 'us')}",
             f"    {rank_bytes / 1e6:.1f} MB read and written = {100 * rank_bytes / r / HBM_PEAK:.2f} % of HBM peak ({HBM_PEAK / 1e12:.0f} TB/s)",
             f"  madtp_lists_sort x 2, device events {summary(per['S'], 1e6, 'us')}",
             f"    {sort_bytes / 1e6:.1f} MB read and written = {100 * sort_bytes / s / HBM_PEAK:.2f} % of HBM peak"]
    for line in lines:
        print(line, flush=True)
        out.append(line)
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-img", type=int, default=0)
    ap.add_argument("--n-txt", type=int, default=0)
    ap.add_argument("--k-test", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lists_ab: needs the GPU (a CPU run measures nothing)")
    hip.load()
    sizes = [(a.n_img, a.n_txt, a.k_test)] if a.n_img and a.n_txt and a.k_test else [(5000, 25010, 256), (1000, 5000, 128)]
    out = [f"tools/lists_ab.py on {torch.cuda.get_device_name(0)}: {a.rounds} alternating rounds, leg B and the events {a.iters} calls "
           "per round, medians of per-round medians"]
    ok = True
    for n_img, n_txt, k in sizes:
        ok &= case(n_img, n_txt, k, a, "cuda", out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    if not ok:
        raise SystemExit("lists_ab: the two legs returned different metrics")


if __name__ == "__main__":
    main()

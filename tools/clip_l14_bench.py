#!/usr/bin/env python
"""CLIP ViT-L/14@336 (the model of the reference's configs/retrieval_{coco,flickr}_clip.yaml) at the driver's evaluation batch:
encode_image + encode_text of B = 32 image-text pairs, serial, in each precision mode asked for.

The temperature is the p = 0.5 one that the driver's initial search (controller.calculate_temperature, the retrieval_clip ladder)
finds with Cur_Gflops measured on this forward (f16x3 mode; the figures are rescaled so that the driver's absolute tolerances mean the
same thing, as tests/test_workloads_gpu.py does).  Times are medians of per-forward wall intervals (synchronised) after warm-up.

    python tools/clip_l14_bench.py --modes bf16 f16x3 --steps 20 --warmup 3 [--out result.json]
    python tools/clip_l14_bench.py --gemm-frac results.db --result run.json   (rocprofv3 --kernel-trace database of a bf16 run:
        the big GEMMs' share of the 2.5 PF bf16 MFMA peak over the forwards after the first)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, SIZE = 32, 336
BF16_PEAK = 2.5e15  # MI355X dense bf16 MFMA, FLOP/s


def big_gemm_flops(w, lens):
    """qkv / proj / fc1 / fc2 FLOPs (2 x MAC) of one forward (both towers) at the per-layer token counts lens"""
    f = 0
    for key, n0, width in (("vit", (w.size // w.patch) ** 2 + 1, w.width), ("text", w.ctx, w.text_width)):
        n = n0
        for n_out in lens[key]:
            f += 2 * (4 * n * width * width + 8 * n_out * width * width)
            n = n_out
    return B * f


def find_temperature(w, model, inp):
    from madtp_amd import controller as C, runtime
    full = C.workload_gflops(w, None)
    target = full * (1 - w.p)
    scale = C.ORI_GFLOPS["retrieval_clip"] / full

    def measure(T):
        if T <= 0:
            return full * scale
        with runtime.precision("f16x3"), torch.no_grad():
            w.step(model, inp, T)
        return C.workload_gflops(w, w.lens(model)) * scale

    cur, T = C.calculate_temperature(measure, full * scale, target * scale, "retrieval_clip", max_iters=400)
    return T, cur / scale, full


def run(args):
    from madtp_amd import build, hip, runtime, workloads
    build.build(verbose=False)
    hip.load()
    w = workloads.Clip(arch="ViT-L/14", size=SIZE)
    model = w.build("cuda")
    inp = w.inputs(B, 0)
    images, text = inp
    if args.T is None:
        T, cur, search_full = find_temperature(w, model, inp)
    else:
        T, cur, search_full = args.T, None, None
    full = w.flops(None) / 1e9
    res = {"model": "CLIP ViT-L/14@336", "B": B, "p": w.p, "temperature": T, "unpruned_gflops_per_pair": full,
           "unpruned_gmac_per_pair": full / 2, "driver_ori_gflops_half": 395.7 / 2, "modes": {}}
    print(f"unpruned: {full:.1f} GFLOP = {full / 2:.1f} G MAC per image-text pair (the driver's Ori_Gflops 395.7 / 2 = "
          f"{395.7 / 2:.2f}: fvcore counts one flop per MAC and also the momentum towers)")
    if cur is not None:  # (controller.workload_gflops counts MACs, as fvcore does)
        res["search_gmac_per_pair"], res["search_target_gmac_per_pair"] = cur, search_full * (1 - w.p)
    print(f"temperature for p = {w.p}: T = {T:.4f}" +
          (f" (search: {cur:.1f} G MAC per pair vs target {search_full * (1 - w.p):.1f})" if cur is not None else ""))
    for mode in args.modes:
        with runtime.precision(mode), torch.no_grad():
            def fwd():
                model.encode_image(images, model.space_dict, T)
                model.encode_text(text, model.space_dict, T)
            for _ in range(args.warmup):
                fwd()
            torch.cuda.synchronize()
            times = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                fwd()
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
        lens = w.lens(model)
        ms = 1e3 * statistics.median(times)
        gflops = w.flops(lens) / 1e9
        r = {"ms_per_forward": ms, "ms_min": 1e3 * min(times), "ms_max": 1e3 * max(times), "images_per_s": B / (ms / 1e3),
             "gflops_per_pair": gflops, "vit_lens": lens["vit"], "text_lens": lens["text"],
             "big_gemm_flops_per_forward": big_gemm_flops(w, lens)}
        res["modes"][mode] = r
        print(f"{mode}: {ms:.2f} ms per forward (min {r['ms_min']:.2f}, max {r['ms_max']:.2f}), {r['images_per_s']:.1f} images/s, "
              f"{gflops:.1f} GFLOP per pair; vision tokens {lens['vit']}")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "modes"}))


def gemm_frac(args):
    """big-GEMM fraction of bf16 peak from a kernel trace: FLOPs of the qkv / proj / fc1 / fc2 GEMMs of the traced forwards (token
    counts from the bench result) / the time of every GEMM kernel after the first forward (which also prepares the weights)"""
    import sqlite3
    res = json.load(open(args.result))
    r = res["modes"]["bf16"]
    c = sqlite3.connect(args.gemm_frac)
    starts = [s for (s,) in c.execute("select start from kernels where name like '%patchify%' order by start")]
    t0 = starts[1]
    n_fwd = len(starts) - 1
    rows = c.execute("select name, count(*), sum(end-start) from kernels where start >= ? and name like '%gemm%' group by name "
                     "order by 3 desc", (t0,)).fetchall()
    t_gemm = sum(x[2] for x in rows) * 1e-9
    frac = r["big_gemm_flops_per_forward"] * n_fwd / t_gemm / BF16_PEAK
    print(f"# {n_fwd} bf16 forwards after the first: GEMM kernels {1e3 * t_gemm / n_fwd:.2f} ms per forward, big-GEMM FLOPs "
          f"{r['big_gemm_flops_per_forward'] / 1e12:.3f} T per forward -> {frac:.3f} of {BF16_PEAK / 1e15:.1f} PF")
    for name, calls, ns in rows:
        print(f"{name[:100]:100s} {calls:6d} {ns / 1e6 / n_fwd:9.3f} ms/forward")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", nargs="+", default=["bf16", "f16x3"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--T", type=float, default=None, help="temperature (default: the p = 0.5 search)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--gemm-frac", default=None, help="rocprofv3 kernel-trace database of a bf16 run")
    ap.add_argument("--result", default=None, help="(with --gemm-frac) the JSON this tool wrote for that run")
    a = ap.parse_args()
    gemm_frac(a) if a.gemm_frac else run(a)

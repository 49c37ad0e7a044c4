#!/usr/bin/env python
"""A/B of the optimizer step: madtp_amd.optim.AdamW (one madtp_adamw_step launch, csrc/optim.hip) against the two torch
implementations, on the parameter sets the drivers train: BLIP_NLVR (built as in tools/train_step_bench.py) and CLIP ViT-B/16 and
ViT-L/14@336 (built as in tools/clip_train_bench.py), with random gradients.

    python tools/adamw_ab.py [--iters N] [--rounds R] [--sets nlvr,clip_b16,clip_l14] [--out profiles/adamw_ab.txt]

  foreach: torch.optim.AdamW(...) with its defaults - the foreach implementation on a GPU, what the drivers run today;
  fused:   torch.optim.AdamW(..., fused=True);
  madtp:   madtp_amd.optim.AdamW (its per-step pointer check included).
Every leg owns its exp_avg / exp_avg_sq and steps the same parameters with the same gradients (lr 1e-6: the values stay put).  A
leg's time is the device-event interval around step() alone; the legs alternate inside every round (shared machine: a drift hits
all three); each figure is the median over the rounds of the per-round medians, with the min and max of those.  Bytes: p, g, m, v
read and p, m, v written = 28 B per element, over the measured time, against the 8 TB/s HBM peak of the MI355X."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from madtp_amd import harness, hip, optim, specs  # noqa: E402
from madtp_amd.clip_model import CLIP  # noqa: E402

HBM = 8.0e12
CLIP_ARCHS = {"clip_b16": dict(D=512, size=224, patch=16, vision_width=768, vision_layers=12, embed_dim=512),
              "clip_l14": dict(D=768, size=336, patch=14, vision_width=1024, vision_layers=24, embed_dim=768)}


def parameter_set(name, dev):
    """-> detached GPU copies of the tensors the driver hands its optimizer"""
    if name == "nlvr":
        model = harness.build_nlvr(224, 0, dev)
        ps = list(model.parameters())
    else:
        a = CLIP_ARCHS[name]
        L, V, D = 77, 49408, a["D"]
        with torch.no_grad():
            model = CLIP(a["embed_dim"], a["size"], a["vision_layers"], a["vision_width"], a["patch"], L, V, D, D // 64, 12, False, None,
                         queue_size=57600)
            model.load_state_dict(specs.synth_weights(specs.clip_shapes(a["size"], a["patch"], a["vision_width"], a["vision_layers"],
                                                                        a["embed_dim"], D, 12), 0), strict=False)
            model.copy_params()
            model = model.to(dev)
        ps = [p for p in model.parameters() if p.requires_grad]
    out = [p.detach().clone().requires_grad_(True) for p in ps]
    del model, ps
    torch.cuda.empty_cache()
    return out


def _median_us(fn, iters):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def ab(fns, iters, rounds, warm=3):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            per[k].append(_median_us(fn, iters))
    return {k: {"us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sets", default="nlvr,clip_b16,clip_l14")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adamw_ab: needs the GPU (a CPU run measures nothing)")
    hip.load()
    dev = "cuda"
    lines = [f"# tools/adamw_ab.py --iters {a.iters} --rounds {a.rounds} on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             "# optimizer.step() alone, device events; median over the rounds of the per-round medians [min .. max of those]; "
             "28 B per element against 8 TB/s"]
    for name in a.sets.split(","):
        ps = parameter_set(name, dev)
        g = torch.Generator(device=dev).manual_seed(0)
        for p in ps:
            p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
        numel = sum(p.numel() for p in ps)
        hp = dict(lr=1e-6, weight_decay=0.05)
        opts = {"foreach": torch.optim.AdamW(ps, **hp), "fused": torch.optim.AdamW(ps, fused=True, **hp), "madtp": optim.AdamW(ps, **hp)}
        r = ab({k: o.step for k, o in opts.items()}, a.iters, a.rounds)
        nbytes = 28 * numel
        lines.append(f"{name}: {len(ps)} tensors, {numel / 1e6:.1f} M elements, {nbytes / 1e9:.2f} GB per step")
        for k, v in r.items():
            lines.append(f"  {k:8s} {v['us'] / 1e3:8.3f} ms [{v['min_us'] / 1e3:.3f} .. {v['max_us'] / 1e3:.3f}]   "
                         f"{nbytes / (v['us'] * 1e-6) / 1e12:5.2f} TB/s = {nbytes / (v['us'] * 1e-6) / HBM:5.1%} of HBM peak")
        lines.append(f"  madtp vs foreach {r['foreach']['us'] / r['madtp']['us']:.2f}x, vs fused {r['fused']['us'] / r['madtp']['us']:.2f}x; "
                     f"pointer-table uploads {opts['madtp'].tables()[0].rebuilds}")
        print("\n".join(lines[-5:]), flush=True)
        del opts, ps
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""CLIP's training step and its two embedding kernels (csrc/clip.hip) at the shape of configs/retrieval_coco_clip.yaml's loop
on the ViT-B/16 checkpoint geometry: B = 16, 224^2, text 77 x 512, vocabulary 49408, Q = 57 600, one GPU.

    python tools/clip_train_bench.py [--iters N] [--rounds R] [--out profiles/clip_train_step.json] [--no-step] [--arch B16|L14]

  embed_grad: madtp_embedding_grad (rank + ordered segmented sum, every row of the [49408, 512] gradient written once)  vs  the
              composition it replaces, torch.zeros_like(table).index_add_(0, ids, dx) (a 101 MB memset and atomic adds);
  embed:      madtp_clip_embed  vs  (table[ids] + pos).float().contiguous()  (clip/model.py:486-488);
  step:       one forward + backward of CLIP.forward (evaluate=False) in f16x3 and fp32 (no earlier version to compare with).
              MADTP_TRAIN_OPT=torch | fused | madtp adds the optimizer step of the driver's loop to it (AdamW, lr 1e-6, weight decay
              0.05: torch's foreach default, torch's fused=True, madtp_amd.optim.AdamW); unset: no optimizer step, as recorded so far.
The two sides of each pair alternate inside every round (shared machine: a drift hits both); each side's figure is the median over
the rounds of its per-round median of device-event intervals, reported with the min and max of those per-round medians.  Captions
are CLIP-shaped: SOT, 6 .. 40 words, EOT, zero padding (synth.synth_clip_tokens), so about 49 of 77 positions share id 0.
Bytes: the algorithm's own (read ids and dx once, write the gradient once), over the measured time, against 8 TB/s.
--arch L14: the geometry the reference's two CLIP configs train (clip_large_retrieval_*.pth, ViT-L/14@336): vision width 1024 /
24 layers / patch 14 at 336^2, text 77 x 768 / 12 layers, embed_dim 768; B = 16, Q = 57 600.  Default out:
profiles/clip_l14_train_step.json."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from madtp_amd import hip, runtime, specs, synth  # noqa: E402
from madtp_amd.clip_model import CLIP  # noqa: E402

HBM = 8.0e12
# text width (= table width D), image size, patch, vision width, vision layers, embed_dim
ARCHS = {"B16": dict(D=512, size=224, patch=16, vision_width=768, vision_layers=12, embed_dim=512),
         "L14": dict(D=768, size=336, patch=14, vision_width=1024, vision_layers=24, embed_dim=768)}


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


def ab(fns, iters, rounds, warm=5):
    """{name: fn} -> {name: {"us": median of the per-round medians, "min_us", "max_us"}}; the sides alternate within a round"""
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--arch", choices=sorted(ARCHS), default="B16")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "clip_train_step.json" if a.arch == "B16" else "clip_l14_train_step.json")
    arch = ARCHS[a.arch]
    if not torch.cuda.is_available():
        raise SystemExit("clip_train_bench: needs the GPU (a CPU run measures nothing)")
    hip.load()
    dev = "cuda"
    B, L, D, V, Q, size = 16, 77, arch["D"], 49408, 57600, arch["size"]
    res = {"arch": a.arch, "B": B, "L": L, "D": D, "embed_dim": arch["embed_dim"], "V": V, "Q": Q, "image": size, "iters": a.iters,
           "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    text = synth.synth_clip_tokens(B, L, 0).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn(V, D, device=dev, generator=g) * 0.02
    pos = torch.randn(L, D, device=dev, generator=g) * 0.01
    dx = torch.randn(B * L, D, device=dev, generator=g)
    ids = text.view(-1)
    res["zero_id_share"] = float((ids == 0).float().mean())

    out = torch.empty(V, D, device=dev)
    ref = torch.zeros_like(table).index_add_(0, ids, dx)
    got = hip.embedding_grad(ids, dx, V, out=out)
    res["embed_grad_max_abs_diff_vs_torch"] = float((got - ref).abs().max())
    assert torch.equal(hip.clip_embed(text, table, pos), (table[text] + pos).float().contiguous())

    r = ab({"hip": lambda: hip.embedding_grad(ids, dx, V, out=out),
            "torch": lambda: torch.zeros_like(table).index_add_(0, ids, dx)}, a.iters, a.rounds)
    res["embed_grad_hip"], res["embed_grad_torch"] = r["hip"], r["torch"]
    grad_bytes = V * D * 4 + B * L * (D * 4 + 8)
    res["embed_grad_bytes"] = grad_bytes
    res["embed_grad_hbm_fraction"] = grad_bytes / (r["hip"]["us"] * 1e-6) / HBM
    r = ab({"hip": lambda: hip.clip_embed(text, table, pos),
            "torch": lambda: (table[text] + pos).float().contiguous()}, a.iters, a.rounds)
    res["embed_hip"], res["embed_torch"] = r["hip"], r["torch"]

    if not a.no_step:
        with torch.no_grad():
            model = CLIP(arch["embed_dim"], size, arch["vision_layers"], arch["vision_width"], arch["patch"], L, V, D, D // 64, 12,
                         False, None, queue_size=Q)
            model.load_state_dict(specs.synth_weights(specs.clip_shapes(size, arch["patch"], arch["vision_width"], arch["vision_layers"],
                                                                        arch["embed_dim"], D, 12), 0), strict=False)
            model.copy_params()
            model = model.to(dev).eval()
        images = synth.synth_images(B, size, 0, device=dev)
        idx = torch.arange(B, device=dev)

        which = os.environ.get("MADTP_TRAIN_OPT", "")
        opt = None
        if which:
            from madtp_amd import optim
            params = [p for p in model.parameters() if p.requires_grad]
            opt = (optim.AdamW(params, lr=1e-6, weight_decay=0.05) if which == "madtp" else
                   torch.optim.AdamW(params, lr=1e-6, weight_decay=0.05, **({"fused": True} if which == "fused" else {})))
            res["step_optimizer"] = which

        def step(mode):
            model.zero_grad(set_to_none=True)
            with runtime.precision(mode), runtime.training_f16x3(mode == "f16x3"):
                ls = model(images, text, 0.4, idx, temperature=4.0)
                (ls[0] + 0.1 * ls[1] + 0.1 * ls[2]).backward()
            if opt is not None:
                opt.step()

        r = ab({"f16x3": lambda: step("f16x3"), "fp32": lambda: step("fp32")}, 3, max(3, a.rounds), warm=2)
        res["step_temperature"] = 4.0
        for k, v in r.items():
            res[f"step_{k}_ms"] = {kk.replace("us", "ms"): vv / 1e3 for kk, vv in v.items()}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

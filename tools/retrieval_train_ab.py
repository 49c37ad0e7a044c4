#!/usr/bin/env python
"""A/B of the retrieval training step's new kernels (csrc/retrieval.hip) against the eager torch composition they replace, at
the config shape (B = 32, D = 256, Q = 57 600, ViT-B at 384^2), on one GPU, plus the time of a whole training step.

    python tools/retrieval_train_ab.py [--iters N] [--out FILE.json] [--no-step] [--dim D]

  itc: both directions of madtp_itc_loss (forward + gradient)  vs  cat(feat.T, queue.clone()), the four [B, B+Q] similarity
       matrices, softmaxes, log_softmax loss and its autograd backward (blip_retrieval.py:116-150);
  ema: madtp_ema_update over every momentum pair (ema_hip_us: EmaTable.update with its per-step pointer check; ema_kernel_us:
       the launch alone)  vs  the per-tensor `p_m.data = p_m.data * m + p.data * (1 - m)` loop (:296-300);
  neg: madtp_itm_negatives  vs  the softmax / masked_fill / 2 B torch.multinomial(...).item() loop (:240-258).
Times are medians of CUDA-event intervals after warm-up.  HBM fraction: bytes moved / time / 8 TB/s (MI355X peak).
--dim D (default 256, BLIP's embed_dim): any other D runs the itc leg alone, at (B 16, Q 57 600) and (B 32, Q 57 600) - CLIP
ViT-L/14 trains at D = 768, B = 16 - with the two sides alternating inside every round; each figure is the median over the rounds
of its per-round median, with the min and max of those.  The other legs are BLIP's and stay at D = 256."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from madtp_amd import harness, hip, runtime, synth  # noqa: E402
from madtp_amd.blip_retrieval import BLIP_Retrieval  # noqa: E402

HBM = 8.0e12


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def ab(fns, iters, rounds=5, warm=5):
    """{name: fn} -> {name: {"us": median of the per-round medians, "min_us", "max_us"}}; the sides alternate within a round"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            per[k].append(timed(fn, iters, warm=0))
    return {k: {"us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in per.items()}


def itc_sides(B, D, Q, dev):
    """-> (itc_hip, itc_torch, (img, txt, idx, temp)): both directions of the loss with its gradient, on seeded unit-norm features"""
    g = torch.Generator(device=dev).manual_seed(0)
    f = lambda n: F.normalize(torch.randn(n, D, device=dev, generator=g), dim=-1)  # noqa: E731
    img, txt, img_m, txt_m = f(B), f(B), f(B), f(B)
    iq, tq = f(Q).t().contiguous(), f(Q).t().contiguous()
    idx = torch.arange(B, device=dev)
    idxq = torch.full((Q,), -100, dtype=torch.long, device=dev)
    temp = torch.tensor([0.07], device=dev)

    def itc_hip():
        hip.itc_loss(img, img_m, txt_m, tq, idx, idxq, temp, 0.4)
        hip.itc_loss(txt, txt_m, img_m, iq, idx, idxq, temp, 0.4)

    tp = torch.nn.Parameter(temp.clone().reshape(()))
    img_p, txt_p = img.clone().requires_grad_(True), txt.clone().requires_grad_(True)

    def itc_torch():
        idx_all = torch.cat([idx.view(1, -1), idxq.view(1, -1)], 1)
        pos = torch.eq(idx.view(-1, 1), idx_all).float()
        tgt = pos / pos.sum(1, keepdim=True)
        with torch.no_grad():
            ia = torch.cat([img_m.t(), iq.clone()], 1)
            ta = torch.cat([txt_m.t(), tq.clone()], 1)
            ti = 0.4 * F.softmax(img_m @ ta / tp, 1) + 0.6 * tgt
            tt = 0.4 * F.softmax(txt_m @ ia / tp, 1) + 0.6 * tgt
        li = -torch.sum(F.log_softmax(img_p @ ta / tp, 1) * ti, 1).mean()
        lt = -torch.sum(F.log_softmax(txt_p @ ia / tp, 1) * tt, 1).mean()
        ((li + lt) / 2).backward()

    return itc_hip, itc_torch, (img, txt, idx, temp)


def itc_only(a, dev):
    Q = 57600
    res = {"D": a.dim, "Q": Q, "iters": a.iters, "rounds": 5, "device": torch.cuda.get_device_name(0), "itc": []}
    for B in (16, 32):
        itc_hip, itc_torch, _ = itc_sides(B, a.dim, Q, dev)
        r = ab({"hip": itc_hip, "torch": itc_torch}, a.iters)
        res["itc"].append({"B": B, "hip": r["hip"], "torch": r["torch"], "bank_bytes": 4 * a.dim * Q * 4,
                           "hbm_fraction": 4 * a.dim * Q * 4 / (r["hip"]["us"] * 1e-6) / HBM})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--dim", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_train_ab: needs the GPU (a CPU run measures nothing)")
    hip.load()
    dev = "cuda"
    if a.dim != 256:
        res = itc_only(a, dev)
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(res, fh, indent=1)
        return
    B, D, Q = 32, 256, 57600
    res = {"B": B, "D": D, "Q": Q}
    itc_hip, itc_torch, (img, txt, idx, temp) = itc_sides(B, D, Q, dev)

    res["itc_hip_us"] = timed(itc_hip, a.iters)
    res["itc_torch_us"] = timed(itc_torch, a.iters)
    itc_bytes = 4 * D * Q * 4  # two passes over each of the two banks
    res["itc_bank_bytes"] = itc_bytes
    res["itc_hbm_fraction"] = itc_bytes / (res["itc_hip_us"] * 1e-6) / HBM

    with torch.no_grad():
        model = BLIP_Retrieval(image_size=384, queue_size=Q, evaluate=False).to(dev)
    pairs = [(pm, p) for p, pm in model.momentum_pairs()]
    n_par = sum(p.numel() for p, _ in pairs)
    res["ema_params"] = n_par
    ema = hip.EmaTable()

    def ema_torch():
        for pm, p in pairs:
            pm.data = pm.data * model.momentum + p.data * (1. - model.momentum)

    res["ema_hip_us"] = timed(lambda: ema.update(pairs, model.momentum), a.iters)  # EmaTable.update: pointer check + launch
    res["ema_kernel_us"] = timed(ema.launch_only, a.iters)                           # the launch alone
    res["ema_torch_us"] = timed(ema_torch, max(3, a.iters // 4))
    res["ema_hbm_fraction"] = 12 * n_par / (res["ema_hip_us"] * 1e-6) / HBM
    res["ema_kernel_hbm_fraction"] = 12 * n_par / (res["ema_kernel_us"] * 1e-6) / HBM
    res["ema_torch_launches"] = 2 * 2 * len(pairs) + len(pairs)

    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    u = torch.rand(2, B, device=dev)
    res["neg_hip_us"] = timed(lambda: hip.itm_negatives(img, txt, img, txt, idx, idx, temp, u, flag), a.iters)

    def neg_torch():
        with torch.no_grad():
            mask = torch.eq(idx.view(-1, 1), idx.view(1, -1))
            wi = F.softmax(img @ txt.t() / temp, 1).masked_fill_(mask, 0)
            wt = F.softmax(txt @ img.t() / temp, 1).masked_fill_(mask, 0)
        return [torch.multinomial(wt[b], 1).item() for b in range(B)] + [torch.multinomial(wi[b], 1).item() for b in range(B)]

    res["neg_torch_us"] = timed(neg_torch, a.iters)

    if not a.no_step:
        model.train()
        images = synth.synth_images(B, 384, 0, device=dev)
        cap = {"input_ids": synth.synth_token_ids(B, 35, 0, first_id=101).to(dev), "attention_mask": harness.padded_mask(B, 35, 5).to(dev)}
        for mode in ("f16x3", "fp32"):
            def step():
                model.zero_grad(set_to_none=True)
                with runtime.precision(mode):
                    cm = runtime.training_f16x3() if mode == "f16x3" else None
                    if cm:
                        cm.__enter__()
                    ls = model(images, cap, 0.4, idx, temperature=1.0)
                    (ls[0] + ls[1] + 0.1 * ls[2] + 0.1 * ls[3]).backward()
                    if cm:
                        cm.__exit__(None, None, None)
            res[f"step_{mode}_ms"] = timed(step, 3, warm=1) / 1e3
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

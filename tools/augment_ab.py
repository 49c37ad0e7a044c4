"""What the augmentation stages add to the image pipeline, on seeded random images (no dataset).

    python tools/augment_ab.py [--out profiles/augment_ab.txt] [--rounds 5] [--batches 12]

  leg P  preprocess.ImagePipeline on the batch with the same crop boxes and flips: pack, uint8 copy, one kernel (resize + normalise)
  leg T  augment.TrainTransform on the same batch, boxes and flips plus the drawn ops (N = 2, M = 5, the reference's ten names):
         pack, uint8 copy, plan copy, resize to bytes, up to two histogram and two apply launches
  leg D  leg T with the draws (boxes, flips, ops) made inside the call, as a loader uses it
Per-batch time = median of an epoch's calls, each ended by a stream synchronise; five alternating rounds; reported: the median of
the per-round medians and their range.  In a run of their own afterwards: every launch of leg T alone, device events around 40
repeats, and its share of the HBM peak over the bytes it must move.  The reference's own route (torchvision's RandomResizedCrop
and OpenCV's warps in loader workers) needs two packages this project's environment does not have: it is NOT measured here."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from madtp_amd import augment, hip, preprocess  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s
SHAPES = [(640, 480), (480, 640)]
CASES = [(32, 384), (128, 384), (32, 224), (128, 224)]  # (B, S)


def images_of(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(SHAPES[i % 2][1], SHAPES[i % 2][0], 3), dtype=np.uint8) for i in range(n)]


def epoch(call, batches):
    times = []
    for _ in range(batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def spread(v):
    return f"{statistics.median(v) * 1e3:8.3f} ms  (rounds {min(v) * 1e3:.3f} .. {max(v) * 1e3:.3f})"


def launch_times(tf, images, plan, reps=40):
    """[(entry point, stage ops, median ms, min, max, bytes it must move)] of one call's launches, each timed alone"""
    rows, tables, masks = augment.build_plan(plan["ops"], tf.Sh, tf.Sw)
    batch = tf.pipe.prepare(images, plan["boxes"], plan["flips"])
    out, launches, keep = tf.launches(batch, rows, tables, masks)
    stream = torch.cuda.current_stream().cuda_stream
    for name, _, launch in launches:  # once in order: every launch then has its real input
        hip._check(launch(stream), name)
    B, plane = batch.B, tf.Sh * tf.Sw
    src = sum(int((b[2] - b[0]) * (b[3] - b[1]) * 3) for b in plan["boxes"])
    result = []
    for name, stage, launch in launches:
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            hip._check(launch(stream), name)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        if name.endswith("resize_u8"):
            what, moved = "crop + resize + flip -> bytes", src + 3 * plane * B
        else:
            ops = rows[stage, :, 0]
            need = int(np.isin(ops, (augment.OP_EQUALIZE, augment.OP_AUTOCONTRAST)).sum())
            if name.endswith("stats"):
                what, moved = f"stage {stage}: histograms of {need} of {B} images", 3 * plane * need + 3 * 256 * need
            else:
                last = stage == rows.shape[0] - 1
                what = f"stage {stage}: {int((ops == augment.OP_WARP).sum())} warps, {need + int((ops == augment.OP_TABLE).sum())} tables, " \
                       f"{int((ops == augment.OP_COPY).sum())} copies -> {'f32' if last else 'bytes'}"
                moved = 3 * plane * B + (12 if last else 3) * plane * B
        result.append((name, stage, what, statistics.median(ms), min(ms), max(ms), moved))
    del keep
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_ab: no GPU - nothing is measured here")
    device = torch.device("cuda", 0)
    lines = [f"training transform A/B, {args.rounds} alternating rounds of {args.batches} batches; {torch.cuda.get_device_name(0)}; sources "
             f"640x480 / 480x640 alternating, seeded; N = 2, M = 5, the reference's ten ops; the reference's own route is not measured "
             f"(torchvision and OpenCV are not installed)"]
    for B, S in CASES:
        images = images_of(B, 7)
        pipe = preprocess.ImagePipeline(S, device=device)
        tf = augment.TrainTransform(S, device=device, seed=11)
        tf(images)  # one drawn call fixes the plan of legs P and T
        plan = tf.last_plan
        same = torch.equal(tf(images, **plan), tf(images, **plan))
        none = torch.equal(tf(images, boxes=plan["boxes"], flips=plan["flips"], ops=[[]] * B), pipe(images, plan["boxes"], plan["flips"]))
        mix = {}
        for calls in plan["ops"]:
            for name, _ in calls:
                mix[name] = mix.get(name, 0) + 1
        p, t, d = [], [], []
        for _ in range(args.rounds):
            p.append(epoch(lambda: pipe(images, plan["boxes"], plan["flips"]), args.batches))
            t.append(epoch(lambda: tf(images, **plan), args.batches))
            d.append(epoch(lambda: tf(images), args.batches))
        lines.append(f"\nB = {B} -> {S} x {S}; drawn ops: {', '.join(f'{k} {v}' for k, v in sorted(mix.items()))}; "
                     f"{sum(not c for c in plan['ops'])} images without an op; two identical calls equal: {same}; with no ops equal to leg P: {none}")
        lines.append(f"  leg P  ImagePipeline (resize + normalise)       {spread(p)} per batch   {B / statistics.median(p):9.0f} img/s")
        lines.append(f"  leg T  TrainTransform, the plan given          {spread(t)} per batch   {B / statistics.median(t):9.0f} img/s")
        lines.append(f"  leg D  TrainTransform, drawing                 {spread(d)} per batch   {B / statistics.median(d):9.0f} img/s")
        lines.append(f"  T - P  what the augmentation stages add        {(statistics.median(t) - statistics.median(p)) * 1e3:8.3f} ms   (T / P {statistics.median(t) / statistics.median(p):.2f})")
        total = 0.0
        for name, _, what, med, lo, hi, moved in launch_times(tf, images, plan):
            total += med
            lines.append(f"    {name:24s} {med:8.4f} ms  ({lo:.4f} .. {hi:.4f})  {what}; must move {moved / 1e6:.1f} MB -> "
                         f"{moved / (med * 1e-3) / 1e12:.2f} TB/s = {100 * moved / (med * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s peak")
        lines.append(f"    launches together        {total:8.4f} ms (device events, each timed alone over 40 repeats)")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""A/B of the image stage on seeded random images (no dataset): the reference's route against madtp_amd/preprocess.py.

    python tools/image_pipeline_ab.py [--out profiles/image_pipeline_ab.txt] [--rounds 5] [--batches 12]

  leg A  the reference's loader: PIL bicubic resize + torch-CPU ToTensor/Normalize in a DataLoader of 16 workers, default collate,
         then the f32 host-to-device copy.  Per-batch time = wall time of an epoch over its batches (the loader is a pipeline:
         single batches have no time of their own), workers already started.
  leg B  this path in the main process: packing into the pinned buffer, the uint8 copy, the kernel.  Per-batch time = median of
         the epoch's calls, each ended by a stream synchronise.
Five alternating rounds; reported: the median of the per-round figures and their range.  The kernel alone: device events around
ImagePipeline.run on a prepared batch, and its share of the HBM peak over the bytes it must move (source bytes in, 12 * Sh * Sw
per image out).  Without Pillow leg A is not run and the report says so; without a GPU nothing is measured."""
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

from madtp_amd import preprocess  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s
B = 32
# (name, [(w, h)] alternating through the batch, output size, mode)
CASES = [("640x480,480x640 -> 384", [(640, 480), (480, 640)], 384, "stretch"),
         ("640x480,480x640 -> 480", [(640, 480), (480, 640)], 480, "stretch"),
         ("500x375 -> 336 short side + crop", [(500, 375)], 336, "short_side_crop")]


def images_of(shapes, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(shapes[i % len(shapes)][1], shapes[i % len(shapes)][0], 3), dtype=np.uint8) for i in range(n)]


class ReferenceDataset(torch.utils.data.Dataset):
    """what data/__init__.py:29-33 / clip/clip.py:80-88 do to one decoded image, on PIL and torch CPU"""

    def __init__(self, shapes, size, mode, n):
        self.images, self.size, self.mode = images_of(shapes, B, 7), size, mode
        self.n = n
        self.mean = torch.as_tensor(preprocess.MEAN, dtype=torch.float32)[:, None, None]
        self.std = torch.as_tensor(preprocess.STD, dtype=torch.float32)[:, None, None]

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        from PIL import Image
        img = Image.fromarray(self.images[i % B], "RGB")
        S = self.size
        if self.mode == "stretch":
            img = img.resize((S, S), Image.BICUBIC)
        else:
            nw, nh, left, top = preprocess.short_side_geometry(img.size[0], img.size[1], S)
            img = img.resize((nw, nh), Image.BICUBIC).crop((left, top, left + S, top + S))
        t = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        return t.sub_(self.mean).div_(self.std)


def leg_a_epoch(loader, device):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for batch in loader:
        batch = batch.to(device, non_blocking=True)
        n += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, batch


def leg_b_epoch(pipe, images, batches):
    times = []
    for _ in range(batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe(images)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), out


def kernel_ms(pipe, images, reps=40):
    batch = pipe.prepare(images)
    out = pipe.run(batch)
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pipe.run(batch, out)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms), sum(int(i.nbytes) for i in images)


def spread(v):
    return f"{statistics.median(v) * 1e3:8.3f} ms  (rounds {min(v) * 1e3:.3f} .. {max(v) * 1e3:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--workers", type=int, default=16)
    args = ap.parse_args()
    try:
        import PIL
        pillow = PIL.__version__
    except ImportError:
        pillow = None
    if not torch.cuda.is_available():
        raise SystemExit("image_pipeline_ab: no GPU - nothing is measured here")
    device = torch.device("cuda", 0)
    lines = [f"image pipeline A/B, B = {B}, {args.rounds} alternating rounds of {args.batches} batches; {torch.cuda.get_device_name(0)}; "
             f"Pillow {pillow or 'absent: leg A not run'}; leg A workers {args.workers}"]
    for name, shapes, size, mode in CASES:
        images = images_of(shapes, B, 7)
        pipe = preprocess.ImagePipeline(size, mode, device=device)
        loader = None
        if pillow:
            ds = ReferenceDataset(shapes, size, mode, B * args.batches)
            loader = torch.utils.data.DataLoader(ds, batch_size=B, num_workers=args.workers, persistent_workers=True,
                                                 multiprocessing_context="spawn", pin_memory=True)
            _, ref = leg_a_epoch(loader, device)  # starts the workers
        _, got = leg_b_epoch(pipe, images, 3)
        same = "not compared" if loader is None else str(bool(torch.equal(ref, got)))
        a, b = [], []
        for _ in range(args.rounds):
            if loader is not None:
                a.append(leg_a_epoch(loader, device)[0])
            b.append(leg_b_epoch(pipe, images, args.batches)[0])
        med, lo, hi, src_bytes = kernel_ms(pipe, images)
        moved = src_bytes + 12 * size * size * B
        lines.append(f"\n{name}  ({mode}); leg B output torch.equal leg A output: {same}")
        if a:
            lines.append(f"  leg A  PIL + normalise in {args.workers} workers + f32 copy  {spread(a)} per batch   {B / statistics.median(a):9.0f} img/s")
        lines.append(f"  leg B  pack + uint8 copy + kernel                {spread(b)} per batch   {B / statistics.median(b):9.0f} img/s")
        if a:
            lines.append(f"  A / B  {statistics.median(a) / statistics.median(b):.2f}")
        lines.append(f"  kernel alone (device events, 40 launches)        {med:8.4f} ms  ({lo:.4f} .. {hi:.4f});  bytes it must move "
                     f"{moved / 1e6:.1f} MB = {src_bytes / 1e6:.1f} in + {12 * size * size * B / 1e6:.1f} out -> "
                     f"{moved / (med * 1e-3) / 1e12:.2f} TB/s = {100 * moved / (med * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM peak (the byte bound; "
                     f"the integer multiply-adds are far from the VALU's)")
        if loader is not None and loader._iterator is not None:
            loader._iterator._shutdown_workers()  # (persistent workers: stopped here rather than at interpreter exit)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

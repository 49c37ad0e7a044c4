"""A/B of the JPEG decode on seeded images that Pillow encoded (no dataset): the reference's route against madtp_amd/jpeg.py.

    python tools/jpeg_ab.py [--out profiles/jpeg_ab.txt] [--rounds 5] [--batches 8]

Sources: 640x480 / 480x640 alternating, smooth seeded content with noise (a photograph's bit rate, see the report's bytes per file),
quality 90, 4:2:0, B = 32.
  leg A  the reference's route: Image.open(BytesIO).convert("RGB") + np.asarray per image on T threads (Pillow releases the GIL in its
         decoder), then the existing ImagePipeline(384).
  leg B  JpegDecoder(workers=T) (entropy decode on T threads, one copy, two launches) + the same ImagePipeline.
Both at T = 1 and T = 8; per-batch time = median of a round's calls, each ended by a stream synchronise; five alternating rounds;
reported: the median of the per-round medians and their range.  Both legs' outputs must be torch.equal.  Separately: the host time per
image of entropy_decode against Pillow's full decode, one thread each, same process; the two kernels alone by device events with the
bytes they must move and their share of the HBM peak; registers / LDS / occupancy as the compiler reports them
(-Rpass-analysis=kernel-resource-usage; needs hipcc, else the line says so).  Needs Pillow and a GPU."""
import argparse
import concurrent.futures
import io
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from madtp_amd import build, jpeg, preprocess  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s
B = 32
SIZE = 384


def source(seed, w, h):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((h, w, 3))
    for c in range(3):
        a, b, p, q = rng.uniform(2.0, 9.0, 4)
        img[:, :, c] = 127.5 + 70.0 * np.sin(a * x / w + p) * np.cos(b * y / h + q) + 30.0 * np.sin((a + b) * (x + y) / (w + h) * 3.0)
    for _ in range(12):  # hard-edged patches
        x0, y0 = rng.randint(0, w - 40), rng.randint(0, h - 40)
        img[y0:y0 + rng.randint(8, 120), x0:x0 + rng.randint(8, 120)] += rng.uniform(-60, 60, 3)
    img += rng.normal(0.0, 6.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def files():
    from PIL import Image
    out = []
    for i in range(B):
        w, h = ((640, 480), (480, 640))[i % 2]
        buf = io.BytesIO()
        Image.fromarray(source(100 + i, w, h)).save(buf, "JPEG", quality=90, subsampling=2)
        out.append(buf.getvalue())
    return out


def pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def timed(fn, batches):
    times = []
    for _ in range(batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), out


def spread(v, unit=1e3, name="ms"):
    return f"{statistics.median(v) * unit:8.3f} {name}  (rounds {min(v) * unit:.3f} .. {max(v) * unit:.3f})"


def event_ms(launch, reps=40):
    stream = torch.cuda.current_stream().cuda_stream
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        code = launch(stream)
        b.record()
        b.synchronize()
        assert code == 0, code
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def resources():
    try:
        err = subprocess.run([build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                               os.path.join(build.CSRC, "jpeg.hip"), "-o", os.devnull],
                             capture_output=True, text=True, timeout=600).stderr
    except (OSError, subprocess.TimeoutExpired) as e:
        return [f"  compiler resource report not available ({e})"]
    rows, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: +(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = t.split(":", 1)[1].strip()
            rows[cur] = {}
        elif cur and ":" in t:
            k, v = t.rsplit(":", 1)
            rows[cur][k.strip()] = v.strip()
    return [f"  {('idct' if 'idct' in n else 'rgb'):5s} VGPRs {r.get('VGPRs')}  scratch {r.get('ScratchSize [bytes/lane]')} B/lane  "
            f"LDS {r.get('LDS Size [bytes/block]')} B/block  occupancy {r.get('Occupancy [waves/SIMD]')} waves/SIMD"
            for n, r in rows.items() if "jpeg" in n] or ["  compiler resource report not available (no remarks)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=8)
    args = ap.parse_args()
    try:
        import PIL
        from PIL import features
    except ImportError:
        raise SystemExit("jpeg_ab: Pillow is needed to encode the sources and to run leg A")
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_ab: no GPU - nothing is measured here")
    device = torch.device("cuda", 0)
    data = files()
    pipe = preprocess.ImagePipeline(SIZE, device=device)
    lines = [f"JPEG decode A/B, B = {B} files of 640x480 / 480x640, quality 90, 4:2:0, {sum(map(len, data)) / B / 1e3:.1f} kB per file; "
             f"{args.rounds} alternating rounds of {args.batches} batches; {torch.cuda.get_device_name(0)}; Pillow {PIL.__version__} "
             f"(jpg {features.version('jpg')}, libjpeg_turbo {features.check_feature('libjpeg_turbo')}); both legs end in ImagePipeline({SIZE})"]

    # the host stage alone, one thread, same process
    host_a, host_b = [], []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for d in data:
            pil_decode(d)
        host_a.append((time.perf_counter() - t0) / B)
        t0 = time.perf_counter()
        for d in data:
            jpeg.entropy_decode(d)
        host_b.append((time.perf_counter() - t0) / B)
    lines.append("\nhost time per image, one thread, same process")
    lines.append(f"  Pillow's whole decode (open + convert('RGB') + asarray)   {spread(host_a)}")
    lines.append(f"  entropy_decode (parse + Huffman, coefficients out)        {spread(host_b)}")
    lines.append(f"  entropy_decode / Pillow  {statistics.median(host_b) / statistics.median(host_a):.2f}")

    for threads in (1, 8):
        dec = jpeg.JpegDecoder(device, workers=threads)
        pool = concurrent.futures.ThreadPoolExecutor(threads) if threads > 1 else None
        decode_a = (lambda: list(pool.map(pil_decode, data))) if pool else (lambda: [pil_decode(d) for d in data])
        leg_a = lambda: pipe(decode_a())
        leg_b = lambda: pipe(dec(data))
        _, ref = timed(leg_a, 2)
        _, got = timed(leg_b, 2)
        same = bool(torch.equal(ref, got))
        a, b, da, db = [], [], [], []
        for _ in range(args.rounds):
            a.append(timed(leg_a, args.batches)[0])
            b.append(timed(leg_b, args.batches)[0])
            da.append(timed(decode_a, args.batches)[0])
            db.append(timed(lambda: dec(data), args.batches)[0])
        lines.append(f"\n{threads} thread{'s' if threads > 1 else ''}; leg B output torch.equal leg A output: {same}")
        lines.append(f"  leg A  Pillow decode + ImagePipeline        {spread(a)} per batch   {B / statistics.median(a):9.0f} img/s")
        lines.append(f"  leg B  JpegDecoder + ImagePipeline          {spread(b)} per batch   {B / statistics.median(b):9.0f} img/s")
        lines.append(f"  A / B  {statistics.median(a) / statistics.median(b):.2f}")
        lines.append(f"  decode alone: Pillow to host arrays         {spread(da)} per batch")
        lines.append(f"  decode alone: JpegDecoder to device images  {spread(db)} per batch")
        if pool:
            pool.shutdown()
        if not same:
            lines.append("  THE LEGS DIFFER")

    # the two kernels alone
    dec = jpeg.JpegDecoder(device, workers=8)
    batch = dec.prepare(data)
    dec.run(batch)
    torch.cuda.synchronize()
    images = [jpeg.entropy_decode(d) for d in data]
    blocks = sum(int(e.coef.shape[0]) for e in images)
    pixels = sum(e.width * e.height for e in images)
    lines.append("\nkernels alone (device events, 40 launches each)")
    for (name, launch), moved, what in zip(dec.launches(batch), (128 * blocks + 384 * B + 64 * blocks, 64 * blocks + 3 * pixels),
                                           ("int16 coefficients + tables in, sample planes out", "sample planes in, RGB out")):
        med, lo, hi = event_ms(launch)
        lines.append(f"  {name:22s} {med:8.4f} ms  ({lo:.4f} .. {hi:.4f});  bytes it must move {moved / 1e6:.1f} MB ({what}) -> "
                     f"{moved / (med * 1e-3) / 1e12:.2f} TB/s = {100 * moved / (med * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM peak")
    lines.append(f"  host-to-device copy of the batch: {batch.copy_bytes / 1e6:.1f} MB of tables and int16 coefficients for {3 * pixels / 1e6:.1f} MB of RGB pixels")
    lines.append("\ncompiler resource report (gfx950)")
    lines += resources()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0 if all("THE LEGS DIFFER" not in line for line in lines) else 1


if __name__ == "__main__":
    sys.exit(main())

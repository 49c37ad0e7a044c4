"""A/B of PNG decoding on seeded images that Pillow encoded (no dataset): Pillow on the host (1 and 8 threads) against png.PngDecoder
with the inflate on the host (zlib in 8 threads) and on the device, same box, same process.

    python tools/png_ab.py [--out profiles/png_ab.txt] [--rounds 5] [--batches 4]

Sources: 500x350 / 350x500 alternating RGB (NLVR2-like), tools/jpeg_ab.py's seeded smooth content with patches and noise, saved by
Pillow at its default level, at B = 32 and 128.  Every leg takes the files' bytes and ends in ImagePipeline(384); the outputs must
be torch.equal.  Per-batch time = median of a round's calls, each ended by a stream synchronise; alternating rounds; reported: the
median of the per-round medians and their range.  Separately: the host time per image of madtp_png_prepare, of zlib's inflate and of
Pillow's whole decode, one thread each; the bytes copied to the device per batch; by device events each kernel alone, with the bytes
it must move against the 8 TB/s HBM peak; the filter types and block counts of the sources; registers / LDS / occupancy as the
compiler reports them.  Needs Pillow and a GPU."""
import argparse
import concurrent.futures
import io
import os
import re
import statistics
import subprocess
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import jpeg_ab  # noqa: E402  (tools/jpeg_ab.py: the sources and the timing helpers)
from madtp_amd import build, png, preprocess  # noqa: E402

SIZE = 384
HBM_PEAK = 8e12


def files(B):
    from PIL import Image
    out = []
    for i in range(B):
        w, h = ((500, 350), (350, 500))[i % 2]
        buf = io.BytesIO()
        Image.fromarray(jpeg_ab.source(100 + i, w, h)).save(buf, "PNG")
        out.append(buf.getvalue())
    return out


def pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def resources():
    try:
        err = subprocess.run([build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                               os.path.join(build.CSRC, "png.hip"), "-o", os.devnull],
                             capture_output=True, text=True, timeout=600).stderr
    except (OSError, subprocess.TimeoutExpired) as e:
        return [f"  compiler resource report not available ({e})"]
    out, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark: +Function Name: (\S+)", line)
        if m:
            cur = {"name": "png_inflate_kernel" if "inflate" in m.group(1) else "png_unfilter_kernel"}
            out.append(cur)
            continue
        m = re.search(r"remark: +([A-Za-z \[\]/]+?): +(\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    if not out:
        return ["  compiler resource report not available (no remarks)"]
    return [f"  {r['name']:20s} VGPRs {r.get('VGPRs')}  SGPRs {r.get('TotalSGPRs')}  scratch {r.get('ScratchSize [bytes/lane]')} B/lane  "
            f"LDS {r.get('LDS Size [bytes/block]')} B/block  occupancy {r.get('Occupancy [waves/SIMD]')} waves/SIMD" for r in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=4)
    args = ap.parse_args()
    try:
        import PIL
    except ImportError:
        raise SystemExit("png_ab: Pillow is needed to encode the sources")
    if not torch.cuda.is_available():
        raise SystemExit("png_ab: no GPU - nothing is measured here")
    device = torch.device("cuda", 0)
    pipe = preprocess.ImagePipeline(SIZE, device=device)
    spread, timed = jpeg_ab.spread, jpeg_ab.timed
    lines = [f"PNG decode: Pillow on the host against PngDecoder (inflate on the host, inflate on the device); files of 500x350 / 350x500 RGB "
             f"saved by Pillow at its default level; {args.rounds} alternating rounds of {args.batches} batches; "
             f"{torch.cuda.get_device_name(0)}; Pillow {PIL.__version__}; zlib {zlib.ZLIB_RUNTIME_VERSION}; every leg ends in ImagePipeline({SIZE})"]
    ok = True
    pools = {n: concurrent.futures.ThreadPoolExecutor(n) for n in (8,)}
    for B in (32, 128):
        data = files(B)
        images = [png.prepare(d) for d in data]
        raws = [zlib.decompress(im.stream.data) for im in images]
        hist = np.zeros(5, np.int64)
        for im, raw in zip(images, raws):
            hist += np.bincount(np.frombuffer(raw, np.uint8)[::1 + im.rowbytes], minlength=5)[:5]
        lines.append(f"\n==== B = {B}: {sum(map(len, data)) / B / 1e3:.1f} kB per file, {sum(map(len, raws)) / B / 1e3:.1f} kB of scanlines; rows by filter "
                     f"type 0..4: {hist.tolist()} ====")
        t_prep, t_inf, t_pil = [], [], []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            for d in data:
                png.prepare(d)
            t_prep.append((time.perf_counter() - t0) / B)
            t0 = time.perf_counter()
            for im in images:
                zlib.decompress(im.stream.data)
            t_inf.append((time.perf_counter() - t0) / B)
            t0 = time.perf_counter()
            for d in data:
                pil_decode(d)
            t_pil.append((time.perf_counter() - t0) / B)
        lines.append("host time per image, one thread, same process")
        lines.append(f"  png.prepare (madtp_png_prepare: chunks, one stream)   {spread(t_prep)}")
        lines.append(f"  zlib.decompress of the stream                         {spread(t_inf)}")
        lines.append(f"  Pillow Image.open(...).convert('RGB') to an array     {spread(t_pil)}")
        legs = {"Pillow, 1 thread": lambda: pipe([pil_decode(d) for d in data]),
                "Pillow, 8 threads": lambda: pipe(list(pools[8].map(pil_decode, data)))}
        decs = {route: png.PngDecoder(device, workers=8, inflate=route) for route in ("host", "device")}
        legs["PngDecoder(inflate='host', 8 threads)"] = lambda: pipe(decs["host"](data))
        legs["PngDecoder(inflate='device')"] = lambda: pipe(decs["device"](data))
        outs = {k: timed(fn, 1)[1] for k, fn in legs.items()}
        ref = outs["Pillow, 1 thread"]
        for k, v in outs.items():
            same = bool(torch.equal(v, ref))
            ok &= same
            if not same:
                lines.append(f"  THE OUTPUT OF {k} DIFFERS FROM PILLOW'S")
        lines.append(f"all four legs torch.equal: {ok}")
        times = {k: [] for k in legs}
        alone = {route: [] for route in decs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                times[k].append(timed(fn, args.batches)[0])
            for route, dec in decs.items():
                alone[route].append(timed(lambda: dec(data), args.batches)[0])
        base = statistics.median(times["Pillow, 8 threads"])
        for k, v in times.items():
            lines.append(f"  {k:40s} + ImagePipeline  {spread(v)} per batch  {B / statistics.median(v):8.0f} img/s   "
                         f"Pillow(8) / this {base / statistics.median(v):.2f}")
        for route, v in alone.items():
            lines.append(f"  decode alone: PngDecoder(inflate='{route}') to device images   {spread(v)} per batch")
        for route, dec in decs.items():
            batch = dec.prepare(data)
            dec.run(batch)
            torch.cuda.synchronize()
            streams, scan, pix = sum(im.stream_bytes for im in images), sum(im.raw_bytes for im in images), sum(3 * im.width * im.height for im in images)
            lines.append(f"inflate='{route}': {batch.copy_bytes / 1e6:.2f} MB copied to the device per batch (streams {streams / 1e6:.2f} MB, scanlines "
                         f"{scan / 1e6:.2f} MB); kernels alone (device events)")
            for name, launch in dec.launches(batch):
                moved = streams + scan if "inflate" in name else scan + pix
                med, lo, hi = jpeg_ab.event_ms(launch, reps=8 if "inflate" in name else 40)
                lines.append(f"  {name:26s} {med:9.4f} ms  ({lo:.4f} .. {hi:.4f})   {moved / 1e6:.2f} MB to move: {moved / (med * 1e-3) / 1e9:8.2f} GB/s, "
                             f"{100 * moved / (med * 1e-3) / HBM_PEAK:.3f} % of the HBM peak")
            if route == "device":
                st = dec.last_status
                lines.append(f"  status words: codes {sorted(set(st[:, png._S['CODE']].tolist()))}; deflate blocks per image {st[:, png._S['BLOCKS']].min()} .. "
                             f"{st[:, png._S['BLOCKS']].max()}")
    lines.append("\ncompiler resource report (gfx950)")
    lines += resources()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

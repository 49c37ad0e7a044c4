"""A/B of the two JPEG decoders on seeded images that Pillow encoded (no dataset): jpeg.JpegDecoder (Huffman decoding on the host,
1 and 8 threads) against jpeg_device.DeviceJpegDecoder (Huffman decoding on the device), same box, same process.

    python tools/jpeg_device_ab.py [--out profiles/jpeg_device_ab.txt] [--rounds 5] [--batches 8]

Sources: tools/jpeg_ab.py's - 640x480 / 480x640 alternating, seeded smooth content with noise, quality 90, 4:2:0 - at B = 32 and 128.
Both legs take the files' bytes and end in ImagePipeline(384); their outputs must be torch.equal.  Per-batch time = median of a
round's calls, each ended by a stream synchronise; five alternating rounds; reported: the median of the per-round medians and their
range.  Separately: the host time per image of madtp_jhuff_prepare against entropy_decode, one thread each; the bytes copied to the
device per batch; by device events the decode kernel alone, the IDCT and colour kernels, and the wait for the status words (from the
launch of the decode kernel to the status words on the host); synchronisation passes per image from the status words; registers /
LDS / occupancy as the compiler reports them.  Needs Pillow and a GPU."""
import argparse
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

if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

import jpeg_ab  # noqa: E402  (tools/jpeg_ab.py: the sources and the timing helpers)
from madtp_amd import build, jpeg, jpeg_device, preprocess  # noqa: E402

SIZE = 384


def files(B):
    import io
    from PIL import Image
    out = []
    for i in range(B):
        w, h = ((640, 480), (480, 640))[i % 2]
        buf = io.BytesIO()
        Image.fromarray(jpeg_ab.source(100 + i, w, h)).save(buf, "JPEG", quality=90, subsampling=2)
        out.append(buf.getvalue())
    return out


def resources():
    try:
        err = subprocess.run([build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                               os.path.join(build.CSRC, "jpeg_huff.hip"), "-o", os.devnull],
                             capture_output=True, text=True, timeout=600).stderr
    except (OSError, subprocess.TimeoutExpired) as e:
        return [f"  compiler resource report not available ({e})"]
    rows = dict(re.findall(r"remark: +([A-Za-z \[\]/]+?): +(\S+) \[-Rpass", err))
    if "VGPRs" not in rows:
        return ["  compiler resource report not available (no remarks)"]
    return [f"  jhuff_decode_kernel  VGPRs {rows.get('VGPRs')}  SGPRs {rows.get('TotalSGPRs')}  scratch {rows.get('ScratchSize [bytes/lane]')} B/lane  "
            f"LDS {rows.get('LDS Size [bytes/block]')} B/block  occupancy {rows.get('Occupancy [waves/SIMD]')} waves/SIMD"]


def status_wait_ms(dec, data, reps=20):
    """host time from the launch of the decode kernel to its status words on the host (the copy and the other launches excluded)"""
    out = []
    for _ in range(reps):
        batch = dec.prepare(data)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.run(batch)  # returns when the status words have arrived; the IDCT and colour kernels are still in flight
        out.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
    return statistics.median(out) * 1e3, min(out) * 1e3, max(out) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=8)
    args = ap.parse_args()
    try:
        import PIL
    except ImportError:
        raise SystemExit("jpeg_device_ab: Pillow is needed to encode the sources")
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_device_ab: no GPU - nothing is measured here")
    device = torch.device("cuda", 0)
    pipe = preprocess.ImagePipeline(SIZE, device=device)
    spread, timed = jpeg_ab.spread, jpeg_ab.timed
    lines = [f"JPEG decode, Huffman stage on the host against on the device; files of 640x480 / 480x640, quality 90, 4:2:0; {args.rounds} "
             f"alternating rounds of {args.batches} batches; {torch.cuda.get_device_name(0)}; Pillow {PIL.__version__}; both legs end in "
             f"ImagePipeline({SIZE})"]
    ok = True
    for B in (32, 128):
        data = files(B)
        lines.append(f"\n==== B = {B}: {sum(map(len, data)) / B / 1e3:.1f} kB per file ====")
        host_a, host_b = [], []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            for d in data:
                jpeg.entropy_decode(d)
            host_a.append((time.perf_counter() - t0) / B)
            t0 = time.perf_counter()
            for d in data:
                jpeg_device.prepare_scan(d)
            host_b.append((time.perf_counter() - t0) / B)
        lines.append("host time per image, one thread, same process")
        lines.append(f"  entropy_decode (parse + Huffman, coefficients out)    {spread(host_a)}")
        lines.append(f"  prepare_scan (madtp_jhuff_prepare: parse + tables)    {spread(host_b)}")
        dev = jpeg_device.DeviceJpegDecoder(device, workers=8)
        leg_d = lambda: pipe(dev(data))
        _, got = timed(leg_d, 2)
        dd, d_alone = [], []
        for threads in (1, 8):
            dec = jpeg.JpegDecoder(device, workers=threads)
            leg_h = lambda: pipe(dec(data))
            _, ref = timed(leg_h, 2)
            same = bool(torch.equal(ref, got))
            ok &= same
            a, b, da, db = [], [], [], []
            for _ in range(args.rounds):
                a.append(timed(leg_h, args.batches)[0])
                b.append(timed(leg_d, args.batches)[0])
                da.append(timed(lambda: dec(data), args.batches)[0])
                db.append(timed(lambda: dev(data), args.batches)[0])
            dd += b
            d_alone += db
            lines.append(f"host leg with {threads} thread{'s' if threads > 1 else ''}; device leg output torch.equal host leg output: {same}")
            lines.append(f"  host leg    JpegDecoder({threads}) + ImagePipeline      {spread(a)} per batch   {B / statistics.median(a):9.0f} img/s")
            lines.append(f"  device leg  DeviceJpegDecoder + ImagePipeline   {spread(b)} per batch   {B / statistics.median(b):9.0f} img/s")
            lines.append(f"  host / device  {statistics.median(a) / statistics.median(b):.2f}")
            lines.append(f"  decode alone: JpegDecoder({threads}) to device images     {spread(da)} per batch")
            lines.append(f"  decode alone: DeviceJpegDecoder to device images {spread(db)} per batch")
            if not same:
                lines.append("  THE LEGS DIFFER")
        batch = dev.prepare(data)
        dev.run(batch)
        torch.cuda.synchronize()
        st = dev.last_status
        S = jpeg_device._S
        host_batch = jpeg.JpegDecoder(device, workers=8).prepare(data)
        lines.append(f"bytes copied to the device per batch: device leg {batch.copy_bytes / 1e6:.2f} MB (files {sum(map(len, data)) / 1e6:.2f} MB, "
                     f"Huffman records {B * jpeg_device.RECORD_BYTES / 1e6:.2f} MB, tables), host leg {host_batch.copy_bytes / 1e6:.2f} MB")
        lines.append("kernels alone (device events, 40 launches each)")
        for name, launch in dev.launches(batch):
            med, lo, hi = jpeg_ab.event_ms(launch)
            lines.append(f"  {name:26s} {med:8.4f} ms  ({lo:.4f} .. {hi:.4f})")
        med, lo, hi = status_wait_ms(dev, data)
        lines.append(f"  launches + wait for the status words (host clock)  {med:8.4f} ms  ({lo:.4f} .. {hi:.4f})")
        lines.append(f"status words: codes {sorted(set(st[:, S['CODE']].tolist()))}; passes per image min {st[:, S['PASSES']].min()} median "
                     f"{int(np.median(st[:, S['PASSES']]))} max {st[:, S['PASSES']].max()}; subsequences per image {st[:, S['SUBSEQS']].min()} .. "
                     f"{st[:, S['SUBSEQS']].max()}; serial lane {int(st[:, S['SERIAL']].sum())}")
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

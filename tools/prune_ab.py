#!/usr/bin/env python
"""A/B of the pruning kernels (csrc/prune.hip) between two builds of the library: same bits, same time.  The tool runs against the
library of the tree it lies in; give the other tree a copy of it and alternate the two in one GPU session:

    python tools/prune_ab.py bits --out A/bits.json        sha256 of every output tensor on seeded inputs
    python tools/prune_ab.py time --out A/time.jsonl       ONE round: appends the device-event median of every leg (call it
                                                           alternately for the two trees, five rounds or more)
    python tools/prune_ab.py report --a A --b B [--names parent,change]
                                                           compares the hashes and prints, per leg, both medians and a's own spread

  bits: token_score (one workgroup per sample: staged, global-read) and token_score_sync (column-split kernels at 577 tokens and
        <= 64 samples, the global-read kernel above), every case with the fast score arithmetic off and on; the exact-f32 att_ft,
        segment by segment, chained, and in one multi-segment launch.
  time: the sizes the workloads run.  A leg's time is the device-event interval around the call; a round's figure is the median over
        --iters launches after warm-up; the report gives the median over the rounds and a's spread (max - min of its rounds): b is
        accepted on a leg when its median is not above a's by more than that spread."""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from madtp_amd import hip  # noqa: E402

K = 100


def score_inputs(B, N, H=12, k=K, seed=0):
    g = torch.Generator().manual_seed(seed)
    nrt = (N + 15) // 16
    side = tuple(torch.rand(*shp, generator=g).cuda() for shp in ((B, nrt, N), (B, H, N), (B, H, N)))
    ta = (torch.randn(B, N, 128, generator=g) * 3.0).cuda()[:, 1:, :k]  # row pitch 128, as the layers pass it
    return side, ta


def att_ft_inputs(B, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, D, generator=g).cuda()
    ta = torch.randn(B, N, 128, generator=g).cuda()[:, 1:, :K]
    return ta, x[:, 1:, :]


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def bits():
    out = {}
    cases = [("token_score", 2, 20, 12, K), ("token_score", 2, 20, 12, 98), ("token_score", 2, 300, 12, K), ("token_score", 1, 1024, 12, K),
             ("token_score_sync", 2, 577, 12, K), ("token_score_sync", 33, 577, 12, K), ("token_score_sync", 65, 577, 12, K),
             ("token_score_sync", 2, 577, 20, K)]
    for fn, B, N, H, k in cases:
        side, ta = score_inputs(B, N, H, k)
        for fast in (0, 1):
            prev = hip.set_score_fast(fast)
            try:
                r = getattr(hip, fn)(side, ta, 3.0, B, H, N)
            finally:
                hip.set_score_fast(prev)
            name = f"{fn} B={B} N={N} H={H} K={k} fast={fast}"
            for part, t in zip(("score", "thr", "count", "k"), r):
                out[f"{name} {part}"] = sha(t) if torch.is_tensor(t) else str(int(t))
    pairs = [att_ft_inputs(2, N, 512, 90 + i) for i, N in enumerate((2, 130, 21))]
    chain = None
    for i, (ta, ft) in enumerate(pairs):
        out[f"att_ft exact single seg{i}"] = sha(hip.query_att_ft(ta, ft))
        chain = hip.query_att_ft(ta, ft, out=chain) if chain is not None else hip.query_att_ft(ta, ft)
    out["att_ft exact chain"] = sha(chain)
    out["att_ft exact multi"] = sha(hip.query_att_ft_multi(pairs, exact=True))
    out["att_ft exact multi accumulate"] = sha(hip.query_att_ft_multi(pairs[1:], out=hip.query_att_ft(*pairs[0]), exact=True))
    return out


def median_us(fn, iters, warm=20):
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
    return statistics.median(ts)


def time_round(iters):
    out = {}
    for B, N, fasts in ((128, 197, (1, 0)), (32, 901, (1,)), (64, 577, (1,)), (128, 577, (1,))):
        side, ta = score_inputs(B, N)
        for fast in fasts:
            prev = hip.set_score_fast(fast)
            try:
                out[f"token_score_sync ({B}, {N}) {'fast' if fast else 'exact'}"] = median_us(
                    lambda: hip.token_score_sync(side, ta, 5.0, B, 12, N), iters)
            finally:
                hip.set_score_fast(prev)
    pairs = [att_ft_inputs(16, 197, 768, 100 + i) for i in range(12)]
    out["query_att_ft exact (16, 197, 768)"] = median_us(lambda: hip.query_att_ft(*pairs[0]), iters)
    out["query_att_ft_multi exact 12 x (16, 197, 768)"] = median_us(lambda: hip.query_att_ft_multi(pairs, exact=True), iters)
    return out


def report(a_dir, b_dir, names):
    na, nb = names
    lines = []
    ha, hb = (json.load(open(os.path.join(d, "bits.json"))) for d in (a_dir, b_dir))
    diff = sorted(k for k in set(ha) | set(hb) if ha.get(k) != hb.get(k))
    lines.append(f"bits: {len(ha)} {na} and {len(hb)} {nb} hashes, {len(diff)} differ" + ("" if diff else ": bit-identical"))
    lines += [f"  DIFFERS {k}: {na} {str(ha.get(k))[:16]} {nb} {str(hb.get(k))[:16]}" for k in diff]
    ra, rb = ([json.loads(x) for x in open(os.path.join(d, "time.jsonl"))] for d in (a_dir, b_dir))
    lines.append(f"time: device-event medians, us; {len(ra)} / {len(rb)} alternated rounds; spread = max - min of {na}'s rounds")
    lines.append(f"  {'leg':48s} {na:>9s} {nb:>9s} {'spread':>8s}")
    ok = not diff
    for leg in ra[0]:
        va, vb = [r[leg] for r in ra], [r[leg] for r in rb]
        ma, mb, sp = statistics.median(va), statistics.median(vb), max(va) - min(va)
        within = mb <= ma + sp
        ok = ok and within
        lines.append(f"  {leg:48s} {ma:9.2f} {mb:9.2f} {sp:8.2f}  {'within' if within else 'SLOWER beyond'} the spread ({mb - ma:+.2f})")
    print("\n".join(lines))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["bits", "time", "report"])
    ap.add_argument("--out")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--a")
    ap.add_argument("--b")
    ap.add_argument("--names", default="parent,change")
    a = ap.parse_args()
    if a.mode == "report":
        raise SystemExit(report(a.a, a.b, a.names.split(",")))
    if not torch.cuda.is_available():
        raise SystemExit("prune_ab: needs the GPU")
    hip.load()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.mode == "bits":
        with open(a.out, "w") as fh:
            json.dump(bits(), fh, indent=1, sort_keys=True)
    else:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(time_round(a.iters)) + "\n")


if __name__ == "__main__":
    main()

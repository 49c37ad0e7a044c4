"""A/B of the token map at the headline shape: NLVR at 384x384, 128 images (64 samples), n0 = 576 patches, 12 layers, the records of
a real forward of the synthetic-weight model.

    python tools/tokenmap_ab.py [--out profiles/tokenmap_ab.txt] [--rounds 5] [--calls 10] [--images 128] [--temperature 5]

Legs, all three from the same `last_prune` records, same box, same process:
  tokenmap   tokenmap.from_records (madtp_tokenmap_build: slot, coef and depth of every layer) and tokenmap.agreement
  torch      the same composition written with torch ops on the device, layer by layer (scatter the kept indices into an inverse
             table, gather the running slots through it): the kept sets only, no merge weights
  harness    harness.compose_ids on host copies of the records, the copies included: what oracle/index_match.py does today
The kept sets of the three legs must be equal.  Device time = device events around a call's launches; wall time = perf_counter around
the call and a stream synchronise.  Per round the median of `calls` calls, alternating rounds; reported: the median of the per-round
medians and their range.  Separately push / pull at C = 768 by device events against the bytes they must move at the 8 TB/s HBM peak,
and registers / LDS / occupancy as the compiler reports them.  Needs a GPU."""
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

from madtp_amd import build, harness, tokenmap  # noqa: E402

HBM_PEAK = 8e12


def torch_compose(records, n0):
    """-> depth int32 [B, n0], with torch ops on the device"""
    first = next(r for r in records if r is not None and r.get("pruned"))
    B, dev = first["indices"].shape[0], first["indices"].device
    cur = torch.arange(n0, device=dev).expand(B, n0).contiguous()
    alive = torch.ones(B, n0, dtype=torch.bool, device=dev)
    depth = torch.zeros(B, n0, dtype=torch.int32, device=dev)
    n = n0
    for rec in records:
        if rec is not None and rec.get("pruned"):
            k = int(rec["k"])
            inv = torch.full((B, n), k, dtype=torch.int64, device=dev)
            inv.scatter_(1, rec["indices"][:, :k], torch.arange(k, device=dev).expand(B, k))
            cur = inv.gather(1, cur)
            alive &= cur < k
            n = k + 1
        depth += alive
    return depth


def torch_agree(da, db, L):
    ls = torch.arange(L, device=da.device, dtype=torch.int32)[None, :, None]
    a, b = da[:, None, :] > ls, db[:, None, :] > ls
    return (a & b).sum(dim=2), (a | b).sum(dim=2)


def harness_sets(records, n0):
    trace = [harness._cpu_info(r) for r in records]  # the host copies belong to this leg
    return harness.compose_ids(trace, n0)


def timed(fn, calls):
    """-> (median device ms by events, median wall ms) of `calls` calls"""
    dev, wall = [], []
    for _ in range(calls):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(e0.elapsed_time(e1))
    return statistics.median(dev), statistics.median(wall)


def resources():
    try:
        err = subprocess.run([build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                               os.path.join(build.CSRC, "tokenmap.hip"), "-o", os.devnull],
                             capture_output=True, text=True, timeout=600).stderr
    except (OSError, subprocess.TimeoutExpired) as e:
        return [f"  (hipcc not run: {e})"]
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark: +(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = {"name": re.sub(r"^_ZN\d+_GLOBAL__N_1\d+", "", t.split(":", 1)[1].strip())}
            rows.append(cur)
        elif cur is not None and ":" in t:
            k, v = t.rsplit(":", 1)
            cur[k.strip()] = v.strip()
    return [f"  {r['name'][:44]:44s} VGPRs {r.get('VGPRs'):>3s}  SGPRs {r.get('TotalSGPRs', r.get('SGPRs')):>3s}  scratch {r.get('ScratchSize [bytes/lane]')}"
            f"  LDS {r.get('LDS Size [bytes/block]'):>5s} B  occupancy {r.get('Occupancy [waves/SIMD]')} waves/SIMD" for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tokenmap_ab.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--temperature", type=float, default=5.0)
    args = ap.parse_args()
    build.build(verbose=False)
    size, n0, L = 384, 576, 12
    model = harness.build_nlvr(size, 0, "cuda")
    images, text, targets = harness.nlvr_inputs(args.images // 2, size, 20, 0)
    with torch.no_grad():
        model(images, text, targets, temperature=args.temperature, train=False)
    records = [b.last_prune for b in model.visual_encoder.blocks]
    records = [None if r is None else {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()} for r in records]  # (own copies: not views)
    lens = harness.token_lengths([harness._cpu_info(r) for r in records], n0 + 1)
    lines = [f"Token map A/B: NLVR visual encoder at {size}x{size}, {args.images} images, n0 = {n0}, {L} layers, temperature {args.temperature}; "
             f"{args.rounds} alternating rounds of {args.calls} calls; {torch.cuda.get_device_name()}",
             f"tokens after each layer (with row 0): {lens}", ""]
    tm = tokenmap.from_records(records, n0)
    want = harness_sets(records, n0)
    depth_t = torch_compose(records, n0)
    equal = torch.equal(depth_t, tm.depth)
    for l in range(L):
        if want[l] is not None:
            kept = tm.kept(l).cpu().numpy()
            equal = equal and all({i for i in s if i < harness.MERGED_BASE} == set(np.nonzero(kept[b])[0].tolist()) for b, s in enumerate(want[l]))
    lines.append(f"kept sets of the three legs equal: {equal}")
    other = tokenmap.TokenMap(tm.slot, tm.coef, torch.minimum(tm.depth, torch.full_like(tm.depth, 3)), tm.n_out, tm.pruned)
    ag = tokenmap.agreement(tm, other)
    ti, tu = torch_agree(tm.depth, other.depth, L)
    lines.append(f"agreement equals the torch restatement: {torch.equal(ag.intersection.long(), ti) and torch.equal(ag.union.long(), tu)}")
    legs = {
        "tokenmap: build launch (table upload + madtp_tokenmap_build)": lambda: tokenmap._build(records, n0),
        "tokenmap: from_records (with the wait for the status words)": lambda: tokenmap.from_records(records, n0),
        "torch:    composition on the device (kept sets only)": lambda: torch_compose(records, n0),
        "harness:  compose_ids with its host copies (kept sets only)": lambda: harness_sets(records, n0),
        "tokenmap: agreement (madtp_tokenmap_agree)": lambda: tokenmap.agreement(tm, other),
        "torch:    agreement by broadcast compare and sum": lambda: torch_agree(tm.depth, other.depth, L),
    }
    for fn in legs.values():
        fn()
    per = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, fn in legs.items():
            per[name].append(timed(fn, args.calls))
    lines.append("")
    lines.append(f"{'leg':64s} {'device ms (rounds)':>34s} {'wall ms (rounds)':>34s}")
    for name, rows in per.items():
        d, w = [r[0] for r in rows], [r[1] for r in rows]
        lines.append(f"{name:64s} {statistics.median(d):10.4f} ({min(d):.4f} .. {max(d):.4f}) {statistics.median(w):12.4f} ({min(w):.4f} .. {max(w):.4f})")
    lines.append("(the harness leg runs on the host: its device time is the copies' only)")
    # push / pull at C = 768 against their bytes
    Cc = 768
    x = torch.randn(tm.B, n0, Cc, device="cuda")
    lines.append("")
    lines.append(f"push / pull of f32 [{tm.B}, {n0}, {Cc}] by device events, bytes that must move against the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    for l in (0, L // 2, L - 1):
        n_l = tm.n_out[l]
        v = torch.randn(tm.B, n_l, Cc, device="cuda")
        moved = (tm.B * n0 * Cc + tm.B * n_l * Cc) * 4 + tm.B * n0 * 8
        for name, fn in ((f"push to layer {l:2d} ({n_l:3d} slots)", lambda: tm.push(x, l)), (f"pull from layer {l:2d} ({n_l:3d} slots)", lambda: tm.pull(v, l, True))):
            fn()
            rows = [timed(fn, args.calls)[0] for _ in range(args.rounds)]
            ms = statistics.median(rows)
            lines.append(f"  {name:32s} {ms:9.4f} ms ({min(rows):.4f} .. {max(rows):.4f})  {moved / 1e6:8.2f} MB: {moved / ms / 1e6:8.1f} GB/s, "
                         f"{100 * moved / (ms * 1e-3) / HBM_PEAK:5.2f} % of the HBM peak")
    lines.append("")
    lines.append("registers / LDS / occupancy (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):")
    lines += resources()
    text_out = "\n".join(lines) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()

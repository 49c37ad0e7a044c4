"""A/B of tokenising on seeded caption-like texts (about 10 words each, the recorded 29 250-entry vocabulary of tests/golden/text_wp.npz):
the installed transformers.BertTokenizer on the host followed by .to(device) - what a user does today - against text.WordPiece, same
box, same process, at padding='max_length', truncation=True, max_length=35 (the retrieval evaluation's call).

    python tools/text_ab.py [--out profiles/text_ab.txt] [--rounds 5] [--resources FILE]

B = 64, 256, and 25 010 texts in batches of 256 (one retrieval evaluation's captions).  Every call ends in a stream synchronise; a
round's figure is the median of its calls (one pass for the 25 010); alternating rounds; reported: the median of the per-round figures
and their range.  The two legs' ids and masks are asserted equal.  Separately for leg B: the kernel alone by device events, the
host packing per text, the wait for the status words.  --resources: the output of tools/kernel_resources.py madtp_amd/csrc/text.hip,
copied into the report.  Needs transformers and a GPU."""
import argparse
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
KW = dict(padding='max_length', truncation=True, max_length=35, return_tensors="pt")


def captions(rng, words, n):
    out = []
    for _ in range(n):
        ws = [rng.choice(words) for _ in range(rng.randint(6, 14))]
        ws[0] = ws[0].capitalize()
        if rng.random() < 0.5:
            ws[rng.randrange(len(ws))] += ","
        out.append(" ".join(ws) + ".")
    return out


def figure(rounds):
    return statistics.median(rounds), min(rounds), max(rounds)


def fmt(name, rounds, per=None):
    med, lo, hi = figure(rounds)
    tail = f"   {per / med * 1e3:10.0f} texts/s" if per else ""
    return f"  {name:58s} {med:10.3f} ms  (rounds {lo:.3f} .. {hi:.3f}){tail}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_ab.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--resources", default=None)
    args = ap.parse_args()
    import tokenizers
    import transformers
    import make_text_golden
    from madtp_amd import hip, text
    hip.load()
    dev = torch.device("cuda", 0)
    g = np.load(os.path.join(ROOT, "tests", "golden", "text_wp.npz"))
    entries = g["vocab_big"].tobytes().decode().split("\n")
    rng = random.Random(3)
    words = make_text_golden.word_list(random.Random(20240611), 3000)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "vocab.txt"), "w", encoding="utf-8") as f:
            f.write("\n".join(entries) + "\n")
        yard = transformers.BertTokenizer(os.path.join(tmp, "vocab.txt"))
    tok = text.WordPiece(entries, dev)
    lines = [f"Tokenising: transformers {transformers.__version__} BertTokenizer (tokenizers {tokenizers.__version__}) + .to(device) against "
             f"text.WordPiece; {len(entries)} entries; seeded captions of 6 .. 14 words; padding='max_length', truncation=True, max_length=35; "
             f"{args.rounds} alternating rounds; {torch.cuda.get_device_name(0)}", ""]

    def leg_a(batch):
        t = yard(batch, **KW)
        ids, mask = t.input_ids.to(dev), t.attention_mask.to(dev)
        torch.cuda.synchronize()
        return ids, mask

    def leg_b(batch):
        t = tok(batch, **KW)
        torch.cuda.synchronize()
        return t.input_ids, t.attention_mask

    for B, total in ((64, 64), (256, 256), (256, 25010)):
        texts = captions(rng, words, total)
        batches = [texts[i:i + B] for i in range(0, total, B)]
        calls = 20 if total == B else 1
        for batch in batches[:3]:  # equal, and warm
            a, b = leg_a(batch), leg_b(batch)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "the two legs' ids differ"
        if total != B:
            for batch in batches:
                a, b = leg_a(batch), leg_b(batch)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "the two legs' ids differ"
        rounds = {"a": [], "b": []}
        for _ in range(args.rounds):
            for name, leg in (("a", leg_a), ("b", leg_b)):
                per_call = []
                for _ in range(calls):
                    t0 = time.perf_counter()
                    for batch in batches:
                        leg(batch)
                    per_call.append((time.perf_counter() - t0) * 1e3)
                rounds[name].append(statistics.median(per_call))
        nbytes = sum(len(t.encode()) for t in texts)
        lines.append(f"==== {total} texts in batches of {B}: {nbytes / total:.1f} bytes per text; both legs' ids and masks torch.equal: True ====")
        lines.append(fmt("A  BertTokenizer(...) + .to(device)", rounds["a"], total))
        lines.append(fmt("B  text.WordPiece(...)", rounds["b"], total))
        lines.append(f"  A / B = {figure(rounds['a'])[0] / figure(rounds['b'])[0]:.2f}")
        # leg B's parts on the first batch
        batch = batches[0]
        pack, kernel, wait = [], [], []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            for _ in range(20):
                text._pack(batch)
            pack.append((time.perf_counter() - t0) / 20 / len(batch) * 1e6)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            packed = tok.encode_raw(batch, 35, 35, True)  # warm
            torch.cuda.synchronize()
            _, raw, off = text._pack(batch)
            ids, mask, status = packed
            data = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(dev)
            doff = torch.from_numpy(off).to(dev)
            ev[0].record()
            for _ in range(20):
                hip._check(text.lib().madtp_text_encode_batch(data.data_ptr(), doff.data_ptr(), tok._chartable.data_ptr(), tok._vocab.data_ptr(),
                                                              ids.data_ptr(), mask.data_ptr(), status.data_ptr(), len(batch), 35, 35, text.TRUNCATE,
                                                              hip._stream()), "madtp_text_encode_batch")
            ev[1].record()
            torch.cuda.synchronize()
            kernel.append(ev[0].elapsed_time(ev[1]) / 20)
            t0 = time.perf_counter()
            for _ in range(20):
                text._waiter.read(status.view(-1))
            wait.append((time.perf_counter() - t0) / 20 * 1e3)
        med, lo, hi = figure(pack)
        lines.append(f"  host packing (encode, join, offsets)                       {med:10.3f} us per text  (rounds {lo:.3f} .. {hi:.3f})")
        lines.append(fmt(f"kernel alone, B = {len(batch)} (device events, 20 launches)", kernel))
        lines.append(fmt("the wait for the status words (idle device)", wait))
        lines.append("")
    if args.resources and os.path.exists(args.resources):
        lines.append("registers / LDS / waves per SIMD as the compiler reports them (tools/kernel_resources.py madtp_amd/csrc/text.hip):")
        with open(args.resources) as f:
            lines += ["  " + " ".join(l.split()) for l in f.read().splitlines() if l.strip()]
    report = "\n".join(lines) + "\n"
    print(report)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(report)


if __name__ == "__main__":
    main()

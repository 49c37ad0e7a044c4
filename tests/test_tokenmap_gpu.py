"""Token maps on the GPU (madtp_amd/tokenmap.py, csrc/tokenmap.hip).  The records are made by the product path's own kernels: seeded
scores go through hip.token_select, a random x through hip.token_gather, chained over the layers (the shapes, ks and score rules of
tests/tokenmap_ref.py); the expected values are the float64 restatement of tests/tokenmap_ref.py on the same records."""
import os

import numpy as np
import pytest
import torch

from tests import tokenmap_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
U = 2.0 ** -24  # one rounding of an f32 result, relative
C = 8           # channels of the chained x: token_gather takes multiples of 4
IDS = [f"B{b}_n{n}_L{l}" for b, n, l in ref.SHAPES]


@pytest.fixture(scope="module")
def env():
    from madtp_amd import build, hip, tokenmap
    build.build(verbose=False)
    hip.load()
    tokenmap.lib()
    return hip, tokenmap


_chains = {}


def chain(env, shape, seed=0, fork=None):
    """The records of one shape made by token_select / token_gather -> dict(records, host (numpy copies), merge_w per layer, x0
    [B, n0 + 1, C], x_last: the chained gather's output, tm, ref: the restatement).  fork = l: the scores of layers >= l come from
    another seed (a second run that diverges there).  Computed once per key and left unchanged."""
    key = (shape, seed, fork)
    if key in _chains:
        return _chains[key]
    hip, tokenmap = env
    B, n0, L = shape
    rng = np.random.default_rng(1000 * n0 + seed)
    rng2 = np.random.default_rng(77 + n0)
    x0 = torch.from_numpy(rng.standard_normal((B, n0 + 1, C), dtype=np.float32)).cuda()
    x, n, records, host, weights = x0, n0, [], [], []
    for l, k in enumerate(ref.KS[shape]):
        if k is None:
            records.append(None), host.append(None), weights.append(None)
            continue
        sc = ref.scores(shape, l, n, rng)
        if fork is not None and l >= fork:
            sc = ref.scores(shape, l, n, rng2)
        sc = ref.select(sc, k, ref.ZERO_LAYER.get(shape) == l)[0]
        score = torch.from_numpy(sc).cuda()
        indices, indices_sort, dst_pos, merge_w = hip.token_select(score, k)
        x = hip.token_gather(x, dst_pos, merge_w, k)
        if shape in ref.WIDE:  # [B, n0] buffers whose first columns count, the rest is never read
            wide = lambda t, fill: torch.cat([t, torch.full((B, n0 - t.shape[1]), fill, dtype=t.dtype, device=t.device)], dim=1)
            indices, indices_sort, score = wide(indices, -1), wide(indices_sort, 1 << 40), wide(score, float("nan"))
        rec = {"pruned": True, "k": k, "indices": indices, "indices_sort": indices_sort, "score": score}
        records.append(rec)
        host.append({k_: (v.cpu().numpy() if torch.is_tensor(v) else v) for k_, v in rec.items()})
        weights.append(merge_w)
        n = k + 1
    out = {"records": records, "host": host, "merge_w": weights, "x0": x0, "x_last": x, "tm": tokenmap.from_records(records, n0),
           "ref": ref.compose(host, n0)}
    _chains[key] = out
    return out


def test_the_shapes_cover_the_cases_the_map_can_go_wrong_at(env):
    seen = set()
    for shape in ref.SHAPES:
        c = chain(env, shape)
        B, n0, L = shape
        ks, r = ref.KS[shape], c["ref"]
        n_in = [n0] + r["n_out"][:-1]
        if any(k is None for k in ks[1:-1]):
            seen.add("an unpruned layer in the middle")
        if 1 in ks:
            seen.add("k = 1")
        if any(k is not None and n - k == 2 for k, n in zip(ks, n_in)):
            seen.add("n_in - k = 2")
        for l in range(1, L):
            if ks[l] is None:
                continue
            before = r["slot"][:, l - 1] == n_in[l] - 1  # the positions of the merged slot entering layer l
            if r["pruned"][l - 1] or any(r["pruned"][:l]):
                now = r["slot"][:, l][before]
                seen.add("a merged slot kept by the next layer" if np.all(now < ks[l]) else "a merged slot merged again" if np.all(now == ks[l]) else "")
        if shape in ref.ZERO_LAYER:
            l = ref.ZERO_LAYER[shape]
            sc, pr = c["host"][l]["score"], c["host"][l]["indices_sort"][:, ks[l]:n_in[l]]
            assert np.all(np.take_along_axis(sc, pr, axis=1) == 0)
            seen.add("a pruned set whose scores are all 0")
        if B > 1 and not np.array_equal(c["host"][0]["indices"][0], c["host"][0]["indices"][1]):
            seen.add("samples with different orders")
        if shape in ref.WIDE and c["records"][0]["indices"].shape[1] > ks[0]:
            seen.add("record tensors wider than k")
    assert seen - {""} == {"an unpruned layer in the middle", "k = 1", "n_in - k = 2", "a merged slot kept by the next layer",
                           "a merged slot merged again", "a pruned set whose scores are all 0", "samples with different orders",
                           "record tensors wider than k"}


@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_slot_and_depth_equal_the_restatement_and_coef_is_within_its_bound(env, shape):
    B, n0, L = shape
    c = chain(env, shape)
    tm, r = c["tm"], c["ref"]
    assert (tm.B, tm.n0, tm.L) == shape and tm.n_out == r["n_out"] and tm.pruned == r["pruned"]
    slot, coef, depth = tm.slot.cpu().numpy(), tm.coef.cpu().numpy(), tm.depth.cpu().numpy()
    assert np.array_equal(slot, r["slot"]) and np.array_equal(depth, r["depth"])
    for l in range(L):
        assert torch.equal(tm.kept(l).cpu(), torch.from_numpy(r["depth"] > l))
    # a sequential f32 sum of up to n_max terms, the + 1e-8, one division and one product per layer: at most (n_max + 3) roundings a
    # layer, L layers (the kernel's sum is 256 short chains and a tree, whose worst case is lower; the issue's bound is the one kept)
    err, bound = np.abs(coef - r["coef"]), L * (n0 + 3) * U * np.abs(r["coef"])
    print(f"{shape}: max |coef - coef64| = {err.max():.3e}, at most {np.max(err / np.maximum(bound, 1e-300)):.4f} of the bound")
    assert np.all(err <= bound) and not np.isnan(coef).any()
    assert np.all(coef[r["depth"][:, None, :] > np.arange(L)[None, :, None]] == 1.0)
    if shape in ref.ZERO_LAYER:
        l = ref.ZERO_LAYER[shape]
        assert np.all(coef[:, l][slot[:, l] == r["n_out"][l] - 1] == 0.0)


@pytest.mark.parametrize("shape", ref.SHAPES + [(65, 400, 1)], ids=IDS + ["B65_n400_L1"])
def test_after_one_layer_coef_has_the_bits_of_token_selects_merge_w(env, shape):
    """(65, 400, 1): more than 320 positions in more than 64 samples, the 1024-thread variant of token_select"""
    hip, tokenmap = env
    B, n0, L = shape
    if shape in ref.KS:
        c = chain(env, shape)
        rec, merge_w, k = c["records"][0], c["merge_w"][0], ref.KS[shape][0]
    else:
        k = 200
        score = torch.from_numpy(np.random.default_rng(400).random((B, n0), dtype=np.float32)).cuda()
        indices, indices_sort, _, merge_w = hip.token_select(score, k)
        rec = {"pruned": True, "k": k, "indices": indices, "indices_sort": indices_sort, "score": score}
    tm = tokenmap.from_records([rec], n0)
    coef, slot = tm.coef[:, 0], tm.slot[:, 0]
    merged = slot == k
    assert int(merged.sum()) == B * (n0 - k) and torch.equal(tm.depth == 0, merged)
    assert torch.equal(coef[merged].view(torch.int32), merge_w[merged].view(torch.int32)), "the pruned sum is not token_select's"
    assert torch.all(coef[~merged] == 1.0) and torch.all(merge_w[~merged] == 0.0)
    # slot i holds indices[b, i]
    assert torch.equal(torch.gather(slot, 1, rec["indices"][:, :k]), torch.arange(k, device="cuda", dtype=torch.int32).expand(B, k))


@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_push_and_the_forwards_own_gather_agree_with_the_restatement(env, shape):
    """y = push(x0, L - 1) and the chained token_gather output, each against the float64 restatement.  A cell of y is a sum of
    `cells` products coef x: `cells` roundings for the sum (the products are fused), and the f32 coef carries one rounding per layer
    (its product) and two for the division and the pruned sum, relative to every term alike: (cells + L + 2) roundings of
    sum |coef x|.  The chained gather rounds the same operations in another order; the bound holds for it alike."""
    B, n0, L = shape
    c = chain(env, shape)
    tm, r = c["tm"], c["ref"]
    n_out = r["n_out"][L - 1]
    x = c["x0"][:, 1:]  # (a view with a batch stride of (n0 + 1) C: read in place)
    y = tm.push(x, L - 1)
    assert y.shape == (B, n_out, C) and torch.equal(y, tm.push(x.contiguous(), L - 1))
    xn = x.cpu().numpy()
    want = ref.push(xn, r["slot"][:, L - 1], r["coef"][:, L - 1], n_out)
    tot, cells = ref.push_abs(xn, r["slot"][:, L - 1], r["coef"][:, L - 1], n_out)
    bound = (cells[:, :, None] + L + 2) * U * tot
    for name, got in (("push", y), ("chained token_gather", c["x_last"][:, 1:])):
        err = np.abs(got.cpu().numpy() - want)
        print(f"{shape} {name}: max err {err.max():.3e}, at most {np.max(err / np.maximum(bound, 1e-300)):.4f} of the bound")
        assert np.all(err <= bound), name
    assert torch.equal(c["x_last"][:, 0], c["x0"][:, 0])  # row 0 is not part of the map
    # a [B, n0] quantity (C = 1, the scalar route) and one with C % 4 != 0, at every layer of the short shapes
    rng = np.random.default_rng(n0)
    for ch in (1, 6):
        q = torch.from_numpy(rng.standard_normal((B, n0, ch), dtype=np.float32)).cuda()
        for l in (range(L) if n0 < 100 else [0, L - 1]):
            got = tm.push(q[:, :, 0] if ch == 1 else q, l).cpu().numpy().reshape(B, r["n_out"][l], ch)
            want = ref.push(q.cpu().numpy(), r["slot"][:, l], r["coef"][:, l], r["n_out"][l])
            tot, cells = ref.push_abs(q.cpu().numpy(), r["slot"][:, l], r["coef"][:, l], r["n_out"][l])
            assert np.all(np.abs(got - want) <= (cells[:, :, None] + L + 2) * U * tot), (ch, l)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_pull_equals_gather(env, shape):
    B, n0, L = shape
    tm = chain(env, shape)["tm"]
    rng = np.random.default_rng(n0 + 1)
    for l in sorted({0, L // 2, L - 1}):
        for ch in (1, 3, 8):
            v = torch.from_numpy(rng.standard_normal((B, tm.n_out[l], ch), dtype=np.float32)).cuda()
            idx = tm.slot[:, l].long()[:, :, None].expand(B, n0, ch)
            want = torch.gather(v, 1, idx)
            assert torch.equal(tm.pull(v, l), want)
            assert torch.equal(tm.pull(v, l, weighted=True), want * tm.coef[:, l][:, :, None])
        flat = torch.from_numpy(rng.standard_normal((B, tm.n_out[l]), dtype=np.float32)).cuda()
        assert torch.equal(tm.pull(flat, l), torch.gather(flat, 1, tm.slot[:, l].long()))
    # pull is the transpose of push: <push(x), v> == <x, pull(v, weighted)> up to rounding
    l = L - 1
    x = torch.from_numpy(rng.standard_normal((B, n0, 4), dtype=np.float32)).cuda()
    v = torch.from_numpy(rng.standard_normal((B, tm.n_out[l], 4), dtype=np.float32)).cuda()
    a, b = (tm.push(x, l).double() * v.double()).sum().item(), (x.double() * tm.pull(v, l, weighted=True).double()).sum().item()
    assert abs(a - b) <= 1e-4 * (1 + abs(a))


@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_agreement_equals_set_arithmetic(env, shape):
    hip, tokenmap = env
    B, n0, L = shape
    a = chain(env, shape)
    same = tokenmap.agreement(a["tm"], a["tm"])
    assert torch.equal(same.intersection, same.union) and bool(same.exact.all()) and bool((same.jaccard == 1).all())
    assert np.array_equal(torch.stack(same, dim=-1).cpu().numpy(), ref.agree(a["ref"]["depth"], a["ref"]["depth"], L))
    if L < 2:
        return
    b = chain(env, shape, fork=1)  # the same layer 0, other scores from layer 1 on
    got = tokenmap.agreement(a["tm"], b["tm"])
    want = ref.agree(a["ref"]["depth"], b["ref"]["depth"], L)
    assert np.array_equal(torch.stack(got, dim=-1).cpu().numpy(), want)
    assert bool(got.exact[:, 0].all())
    if ref.KS[shape][1] is not None:  # (an unpruned layer 1 keeps what layer 0 kept)
        assert not bool(got.exact[:, 1].all()), "the two runs diverge at layer 1"
    jac = want[..., 0] / np.maximum(want[..., 1], 1)
    assert np.allclose(got.jaccard.cpu().numpy(), np.where(want[..., 1] > 0, jac, 1.0), rtol=1e-6)


def test_shade_equals_the_integer_formula(env):
    hip, tokenmap = env
    rng = np.random.default_rng(3)
    for shape, grid, patch in (((2, 196, 12), (14, 14), (4, 4)), ((2, 63, 3), (7, 9), (8, 2)), ((1, 900, 12), (30, 30), (2, 4)), ((1, 3, 1), (1, 3), (16, 16))):
        B, n0, L = shape
        tm = chain(env, shape)["tm"]
        images = rng.integers(0, 256, (B, grid[0] * patch[0], grid[1] * patch[1], 3), dtype=np.uint8)
        depth = tm.depth.cpu().numpy()
        for levels in (None, [0] * L + [255], list(range(255 - L, 256))):
            got = tokenmap.shade(torch.from_numpy(images).cuda(), tm, grid, levels)
            want = ref.shade(images, depth, grid, tokenmap.default_levels(L) if levels is None else levels)
            assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (shape, levels)
    with pytest.raises(ValueError, match="does not divide"):
        tokenmap.shade(torch.zeros(1, 16, 48, 3, dtype=torch.uint8, device="cuda"), chain(env, (1, 3, 1))["tm"], (3, 1))
    with pytest.raises(ValueError, match="not a multiple of 16"):
        tokenmap.shade(torch.zeros(1, 1, 3, 3, dtype=torch.uint8, device="cuda"), chain(env, (1, 3, 1))["tm"], (1, 3))


def test_repeated_calls_give_identical_bits(env):
    hip, tokenmap = env
    shape = (2, 196, 12)
    c = chain(env, shape)
    tm = c["tm"]
    again = tokenmap.from_records(c["records"], 196)
    for a, b in ((tm.slot, again.slot), (tm.depth, again.depth), (tm.coef.view(torch.int32), again.coef.view(torch.int32))):
        assert torch.equal(a, b)
    x = c["x0"][:, 1:]
    v = torch.from_numpy(np.random.default_rng(0).standard_normal((2, tm.n_out[11], C), dtype=np.float32)).cuda()
    images = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (2, 56, 56, 3), dtype=np.uint8)).cuda()
    first = (tm.push(x, 11), tm.pull(v, 11, True), tokenmap.agreement(tm, again).union, tokenmap.shade(images, tm, (14, 14)))
    for _ in range(3):
        second = (tm.push(x, 11), tm.pull(v, 11, True), tokenmap.agreement(tm, again).union, tokenmap.shade(images, tm, (14, 14)))
        for a, b in zip(first, second):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_device_equals_the_host_emulation(env):
    """the same lane routines on both sides: slot, depth, coef and the pushed sums bit for bit"""
    hip, tokenmap = env
    for shape in ((3, 64, 4), (1, 900, 12)):
        B, n0, L = shape
        c = chain(env, shape)
        tm = c["tm"]
        slot, coef, depth, status = tokenmap.build_host(c["host"], n0)
        assert status.tolist() == [0] * B and np.array_equal(slot, tm.slot.cpu().numpy()) and np.array_equal(depth, tm.depth.cpu().numpy())
        assert np.array_equal(coef.view(np.int32), tm.coef.cpu().numpy().view(np.int32))
        x = c["x0"][:, 1:].contiguous()
        y = tokenmap.push_host(x.cpu().numpy(), slot[:, L - 1], coef[:, L - 1], tm.n_out[L - 1])
        assert np.array_equal(y.view(np.int32), tm.push(x, L - 1).cpu().numpy().view(np.int32))


# ---- model level ---------------------------------------------------------------------------------------------------------------------
def _golden_map(g, key, n0):
    lens = g[key + "_lens"].tolist()
    trace = [{"pruned": True, "indices": g[f"{key}{l}_idx"][:, :lens[l] - 2], "k": lens[l] - 2} if f"{key}{l}_idx" in g.files else None
             for l in range(12)]
    if all(t is None for t in trace):
        return None, lens
    return ref.compose(trace, n0), lens


def _same_sets(tm, want, lens, n0, what):
    assert [n + 1 for n in tm.n_out] == lens, what
    for l in range(tm.L):
        kept = tm.kept(l).cpu().numpy()
        assert np.array_equal(kept, np.ones_like(kept) if want is None else want["depth"] > l), f"{what}: kept sets differ at layer {l}"


def _host_records(records):
    return [None if r is None or not r.get("pruned") else {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}
            for r in records]


def _one_hot_rows(tm, records, n0):
    """push of the one-hot identity at the last layer: row s sums to the total coef of slot s"""
    r = ref.compose(_host_records(records), n0)
    l = tm.L - 1
    eye = torch.eye(n0, device="cuda").expand(tm.B, n0, n0)
    y = tm.push(eye, l)
    assert y.shape == (tm.B, tm.n_out[l], n0)
    want = np.stack([np.bincount(r["slot"][b, l], weights=r["coef"][b, l], minlength=tm.n_out[l]) for b in range(tm.B)])
    cells = np.stack([np.bincount(r["slot"][b, l], minlength=tm.n_out[l]) for b in range(tm.B)])
    err = np.abs(y.double().sum(dim=2).cpu().numpy() - want)
    assert np.all(err <= (cells + tm.L * (n0 + 3)) * U * np.maximum(want, 1e-30)), err.max()
    # every column has one entry: the position's own coef, in its own slot
    assert torch.equal((y != 0).sum(dim=1) <= 1, torch.ones(tm.B, n0, dtype=torch.bool, device="cuda"))
    assert np.array_equal(tm.slot.cpu().numpy(), r["slot"]) and np.array_equal(tm.depth.cpu().numpy(), r["depth"])


def test_nlvr_model_maps_equal_the_reference_traces(env):
    from madtp_amd import harness, runtime
    hip, tokenmap = env
    g = np.load(os.path.join(GOLDEN, "nlvr_b2_T5.npz"))
    B, size, L, T, seed = int(g["B"]), int(g["size"]), int(g["L"]), float(g["temperature"]), int(g["seed"])
    model = harness.build_nlvr(size, 0, "cuda")
    images, text, targets = harness.nlvr_inputs(B, size, L, seed, pad_tail=int(g["pad_tail"]) if "pad_tail" in g.files else 0)
    with runtime.precision("fp32"), torch.no_grad():
        model(images, text, targets, temperature=T, train=False)
        n0 = (size // 16) ** 2
        vit = tokenmap.from_vit(model.visual_encoder)
        txt = tokenmap.from_text(model.text_encoder)
    want, lens = _golden_map(g, "vit", n0)
    assert want is not None and (vit.B, vit.L, vit.n0) == (2 * B, 12, n0)
    _same_sets(vit, want, lens, n0, "vit")
    _one_hot_rows(vit, [b.last_prune for b in model.visual_encoder.blocks], n0)
    want, lens = _golden_map(g, "txt", L - 1)
    assert (txt.L, txt.n0) == (12, L - 1)
    _same_sets(txt, want, lens, L - 1, "text")


def test_clip_tower_map_equals_the_reference_trace(env):
    from madtp_amd import runtime, specs, synth
    from madtp_amd.clip_model import VisionTransformer
    hip, tokenmap = env
    g = np.load(os.path.join(GOLDEN, "clip_vit_b2.npz"))
    B, size, T, seed = int(g["B"]), int(g["size"]), float(g["temperature"]), int(g["seed"])
    model = VisionTransformer(input_resolution=size, patch_size=16, width=768, layers=12, heads=12, output_dim=512, sd_dim=768)
    model.load_state_dict(specs.synth_weights(specs.clip_vit_shapes("", size), seed), strict=True)
    model = model.eval().cuda()
    images = synth.synth_images(B, size, seed).cuda()
    space_dict = synth.synth_tensor("space_dict", (100, 768), seed).cuda()
    with runtime.precision("fp32"), torch.no_grad():
        model(images, space_dict, T, 1)
        tm = tokenmap.from_clip(model)
    n0 = (size // 16) ** 2
    want, lens = _golden_map(g, "vit", n0)
    assert want is not None and (tm.B, tm.L, tm.n0) == (B, 12, n0)
    _same_sets(tm, want, lens, n0, "clip")
    _one_hot_rows(tm, [b.last_prune for b in model.transformer.resblocks], n0)


# ---- damaged records: sent only after the host emulation gave each its code (tests/test_tokenmap_cpu.py) ------------------------------
@pytest.mark.parametrize("what,code", [("index == n_in", "RANGE"), ("negative index", "RANGE"), ("repeat", "REPEAT"), ("k > n_in", "K")])
def test_a_damaged_record_raises_naming_sample_and_layer(env, what, code):
    hip, tokenmap = env
    shape, layer = (2, 196, 12), 5
    B, n0, L = shape
    c = chain(env, shape)
    recs = [None if r is None else dict(r) for r in c["records"]]
    r = recs[layer]
    k, n_in = r["k"], c["ref"]["n_out"][layer - 1]
    for name in ("indices", "indices_sort"):
        r[name] = r[name].clone()
    if what == "index == n_in":
        r["indices"][1, k // 2] = n_in
    elif what == "negative index":
        r["indices"][1, 0] = -1
    elif what == "repeat":
        r["indices"][1, 0] = r["indices"][1, k - 1]
    else:
        r["k"] = n_in + 1  # (the buffers are n0 wide: nothing the kernel might read is missing)
    sample = 0 if code == "K" else 1
    with pytest.raises(ValueError, match=rf"sample {sample}, layer {layer}: .*\(code {tokenmap.E[code]}\)"):
        tokenmap.from_records(recs, n0)
    slot, coef, depth, status, _, _ = tokenmap._build(recs, n0, fill=-7)
    status = status.cpu().numpy()
    assert tokenmap.status_fields(status[1]) == (tokenmap.E[code], layer)
    assert bool((slot[1] == -7).all()) and bool((coef[1] == -7).all()) and bool((depth[1] == -7).all()), "the outputs stay untouched"
    if code != "K":
        tm = c["tm"]
        assert status[0] == 0 and torch.equal(slot[0], tm.slot[0]) and torch.equal(depth[0], tm.depth[0]) and torch.equal(coef[0], tm.coef[0])
    else:
        assert tokenmap.status_fields(status[0]) == (tokenmap.E[code], layer) and bool((slot[0] == -7).all())


def test_cpu_tensors_raise(env):
    hip, tokenmap = env
    c = chain(env, (2, 63, 3))
    with pytest.raises(ValueError, match="CPU tensor.*no CPU fallback"):
        tokenmap.from_records([None if r is None else {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in r.items()} for r in c["records"]], 63)
    with pytest.raises(ValueError, match="x is a CPU tensor"):
        c["tm"].push(torch.zeros(2, 63, 4), 0)
    with pytest.raises(ValueError, match="v is a CPU tensor"):
        c["tm"].pull(torch.zeros(2, c["tm"].n_out[2]), 2)

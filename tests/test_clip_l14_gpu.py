"""CLIP ViT-L/14@336 on the HIP path (the model of the reference's configs/retrieval_{coco,flickr}_clip.yaml): patchify of patch
sizes that are not a multiple of 4 into zero-tailed GEMM rows, the padded patch-embedding GEMM, both towers against the reference
fixtures at width 1024 / 16 heads / 577 tokens (vision) and width 768 / 12 heads (text), the vision tower's backward, and the
low-precision modes at the driver's evaluation batch."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
L14 = (336, 14, 1024, 24, 768, 768, 12)  # specs.clip_shapes(size, patch, vision width, vision layers, embed, text width, text layers)


@pytest.fixture(scope="module")
def hip():
    from madtp_amd import build, hip as h
    build.build(verbose=False)
    h.load()
    assert torch.cuda.is_available()
    return h


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _unfold_padded(img, P):
    """torch's im2col of the non-overlapping patches, columns c*P*P + ky*P + kx, zero-padded to the kernel's row width"""
    unf = F.unfold(img, P, stride=P).transpose(1, 2).reshape(-1, 3 * P * P)
    kp = (3 * P * P + 63) // 64 * 64
    return F.pad(unf, (0, kp - unf.shape[1]))


@pytest.mark.parametrize("P,S", [(14, 336), (14, 56), (7, 42), (6, 36)])
def test_patchify_non_multiple_of_4(hip, P, S):
    """P = 14 (ViT-L/14) and other P % 4 != 0 (odd: scalar loads; even: 8-byte loads) in every output format, zero tail included."""
    from madtp_amd import runtime
    img = _rand(3, 3, S, S, seed=P + S)
    ref = _unfold_padded(img, P)
    kp = ref.shape[1]
    assert kp % 64 == 0 and kp > 3 * P * P
    cols = hip.patchify(img.cuda(), P, torch.float32)
    assert tuple(cols.shape) == tuple(ref.shape) and torch.equal(cols.cpu(), ref)
    with runtime.precision("bf16"):
        colsb = hip.patchify(img.cuda(), P, torch.bfloat16)
    assert torch.equal(colsb.cpu(), ref.to(torch.bfloat16))
    with runtime.precision("f16"):   # plain f16 (MADTP_F16) in a bf16-typed buffer
        colsh = hip.patchify(img.cuda(), P, torch.bfloat16)
    assert torch.equal(colsh.view(torch.float16).cpu(), ref.to(torch.float16))
    planes = hip.patchify(img.cuda(), P, torch.float16)  # f16-split planes [P0 | P1], 2 * Kp wide
    assert tuple(planes.shape) == (ref.shape[0], 2 * kp)
    assert torch.equal(planes, hip.split_f16(cols))
    assert not planes[:, 3 * P * P:kp].any() and not planes[:, kp + 3 * P * P:].any()
    # P = 16 rows keep their width (no tail)
    assert hip.patchify(_rand(1, 3, 32, 32, seed=1).cuda(), 16, torch.float32).shape[1] == 768


@pytest.mark.parametrize("mode", ["fp32", "f16x3", "bf16"])
def test_padded_patch_embedding_gemm_matches_conv2d(hip, mode):
    """patchify rows of Kp = 640 columns @ conv1.weight prepared as [1024, 640] with zero columns == F.conv2d in float64 on the same
    rounded operands (bf16: both operands rounded to bf16 first)."""
    from madtp_amd import clip_model, runtime
    B, S, P, D = 2, 336, 14, 1024
    vt = clip_model.VisionTransformer(S, P, D, 1, 16, 768).cuda()
    img = _rand(B, 3, S, S, seed=3)
    with torch.no_grad():
        vt.conv1.weight.copy_(_rand(D, 3, P, P, seed=4, scale=0.02))
    w = vt.conv1.weight.detach().cpu()
    with runtime.precision(mode):
        cdt = runtime.compute_dtype()
        conv = runtime.prepare_linear([vt.conv_weight_cols()], None, cdt)
        assert conv.n == D and conv.w.shape[0] == D and conv.w.shape[1] == (2 if mode == "f16x3" else 1) * 640
        cols = hip.patchify(img.cuda(), P, cdt)
        out = hip.gemm(cols, conv.w, None, out_dtype=torch.float32, n=conv.n).cpu().double()
    if mode == "bf16":
        img, w = img.bfloat16().float(), w.bfloat16().float()
    ref = F.conv2d(img.double(), w.double(), stride=P).flatten(2).transpose(1, 2).reshape(-1, D)
    err = (out - ref).abs().max().item() / ref.abs().max().item()
    print(f"patch embedding {mode}: max rel err {err:.2e}")
    assert err < 1e-5


def _l14_model(seed, device="cuda"):
    from madtp_amd import specs
    from madtp_amd import clip_model as cm
    W = specs.synth_weights(specs.clip_shapes(*L14), seed, device=device)
    model = cm.build_model(dict(W), evaluate=True).eval().cuda()
    v = model.visual
    assert (v.patch_size, v.transformer.width, len(v.transformer.resblocks), v.input_resolution) == (14, 1024, 24, 336)
    assert v.transformer.resblocks[0].n_head == 16 and model.transformer.resblocks[0].n_head == 12
    return model, W


def _traces(blocks):
    return [None if b.last_prune is None else {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in b.last_prune.items()}
            for b in blocks]


L14_FULL_CASES = ["clipl14_full_b2_T4", "clipl14_full_b2_T40"]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", L14_FULL_CASES)
def test_clip_l14_both_towers(hip, name, mode):
    """encode_image / encode_text of ViT-L/14@336 vs the reference's own (tools/make_golden.py clip_full_case): vision kept sets and
    lengths identical, features within 1e-3; the text tower (768 wide, 12 heads) vs the oracle in the canonical token order - lengths
    and kept sets identical, features within 1e-3 - and vs the reference up to its first pruned layer."""
    from madtp_amd import harness, runtime, synth
    from oracle import madtp_oracle as O
    g = np.load(os.path.join(GOLD, name + ".npz"))
    B, size, T, seed = int(g["B"]), int(g["size"]), float(g["temperature"]), int(g["seed"])
    assert size == 336 and int(g["patch"]) == 14
    model, W = _l14_model(seed)
    Wc = {k: v.cpu() for k, v in W.items() if not k.startswith("visual.")}
    images = synth.synth_images(B, size, seed).cuda()
    text = synth.synth_clip_tokens(B, 77, seed, int(g["min_len"]), int(g["max_len"]))
    otr = []
    with torch.no_grad():
        ref_ft, ref_sd = O.clip_encode_text(Wc, text, Wc["space_dict"], T, order="ascending", trace=otr, heads=12)
    with runtime.precision(mode), torch.no_grad():
        fi, sd_i = model.encode_image(images, model.space_dict, T)
        vtr = _traces(model.visual.transformer.resblocks)
        ft, sd_t = model.encode_text(text.cuda(), model.space_dict, T)
        ttr = _traces(model.transformer.resblocks)
    # vision tower == reference
    assert harness.token_lengths(vtr, 577) == g["vit_lens"].tolist()
    ref_v = [{"pruned": True, "indices": g[f"vit{l}_idx"]} if f"vit{l}_idx" in g.files else None for l in range(24)]
    assert harness.compose_ids(vtr, 576) == harness.compose_ids(ref_v, 576)
    assert np.abs(fi.cpu().numpy() - g["image_features"]).max() < 1e-3
    assert abs(float(sd_i.double().norm()) - float(g["sd_img_norm"])) < 1e-4 * float(g["sd_img_norm"])
    # text tower == oracle in canonical (ascending) order: lengths, kept sets, features (the oracle in the reference's order
    # reproduces the fixture: tests/test_clip_l14_cpu.py)
    assert harness.token_lengths(ttr, 77) == harness.token_lengths(otr, 77)
    assert harness.compose_ids(ttr, 76) == O.compose_ids(otr, 76)
    assert (ft.cpu() - ref_ft).abs().max().item() < 1e-3
    assert (sd_t.cpu() - ref_sd).abs().max().item() < 1e-3 * max(1.0, ref_sd.abs().max().item())
    # ... and == reference up to the first pruned layer (same input there, so the same kept SET and the same k)
    first = next(l for l in range(12) if f"txt{l}_idx" in g.files)
    assert harness.token_lengths(ttr, 77)[: first + 1] == g["txt_lens"].tolist()[: first + 1]
    assert (np.sort(ttr[first]["indices"].numpy(), 1) == np.sort(g[f"txt{first}_idx"], 1)).all()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_clip_l14_vision_backward_matches_reference_grads(hip, mode):
    """The ViT-L/14 vision tower under autograd (112^2: 65 tokens, all 24 blocks, 16 heads, width 1024; conv1 through the
    zero-tailed 640-column patch rows) against the reference's own .grad (tools/make_golden.py clip_vit_grad_case)."""
    from madtp_amd import clip_model, specs, synth
    from tests import grad_case
    from tests.test_backward_gpu import _train_mode
    g = np.load(os.path.join(GOLD, "clipl14vitgrad_b2.npz"))
    B, size, seed, T = int(g["B"]), int(g["size"]), int(g["seed"]), float(g["temperature"])
    patch, width, layers, out_dim = int(g["patch"]), int(g["width"]), int(g["layers"]), int(g["out_dim"])
    assert (patch, width, layers, out_dim) == (14, 1024, 24, 768)
    vt = clip_model.VisionTransformer(input_resolution=size, patch_size=patch, width=width, layers=layers, heads=width // 64,
                                      output_dim=out_dim, sd_dim=768)
    vt.load_state_dict(specs.synth_weights(specs.clip_vit_shapes("", size, patch, width, layers, out_dim), seed), strict=True)
    vt = vt.cuda().eval()
    for p_ in vt.parameters():
        p_.requires_grad_(True)
        p_.grad = None
    sd = synth.synth_tensor("space_dict", (100, 768), seed).cuda().requires_grad_(True)
    c = torch.from_numpy(synth.uniform_pm1("clipgrad_c", B * out_dim, seed).reshape(B, out_dim)).cuda()
    a = torch.from_numpy(synth.uniform_pm1("vitgrad_a", B * 100 * 768, seed).reshape(B, 100, 768)).cuda()
    with _train_mode(mode):
        feat, sd_all = vt(synth.synth_images(B, size, seed).cuda(), sd, T, 1)
        assert feat.requires_grad and (feat.detach().cpu() - torch.from_numpy(g["features"])).abs().max().item() < 1e-4
        n, got = (size // patch) ** 2 + 1, []
        for b in vt.transformer.resblocks:
            if b.last_prune and b.last_prune.get("pruned"):
                n = int(b.last_prune["indices"].shape[1]) + 2
            got.append(n)
        assert got == g["vit_lens"].tolist()
        ((feat * c).sum() + (sd_all * a).sum()).backward()
    grads = {k: p_.grad for k, p_ in vt.named_parameters() if p_.grad is not None}
    grads["space_dict"] = sd.grad
    assert tuple(grads["conv1.weight"].shape) == (1024, 3, 14, 14)
    missing = [k[2:-7] for k in g.files if k.startswith("g_") and k.endswith("_sample") and k[2:-7] not in grads]
    assert not missing, f"no gradient produced for {missing[:5]}"
    grad_case.check_against_fixture(g, grads, 1e-3, "HIP CLIP ViT-L/14 vision tower backward vs reference")


@pytest.mark.timeout(900)
def test_clip_l14_eval_batch_all_modes(hip):
    """B = 32 at 336^2 (the driver's evaluation batch), T = 4: f16x3 keeps exactly fp32's per-layer token sets in both towers;
    bf16 / f16 agree with fp32 to the bounds below (set just under the values measured on MI355X, quoted next to them)."""
    from madtp_amd import harness, runtime, synth
    B, T = 32, 4.0
    model, _ = _l14_model(0)
    images = synth.synth_images(B, 336, 7, device="cuda")
    text = synth.synth_clip_tokens(B, 77, 7).cuda()
    out = {}
    for mode in ("fp32", "f16x3", "bf16", "f16"):
        with runtime.precision(mode), torch.no_grad():
            fi, _ = model.encode_image(images, model.space_dict, T)
            vtr = _traces(model.visual.transformer.resblocks)
            ft, _ = model.encode_text(text, model.space_dict, T)
            ttr = _traces(model.transformer.resblocks)
        assert torch.isfinite(fi).all() and torch.isfinite(ft).all(), mode
        out[mode] = (fi.float(), ft.float(), harness.compose_ids(vtr, 576), harness.compose_ids(ttr, 76),
                     harness.token_lengths(vtr, 577), harness.token_lengths(ttr, 77))
    f32 = out["fp32"]
    assert out["f16x3"][2] == f32[2] and out["f16x3"][3] == f32[3]
    assert (out["f16x3"][0] - f32[0]).abs().max().item() < 1e-3 and (out["f16x3"][1] - f32[1]).abs().max().item() < 1e-3
    report = {}
    for mode in ("bf16", "f16"):
        fi, ft, vids, tids, vl, tl = out[mode]
        cos_i = F.cosine_similarity(fi, f32[0], dim=-1).min().item()
        cos_t = F.cosine_similarity(ft, f32[1], dim=-1).min().item()
        # per-layer agreement of the kept vision sets (Jaccard over the batch) at the last layer, and token counts
        last = [l for l in range(24) if vids[l] is not None and f32[2][l] is not None][-1]
        jac = np.mean([len(set(a) & set(b)) / max(1, len(set(a) | set(b))) for a, b in zip(vids[last], f32[2][last])])
        dlen = max(abs(a - b) for a, b in zip(vl, f32[4]))
        report[mode] = (cos_i, cos_t, jac, dlen, tl == f32[5])
        print(f"CLIP L/14 B=32 {mode} vs fp32: min cosine image {cos_i:.4f} text {cos_t:.4f}, last-layer kept-set Jaccard "
              f"{jac:.3f}, max |dlen| {dlen}, text lengths equal {tl == f32[5]}")
    for mode, (cos_i, cos_t, jac, dlen, _) in report.items():
        assert cos_i > BOUNDS[mode]["cos_i"] and cos_t > BOUNDS[mode]["cos_t"], (mode, cos_i, cos_t)
        assert jac > BOUNDS[mode]["jac"] and dlen <= BOUNDS[mode]["dlen"], (mode, jac, dlen)


# measured on MI355X (B = 32, 336^2, T = 4): bf16 min cosine image 0.9998 / text 0.9614, last-layer Jaccard 0.919, max |dlen| 8;
# f16 0.9999 / 1.0000, 0.973, 3
BOUNDS = {"bf16": {"cos_i": 0.999, "cos_t": 0.95, "jac": 0.9, "dlen": 10},
          "f16": {"cos_i": 0.999, "cos_t": 0.999, "jac": 0.96, "dlen": 4}}

"""CLIP ViT-L/14@336 (the geometry of the reference's configs/retrieval_{coco,flickr}_clip.yaml) without a GPU: the reference's own
clip.load() builds the mirror at that geometry, madtp_patchify still validates its arguments on the host for the patch sizes it
now accepts, and the workload's analytic FLOPs follow the L/14 widths."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "models")), reason="reference tree not present")
FIXTURE = os.path.join(ROOT, "tests", "golden", "clipl14_full_b2_T4.npz")


def _run(code):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_fixtures_present():
    for name in ("clipl14_full_b2_T4", "clipl14_full_b2_T40", "clipl14vitgrad_b2"):
        assert os.path.isfile(os.path.join(ROOT, "tests", "golden", name + ".npz")), name
    g = np.load(FIXTURE)
    assert (int(g["patch"]), int(g["vision_width"]), int(g["vision_layers"]), int(g["text_width"]), int(g["size"])) == \
        (14, 1024, 24, 768, 336)
    assert len(g["vit_lens"]) == 24 and len(g["txt_lens"]) == 12


@needs_ref
def test_reference_clip_load_builds_the_l14_mirror(tmp_path):
    """compress_retrieval_clip_dtp.py:262 clip.load() of a clip_large_retrieval_*-shaped checkpoint (ViT-L/14@336) with the
    reference's own clip/clip.py -> build_model of the mirror: 16 vision heads / 24 layers / patch 14, 12 text heads; state-dict keys
    == the reference CLIP's at that geometry (fixture) less the training-only momentum copies and queues."""
    out = _run(f"""
        import sys, json, numpy as np, torch
        sys.path.insert(0, {ROOT!r} + "/tools")
        import ref_shims
        ref_shims.install(chdir=True, import_models=False)
        ref_shims.fast_init()
        import madtp_amd.dropin as dropin
        dropin.install({REF!r})
        from clip import clip
        assert clip.__file__.startswith({REF!r}), clip.__file__
        import madtp_amd.clip_model as mirror
        from madtp_amd import specs
        # fp16 values, as the released CLIP checkpoints store them (load() returns model.float())
        shapes = specs.clip_shapes(336, 14, 1024, 24, 768, 768, 12)
        sd = {{k: torch.full(tuple(shape), 1e-3 * (i % 97 + 1), dtype=torch.float16) for i, (k, shape) in enumerate(shapes.items())}}
        path = {str(tmp_path)!r} + "/clip_large_synth.pth"
        torch.save({{"model": sd}}, path)
        model, _ = clip.load(name=path, device="cpu", evaluate=True, config={{"sd_dim": 768, "sd_num": 100}})
        assert type(model) is mirror.CLIP
        v, t = model.visual, model.transformer
        geo = {{"v_heads": [b.n_head for b in v.transformer.resblocks], "t_heads": [b.n_head for b in t.resblocks],
               "v_layers": len(v.transformer.resblocks), "t_layers": len(t.resblocks), "patch": v.patch_size,
               "res": v.input_resolution, "v_width": v.transformer.width, "t_width": t.width, "embed": model.embed_dim}}
        g = np.load({FIXTURE!r}, allow_pickle=False)
        ref_keys = [str(k) for k in g["state_dict_keys"]]
        msd = model.state_dict()
        mine = sorted(msd.keys())
        same_vals = all(torch.equal(msd[k].float(), sd[k].float()) for k in sd if k in msd)
        print(json.dumps({{"geo": geo, "n": len(mine), "missing": sorted(set(ref_keys) - set(mine)),
                          "extra": sorted(set(mine) - set(ref_keys)), "same_vals": same_vals}}))
        """)
    import json
    rep = json.loads(out.strip().splitlines()[-1])
    geo = rep["geo"]
    assert geo["v_heads"] == [16] * 24 and geo["t_heads"] == [12] * 12
    assert (geo["v_layers"], geo["t_layers"], geo["patch"], geo["res"]) == (24, 12, 14, 336)
    assert (geo["v_width"], geo["t_width"], geo["embed"]) == (1024, 768, 768)
    training_only = lambda k: k.split(".")[0].endswith("_m") or k.split(".")[0].endswith("_queue")  # noqa: E731
    assert all(training_only(k) for k in rep["missing"]), [k for k in rep["missing"] if not training_only(k)][:10]
    assert rep["extra"] == [], rep["extra"][:10]
    assert rep["n"] > 500 and rep["same_vals"]


def test_patchify_validates_arguments_without_gpu():
    """madtp_patchify rejects bad arguments on the host, before any launch, for every patch size it accepts."""
    from madtp_amd import build, hip
    build.build(verbose=False)
    lib = hip.load()
    assert lib.madtp_abi_version() == 31
    E_BADARG, E_SHAPE, E_DTYPE = -1, -2, -3
    for P in (14, 16, 7):
        assert lib.madtp_patchify(0, 16, 2, 336, P, hip.F32, None) == E_BADARG    # null image
        assert lib.madtp_patchify(16, 0, 2, 336, P, hip.F32, None) == E_BADARG    # null output
        assert lib.madtp_patchify(16, 16, 0, 336, P, hip.F32, None) == E_BADARG   # no images
    assert lib.madtp_patchify(16, 16, 2, 336, 0, hip.F32, None) == E_BADARG
    assert lib.madtp_patchify(16, 16, 2, 336, 15, hip.F32, None) == E_SHAPE       # 336 % 15 != 0
    assert lib.madtp_patchify(16, 16, 2, 100, 14, hip.BF16, None) == E_SHAPE      # 100 % 14 != 0
    assert lib.madtp_patchify(16, 16, 2, 100, 16, hip.F16S, None) == E_SHAPE      # 100 % 16 != 0
    assert lib.madtp_patchify(16, 16, 2, 336, 14, 99, None) == E_DTYPE
    assert [hip.patch_cols(p) for p in (16, 14, 8, 7, 32)] == [768, 640, 192, 192, 3072]


def test_clip_l14_flops_hand_count():
    """workloads.Clip(arch="ViT-L/14", size=336).flops(None): 2 x MAC per image-text pair, both towers unpruned, by hand."""
    from madtp_amd import workloads
    w = workloads.Clip(arch="ViT-L/14", size=336)
    assert (w.patch, w.width, w.layers, w.text_width, w.embed_dim) == (14, 1024, 24, 768, 768)
    K, sd = 100, 768                                 # space_dict entries, their width

    def block(n, d):                                 # one unpruned ResidualAttentionBlock on n tokens, width d (MACs)
        qkv, attn, proj, mlp = n * d * 3 * d, 2 * n * n * d, n * d * d, 2 * n * d * 4 * d
        query = (n - 1) * d * sd + (n - 1) * sd * K + K * (n - 1) * sd  # q_map, logits, att_ft
        return qkv + attn + proj + mlp + query

    patch_embed = 576 * 588 * 1024                   # (336 / 14)^2 patches x 3 * 14^2 inputs x width 1024
    mac = patch_embed + 24 * block(577, 1024) + 12 * block(77, 768)
    assert w.flops(None) == 2 * mac
    # the driver's Ori_Gflops = 395.7 (compress_retrieval_clip_dtp.py:281, fvcore: one "flop" per MAC, momentum towers included)
    # is ~198 G MAC per model; this count also has the query models' terms
    assert 0.95 < (mac / 1e9) / (395.7 / 2) < 1.1
    # the default geometry is unchanged (bench.py's "clip" config)
    b = workloads.Clip()
    assert (b.arch, b.size, b.patch, b.width, b.layers, b.text_width) == ("ViT-B/16", 224, 16, 768, 12, 512)
    assert "clip" in workloads.NAMES and len(workloads.NAMES) == 4
    with pytest.raises(ValueError):
        workloads.Clip(arch="RN50")


@pytest.mark.parametrize("name", ["clipl14_full_b2_T4", "clipl14_full_b2_T40"])
def test_oracle_l14_text_tower_matches_reference_fixture(name):
    """The 768-wide, 12-head text tower of ViT-L/14 CLIP: oracle.clip_encode_text(heads=12) in the reference's token order
    reproduces the reference's own per-layer lengths, features and att_ft norm - the oracle the GPU test holds the HIP text tower
    to (in the canonical order)."""
    import torch
    from madtp_amd import harness, specs, synth
    from oracle import madtp_oracle as O
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    B, T, seed = int(g["B"]), float(g["temperature"]), int(g["seed"])
    shapes = {k: v for k, v in specs.clip_shapes(336, 14, 1024, 24, 768, 768, 12).items() if not k.startswith("visual.")}
    W = specs.synth_weights(shapes, seed)
    text = synth.synth_clip_tokens(B, 77, seed, int(g["min_len"]), int(g["max_len"]))
    tr = []
    with torch.no_grad():
        ft, sd = O.clip_encode_text(W, text, W["space_dict"], T, order="reference", trace=tr, heads=12)
    assert harness.token_lengths(tr, 77) == g["txt_lens"].tolist()
    assert np.abs(ft.numpy() - g["text_features"]).max() < 1e-4
    assert abs(float(sd.double().norm()) - float(g["sd_txt_norm"])) < 1e-5 * float(g["sd_txt_norm"])

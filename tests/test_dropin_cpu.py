"""Drop-in boundary in the build container:
  * madtp_amd.dropin.install() makes the REFERENCE's own, unmodified models/blip_nlvr.py / blip_retrieval.py construct on top
    of the MI355X mirrors of models.{vit,med,nlvr_encoder,utils}; the resulting state_dict() keys and shapes equal the pure
    reference model's (recorded in the golden fixtures by tools/make_golden.py);
  * load_checkpoint semantics (models/blip.py:254-278, models/blip_nlvr.py:130-159): position-embedding interpolation equals
    the reference's, twin-branch key duplication, shape filtering.
The reference-importing tests are skipped where the reference tree is absent; the checkpoint tests and the stand-in / fixture
versions of the import-order and pos-embed checks run anywhere."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "models")), reason="reference tree not present")


def _run(code):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@needs_ref
def test_reference_blip_nlvr_constructs_on_the_mirrors():
    out = _run(f"""
        import sys, json, numpy as np
        sys.path.insert(0, {ROOT!r} + "/tools")
        import ref_shims
        ref_shims.install(chdir=True, import_models=False)   # third-party stand-ins only (timm hub, tokenizer files ...)
        ref_shims.fast_init()                                # keys / shapes only: skip the random initialisers
        import madtp_amd.dropin as dropin
        dropin.install({REF!r})
        import models.blip as blip                            # the reference's own glue files, unmodified
        blip.init_tokenizer = lambda: ref_shims.FakeTokenizer()
        import models.blip_nlvr as ref_nlvr
        ref_nlvr.init_tokenizer = blip.init_tokenizer
        assert ref_nlvr.__file__.startswith({REF!r}), ref_nlvr.__file__
        import models.vit, models.med, models.nlvr_encoder, models.utils
        import madtp_amd.vit, madtp_amd.bert
        model = ref_nlvr.blip_nlvr(pretrained='', image_size=224, vit='base', evaluate=True, config=None)
        assert type(model).__module__ == 'models.blip_nlvr'
        assert isinstance(model.visual_encoder, madtp_amd.vit.VisionTransformer)
        assert isinstance(model.text_encoder, madtp_amd.bert.NlvrBertModel)
        sd = model.state_dict()
        g = np.load({ROOT!r} + "/tests/golden/nlvr_b2_T1.npz", allow_pickle=False)
        ref_keys = [str(k) for k in g["state_dict_keys"]]
        mine = sorted(k for k in sd.keys())
        missing = sorted(set(ref_keys) - set(mine)); extra = sorted(set(mine) - set(ref_keys))
        print(json.dumps({{"n": len(mine), "missing": missing, "extra": extra}}))
        """)
    import json
    rep = json.loads(out.strip().splitlines()[-1])
    # buffers that only the reference registers (position_ids) may be absent; nothing else may differ
    assert all("position_ids" in k for k in rep["missing"]), rep["missing"][:10]
    assert all("position_ids" in k for k in rep["extra"]), rep["extra"][:10]
    assert rep["n"] > 500


@needs_ref
def test_reference_clip_load_builds_the_mirror(tmp_path):
    """compress_retrieval_clip_dtp.py:21,262: `from clip import clip; clip.load(name=<checkpoint>, evaluate=True, config=...)`
    with the reference's own clip/clip.py -> build_model of the mirror; state-dict keys == the reference CLIP's (fixture)."""
    out = _run(f"""
        import sys, json, numpy as np, torch
        sys.path.insert(0, {ROOT!r} + "/tools")
        import ref_shims
        ref_shims.install(chdir=True, import_models=False)
        ref_shims.fast_init()
        import madtp_amd.dropin as dropin
        dropin.install({REF!r})
        from clip import clip                                    # the reference's clip/clip.py, unmodified (the driver's import)
        assert clip.__file__.startswith({REF!r}), clip.__file__
        import sys as _s
        clip_pkg = _s.modules["clip"]
        import madtp_amd.clip_model as mirror
        assert _s.modules["clip.model"].build_model is mirror.build_model and clip.build_model is mirror.build_model
        assert "clip.mock" in _s.modules
        assert clip_pkg.load is clip.load and clip_pkg.tokenize is clip.tokenize   # clip/__init__.py: from .clip import *
        from madtp_amd import specs
        # (any values do: the check is that load() copies them into the mirror; the deterministic generator takes ~10 s here)
        sd = {{k: torch.full(tuple(shape), 1e-3 * (i % 97 + 1)) for i, (k, shape) in enumerate(specs.clip_shapes(224).items())}}
        path = {str(tmp_path)!r} + "/clip_synth.pth"
        torch.save({{"model": sd}}, path)
        model, _ = clip.load(name=path, device="cpu", evaluate=True, config={{"sd_dim": 768, "sd_num": 100}})
        assert type(model) is mirror.CLIP and isinstance(model.visual.transformer.resblocks[0], mirror.ResidualAttentionBlock)
        g = np.load({ROOT!r} + "/tests/golden/clip_full_b3_T4.npz", allow_pickle=False)
        ref_keys = [str(k) for k in g["state_dict_keys"]]
        mine = sorted(model.state_dict().keys())
        same_vals = all(torch.equal(model.state_dict()[k].float(), sd[k].float()) for k in sd if k in model.state_dict())
        print(json.dumps({{"n": len(mine), "missing": sorted(set(ref_keys) - set(mine)), "extra": sorted(set(mine) - set(ref_keys)),
                          "same_vals": same_vals}}))
        """)
    import json
    rep = json.loads(out.strip().splitlines()[-1])
    # the mirror holds the EVALUATION state: the momentum copies (`*_m`, clip/model.py:398-427) and the queues (:429-437) of the
    # reference only feed the training loss and are absent; a reference checkpoint's extra keys are ignored by strict=False
    training_only = lambda k: k.split(".")[0].endswith("_m") or k.split(".")[0].endswith("_queue")  # noqa: E731
    assert all(training_only(k) for k in rep["missing"]), [k for k in rep["missing"] if not training_only(k)][:10]
    assert rep["extra"] == [], rep["extra"][:10]
    assert rep["n"] > 300 and rep["same_vals"]


@needs_ref
@pytest.mark.parametrize("which", ["blip_retrieval", "blip_vqa"])
def test_reference_blip_glue_constructs_on_the_mirrors(which):
    """models/blip_retrieval.py / models/blip_vqa.py (the reference's own files) construct on the mirrors; state-dict keys of
    the encoder side equal the reference model's (fixture key list).  blip_vqa's text DECODER (BertLMHeadModel) is the
    rank_answer mirror of madtp_amd.bert (inference half of SURVEY 8(f) rank 4)."""
    fixture = {"blip_retrieval": "retr_i6_t12", "blip_vqa": "vqa480_b2"}[which]
    out = _run(f"""
        import sys, json, numpy as np
        sys.path.insert(0, {ROOT!r} + "/tools")
        import ref_shims
        ref_shims.install(chdir=True, import_models=False)
        ref_shims.fast_init()
        import madtp_amd.dropin as dropin
        dropin.install({REF!r})
        import models.blip as blip
        blip.init_tokenizer = lambda: ref_shims.FakeTokenizer()
        import models.{which} as ref_mod
        ref_mod.init_tokenizer = blip.init_tokenizer
        assert ref_mod.__file__.startswith({REF!r}), ref_mod.__file__
        import madtp_amd.vit, madtp_amd.bert
        if {which!r} == "blip_retrieval":
            model = ref_mod.blip_retrieval(pretrained='', image_size=224, vit='base', evaluate=True, config={{"sd_dim": 768, "sd_num": 100}}, queue_size=16)
        else:
            model = ref_mod.blip_vqa(pretrained='', image_size=480, vit='base', evaluate=True,
                                     config={{"sd_dim": 768, "sd_num": 100, "batch_size_train": 16}})
            import madtp_amd.bert as mb
            assert isinstance(model.text_decoder, mb.BertLMHeadModel)   # the teacher-forced decoder mirror (rank_answer)
        assert type(model).__module__ == 'models.{which}'
        assert isinstance(model.visual_encoder, madtp_amd.vit.VisionTransformer)
        assert isinstance(model.text_encoder, madtp_amd.bert.MedBertModel)
        g = np.load({ROOT!r} + "/tests/golden/{fixture}.npz", allow_pickle=False)
        ref_keys = [str(k) for k in g["state_dict_keys"]]
        mine = sorted(model.state_dict().keys())
        print(json.dumps({{"n": len(mine), "missing": sorted(set(ref_keys) - set(mine)), "extra": sorted(set(mine) - set(ref_keys))}}))
        """)
    import json
    rep = json.loads(out.strip().splitlines()[-1])
    ok = lambda k: "position_ids" in k  # noqa: E731  (buffers only the reference registers)
    # the fixture lists the evaluation-side keys; the reference's own glue class also builds its training state on the mirrors
    # (momentum encoders, queues, temp: blip_retrieval.py:67-93) and, for VQA, the answer decoder
    train = lambda k: k.split(".")[0].endswith(("_m", "_queue")) or k.split(".")[0] in ("temp", "text_decoder")  # noqa: E731
    assert all(ok(k) for k in rep["missing"]), rep["missing"][:10]
    assert all(ok(k) or train(k) for k in rep["extra"]), [k for k in rep["extra"] if not (ok(k) or train(k))][:10]
    assert rep["n"] > 300


@needs_ref
def test_install_after_reference_import_is_refused():
    _run(f"""
        import sys
        sys.path.insert(0, {ROOT!r} + "/tools")
        import ref_shims
        ref_shims.install(chdir=True, import_models=True)    # imports the reference's own models.vit
        import madtp_amd.dropin as dropin
        try:
            dropin.install({REF!r})
        except RuntimeError as e:
            assert "before the first" in str(e)
        else:
            raise SystemExit("install() after `import models.vit` must be refused")
        """)


@needs_ref
def test_interpolate_pos_embed_equals_reference():
    out = _run(f"""
        import sys, torch
        sys.path.insert(0, {ROOT!r} + "/tools")
        import ref_shims
        ref_shims.install(chdir=True, import_models=True)
        import models.vit as ref_vit
        from madtp_amd.vit import interpolate_pos_embed
        class Enc:  # the two attributes the function reads
            class patch_embed: num_patches = 576
            pos_embed = torch.zeros(1, 577, 768)
        torch.manual_seed(0)
        ck = torch.randn(1, 197, 768)
        a, b = ref_vit.interpolate_pos_embed(ck, Enc), interpolate_pos_embed(ck, Enc)
        assert a.shape == (1, 577, 768) and torch.equal(a, b)
        Enc.patch_embed.num_patches, Enc.pos_embed = 196, torch.zeros(1, 197, 768)
        assert interpolate_pos_embed(ck, Enc) is ck
        print("ok")
        """)
    assert "ok" in out


def test_install_after_foreign_models_import_is_refused(tmp_path):
    """The refusal above without the reference tree: a stand-in `models` package whose vit.py is not a mirror."""
    (tmp_path / "models").mkdir()
    (tmp_path / "models" / "__init__.py").write_text("")
    (tmp_path / "models" / "vit.py").write_text("FOREIGN = True\n")
    _run(f"""
        import sys
        sys.path.insert(0, {str(tmp_path)!r})
        import models.vit
        assert models.vit.FOREIGN
        import madtp_amd.dropin as dropin
        try:
            dropin.install({str(tmp_path)!r})
        except RuntimeError as e:
            assert "before the first" in str(e)
        else:
            raise SystemExit("install() after `import models.vit` must be refused")
        """)


def test_interpolate_pos_embed_equals_reference_fixture(golden_dir):
    """The comparison above without the reference tree: the reference's own output for a seeded 14x14 (+ CLS) grid resized to
    24x24, recorded by tools/make_golden.py (pos_embed_384)."""
    from madtp_amd.vit import interpolate_pos_embed
    g = np.load(os.path.join(golden_dir, "pos_embed_384.npz"))
    ck, ref = torch.from_numpy(g["checkpoint"]), torch.from_numpy(g["resized"])

    class Enc:
        class patch_embed: num_patches = 576
        pos_embed = torch.zeros(1, 577, ck.shape[-1])
    out = interpolate_pos_embed(ck, Enc)
    assert out.shape == ref.shape == (1, 577, ck.shape[-1]) and torch.equal(out, ref)
    Enc.patch_embed.num_patches, Enc.pos_embed = 196, torch.zeros(1, 197, ck.shape[-1])
    assert interpolate_pos_embed(ck, Enc) is ck


def test_load_checkpoint_semantics(tmp_path):
    """blip_nlvr(pretrained=path): pos-embed interpolation 14x14 -> 24x24, crossattention.self -> self0/self1 and
    output.dense -> dense0/dense1 duplication, strict=False; blip.load_checkpoint: keys with a different shape are dropped."""
    from madtp_amd.checkpoint import load_checkpoint, load_checkpoint_nlvr
    from madtp_amd.vit import VisionTransformer, interpolate_pos_embed

    class Tiny(torch.nn.Module):
        def __init__(self, img):
            super().__init__()
            self.visual_encoder = VisionTransformer(img_size=img, patch_size=16, embed_dim=768, depth=1, num_heads=12, evaluate=True)
            self.crossattention = torch.nn.ModuleDict({"self0": torch.nn.Linear(4, 4), "self1": torch.nn.Linear(4, 4)})
            self.other = torch.nn.Linear(3, 3)
    src = Tiny(224)
    torch.manual_seed(1)
    for p in src.parameters():
        p.data.normal_()
    sd = {k: v.clone() for k, v in src.state_dict().items() if "self0" not in k and "self1" not in k}
    sd["crossattention.self.weight"] = torch.randn(4, 4)
    sd["crossattention.self.bias"] = torch.randn(4)
    path = os.path.join(tmp_path, "ck.pth")
    torch.save({"model": sd, "temperature": 3.0}, path)
    sd["other.weight"] = torch.randn(5, 5)                     # wrong shape: dropped by blip.load_checkpoint (second half)
    dst = Tiny(384)
    dst, msg = load_checkpoint_nlvr(dst, path)
    got = dst.state_dict()
    assert got["visual_encoder.pos_embed"].shape == (1, 577, 768)
    assert torch.equal(got["visual_encoder.pos_embed"], interpolate_pos_embed(sd["visual_encoder.pos_embed"], dst.visual_encoder))
    assert torch.equal(got["crossattention.self0.weight"], sd["crossattention.self.weight"])
    assert torch.equal(got["crossattention.self1.bias"], sd["crossattention.self.bias"])
    assert "crossattention.self.weight" in msg.unexpected_keys
    dst2 = Tiny(384)
    before = dst2.other.weight.clone()
    sd2 = dict(sd); sd2.pop("crossattention.self.weight"); sd2.pop("crossattention.self.bias")
    dst2, msg2 = load_checkpoint(dst2, {"model": sd2})
    assert torch.equal(dst2.other.weight, before) and "other.weight" in msg2.missing_keys
    assert dst2.state_dict()["visual_encoder.pos_embed"].shape == (1, 577, 768)
    with pytest.raises(RuntimeError):
        load_checkpoint(dst2, "https://example.com/x.pth")


@needs_ref
def test_reference_blip_decoder_constructs_on_the_mirrors():
    """models/blip.py BLIP_Decoder (the captioning model of compress_caption_dtp.py; the reference's own file) constructs on the
    mirrors: state-dict keys equal the reference model's, and its `self.text_decoder.generate(...)` call site (:189-196) resolves
    to the beam search of madtp_amd.bert.BertLMHeadModel with the keyword arguments the reference passes."""
    out = _run(f"""
        import sys, json, inspect, numpy as np
        sys.path.insert(0, {ROOT!r} + "/tools")
        import ref_shims
        ref_shims.install(chdir=True, import_models=False)
        ref_shims.fast_init()
        import madtp_amd.dropin as dropin
        dropin.install({REF!r})
        import models.blip as blip
        blip.init_tokenizer = lambda: ref_shims.FakeTokenizer()
        assert blip.__file__.startswith({REF!r}), blip.__file__
        import madtp_amd.vit, madtp_amd.bert as mb
        model = blip.blip_decoder(pretrained='', image_size=224, vit='base', evaluate=True, config={{"sd_dim": 768, "sd_num": 100}})
        assert type(model).__module__ == 'models.blip' and model.prompt_length == 4
        assert isinstance(model.visual_encoder, madtp_amd.vit.VisionTransformer)
        assert isinstance(model.text_decoder, mb.BertLMHeadModel)
        params = set(inspect.signature(model.text_decoder.generate).parameters)
        need = {{"input_ids", "max_length", "min_length", "num_beams", "eos_token_id", "pad_token_id", "repetition_penalty",
                 "encoder_hidden_states", "encoder_attention_mask"}}
        g = np.load({ROOT!r} + "/tests/golden/cap_gen_b2_T6.npz", allow_pickle=False)
        ref_keys = [str(k) for k in g["state_dict_keys"]]
        mine = sorted(model.state_dict().keys())
        print(json.dumps({{"n": len(mine), "missing": sorted(set(ref_keys) - set(mine)), "extra": sorted(set(mine) - set(ref_keys)),
                          "generate_args_missing": sorted(need - params)}}))
        """)
    import json
    rep = json.loads(out.strip().splitlines()[-1])
    assert all("position_ids" in k for k in rep["missing"]), rep["missing"][:10]
    assert all("position_ids" in k for k in rep["extra"]), rep["extra"][:10]
    assert rep["generate_args_missing"] == [] and rep["n"] > 300

#!/usr/bin/env python
"""Generates tests/golden/*.npz by IMPORTING THE REFERENCE (read-only, /root/reference) in this container.

Runs only here (the reference never travels to the GPU box).  For each case it
  1. builds the reference model (models.blip_nlvr.BLIP_NLVR, ...) behind tools/ref_shims.py,
  2. loads the repo's deterministic synthetic weights (madtp_amd.synth) into it BY STATE-DICT KEY,
  3. runs the reference forward on the repo's synthetic inputs and records, per layer, the `indices` the
     reference passes to vector_gather (kept tokens, vit.py:153-154 / nlvr_encoder.py:440-441), plus logits
     and a few float checksums.
The fixtures are data only: seeds, temperatures, integer index arrays, small float vectors.

usage: python tools/make_golden.py [case ...]     (default: all cases)
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_shims  # noqa: E402

ref_shims.install()

from madtp_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


class GatherTap:
    """Wraps a module-global `vector_gather` so the first call of each Reduce_token (kept `indices`) and the
    second (`indices_sort`) are recorded under the current layer tag."""

    def __init__(self, module):
        self.module = module
        self.orig = module.vector_gather
        self.records = {}
        self.tag = None
        self.calls = 0
        module.vector_gather = self

    def set_tag(self, tag):
        self.tag = tag
        self.calls = 0

    def __call__(self, vectors, indices):
        if self.tag is not None and vectors.shape[-1] > 1:
            name = "idx" if self.calls == 0 else "sort"
            if self.calls < 2:
                self.records[f"{self.tag}_{name}"] = indices.detach().cpu().numpy().astype(np.int32)
            self.calls += 1
        return self.orig(vectors, indices)

    def restore(self):
        self.module.vector_gather = self.orig


def nlvr_case(name, B, size, L, temperature, seed=0, pad_tail=0, pad_list=None):
    import models.blip_nlvr as bn
    import models.vit as rvit
    import models.nlvr_encoder as rnl
    ref_shims.patch_tokenizer(bn)
    model = bn.BLIP_NLVR(image_size=size, evaluate=True, config={"sd_num": 100, "sd_dim": 768, "batch_size_train": 16})
    model.eval()
    sd = synth.fill_state_dict(model, seed)
    missing = model.load_state_dict(sd, strict=True)
    images = synth.synth_images(2 * B, size, seed)
    ids = synth.synth_token_ids(B, L, seed, first_id=None)
    from madtp_amd import harness
    text = {"input_ids": ids, "attention_mask": harness.padded_mask(B, L, pad_list if pad_list is not None else pad_tail)}
    tap_v, tap_t = GatherTap(rvit), GatherTap(rnl)
    hooks = []
    lens_v, lens_t = [], []
    for i, blk in enumerate(model.visual_encoder.blocks):
        hooks.append(blk.register_forward_pre_hook(lambda m, a, i=i: tap_v.set_tag(f"vit{i}")))
        hooks.append(blk.register_forward_hook(lambda m, a, o: lens_v.append(o.shape[1])))
    for i, lay in enumerate(model.text_encoder.encoder.layer):
        hooks.append(lay.register_forward_pre_hook(lambda m, a, i=i: tap_t.set_tag(f"txt{i}")))
        hooks.append(lay.register_forward_hook(lambda m, a, o: lens_t.append(o[0].shape[1])))
    feats = {}
    hooks.append(model.visual_encoder.register_forward_hook(lambda m, a, o: feats.__setitem__("img", o[0].detach())))
    t0 = time.time()
    with torch.no_grad():
        logits = model(images, text, torch.zeros(B, dtype=torch.long), temperature=temperature, train=False)
    dt = time.time() - t0
    for h in hooks:
        h.remove()
    tap_v.restore()
    tap_t.restore()
    # the reference's forward timed properly for bench.py's cpu_baseline.reference_proper: hooks off, warm, median of 5 (the first,
    # un-warmed forward above carries the taps and one-time allocations: 0.74 s against a 0.41 s median on this container's 8 threads)
    import copy
    times = []
    with torch.no_grad():
        for _ in range(6):
            txt = {k: v.clone() for k, v in text.items()}
            t1 = time.time()
            model(images, txt, torch.zeros(B, dtype=torch.long), temperature=temperature, train=False)
            times.append(time.time() - t1)
    dt_first, dt = dt, float(np.median(times[1:]))
    out = {"kind": "nlvr", "B": B, "size": size, "L": L, "temperature": np.float64(temperature), "seed": seed, "pad_tail": pad_tail,
           "logits": logits.numpy(), "vit_lens": np.array(lens_v), "txt_lens": np.array(lens_t),
           "img_embeds_cls": feats["img"][:, 0, :16].numpy(), "img_embeds_absmean": feats["img"].abs().mean().numpy(),
           "state_dict_keys": np.array(sorted(sd.keys())), "ref_seconds": dt, "ref_seconds_first_call": dt_first,
           "ref_seconds_runs": np.array(times[1:]), "threads": torch.get_num_threads()}
    if pad_list is not None:
        out["pad_list"] = np.array(pad_list)
    out.update(tap_v.records)
    out.update(tap_t.records)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(f"[{name}] T={temperature} vit_lens={lens_v} txt_lens={lens_t} logits={logits.numpy().round(4).tolist()} "
          f"({dt:.2f}s)")


def nlvr_model_grad_case(name, B, size, L, temperature, seed=0, pad_tail=0, nsample=128, train=False):
    """SURVEY 8(f) rank 4 (backward), the headline model end to end: the reference's OWN autograd through
    models/blip_nlvr.py BLIP_NLVR.forward(train=False) - pruned ViT on both images, BERT embeddings, twelve NLVR layers with twin
    cross-attention, cls_head - with every parameter (space_dict included) as a leaf and loss = sum(logits * c).  Recorded: per-layer
    lengths, the logits, and of every gradient its L2 norm, sum and `nsample` sampled entries."""
    import models.blip_nlvr as bn
    import models.vit as rvit
    import models.nlvr_encoder as rnl
    ref_shims.patch_tokenizer(bn)
    model = bn.BLIP_NLVR(image_size=size, evaluate=True, config={"sd_num": 100, "sd_dim": 768, "batch_size_train": 16})
    model.eval()
    sd = synth.fill_state_dict(model, seed)
    model.load_state_dict(sd, strict=True)
    images = synth.synth_images(2 * B, size, seed)
    ids = synth.synth_token_ids(B, L, seed, first_id=None)
    from madtp_amd import harness
    text = {"input_ids": ids, "attention_mask": harness.padded_mask(B, L, pad_tail)}
    lens_v, lens_t, hooks = [], [], []
    for blk in model.visual_encoder.blocks:
        hooks.append(blk.register_forward_hook(lambda m, a, o: lens_v.append(o.shape[1])))
    for lay in model.text_encoder.encoder.layer:
        hooks.append(lay.register_forward_hook(lambda m, a, o: lens_t.append(o[0].shape[1])))
    for p_ in model.parameters():
        p_.requires_grad_(True)
        p_.grad = None
    targets = torch.arange(B, dtype=torch.long) % 2
    if train:
        # the reference's training step (compress_nlvr_dtp.py:52-56) in model.eval() (no dropout / DropPath: deterministic):
        # loss = loss_ori + 0.1 * loss_fdt (cross-entropy + cosine embedding loss of the dictionary features, blip_nlvr.py:84-98)
        loss_ori, loss_fdt = model(images, text, targets, temperature=temperature, train=True)
        logits = torch.zeros(B, 2)
        (loss_ori + 0.1 * loss_fdt).backward()
    else:
        logits = model(images, text, targets, temperature=temperature, train=False)
        c = torch.from_numpy(synth.uniform_pm1("nlvrgrad_c", B * 2, seed).reshape(B, 2))
        (logits * c).sum().backward()
    for h in hooks:
        h.remove()
    rec = {"kind": "nlvr_model_grad", "B": B, "size": size, "L": L, "temperature": np.float64(temperature), "seed": seed,
           "pad_tail": pad_tail, "nsample": nsample, "logits": logits.detach().numpy(), "vit_lens": np.array(lens_v),
           "txt_lens": np.array(lens_t), "train": int(train)}
    if train:
        rec["loss_ori"], rec["loss_fdt"] = np.float64(loss_ori.item()), np.float64(loss_fdt.item())
    n = 0
    with_grad = [(k, v) for k, v in model.named_parameters() if v.grad is not None]
    # the three LARGEST parameters (word embeddings, the first MLP weights): 4096 sampled entries each on top of the common
    # sample, so that a localised error in a 23 M-entry gradient cannot hide behind its norm (hygiene)
    big = {k for k, _ in sorted(with_grad, key=lambda kv: -kv[1].numel())[:3]}
    rec["nsample_big"] = 4096
    for k, v in with_grad:
        flat = v.grad.detach().reshape(-1)
        idx = grad_sample_index(flat.numel(), nsample)
        rec[f"g_{k}_sample"] = flat[torch.from_numpy(idx)].numpy()
        rec[f"g_{k}_norm"] = np.float64(flat.double().norm().item())
        if k in big:
            rec[f"g_{k}_bigsample"] = flat[torch.from_numpy(grad_sample_index(flat.numel(), 4096, stride=104729))].numpy()
        n += 1
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] T={temperature} vit_lens={lens_v} txt_lens={lens_t} logits={logits.detach().numpy().round(4).tolist()} "
          f"{n} gradients")


def vqa_case(name, B, size, L, temperature, seed=0, pad_tail=0):
    """models/blip_vqa.py BLIP_VQA, encoder leg of forward(train=False) (:59-64, :118-125): the reference's own visual_encoder
    and text_encoder (MED, multimodal mode) called exactly as those lines do; the answer decoder that follows is out of scope."""
    import models.blip_vqa as bv
    import models.vit as rvit
    import models.med as rmed
    ref_shims.patch_tokenizer(bv)
    model = bv.BLIP_VQA(image_size=size, evaluate=True, config={"sd_num": 100, "sd_dim": 768, "batch_size_train": 16})
    model.eval()
    sd = synth.fill_state_dict(model, seed)
    model.load_state_dict(sd, strict=True)
    images = synth.synth_images(B, size, seed)
    ids = synth.synth_token_ids(B, L, seed, first_id=None)
    from madtp_amd import harness
    att = harness.padded_mask(B, L, pad_tail)
    tap_v, tap_t = GatherTap(rvit), GatherTap(rmed)
    hooks, lens_v, lens_t = [], [], []
    for i, blk in enumerate(model.visual_encoder.blocks):
        hooks.append(blk.register_forward_pre_hook(lambda m, a, i=i: tap_v.set_tag(f"vit{i}")))
        hooks.append(blk.register_forward_hook(lambda m, a, o: lens_v.append(o.shape[1])))
    for i, lay in enumerate(model.text_encoder.encoder.layer):
        hooks.append(lay.register_forward_pre_hook(lambda m, a, i=i: tap_t.set_tag(f"txt{i}")))
        hooks.append(lay.register_forward_hook(lambda m, a, o: lens_t.append(o[0].shape[1])))
    t0 = time.time()
    with torch.no_grad():
        image_embeds, sd_img_ft = model.visual_encoder(images, space_dict=model.space_dict, temperature=temperature)  # :59
        image_atts = torch.ones(image_embeds.size()[:-1], dtype=torch.long)  # :60
        q_ids = ids.clone()
        q_ids[:, 0] = model.tokenizer.enc_token_id  # :64
        question_output = model.text_encoder(q_ids, attention_mask=att, encoder_hidden_states=image_embeds,
                                             encoder_attention_mask=image_atts, return_dict=True,
                                             space_dict=model.space_dict, temperature=temperature)[0]  # :118-124
    dt = time.time() - t0
    for h in hooks:
        h.remove()
    tap_v.restore()
    tap_t.restore()
    hid = question_output.last_hidden_state
    enc_keys = sorted(k for k in sd.keys() if not k.startswith("text_decoder."))
    out = {"kind": "vqa", "B": B, "size": size, "L": L, "temperature": np.float64(temperature), "seed": seed, "pad_tail": pad_tail,
           "vit_lens": np.array(lens_v), "txt_lens": np.array(lens_t), "hidden_cls": hid[:, 0, :32].numpy(),
           "hidden_shape": np.array(hid.shape), "img_embeds_cls": image_embeds[:, 0, :16].numpy(),
           "state_dict_keys": np.array(enc_keys), "ref_seconds": dt, "threads": torch.get_num_threads()}
    out.update({k: v for k, v in tap_v.records.items() if k.endswith("_idx")})
    out.update(tap_t.records)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(f"[{name}] size={size} T={temperature} vit_lens={lens_v} txt_lens={lens_t} ({dt:.1f}s)")


def med_case(name, B, L, Nimg, temperature, mode, seed=0, pad_tail=0):
    """models/med.py BertModel (MED) stand-alone: text mode / multimodal mode with synthetic image tokens and an
    optional padded tail in attention_mask (exercises med.py:388-390 mask compaction)."""
    import models.med as rmed
    from madtp_amd import specs
    cfg = rmed.BertConfig.from_json_file("configs/med_config.json")
    cfg.encoder_width = 768
    cfg.evaluate = True
    model = rmed.BertModel(config=cfg, add_pooling_layer=False)
    model.eval()
    shapes = specs.bert_shapes("", "med")
    sd = specs.synth_weights(shapes, seed)
    msg = model.load_state_dict(sd, strict=False)
    assert not msg.unexpected_keys and all("query_model" in k or "position_ids" in k for k in msg.missing_keys), msg
    space_dict = synth.synth_tensor("space_dict", (100, 768), seed)
    ids = synth.synth_token_ids(B, L, seed + 1)
    att = torch.ones_like(ids)
    if pad_tail:
        for b in range(B):
            att[b, L - (b % (pad_tail + 1)):] = 0
    enc = synth.synth_tensor("image_embeds", (B, Nimg, 768), seed).mul(25.0) if mode == "multimodal" else None
    enc_att = torch.ones(B, Nimg, dtype=torch.long) if enc is not None else None
    tap = GatherTap(rmed)
    hooks, lens = [], []
    for i, lay in enumerate(model.encoder.layer):
        hooks.append(lay.register_forward_pre_hook(lambda m, a, i=i: tap.set_tag(f"txt{i}")))
        hooks.append(lay.register_forward_hook(lambda m, a, o: lens.append(o[0].shape[1])))
    with torch.no_grad():
        out, _ = model(ids, attention_mask=att, encoder_hidden_states=enc, encoder_attention_mask=enc_att, return_dict=True,
                       mode=mode, space_dict=space_dict, temperature=temperature)
    for h in hooks:
        h.remove()
    tap.restore()
    hid = out.last_hidden_state
    rec = {"kind": "med", "B": B, "L": L, "Nimg": Nimg, "mode": mode, "temperature": np.float64(temperature), "seed": seed,
           "pad_tail": pad_tail, "txt_lens": np.array(lens), "hidden_cls": hid[:, 0, :32].numpy(),
           "hidden_absmean": hid.abs().mean().numpy(), "hidden_shape": np.array(hid.shape)}
    rec.update(tap.records)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] T={temperature} mode={mode} txt_lens={lens}")


def med_layer_grad_case(name, B, L, temperature, layer=0, seed=0, pad_tail=0, nsample=512, mode="text", Nimg=0):
    """SURVEY 8(f) rank 4 (backward), text side: the reference's OWN autograd through models/med.py BertLayer.forward (mode
    'text': self-attention with the padding mask, output LayerNorm, Reduce_token on the post-LN tokens, FFN; mode 'multimodal':
    cross-attention to synthetic image tokens between the pruning step and the FFN, the tokens a leaf as well) for one layer.  The
    layer's input, additive mask and token_attn are captured from a no-grad forward of the reference BertModel (pre-hook of layer
    `layer`, token_attn cloned before Reduce_token divides it in place, med.py:360), then the layer runs again alone with
    hidden_states and token_attn as leaves and loss = oracle.vit_loss(out, g, h) (token-order invariant).  Recorded: the pruning
    decision and of every gradient (hidden, token_attn, the layer's 16 parameters) its L2 norm, sum and sampled entries."""
    import models.med as rmed
    from madtp_amd import specs
    from oracle import madtp_oracle as O
    cfg = rmed.BertConfig.from_json_file("configs/med_config.json")
    cfg.encoder_width = 768
    cfg.evaluate = True
    model = rmed.BertModel(config=cfg, add_pooling_layer=False)
    model.eval()
    msg = model.load_state_dict(specs.synth_weights(specs.bert_shapes("", "med"), seed), strict=False)
    assert not msg.unexpected_keys
    space_dict = synth.synth_tensor("space_dict", (100, 768), seed)
    ids = synth.synth_token_ids(B, L, seed + 1)
    att = torch.ones_like(ids)
    if pad_tail:
        for b in range(B):
            att[b, L - (b % (pad_tail + 1)):] = 0
    cap = {}
    lay = model.encoder.layer[layer]
    hk = lay.register_forward_pre_hook(lambda m, a, kw: cap.update(h=a[0].detach().clone(), mask=a[1].detach().clone(),
                                                                    ta=kw["token_attn"].detach().clone()), with_kwargs=True)
    enc = synth.synth_tensor("image_embeds", (B, Nimg, 768), seed).mul(25.0) if mode == "multimodal" else None
    enc_att = torch.ones(B, Nimg, dtype=torch.long) if enc is not None else None
    with torch.no_grad():
        model(ids, attention_mask=att, encoder_hidden_states=enc, encoder_attention_mask=enc_att, return_dict=True, mode=mode,
              space_dict=space_dict, temperature=temperature)
    hk.remove()
    hid = cap["h"].clone().requires_grad_(True)
    ta = cap["ta"].clone().requires_grad_(True)
    encl = enc.clone().requires_grad_(True) if enc is not None else None
    enc_mask = model.invert_attention_mask(enc_att) if enc is not None else None
    tap = GatherTap(rmed)
    tap.set_tag("lay")
    for p_ in lay.parameters():
        p_.grad = None
    out = lay(hid, cap["mask"], None, encl, enc_mask, None, False, mode=mode, space_dict=space_dict, token_attn=ta * 1.0,
              reduce_num=0, temperature=temperature)
    tap.restore()
    y = out[0]
    g = torch.from_numpy(synth.uniform_pm1("vitgrad_g", B * 768, seed).reshape(B, 768))
    h = torch.from_numpy(synth.uniform_pm1("vitgrad_h", B * 768, seed).reshape(B, 768))
    O.vit_loss(y, g, h).backward()
    rec = {"kind": "med_layer_grad", "B": B, "L": L, "temperature": np.float64(temperature), "seed": seed, "layer": layer,
           "pad_tail": pad_tail, "nsample": nsample, "out_shape": np.array(y.shape), "mode": mode, "Nimg": Nimg,
           "y_norm": np.float64(y.detach().double().norm().item()), "mask_out": out[-1].detach()[:, 0, 0, :].numpy(),
           "h_head": cap["h"][:, :2, :8].numpy(), "ta_head": cap["ta"][:, :2, :8].numpy()}
    rec.update(tap.records)
    grads = {"hidden": hid.grad, "token_attn": ta.grad}
    if encl is not None:
        grads["enc"] = encl.grad
    grads.update({k: v.grad for k, v in lay.named_parameters() if v.grad is not None})
    assert ta.grad is not None and y.shape[1] < L, f"layer not pruned at T={temperature}: output {tuple(y.shape)}"
    for k, gr in grads.items():
        flat = gr.detach().reshape(-1)
        idx = grad_sample_index(flat.numel(), nsample)
        rec[f"g_{k}_sample"] = flat[torch.from_numpy(idx)].numpy()
        rec[f"g_{k}_norm"] = np.float64(flat.double().norm().item())
        rec[f"g_{k}_sum"] = np.float64(flat.double().sum().item())
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] layer {layer} T={temperature} out {tuple(y.shape)} {len(grads)} gradients: {sorted(grads)[:4]}... "
          f"|dh| {rec['g_hidden_norm']:.4e} |dta| {rec['g_token_attn_norm']:.4e} records {sorted(tap.records)}")


def nlvr_layer_grad_case(name, B, L, temperature, layer, seed=0, pad_tail=0, nsample=384, Nimg=40):
    """SURVEY 8(f) rank 4 (backward), the headline's text layer: the reference's OWN autograd through models/nlvr_encoder.py
    BertLayer.forward (mode 'multimodal': masked self-attention, output LayerNorm, Reduce_token, TWIN cross-attention to two image
    token sequences - averaged below layer 6, merged by merge_layer from layer 6 on - FFN).  The layer's inputs are captured from a
    no-grad forward of the reference BertModel; the layer then runs alone with hidden_states, token_attn and both image sequences as
    leaves, loss = oracle.vit_loss(out, g, h)."""
    import models.nlvr_encoder as rnl
    import models.med as rmed
    from madtp_amd import specs
    from oracle import madtp_oracle as O
    cfg = rmed.BertConfig.from_json_file("configs/med_config.json")
    cfg.encoder_width = 768
    cfg.evaluate = True
    model = rnl.BertModel(config=cfg, add_pooling_layer=False)
    model.eval()
    msg = model.load_state_dict(specs.synth_weights(specs.bert_shapes("", "nlvr"), seed), strict=False)
    assert not msg.unexpected_keys, msg
    space_dict = synth.synth_tensor("space_dict", (100, 768), seed)
    ids = synth.synth_token_ids(B, L, seed + 1)
    att = torch.ones_like(ids)
    if pad_tail:
        for b in range(B):
            att[b, L - (b % (pad_tail + 1)):] = 0
    encs = [synth.synth_tensor(f"image_embeds{i}", (B, Nimg, 768), seed).mul(25.0) for i in range(2)]
    enc_atts = [torch.ones(B, Nimg, dtype=torch.long) for _ in range(2)]
    cap = {}
    lay = model.encoder.layer[layer]
    hk = lay.register_forward_pre_hook(lambda m, a, kw: cap.update(h=a[0].detach().clone(), mask=a[1].detach().clone(),
                                                                    emask=[t.detach().clone() for t in a[5]],
                                                                    ta=kw["token_attn"].detach().clone()), with_kwargs=True)
    with torch.no_grad():
        model(ids, attention_mask=att, encoder_hidden_states=encs, encoder_attention_mask=enc_atts, return_dict=True,
              mode="multimodal", space_dict=space_dict, temperature=temperature)
    hk.remove()
    hid = cap["h"].clone().requires_grad_(True)
    ta = cap["ta"].clone().requires_grad_(True)
    encl = [e.clone().requires_grad_(True) for e in encs]
    tap = GatherTap(rnl)
    tap.set_tag("lay")
    for p_ in lay.parameters():
        p_.grad = None
    out = lay(hid, cap["mask"], space_dict, None, encl, cap["emask"], None, False, mode="multimodal", token_attn=ta * 1.0,
              reduce_num=0, temperature=temperature)
    tap.restore()
    y = out[0]
    g = torch.from_numpy(synth.uniform_pm1("vitgrad_g", B * 768, seed).reshape(B, 768))
    h = torch.from_numpy(synth.uniform_pm1("vitgrad_h", B * 768, seed).reshape(B, 768))
    O.vit_loss(y, g, h).backward()
    rec = {"kind": "nlvr_layer_grad", "B": B, "L": L, "temperature": np.float64(temperature), "seed": seed, "layer": layer,
           "pad_tail": pad_tail, "nsample": nsample, "out_shape": np.array(y.shape), "Nimg": Nimg,
           "y_norm": np.float64(y.detach().double().norm().item()), "mask_out": out[-1].detach()[:, 0, 0, :].numpy(),
           "h_head": cap["h"][:, :2, :8].numpy(), "ta_head": cap["ta"][:, :2, :8].numpy()}
    rec.update(tap.records)
    grads = {"hidden": hid.grad, "token_attn": ta.grad, "enc0": encl[0].grad, "enc1": encl[1].grad}
    grads.update({k: v.grad for k, v in lay.named_parameters() if v.grad is not None})
    assert ta.grad is not None and y.shape[1] < L, f"layer not pruned at T={temperature}: output {tuple(y.shape)}"
    for k, gr in grads.items():
        flat = gr.detach().reshape(-1)
        idx = grad_sample_index(flat.numel(), nsample)
        rec[f"g_{k}_sample"] = flat[torch.from_numpy(idx)].numpy()
        rec[f"g_{k}_norm"] = np.float64(flat.double().norm().item())
        rec[f"g_{k}_sum"] = np.float64(flat.double().sum().item())
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] layer {layer} T={temperature} out {tuple(y.shape)} {len(grads)} gradients |dh| {rec['g_hidden_norm']:.4e} "
          f"|denc0| {rec['g_enc0_norm']:.4e} records {sorted(tap.records)}")


def vit_case(name, B, size, temperature, seed=0):
    """models/vit.py VisionTransformer stand-alone at a large image size (384 -> 577 tokens: retrieval/NLVR yaml
    configs; 480 -> 901 tokens: configs/vqa.yaml)."""
    import models.vit as rvit
    from madtp_amd import specs
    model = rvit.VisionTransformer(img_size=size, patch_size=16, embed_dim=768, depth=12, num_heads=12, evaluate=True, sd_dim=768)
    model.eval()
    sd = specs.synth_weights(specs.vit_shapes("", size), seed)
    model.load_state_dict(sd, strict=True)
    images = synth.synth_images(B, size, seed)
    space_dict = synth.synth_tensor("space_dict", (100, 768), seed)
    tap = GatherTap(rvit)
    hooks, lens = [], []
    for i, blk in enumerate(model.blocks):
        hooks.append(blk.register_forward_pre_hook(lambda m, a, i=i: tap.set_tag(f"vit{i}")))
        hooks.append(blk.register_forward_hook(lambda m, a, o: lens.append(o.shape[1])))
    with torch.no_grad():
        out, sd_ft = model(images, space_dict=space_dict, temperature=temperature)
    for h in hooks:
        h.remove()
    tap.restore()
    rec = {"kind": "vit", "B": B, "size": size, "temperature": np.float64(temperature), "seed": seed,
           "vit_lens": np.array(lens), "cls": out[:, 0, :32].numpy(), "out_shape": np.array(out.shape),
           "sd_ft_head": sd_ft[:, :4, :16].numpy()}
    rec.update({k: v for k, v in tap.records.items() if k.endswith("_idx")})
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] size={size} T={temperature} vit_lens={lens}")


def grad_sample_index(numel, n=1024, stride=7919):
    """deterministic sample positions of a flattened gradient tensor (shared with tests/test_oracle_golden.py and the GPU test)"""
    return (np.arange(min(n, numel), dtype=np.int64) * stride) % numel


def vit_block_grad_case(name, B, size, temperature, layer=0, seed=0):
    """the reference's OWN autograd through models/vit.py Block.forward for one layer.  The block
    input x and the query model's token_attn are captured from a no-grad forward of the reference VisionTransformer (pre-hook of
    block `layer`, cloned before Reduce_token divides token_attn in place, vit.py:137), then block `layer` runs again alone with
    x and token_attn as leaves and loss = sum(y * G); recorded: the pruning decision, and of every gradient (x, token_attn, the 12
    parameters) its L2 norm, its sum and 1024 sampled entries (grad_sample_index) - data only."""
    import models.vit as rvit
    from madtp_amd import specs
    model = rvit.VisionTransformer(img_size=size, patch_size=16, embed_dim=768, depth=12, num_heads=12, evaluate=True, sd_dim=768)
    model.eval()
    model.load_state_dict(specs.synth_weights(specs.vit_shapes("", size), seed), strict=True)
    images = synth.synth_images(B, size, seed)
    space_dict = synth.synth_tensor("space_dict", (100, 768), seed)
    cap = {}
    blk = model.blocks[layer]
    h = blk.register_forward_pre_hook(lambda m, a: cap.update(x=a[0].detach().clone(), ta=a[4].detach().clone()))
    with torch.no_grad():
        model(images, space_dict=space_dict, temperature=temperature)
    h.remove()
    x = cap["x"].clone().requires_grad_(True)
    ta = cap["ta"].clone().requires_grad_(True)
    tap = GatherTap(rvit)
    tap.set_tag("blk")
    for p_ in blk.parameters():
        p_.grad = None
    y = blk(x, False, 0, temperature, ta * 1.0)   # (ta * 1.0: the block divides its argument in place; keep the leaf intact)
    tap.restore()
    G = torch.from_numpy(synth.uniform_pm1("grad_out", y.numel(), seed).reshape(tuple(y.shape)))
    (y * G).sum().backward()
    rec = {"kind": "vit_block_grad", "B": B, "size": size, "temperature": np.float64(temperature), "seed": seed, "layer": layer,
           "out_shape": np.array(y.shape), "y_head": y.detach()[:, :3, :16].numpy(), "blk_idx": tap.records["blk_idx"],
           "x_head": cap["x"][:, :2, :8].numpy(), "ta_head": cap["ta"][:, :2, :8].numpy()}
    grads = {"x": x.grad, "token_attn": ta.grad}
    grads.update({k: v.grad for k, v in blk.named_parameters()})
    for k, g in grads.items():
        flat = g.detach().reshape(-1)
        idx = grad_sample_index(flat.numel())
        rec[f"g_{k}_sample"] = flat[torch.from_numpy(idx)].numpy()
        rec[f"g_{k}_norm"] = np.float64(flat.double().norm().item())
        rec[f"g_{k}_sum"] = np.float64(flat.double().sum().item())
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] layer {layer} T={temperature} out {tuple(y.shape)} |dx| {rec['g_x_norm']:.4e} |dta| {rec['g_token_attn_norm']:.4e}")


def vit_grad_case(name, B, size, temperature, seed=0, nsample=256):
    """SURVEY 8(f) rank 4 (backward), the whole encoder: the reference's OWN autograd through models/vit.py
    VisionTransformer.forward (12 pruned blocks, query-model logits, patch embedding, final LayerNorm) with every parameter and
    space_dict as leaves, loss = oracle.vit_loss(y, g, h) (token-order invariant) + sum(sd_img_ft_all * a).  Recorded: per-layer lengths and kept sets, the
    output's head, and of every gradient its L2 norm, sum and `nsample` sampled entries (grad_sample_index) - data only."""
    import models.vit as rvit
    from madtp_amd import specs
    from oracle import madtp_oracle as O
    model = rvit.VisionTransformer(img_size=size, patch_size=16, embed_dim=768, depth=12, num_heads=12, evaluate=True, sd_dim=768)
    model.eval()
    model.load_state_dict(specs.synth_weights(specs.vit_shapes("", size), seed), strict=True)
    images = synth.synth_images(B, size, seed)
    space_dict = synth.synth_tensor("space_dict", (100, 768), seed).clone().requires_grad_(True)
    g = torch.from_numpy(synth.uniform_pm1("vitgrad_g", B * 768, seed).reshape(B, 768))
    h = torch.from_numpy(synth.uniform_pm1("vitgrad_h", B * 768, seed).reshape(B, 768))
    tap = GatherTap(rvit)
    hooks, lens = [], []
    for i, blk in enumerate(model.blocks):
        hooks.append(blk.register_forward_pre_hook(lambda m, a, i=i: tap.set_tag(f"vit{i}")))
        hooks.append(blk.register_forward_hook(lambda m, a, o: lens.append(o.shape[1])))
    for p_ in model.parameters():
        p_.grad = None
    a = torch.from_numpy(synth.uniform_pm1("vitgrad_a", B * 100 * 768, seed).reshape(B, 100, 768))
    y, sd_all = model(images, space_dict=space_dict, temperature=temperature)
    for hk in hooks:
        hk.remove()
    tap.restore()
    (O.vit_loss(y, g, h) + (sd_all * a).sum()).backward()   # both outputs of VisionTransformer.forward enter the loss
    rec = {"kind": "vit_grad", "B": B, "size": size, "temperature": np.float64(temperature), "seed": seed, "nsample": nsample,
           "vit_lens": np.array(lens), "out_shape": np.array(y.shape), "y_norm": np.float64(y.detach().double().norm().item()),
           "sd_all_norm": np.float64(sd_all.detach().double().norm().item()), "loss_has_sd_all": 1,
           "loss": np.float64(O.vit_loss(y.detach().double(), g.double(), h.double()).item())}
    rec.update(tap.records)
    grads = {"space_dict": space_dict.grad}
    grads.update({k: v.grad for k, v in model.named_parameters() if v.grad is not None})
    for k, gr in grads.items():
        flat = gr.detach().reshape(-1)
        idx = grad_sample_index(flat.numel(), nsample)
        rec[f"g_{k}_sample"] = flat[torch.from_numpy(idx)].numpy()
        rec[f"g_{k}_norm"] = np.float64(flat.double().norm().item())
        rec[f"g_{k}_sum"] = np.float64(flat.double().sum().item())
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] T={temperature} lens {lens} {len(grads)} gradients, |d space_dict| {rec['g_space_dict_norm']:.4e} "
          f"|d pos_embed| {rec['g_pos_embed_norm']:.4e}")


def clip_case(name, B, temperature, seed=0, size=224):
    """clip/model.py VisionTransformer (ViT-B/16 geometry) with clip/mock.py's patched MultiheadAttention."""
    import clip.mock  # noqa: F401  (monkey-patches torch.nn.MultiheadAttention, as the reference does on import)
    import clip.model as cm
    from madtp_amd import specs
    model = cm.VisionTransformer(input_resolution=size, patch_size=16, width=768, layers=12, heads=12, output_dim=512, sd_dim=768)
    model.eval()
    sd = specs.synth_weights(specs.clip_vit_shapes("", size), seed)
    model.load_state_dict(sd, strict=True)
    images = synth.synth_images(B, size, seed)
    space_dict = synth.synth_tensor("space_dict", (100, 768), seed)
    tap = GatherTap(cm)
    hooks, lens = [], []
    for i, blk in enumerate(model.transformer.resblocks):
        hooks.append(blk.register_forward_pre_hook(lambda m, a, i=i: tap.set_tag(f"vit{i}")))
        hooks.append(blk.register_forward_hook(lambda m, a, o: lens.append(o[0].shape[0])))
    with torch.no_grad():
        feat, sd_ft = model(images, space_dict, temperature, 1)
    for h in hooks:
        h.remove()
    tap.restore()
    rec = {"kind": "clip_vit", "B": B, "size": size, "temperature": np.float64(temperature), "seed": seed,
           "vit_lens": np.array(lens), "features": feat.numpy(), "sd_ft_head": sd_ft[:, :4, :16].numpy(),
           "state_dict_keys": np.array(sorted(sd.keys()))}
    rec.update(tap.records)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] T={temperature} vit_lens={lens}")


def clip_block_grad_case(name, B, temperature, layer, seed=0, size=96, nsample=512):
    """SURVEY 8(f) rank 4 (backward), CLIP: the reference's OWN autograd through clip/model.py ResidualAttentionBlock.forward (with
    clip/mock.py's patched MultiheadAttention) for one block of the vision tower.  The block's input tuple is captured from a
    no-grad forward of the reference VisionTransformer; the block then runs alone with x [N,B,C] and space_dict as leaves and
    sd_ft_all = None, loss = oracle.vit_loss on the output tokens (order invariant) + sum(sd_ft * a).  The block owns its query
    model (q_map: a Linear in front of the logits), whose parameters are recorded too."""
    import clip.mock  # noqa: F401
    import clip.model as cm
    from madtp_amd import specs
    from oracle import madtp_oracle as O
    model = cm.VisionTransformer(input_resolution=size, patch_size=16, width=768, layers=12, heads=12, output_dim=512, sd_dim=768)
    model.eval()
    model.load_state_dict(specs.synth_weights(specs.clip_vit_shapes("", size), seed), strict=True)
    images = synth.synth_images(B, size, seed)
    space_dict = synth.synth_tensor("space_dict", (100, 768), seed)
    cap = {}
    blk = model.transformer.resblocks[layer]
    hk = blk.register_forward_pre_hook(lambda m, a: cap.update(x=a[0][0].detach().clone(), max_keep=a[0][4]))
    with torch.no_grad():
        model(images, space_dict, temperature, 1)
    hk.remove()
    x = cap["x"].clone().requires_grad_(True)
    sdl = space_dict.clone().requires_grad_(True)
    tap = GatherTap(cm)
    tap.set_tag("blk")
    for p_ in blk.parameters():
        p_.grad = None
    y, _, _, sd_ft, _ = blk((x, sdl, temperature, None, cap["max_keep"]))
    tap.restore()
    yb = y.permute(1, 0, 2)
    g = torch.from_numpy(synth.uniform_pm1("vitgrad_g", B * 768, seed).reshape(B, 768))
    h = torch.from_numpy(synth.uniform_pm1("vitgrad_h", B * 768, seed).reshape(B, 768))
    a = torch.from_numpy(synth.uniform_pm1("vitgrad_a", B * 100 * 768, seed).reshape(B, 100, 768))
    (O.vit_loss(yb, g, h) + (sd_ft * a).sum()).backward()
    rec = {"kind": "clip_block_grad", "B": B, "size": size, "temperature": np.float64(temperature), "seed": seed, "layer": layer,
           "nsample": nsample, "max_keep": int(cap["max_keep"]), "out_shape": np.array(yb.shape),
           "y_norm": np.float64(yb.detach().double().norm().item()), "x_head": cap["x"].permute(1, 0, 2)[:, :2, :8].numpy(),
           "sd_ft_norm": np.float64(sd_ft.detach().double().norm().item())}
    rec.update(tap.records)
    grads = {"x": x.grad.permute(1, 0, 2).contiguous(), "space_dict": sdl.grad}
    grads.update({k: v.grad for k, v in blk.named_parameters() if v.grad is not None})
    for k, gr in grads.items():
        flat = gr.detach().reshape(-1)
        idx = grad_sample_index(flat.numel(), nsample)
        rec[f"g_{k}_sample"] = flat[torch.from_numpy(idx)].numpy()
        rec[f"g_{k}_norm"] = np.float64(flat.double().norm().item())
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] layer {layer} T={temperature} in {tuple(cap['x'].shape)} out {tuple(y.shape)} {len(grads)} gradients: "
          f"{sorted(grads)} records {sorted(tap.records)}")


def clip_vit_grad_case(name, B, temperature, seed=0, size=96, nsample=192, patch=16, width=768, layers=12, out_dim=512):
    """SURVEY 8(f) rank 4 (backward), CLIP's vision tower end to end: the reference's OWN autograd through clip/model.py
    VisionTransformer.forward (conv1, class / positional embedding, ln_pre, twelve pruned blocks each with its own query model,
    ln_post, proj) with every parameter and space_dict as leaves, loss = sum(features * c) + sum(sd_img_ft_all * a)."""
    import clip.mock  # noqa: F401
    import clip.model as cm
    from madtp_amd import specs
    model = cm.VisionTransformer(input_resolution=size, patch_size=patch, width=width, layers=layers, heads=width // 64,
                                 output_dim=out_dim, sd_dim=768)
    model.eval()
    model.load_state_dict(specs.synth_weights(specs.clip_vit_shapes("", size, patch, width, layers, out_dim), seed), strict=True)
    images = synth.synth_images(B, size, seed)
    space_dict = synth.synth_tensor("space_dict", (100, 768), seed).clone().requires_grad_(True)
    lens, hooks = [], []
    for blk in model.transformer.resblocks:
        hooks.append(blk.register_forward_hook(lambda m, a, o: lens.append(o[0].shape[0])))
    for p_ in model.parameters():
        p_.requires_grad_(True)
        p_.grad = None
    feat, sd_all = model(images, space_dict, temperature, 1)
    for h in hooks:
        h.remove()
    c = torch.from_numpy(synth.uniform_pm1("clipgrad_c", B * out_dim, seed).reshape(B, out_dim))
    a = torch.from_numpy(synth.uniform_pm1("vitgrad_a", B * 100 * 768, seed).reshape(B, 100, 768))
    ((feat * c).sum() + (sd_all * a).sum()).backward()
    rec = {"kind": "clip_vit_grad", "B": B, "size": size, "temperature": np.float64(temperature), "seed": seed, "nsample": nsample,
           "patch": patch, "width": width, "layers": layers, "out_dim": out_dim,
           "vit_lens": np.array(lens), "features": feat.detach().numpy(), "sd_all_norm": np.float64(sd_all.detach().double().norm().item())}
    grads = {"space_dict": space_dict.grad}
    grads.update({k: v.grad for k, v in model.named_parameters() if v.grad is not None})
    for k, gr in grads.items():
        flat = gr.detach().reshape(-1)
        idx = grad_sample_index(flat.numel(), nsample)
        rec[f"g_{k}_sample"] = flat[torch.from_numpy(idx)].numpy()
        rec[f"g_{k}_norm"] = np.float64(flat.double().norm().item())
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] T={temperature} lens {lens} {len(grads)} gradients")


def clip_text_block_grad_case(name, B, N, temperature, max_keep, seed=0, nsample=512):
    """As clip_block_grad_case for a block of CLIP's TEXT tower (width 512, 8 heads, causal attn_mask [77,77] applied as
    mask[:N,:N], clip/mock.py:309-310): a stand-alone reference ResidualAttentionBlock with synthetic weights on a synthetic token
    tensor x [N,B,512] - exercises the causal mask together with the pruning score terms in the attention backward."""
    import clip.mock  # noqa: F401
    import clip.model as cm
    from oracle import madtp_oracle as O
    mask = torch.empty(77, 77).fill_(float("-inf")).triu_(1)   # CLIP.build_attention_mask (clip/model.py:383-389)
    blk = cm.ResidualAttentionBlock(512, 8, mask, sd_dim=768)
    blk.eval()
    blk.load_state_dict(synth.fill_state_dict(blk, seed, prefix="clip_text_block."), strict=True)
    x = synth.synth_tensor("clip_text_x", (N, B, 512), seed).clone().requires_grad_(True)
    sdl = synth.synth_tensor("space_dict", (100, 768), seed).clone().requires_grad_(True)
    tap = GatherTap(cm)
    tap.set_tag("blk")
    y, _, _, sd_ft, _ = blk((x, sdl, temperature, None, max_keep))
    tap.restore()
    yb = y.permute(1, 0, 2)
    g = torch.from_numpy(synth.uniform_pm1("vitgrad_g", B * 512, seed).reshape(B, 512))
    h = torch.from_numpy(synth.uniform_pm1("vitgrad_h", B * 512, seed).reshape(B, 512))
    a = torch.from_numpy(synth.uniform_pm1("vitgrad_a", B * 100 * 768, seed).reshape(B, 100, 768))
    (O.vit_loss(yb, g, h) + (sd_ft * a).sum()).backward()
    assert yb.shape[1] < N, f"block not pruned at T={temperature}: {tuple(yb.shape)}"
    rec = {"kind": "clip_text_block_grad", "B": B, "N": N, "temperature": np.float64(temperature), "seed": seed, "nsample": nsample,
           "max_keep": int(max_keep), "out_shape": np.array(yb.shape), "y_norm": np.float64(yb.detach().double().norm().item()),
           "sd_ft_norm": np.float64(sd_ft.detach().double().norm().item())}
    rec.update(tap.records)
    grads = {"x": x.grad.permute(1, 0, 2).contiguous(), "space_dict": sdl.grad}
    grads.update({k: v.grad for k, v in blk.named_parameters() if v.grad is not None})
    for k, gr in grads.items():
        flat = gr.detach().reshape(-1)
        idx = grad_sample_index(flat.numel(), nsample)
        rec[f"g_{k}_sample"] = flat[torch.from_numpy(idx)].numpy()
        rec[f"g_{k}_norm"] = np.float64(flat.double().norm().item())
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] T={temperature} in ({N},{B},512) out {tuple(y.shape)} {len(grads)} gradients")


def clip_full_case(name, B, temperature, seed=0, size=224, min_len=6, max_len=40, patch=16, vision_width=768, vision_layers=12,
                   embed_dim=512, text_width=512):
    """clip/model.py CLIP (ViT-B/16 geometry by default, text width 512 / 8 heads / 12 layers / ctx 77; ViT-L/14@336: patch 14,
    vision width 1024 / 24 layers, embed_dim 768, text width 768 / 12 heads): the reference's own encode_image / encode_text
    (compress_retrieval_clip_dtp.py:92,100 call sites) with clip/mock.py's patched MHA."""
    import clip.mock  # noqa: F401
    import clip.model as cm
    from madtp_amd import specs
    model = cm.CLIP(embed_dim, size, vision_layers, vision_width, patch, 77, 49408, text_width, text_width // 64, 12, True, None)
    model.eval()
    sd = specs.synth_weights(specs.clip_shapes(size, patch, vision_width, vision_layers, embed_dim, text_width, 12), seed)
    msg = model.load_state_dict(sd, strict=False)
    assert not msg.unexpected_keys, msg.unexpected_keys
    assert all(k.endswith("_m") or "_m." in k or "queue" in k for k in msg.missing_keys), msg.missing_keys[:8]
    images = synth.synth_images(B, size, seed)
    text = synth.synth_clip_tokens(B, 77, seed, min_len, max_len)
    tap = GatherTap(cm)
    hooks, vlens, tlens = [], [], []
    for i, blk in enumerate(model.visual.transformer.resblocks):
        hooks.append(blk.register_forward_pre_hook(lambda m, a, i=i: tap.set_tag(f"vit{i}")))
        hooks.append(blk.register_forward_hook(lambda m, a, o: vlens.append(o[0].shape[0])))
    for i, blk in enumerate(model.transformer.resblocks):
        hooks.append(blk.register_forward_pre_hook(lambda m, a, i=i: tap.set_tag(f"txt{i}")))
        hooks.append(blk.register_forward_hook(lambda m, a, o: tlens.append(o[0].shape[0])))
    with torch.no_grad():
        img_feat, sd_img = model.encode_image(images, model.space_dict, temperature)
        txt_feat, sd_txt = model.encode_text(text, model.space_dict, temperature)
    for h in hooks:
        h.remove()
    tap.restore()
    rec = {"kind": "clip_full", "B": B, "size": size, "temperature": np.float64(temperature), "seed": seed,
           "min_len": min_len, "max_len": max_len, "patch": patch, "vision_width": vision_width, "vision_layers": vision_layers,
           "embed_dim": embed_dim, "text_width": text_width,
           "sd_img_norm": np.float64(sd_img.double().norm().item()), "sd_txt_norm": np.float64(sd_txt.double().norm().item()),
           "vit_lens": np.array(vlens), "txt_lens": np.array(tlens),
           "image_features": img_feat.numpy(), "text_features": txt_feat.numpy(), "eot_pos": text.argmax(-1).numpy(),
           "sd_img_head": sd_img[:, :4, :16].numpy(), "sd_txt_head": sd_txt[:, :4, :16].numpy(),
           "state_dict_keys": np.array(sorted(k for k in model.state_dict().keys()))}
    rec.update(tap.records)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] T={temperature} vit_lens={vlens} txt_lens={tlens} eot={text.argmax(-1).tolist()}")


def retrieval_case(name, n_img, img_bs, n_txt, size, temperature, k_test, seed=0):
    """compress_retrieval_dtp.py evaluate() - the reference's own function, imported behind the shims - on a synthetic
    evaluation set: text features (text mode), image features with the cross-batch CLS-repeat padding, similarity
    matrix, ITM re-ranking of the top k_test candidates in both directions."""
    import types
    import compress_retrieval_dtp as crd
    import models.blip_retrieval as rbr
    from madtp_amd import harness, specs
    ref_shims.patch_tokenizer(rbr)
    model = rbr.BLIP_Retrieval(image_size=size, vit="base", queue_size=8, evaluate=True)
    model.eval()
    sd = specs.synth_weights(specs.blip_retrieval_shapes(size), seed)
    msg = model.load_state_dict(sd, strict=False)
    used = ("visual_encoder.", "text_encoder.", "vision_proj.", "text_proj.", "itm_head.", "space_dict")
    assert not msg.unexpected_keys, msg.unexpected_keys
    assert all((not k.startswith(used)) or "query_model" in k or "position_ids" in k for k in msg.missing_keys), \
        [k for k in msg.missing_keys if k.startswith(used)]
    batches, ids, att = harness.retrieval_inputs(n_img, img_bs, n_txt, size, 35, seed)

    class Texts:  # data_loader.dataset.text: len() and slicing -> what FakeTokenizer passes through
        def __len__(self): return n_txt
        def __getitem__(self, sl): return {"input_ids": ids[sl], "attention_mask": att[sl]}

    class Loader:
        dataset = types.SimpleNamespace(text=Texts(), image=list(range(n_img)))
        def __len__(self): return len(batches)
        def __iter__(self):
            for b, img in enumerate(batches):
                yield img, ["caption"] * img.shape[0], torch.arange(img.shape[0]) + b * img_bs

    lens = []
    hook = model.visual_encoder.register_forward_hook(lambda m, a, o: lens.append(o[0].shape[1]))
    crd.args = types.SimpleNamespace(distributed=False)
    t0 = time.time()
    i2t, t2i, _ = crd.evaluate(model, Loader(), torch.device("cpu"), {"k_test": k_test, "alpha": 0.4}, temperature)
    dt = time.time() - t0
    hook.remove()
    rec = {"kind": "retrieval", "n_img": n_img, "img_bs": img_bs, "n_txt": n_txt, "size": size, "k_test": k_test,
           "temperature": np.float64(temperature), "seed": seed, "score_i2t": i2t, "score_t2i": t2i,
           "vit_out_lens": np.array(lens), "ref_seconds": dt, "state_dict_keys": np.array(sorted(sd.keys()))}
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] T={temperature} vit_out_lens={lens} i2t[0]={np.round(i2t[0], 3).tolist()} ({dt:.1f}s)")


def vqa_rank_case(name, B, size, L, temperature, n_answers, answer_len, k_test, seed=0, pad_tail=0):
    """models/blip_vqa.py BLIP_VQA.forward(train=False, inference='rank') (:57-64, :117-154) -> rank_answer (:156-203): the
    reference's own encoder leg, answer decoder (models/med.py BertLMHeadModel, teacher-forced) and candidate ranking.  The LM
    head's output embedding / bias are given the values of the entries they alias in any saved checkpoint (specs.TIED_KEYS):
    the import shim turns transformers' tie_weights() into a no-op."""
    import models.blip_vqa as bv
    from madtp_amd import harness, specs
    ref_shims.patch_tokenizer(bv)
    model = bv.BLIP_VQA(image_size=size, evaluate=True, config={"sd_num": 100, "sd_dim": 768, "batch_size_train": 16})
    model.eval()
    sd = specs.tie_keys(synth.fill_state_dict(model, seed))
    model.load_state_dict(sd, strict=True)
    images = synth.synth_images(B, size, seed)
    ids = synth.synth_token_ids(B, L, seed, first_id=None)
    att = harness.padded_mask(B, L, pad_tail)
    a_ids, a_att = synth.synth_answer_ids(n_answers, answer_len, seed)
    calls = []
    orig = model.text_decoder.forward

    def tapped(*a, **k):
        out = orig(*a, **k)
        calls.append({"logits": out.logits.detach(), "loss": None if out.loss is None else out.loss.detach(),
                      "input_ids": a[0].detach().clone()})
        return out
    model.text_decoder.forward = tapped
    lens_v, lens_t, hooks = [], [], []
    for blk in model.visual_encoder.blocks:
        hooks.append(blk.register_forward_hook(lambda m, a, o: lens_v.append(o.shape[1])))
    for lay in model.text_encoder.encoder.layer:
        hooks.append(lay.register_forward_hook(lambda m, a, o: lens_t.append(o[0].shape[1])))
    t0 = time.time()
    with torch.no_grad():
        max_ids = model(images, {"input_ids": ids, "attention_mask": att},
                        ref_shims.FakeTokenizer._Batch({"input_ids": a_ids, "attention_mask": a_att}),
                        temperature=temperature, train=False, inference='rank', k_test=k_test)
    dt = time.time() - t0
    for h in hooks:
        h.remove()
    model.text_decoder.forward = orig
    first_logits = calls[0]["logits"][:, 0, :]
    prob_first = torch.softmax(first_logits, dim=1).index_select(1, a_ids[:, 1])
    topk_probs, topk_ids = prob_first.topk(k_test, dim=1)
    assert torch.equal(calls[1]["input_ids"], torch.cat([a_ids.index_select(0, t) for t in topk_ids], 0))
    log_probs_sum = (-calls[1]["loss"]).view(B, k_test)
    dec_keys = sorted(k for k in sd.keys() if k.startswith("text_decoder."))
    out = {"kind": "vqa_rank", "B": B, "size": size, "L": L, "temperature": np.float64(temperature), "seed": seed,
           "pad_tail": pad_tail, "n_answers": n_answers, "answer_len": answer_len, "k_test": k_test,
           "vit_lens": np.array(lens_v), "txt_lens": np.array(lens_t), "max_ids": max_ids.numpy(),
           "topk_ids": topk_ids.numpy(), "topk_probs": topk_probs.numpy(), "prob_first_token": prob_first.numpy(),
           "log_probs_sum": log_probs_sum.numpy(), "first_logits_sample": first_logits[:, :64].numpy(),
           "first_logits_absmean": first_logits.abs().mean().numpy(),
           "decoder_state_dict_keys": np.array(dec_keys), "ref_seconds": dt, "threads": torch.get_num_threads()}
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(f"[{name}] T={temperature} vit_lens={lens_v} txt_lens={lens_t} max_ids={max_ids.tolist()} topk_ids={topk_ids.tolist()} "
          f"log_probs_sum[0]={np.round(log_probs_sum[0].numpy(), 3).tolist()} ({dt:.1f}s)")


def decoder_grad_case(name, B, L, Nq, seed=0, pad_tail=2, nsample=128):
    """SURVEY 8(f) rank 4 (backward), the answer / caption decoder: the reference's OWN autograd through models/med.py
    BertLMHeadModel.forward as blip_vqa.py:101-113 trains it - teacher-forced answers with a padded tail, labels = ids with the
    padding set to -100, cross-attention to question states [B,Nq,768] (a leaf as well), reduction='none', loss =
    sum(weights * per-sequence loss) / B.  Recorded: the per-sequence losses and of every gradient its norm and sampled entries."""
    import models.med as rmed
    from madtp_amd import specs
    cfg = rmed.BertConfig.from_json_file("configs/med_config.json")
    cfg.encoder_width = 768
    cfg.evaluate = True
    model = rmed.BertLMHeadModel(config=cfg)
    model.eval()
    sd = specs.tie_keys(synth.fill_state_dict(model, seed))
    model.load_state_dict(sd, strict=True)
    model.cls.predictions.decoder.weight = model.bert.embeddings.word_embeddings.weight   # (the shim makes tie_weights a no-op)
    ids = synth.synth_token_ids(B, L, seed + 3)
    att = torch.ones_like(ids)
    for b in range(B):
        att[b, L - (b % (pad_tail + 1)):] = 0
    labels = ids.masked_fill(att == 0, -100)
    enc = synth.synth_tensor("question_states", (B, Nq, 768), seed).clone().requires_grad_(True)
    enc_att = torch.ones(B, Nq, dtype=torch.long)
    w = torch.tensor([1.0, 0.5, 2.0, 1.5][:B])
    for p_ in model.parameters():
        p_.requires_grad_(True)
        p_.grad = None
    out = model(ids, attention_mask=att, encoder_hidden_states=enc, encoder_attention_mask=enc_att, labels=labels,
                return_dict=True, reduction='none')
    ((w * out.loss).sum() / B).backward()
    rec = {"kind": "decoder_grad", "B": B, "L": L, "Nq": Nq, "seed": seed, "pad_tail": pad_tail, "nsample": nsample,
           "loss": out.loss.detach().numpy(), "weights": w.numpy()}
    grads = {"enc": enc.grad}
    seen = set()
    for k, v in model.named_parameters():
        if v.grad is not None and id(v) not in seen:
            seen.add(id(v))
            grads[k] = v.grad
    for k, gr in grads.items():
        flat = gr.detach().reshape(-1)
        idx = grad_sample_index(flat.numel(), nsample)
        rec[f"g_{k}_sample"] = flat[torch.from_numpy(idx)].numpy()
        rec[f"g_{k}_norm"] = np.float64(flat.double().norm().item())
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] loss={out.loss.detach().numpy().round(4).tolist()} {len(grads)} gradients "
          f"|d word_embeddings| {rec['g_bert.embeddings.word_embeddings.weight_norm']:.4e} |d enc| {rec['g_enc_norm']:.4e}")


def vqa_train_case(name, B, size, L, temperature, n_list, answer_len, seed=0, pad_tail=1, nsample=48):
    """SURVEY 8(f) rank 4 (backward), the second task model end to end: the reference's OWN training step of models/blip_vqa.py
    BLIP_VQA.forward(train=True) (:66-115; model.eval(): no dropout) - pruned ViT, question encoder (MED, multimodal, pruned), answer
    decoder teacher-forced on the question states repeated n[b] times, loss = loss_vqa + 0.1 loss_fdt - with every parameter a leaf.
    Recorded: both losses, per-layer lengths, and of every gradient its norm and sampled entries."""
    import models.blip_vqa as bv
    from madtp_amd import harness, specs
    ref_shims.patch_tokenizer(bv)
    model = bv.BLIP_VQA(image_size=size, evaluate=True, config={"sd_num": 100, "sd_dim": 768, "batch_size_train": 16})
    model.eval()
    sd = specs.tie_keys(synth.fill_state_dict(model, seed))
    model.load_state_dict(sd, strict=True)
    model.text_decoder.cls.predictions.decoder.weight = model.text_decoder.bert.embeddings.word_embeddings.weight
    images = synth.synth_images(B, size, seed)
    ids = synth.synth_token_ids(B, L, seed, first_id=None)
    att = harness.padded_mask(B, L, pad_tail)
    a_ids, a_att = synth.synth_answer_ids(sum(n_list), answer_len, seed)
    weights = torch.tensor([0.6, 0.4, 1.0, 0.7, 0.3][:sum(n_list)])
    lens_v, lens_t, hooks = [], [], []
    for blk in model.visual_encoder.blocks:
        hooks.append(blk.register_forward_hook(lambda m, a, o: lens_v.append(o.shape[1])))
    for lay in model.text_encoder.encoder.layer:
        hooks.append(lay.register_forward_hook(lambda m, a, o: lens_t.append(o[0].shape[1])))
    for p_ in model.parameters():
        p_.requires_grad_(True)
        p_.grad = None
    loss_vqa, loss_fdt = model(images, {"input_ids": ids, "attention_mask": att},
                               ref_shims.FakeTokenizer._Batch({"input_ids": a_ids, "attention_mask": a_att}),
                               temperature=temperature, train=True, n=list(n_list), weights=weights)
    for h in hooks:
        h.remove()
    (loss_vqa + 0.1 * loss_fdt).backward()
    rec = {"kind": "vqa_train", "B": B, "size": size, "L": L, "temperature": np.float64(temperature), "seed": seed,
           "pad_tail": pad_tail, "nsample": nsample, "n_list": np.array(n_list), "answer_len": answer_len, "weights": weights.numpy(),
           "loss_vqa": np.float64(loss_vqa.item()), "loss_fdt": np.float64(loss_fdt.item()), "vit_lens": np.array(lens_v),
           "txt_lens": np.array(lens_t)}
    seen, n = set(), 0
    for k, v in model.named_parameters():
        if v.grad is None or id(v) in seen:
            continue
        seen.add(id(v))
        flat = v.grad.detach().reshape(-1)
        idx = grad_sample_index(flat.numel(), nsample)
        rec[f"g_{k}_sample"] = flat[torch.from_numpy(idx)].numpy()
        rec[f"g_{k}_norm"] = np.float64(flat.double().norm().item())
        n += 1
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] T={temperature} vit_lens={lens_v} txt_lens={lens_t} loss_vqa={loss_vqa.item():.4f} loss_fdt={loss_fdt.item():.4f} "
          f"{n} gradients")


def cap_train_case(name, B, size, L, temperature, seed=0, nsample=48):
    """SURVEY 8(f) rank 4 (backward), the caption model: the reference's OWN training step of models/blip.py
    BLIP_Decoder.forward(train=True) (:111-158; model.eval()) - pruned ViT, decoder teacher-forced on the caption (prompt positions
    and padding masked out of the targets), loss = loss_lm + 0.1 loss_fdt with loss_fdt = loss_lm (no text-side dictionary
    features) - with every parameter a leaf."""
    import models.blip as blip
    from madtp_amd import specs
    ref_shims.patch_tokenizer(blip)
    model = blip.BLIP_Decoder(image_size=size, evaluate=True, config={"sd_num": 100, "sd_dim": 768})
    model.eval()
    sd = specs.tie_keys(synth.fill_state_dict(model, seed))
    model.load_state_dict(sd, strict=True)
    model.text_decoder.cls.predictions.decoder.weight = model.text_decoder.bert.embeddings.word_embeddings.weight
    images = synth.synth_images(B, size, seed)
    ids = synth.synth_token_ids(B, L, seed + 5)
    ids[:, :4] = torch.tensor([101, 1037, 3861, 1997])   # "[CLS] a picture of" - the prompt every caption starts with
    att = torch.ones_like(ids)
    for b in range(B):
        if b % 2:
            ids[b, L - 3] = 102
            ids[b, L - 2:] = 0
            att[b, L - 2:] = 0
    lens_v, hooks = [], []
    for blk in model.visual_encoder.blocks:
        hooks.append(blk.register_forward_hook(lambda m, a, o: lens_v.append(o.shape[1])))
    for p_ in model.parameters():
        p_.requires_grad_(True)
        p_.grad = None
    loss_lm, loss_fdt = model(images, {"input_ids": ids.clone(), "attention_mask": att}, temperature=temperature, train=True)
    for h in hooks:
        h.remove()
    (loss_lm + 0.1 * loss_fdt).backward()
    rec = {"kind": "cap_train", "B": B, "size": size, "L": L, "temperature": np.float64(temperature), "seed": seed,
           "nsample": nsample, "loss_lm": np.float64(loss_lm.item()), "loss_fdt": np.float64(loss_fdt.item()),
           "vit_lens": np.array(lens_v), "prompt_length": int(model.prompt_length), "ids": ids.numpy(), "att": att.numpy()}
    seen, n = set(), 0
    for k, v in model.named_parameters():
        if v.grad is None or id(v) in seen:
            continue
        seen.add(id(v))
        flat = v.grad.detach().reshape(-1)
        idx = grad_sample_index(flat.numel(), nsample)
        rec[f"g_{k}_sample"] = flat[torch.from_numpy(idx)].numpy()
        rec[f"g_{k}_norm"] = np.float64(flat.double().norm().item())
        n += 1
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] T={temperature} vit_lens={lens_v} loss_lm={loss_lm.item():.4f} loss_fdt={loss_fdt.item():.4f} "
          f"prompt_length={model.prompt_length} {n} gradients")


def vqa_gen_case(name, B, size, L, temperature, eos_bias, seed=0, pad_tail=0):
    """models/blip_vqa.py BLIP_VQA.forward(train=False, inference='generate') (:117-147): the reference's encoder leg and its
    `text_decoder.generate(num_beams=3, max_length=10, min_length=1)` call, run under the installed transformers 5.15 with the
    shims of ref_shims.enable_generate().  eos_bias is added to the LM head's bias of [SEP] (and its tied alias): with random
    weights [SEP] never ranks among the 6 candidates otherwise and no hypothesis would ever finish before max_length.
    NOTE the search is 5.15's re-implementation: finished hypotheses are normalised by (length incl. EOS - prompt length) where
    4.15 (the reference's pinned version) divides by the length without the EOS, prompt included - the same number for this
    one-token prompt - but a beam that reaches max_length is scored / (max_length - 1) instead of / max_length, and the
    early-stop heuristic differs.  Recorded: the sequences and the per-step decoder inputs (which beams were expanded)."""
    import models.blip_vqa as bv
    from madtp_amd import harness, specs
    ref_shims.patch_tokenizer(bv)
    ref_shims.enable_generate()
    model = bv.BLIP_VQA(image_size=size, evaluate=True, config={"sd_num": 100, "sd_dim": 768, "batch_size_train": 16})
    model.eval()
    sd = synth.fill_state_dict(model, seed)
    sd["text_decoder.cls.predictions.bias"][102] += eos_bias
    sd = specs.tie_keys(sd)
    model.load_state_dict(sd, strict=True)
    images = synth.synth_images(B, size, seed)
    ids = synth.synth_token_ids(B, L, seed, first_id=None)
    att = harness.padded_mask(B, L, pad_tail)
    steps = []
    orig = model.text_decoder.forward

    import functools

    @functools.wraps(orig)  # (generate() validates model_kwargs against forward's signature)
    def tapped(*a, **k):
        out = orig(*a, **k)
        inp = k.get("input_ids", a[0] if a else None)
        steps.append({"input_ids": inp.detach().clone(), "last_logits": out.logits[:, -1, :].detach().clone()})
        return out
    model.text_decoder.forward = tapped
    raw = []
    gen = model.text_decoder.generate

    def tapped_gen(*a, **k):
        out = gen(*a, **k)
        raw.append(out.detach().clone())
        return out
    model.text_decoder.generate = tapped_gen
    t0 = time.time()
    with torch.no_grad():
        answers = model(images, {"input_ids": ids, "attention_mask": att}, None, temperature=temperature, train=False,
                        inference='generate')
    dt = time.time() - t0
    seqs = raw[0]
    T = max(s["input_ids"].shape[1] for s in steps)
    step_ids = np.zeros((len(steps), steps[0]["input_ids"].shape[0], T), dtype=np.int64)
    for i, s_ in enumerate(steps):
        step_ids[i, :, :s_["input_ids"].shape[1]] = s_["input_ids"].numpy()
    out = {"kind": "vqa_gen", "B": B, "size": size, "L": L, "temperature": np.float64(temperature), "seed": seed,
           "pad_tail": pad_tail, "eos_bias": np.float64(eos_bias), "num_beams": 3, "max_length": 10, "min_length": 1,
           "sequences": seqs.numpy(), "step_input_ids": step_ids, "step_lens": np.array([s_["input_ids"].shape[1] for s_ in steps]),
           "first_logits_sample": steps[0]["last_logits"][:, :64].numpy(),
           "first_log_probs_top": torch.log_softmax(steps[0]["last_logits"], -1).topk(6, dim=1)[0].numpy(),
           "transformers_version": np.array(__import__("transformers").__version__), "ref_seconds": dt}
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(f"[{name}] T={temperature} eos_bias={eos_bias} sequences={seqs.tolist()} steps={len(steps)} ({dt:.1f}s)")


def cap_gen_case(name, B, size, temperature, eos_bias, max_length, min_length, seed=0):
    """models/blip.py BLIP_Decoder.generate(sample=False, num_beams=3, ...) (:161-202, the evaluation call of
    compress_caption_dtp.py:86) of the reference's own modules, under the shims / caveats of vqa_gen_case (the search that runs
    is transformers 5.15's; with the 4-token prompt its finished-hypothesis normalisation differs from 4.15's)."""
    import models.blip as blip
    from madtp_amd import specs
    ref_shims.patch_tokenizer(blip)
    ref_shims.enable_generate()
    model = blip.BLIP_Decoder(image_size=size, evaluate=True, config={"sd_num": 100, "sd_dim": 768})
    model.eval()
    sd = synth.fill_state_dict(model, seed)
    sd["text_decoder.cls.predictions.bias"][102] += eos_bias
    sd = specs.tie_keys(sd)
    model.load_state_dict(sd, strict=True)
    images = synth.synth_images(B, size, seed)
    steps, raw = [], []
    orig = model.text_decoder.forward
    import functools

    @functools.wraps(orig)
    def tapped(*a, **k):
        out = orig(*a, **k)
        inp = k.get("input_ids", a[0] if a else None)
        steps.append({"input_ids": inp.detach().clone(), "last_logits": out.logits[:, -1, :].detach().clone()})
        return out
    model.text_decoder.forward = tapped
    gen = model.text_decoder.generate

    def tapped_gen(*a, **k):
        out = gen(*a, **k)
        raw.append(out.detach().clone())
        return out
    model.text_decoder.generate = tapped_gen
    lens_v, hooks = [], []
    for blk in model.visual_encoder.blocks:
        hooks.append(blk.register_forward_hook(lambda m, a, o: lens_v.append(o.shape[1])))
    t0 = time.time()
    with torch.no_grad():
        model.generate(images, sample=False, num_beams=3, max_length=max_length, min_length=min_length, temperature=temperature)
    dt = time.time() - t0
    for h in hooks:
        h.remove()
    seqs = raw[0]
    keys = sorted(sd.keys())
    out = {"kind": "cap_gen", "B": B, "size": size, "temperature": np.float64(temperature), "seed": seed,
           "eos_bias": np.float64(eos_bias), "num_beams": 3, "max_length": max_length, "min_length": min_length,
           "sequences": seqs.numpy(), "vit_lens": np.array(lens_v), "prompt_input_ids": steps[0]["input_ids"].numpy(),
           "first_log_probs_top": torch.log_softmax(steps[0]["last_logits"], -1).topk(6, dim=1)[0].numpy(),
           "second_step_input_ids": steps[1]["input_ids"].numpy(), "state_dict_keys": np.array(keys),
           "transformers_version": np.array(__import__("transformers").__version__), "ref_seconds": dt}
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(f"[{name}] T={temperature} eos_bias={eos_bias} vit_lens={lens_v} sequences={seqs.tolist()} steps={len(steps)} ({dt:.1f}s)")


def med_layer_options_case(name, B, L, Nimg, temperature, seed=0, pad_tail=0, Lp=5):
    """The parts of models/med.py BertLayer.forward's signature beyond the pruned-encoder call (med.py:393-407): `output_attentions=True`
    (self- and cross-attention probabilities in the returned tuple, :170-222, :450-456), `head_mask` ([1,H,1,1]: attention_probs_dropped *
    head_mask, :215-217) and `past_key_value` (cached self-attention keys / values concatenated in front of the new ones, :164-168; the
    returned tuple's [-2] is the updated cache, :458-462).  Layer 0 of the reference BertModel on the embeddings of synthetic ids (the
    inputs tests/grad_case.py::build_med rebuilds); every call under no_grad:
      oa0 / oaT   output_attentions=True, mode 'multimodal', temperature 0 / T (T: the layer prunes; cross-attention rows are then in
                  the reference's kept-token order, recorded)
      hm0 / hmT   head_mask, mode 'multimodal' at temperature 0; mode 'text' at T (kept sets recorded)
      pk1 / pk2   past_key_value: the layer on the first Lp tokens gives the cache; then ONE new token (and, separately, TWO new tokens
                  under a [B,1,1,Lp+2] padding mask) against it, mode 'multimodal'"""
    import models.med as rmed
    from madtp_amd import specs
    cfg = rmed.BertConfig.from_json_file("configs/med_config.json")
    cfg.encoder_width = 768
    cfg.evaluate = True
    model = rmed.BertModel(config=cfg, add_pooling_layer=False)
    model.eval()
    msg = model.load_state_dict(specs.synth_weights(specs.bert_shapes("", "med"), seed), strict=False)
    assert not msg.unexpected_keys
    space_dict = synth.synth_tensor("space_dict", (100, 768), seed)
    ids = synth.synth_token_ids(B, L, seed + 1)
    att = torch.ones_like(ids)
    if pad_tail:
        for b in range(B):
            att[b, L - (b % (pad_tail + 1)):] = 0
    enc = synth.synth_tensor("image_embeds", (B, Nimg, 768), seed).mul(25.0)
    enc_att = torch.ones(B, Nimg, dtype=torch.long)
    cap = {}
    lay = model.encoder.layer[0]
    hk = lay.register_forward_pre_hook(lambda m, a, kw: cap.update(h=a[0].detach().clone(), mask=a[1].detach().clone(),
                                                                    ta=kw["token_attn"].detach().clone()), with_kwargs=True)
    with torch.no_grad():
        model(ids, attention_mask=att, encoder_hidden_states=enc, encoder_attention_mask=enc_att, return_dict=True, mode="multimodal",
              space_dict=space_dict, temperature=temperature)
    hk.remove()
    enc_mask = model.invert_attention_mask(enc_att)
    H = cfg.num_attention_heads
    hm = torch.from_numpy(0.2 + 0.5 * (synth.uniform_pm1("head_mask", H, seed) + 1.0)).float().view(1, H, 1, 1)  # in [0.2, 1.2]
    rec = {"kind": "med_layer_options", "B": B, "L": L, "Nimg": Nimg, "temperature": np.float64(temperature), "seed": seed, "layer": 0,
           "pad_tail": pad_tail, "mode": "multimodal", "Lp": Lp, "head_mask": hm.view(H).numpy(), "h_head": cap["h"][:, :2, :8].numpy()}

    def call(hid, mask, head_mask, past, oa, mode, T, tag):
        tap = GatherTap(rmed)
        tap.set_tag(tag)
        with torch.no_grad():
            out = lay(hid.clone(), mask.clone(), head_mask, enc if mode == "multimodal" else None, enc_mask if mode == "multimodal" else None,
                      past, oa, mode=mode, space_dict=space_dict, token_attn=cap["ta"].clone() if T > 0 else None, reduce_num=0, temperature=T)
        tap.restore()
        rec.update(tap.records)
        return out

    def put(key, t):
        """hidden states / caches: the first 16 columns and the L2 norm of every row (the whole tensors would make a 2.7 MB fixture)"""
        t = t.detach()
        rec[key + "_shape"] = np.array(t.shape)
        rec[key + "_sl"] = t[..., :16].numpy().copy()
        rec[key + "_rownorm"] = t.double().norm(dim=-1).numpy()

    # --- output_attentions
    for tag, T in (("oa0", 0.0), ("oaT", temperature)):
        out = call(cap["h"], cap["mask"], None, None, True, "multimodal", T, tag)
        assert len(out) == 5, len(out)  # (layer_output, self probs, cross probs, present_key_value, attention_mask)
        put(f"{tag}_out", out[0])
        rec[f"{tag}_self_probs"], rec[f"{tag}_cross_probs"] = out[1].numpy(), out[2].numpy()
        put(f"{tag}_present_k", out[3][0])
        put(f"{tag}_present_v", out[3][1])
        rec[f"{tag}_mask_out"] = out[4][:, 0, 0, :].numpy()
    assert rec["oaT_out_shape"][1] < L, "the layer did not prune at this temperature"
    # --- head_mask
    out = call(cap["h"], cap["mask"], hm, None, False, "multimodal", 0.0, "hm0")
    assert len(out) == 3
    put("hm0_out", out[0])
    out = call(cap["h"], cap["mask"], hm, None, False, "text", temperature, "hmT")
    put("hmT_out", out[0])
    rec["hmT_mask_out"] = out[2][:, 0, 0, :].numpy()
    # --- past_key_value
    first = call(cap["h"][:, :Lp], cap["mask"][:, :, :, :Lp], None, None, False, "multimodal", 0.0, "pk0")
    past = first[1]
    put("pk0_out", first[0])
    for tag, n_new in (("pk1", 1), ("pk2", 2)):
        out = call(cap["h"][:, Lp:Lp + n_new], cap["mask"][:, :, :, :Lp + n_new], None, past, False, "multimodal", 0.0, tag)
        rec[f"{tag}_out"] = out[0].numpy()
        put(f"{tag}_present_k", out[1][0])
        put(f"{tag}_present_v", out[1][1])
        assert out[1][0].shape[2] == Lp + n_new
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] T={temperature} oaT_out {rec['oaT_out_shape']} hmT_out {rec['hmT_out_shape']} pk1 {rec['pk1_out'].shape} "
          f"keys {sorted(k for k in rec if k.endswith('_idx') or k.endswith('_sort'))}")


def pos_embed_case(name, width=64, seed=0):
    """models/vit.py:398-422 interpolate_pos_embed: a 14x14 checkpoint grid (+ CLS) resized to this encoder's 24x24 grid (384^2
    images); `width` channels of the 768 (the resize is per channel)."""
    import models.vit as ref_vit

    class Enc:  # the two attributes the function reads
        class patch_embed:
            num_patches = 576
        pos_embed = torch.zeros(1, 577, width)
    g = torch.Generator().manual_seed(seed)
    ck = torch.randn(1, 197, width, generator=g)
    out = ref_vit.interpolate_pos_embed(ck, Enc)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), checkpoint=ck.numpy(), resized=out.numpy())


def retr_train_case(name, B, size, L, temperature, idx, alpha, queue_size, seed=0, pad_tail=2, nsample=32, lr=0.05):
    """The reference's OWN retrieval training step (models/blip_retrieval.py:99-282, BLIP_Retrieval(evaluate=False), model.eval():
    no dropout / DropPath) at world 1: student ViT + MED text / multimodal towers, momentum towers after the EMA, ITC against the
    feature queues, in-batch hard negatives for ITM, dequeue-and-enqueue; loss = loss_ita + loss_itm + 0.1 (loss_fdt + loss_fdt_m)
    as compress_retrieval_dtp.py:64-65.  torch.multinomial is replaced - for this recording only - by the inverse CDF at seeded
    uniforms (the first j with cumsum(w)_j > u sum(w)), the rule the HIP path draws by; the uniforms are stored.  Then
    torch.optim.SGD(lr) steps on the gradients and a SECOND forward is recorded (its four losses only)."""
    import models.blip_retrieval as rbr
    from madtp_amd import harness
    ref_shims.patch_tokenizer(rbr)
    rbr.concat_all_gather = lambda t: t  # world 1 (the reference's all_gather over one rank)
    torch.manual_seed(seed)
    model = rbr.BLIP_Retrieval(image_size=size, vit="base", queue_size=queue_size, negative_all_rank=False, evaluate=False)
    model.eval()
    keys = list(model.state_dict().keys())
    pairing = []
    for a_mod, m_mod in model.model_pairs:
        an = [n for n, p in a_mod.named_parameters() if "alpha" not in n]
        mn = [n for n, _ in m_mod.named_parameters()]
        a_pre = [k for k, m in model.named_modules() if m is a_mod][0]
        m_pre = [k for k, m in model.named_modules() if m is m_mod][0]
        pairing += [f"{a_pre}.{x}|{m_pre}.{y}" for x, y in zip(an, mn)]
    sd = synth.fill_state_dict(model, seed)
    # the buffers the HIP test rebuilds from the fixture itself: unit-norm queue columns, ids (some equal to batch ids), ptr, temp
    g = torch.Generator().manual_seed(1000 + seed)
    sd["image_queue"] = torch.nn.functional.normalize(torch.randn(256, queue_size, generator=g), dim=0)
    sd["text_queue"] = torch.nn.functional.normalize(torch.randn(256, queue_size, generator=g), dim=0)
    iq = torch.full((1, queue_size), -100, dtype=torch.long)
    iq[0, 1] = idx[0]
    iq[0, queue_size // 2] = idx[-1]
    iq[0, 2] = 11
    sd["idx_queue"] = iq
    sd["ptr_queue"] = torch.tensor([B], dtype=torch.long)
    sd["temp"] = torch.tensor(0.07)
    model.load_state_dict(sd, strict=True)
    momentum = {id(p) for _, m in model.model_pairs for p in m.parameters()}
    images = synth.synth_images(B, size, seed)
    ids = synth.synth_token_ids(B, L, seed, first_id=101)
    att = harness.padded_mask(B, L, pad_tail)
    idx_t = torch.tensor(idx, dtype=torch.long)
    gu = torch.Generator().manual_seed(2000 + seed)
    u = torch.rand(2, B, generator=gu)
    drawn, calls = [], [0]
    orig_multinomial = torch.multinomial

    def inverse_cdf(w, n):
        k = calls[0]
        calls[0] += 1
        c = torch.cumsum(w, 0)
        j = int(torch.nonzero(c > u[k // B, k % B] * c[-1])[0, 0])
        drawn.append(j)
        return torch.tensor([j])

    lens = {"vit": [], "txt": [], "vit_m": [], "txt_m": []}
    hooks = []
    for tag, enc in (("vit", model.visual_encoder), ("vit_m", model.visual_encoder_m)):
        for blk in enc.blocks:
            hooks.append(blk.register_forward_hook(lambda m, a, o, t=tag: lens[t].append(o.shape[1])))
    for tag, enc in (("txt", model.text_encoder), ("txt_m", model.text_encoder_m)):
        for lay in enc.encoder.layer:
            hooks.append(lay.register_forward_hook(lambda m, a, o, t=tag: lens[t].append(o[0].shape[1])))
    for p_ in model.parameters():
        if id(p_) not in momentum:
            p_.requires_grad_(True)
        p_.grad = None
    caption = {"input_ids": ids, "attention_mask": att}
    torch.multinomial = inverse_cdf
    try:
        losses = model(images, caption, alpha, idx_t, temperature=temperature, train=True)
    finally:
        torch.multinomial = orig_multinomial
    for h in hooks:
        h.remove()
    loss = losses[0] + losses[1] + 0.1 * losses[2] + 0.1 * losses[3]
    loss.backward()
    rec = {"kind": "retr_train", "B": B, "size": size, "L": L, "temperature": np.float64(temperature), "seed": seed,
           "pad_tail": pad_tail, "nsample": nsample, "alpha": np.float64(alpha), "idx": np.array(idx), "queue_size": queue_size,
           "lr": np.float64(lr), "momentum": np.float64(model.momentum), "state_dict_keys": np.array(keys),
           "pairing": np.array(pairing), "u": u.numpy(), "neg": np.array(drawn).reshape(2, B),
           "init_image_queue": sd["image_queue"].numpy(), "init_text_queue": sd["text_queue"].numpy(),
           "init_idx_queue": sd["idx_queue"].numpy(), "init_ptr": int(sd["ptr_queue"][0]), "init_temp": np.float64(0.07),
           "losses": np.array([float(x) for x in losses], dtype=np.float64),
           "image_queue": model.image_queue.numpy().copy(), "text_queue": model.text_queue.numpy().copy(),
           "idx_queue": model.idx_queue.numpy().copy(), "ptr": int(model.ptr_queue[0])}  # (copies: the second step writes on)
    for t, v in lens.items():
        rec[f"{t}_lens"] = np.array(v)
    n = 0
    for k, v in model.named_parameters():
        if v.grad is None:
            continue
        flat = v.grad.detach().reshape(-1)
        ix = grad_sample_index(flat.numel(), nsample)
        rec[f"g_{k}_sample"] = flat[torch.from_numpy(ix)].numpy()
        rec[f"g_{k}_norm"] = np.float64(flat.double().norm().item())
        n += 1
    for k, v in model.named_parameters():
        if id(v) in momentum:
            flat = v.detach().reshape(-1)
            rec[f"m_{k}"] = flat[torch.from_numpy(grad_sample_index(flat.numel(), 16, stride=104729))].numpy()
    torch.optim.SGD([p_ for p_ in model.parameters() if p_.grad is not None], lr=lr).step()
    torch.multinomial = inverse_cdf
    calls[0] = 0
    try:
        with torch.no_grad():
            losses2 = model(images, caption, alpha, idx_t, temperature=temperature, train=True)
    finally:
        torch.multinomial = orig_multinomial
    rec["losses2"] = np.array([float(x) for x in losses2], dtype=np.float64)
    rec["neg2"] = np.array(drawn[2 * B:]).reshape(2, B)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] T={temperature} lens={ {t: v for t, v in lens.items()} } losses={rec['losses'].round(5).tolist()} "
          f"losses2={rec['losses2'].round(5).tolist()} neg={rec['neg'].tolist()} {n} gradients")


class CanonicalTap(GatherTap):
    """GatherTap that also puts the kept `indices` of each Reduce_token (the first vector_gather of a block call, the unsorted
    torch.topk of clip/model.py:224) in ascending token order - the canonical order of the HIP path; the
    reference's own order is implementation-defined and, in the causal text tower, visible in the values."""

    def __call__(self, vectors, indices):
        if self.tag is not None and vectors.shape[-1] > 1 and self.calls == 0:
            indices = indices.sort(dim=-1).values
        return super().__call__(vectors, indices)


def clip_train_tokens(lens, seed):
    """[B,77] CLIP token rows with exactly lens[b] word ids each (synth.synth_clip_tokens, one row per call)."""
    return torch.cat([synth.synth_clip_tokens(1, 77, 100 * seed + b, n, n) for b, n in enumerate(lens)], 0)


def clip_train_case(name, B, temperature, idx, cap_lens, alpha=0.4, queue_size=48, seed=0, size=96, nsample=32, lr=0.05,
                    patch=16, vision_width=768, vision_layers=12, embed_dim=512, text_width=512, text_layers=12):
    """The reference's OWN CLIP training step (clip/model.py:529-595, CLIP(evaluate=False), model.eval()) at world 1, by default on
    the ViT-B/16 geometry at 96^2 (37 tokens) with the 12-layer text tower (the geometry keywords are those of clip_full_case;
    heads = width // 64 in both towers): student towers, EMA, momentum pass (encode_text_m runs
    the STUDENT transformer, :516), ITC against a small seeded queue, dequeue-and-enqueue of the student features;
    loss = loss_ita + 0.1 loss_fdt + 0.1 loss_fdt_m as compress_retrieval_clip_dtp.py does.  For this recording only the kept
    tokens of every pruning step are put in ascending order (CanonicalTap).  Then torch.optim.SGD(lr) steps on the gradients and a
    SECOND forward is recorded (its losses only)."""
    import clip.mock  # noqa: F401
    import clip.model as cm
    from madtp_amd import specs
    cm.concat_all_gather = lambda t: t  # world 1
    torch.manual_seed(seed)
    model = cm.CLIP(embed_dim, size, vision_layers, vision_width, patch, 77, 49408, text_width, text_width // 64, text_layers,
                    False, None)
    model.eval()
    sd = specs.synth_weights(specs.clip_shapes(size, patch, vision_width, vision_layers, embed_dim, text_width, text_layers), seed)
    sd["logit_scale"] = torch.tensor(2.6592600369327779)  # log(1 / 0.07), the reference's initial value (:387)
    msg = model.load_state_dict(sd, strict=False)
    assert not msg.unexpected_keys, msg.unexpected_keys
    assert all(k.endswith("_m") or "_m." in k or "queue" in k for k in msg.missing_keys), msg.missing_keys[:8]
    g = torch.Generator().manual_seed(1000 + seed)
    model.queue_size = queue_size
    iq = torch.full((1, queue_size), -100, dtype=torch.long)
    iq[0, 1] = idx[-1]                     # an id of the batch already in the queue
    iq[0, queue_size // 2] = 11
    init = {"image_queue": torch.nn.functional.normalize(torch.randn(embed_dim, queue_size, generator=g), dim=0),
            "text_queue": torch.nn.functional.normalize(torch.randn(embed_dim, queue_size, generator=g), dim=0),
            "idx_queue": iq, "ptr_queue": torch.tensor([B + 1], dtype=torch.long)}  # (an unaligned pointer: rounded down, :609-610)
    for k, v in init.items():
        setattr(model, k, v.clone())
    model.copy_params()
    keys = sorted(model.state_dict().keys())
    momentum = {id(p) for _, m in model.model_pairs for p in m.parameters()} | {id(pm) for _, pm in model.params_pairs}
    images = synth.synth_images(B, size, seed)
    text = clip_train_tokens(cap_lens, seed)
    model.tokenize = lambda caption: text
    idx_t = torch.tensor(idx, dtype=torch.long)
    tap = CanonicalTap(cm)
    lens = {"vit": [], "txt": [], "vit_m": []}
    hooks = []
    for tag, blocks in (("vit", model.visual.transformer.resblocks), ("txt", model.transformer.resblocks),
                        ("vit_m", model.visual_m.transformer.resblocks)):
        for i, blk in enumerate(blocks):
            hooks.append(blk.register_forward_pre_hook(lambda m, a, t=tag, i=i: tap.set_tag(f"{t}{i}")))
            hooks.append(blk.register_forward_hook(lambda m, a, o, t=tag: lens[t].append(o[0].shape[0])))
    for p_ in model.parameters():
        if id(p_) not in momentum:
            p_.requires_grad_(True)
        p_.grad = None
    losses = model(images, ["caption"] * B, alpha, idx_t, temperature=temperature)
    n_lens = {t: len(v) for t, v in lens.items()}
    (losses[0] + 0.1 * losses[1] + 0.1 * losses[2]).backward()
    rec = {"kind": "clip_train", "B": B, "size": size, "temperature": np.float64(temperature), "seed": seed, "nsample": nsample,
           "alpha": np.float64(alpha), "idx": np.array(idx), "queue_size": queue_size, "lr": np.float64(lr),
           "momentum": np.float64(model.momentum), "state_dict_keys": np.array(keys), "text": text.numpy(),
           "cap_lens": np.array(cap_lens), "eot_pos": text.argmax(-1).numpy(), "init_logit_scale": np.float64(sd["logit_scale"].item()),
           "init_image_queue": init["image_queue"].numpy(), "init_text_queue": init["text_queue"].numpy(),
           "init_idx_queue": init["idx_queue"].numpy(), "init_ptr": int(init["ptr_queue"][0]),
           "losses": np.array([float(x) for x in losses], dtype=np.float64),
           "idx_queue": model.idx_queue.numpy().copy(), "ptr": int(model.ptr_queue[0]),
           "vit_lens": np.array(lens["vit"]), "vit_m_lens": np.array(lens["vit_m"]),
           "txt_lens": np.array(lens["txt"][:text_layers]),
           "txt_m_lens": np.array(lens["txt"][text_layers:2 * text_layers])}  # (both calls of the student blocks)
    assert n_lens == {"vit": vision_layers, "txt": 2 * text_layers, "vit_m": vision_layers}, n_lens
    # the queues after the step: the B columns written at the rounded-down pointer (the others must equal the initial queue)
    p0 = rec["init_ptr"] // B * B
    for k in ("image_queue", "text_queue"):
        after = getattr(model, k).numpy()
        rest = np.ones(queue_size, dtype=bool)
        rest[p0:p0 + B] = False
        assert np.array_equal(after[:, rest], init[k].numpy()[:, rest])
        rec[f"enq_{k}"] = after[:, p0:p0 + B].copy()
    rec["enq_at"] = p0
    n = 0
    for k, v in model.named_parameters():
        if v.grad is None:
            continue
        flat = v.grad.detach().reshape(-1)
        ix = grad_sample_index(flat.numel(), nsample)
        rec[f"g_{k}_sample"] = flat[torch.from_numpy(ix)].numpy()
        rec[f"g_{k}_norm"] = np.float64(flat.double().norm().item())
        n += 1
    for k, v in model.named_parameters():
        if id(v) in momentum:
            flat = v.detach().reshape(-1)
            rec[f"m_{k}"] = flat[torch.from_numpy(grad_sample_index(flat.numel(), 16, stride=104729))].numpy()
    torch.optim.SGD([p_ for p_ in model.parameters() if p_.grad is not None], lr=lr).step()
    with torch.no_grad():
        losses2 = model(images, ["caption"] * B, alpha, idx_t, temperature=temperature)
    for h in hooks:
        h.remove()
    tap.restore()
    rec["losses2"] = np.array([float(x) for x in losses2], dtype=np.float64)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **rec)
    print(f"[{name}] T={temperature} eot={rec['eot_pos'].tolist()} lens={ {t: v.tolist() for t, v in rec.items() if t.endswith('_lens')} } "
          f"losses={rec['losses'].round(5).tolist()} losses2={rec['losses2'].round(5).tolist()} {n} gradients")


def clip_eval_case(name, n_img, img_bs, cap, temperature, seed=0, size=96, n_seeds=16, min_gap=1e-4):
    """compress_retrieval_clip_dtp.py evaluate() and itm_eval() - the reference's own functions, imported behind the shims - on
    the reference's CLIP (clip/model.py, ViT-B/16 geometry at 96^2 as in clip_train_case, evaluate=True, synthetic weights): n_img
    images in batches of img_bs, cap captions each (caption j belongs to image j // cap).  As in clip_train_case the kept tokens
    of every pruning step are put in ascending order (CanonicalTap).  Recorded: the normalised embeddings (the outputs of
    encode_image / encode_text, captured on their way through evaluate() and normalised as :93 / :101 do), sims, the nine metrics,
    the per-target ranks and the per-layer lengths of every batch.
    Gap.  A rank of the recording survives another implementation's rounding only where the ground-truth score is further from
    every other score of its row (column) than that rounding.  100x the feature tolerance of
    tests/test_model_parity_gpu.py::test_clip_both_towers (1e-3) would be 0.1, which no seed can give: with synthetic weights
    the two towers are unrelated and all n_img * n_txt cosine scores lie within ~0.12 of each other.  So every seed of
    [seed, seed + n_seeds) is run and the one with the LARGEST smallest float64 gap is kept (seeds 0-15: 4e-6 .. 2.0e-4, kept:
    seed 13 at 1.98e-4); the recorder asserts min_gap = 1e-4 - a thousand times the f32 rounding of a 512-term dot product of
    unit vectors (~1e-7), so the ranks of the RECORDED embeddings are reproducible exactly by any f32 summation order - and stores
    the per-target gaps, with which a test decides which ranks of a live model (features within 1e-3) are pinned."""
    import types
    import clip.mock  # noqa: F401
    import clip.model as cm
    import compress_retrieval_clip_dtp as crc
    from madtp_amd import specs
    n_txt = n_img * cap
    txt2img = [j // cap for j in range(n_txt)]
    img2txt = [list(range(i * cap, (i + 1) * cap)) for i in range(n_img)]
    nb = (n_img + img_bs - 1) // img_bs

    def pos(row):
        order = np.argsort(row, kind="stable")[::-1]
        p = np.empty(len(order), dtype=np.int64)
        p[order] = np.arange(len(order))
        return p

    def record(s):
        model = cm.CLIP(512, size, 12, 768, 16, 77, 49408, 512, 8, 12, True, None)
        model.eval()
        sd = specs.synth_weights(specs.clip_shapes(size), s)
        msg = model.load_state_dict(sd, strict=False)
        assert not msg.unexpected_keys, msg.unexpected_keys
        assert all(k.endswith("_m") or "_m." in k or "queue" in k for k in msg.missing_keys), msg.missing_keys[:8]
        images = synth.synth_images(n_img, size, s)
        text = synth.synth_clip_tokens(n_txt, 77, s, 6, 40)
        model.tokenize = lambda t: t

        class Loader:
            dataset = types.SimpleNamespace(text=text)
            def __len__(self): return nb
            def __iter__(self):
                for b in range(0, n_img, img_bs):
                    yield images[b:b + img_bs], ["caption"] * len(images[b:b + img_bs]), torch.arange(b, min(n_img, b + img_bs))

        tap = CanonicalTap(cm)
        hooks, vlens, tlens, feats = [], [], [], {"img": [], "txt": []}
        for i, blk in enumerate(model.visual.transformer.resblocks):
            hooks.append(blk.register_forward_pre_hook(lambda m, a, i=i: tap.set_tag(f"vit{i}")))
            hooks.append(blk.register_forward_hook(lambda m, a, o: vlens.append(o[0].shape[0])))
        for i, blk in enumerate(model.transformer.resblocks):
            hooks.append(blk.register_forward_pre_hook(lambda m, a, i=i: tap.set_tag(f"txt{i}")))
            hooks.append(blk.register_forward_hook(lambda m, a, o: tlens.append(o[0].shape[0])))
        enc_i, enc_t = model.encode_image, model.encode_text

        def keep(kind, out):
            feats[kind].append(out[0].detach().clone())
            return out
        model.encode_image = lambda *a, **k: keep("img", enc_i(*a, **k))
        model.encode_text = lambda *a, **k: keep("txt", enc_t(*a, **k))
        sims, sims_t, _ = crc.evaluate(model, Loader(), torch.device("cpu"), {"alpha": 0.4}, temperature)
        metrics = crc.itm_eval(sims, sims_t, txt2img, img2txt)
        for h in hooks:
            h.remove()
        tap.restore()
        img_e = torch.cat([f / f.norm(dim=1, keepdim=True) for f in feats["img"]], 0)
        txt_e = torch.cat([f / f.norm(dim=1, keepdim=True) for f in feats["txt"]], 0)
        assert np.array_equal(sims, (img_e @ txt_e.t()).numpy()) and np.array_equal(sims_t, sims.T)
        s64 = (img_e.double() @ txt_e.double().t()).numpy()
        gap_i2t = np.array([np.abs(np.delete(s64[txt2img[j]], j) - s64[txt2img[j], j]).min() for j in range(n_txt)])
        gap_t2i = np.array([np.abs(np.delete(s64[:, j], txt2img[j]) - s64[txt2img[j], j]).min() for j in range(n_txt)])
        gap = float(min(gap_i2t.min(), gap_t2i.min()))
        rank_tgt_i2t = np.array([pos(sims[i])[j] for i in range(n_img) for j in img2txt[i]], dtype=np.int32)
        rank_tgt_t2i = np.array([pos(sims_t[j])[txt2img[j]] for j in range(n_txt)], dtype=np.int32)
        assert len(vlens) == 12 * nb and len(tlens) == 12, (len(vlens), len(tlens))
        rec = {"kind": "clip_eval", "n_img": n_img, "img_bs": img_bs, "cap": cap, "size": size, "temperature": np.float64(temperature),
               "seed": s, "gap": np.float64(gap), "gap_i2t": gap_i2t, "gap_t2i": gap_t2i, "image_embeds": img_e.numpy(),
               "text_embeds": txt_e.numpy(), "sims": sims, "txt2img": np.array(txt2img, dtype=np.int32),
               "rank_tgt_i2t": rank_tgt_i2t, "rank_tgt_t2i": rank_tgt_t2i, "rank_row_i2t": rank_tgt_i2t.reshape(n_img, cap).min(1),
               "metric_names": np.array(sorted(metrics)), "metrics": np.array([metrics[k] for k in sorted(metrics)], dtype=np.float64),
               "vit_lens": np.array(vlens).reshape(nb, 12), "txt_lens": np.array(tlens).reshape(1, 12)}
        print(f"[{name}] seed {s}: smallest gap around a ground-truth score {gap:.3e}")
        return rec

    best = max((record(s) for s in range(seed, seed + n_seeds)), key=lambda r: float(r["gap"]))
    assert float(best["gap"]) >= min_gap, f"largest gap over seeds [{seed}, {seed + n_seeds}) is {float(best['gap']):.3e} < {min_gap}"
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **best)
    print(f"[{name}] T={temperature} kept seed {int(best['seed'])} gap {float(best['gap']):.3e} vit_lens={best['vit_lens'].tolist()} "
          f"txt_lens={best['txt_lens'].tolist()} metrics={dict(zip(best['metric_names'].tolist(), best['metrics'].round(2).tolist()))}")


L14 = dict(patch=14, vision_width=1024, vision_layers=24, embed_dim=768, text_width=768)

CASES = {
    "pos_embed_384": lambda: pos_embed_case("pos_embed_384"),
    "medopts_b2": lambda: med_layer_options_case("medopts_b2", 2, 35, 10, 30.0, pad_tail=1, Lp=20),
    "cap_gen_b2_T6": lambda: cap_gen_case("cap_gen_b2_T6", 2, 224, 6.0, 0.0, 12, 5),
    "cap_gen_b3_T30_eos": lambda: cap_gen_case("cap_gen_b3_T30_eos", 3, 224, 30.0, 2.4, 12, 5, seed=1),
    "vqa_gen_b2": lambda: vqa_gen_case("vqa_gen_b2", 2, 224, 12, 0.0, 0.0),
    "vqa_gen_b3_T30_eos": lambda: vqa_gen_case("vqa_gen_b3_T30_eos", 3, 224, 16, 30.0, 2.2, seed=1, pad_tail=3),
    "vqa_gen_b4_eos26": lambda: vqa_gen_case("vqa_gen_b4_eos26", 4, 224, 12, 0.0, 2.6, seed=2),
    "nlvr_b2_T1": lambda: nlvr_case("nlvr_b2_T1", 2, 224, 20, 1.0),
    "nlvr_b2_T5": lambda: nlvr_case("nlvr_b2_T5", 2, 224, 20, 5.0),
    "nlvr_b3_T30_pad": lambda: nlvr_case("nlvr_b3_T30_pad", 3, 224, 35, 30.0, pad_tail=3),
    # ragged captions (0 / 14 / 26 padded positions of 35): k = max_b count is set by the long caption, so the short ones keep
    # PADDED tokens inside their top-(k+1) - the token / mask pairing of nlvr_encoder.py:440-452 is exercised
    "nlvrpad_b3_T12": lambda: nlvr_case("nlvrpad_b3_T12", 3, 224, 35, 12.0, seed=0, pad_list=[0, 14, 26]),
    # the same edge at ONE text layer only (layer 4, the first one that prunes; 0 / 1 / 2 padded positions): what differs from
    # the recording can be stated slot by slot (tests)
    "nlvrpad_b3_T20_one": lambda: nlvr_case("nlvrpad_b3_T20_one", 3, 224, 35, 20.0, seed=0, pad_list=[0, 1, 2]),
    "med_text_b3": lambda: med_case("med_text_b3", 3, 35, 0, 30.0, "text", pad_tail=3),
    "med_mm_b3": lambda: med_case("med_mm_b3", 3, 35, 50, 30.0, "multimodal", pad_tail=3),
    "vqa480_b2": lambda: vqa_case("vqa480_b2", 2, 480, 20, 6.0, pad_tail=2),
    "vqa480_b2_T30": lambda: vqa_case("vqa480_b2_T30", 2, 480, 35, 30.0, seed=2, pad_tail=4),
    "vqa_rank_b3": lambda: vqa_rank_case("vqa_rank_b3", 3, 224, 20, 6.0, n_answers=12, answer_len=7, k_test=4, pad_tail=2),
    "vqa_rank_b2_T30": lambda: vqa_rank_case("vqa_rank_b2_T30", 2, 224, 35, 30.0, n_answers=9, answer_len=5, k_test=3, seed=2,
                                             pad_tail=4),
    "clip_vit_b2": lambda: clip_case("clip_vit_b2", 2, 4.0),
    "clip_full_b3_T4": lambda: clip_full_case("clip_full_b3_T4", 3, 4.0),
    "clip_full_b3_T40": lambda: clip_full_case("clip_full_b3_T40", 3, 40.0, seed=1),
    "vit384_b2": lambda: vit_case("vit384_b2", 2, 384, 6.0),
    "vit480_b1": lambda: vit_case("vit480_b1", 1, 480, 6.0),
    "retr_i6_t12": lambda: retrieval_case("retr_i6_t12", 6, 3, 12, 224, 6.0, 4),
    "retr_384_i4_t6": lambda: retrieval_case("retr_384_i4_t6", 4, 2, 6, 384, 4.0, 3, seed=1),
    # backward of one pruned ViT block: the reference's own .grad (layer 0 at T = 5: 196 -> ~133 kept + 1 merged token; layer 3
    # at the same temperature enters with an already pruned sequence of 101 tokens; margins of every pruning decision on the way are >= 8e-5 relative, far above f32 rounding)
    "blockgrad_b2": lambda: vit_block_grad_case("blockgrad_b2", 2, 224, 5.0, layer=0),
    "blockgrad_b2_l3": lambda: vit_block_grad_case("blockgrad_b2_l3", 2, 224, 5.0, layer=3),
    "encgrad_b2_s96": lambda: vit_grad_case("encgrad_b2_s96", 2, 96, 5.0),
    "medgrad_b3_l0": lambda: med_layer_grad_case("medgrad_b3_l0", 3, 35, 30.0, layer=0, pad_tail=3),
    "medgrad_b3_l3": lambda: med_layer_grad_case("medgrad_b3_l3", 3, 35, 30.0, layer=3, pad_tail=3),
    "clipvitgrad_b2": lambda: clip_vit_grad_case("clipvitgrad_b2", 2, 4.0),
    # ViT-L/14@336, the geometry of the reference's configs/retrieval_{coco,flickr}_clip.yaml (clip_large_retrieval_*.pth)
    "clipl14_full_b2_T4": lambda: clip_full_case("clipl14_full_b2_T4", 2, 4.0, size=336, **L14),
    "clipl14_full_b2_T40": lambda: clip_full_case("clipl14_full_b2_T40", 2, 40.0, seed=1, size=336, **L14),
    "clipl14vitgrad_b2": lambda: clip_vit_grad_case("clipl14vitgrad_b2", 2, 4.0, size=112, patch=14, width=1024, layers=24,
                                                    out_dim=768),
    "cliptextgrad_b2": lambda: clip_text_block_grad_case("cliptextgrad_b2", 2, 24, 3.0, 4),
    "clipgrad_b2_l1": lambda: clip_block_grad_case("clipgrad_b2_l1", 2, 4.0, layer=1),
    "trainstep_cap_b2": lambda: cap_train_case("trainstep_cap_b2", 2, 96, 12, 20.0),
    "trainstep_vqa_b2": lambda: vqa_train_case("trainstep_vqa_b2", 2, 96, 20, 20.0, [2, 1], 6),
    "decgrad_b3": lambda: decoder_grad_case("decgrad_b3", 3, 8, 12),
    "trainstep_nlvr_b2": lambda: nlvr_model_grad_case("trainstep_nlvr_b2", 2, 96, 35, 30.0, pad_tail=0, nsample=64, train=True),
    # the retrieval training step (BLIP_Retrieval.forward, evaluate=False): duplicate ids, ids shared with the queue, T = 20 and 0
    "trainstep_retr_b3_T20": lambda: retr_train_case("trainstep_retr_b3_T20", 3, 96, 20, 20.0, [5, 7, 5], 0.4, 12),
    "trainstep_retr_b4_T0": lambda: retr_train_case("trainstep_retr_b4_T0", 4, 96, 16, 0.0, [3, 8, 9, 4], 0.4, 12, seed=1),
    # the CLIP training step (CLIP.forward, evaluate=False): a duplicate id in the batch, an id shared with the queue, captions of
    # 5 .. 60 words with one EOT near position 40
    "trainstep_clip_b4_T0": lambda: clip_train_case("trainstep_clip_b4_T0", 4, 0.0, [3, 8, 3, 4], [5, 39, 60, 14], seed=1),
    "trainstep_clip_b3_T4": lambda: clip_train_case("trainstep_clip_b3_T4", 3, 4.0, [5, 7, 5], [7, 39, 22]),
    # the same step at the ViT-L/14 widths (vision 1024 / 16 heads, text 768 / 12 heads, embed_dim 768) with 4 layers per tower
    # at 112^2 (65 tokens): every block applies the same pruning rule, and clipl14vitgrad_b2 covers the 24-layer depth
    "trainstep_clipl14_b3_T4": lambda: clip_train_case("trainstep_clipl14_b3_T4", 3, 4.0, [5, 7, 5], [7, 39, 22], queue_size=24,
                                                       size=112, patch=14, vision_width=1024, vision_layers=4, embed_dim=768,
                                                       text_width=768, text_layers=4),
    "modelgrad_nlvr_b2": lambda: nlvr_model_grad_case("modelgrad_nlvr_b2", 2, 96, 35, 30.0, pad_tail=0, nsample=64),
    "nlvrgrad_b3_l3": lambda: nlvr_layer_grad_case("nlvrgrad_b3_l3", 3, 35, 30.0, layer=3, pad_tail=3),
    "nlvrgrad_b3_l7": lambda: nlvr_layer_grad_case("nlvrgrad_b3_l7", 3, 35, 30.0, layer=7, pad_tail=3),
    # the CLIP driver's evaluate() + itm_eval(): 6 images in batches of 4 + 2, 3 captions each
    "clipeval_b6_T4": lambda: clip_eval_case("clipeval_b6_T4", 6, 4, 3, 4.0),
    "medgrad_mm_b3_l3": lambda: med_layer_grad_case("medgrad_mm_b3_l3", 3, 35, 30.0, layer=3, pad_tail=3, mode="multimodal", Nimg=50),
}

if __name__ == "__main__":
    os.makedirs(GOLD, exist_ok=True)
    todo = sys.argv[1:] or list(CASES)
    for c in todo:
        CASES[c]()

"""Mirror of the reference's CLIP with token pruning (clip/model.py: LayerNorm :158, QuickGELU :167, ResidualAttentionBlock
:174-261, Transformer :264-272, VisionTransformer :275-313, CLIP :316-503 evaluation side, build_model :678-716, with
clip/mock.py's patched nn.MultiheadAttention): same constructor arguments, parameter names and forward() contracts - a block
takes and returns the 5-tuple (x[L,B,C], space_dict, temperature, sd_ft_all, max_keep).

Both towers run (BASELINE config 4).  The text tower's blocks carry the causal attn_mask, applied as
attn_mask[:L,:L] to the CURRENT (possibly pruned) sequence exactly as clip/mock.py:309-310 does.  One documented difference:
the reference keeps pruned tokens in torch.topk(sorted=False)'s implementation-defined order, this path in ascending token
order ("replicate a canonical order and document it").  In the vision tower the order is immaterial; in
the text tower the positional mask and the read-out x[b, argmax(text[b])] (:501) see the order, so text features of PRUNED
sequences are pinned by the oracle run with order="ascending" (oracle.clip_encode_text), and the oracle with
order="reference" is pinned to the reference fixture.
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn

from . import hip
from .runtime import autograd_precision as _autograd_precision, PreparedCache, get_precision, f32_ptr, compute_dtype, dtype_code, lin_of, note_updated, prepare_linear, require_gpu, as_f32_contig, to_compute
from .utils import DeferredAttFt, Query_model


class LayerNorm(nn.LayerNorm):
    """clip/model.py:158-165 (fp16-safe LayerNorm; parameters only - the kernels always normalise in f32)."""


class QuickGELU(nn.Module):
    """clip/model.py:167-169: x * sigmoid(1.702 x); fused into the c_fc GEMM epilogue (MADTP_ACT_QUICK_GELU)."""

    def forward(self, x):
        raise NotImplementedError("fused into ResidualAttentionBlock.forward")


class _InProj:
    """adapter: nn.MultiheadAttention's packed in_proj_{weight,bias} viewed as a Linear for lin_of()."""

    def __init__(self, mha):
        self.weight, self.bias = mha.in_proj_weight, mha.in_proj_bias


class ResidualAttentionBlock(nn.Module):
    def __init__(self, d_model: int, n_head: int, attn_mask: torch.Tensor = None, sd_dim=768):
        super().__init__()
        if d_model // n_head != 64:
            raise ValueError("the gfx950 attention kernels are built for head_dim 64 (CLIP ViT-B/16, ViT-L/14)")
        # parameter container with the reference's names: attn.in_proj_weight/in_proj_bias/out_proj.{weight,bias}
        self.attn = nn.MultiheadAttention(d_model, n_head)
        self.ln_1 = LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(d_model, d_model * 4)), ("gelu", QuickGELU()),
                                              ("c_proj", nn.Linear(d_model * 4, d_model))]))
        self.ln_2 = LayerNorm(d_model)
        self.attn_mask = attn_mask
        self._mask_dev = None  # f32 GPU copy of attn_mask handed to the attention kernel
        self.query_model = Query_model(ft_dim=d_model, sd_dim=sd_dim, temperature=1, att_func_type='sparsemax',
                                       pool_type='max', map_func=True)
        self.n_head, self.d_model = n_head, d_model
        self.last_prune = None
        self._cache = PreparedCache()

    def _weights(self):
        params = [self.ln_1.weight, self.ln_1.bias, self.ln_2.weight, self.ln_2.bias, self.attn.in_proj_weight,
                  self.attn.in_proj_bias, self.attn.out_proj.weight, self.attn.out_proj.bias, self.mlp.c_fc.weight,
                  self.mlp.c_fc.bias, self.mlp.c_proj.weight, self.mlp.c_proj.bias]

        def build():
            lins = [lin_of(self._cache, "qkv", [_InProj(self.attn)]), lin_of(self._cache, "proj", [self.attn.out_proj]),
                    lin_of(self._cache, "fc1", [self.mlp.c_fc]), lin_of(self._cache, "fc2", [self.mlp.c_proj])]
            w = hip.VitBlockW()
            w.ln1_g, w.ln1_b = f32_ptr(self.ln_1.weight, "LayerNorm parameter"), f32_ptr(self.ln_1.bias, "LayerNorm parameter")
            w.ln2_g, w.ln2_b = f32_ptr(self.ln_2.weight, "LayerNorm parameter"), f32_ptr(self.ln_2.bias, "LayerNorm parameter")
            w.eps, w.scale = self.ln_1.eps, (self.d_model // self.n_head) ** -0.5
            w.qkv, w.proj, w.fc1, w.fc2 = [hip.lin_struct(l) for l in lins]
            w.heads, w.dim = self.n_head, self.d_model
            w.dtype = dtype_code()
            w.act = hip.ACT_QUICK_GELU
            keep = [lins]
            if self.attn_mask is not None:  # :191-192 attention(): the mask follows x's device
                dev = self.ln_1.weight.device
                if self._mask_dev is None or self._mask_dev.device != dev:
                    self._mask_dev = self.attn_mask.detach().to(device=dev, dtype=torch.float32).contiguous()
                w.attn_mask, w.ld_attn_mask = self._mask_dev.data_ptr(), self._mask_dev.stride(0)
                keep.append(self._mask_dev)
            return (w, keep)

        return self._cache.get("w", params, build)[0]

    def forward(self, inputs):
        x, space_dict, temperature, sd_ft_all, max_keep = inputs  # x: (N, B, C)   clip/model.py:238
        require_gpu(x, "x")
        if self.attn_mask is not None and x.shape[0] > self.attn_mask.shape[0]:
            raise ValueError(f"sequence of {x.shape[0]} tokens exceeds the {self.attn_mask.shape[0]}-token attention mask")
        xb = as_f32_contig(x.permute(1, 0, 2))  # (B, N, C); a no-op view when x came from the previous block
        B, N, C = xb.shape
        if torch.is_grad_enabled() and _autograd_precision() and (
                xb.requires_grad or (space_dict is not None and space_dict.requires_grad) or any(p.requires_grad for p in self.parameters())):
            # training use: the block as autograd Functions around the same kernels (madtp_amd/backward.py);
            # sd_ft_all (the running att_ft sum, :241-245) carries a graph as well
            from .backward import QueryModelFunction, block_forward_with_grad
            token_attn = None
            if space_dict is not None:
                if isinstance(sd_ft_all, DeferredAttFt):
                    sd_ft_all = None
                qmap = self.query_model.q_map[0]
                token_attn, sd_ft = QueryModelFunction.apply(self.query_model, xb, space_dict, qmap.weight, qmap.bias)
                sd_ft_all = sd_ft if sd_ft_all is None else sd_ft_all + sd_ft
            prune = space_dict is not None and temperature > 0
            if self.attn_mask is not None:
                self._weights()  # (makes the f32 device copy of the mask the backward reads)
            y = block_forward_with_grad(self, xb, temperature if prune else 0, token_attn, max_keep=int(max_keep))
            return y.permute(1, 0, 2), space_dict, temperature, sd_ft_all, max_keep
        token_attn = None
        if space_dict is not None:  # :239-245
            if isinstance(sd_ft_all, DeferredAttFt):  # Transformer.forward sums the blocks' att_ft in one launch at the end
                token_attn, _, _ = self.query_model(xb[:, 1:, :], space_dict, return_token_att=True, defer=sd_ft_all)
            else:
                token_attn, sd_ft_all, _ = self.query_model(xb[:, 1:, :], space_dict, return_token_att=True, acc_ft=sd_ft_all)
        prune = space_dict is not None and temperature > 0
        w = self._weights()
        # :247 + Reduce_token :196-218 + :222-234, :260 in one library call: the host read of k overlaps the projection GEMM
        # (max_keep is a 0-dim tensor on the text side, :492 - Transformer.forward converts it once)
        y, self.last_prune = hip.vit_block(w, xb, token_attn, temperature if prune else 0, max_keep=int(max_keep))
        return y.permute(1, 0, 2), space_dict, temperature, sd_ft_all, max_keep


class Transformer(nn.Module):
    """clip/model.py:264-272."""

    def __init__(self, width: int, layers: int, heads: int, attn_mask: torch.Tensor = None, sd_dim=768):
        super().__init__()
        self.width = width
        self.layers = layers
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads, attn_mask, sd_dim=sd_dim) for _ in range(layers)])

    def forward(self, x: torch.Tensor, space_dict=None, temperature=0, sd_ft_all=None, max_keep=1):
        # `sd_ft_all = sd_ft_all + sd_ft` of every block (clip/model.py:243-245) as ONE launch behind the last block when the
        # sum starts here (sd_ft_all is None): the blocks record their (logits, mapped q) pairs in a DeferredAttFt that rides in
        # the tuple's sd_ft_all slot (same values: fast mode one bf16-MFMA launch, parity modes the exact kernel in layer order)
        defer = None
        if space_dict is not None and sd_ft_all is None and len(self.resblocks) > 0 \
                and all(isinstance(b, ResidualAttentionBlock) for b in self.resblocks):
            defer = self.resblocks[0].query_model.deferred()
        if torch.is_tensor(max_keep):
            max_keep = int(max_keep)  # one host read per tower instead of one per block
        if defer is None:
            return self.resblocks((x, space_dict, temperature, sd_ft_all, max_keep))
        x, space_dict, temperature, d, max_keep = self.resblocks((x, space_dict, temperature, defer, max_keep))
        if not isinstance(d, DeferredAttFt):  # the blocks ran under autograd and summed their att_ft themselves
            return x, space_dict, temperature, d, max_keep
        return x, space_dict, temperature, (d.finish() if d.pairs else None), max_keep


class VisionTransformer(nn.Module):
    """clip/model.py:275-313."""

    def __init__(self, input_resolution: int, patch_size: int, width: int, layers: int, heads: int, output_dim: int, sd_dim=768):
        super().__init__()
        self.input_resolution = input_resolution
        self.output_dim = output_dim
        self.patch_size = patch_size
        self.conv1 = nn.Conv2d(in_channels=3, out_channels=width, kernel_size=patch_size, stride=patch_size, bias=False)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn((input_resolution // patch_size) ** 2 + 1, width))
        self.ln_pre = LayerNorm(width)
        self.transformer = Transformer(width, layers, heads, sd_dim=sd_dim)
        self.ln_post = LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))
        self._cache = PreparedCache()

    def conv_weight_cols(self):
        """conv1.weight as the patch-embedding GEMM's [width, Kp] operand (hip.patch_cols): zero columns past 3 * P^2, which
        meet the zero tail of the patchify rows (ViT-L/14: 588 -> 640; ViT-B/16: 768, no tail)"""
        w = self.conv1.weight.detach().reshape(self.conv1.weight.shape[0], -1).float()
        kp = hip.patch_cols(self.patch_size)
        return w if kp == w.shape[1] else torch.nn.functional.pad(w, (0, kp - w.shape[1]))

    def forward(self, x: torch.Tensor, space_dict=None, temperature=0, max_keep=1):
        img = as_f32_contig(require_gpu(x, "image"))
        B = img.shape[0]
        if torch.is_grad_enabled() and _autograd_precision() and (
                (space_dict is not None and space_dict.requires_grad) or any(p.requires_grad for p in self.parameters())):
            from .backward import clip_vision_forward_with_grad  # (the tower under autograd)
            return clip_vision_forward_with_grad(self, img, space_dict, temperature, max_keep)
        cdt = compute_dtype()
        conv = self._cache.get(("conv", cdt), [self.conv1.weight], lambda: prepare_linear([self.conv_weight_cols()], None, cdt))
        cols = hip.patchify(img, self.patch_size, cdt)
        patches = hip.gemm(cols, conv.w, None, out_dtype=torch.float32, n=conv.n)  # :293-295
        np_ = patches.shape[0] // B
        tok = hip.assemble_tokens(patches, self.class_embedding, self.positional_embedding, B, np_)  # :296-297
        tok, _ = hip.layernorm(tok, self.ln_pre.weight, self.ln_pre.bias, self.ln_pre.eps)  # :298
        xs = tok.permute(1, 0, 2)  # NLD -> LND (a view; the blocks undo it without a copy)
        sd_img_ft_all = None
        if space_dict is not None:
            xs, _, _, sd_img_ft_all, _ = self.transformer(xs, space_dict, temperature, sd_img_ft_all, max_keep)
        else:
            xs = self.transformer(xs)[0]
        cls = xs.permute(1, 0, 2)[:, 0, :].contiguous()  # :307-309
        cls, _ = hip.layernorm(cls, self.ln_post.weight, self.ln_post.bias, self.ln_post.eps)
        if self.proj is not None:  # x @ proj  :311-312
            pj = self._cache.get(("proj", cdt), [self.proj], lambda: prepare_linear([self.proj.t()], None, cdt))
            cls = hip.gemm(to_compute(cls), pj.w, None, out_dtype=torch.float32, n=pj.n)
        return cls, sd_img_ft_all


class CLIP(nn.Module):
    """clip/model.py:316-652: the towers, embeddings and projections with the reference's parameter names (checkpoints load by
    key), encode_image :482-483 and encode_text :485-503.

    evaluate=True is the evaluation model: the momentum copies `*_m` and the queues of :395-437 are not created
    (load_state_dict(strict=False), as build_model :715 does, skips them) and forward() raises.  evaluate=False adds the
    reference's training state under its names - visual_m, transformer_m, token_embedding_m, ln_final_m, text_projection_m,
    positional_embedding_m, image_queue, text_queue, idx_queue, ptr_queue - and forward() is the contrastive training step of
    :529-595 (see CLIP.forward).  queue_size: the reference hard-codes 57600 (:430); a keyword here, as in BLIP_Retrieval."""

    def __init__(self, embed_dim: int, image_resolution: int, vision_layers, vision_width: int, vision_patch_size: int,
                 context_length: int, vocab_size: int, transformer_width: int, transformer_heads: int,
                 transformer_layers: int, evaluate: bool = True, config=None, queue_size: int = 57600):
        super().__init__()
        self.context_length = context_length
        self.sd_num = 100 if config is None else config['sd_num']
        self.sd_dim = 768 if config is None else config['sd_dim']
        self.space_dict = nn.Parameter(torch.randn(self.sd_num, self.sd_dim))
        if isinstance(vision_layers, (tuple, list)):
            raise NotImplementedError("ModifiedResNet vision towers (clip/model.py:94-155) are off the pruned ViT path")
        self.visual = VisionTransformer(input_resolution=image_resolution, patch_size=vision_patch_size, width=vision_width,
                                        layers=vision_layers, heads=vision_width // 64, output_dim=embed_dim, sd_dim=self.sd_dim)
        self.transformer = Transformer(width=transformer_width, layers=transformer_layers, heads=transformer_heads,
                                       attn_mask=self.build_attention_mask(), sd_dim=self.sd_dim)
        self.vocab_size = vocab_size
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(self.context_length, transformer_width))
        self.ln_final = LayerNorm(transformer_width)
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * 2.6592600369327779)  # log(1 / 0.07)
        self.embed_dim = embed_dim
        self.tokenize = None
        self.vision_layers, self.transformer_layers = vision_layers, transformer_layers
        self._cache = PreparedCache()
        self.evaluate = evaluate
        if evaluate:
            return
        self.initialize_parameters()
        # the training state of :347, :395-437, the reference's names and order
        self.criterion = nn.CosineEmbeddingLoss()
        self.momentum = 0.995
        self.visual_m = VisionTransformer(input_resolution=image_resolution, patch_size=vision_patch_size, width=vision_width,
                                          layers=vision_layers, heads=vision_width // 64, output_dim=embed_dim, sd_dim=self.sd_dim)
        self.transformer_m = Transformer(width=transformer_width, layers=transformer_layers, heads=transformer_heads,
                                         attn_mask=self.build_attention_mask(), sd_dim=self.sd_dim)
        self.token_embedding_m = nn.Embedding(vocab_size, transformer_width)
        self.ln_final_m = LayerNorm(transformer_width)
        self.model_pairs = [[self.visual, self.visual_m], [self.transformer, self.transformer_m],
                            [self.token_embedding, self.token_embedding_m], [self.ln_final, self.ln_final_m]]
        self.text_projection_m = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.positional_embedding_m = nn.Parameter(torch.empty(self.context_length, transformer_width))
        self.params_pairs = [[self.text_projection, self.text_projection_m],
                             [self.positional_embedding, self.positional_embedding_m]]
        self.copy_params()
        self.queue_size = queue_size
        self.register_buffer("image_queue", F.normalize(torch.randn(embed_dim, queue_size), dim=0))
        self.register_buffer("text_queue", F.normalize(torch.randn(embed_dim, queue_size), dim=0))
        self.register_buffer("idx_queue", torch.full((1, queue_size), -100))
        self.register_buffer("ptr_queue", torch.zeros(1, dtype=torch.long))
        self._ema = hip.EmaTable()
        self._ema_pairs = None  # [(param_m, param)] of momentum_pairs(), built at the first update
        self._ptr_host = None   # host mirror of ptr_queue: (value, ptr_queue._version it was read / written at)

    def initialize_parameters(self):
        """clip/model.py:438-464."""
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        proj_std = (self.transformer.width ** -0.5) * ((2 * self.transformer.layers) ** -0.5)
        attn_std = self.transformer.width ** -0.5
        fc_std = (2 * self.transformer.width) ** -0.5
        for block in self.transformer.resblocks:
            nn.init.normal_(block.attn.in_proj_weight, std=attn_std)
            nn.init.normal_(block.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(block.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(block.mlp.c_proj.weight, std=proj_std)
        nn.init.normal_(self.text_projection, std=self.transformer.width ** -0.5)

    def build_attention_mask(self):
        """clip/model.py:466-472: additive causal mask, -inf above the diagonal."""
        mask = torch.empty(self.context_length, self.context_length)
        mask.fill_(float("-inf"))
        mask.triu_(1)
        return mask

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    def encode_image(self, image, space_dict=None, temperature=0):
        return self.visual(image, space_dict=space_dict, temperature=temperature)  # :482-483

    def encode_text(self, text, space_dict=None, temperature=0):
        """:485-503.  -> (features [B, embed_dim], sd_txt_ft_all)"""
        require_gpu(text, "text")
        B, L = text.shape
        # token + positional embeddings: an embedding-row gather and an add (the BERT kernel with its LayerNorm does not apply)
        x = (self.token_embedding.weight[text] + self.positional_embedding[:L]).float().contiguous()  # :486-488
        eot = text.argmax(dim=-1)
        max_keep = eot.max() + 2  # :492
        xs = x.permute(1, 0, 2)  # NLD -> LND (a view)
        xs, _, _, sd_txt_ft_all, _ = self.transformer(xs, space_dict, temperature, None, max_keep)  # :493
        xb = as_f32_contig(xs.permute(1, 0, 2))
        rows = xb[torch.arange(B, device=xb.device), eot].contiguous()  # :501 (LayerNorm is row-wise: gather first)
        rows, _ = hip.layernorm(rows, self.ln_final.weight, self.ln_final.bias, self.ln_final.eps)  # :497
        cdt = compute_dtype()
        pj = self._cache.get(("text_projection", cdt), [self.text_projection],
                             lambda: prepare_linear([self.text_projection.t()], None, cdt))
        return hip.gemm(to_compute(rows), pj.w, None, out_dtype=torch.float32, n=pj.n), sd_txt_ft_all

    # ---- training state (evaluate=False): clip/model.py:505-652 ----
    def encode_image_m(self, image, space_dict=None, temperature=0):
        return self.visual_m(image, space_dict=space_dict, temperature=temperature)  # :505-506

    def encode_text_m(self, text, space_dict=None, temperature=0):
        """:508-526 as written: token_embedding_m, positional_embedding_m and text_projection_m around the STUDENT's
        self.transformer and self.ln_final (:516, :520) - transformer_m and ln_final_m follow the EMA and never run."""
        require_gpu(text, "text")
        B = text.shape[0]
        x = hip.clip_embed(text.contiguous(), self.token_embedding_m.weight.detach(), self.positional_embedding_m.detach())  # :509-511
        eot = text.argmax(dim=-1)
        max_keep = eot.max() + 2  # :515
        xs, _, _, sd_txt_ft_all, _ = self.transformer(x.permute(1, 0, 2), space_dict, temperature, None, max_keep)  # :516
        xb = as_f32_contig(xs.permute(1, 0, 2))
        rows = xb[torch.arange(B, device=xb.device), eot].contiguous()  # :524
        rows, _ = hip.layernorm(rows, self.ln_final.weight, self.ln_final.bias, self.ln_final.eps)  # :520
        cdt = compute_dtype()
        pj = self._cache.get(("text_projection_m", cdt), [self.text_projection_m],
                             lambda: prepare_linear([self.text_projection_m.t()], None, cdt))
        return hip.gemm(to_compute(rows), pj.w, None, out_dtype=torch.float32, n=pj.n), sd_txt_ft_all

    @staticmethod
    def _remove_alpha(model):
        return [param for name, param in model.named_parameters() if 'alpha' not in name]

    def momentum_pairs(self):
        """[(param, param_m)] of :621-643: the module pairs by position after dropping names containing 'alpha', then the two
        bare parameter pairs."""
        pairs = [(p, pm) for a, m in self.model_pairs for p, pm in zip(self._remove_alpha(a), m.parameters())]
        return pairs + [(p, pm) for p, pm in self.params_pairs]

    @torch.no_grad()
    def copy_params(self):  # :620-632
        for p, pm in self.momentum_pairs():
            pm.data.copy_(p.data)
            pm.requires_grad = False

    @torch.no_grad()
    def _momentum_update(self):
        """:634-643 p_m = p_m m + p (1 - m) for every pair, the two bare parameters included, in one launch (madtp_ema_update),
        in place, and noted (runtime.note_updated) so that prepared weights follow."""
        if self._ema_pairs is None:
            self._ema_pairs = [(pm, p) for p, pm in self.momentum_pairs()]
        self._ema.update(self._ema_pairs, self.momentum)
        note_updated([pm for pm, _ in self._ema_pairs])

    @torch.no_grad()
    def _dequeue_and_enqueue(self, image_feat, text_feat, idxs):
        """:598-618 with the pointer mirrored on the host (no int(ptr_queue) sync once it is known)."""
        from .blip_retrieval import _all_gather
        image_feats, text_feats = _all_gather(image_feat), _all_gather(text_feat)
        n = image_feats.shape[0]
        if self._ptr_host is None or self._ptr_host[1] != self.ptr_queue._version:
            self._ptr_host = (int(self.ptr_queue[0]), self.ptr_queue._version)
        ptr = self._ptr_host[0]
        assert self.queue_size % n == 0  # for simplicity (:607)
        if ptr % n != 0:
            ptr = (ptr // n) * n
        self.image_queue[:, ptr:ptr + n] = image_feats.T
        self.text_queue[:, ptr:ptr + n] = text_feats.T
        self.idx_queue[:, ptr:ptr + n] = idxs.view(1, -1)
        ptr = (ptr + n) % self.queue_size
        self.ptr_queue.fill_(ptr)
        self._ptr_host = (ptr, self.ptr_queue._version)

    @torch.no_grad()
    def reset_queue(self):  # :645-652
        dev = self.image_queue.device
        self.image_queue = F.normalize(torch.randn(self.embed_dim, self.queue_size), dim=0).to(dev)
        self.text_queue = F.normalize(torch.randn(self.embed_dim, self.queue_size), dim=0).to(dev)
        self.idx_queue = torch.full((1, self.queue_size), -100).to(dev)
        self.ptr_queue = torch.zeros(1, dtype=torch.long).to(dev)
        self._ptr_host = None

    def _fdt(self, sd_img_ft, sd_txt_ft):  # :578-584
        si = sd_img_ft / (sd_img_ft.norm(dim=-1, keepdim=True) + 1e-10)
        st = sd_txt_ft / (sd_txt_ft.norm(dim=-1, keepdim=True) + 1e-10)
        si, st = si.reshape(-1, self.sd_dim), st.reshape(-1, self.sd_dim)
        labels = torch.ones(si.shape[0], device=st.device).long()
        return self.criterion(si, st, labels)

    def forward(self, image, caption, alpha, idx, temperature=0):
        """The training step of clip/model.py:529-595 -> (loss_ita, loss_fdt, loss_fdt_m).  evaluate=False models only.

        caption: raw strings with model.tokenize set (as the reference's driver does), or an int tensor [B, context] of token ids,
        passed through.  idx: int [B] image ids.  Student towers on the autograd routes of the HIP path
        (backward.clip_vision_forward_with_grad / clip_text_forward_with_grad); then, under no_grad, the EMA (madtp_ema_update)
        and the momentum pass on the inference kernels - the reference as written: encode_text_m runs the student's transformer
        and ln_final a second time.  ITC: madtp_itc_loss per direction against [in-batch momentum features | queue] at
        temp = exp(-logit_scale) formed on the device, BEFORE the queues advance (the gradient is formed there); the STUDENT
        features are what the reference enqueues (:572).  temperature = 0: loss_fdt and loss_fdt_m are loss_ita itself.
        With a process group the features and ids are gathered for the queue (blip_retrieval._all_gather).
        Needs runtime.precision('fp32') or 'f16x3' (with runtime.training_f16x3()); embed_dim % 64 == 0 and <= 1024 (madtp_itc_loss)."""
        if self.evaluate:
            raise NotImplementedError("CLIP(evaluate=True) is the evaluation model (encode_image / encode_text): build it with "
                                      "evaluate=False to train")
        from .backward import _check_mode, clip_text_forward_with_grad
        from .blip_retrieval import _ItcLoss, _all_gather, _dist_world
        _check_mode("CLIP.forward (training)")
        require_gpu(image, "image")
        dev = image.device
        with torch.no_grad():
            self.logit_scale.clamp_(0, 4.6052)  # :530-531
        B = image.size(0)
        world = _dist_world()
        if self.queue_size % (world * B) != 0:  # :607 (checked on the host, before any state moves)
            raise AssertionError(f"queue_size {self.queue_size} is not a multiple of the gathered batch {world * B}")
        idx = idx.to(device=dev, dtype=torch.int64).view(-1).contiguous()
        sd = self.space_dict

        image_features, sd_img_ft = self.encode_image(image, space_dict=sd, temperature=temperature)  # :537
        if torch.is_tensor(caption) and not caption.is_floating_point():
            text = caption.to(device=dev, dtype=torch.int64)
        elif self.tokenize is not None:
            text = self.tokenize(caption).to(device=dev, dtype=torch.int64)  # :538
        else:
            raise TypeError("caption must be an int tensor [B, context] of token ids, or model.tokenize must be set")
        text = text.contiguous()
        if torch.is_grad_enabled():
            text_features, sd_txt_ft = clip_text_forward_with_grad(self, text, sd, temperature)  # :539
        else:
            text_features, sd_txt_ft = self.encode_text(text, space_dict=sd, temperature=temperature)
        image_features = image_features / image_features.norm(dim=1, keepdim=True)  # :542-543
        text_features = text_features / text_features.norm(dim=1, keepdim=True)
        temp = torch.exp(-self.logit_scale)  # s = q k / temp = exp(logit_scale) q k (:545, :563-564)

        with torch.no_grad():  # :547-552 momentum features (the EMA first)
            self._momentum_update()
            image_features_m, sd_img_ft_m = self.encode_image_m(image, space_dict=sd, temperature=temperature)
            text_features_m, sd_txt_ft_m = self.encode_text_m(text, space_dict=sd, temperature=temperature)
            image_features_m = (image_features_m / image_features_m.norm(dim=1, keepdim=True)).contiguous()
            text_features_m = (text_features_m / text_features_m.norm(dim=1, keepdim=True)).contiguous()

        # :533-536, :553-569 ITC against [in-batch momentum features | queue] (the queue as it is BEFORE this step's enqueue)
        idx_q = self.idx_queue[0]
        loss_i2t = _ItcLoss.apply(image_features, temp, image_features_m, text_features_m, self.text_queue, idx, idx_q, float(alpha))
        loss_t2i = _ItcLoss.apply(text_features, temp, text_features_m, image_features_m, self.image_queue, idx, idx_q, float(alpha))
        loss_ita = (loss_i2t + loss_t2i) / 2

        idxs = _all_gather(idx)  # :571-572
        self._dequeue_and_enqueue(image_features.detach(), text_features.detach(), idxs)

        loss_fdt = loss_ita
        loss_fdt_m = loss_ita
        if temperature != 0 and sd_img_ft is not None and sd_txt_ft is not None:  # :576-584
            loss_fdt = self._fdt(sd_img_ft, sd_txt_ft)
        if temperature != 0 and sd_img_ft_m is not None and sd_txt_ft_m is not None:  # :586-593
            with torch.no_grad():
                loss_fdt_m = self._fdt(sd_img_ft_m, sd_txt_ft_m)
        return loss_ita, loss_fdt, loss_fdt_m


def build_model(state_dict: dict, evaluate: bool = False, config=None):
    """clip/model.py:678-716: geometry inferred from the checkpoint's tensor shapes (ViT towers), strict=False load.  The
    reference casts weights to fp16 (convert_weights :653-675) and back to fp32 (clip/clip.py:148); here they stay fp32.
    evaluate=False (the reference's default, and what the driver's training model is built with) gives the model with the
    momentum copies and queues; as in the reference they are not re-copied after the load - the driver's checkpoints carry them."""
    if "visual.proj" not in state_dict:
        raise NotImplementedError("ResNet CLIP checkpoints are off the pruned ViT path")
    vision_width = state_dict["visual.conv1.weight"].shape[0]
    vision_layers = len([k for k in state_dict.keys() if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")])
    vision_patch_size = state_dict["visual.conv1.weight"].shape[-1]
    grid_size = round((state_dict["visual.positional_embedding"].shape[0] - 1) ** 0.5)
    image_resolution = vision_patch_size * grid_size
    embed_dim = state_dict["text_projection"].shape[1]
    context_length = state_dict["positional_embedding"].shape[0]
    vocab_size = state_dict["token_embedding.weight"].shape[0]
    transformer_width = state_dict["ln_final.weight"].shape[0]
    transformer_heads = transformer_width // 64
    transformer_layers = len(set(k.split(".")[2] for k in state_dict if k.startswith("transformer.resblocks")))
    model = CLIP(embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size, context_length, vocab_size,
                 transformer_width, transformer_heads, transformer_layers, evaluate, config)
    sd = {k: v for k, v in state_dict.items() if k not in ("input_resolution", "context_length", "vocab_size")}
    model.load_state_dict(sd, strict=False)
    return model

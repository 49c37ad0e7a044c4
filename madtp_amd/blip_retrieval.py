"""Mirror of the reference's models/blip_retrieval.py BLIP_Retrieval and of compress_retrieval_dtp.py evaluate() (:84-207).

evaluate=True (the reference driver's evaluation model, compress_retrieval_dtp.py:350-373) builds the modules evaluation uses
(:19-66) - text features, image features with the cross-batch CLS-repeat padding, similarity matrix, ITM re-ranking of the top
k_test candidates in both directions - and forward() raises.  evaluate=False (the driver's training model) adds the training
state of :67-93 under the reference's names (visual_encoder_m, vision_proj_m, text_encoder_m, text_proj_m, image_queue,
text_queue, idx_queue, ptr_queue, temp), so reference checkpoints load by key, and forward() is the ITC / ITM training step
of :99-282 (see BLIP_Retrieval.forward).

Everything heavy runs through the HIP library (pruned ViT, MED BERT in text and multimodal mode, projections, ITM head, and
for training the contrastive loss over the queues, the EMA of the momentum encoders and the hard-negative draw of
csrc/retrieval.hip); torch only does the glue the reference does in torch as well (topk, row gathers, normalisation of
[n,256] features, the queue writes) - on the GPU, the image tokens never visit the host."""
import os

import torch
import torch.nn.functional as F
from torch import nn

from . import hip
from .bert import BertConfig
from .blip_nlvr import ENC_TOKEN_ID, create_vit
from .bert import EncoderKVCache
from .med import BertModel
from .runtime import PreparedCache, compute_dtype, lin_of, note_updated, require_gpu, to_compute


def _dist_world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size()
    return 1


def _all_gather(t):
    """concat_all_gather of blip_retrieval.py:335-345 (no gradient); identity at world 1.  gloo gathers through the host."""
    import torch.distributed as dist
    if _dist_world() == 1:
        return t
    src = t if dist.get_backend() == "nccl" else t.cpu()
    parts = [torch.empty_like(src) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, src.contiguous())
    return torch.cat(parts, 0).to(t.device)


class _GatherWithGrad(torch.autograd.Function):
    """all_gather_with_grad of blip_retrieval.py:348-380: the gradient of this rank's slice is the SUM over the ranks of the
    gradients of the gathered tensor (all_reduce), as the reference's GatherLayer does."""

    @staticmethod
    def forward(ctx, x):
        return _all_gather(x)

    @staticmethod
    def backward(ctx, g):
        import torch.distributed as dist
        src = g.contiguous() if dist.get_backend() == "nccl" else g.cpu().contiguous()
        dist.all_reduce(src)
        B = g.shape[0] // dist.get_world_size()
        r = dist.get_rank()
        return src[r * B:(r + 1) * B].to(g.device)


class _ItcLoss(torch.autograd.Function):
    """mean over rows of one direction of the contrastive loss (madtp_itc_loss).  The gradient is formed in the forward, before
    the queue is overwritten; backward only scales it by grad_out."""

    @staticmethod
    def forward(ctx, q, temp, q_m, keys_batch, queue, idx, idx_queue, alpha):
        loss, dq, dtemp = hip.itc_loss(q.contiguous(), q_m.contiguous(), keys_batch.contiguous(), queue, idx, idx_queue,
                                       temp.detach().reshape(1), alpha)
        ctx.save_for_backward(dq, dtemp)
        ctx.temp_shape = temp.shape
        return loss.mean()

    @staticmethod
    def backward(ctx, g):
        dq, dtemp = ctx.saved_tensors
        return dq * g, (dtemp * g).reshape(ctx.temp_shape), None, None, None, None, None, None


class BLIP_Retrieval(nn.Module):
    def __init__(self, med_config='configs/med_config.json', image_size=384, vit='base', vit_grad_ckpt=False,
                 vit_ckpt_layer=0, embed_dim=256, queue_size=57600, momentum=0.995, negative_all_rank=False,
                 evaluate=False, config=None):
        super().__init__()
        if config is None:
            self.sd_num, self.sd_dim = 100, 768
        else:
            self.sd_num, self.sd_dim = config['sd_num'], config['sd_dim']
        self.space_dict = nn.Parameter(torch.randn(self.sd_num, self.sd_dim))
        self.world_size = int(os.environ.get('WORLD_SIZE', 1))
        self.layers = 12
        self.visual_encoder, vision_width = create_vit(vit, image_size, vit_grad_ckpt, vit_ckpt_layer, 0,
                                                       evaluate=evaluate, sd_dim=self.sd_dim)
        self.tokenizer = None  # set to a BertTokenizer-like callable to pass raw strings, as the reference does
        if isinstance(med_config, str):
            med_config = BertConfig.from_json_file(med_config) if os.path.exists(med_config) else BertConfig.med_default()
        med_config.encoder_width = vision_width
        med_config.evaluate = evaluate
        self.text_encoder = BertModel(config=med_config, add_pooling_layer=False, sd_dim=self.sd_dim)
        text_width = self.text_encoder.config.hidden_size
        self.vision_proj = nn.Linear(vision_width, embed_dim)
        self.text_proj = nn.Linear(text_width, embed_dim)
        self.itm_head = nn.Linear(text_width, 2)
        self.queue_size, self.momentum, self.negative_all_rank = queue_size, momentum, negative_all_rank
        self._cache = PreparedCache()
        self.evaluate = evaluate
        if evaluate:
            return
        # the training state of :67-93, the reference's names and order
        self.criterion = nn.CosineEmbeddingLoss()
        self.visual_encoder_m, vision_width = create_vit(vit, image_size, evaluate=evaluate, sd_dim=self.sd_dim)
        self.vision_proj_m = nn.Linear(vision_width, embed_dim)
        self.text_encoder_m = BertModel(config=med_config, add_pooling_layer=False, sd_dim=self.sd_dim)
        self.text_proj_m = nn.Linear(text_width, embed_dim)
        self.model_pairs = [[self.visual_encoder, self.visual_encoder_m], [self.vision_proj, self.vision_proj_m],
                            [self.text_encoder, self.text_encoder_m], [self.text_proj, self.text_proj_m]]
        self.copy_params()
        self.register_buffer("image_queue", F.normalize(torch.randn(embed_dim, queue_size), dim=0))
        self.register_buffer("text_queue", F.normalize(torch.randn(embed_dim, queue_size), dim=0))
        self.register_buffer("idx_queue", torch.full((1, queue_size), -100))
        self.register_buffer("ptr_queue", torch.zeros(1, dtype=torch.long))
        self.temp = nn.Parameter(0.07 * torch.ones([]))
        # itm_uniforms: None (torch.rand(2, B) on the device, seeded by torch.manual_seed) or a f32 [2,B] tensor of uniforms in
        # [0,1) for the hard-negative draw - row 0 picks each text's negative image, row 1 each image's negative text
        self.itm_uniforms = None
        self._ema = hip.EmaTable()
        self._ema_pairs = None       # [(param_m, param)] of momentum_pairs(), built at the first update
        self._ptr_host = None        # host mirror of ptr_queue: (value, ptr_queue._version it was read / written at)
        self._neg_flag = None        # device int32: set by madtp_itm_negatives when a row had no admissible negative
        self._neg_flag_host = None   # pinned copy of it, read at the next forward after its event
        self._neg_flag_event = None
        self.last_negatives = None   # int64 [2,B] of the last forward (world columns): the drawn negative image / text

    @staticmethod
    def _remove_alpha(model):
        return [param for name, param in model.named_parameters() if 'alpha' not in name]

    def momentum_pairs(self):
        """[(param, param_m)] of :287-300, paired by position after dropping names containing 'alpha' (remove_alpha)."""
        return [(p, pm) for a, m in self.model_pairs for p, pm in zip(self._remove_alpha(a), m.parameters())]

    @torch.no_grad()
    def copy_params(self):  # :285-291
        for p, pm in self.momentum_pairs():
            pm.data.copy_(p.data)
            pm.requires_grad = False

    @torch.no_grad()
    def _momentum_update(self):
        """:293-300 p_m = p_m m + p (1 - m) for every pair in one launch (madtp_ema_update), in place.  The reference assigns new
        storage; here the storage stays and the update is noted, so that the prepared weights of the momentum towers are rebuilt."""
        if self._ema_pairs is None:
            self._ema_pairs = [(pm, p) for p, pm in self.momentum_pairs()]
        self._ema.update(self._ema_pairs, self.momentum)
        note_updated([pm for pm, _ in self._ema_pairs])

    def forward(self, image, caption, alpha, idx, temperature=0, train=True):
        """The training step of blip_retrieval.py:99-282 -> (loss_ita, loss_itm, loss_fdt, loss_fdt_m).  evaluate=False models only.

        caption: {'input_ids', 'attention_mask'} tensors (or raw strings with model.tokenizer set), idx: int64 [B] image ids.
        Student towers on the autograd routes of the HIP path; momentum towers (after the EMA, madtp_ema_update) on the inference
        path under no_grad at the same temperature.  ITC: madtp_itc_loss per direction against [in-batch | queue] BEFORE the
        queues advance (the gradient is formed there).  ITM: hard negatives drawn by madtp_itm_negatives at uniforms
        `itm_uniforms` (default torch.rand on the device) - the inverse CDF of the masked softmax weights; a row with no
        admissible negative (every column shares its id, where torch.multinomial raises) makes the NEXT forward raise.
        With a process group: the momentum features and ids are gathered for the queue (it advances by world * B), and with
        negative_all_rank the negatives are drawn from every rank's batch (image_embeds gathered with gradient; the ranks must
        hold image tokens of one length).  Needs runtime.precision('fp32') or 'f16x3'; model.train() applies the reference's
        dropout / DropPath with the counter-based masks (runtime.set_dropout_seed)."""
        if self.evaluate:
            raise NotImplementedError("BLIP_Retrieval(evaluate=True) is the evaluation model (compress_retrieval_dtp.py:350-373): "
                                      "build it with evaluate=False to train, or use blip_retrieval.evaluate()")
        from .backward import LinearFunction, _check_mode
        _check_mode("BLIP_Retrieval.forward (training)")
        require_gpu(image, "image")
        dev = image.device
        self._raise_pending_negative_error()
        with torch.no_grad():
            self.temp.clamp_(0.001, 0.5)
        sd = self.space_dict
        B = image.size(0)
        world = _dist_world()
        if self.queue_size % (world * B) != 0:  # :307 (checked on the host)
            raise AssertionError(f"queue_size {self.queue_size} is not a multiple of the gathered batch {world * B}")

        image_embeds, sd_img_ft = self.visual_encoder(image, space_dict=sd, temperature=temperature)  # :103
        image_atts = torch.ones(image_embeds.size()[:-1], dtype=torch.long, device=dev)
        image_feat = F.normalize(LinearFunction.apply(image_embeds[:, 0, :].contiguous(), self.vision_proj.weight,
                                                      self.vision_proj.bias, hip.ACT_NONE), dim=-1)  # :105
        ids, att = _tokens(self, caption, dev)  # :107-108
        text_output, sd_txt_ft = self.text_encoder(ids, attention_mask=att, return_dict=True, mode='text', space_dict=sd,
                                                   temperature=temperature)  # :110-113
        text_feat = F.normalize(LinearFunction.apply(text_output.last_hidden_state[:, 0, :].contiguous(), self.text_proj.weight,
                                                     self.text_proj.bias, hip.ACT_NONE), dim=-1)  # :114

        idx = idx.to(dev).view(-1)
        with torch.no_grad():  # :122-139 momentum features (the EMA first, as :123)
            self._momentum_update()
            image_embeds_m, sd_img_ft_m = self.visual_encoder_m(image, space_dict=sd, temperature=temperature)
            image_feat_m = F.normalize(self._linear("vp_m", self.vision_proj_m, image_embeds_m[:, 0, :]), dim=-1)
            text_output_m, sd_txt_ft_m = self.text_encoder_m(ids, attention_mask=att, return_dict=True, mode='text',
                                                             space_dict=sd, temperature=temperature)
            text_feat_m = F.normalize(self._linear("tp_m", self.text_proj_m, text_output_m.last_hidden_state[:, 0, :]), dim=-1)
            image_feat_m, text_feat_m = image_feat_m.contiguous(), text_feat_m.contiguous()

        # :116-150 ITC against [in-batch momentum features | queue] (the queue as it is BEFORE this step's enqueue)
        idx_q = self.idx_queue[0]
        loss_i2t = _ItcLoss.apply(image_feat, self.temp, image_feat_m, text_feat_m, self.text_queue, idx, idx_q, float(alpha))
        loss_t2i = _ItcLoss.apply(text_feat, self.temp, text_feat_m, image_feat_m, self.image_queue, idx, idx_q, float(alpha))
        loss_ita = (loss_i2t + loss_t2i) / 2

        loss_fdt = loss_ita
        loss_fdt_m = loss_ita
        if temperature != 0 and sd_img_ft is not None and sd_txt_ft is not None and train:  # :154-162
            loss_fdt = self._fdt(sd_img_ft, sd_txt_ft)
        if temperature != 0 and sd_img_ft_m is not None and sd_txt_ft_m is not None and train:  # :164-171
            with torch.no_grad():
                loss_fdt_m = self._fdt(sd_img_ft_m, sd_txt_ft_m)

        idxs = _all_gather(idx)  # :173-174
        self._dequeue_and_enqueue(image_feat_m, text_feat_m, idxs)

        # :176-282 ITM
        encoder_input_ids = ids.clone()
        encoder_input_ids[:, 0] = ENC_TOKEN_ID
        output_pos, _ = self.text_encoder(encoder_input_ids, attention_mask=att, encoder_hidden_states=image_embeds,
                                          encoder_attention_mask=image_atts, return_dict=True, space_dict=sd,
                                          temperature=temperature)  # :180-187
        if self.negative_all_rank and world > 1:
            self._check_equal_lengths(image_embeds.shape[1])
            with torch.no_grad():
                image_feat_world = _all_gather(image_feat.detach().contiguous())
                text_feat_world = _all_gather(text_feat.detach().contiguous())
            image_embeds_world = _GatherWithGrad.apply(image_embeds)
            input_ids_world = _all_gather(encoder_input_ids)
            att_world = _all_gather(att)
            idx_world = idxs
        else:
            image_feat_world, text_feat_world = image_feat.detach(), text_feat.detach()
            image_embeds_world, input_ids_world, att_world, idx_world = image_embeds, encoder_input_ids, att, idx
        neg = self._draw_negatives(image_feat.detach().contiguous(), text_feat.detach().contiguous(),
                                   image_feat_world.contiguous(), text_feat_world.contiguous(), idx, idx_world.contiguous())
        sel = neg.clamp_min(0)  # -1 (no admissible negative) is reported by the next forward; never used as an index
        image_embeds_neg = image_embeds_world.index_select(0, sel[0])
        text_ids_neg = input_ids_world.index_select(0, sel[1])
        text_atts_neg = att_world.index_select(0, sel[1])

        text_ids_all = torch.cat([encoder_input_ids, text_ids_neg], dim=0)  # :260-264
        text_atts_all = torch.cat([att, text_atts_neg], dim=0)
        image_embeds_all = torch.cat([image_embeds_neg, image_embeds], dim=0)
        image_atts_all = torch.cat([image_atts, image_atts], dim=0)
        output_neg, _ = self.text_encoder(text_ids_all, attention_mask=text_atts_all, encoder_hidden_states=image_embeds_all,
                                          encoder_attention_mask=image_atts_all, return_dict=True, space_dict=sd,
                                          temperature=temperature)  # :266-273
        vl_embeddings = torch.cat([output_pos.last_hidden_state[:, 0, :], output_neg.last_hidden_state[:, 0, :]], dim=0)
        vl_output = LinearFunction.apply(vl_embeddings.contiguous(), self.itm_head.weight, self.itm_head.bias, hip.ACT_NONE)
        itm_labels = torch.cat([torch.ones(B, dtype=torch.long), torch.zeros(2 * B, dtype=torch.long)], dim=0).to(dev)
        loss_itm = F.cross_entropy(vl_output, itm_labels)  # :280
        return loss_ita, loss_itm, loss_fdt, loss_fdt_m

    def _fdt(self, sd_img_ft, sd_txt_ft):
        si = sd_img_ft / (sd_img_ft.norm(dim=-1, keepdim=True) + 1e-10)
        st = sd_txt_ft / (sd_txt_ft.norm(dim=-1, keepdim=True) + 1e-10)
        si, st = si.reshape(-1, self.sd_dim), st.reshape(-1, self.sd_dim)
        labels = torch.ones(si.shape[0], device=st.device).long()
        return self.criterion(si, st, labels)

    def _check_equal_lengths(self, n):
        """The reference all_gathers image_embeds [B, n, 768]: undefined when pruning left the ranks different n.  Decided
        collectively before any gather, so that every rank raises together."""
        import torch.distributed as dist
        from . import dist as mdist
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"  # NCCL / RCCL reduce device tensors only
        lo, hi = mdist.min_over_ranks(float(n), device=dev), mdist.max_over_ranks(float(n), device=dev)
        if lo != hi:
            raise RuntimeError(f"negative_all_rank: the ranks hold image tokens of different lengths ({int(lo)} .. {int(hi)}) after "
                               "pruning; the reference's all_gather of image_embeds is undefined then (use temperature 0 or "
                               "negative_all_rank=False)")

    @torch.no_grad()
    def _dequeue_and_enqueue(self, image_feat_m, text_feat_m, idxs):
        """:302-322 with the pointer mirrored on the host (no int(ptr_queue) sync): stream-ordered after the ITC kernels."""
        image_feats, text_feats = _all_gather(image_feat_m), _all_gather(text_feat_m)
        n = image_feats.shape[0]
        if self._ptr_host is None or self._ptr_host[1] != self.ptr_queue._version:
            self._ptr_host = (int(self.ptr_queue[0]), self.ptr_queue._version)
        ptr = self._ptr_host[0]
        assert self.queue_size % n == 0
        if ptr % n != 0:
            ptr = (ptr // n) * n
        self.image_queue[:, ptr:ptr + n] = image_feats.T
        self.text_queue[:, ptr:ptr + n] = text_feats.T
        self.idx_queue[:, ptr:ptr + n] = idxs.view(1, -1)
        ptr = (ptr + n) % self.queue_size
        self.ptr_queue.fill_(ptr)
        self._ptr_host = (ptr, self.ptr_queue._version)

    def _draw_negatives(self, image_feat, text_feat, image_feat_world, text_feat_world, idx, idx_world):
        B = image_feat.shape[0]
        dev = image_feat.device
        if self._neg_flag is None or self._neg_flag.device != dev:
            self._neg_flag = torch.zeros(1, dtype=torch.int32, device=dev)
            self._neg_flag_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        u = self.itm_uniforms
        if u is None:
            u = torch.rand(2, B, device=dev)
        u = u.to(device=dev, dtype=torch.float32).contiguous()
        neg = hip.itm_negatives(image_feat, text_feat, image_feat_world, text_feat_world, idx.contiguous(), idx_world,
                                self.temp.detach().reshape(1), u, self._neg_flag)
        self._neg_flag_host.copy_(self._neg_flag, non_blocking=True)
        self._neg_flag_event = torch.cuda.Event()
        self._neg_flag_event.record()
        self.last_negatives = neg
        return neg

    def _raise_pending_negative_error(self):
        if self._neg_flag_event is None:
            return
        self._neg_flag_event.synchronize()
        self._neg_flag_event = None
        if int(self._neg_flag_host[0]) != 0:
            self._neg_flag.zero_()
            self._neg_flag_host.zero_()
            raise RuntimeError("BLIP_Retrieval: in the previous step a row had no admissible hard negative (every candidate shared "
                               "its idx; torch.multinomial raises there) - its ITM pair was drawn from column 0")

    # ---- the small Linears of the evaluation path on the library GEMM ----
    def _linear(self, key, lin, x32):
        l = lin_of(self._cache, key, [lin])  # (the momentum projections: the cache follows note_updated)
        return hip.gemm(to_compute(x32.contiguous()), l.w, l.b, out_dtype=torch.float32, n=l.n)

    def project_image(self, cls_rows):
        return F.normalize(self._linear("vp", self.vision_proj, cls_rows), dim=-1)  # compress_retrieval_dtp.py:121-122

    def project_text(self, cls_rows):
        return F.normalize(self._linear("tp", self.text_proj, cls_rows))  # :104

    def itm_score(self, cls_rows):
        return self._linear("itm", self.itm_head, cls_rows)[:, 1]  # :172


def blip_retrieval(pretrained='', **kwargs):
    model = BLIP_Retrieval(**kwargs)
    if pretrained:  # blip_retrieval.py (blip_retrieval) -> models/blip.py:254-278
        from .checkpoint import load_checkpoint
        model, msg = load_checkpoint(model, pretrained)
        print("missing keys:")
        print(msg.missing_keys)
    return model


def _tokens(model, text, device):
    if isinstance(text, dict) or hasattr(text, "input_ids"):
        ids = text["input_ids"] if isinstance(text, dict) else text.input_ids
        att = text["attention_mask"] if isinstance(text, dict) else text.attention_mask
    elif model.tokenizer is not None:
        t = model.tokenizer(text, padding='max_length', truncation=True, max_length=35, return_tensors="pt")
        ids, att = t.input_ids, t.attention_mask
    else:
        raise TypeError("dataset.text must yield {'input_ids','attention_mask'} tensors or model.tokenizer must be set "
                        "(no vocabulary offline)")
    return ids.to(device), att.to(device)


def all_reduce_scores(score_i2t, score_t2i):
    """compress_retrieval_dtp.py:200-203: SUM all-reduce of the two score matrices over the ranks (every rank filled only the
    rows of its slice, the rest is -100), so all entries re-ranked by some rank end up shifted by the same -100*(world-1)
    and the rankings of itm_eval() are those of a single-rank run.  numpy in, numpy out; no-op without a process group."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return score_i2t, score_t2i
    dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    a, b = torch.from_numpy(score_i2t.copy()).to(dev), torch.from_numpy(score_t2i.copy()).to(dev)
    dist.all_reduce(a, op=dist.ReduceOp.SUM)
    dist.all_reduce(b, op=dist.ReduceOp.SUM)
    return a.cpu().numpy(), b.cpu().numpy()


def rank_rows(n, rank, world_size):
    """Row slice [start, end) of an n-row score matrix that `rank` fills (compress_retrieval_dtp.py:158-162 / :181-183)."""
    step = n // world_size + 1
    return min(n, rank * step), min(n, rank * step + step)


def all_gather_scores(score_i2t, score_t2i):
    """the exchange the path actually needs - every rank contributes only the ROWS it re-ranked (rank_rows) and
    all ranks end up with exactly the matrices of a single-rank evaluation (no -100*(world-1) shift, 1/world of the
    all-reduce's traffic: at COCO 5k x 25k the two SUM all-reduces move 2 x 500 MB per rank).  numpy in, numpy out; no-op
    without a process group.  Slices are padded to the common step so one all_gather per matrix suffices."""
    import numpy as np
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return score_i2t, score_t2i
    world, rank = dist.get_world_size(), dist.get_rank()
    dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    outs = []
    for m in (score_i2t, score_t2i):
        n, step = m.shape[0], m.shape[0] // world + 1
        s, e = rank_rows(n, rank, world)
        mine = np.full((step, m.shape[1]), -100.0, dtype=m.dtype)
        mine[:e - s] = m[s:e]
        parts = [torch.empty((step, m.shape[1]), dtype=torch.from_numpy(mine).dtype, device=dev) for _ in range(world)]
        dist.all_gather(parts, torch.from_numpy(mine).to(dev))
        full = np.full_like(m, -100.0)
        for r, part in enumerate(parts):
            rs, re = rank_rows(n, r, world)
            full[rs:re] = part[:re - rs].cpu().numpy()
        outs.append(full)
    return outs[0], outs[1]


def all_gather_lists(lists_i2t, lists_t2i):
    """all_gather_scores() for what evaluate(scores="lists") returns: every rank contributes the rows it re-ranked (rank_rows) of
    idx and val, padded to the common step, and all ranks end up with the lists of a single-rank evaluation, on the device the
    lists are on (through the host with a gloo group).  16 bytes per slot: n * k_test pairs instead of two n_img x n_txt
    matrices.  No-op without a process group."""
    import torch.distributed as dist
    from .lists import CandidateLists
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return lists_i2t, lists_t2i
    world, rank = dist.get_world_size(), dist.get_rank()
    outs = []
    for cl in (lists_i2t, lists_t2i):
        dev = cl.idx.device if dist.get_backend() == "nccl" else torch.device("cpu")
        (n, k), step = cl.idx.shape, cl.idx.shape[0] // world + 1
        s, e = rank_rows(n, rank, world)
        whole = []
        for t, empty in ((cl.idx, -1), (cl.val, cl.fill)):
            mine = torch.full((step, k), empty, dtype=t.dtype, device=dev)
            mine[:e - s] = t[s:e]
            parts = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(parts, mine)
            full = torch.full((n, k), empty, dtype=t.dtype, device=dev)
            for r, part in enumerate(parts):
                rs, re = rank_rows(n, r, world)
                full[rs:re] = part[:re - rs]
            whole.append(full.to(cl.idx.device))
        outs.append(CandidateLists(whole[0], whole[1], cl.nk, cl.fill))
    return outs[0], outs[1]


@torch.no_grad()
def evaluate(model, data_loader, device, config, temperature=0, rank=0, world_size=1, text_bs=256, kv_cache=True,
             candidates="dense", coarse=None, scores="dense"):
    """compress_retrieval_dtp.py evaluate() :84-207 -> (score_matrix_i2t, score_matrix_t2i) as numpy arrays and the GFLOPs
    placeholder (0.0: the reference's fvcore count of the TRAINING forward is out of scope, harness.nlvr_forward_flops is
    the analytic counter of this repo).  rank / world_size select this process's row slices exactly as :158-162 / :181-183
    do; the caller all-reduces the two matrices (SUM) when world_size > 1, as :200-203.
    kv_cache: project the image tokens to every layer's cross-attention [k|v] ONCE (EncoderKVCache) and let the re-ranking
    batches index that cache; False reproduces the reference's data flow (each pair re-projects its image).
    candidates: "dense" (the default, the reference's data flow) forms sims_matrix and takes topk(k_test) of one row per loop
    iteration; "device" takes the k_test candidates of all rows, in both directions, from two search.topk_embeds calls before the
    loops and never forms sims_matrix (its ITC term is the exact-f32 score of that kernel, its order among equal scores the one
    of madtp_search.h).
    coarse: None, or "bf16" with candidates="device": the same candidates through the certified bf16 shortlist of
    search.topk_embeds (k_test <= 128).
    scores: "dense" (the default) returns the two matrices; "lists" with candidates="device" returns (lists.CandidateLists image ->
    text, the same text -> image, 0.0) on the device instead: the k_test re-ranked values of a row next to the indices topk_embeds
    gave it, rows outside this rank's slice empty - the matrices are .to_dense() of them and are never allocated.  Several ranks
    exchange them with all_gather_lists(); retrieval_eval.itm_eval() takes them as they are."""
    if candidates not in ("dense", "device"):
        raise ValueError(f"candidates = {candidates!r}: expected 'dense' or 'device'")
    if scores not in ("dense", "lists"):
        raise ValueError(f"scores = {scores!r}: expected 'dense' or 'lists'")
    if scores == "lists" and candidates != "device":
        raise ValueError(f"scores = 'lists' needs candidates='device' (candidates = {candidates!r})")
    k_test = config['k_test']
    if coarse is not None:
        from . import search
        if candidates != "device":
            raise ValueError(f"coarse = {coarse!r} needs candidates='device'")
        search.check_coarse(coarse, k_test, "evaluate: k_test")
    sd = model.space_dict
    texts = data_loader.dataset.text
    num_text = len(texts)
    text_ids, text_embeds, text_atts = [], [], []
    for i in range(0, num_text, text_bs):  # :100-110
        ids, att = _tokens(model, texts[i:min(num_text, i + text_bs)], device)
        out, _ = model.text_encoder(ids, attention_mask=att, mode='text', space_dict=sd, temperature=temperature)
        text_embeds.append(model.project_text(out.last_hidden_state[:, 0, :]))
        text_ids.append(ids)
        text_atts.append(att)
    text_embeds = torch.cat(text_embeds, 0)
    text_ids = torch.cat(text_ids, 0).clone()
    text_atts = torch.cat(text_atts, 0)
    text_ids[:, 0] = ENC_TOKEN_ID  # :114

    image_feats, image_embeds = [], []
    for image, _caption, _img_id in data_loader:  # :118-125 (the tokens stay on the GPU)
        feat, _ = model.visual_encoder(require_gpu(image.to(device), "image"), space_dict=sd, temperature=temperature)
        image_embeds.append(model.project_image(feat[:, 0, :]))
        image_feats.append(feat)
    image_embeds = torch.cat(image_embeds, 0)
    n = max(f.shape[1] for f in image_feats)  # :141-153: batches pruned to different lengths, padded with their CLS row
    image_feats = torch.cat([torch.cat([f, f[:, 0:1, :].expand(-1, n - f.shape[1], -1)], 1) if f.shape[1] < n else f
                             for f in image_feats], 0)

    cache = EncoderKVCache.build(model.text_encoder, image_feats) if kv_cache else None

    def rerank(ids, att, img_index):
        if cache is not None:
            out = model.text_encoder(ids, attention_mask=att, return_dict=True, space_dict=sd, temperature=temperature,
                                     encoder_kv_cache=cache.select(img_index))[0]
        else:
            enc = image_feats[img_index].contiguous()
            enc_att = torch.ones(enc.shape[:-1], dtype=torch.long, device=device)
            out = model.text_encoder(ids, attention_mask=att, encoder_hidden_states=enc, encoder_attention_mask=enc_att,
                                     return_dict=True, space_dict=sd, temperature=temperature)[0]
        return model.itm_score(out.last_hidden_state[:, 0, :])

    n_img = image_embeds.shape[0]
    if candidates == "device":
        from . import search
        if k_test > min(n_img, num_text):  # (what topk() of the dense path refuses)
            raise RuntimeError(f"k_test = {k_test} exceeds the {n_img} images or the {num_text} texts")
        kw = {} if coarse is None else {"coarse": coarse}
        i2t_sim, i2t_idx = search.topk_embeds(image_embeds.float(), text_embeds.float(), k_test, **kw)
        t2i_sim, t2i_idx = search.topk_embeds(text_embeds.float(), image_embeds.float(), k_test, **kw)
        top_i2t, top_t2i = (lambda i: (i2t_sim[i], i2t_idx[i])), (lambda i: (t2i_sim[i], t2i_idx[i]))
    else:
        sims_matrix = image_embeds @ text_embeds.t()  # :155
        sims_t = sims_matrix.t()
        top_i2t, top_t2i = (lambda i: sims_matrix[i].topk(k=k_test, dim=0)), (lambda i: sims_t[i].topk(k=k_test, dim=0))
    if scores == "lists":
        from .lists import CandidateLists

        def reranked(n_rows, nk, sim, idx, pairs):
            """the loops below with row i's k_test values written next to its indices instead of scattered into a dense row;
            the rows of other ranks stay empty (the dense route leaves them at -100)"""
            start, end = rank_rows(n_rows, rank, world_size)
            val = torch.full((n_rows, k_test), -100.0, device=device)
            for i in range(start, end):
                val[i] = rerank(*pairs(i, idx[i])) + sim[i]
            held = torch.full_like(idx, -1)
            held[start:end] = idx[start:end]
            return CandidateLists(held, val, nk)
        return (reranked(n_img, num_text, i2t_sim, i2t_idx, lambda i, top: (
                    text_ids[top], text_atts[top], torch.full((k_test,), i, dtype=torch.long, device=device))),
                reranked(num_text, n_img, t2i_sim, t2i_idx, lambda i, top: (
                    text_ids[i].repeat(k_test, 1), text_atts[i].repeat(k_test, 1), top)), 0.0)
    score_i2t = torch.full((n_img, num_text), -100.0, device=device)
    start, end = rank_rows(n_img, rank, world_size)
    for i in range(start, end):  # :164-174
        topk_sim, topk_idx = top_i2t(i)
        score_i2t[i, topk_idx] = rerank(text_ids[topk_idx], text_atts[topk_idx],
                                        torch.full((k_test,), i, dtype=torch.long, device=device)) + topk_sim

    score_t2i = torch.full((num_text, n_img), -100.0, device=device)
    start, end = rank_rows(num_text, rank, world_size)
    for i in range(start, end):  # :186-198
        topk_sim, topk_idx = top_t2i(i)
        score_t2i[i, topk_idx] = rerank(text_ids[i].repeat(k_test, 1), text_atts[i].repeat(k_test, 1), topk_idx) + topk_sim
    return score_i2t.cpu().numpy(), score_t2i.cpu().numpy(), 0.0

"""The training kernels of csrc/backward.hip one by one against float64 autograd of the same operation, at the token counts training
runs (BLIP NLVR fine-tunes at 384^2: 577 tokens, VQA at 480^2: 901; the entries accept up to 1024 keys), with the branches the small
whole-layer fixtures never reach: key masks, the decoder's causal mask, attention_probs dropout, the pruning score's gradient terms
(da / dp0 / dnrm_scale), head arg-max ties, partial 16-row / 16-key tiles and several 64-key column blocks.

The kernels are exact f32 (16x16x4 f32 MFMA, fixed summation orders): errors are measured relative to each tensor's largest entry
and held to ~10x what the MI355X measured (the `# measured on MI355X` comments)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SCALE = 0.125  # head dim 64
DROP = (0.1, 0x5EED_0F_D40, 11)  # (p, seed, site) of the attention_probs dropout cases

# Tolerances, relative to each tensor's max |value|: ~10x the largest error measured on MI355X over each test's cases
# (max at N = 577 / 901 / 1024 in brackets where the test reaches them).
TOL_TRAIN = 1e-5   # measured on MI355X: P 1.1e-6 (3.0e-7 / 1.1e-6 / 7.6e-7), out 1.1e-6 (4.4e-7 / 1.1e-6 / 6.8e-7),
#                    colsum_part 6.0e-7, p0 9.4e-7, onorm 6.9e-7
TOL_BWD = 2e-5     # measured on MI355X: dq 1.1e-6 (1.1e-6 / 9.1e-7 / 1.1e-6), dk 2.0e-6 (1.3e-6 / 2.0e-6 / 1.8e-6),
#                    dv 2.1e-6 (2.1e-6 / 1.9e-6 / 1.7e-6), dp_out 4.5e-7 (4.5e-7 / 3.4e-7 / 4.1e-7)
TOL_CROSS = 1.5e-5  # measured on MI355X: dq 1.1e-6, dk 1.6e-6, dv 1.3e-6 (Nk = 1024: 1.1e-6 / 1.6e-6 / 1.3e-6)
TOL_SCORE = 3e-6   # measured on MI355X: dx 6.4e-8, dw 1.6e-7, da 3.2e-7, dp0 2.9e-7, dnrm_scale 2.9e-7, dtoken_attn 3.5e-7
TOL_LN = 2e-6      # measured on MI355X: dx 1.9e-7, dgamma 1.7e-7, dbeta 1.3e-7
TOL_PROBS = 1e-5   # measured on MI355X: attention_probs 7.4e-7, attention_probs_x 9.3e-7


@pytest.fixture(scope="module")
def hip():
    from madtp_amd import build, hip as h
    build.build(verbose=False)
    h.load()
    assert torch.cuda.is_available()
    return h


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-12)


def _report(what, errs, tol):
    """print the measured errors (the numbers behind the tolerances above) and hold every one to tol"""
    print(f"{what}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v < tol}
    assert not bad, f"{what}: {bad} of the tensor's maximum (tolerance {tol:.1e})"


def _key_mask(B, N, seed, dead_sample=True):
    """additive [B, N] key mask: -10000 on ~15 % of the keys (never key 0) and, with B > 1 and dead_sample, a last sample whose keys
    are all masked but key 0"""
    g = torch.Generator().manual_seed(seed)
    m = torch.where(torch.rand(B, N, generator=g) < 0.15, -10000.0, 0.0)
    m[:, 0] = 0.0
    if dead_sample and B > 1:
        m[-1, 1:] = -10000.0
    return m.cuda()


def _causal(Nq, Nk):
    """the decoder's additive causal mask: query i sees keys 0 .. i"""
    return torch.triu(torch.full((Nq, Nk), -10000.0), diagonal=1).cuda()


def _drop_mask(B, H, Nq, Nk):
    """keep / (1 - p) factors of the attention_probs dropout: element (b h Nq + i) Nk + j is the memory order of [B, H, Nq, Nk]"""
    from oracle import madtp_oracle as O
    p, seed, site = DROP
    return O.dropout_mask(seed, site, (B, H, Nq, Nk), p).cuda().double()


def _heads(t, B, N, H):
    """[B*N, H*64] row view -> [B, H, N, 64]"""
    return t.reshape(B, N, H, 64).transpose(1, 2)


def _probs64(q, k, B, H, Nq, Nk, km=None, mqk=None):
    """float64 P = softmax(scale q k^T + key_mask + mask_qk) [B, H, Nq, Nk] from [B, H, N, 64] operands"""
    s = (q @ k.transpose(-1, -2)) * SCALE
    if km is not None:
        s = s + km.double()[:, None, None, :]
    if mqk is not None:
        s = s + mqk.double()
    return s.softmax(-1)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. madtp_attention_train: P, out and the pruning score's side outputs
# ---------------------------------------------------------------------------------------------------------------------------------
TRAIN_SHAPES = [(2, 12, 577, 577), (1, 12, 901, 901), (1, 12, 1024, 1024), (3, 12, 17, 17), (2, 1, 5, 5), (4, 3, 16, 16),
                (2, 12, 20, 901), (1, 12, 1, 1024)]


@pytest.mark.parametrize("variant", ["plain", "masks", "drop", "all"])
@pytest.mark.parametrize("B,H,Nq,Nk", TRAIN_SHAPES, ids=[f"b{b}h{h}q{q}k{k}" for b, h, q, k in TRAIN_SHAPES])
def test_attention_train(hip, B, H, Nq, Nk, variant):
    """out = (P o dropout mask) V, P, and - self-attention - colsum_part[b, rt, j] = sum over rows i >= 1 of row tile rt of
    max_h P[b, h, i, j], p0 = P[:, :, 0, :], onorm = ||out_h|| of the dropped output; P is the bits of madtp_attention_probs_x."""
    from madtp_amd import backward as bw
    D = H * 64
    q, kv = _rand(B * Nq, D, seed=Nq).cuda(), _rand(B * Nk, 2 * D, seed=Nk + 1).cuda()
    k, v = kv[:, :D], kv[:, D:]
    masks = variant in ("masks", "all")
    km = _key_mask(B, Nk, seed=3) if masks else None
    mqk = _causal(Nq, Nk) if masks else None
    drop = DROP if variant in ("drop", "all") else (0.0, 0, 0)
    self_attn = Nq == Nk
    P = torch.empty(B * H * Nq * Nk, device="cuda")
    out, side = bw.attention_train(q, k, v, B, H, Nq, Nk, SCALE, drop, key_mask=km, mask_qk=mqk, scores=self_attn, P=P)
    P = P.view(B, H, Nq, Nk)
    P64 = _probs64(_heads(q.double(), B, Nq, H), _heads(k.double(), B, Nk, H), B, H, Nq, Nk, km, mqk)
    Pd = P64 * _drop_mask(B, H, Nq, Nk) if drop[0] > 0 else P64
    o64 = Pd @ _heads(v.double(), B, Nk, H)
    errs = {"P": _rel(P, P64), "out": _rel(out, o64.transpose(1, 2).reshape(B * Nq, D))}
    assert torch.equal(P, hip.attention_probs_x(q, k, B, H, Nq, Nk, SCALE, key_mask=km, mask_qk=mqk))
    if self_attn:
        cs, p0, on = side
        N, nrt = Nq, (Nq + 15) // 16
        hm = torch.zeros(B, nrt * 16, N, device="cuda", dtype=torch.float64)
        hm[:, 1:N] = P64[:, :, 1:].max(1)[0]
        errs.update(colsum_part=_rel(cs, hm.view(B, nrt, 16, N).sum(2)), p0=_rel(p0, P64[:, :, 0, :]), onorm=_rel(on, o64.norm(dim=-1)))
    else:  # the side outputs are self-attention's: refused when Nq != Nk
        with pytest.raises(RuntimeError, match=r"\(code -1\)"):
            bw.attention_train(q, k, v, B, H, Nq, Nk, SCALE, drop, key_mask=km, mask_qk=mqk, scores=True)
    _report(f"attention_train B{B} H{H} Nq{Nq} Nk{Nk} {variant}", errs, TOL_TRAIN)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. madtp_attention_bwd (self-attention) with every input switched on
# ---------------------------------------------------------------------------------------------------------------------------------
def _self_attn_grads(qkv, B, H, N, G, da, dp0, dn, hm, km=None, mqk=None, dmask=None):
    """float64 autograd of  sum(out G) + sum(da . colsum(headmax P)) + sum(dp0 . P[:, :, 0, :]) + sum(dn . ||out_h||)  - the columns
    j >= 1 and rows i >= 1 of the head-max mass and the columns j >= 1 of the CLS row, as the pruning score reads them - one term at
    a time: {term: (d qkv, d P)}, out [B*N, D] and P.  hm [B, N, N]: the head the max is taken from (the gradient of max_h goes to
    that head only)."""
    D = H * 64
    r = qkv.double().requires_grad_(True)
    q, k, v = (_heads(r[:, i * D:(i + 1) * D], B, N, H) for i in range(3))
    P = _probs64(q, k, B, H, N, N, km, mqk)
    o = (P * dmask if dmask is not None else P) @ v
    out = o.transpose(1, 2).reshape(B * N, D)
    terms = {"G": (out * G.double()).sum(), "dn": (dn.double() * o.norm(dim=-1)).sum()}
    if N > 1:
        terms["da"] = (da.double()[:, 1:] * P.gather(1, hm[:, None]).squeeze(1)[:, 1:, 1:].sum(1)).sum()
        terms["dp0"] = (dp0.double()[:, :, 1:] * P[:, :, 0, 1:]).sum()
    grads = {t: torch.autograd.grad(L, (r, P), retain_graph=True) for t, L in terms.items()}
    return grads, out.detach(), P.detach()


def _head_argmax(hip, qkv, B, H, N, km=None, mqk=None, rule="first"):
    """the head arg-max of the f32 probabilities the kernel recomputes (madtp_attention_probs_x: the same kernel, the same bits) - the
    first maximum as torch.max takes it, or the last"""
    D = H * 64
    P32 = hip.attention_probs_x(qkv[:, :D], qkv[:, D:2 * D], B, H, N, N, SCALE, key_mask=km, mask_qk=mqk)
    return P32.argmax(1) if rule == "first" else H - 1 - P32.flip(1).argmax(1)


def _run_self_bwd(hip, B, H, N, qkv, km=None, mqk=None, drop=None, seed=0):
    """kernel vs float64 autograd, the score terms scaled so that each moves d qkv by half as much as the out term; returns
    (errors, {term: its share of d qkv relative to the whole}, the reference's per-term grads, the reference's inputs)"""
    from madtp_amd import backward as bw
    D = H * 64
    G, da, dp0, dn = (_rand(*s, seed=seed + i).cuda() for i, s in enumerate([(B * N, D), (B, N), (B, H, N), (B, H, N)]))
    dmask = _drop_mask(B, H, N, N) if drop is not None else None
    hm = _head_argmax(hip, qkv, B, H, N, km, mqk)
    grads, out, P64 = _self_attn_grads(qkv, B, H, N, G, da, dp0, dn, hm, km, mqk, dmask)
    # where f32 rounding picks another head than float64 would, the two heads' probabilities are equal to rounding (max_h is
    # discontinuous there: the reference follows the kernel's decision, as the block tests follow its kept set)
    pm = P64.max(1)[0]
    assert bool(((pm - P64.gather(1, hm[:, None]).squeeze(1)) <= 1e-6 * pm).all()), "head arg-max differs beyond rounding"
    big = float(grads["G"][0].abs().max())
    c = {t: (0.5 * big / float(g[0].abs().max()) if float(g[0].abs().max()) > 0 else 1.0) for t, g in grads.items() if t != "G"}
    ref_qkv = grads["G"][0] + sum(c[t] * grads[t][0] for t in c)
    ref_dP = grads["G"][1] + sum(c[t] * grads[t][1] for t in c)
    share = {t: float((c[t] * grads[t][0]).abs().max()) / float(ref_qkv.abs().max()) for t in c}
    out32 = out.float().contiguous()
    onorm = _heads(out, B, N, H).norm(dim=-1)
    da_k = (da * c.get("da", 1.0)).contiguous()
    dp0_k = (dp0 * c.get("dp0", 1.0)).contiguous()
    # dnrm_scale = dn / ||out_h||, 0 where the norm is 0 (a row dropped whole): score_bwd_kernel's output
    dnrm_k = torch.where(onorm > 0, dn.double() * c["dn"] / onorm, 0.0).float().contiguous()

    def run():
        dp_out = torch.empty(B, H, N, N, device="cuda")
        dqkv = bw.attention_bwd(qkv, G, out32, B, H, N, SCALE, dnrm=dnrm_k, da=da_k, dp0=dp0_k, key_mask=km, mask_qk=mqk, dp_out=dp_out,
                                drop=drop)
        return dqkv, dp_out

    dqkv, dp_out = run()
    dqkv2, dp_out2 = run()
    assert torch.equal(dqkv, dqkv2) and torch.equal(dp_out, dp_out2)  # fixed summation orders
    errs = {"dq": _rel(dqkv[:, :D], ref_qkv[:, :D]), "dk": _rel(dqkv[:, D:2 * D], ref_qkv[:, D:2 * D]),
            "dv": _rel(dqkv[:, 2 * D:], ref_qkv[:, 2 * D:]), "dp_out": _rel(dp_out, ref_dP)}
    return errs, share, grads, dict(G=G, da=da, dp0=dp0, dn=dn, c=c, ref_qkv=ref_qkv)


BWD_N = [1, 15, 16, 17, 65, 197, 577, 901, 1024]


def _bwd_batch(N, H):
    return 1 if N * N * H > 4_000_000 else (2 if N >= 197 else 3)


@pytest.mark.parametrize("variant", ["terms", "key_mask", "mask_qk", "drop"])
@pytest.mark.parametrize("H", [1, 3, 12])
@pytest.mark.parametrize("N", BWD_N)
def test_attention_bwd_score_terms(hip, N, H, variant):
    """dq / dk / dv and dp_out (the gradient of P itself) of madtp_attention_bwd with dnrm_scale, da and dp0 all on, against float64
    autograd; every score term changes d qkv by >= 100x the tolerance (so a kernel that drops one cannot pass), except where it
    cannot reach the loss: da and dp0 at N = 1 (no key j >= 1), dp0 under the causal mask (the CLS row sees key 0 only)."""
    B = _bwd_batch(N, H)
    D = H * 64
    qkv = _rand(B * N, 3 * D, seed=N * 7 + H).cuda()
    km = _key_mask(B, N, seed=N) if variant == "key_mask" else None
    mqk = _causal(N, N) if variant == "mask_qk" else None
    drop = DROP if variant == "drop" else None
    errs, share, grads, _ = _run_self_bwd(hip, B, H, N, qkv, km, mqk, drop, seed=N + H)
    for t in ("da", "dp0", "dn"):
        if (N == 1 and t != "dn") or (t == "dp0" and mqk is not None):
            assert t not in grads or float(grads[t][0].abs().max()) == 0.0, t
        else:
            assert share[t] >= 100 * TOL_BWD, f"score term {t} moves d qkv by only {share[t]:.2e} of its maximum"
    _report(f"attention_bwd B{B} H{H} N{N} {variant}", errs, TOL_BWD)


@pytest.mark.parametrize("N", [197, 577])
def test_attention_bwd_head_ties(hip, N):
    """heads 0 and 2 see identical q / k, so their P are identical: the head arg-max of the da term (attn_headmax_kernel) takes the
    FIRST of tied heads, as torch.max does.  The last-max rule gives a d qkv >= 100x the tolerance away (asserted: the test tells the
    two rules apart)."""
    B, H = 2, 3
    D = H * 64
    qkv = _rand(B * N, 3 * D, seed=N).cuda()
    for base in (0, D):  # q, k of head 2 := those of head 0
        qkv[:, base + 128:base + 192] = qkv[:, base:base + 64]
    errs, share, grads, ins = _run_self_bwd(hip, B, H, N, qkv, seed=5)
    assert share["da"] >= 100 * TOL_BWD
    hm_last = _head_argmax(hip, qkv, B, H, N, rule="last")
    assert bool((hm_last != _head_argmax(hip, qkv, B, H, N)).any()), "no head ties"
    last, _, _ = _self_attn_grads(qkv, B, H, N, ins["G"], ins["da"], ins["dp0"], ins["dn"], hm_last)
    c = ins["c"]
    alt = last["G"][0] + sum(c[t] * last[t][0] for t in c)
    assert _rel(alt, ins["ref_qkv"]) >= 100 * TOL_BWD, "no head ties reached the da term"
    _report(f"attention_bwd head ties B{B} H{H} N{N}", errs, TOL_BWD)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. madtp_attention_bwd_cross
# ---------------------------------------------------------------------------------------------------------------------------------
CROSS_SHAPES = [(2, 35, 901), (1, 1, 1024), (3, 17, 577), (2, 16, 13)]


@pytest.mark.parametrize("variant", ["key_mask", "drop", "both"])
@pytest.mark.parametrize("B,Nq,Nk", CROSS_SHAPES)
def test_attention_bwd_cross(hip, B, Nq, Nk, variant):
    """cross-attention backward (Nq queries against Nk keys of a fused [k|v] projection) with a key mask and / or attention_probs
    dropout vs float64 autograd."""
    from madtp_amd import backward as bw
    H = 12
    D = H * 64
    q, kv, dout = _rand(B * Nq, D, seed=Nq).cuda(), _rand(B * Nk, 2 * D, seed=Nk).cuda(), _rand(B * Nq, D, seed=3).cuda()
    km = _key_mask(B, Nk, seed=Nk) if variant != "drop" else None
    drop = DROP if variant != "key_mask" else None
    qr, kvr = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    P = _probs64(_heads(qr, B, Nq, H), _heads(kvr[:, :D], B, Nk, H), B, H, Nq, Nk, km)
    if drop is not None:
        P = P * _drop_mask(B, H, Nq, Nk)
    o = (P @ _heads(kvr[:, D:], B, Nk, H)).transpose(1, 2).reshape(B * Nq, D)
    o.backward(dout.double())
    dq, dkv = bw.attention_bwd_cross(q, kv, dout, B, H, Nq, Nk, SCALE, key_mask=km, drop=drop)
    dq2, dkv2 = bw.attention_bwd_cross(q, kv, dout, B, H, Nq, Nk, SCALE, key_mask=km, drop=drop)
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)
    errs = {"dq": _rel(dq, qr.grad), "dk": _rel(dkv[:, :D], kvr.grad[:, :D]), "dv": _rel(dkv[:, D:], kvr.grad[:, D:])}
    _report(f"attention_bwd_cross B{B} Nq{Nq} Nk{Nk} {variant}", errs, TOL_CROSS)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. madtp_token_score_bwd + madtp_token_gather_bwd, fed by madtp_attention_train's side outputs
# ---------------------------------------------------------------------------------------------------------------------------------
# k: 1, a typical value and N - 3, the largest the pruning rule takes (vit.py:148: n - k >= 2 of the n = N - 1 patch tokens)
SCORE_CASES = [(B, N, k) for B, N in ((16, 197), (4, 577), (2, 901)) for k in (1, (N - 1) // 2, N - 3)]


@pytest.mark.parametrize("layout", ["dense", "strided_ties"])
@pytest.mark.parametrize("B,N,k", SCORE_CASES)
def test_token_score_and_gather_bwd(hip, monkeypatch, B, N, k, layout):
    """The pruning step's backward: token_gather_bwd (dx, dw = d merge weights) and token_score_bwd (da, dp0, dnrm_scale,
    dtoken_attn) against float64 autograd through oracle.importance_and_threshold + reduce_token (ViT variant) with self_attn = P,
    attn_out (-> cls_attn_score) and token_attn as leaves.  The score side comes from madtp_attention_train's side outputs;
    strided_ties: token_attn is a strided view (ldt_row != K, ldt_batch != n K) whose rows often hold their maximum twice - the
    gradient goes to the first one."""
    from madtp_amd import backward as bw
    from oracle import madtp_oracle as O
    H, K, dim, T = 12, 100, 768, 1.0
    D, n = H * 64, N - 1
    q, kv = _rand(B * N, D, seed=N).cuda(), _rand(B * N, 2 * D, seed=N + 1).cuda()
    P = torch.empty(B * H * N * N, device="cuda")
    out, side = bw.attention_train(q, kv[:, :D], kv[:, D:], B, H, N, N, SCALE, (0.0, 0, 0), scores=True, P=P)
    ta = _rand(B, n, K, seed=7).cuda()
    if layout == "strided_ties":
        g = torch.Generator().manual_seed(8)
        rows = torch.rand(B, n, generator=g) < 0.5
        c1 = torch.randint(0, K // 2, (B, n), generator=g)
        c2 = torch.randint(K // 2, K, (B, n), generator=g)
        top = ta.amax(-1).cpu() + 0.5
        for b, j in rows.nonzero().tolist():
            ta[b, j, c1[b, j]] = ta[b, j, c2[b, j]] = float(top[b, j])
        buf = torch.zeros(B, n + 3, K + 28, device="cuda")
        buf[:, :n, 5:5 + K] = ta
        ta = buf[:, :n, 5:5 + K]
        assert ta.stride(1) != K and ta.stride(0) != n * K
    score, _, _, _ = hip.token_score(side, ta, T, B, H, N)
    indices, _, dst_pos, merge_w = hip.token_select(score, k)
    x_attn, dy = _rand(B, N, dim, seed=9).cuda(), _rand(B, k + 2, dim, seed=10).cuda()
    dx, dw = bw.token_gather_bwd(dy, x_attn, dst_pos, merge_w, k)
    da, dp0, dnrm, dta = bw.token_score_bwd(dw, score, dst_pos, merge_w, side, ta, B, H, N)

    # the reference, with the kernels' k (count forced to k; reduce_token's own k is the batch-max count)
    real = O.importance_and_threshold

    def forced_k(*args):
        s, thr, count = real(*args)
        return s, thr, torch.full_like(count, k)

    monkeypatch.setattr(O, "importance_and_threshold", forced_k)
    P64 = P.view(B, H, N, N).double().requires_grad_(True)
    o64 = _heads(out.double(), B, N, H).detach().requires_grad_(True)
    ta64 = ta.double().requires_grad_(True)
    x64 = x_attn.double().requires_grad_(True)
    y, _, info = O.reduce_token(x64[:, 1:], T, P64, O.cls_attn_score(P64, o64), ta64, variant="vit", order="ascending")
    assert info["pruned"] and info["k"] == k and torch.equal(info["indices"], indices), "kept sets differ"
    (y * dy[:, 1:].double()).sum().backward()
    ref_dx = torch.cat([dy[:, :1].double(), x64.grad[:, 1:]], 1)
    dropped = dst_pos < 0
    ref_dw = torch.where(dropped, (dy[:, k + 1:k + 2].double() * x64[:, 1:].detach()).sum(-1), 0.0)
    errs = {"dx": _rel(dx, ref_dx), "dw": _rel(dw, ref_dw),
            # d P at rows i >= 1, columns j >= 1 is da[j] on the head-max head of (i, j), zero elsewhere
            "da": _rel(da[:, None, 1:].expand(B, n, n), P64.grad[:, :, 1:, 1:].sum(1)), "da0": float(da[:, 0].abs().max()),
            "dp0": _rel(dp0, P64.grad[:, :, 0, :]), "dnrm_scale": _rel(dnrm[..., None] * o64.detach(), o64.grad),
            "dtoken_attn": _rel(dta, ta64.grad)}
    assert int((dta != 0).sum(-1).max()) <= 1
    _report(f"token_score/gather_bwd B{B} N{N} k{k} {layout}", errs, TOL_SCORE)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. madtp_layernorm_bwd and the output_attentions maps
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("rows,dim,eps", [(1, 768, 1e-6), (77, 512, 1e-5), (3000, 768, 1e-12)])
def test_layernorm_bwd(hip, rows, dim, eps, with_add):
    from madtp_amd import backward as bw
    x = (_rand(rows, dim, seed=1) * 2 + 0.5).cuda()
    dy, add = _rand(rows, dim, seed=2).cuda(), _rand(rows, dim, seed=3).cuda() if with_add else None
    gamma, beta = (1 + 0.1 * _rand(dim, seed=4)).cuda(), _rand(dim, seed=5).cuda()
    xr, gr, br = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    F.layer_norm(xr, (dim,), gr, br, eps).backward(dy.double())
    dx, dgamma, dbeta = bw.layernorm_bwd(x, gamma, dy, eps, add=add)
    ref_dx = xr.grad + add.double() if with_add else xr.grad
    _report(f"layernorm_bwd {rows}x{dim} eps {eps} add={with_add}", {"dx": _rel(dx, ref_dx), "dgamma": _rel(dgamma, gr.grad),
                                                                     "dbeta": _rel(dbeta, br.grad)}, TOL_LN)


PROBS_CASES = [(1, 12, 1024, 1024, "self"), (2, 3, 577, 577, "self"), (3, 1, 17, 17, "self"), (2, 12, 35, 901, "x"),
               (1, 12, 1024, 1024, "x"), (2, 3, 1, 17, "x"), (1, 12, 20, 1024, "x")]


@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("B,H,Nq,Nk,entry", PROBS_CASES)
def test_attention_probs_maps(hip, B, H, Nq, Nk, entry, masks):
    """the output_attentions maps: madtp_attention_probs (self, key mask) and madtp_attention_probs_x (Nq != Nk, key mask + causal
    mask_qk) vs float64."""
    D = H * 64
    q, k = _rand(B * Nq, D, seed=Nq).cuda(), _rand(B * Nk, D, seed=Nk + 2).cuda()
    km = _key_mask(B, Nk, seed=Nk) if masks else None
    if entry == "self":
        P = hip.attention_probs(q, k, B, H, Nq, SCALE, key_mask=km)
        mqk = None
    else:
        mqk = _causal(Nq, Nk) if masks else None
        P = hip.attention_probs_x(q, k, B, H, Nq, Nk, SCALE, key_mask=km, mask_qk=mqk)
    P64 = _probs64(_heads(q.double(), B, Nq, H), _heads(k.double(), B, Nk, H), B, H, Nq, Nk, km, mqk)
    _report(f"attention_probs{'' if entry == 'self' else '_x'} B{B} H{H} Nq{Nq} Nk{Nk} masks={masks}", {"P": _rel(P, P64)}, TOL_PROBS)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. vit.Block forward + backward at the real token counts
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [384, 480])
def test_block_backward_at_training_token_counts(hip, size):
    """vit.Block (fp32 mode) at 384^2 (577 tokens) and 480^2 (901 tokens), B = 2, synthetic weights: the same kept sets as the CPU
    oracle, then every gradient within 1e-3 of autograd through oracle.vit_block_grads, every entry."""
    from madtp_amd import runtime, specs, synth, vit
    from oracle import madtp_oracle as O
    from tests import grad_case
    B, T, seed, prefix = 2, 5.0, 0, "blocks.0."
    W = specs.synth_weights(specs.vit_shapes("", size, depth=1), seed)
    images = synth.synth_images(B, size, seed)
    with torch.no_grad():
        x = O.patch_embed(W, "", images)
        token_attn, _ = O.query_model(x[:, 1:, :], synth.synth_tensor("space_dict", (100, 768), seed))
    token_attn = token_attn.contiguous()
    assert x.shape[1] == (size // 16) ** 2 + 1
    with torch.no_grad():
        y_ref, info_ref = O.vit_block(W, prefix, x, T, token_attn)
    assert info_ref["pruned"], "the synthetic case must prune"
    G = torch.from_numpy(synth.uniform_pm1("grad_out", y_ref.numel(), seed).reshape(tuple(y_ref.shape)))
    ref, _, oinfo = O.vit_block_grads(W, prefix, x, token_attn, T, G)
    blk = vit.Block(768, 12, qkv_bias=True, norm_layer=lambda d: torch.nn.LayerNorm(d, eps=1e-6))
    blk.load_state_dict({k[len(prefix):]: v for k, v in W.items() if k.startswith(prefix)}, strict=True)
    blk = blk.cuda()
    xg = x.cuda().requires_grad_(True)
    tg = token_attn.cuda().requires_grad_(True)
    with runtime.precision("fp32"):
        y = blk(xg, False, 0, T, tg)
        assert tuple(y.shape) == tuple(y_ref.shape)
        own = blk.last_prune["indices"].cpu().numpy()
        for b in range(B):
            assert {int(v) for v in own[b]} == {int(v) for v in oinfo["indices"][b]}, "kept set differs from the oracle"
        (y * grad_case.permute_G(G, oinfo["indices"].numpy(), own).cuda()).sum().backward()
    grads = {"x": xg.grad, "token_attn": tg.grad}
    grads.update({k: p.grad for k, p in blk.named_parameters()})
    errs = {name: _rel(grads[name].cpu(), r) for name, r in ref.items()}
    _report(f"vit.Block {size}^2 B{B} k{oinfo['k']}", errs, 1e-3)  # measured on MI355X: 2.1e-6 (x), 4.5e-6 (weights) at 480^2

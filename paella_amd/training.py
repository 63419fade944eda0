"""Training-mode forward of `Paella`: a differentiable evaluation built from torch ops over the module's own parameters.

SURVEY 8(f) rank 3: the reference's training loops (src/train.py:59-66, src_distributed/train.py:104-114) call
`model.train(); pred = model(noised, t, byt5...); loss.backward()`.  The HIP engine behind `Paella.forward` is an inference
engine (no saved activations; its only backward kernels are the loss head's and the MLP activation's, below), so in TRAIN mode -- `model.train()`, exactly the switch the reference's
loops flip -- `forward` routes here instead: the same network written as autograd-tracked torch ops (dropout active, as in the
reference).  `model.eval()` (the state a `paella_amd.Paella` is constructed in, and what the sampling path requires) never
reaches this file: sampling always runs the hand-written HIP kernels and fails loudly without them.

The arithmetic follows the reference's module definitions (file:line cited per function); it is written functionally over
the state-dict names so that the parameters of the SAME module are trained and the HIP engine picks the updated values up
on the next eval-mode call (`Paella._signature` tracks in-place optimizer updates).
"""
import math

import torch
import torch.nn.functional as F


def _ln_nchw(x, eps=1e-6):
    """LayerNorm2d without affine (src/modules.py:22-27): normalise over channels of an NCHW tensor."""
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.size(1),), None, None, eps).permute(0, 3, 1, 2)


def _channelwise(blk, x_nhwc, p_drop, training, hip_act=False):
    """Linear -> GELU -> GlobalResponseNorm -> Dropout -> Linear (src/modules.py:49-53 / 30-40).  hip_act (Paella.set_training_activation("hip"), train mode on a cuda
    device): the three middle stages run as one HIP op in both directions (`gelu_grn_dropout` below)."""
    cw = blk.channelwise._modules
    if hip_act:
        h = gelu_grn_dropout(F.linear(x_nhwc, cw["0"].weight, cw["0"].bias), cw["2"].gamma, cw["2"].beta, p_drop)
        return F.linear(h, cw["4"].weight, cw["4"].bias)
    h = F.gelu(F.linear(x_nhwc, cw["0"].weight, cw["0"].bias))
    gx = torch.norm(h, p=2, dim=(1, 2), keepdim=True)
    nx = gx / (gx.mean(dim=-1, keepdim=True) + 1e-6)
    h = cw["2"].gamma * (h * nx) + cw["2"].beta + h
    h = F.dropout(h, p_drop, training)
    return F.linear(h, cw["4"].weight, cw["4"].bias)


def _res_block(blk, x, skip, p_drop, training, hip_act=False, hip_dw=False):
    """ResBlock (src/modules.py:43-62): depthwise 3x3 (groups = c, over cat([x, skip]) when a skip arrives) -> LN -> MLP -> + x.  hip_dw
    (Paella.set_training_depthwise("hip"), train mode on a cuda device): everything in front of the MLP runs as one HIP op in both directions
    (`dwconv_layernorm` below), x and skip handed over separately -- no torch.cat."""
    res = x
    if hip_dw:
        y = dwconv_layernorm(x, blk.depthwise.weight, blk.depthwise.bias, skip)
        return _channelwise(blk, y, p_drop, training, hip_act).permute(0, 3, 1, 2) + res
    if skip is not None:
        x = torch.cat([x, skip], dim=1)
    dw = blk.depthwise
    c = dw.weight.size(0)
    x = _ln_nchw(F.conv2d(x, dw.weight, dw.bias, padding=dw.weight.size(-1) // 2, groups=c)).permute(0, 2, 3, 1)
    return _channelwise(blk, x, p_drop, training, hip_act).permute(0, 3, 1, 2) + res


def _ff_block(blk, x, p_drop, training, hip_act=False):
    """FeedForwardBlock (src/modules.py:82-96)."""
    return x + _channelwise(blk, _ln_nchw(x).permute(0, 2, 3, 1), p_drop, training, hip_act).permute(0, 3, 1, 2)


def _timestep_block(blk, x, r_embed):
    """TimestepBlock (src/modules.py:99-106)."""
    a, b = F.linear(r_embed, blk.mapper.weight, blk.mapper.bias)[:, :, None, None].chunk(2, dim=1)
    return x * (1 + a) + b


def _attn_block(blk, x, c_embed, nhead, self_attn, p_drop, training, attn_weights=None):
    """AttnBlock (src/modules.py:65-79) around nn.MultiheadAttention semantics (Attention2D :7-19): queries = LN(x) positions,
    keys = values = [LN(x) positions | kv_mapper(SiLU(c_embed))], residual on the un-normed x."""
    kvm = blk.kv_mapper._modules["1"]
    kv = F.linear(F.silu(c_embed), kvm.weight, kvm.bias)
    B, C, H, W = x.shape
    q = _ln_nchw(x).reshape(B, C, H * W).permute(0, 2, 1)
    if self_attn:
        kv = torch.cat([q, kv], dim=1)
    at = blk.attention.attn
    if attn_weights is None:
        # torch's own functional form of nn.MultiheadAttention.forward (batch_first handled by the transposes): identical
        # arithmetic and identical dropout-stream consumption to the module the reference instantiates
        out, _ = F.multi_head_attention_forward(q.transpose(0, 1), kv.transpose(0, 1), kv.transpose(0, 1), C, nhead, at.in_proj_weight, at.in_proj_bias,
                                                None, None, False, p_drop, at.out_proj.weight, at.out_proj.bias, training=training,
                                                need_weights=False)
        out = out.transpose(0, 1)
    else:  # utils/alter_attention.py:4-43: post-softmax multiply of the last n key columns
        d = C // nhead
        wq, wk, wv = at.in_proj_weight.chunk(3)
        bq, bk, bv = at.in_proj_bias.chunk(3)
        qh = F.linear(q, wq, bq).view(B, -1, nhead, d).transpose(1, 2)
        kh = F.linear(kv, wk, bk).view(B, -1, nhead, d).transpose(1, 2)
        vh = F.linear(kv, wv, bv).view(B, -1, nhead, d).transpose(1, 2)
        w = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(d), dim=-1)
        n = attn_weights.numel()
        w = torch.cat([w[..., :-n], w[..., -n:] * attn_weights], dim=-1)
        w = F.dropout(w, p_drop, training)
        out = F.linear((w @ vh).transpose(1, 2).reshape(B, -1, C), at.out_proj.weight, at.out_proj.bias)
    return x + out.permute(0, 2, 1).reshape(B, C, H, W)


def r_embedding(r, c_r, max_positions=10000):
    """gen_r_embedding (src/modules.py:212-221)."""
    r = r * max_positions
    half = c_r // 2
    freqs = torch.arange(half, device=r.device).float().mul(-math.log(max_positions) / (half - 1)).exp()
    emb = r[:, None] * freqs[None, :]
    emb = torch.cat([emb.sin(), emb.cos()], dim=1)
    return F.pad(emb, (0, 1)) if c_r % 2 == 1 else emb


def c_embeddings(model, byt5, clip, clip_image):
    """gen_c_embeddings (src/modules.py:223-232; list-valued clip_image as utils/modules.py:229-235)."""
    c_cond = model.c_cond
    seq = F.linear(byt5, model.byt5_mapper.weight, model.byt5_mapper.bias)
    if clip is not None:
        seq = torch.cat([seq, F.linear(clip, model.clip_mapper.weight, model.clip_mapper.bias).view(clip.size(0), -1, c_cond)], dim=1)
    if clip_image is not None:
        for ci in (clip_image if isinstance(clip_image, (list, tuple)) else [clip_image]):
            seq = torch.cat([seq, F.linear(ci, model.clip_image_mapper.weight, model.clip_image_mapper.bias).view(ci.size(0), -1, c_cond)], dim=1)
    return F.layer_norm(seq, (c_cond,), None, None, 1e-6)


def _forward_features(model, x, r, byt5, clip=None, clip_image=None, x_cat=None, attn_weights=None):
    """Paella.forward (src/modules.py:263-275) as autograd-tracked torch ops, up to and including the LayerNorm2d in front of out_mapper's convolution:
    [B, c_out, H, W] as the permuted view of an NHWC tensor that `_ln_nchw` returns."""
    cfg = model._cfg
    training = model.training
    p_drop = float(model.dropout) if not isinstance(model.dropout, (list, tuple)) else None
    drop = (lambda lvl: p_drop) if p_drop is not None else (lambda lvl: float(model.dropout[lvl]))
    if x_cat is not None:
        x = torch.cat([x, x_cat], dim=1)
    r_embed = r_embedding(r.float(), cfg["c_r"])
    c_embed = c_embeddings(model, byt5, clip, clip_image)
    patch = cfg["patch_size"]
    n_levels = len(cfg["c_hidden"])

    h = F.layer_norm(F.embedding(x, model.in_mapper._modules["0"].weight), (cfg["c_in"],), None, None, 1e-6).permute(0, 3, 1, 2)
    emb = model.embedding._modules["1"]
    h = _ln_nchw(F.conv2d(F.pixel_unshuffle(h, patch), emb.weight, emb.bias))

    # Paella.set_training_activation: the switch acts in train mode on a cuda device only; its default leaves every call below as it is
    hip_act = training and getattr(model, "_train_activation", "torch") == "hip" and x.is_cuda
    # Paella.set_training_depthwise: likewise.  Under it the trunk is made channels_last once, here, so that the blocks hand each other NHWC memory
    hip_dw = training and getattr(model, "_train_depthwise", "torch") == "hip" and x.is_cuda
    if hip_dw:
        h = h.contiguous(memory_format=torch.channels_last)

    def run(blk, level, h, skip=None):
        if blk.kind == 'C':
            return _res_block(blk, h, skip, drop(level), training, hip_act, hip_dw)
        if blk.kind == 'A':
            return _attn_block(blk, h, c_embed, cfg["nhead"][level], cfg["self_attn"], drop(level), training, attn_weights)
        if blk.kind == 'T':
            return _timestep_block(blk, h, r_embed)
        if blk.kind == 'F':
            return _ff_block(blk, h, drop(level), training, hip_act)
        if blk.kind == 'D':  # LayerNorm2d + Conv2d(k2, s2)   (src/modules.py:153-156)
            cv = blk._modules["1"]
            return F.conv2d(_ln_nchw(h), cv.weight, cv.bias, stride=2)
        if blk.kind == 'U':  # LayerNorm2d + ConvTranspose2d(k2, s2)   (src/modules.py:172-175)
            cv = blk._modules["1"]
            return F.conv_transpose2d(_ln_nchw(h), cv.weight, cv.bias, stride=2)
        raise RuntimeError("unknown block kind %r" % blk.kind)

    level_outputs = []
    for i, level in enumerate(model.down_blocks):          # _down_encode (src/modules.py:234-247)
        for blk in level:
            h = run(blk, i, h)
        level_outputs.insert(0, h)
    h = level_outputs[0]
    for u, level in enumerate(model.up_blocks):            # _up_decode (src/modules.py:249-261)
        i = n_levels - 1 - u
        for j, blk in enumerate(level):
            h = run(blk, i, h, level_outputs[u] if (j == 0 and u > 0 and blk.kind == 'C') else None)
    clf = model.clf._modules["1"]
    h = F.pixel_shuffle(F.conv2d(_ln_nchw(h), clf.weight, clf.bias), patch)
    return _ln_nchw(h)


def forward_autograd(model, x, r, byt5, clip=None, clip_image=None, x_cat=None, attn_weights=None):
    """Paella.forward (src/modules.py:263-275) as autograd-tracked torch ops.  Returns logits [B, num_labels, H, W]."""
    return F.conv2d(_forward_features(model, x, r, byt5, clip, clip_image, x_cat, attn_weights), model.out_mapper._modules["1"].weight)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Training loss head: out_mapper's convolution + label-smoothed cross-entropy as ONE HIP op, forward and backward (paella_amd/csrc/loss.hip,
# include/paella_hip.h "Training loss head").  The [rows, num_labels] logits, their log-softmax and their gradient are never stored: the forward keeps
# five numbers per row, the backward recomputes the logit tiles from h, the weight and the saved lse.
# ---------------------------------------------------------------------------------------------------------------------------------------------------
HEAD_MAX_K, HEAD_MAX_LABELS, HEAD_MAX_ROWS = 256, 65536, 1 << 24


class _HeadCrossEntropy(torch.autograd.Function):
    """(h [rows, K], weight [N, K], target [rows]) -> (loss fp32 [rows], argmax int32 [rows]); saves h, weight, target and lse [rows]."""

    @staticmethod
    def forward(ctx, h, weight, target, eps):
        from . import _lib
        lib = _lib.load()
        rows, K = h.shape
        N = weight.size(0)
        dev = h.device
        loss = torch.empty(rows, dtype=torch.float32, device=dev)
        lse = torch.empty(rows, dtype=torch.float32, device=dev)
        argmax = torch.empty(rows, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            ws = _lib.new_workspace(lib.paella_head_loss_workspace_bytes(rows, N, K), dev)
            _lib.check(lib.paella_head_loss_forward(_lib.ptr(h), _lib.ptr(weight), _lib.ptr(target), rows, N, K, eps, _lib.ptr(loss), _lib.ptr(lse), _lib.ptr(argmax),
                                                    _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        ctx.save_for_backward(h, weight, target, lse)
        ctx.eps = eps
        ctx.mark_non_differentiable(argmax)
        return loss, argmax

    @staticmethod
    def backward(ctx, grad_loss, _grad_argmax):
        from . import _lib
        lib = _lib.load()
        h, weight, target, lse = ctx.saved_tensors
        rows, K = h.shape
        N = weight.size(0)
        dev = h.device
        g = grad_loss.to(torch.float32).contiguous()
        dh = torch.empty_like(h) if ctx.needs_input_grad[0] else None  # a NULL output = that kernel is not launched
        dw = torch.empty_like(weight) if ctx.needs_input_grad[1] else None
        if dh is not None or dw is not None:
            with torch.cuda.device(dev):
                ws = _lib.new_workspace(lib.paella_head_loss_workspace_bytes(rows, N, K), dev)
                _lib.check(lib.paella_head_loss_backward(_lib.ptr(h), _lib.ptr(weight), _lib.ptr(target), _lib.ptr(lse), _lib.ptr(g), rows, N, K, ctx.eps,
                                                         _lib.ptr(dh), _lib.ptr(dw), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        return dh, dw, None, None


def head_cross_entropy(h, weight, target, label_smoothing=0.0):
    """Classifier head + cross-entropy without a logits tensor: with l = h @ weight^T,
        loss   = nn.CrossEntropyLoss(label_smoothing=label_smoothing, reduction='none')(l, target)     (fp32, the shape of `target`; differentiable in h and weight)
        argmax = l.argmax(-1), the lowest label on ties                                                  (int32, not differentiable)
    h fp32 [..., K]; weight fp32 [N, K] or [N, K, 1, 1] (out_mapper.1.weight); target int64 with the leading shape of h.  A target outside [0, N) marks an
    ignored position (loss 0, no gradient), as ignore_index does.  K a multiple of 16 up to 256, N a multiple of 16 up to 65536, at most 2^24 positions.
    HIP only and exact fp32 only: anything else raises ValueError -- there is no torch fallback."""
    if not (torch.is_tensor(h) and torch.is_tensor(weight) and torch.is_tensor(target)):
        raise ValueError("head_cross_entropy takes tensors")
    if not h.is_cuda or weight.device != h.device or target.device != h.device:
        raise ValueError("head_cross_entropy runs on the HIP device only: h, weight and target must live on the same cuda device (got %s, %s, %s)"
                         % (h.device, weight.device, target.device))
    if h.dtype != torch.float32 or weight.dtype != torch.float32 or target.dtype != torch.int64:
        raise ValueError("head_cross_entropy takes fp32 h and weight and int64 target (got %s, %s, %s)" % (h.dtype, weight.dtype, target.dtype))
    if weight.dim() == 4 and weight.size(2) == 1 and weight.size(3) == 1:
        weight = weight.reshape(weight.size(0), weight.size(1))
    if weight.dim() != 2 or h.dim() < 1 or h.size(-1) != weight.size(1):
        raise ValueError("weight must be [N, K] or [N, K, 1, 1] with K = h.size(-1) (got h %s, weight %s)" % (tuple(h.shape), tuple(weight.shape)))
    N, K = weight.shape
    lead = h.shape[:-1]
    if tuple(target.shape) != tuple(lead):
        raise ValueError("target must have the leading shape of h, %s (got %s)" % (tuple(lead), tuple(target.shape)))
    rows = target.numel()
    if K % 16 or not 16 <= K <= HEAD_MAX_K:
        raise ValueError("K = %d: the fused head takes a multiple of 16 in 16...%d" % (K, HEAD_MAX_K))
    if N % 16 or not 16 <= N <= HEAD_MAX_LABELS:
        raise ValueError("N = %d labels: the fused head takes a multiple of 16 in 16...%d" % (N, HEAD_MAX_LABELS))
    if not 1 <= rows <= HEAD_MAX_ROWS:
        raise ValueError("%d positions: the fused head takes 1...%d" % (rows, HEAD_MAX_ROWS))
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:  # (false for NaN)
        raise ValueError("label_smoothing = %r: must lie in [0, 1)" % (label_smoothing,))
    # rows must be contiguous; the NHWC view behind `_ln_nchw`'s result already is (no copy)
    h2 = h.view(rows, K) if h.is_contiguous() else h.contiguous().view(rows, K)
    loss, argmax = _HeadCrossEntropy.apply(h2, weight.contiguous(), target.contiguous().view(rows), eps)
    return loss.view(lead), argmax.view(lead)


def forward_loss(model, x, r, target, byt5, clip=None, clip_image=None, x_cat=None, attn_weights=None, label_smoothing=0.1):
    """One training forward with the loss head fused: (loss [B, H, W], correct [B, H, W] bool) instead of logits [B, num_labels, H, W]."""
    feat = _forward_features(model, x, r, byt5, clip, clip_image, x_cat, attn_weights)
    loss, argmax = head_cross_entropy(feat.permute(0, 2, 3, 1), model.out_mapper._modules["1"].weight, target, label_smoothing)
    return loss, argmax == target


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Training MLP activation: GELU -> GlobalResponseNorm -> Dropout of `_channelwise` as ONE HIP op, forward and backward (paella_amd/csrc/grn_act.hip,
# include/paella_hip.h "Training MLP activation").  Of the widest activation of the network, [B, H, W, 4c], autograd keeps the pre-activation only (plus
# G [B, 4c]): the GELU output, h * nx, the dropout mask and the dropout input are recomputed, the mask from a (seed, element index) counter.
# ---------------------------------------------------------------------------------------------------------------------------------------------------
ACT_MAX_B, ACT_MAX_P, ACT_MAX_C = 65535, 1 << 20, 16384


class _GeluGrnDropout(torch.autograd.Function):
    """(u [B, P, C], gamma [C], beta [C]) -> z [B, P, C]; saves u, gamma and gx [B, C]."""

    @staticmethod
    def forward(ctx, u, gamma, beta, p, seed):
        from . import _lib
        lib = _lib.load()
        B, P, C = u.shape
        dev = u.device
        z = torch.empty_like(u)
        gx = torch.empty(B, C, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ws = torch.empty(lib.paella_grn_act_workspace_bytes(B, P, C), dtype=torch.uint8, device=dev)  # no state, no initialisation
            _lib.check(lib.paella_grn_act_forward(_lib.ptr(u), _lib.ptr(gamma), _lib.ptr(beta), B, P, C, p, seed, _lib.ptr(z), _lib.ptr(gx), _lib.ptr(ws), ws.numel(),
                                                  _lib.stream_ptr(dev)))
        ctx.save_for_backward(u, gamma, gx)
        ctx.p, ctx.seed = p, seed
        return z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dz):
        from . import _lib
        lib = _lib.load()
        u, gamma, gx = ctx.saved_tensors
        B, P, C = u.shape
        dev = u.device
        dz = _aligned(dz.to(torch.float32).contiguous())
        du = torch.empty_like(u) if ctx.needs_input_grad[0] else None  # a NULL output is not computed
        dgamma = torch.empty_like(gamma) if ctx.needs_input_grad[1] else None
        dbeta = torch.empty_like(gamma) if ctx.needs_input_grad[2] else None
        if du is not None or dgamma is not None or dbeta is not None:
            with torch.cuda.device(dev):
                ws = torch.empty(lib.paella_grn_act_workspace_bytes(B, P, C), dtype=torch.uint8, device=dev)
                _lib.check(lib.paella_grn_act_backward(_lib.ptr(u), _lib.ptr(gamma), _lib.ptr(gx), _lib.ptr(dz), B, P, C, ctx.p, ctx.seed, _lib.ptr(du), _lib.ptr(dgamma),
                                                       _lib.ptr(dbeta), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        return du, dgamma, dbeta, None, None


def _aligned(t):
    """the kernels move 16-byte vectors: a contiguous view that starts off that grain is copied"""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def gelu_grn_dropout(u, gamma, beta, p=0.0, seed=None):
    """The middle of a ResBlock / FeedForwardBlock MLP in train mode as one op: with h = gelu(u),
        z = dropout(gamma * (h * nx) + beta + h, p),   nx = Gx / (mean_c Gx + 1e-6),   Gx = ||h||_2 over the positions of a sample
    (src/modules.py:30-40, 49-53).  u fp32 [B, ..., C] (the dimensions between the first and the last are the positions of a sample); gamma, beta fp32 with C
    elements (the module's [1, 1, 1, C] parameters as they are).  Once differentiable in u, gamma and beta; autograd keeps u, gamma and Gx [B, C] only.  p in
    [0, 1); p = 0 draws nothing.  The dropout mask is a function of (seed, element index): seed = None with p > 0 draws one 64-bit seed from torch's default CPU
    generator, so torch.manual_seed reproduces a run.  C a multiple of 4 up to 16384, at most 2^20 positions per sample, B up to 65535.  HIP only and exact fp32
    only: anything else raises ValueError -- there is no torch fallback."""
    if not (torch.is_tensor(u) and torch.is_tensor(gamma) and torch.is_tensor(beta)):
        raise ValueError("gelu_grn_dropout takes tensors")
    if u.dtype != torch.float32 or gamma.dtype != torch.float32 or beta.dtype != torch.float32:
        raise ValueError("gelu_grn_dropout takes fp32 u, gamma and beta (got %s, %s, %s)" % (u.dtype, gamma.dtype, beta.dtype))
    if u.dim() < 2:
        raise ValueError("u must be [B, ..., C] (got %s)" % (tuple(u.shape),))
    B, C = u.size(0), u.size(-1)
    if gamma.numel() != C or beta.numel() != C:
        raise ValueError("gamma and beta must have C = u.size(-1) = %d elements (got %s, %s)" % (C, tuple(gamma.shape), tuple(beta.shape)))
    if C % 4 or not 4 <= C <= ACT_MAX_C:
        raise ValueError("C = %d: the fused activation takes a multiple of 4 in 4...%d" % (C, ACT_MAX_C))
    P = u.numel() // (B * C) if B else 0
    if not 1 <= B <= ACT_MAX_B or not 1 <= P <= ACT_MAX_P:
        raise ValueError("u %s: the fused activation takes 1...%d samples of 1...%d positions" % (tuple(u.shape), ACT_MAX_B, ACT_MAX_P))
    p = float(p)
    if not 0.0 <= p < 1.0:  # (false for NaN)
        raise ValueError("p = %r: must lie in [0, 1)" % (p,))
    if not u.is_cuda or gamma.device != u.device or beta.device != u.device:
        raise ValueError("gelu_grn_dropout runs on the HIP device only: u, gamma and beta must live on the same cuda device (got %s, %s, %s)"
                         % (u.device, gamma.device, beta.device))
    if p == 0.0:
        seed = 0
    elif seed is None:
        seed = int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    z = _GeluGrnDropout.apply(_aligned(u.contiguous()).view(B, P, C), _aligned(gamma.contiguous().view(C)), _aligned(beta.contiguous().view(C)), p, seed)
    return z.view(u.shape)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Training ResBlock front: [cat with the skip ->] depthwise 3x3 -> LayerNorm2d -> NHWC as ONE HIP op, forward and backward (paella_amd/csrc/dwconv_train.hip,
# include/paella_hip.h "Training ResBlock front").  x and skip are read in place (no concatenation), the weight is used and its gradient returned in the
# parameter's layout, and besides the op's inputs and its output autograd keeps one float per position (rstd): the concatenated input, the convolution output and
# the LayerNorm's contiguous copy of the torch chain never exist.
# ---------------------------------------------------------------------------------------------------------------------------------------------------
DW_MAX_C, DW_MAX_C_SKIP, DW_MAX_POSITIONS = 8192, 4096, 2 ** 31 - 1
# diagnostic: how often `dwconv_layernorm` ran and how many of its x / skip arguments were not dense NHWC memory and had to be copied (tools/bench_train_dwconv.py)
DW_COUNTERS = {"calls": 0, "copied": 0}


class _DwconvLayerNorm(torch.autograd.Function):
    """(x [B, H, W, C], skip [B, H, W, C] or None, weight [C, J, 3, 3], bias [C]) -> y [B, H, W, C]; saves x, skip, weight, y and rstd [B, H, W]."""

    @staticmethod
    def forward(ctx, x, skip, weight, bias, eps):
        from . import _lib
        lib = _lib.load()
        B, H, W, C = x.shape
        dev = x.device
        y = torch.empty_like(x)
        rstd = torch.empty(B, H, W, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            # the forward asks for the repacked weights only, which is what the sizing call returns for one position
            ws = torch.empty(lib.paella_dwconv_ln_train_workspace_bytes(1, 1, 1, C, int(skip is not None)), dtype=torch.uint8, device=dev)
            _lib.check(lib.paella_dwconv_ln_train_forward(_lib.ptr(x), _lib.ptr(skip), _lib.ptr(weight), _lib.ptr(bias), B, H, W, C, eps, _lib.ptr(y), _lib.ptr(rstd),
                                                          _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        ctx.save_for_backward(x, skip, weight, y, rstd)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        from . import _lib
        lib = _lib.load()
        x, skip, weight, y, rstd = ctx.saved_tensors
        B, H, W, C = x.shape
        dev = x.device
        dy = _aligned(dy.to(torch.float32).contiguous())
        need = ctx.needs_input_grad
        dx = torch.empty_like(x) if need[0] else None  # a NULL output is not computed
        dskip = torch.empty_like(skip) if skip is not None and need[1] else None
        dw = torch.empty_like(weight) if need[2] else None
        dbias = torch.empty(C, dtype=torch.float32, device=dev) if need[3] else None
        if dx is not None or dskip is not None or dw is not None or dbias is not None:
            with torch.cuda.device(dev):
                ws = torch.empty(lib.paella_dwconv_ln_train_workspace_bytes(B, H, W, C, int(skip is not None)), dtype=torch.uint8, device=dev)
                _lib.check(lib.paella_dwconv_ln_train_backward(_lib.ptr(x), _lib.ptr(skip), _lib.ptr(weight), _lib.ptr(y), _lib.ptr(rstd), _lib.ptr(dy), B, H, W, C,
                                                               _lib.ptr(dx), _lib.ptr(dskip), _lib.ptr(dw), _lib.ptr(dbias), _lib.ptr(ws), ws.numel(),
                                                               _lib.stream_ptr(dev)))
        return dx, dskip, dw, dbias, None


def _nhwc(t):
    """[B, C, H, W] of any strides -> its [B, H, W, C] view when the memory is already dense NHWC and 16-byte aligned, else one copy"""
    v = t.permute(0, 2, 3, 1)
    if v.is_contiguous() and v.data_ptr() % 16 == 0:
        return v
    DW_COUNTERS["copied"] += 1
    return v.contiguous() if not v.is_contiguous() else v.clone()


def dwconv_layernorm(x, weight, bias, skip=None, eps=1e-6):
    """The front of a ResBlock in train mode as one op (src/modules.py:46-47, 55-58):
        y = layer_norm(conv2d(cat([x, skip], 1) if skip is not None else x, weight, bias, padding=1, groups=C).permute(0, 2, 3, 1), (C,), eps=eps)
    x and skip fp32 with logical shape [B, C, H, W] and any strides: memory that is already dense NHWC (`x.permute(0, 2, 3, 1).is_contiguous()`) is used in place,
    anything else is copied once.  weight fp32 [C, 1, 3, 3], or [C, 2, 3, 3] with a skip, and bias fp32 [C]: the module's parameters as they are.  Returns y
    [B, H, W, C], contiguous -- what `_channelwise` consumes.  Once differentiable in x, skip, weight and bias; the gradients of x and skip come back with logical
    shape [B, C, H, W] over NHWC memory, the weight's in the parameter's layout.  Besides its inputs and y autograd keeps one float per position.  C a multiple of
    4 up to 8192, with a skip a multiple of 8 up to 4096; at most 2^31 - 1 positions.  HIP only, exact fp32 only, 3 x 3 only: anything else raises ValueError --
    there is no torch fallback."""
    if not (torch.is_tensor(x) and torch.is_tensor(weight) and torch.is_tensor(bias)) or not (skip is None or torch.is_tensor(skip)):
        raise ValueError("dwconv_layernorm takes tensors")
    if x.dtype != torch.float32 or weight.dtype != torch.float32 or bias.dtype != torch.float32 or (skip is not None and skip.dtype != torch.float32):
        raise ValueError("dwconv_layernorm takes fp32 x, skip, weight and bias (got %s, %s, %s, %s)" % (x.dtype, None if skip is None else skip.dtype, weight.dtype, bias.dtype))
    if x.dim() != 4:
        raise ValueError("x must be [B, C, H, W] (got %s)" % (tuple(x.shape),))
    B, C, H, W = x.shape
    if skip is not None and tuple(skip.shape) != tuple(x.shape):
        raise ValueError("skip must have the shape of x, %s (got %s)" % (tuple(x.shape), tuple(skip.shape)))
    J = 1 if skip is None else 2
    if weight.dim() != 4 or weight.size(2) != 3 or weight.size(3) != 3:
        raise ValueError("weight %s: the fused ResBlock front takes a 3 x 3 depthwise kernel only" % (tuple(weight.shape),))
    if tuple(weight.shape) != (C, J, 3, 3) or bias.numel() != C:
        raise ValueError("weight must be [C, %d, 3, 3] %s a skip and bias [C] with C = x.size(1) = %d (got %s, %s)"
                         % (J, "with" if J == 2 else "without", C, tuple(weight.shape), tuple(bias.shape)))
    cmax, grain = (DW_MAX_C, 4) if skip is None else (DW_MAX_C_SKIP, 8)
    if C % grain or not grain <= C <= cmax:
        raise ValueError("C = %d: the fused ResBlock front takes a multiple of %d in %d...%d%s" % (C, grain, grain, cmax, "" if skip is None else " with a skip"))
    if B < 1 or H < 1 or W < 1 or B * H * W > DW_MAX_POSITIONS:
        raise ValueError("x %s: the fused ResBlock front takes 1...2^31 - 1 positions" % (tuple(x.shape),))
    eps = float(eps)
    if not 0.0 < eps < 1e30:  # (false for NaN)
        raise ValueError("eps = %r: must be positive and finite" % (eps,))
    if not x.is_cuda or weight.device != x.device or bias.device != x.device or (skip is not None and skip.device != x.device):
        raise ValueError("dwconv_layernorm runs on the HIP device only: x, skip, weight and bias must live on the same cuda device (got %s, %s, %s, %s)"
                         % (x.device, None if skip is None else skip.device, weight.device, bias.device))
    DW_COUNTERS["calls"] += 1
    return _DwconvLayerNorm.apply(_nhwc(x), None if skip is None else _nhwc(skip), _aligned(weight.contiguous()), _aligned(bias.contiguous().view(C)), eps)

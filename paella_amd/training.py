"""Training-mode forward of `Paella`: a differentiable evaluation built from torch ops over the module's own parameters.

SURVEY 8(f) rank 3: the reference's training loops (src/train.py:59-66, src_distributed/train.py:104-114) call
`model.train(); pred = model(noised, t, byt5...); loss.backward()`.  The HIP engine behind `Paella.forward` is an inference
engine (no saved activations; its only backward kernels are those of the training ops, paella_amd/train_ops.py), so in TRAIN mode -- `model.train()`, exactly the switch the reference's
loops flip -- `forward` routes here instead: the same network written as autograd-tracked torch ops (dropout active, as in the
reference).  `model.eval()` (the state a `paella_amd.Paella` is constructed in, and what the sampling path requires) never
reaches this file: sampling always runs the hand-written HIP kernels and fails loudly without them.

The arithmetic follows the reference's module definitions (file:line cited per function); it is written functionally over
the state-dict names so that the parameters of the SAME module are trained and the HIP engine picks the updated values up
on the next eval-mode call (`Paella._signature` tracks in-place optimizer updates).
"""
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from ._graph import GraphOwner

# the training ops and their limits live in train_ops.py; the network below calls them through THESE module globals (which is also where tests and tools look)
from .train_ops import (ACT_MAX_B, ACT_MAX_C, ACT_MAX_P, ATTN_COUNTERS, ATTN_MAX_B, ATTN_MAX_HEADS, ATTN_MAX_L, ATTN_MAX_P, ATTN_MAX_ROWS, DW_COUNTERS,  # noqa: F401
                        DW_MAX_C, DW_MAX_C_SKIP, DW_MAX_POSITIONS, HEAD_MAX_K, HEAD_MAX_LABELS, HEAD_MAX_ROWS, MOD_COUNTERS, MOD_MAX_B, MOD_MAX_C, MOD_MAX_P,
                        MOD_MAX_POSITIONS, attention_dropout, dwconv_layernorm, gelu_grn_dropout, head_cross_entropy, refuse_head_widths, timestep_modulate)
# the other half of an iteration: clip_grad_norm_ + AdamW as one HIP op, and the gradient norm alone
from .train_ops import ADAMW_COUNTERS, ClippedAdamW, adamw_chunk_plan, grad_norm  # noqa: F401
# the routed linears on bf16 operands (Paella.set_training_gemm("bf16")): the op, its shape rule, its counters, and the pack alone
from .train_ops import LINEAR_COUNTERS, LINEAR_GRAIN, LINEAR_MAX_DIM, linear_bf16, linear_shapes_ok, pack_bf16  # noqa: F401
# the dropout seeds of a forward as device words (`forward_loss(..., seeds=)`, `GraphTrainStep`)
from .train_ops import SEEDS_MAX_SITES, TrainSeeds  # noqa: F401
# the token stem as one op (Paella.set_training_embedding("hip")): embedding + LayerNorm + PixelUnshuffle, its counters and its limits
from .train_ops import EMBED_COUNTERS, EMBED_MAX_C, EMBED_MAX_LABELS, EMBED_MAX_POSITIONS, token_embed_layernorm  # noqa: F401

# The training switches of `Paella`, one row each: the field of the per-forward plan, the name everything else derives from, and its two settings (off is the
# default).  A new switch is a row here plus its branch in one block function below.  act = the middle of the MLP as one HIP op (`gelu_grn_dropout`), dw = the front
# of a ResBlock (`dwconv_layernorm`), attn = the attention core of an AttnBlock (`attention_dropout`), mod = the JOINT between blocks (`timestep_modulate`: a
# ResBlock / FeedForwardBlock in front of a TimestepBlock hands its two summands over unadded -- defer -- and the op's LayerNorm rows -- z -- go to the AttnBlock /
# FeedForwardBlock behind it), gemm = the routed linears -- the two of every MLP and, on the attn branch, the three projections of an AttnBlock -- through `_linear`,
# stem = the token stem at the top of `_forward_features` (`token_embed_layernorm`: embedding + LayerNorm + PixelUnshuffle as one HIP op, the 1x1 convolution behind it
# as a linear over its rows)
class Switch(namedtuple("Switch", "field name off on")):
    __slots__ = ()
    attr = property(lambda self: "_train_" + self.name)             # the module attribute (pickled state)
    setter = property(lambda self: "set_training_" + self.name)     # the public method of `Paella`
    label = property(lambda self: "training " + self.name)          # what `GraphTrainStep` calls it when it went stale
    refusal = property(lambda self: "training %s must be '%s' or '%s'" % (self.name, self.off, self.on))

    def read(self, model):
        """the present setting; a module unpickled from before the switch existed has its default"""
        return getattr(model, self.attr, self.off)


TRAIN_SWITCHES = (Switch("act", "activation", "torch", "hip"), Switch("dw", "depthwise", "torch", "hip"), Switch("attn", "attention", "torch", "hip"),
                  Switch("mod", "modulation", "torch", "hip"), Switch("gemm", "gemm", "fp32", "bf16"), Switch("stem", "embedding", "torch", "hip"))
# what `_forward_features` decides once per forward and hands down: per switch whether it ACTS, then train mode and the seed table
_Plan = namedtuple("_Plan", tuple(s.field for s in TRAIN_SWITCHES) + ("training", "seeds"))


def _plan(model, on, seeds=None):
    """on: whether the switches can act at all -- train mode on a cuda device; a switch at its default leaves every call as it is"""
    return _Plan(*(on and s.read(model) == s.on for s in TRAIN_SWITCHES), training=model.training, seeds=seeds)


def _levels(model):
    """(level index, blocks, whether the level takes its encoder output as a skip) in forward order: _down_encode, then _up_decode (src/modules.py:234-261)"""
    n_levels = len(model._cfg["c_hidden"])
    for i, blocks in enumerate(model.down_blocks):
        yield i, blocks, False
    for u, blocks in enumerate(model.up_blocks):
        yield n_levels - 1 - u, blocks, u > 0


def _level_dropout(model):
    """level index -> p of `model.dropout`, a scalar or one per level"""
    if isinstance(model.dropout, (list, tuple)):
        return lambda lvl: float(model.dropout[lvl])
    p_drop = float(model.dropout)
    return lambda lvl: p_drop


def _draws(plan, kind, p_drop):
    """whether a block of this kind draws a dropout mask in a HIP op, i.e. consumes a seed word: C / F under act, A under attn, where p > 0"""
    return p_drop > 0.0 and (plan.act if kind in ('C', 'F') else plan.attn if kind == 'A' else False)


def _linear(x, weight, bias, gemm=False):
    """F.linear; gemm (Paella.set_training_gemm("bf16"), train mode on a cuda device): `linear_bf16` where `linear_shapes_ok` holds, F.linear where it does not
    (counted in LINEAR_COUNTERS["fallbacks"])"""
    if gemm:
        if linear_shapes_ok(x.numel() // max(x.size(-1), 1), weight.size(0), weight.size(1)):
            return linear_bf16(x, weight, bias)
        LINEAR_COUNTERS["fallbacks"] += 1
    return F.linear(x, weight, bias)


def _ln_nchw(x, eps=1e-6):
    """LayerNorm2d without affine (src/modules.py:22-27): normalise over channels of an NCHW tensor."""
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.size(1),), None, None, eps).permute(0, 3, 1, 2)


def _site(plan, kind, p_drop):
    """the `seed=` of one HIP dropout op call: the next word of the table where the call draws a mask (p > 0), else None -- the op's own default"""
    return plan.seeds.site() if plan.seeds is not None and _draws(plan, kind, p_drop) else None


def _channelwise(blk, x_nhwc, p_drop, plan):
    """Linear -> GELU -> GlobalResponseNorm -> Dropout -> Linear (src/modules.py:49-53 / 30-40).  plan.act (Paella.set_training_activation("hip"), train mode on a cuda
    device): the three middle stages run as one HIP op in both directions (`gelu_grn_dropout`)."""
    cw = blk.channelwise._modules
    if plan.act:
        h = gelu_grn_dropout(_linear(x_nhwc, cw["0"].weight, cw["0"].bias, plan.gemm), cw["2"].gamma, cw["2"].beta, p_drop, _site(plan, blk.kind, p_drop))
        return _linear(h, cw["4"].weight, cw["4"].bias, plan.gemm)
    h = F.gelu(_linear(x_nhwc, cw["0"].weight, cw["0"].bias, plan.gemm))
    gx = torch.norm(h, p=2, dim=(1, 2), keepdim=True)
    nx = gx / (gx.mean(dim=-1, keepdim=True) + 1e-6)
    h = cw["2"].gamma * (h * nx) + cw["2"].beta + h
    h = F.dropout(h, p_drop, plan.training)
    return _linear(h, cw["4"].weight, cw["4"].bias, plan.gemm)


def _res_block(blk, x, skip, p_drop, plan, defer=False):
    """ResBlock (src/modules.py:43-62): depthwise 3x3 (groups = c, over cat([x, skip]) when a skip arrives) -> LN -> MLP -> + x.  plan.dw
    (Paella.set_training_depthwise("hip"), train mode on a cuda device): everything in front of the MLP runs as one HIP op in both directions
    (`dwconv_layernorm`), x and skip handed over separately -- no torch.cat.  defer: the two summands (MLP output, x) come back unadded."""
    res = x
    if plan.dw:
        y = dwconv_layernorm(x, blk.depthwise.weight, blk.depthwise.bias, skip)
    else:
        if skip is not None:
            x = torch.cat([x, skip], dim=1)
        dw = blk.depthwise
        c = dw.weight.size(0)
        y = _ln_nchw(F.conv2d(x, dw.weight, dw.bias, padding=dw.weight.size(-1) // 2, groups=c)).permute(0, 2, 3, 1)
    out = _channelwise(blk, y, p_drop, plan).permute(0, 3, 1, 2)
    return (out, res) if defer else out + res


def _ff_block(blk, x, p_drop, plan, z=None, defer=False):
    """FeedForwardBlock (src/modules.py:82-96).  z [B, H W, C]: the LayerNorm rows of x, already made by `timestep_modulate`; defer: the two summands
    (MLP output, x) come back unadded."""
    rows = _ln_nchw(x).permute(0, 2, 3, 1) if z is None else z.view(x.size(0), x.size(2), x.size(3), x.size(1))
    out = _channelwise(blk, rows, p_drop, plan).permute(0, 3, 1, 2)
    return (out, x) if defer else x + out


def _timestep_block(blk, x, r_embed):
    """TimestepBlock (src/modules.py:99-106)."""
    a, b = F.linear(r_embed, blk.mapper.weight, blk.mapper.bias)[:, :, None, None].chunk(2, dim=1)
    return x * (1 + a) + b


def _attn_block(blk, x, c_embed, nhead, self_attn, p_drop, plan, attn_weights=None, z=None):
    """AttnBlock (src/modules.py:65-79) around nn.MultiheadAttention semantics (Attention2D :7-19): queries = LN(x) positions,
    keys = values = [LN(x) positions | kv_mapper(SiLU(c_embed))], residual on the un-normed x.  plan.attn (Paella.set_training_attention("hip"), train mode
    on a cuda device): between the in-projection (one F.linear for the queries, one for keys and values together) and the out-projection the block runs as one HIP
    op in both directions (`attention_dropout`).  With attn_weights the torch branch below runs under either setting: the key-weight table stays an inference
    feature.  z [B, H W, C]: the LayerNorm rows of x, already made by `timestep_modulate` -- the queries on all three branches.  plan.gemm
    (Paella.set_training_gemm("bf16")): the q, kv and out projections of the plan.attn branch go through `_linear`; the other two branches keep their torch calls."""
    kvm = blk.kv_mapper._modules["1"]
    kv = F.linear(F.silu(c_embed), kvm.weight, kvm.bias)
    B, C, H, W = x.shape
    q = _ln_nchw(x).reshape(B, C, H * W).permute(0, 2, 1) if z is None else z
    if self_attn:
        kv = torch.cat([q, kv], dim=1)
    at = blk.attention.attn
    if attn_weights is None and plan.attn:
        w, bias = at.in_proj_weight, at.in_proj_bias
        out = attention_dropout(_linear(q, w[:C], bias[:C], plan.gemm), _linear(kv, w[C:], bias[C:], plan.gemm), nhead, p_drop, _site(plan, blk.kind, p_drop))
        out = _linear(out, at.out_proj.weight, at.out_proj.bias, plan.gemm)
    elif attn_weights is None:
        # torch's own functional form of nn.MultiheadAttention.forward (batch_first handled by the transposes): identical
        # arithmetic and identical dropout-stream consumption to the module the reference instantiates
        out, _ = F.multi_head_attention_forward(q.transpose(0, 1), kv.transpose(0, 1), kv.transpose(0, 1), C, nhead, at.in_proj_weight, at.in_proj_bias,
                                                None, None, False, p_drop, at.out_proj.weight, at.out_proj.bias, training=plan.training,
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
        w = F.dropout(w, p_drop, plan.training)
        out = F.linear((w @ vh).transpose(1, 2).reshape(B, -1, C), at.out_proj.weight, at.out_proj.bias)
    return x + out.permute(0, 2, 1).reshape(B, C, H, W)


@functools.lru_cache(maxsize=None)
def _timestep_freqs(half, max_positions, device):
    """The frequency table of gen_r_embedding, made on the HOST as the engine's is (Paella._engine: paella_unet_set_timestep_freqs) and kept per device.  The
    device's exp differs from the host's by one ulp in some entries (c_r = 64: entries near 1), and with angles of up to 1e4 a one-ulp frequency moves sine and
    cosine by up to 5e-4: made on the device, the table gave train mode another timestep embedding than eval mode evaluates for the same r.  The first call per
    (c_r, device) copies the table from the host inside the forward: a stream capture of a training step must follow an eager step (`GraphTrainStep` warms up first)."""
    return torch.arange(half).float().mul(-math.log(max_positions) / (half - 1)).exp().to(device)


def r_embedding(r, c_r, max_positions=10000):
    """gen_r_embedding (src/modules.py:212-221)."""
    r = r * max_positions
    half = c_r // 2
    freqs = _timestep_freqs(half, max_positions, r.device)
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


# torch's embedding backward has two forms: up to this many tokens one kernel, above it a sort of the tokens followed by a segmented sum (aten's embedding backward
# kernels: `num_indices <= 3072`)
EMBEDDING_CHUNK = 3072


def _token_embedding(x, weight, chunked):
    """F.embedding(x, weight).  chunked (a forward under a seed table -- the form a stream capture takes): in pieces of at most EMBEDDING_CHUNK tokens, so that every
    piece's backward is the one-kernel form.  OBSERVED: with the sorting form captured at 16 x 32x32 tokens, a later replay ended in a GPU memory fault inside
    rocprim's partition_kernel (the unique-by-key step of that form); graphs that hold the one-kernel form replay without one, at 512, 3200, 16384 and 65536 tokens.
    The cause is NOT established: by the kernels it launches here the sorting form keeps its segment count behind a device pointer and should be capturable, so what is wrong with it in a captured
    graph -- in torch, in the sort / partition library or in the graph runtime -- is an open question, and the pieces are a way round it, not a fix.  The weight's
    gradient is then the sum of the pieces' gradients: the values of the one-piece call in another summation order.  Up to EMBEDDING_CHUNK tokens the call is
    F.embedding itself.  Paella.set_training_embedding("hip") takes the whole stem off this path: `token_embed_layernorm` writes the weight's gradient in one launch
    that a graph holds at any token count, and this function is then not reached, with or without seeds."""
    if not chunked or x.numel() <= EMBEDDING_CHUNK:
        return F.embedding(x, weight)
    pieces = [F.embedding(piece, weight) for piece in x.reshape(-1).split(EMBEDDING_CHUNK)]
    return torch.cat(pieces, dim=0).view(*x.shape, weight.size(1))


def _forward_features(model, x, r, byt5, clip=None, clip_image=None, x_cat=None, attn_weights=None, seeds=None):
    """Paella.forward (src/modules.py:263-275) as autograd-tracked torch ops, up to and including the LayerNorm2d in front of out_mapper's convolution:
    [B, c_out, H, W] as the permuted view of an NHWC tensor that `_ln_nchw` returns.  seeds (a `TrainSeeds`): every HIP dropout op call with p > 0 takes the
    table's next word as its seed, in forward order (`dropout_sites` counts them); a call at p = 0 and the torch routes consume none.  Under seeds the token
    embedding of more than EMBEDDING_CHUNK tokens is looked up in pieces (`_token_embedding`): the one difference from the forward without seeds -- and none with
    plan.stem (Paella.set_training_embedding("hip"), train mode on a cuda device), where the stem up to the 1x1 convolution's input is one HIP op in both directions
    (`token_embed_layernorm`) and the convolution a linear over its rows."""
    if seeds is not None:
        seeds.begin()
    cfg = model._cfg
    # the training switches (TRAIN_SWITCHES): decided once, here -- a switch acts in train mode on a cuda device only; its default leaves every call below as it is
    plan = _plan(model, model.training and x.is_cuda, seeds)
    drop = _level_dropout(model)
    if x_cat is not None:
        x = torch.cat([x, x_cat], dim=1)
    # (the embedding is made in fp32 whatever the module's dtype -- its angles are fp32 products by definition -- and handed over in the dtype of the parameters:
    # an fp32 module gets the same tensor, a module converted with .double() the fp32 embedding widened)
    r_embed = r_embedding(r.float(), cfg["c_r"]).to(model.clf._modules["1"].weight.dtype)
    c_embed = c_embeddings(model, byt5, clip, clip_image)
    patch = cfg["patch_size"]

    emb = model.embedding._modules["1"]
    if plan.stem:
        rows = token_embed_layernorm(x, model.in_mapper._modules["0"].weight, patch)         # [B, H/p, W/p, c_in p^2]
        h = _linear(rows, emb.weight.view(emb.weight.size(0), -1), emb.bias, plan.gemm)     # the 1x1 convolution as a linear
        # the NCHW view of NHWC memory: plan.dw's channels_last copy below is then a no-op
        h = F.layer_norm(h, (emb.weight.size(0),), None, None, 1e-6).permute(0, 3, 1, 2)
    else:
        h = F.layer_norm(_token_embedding(x, model.in_mapper._modules["0"].weight, seeds is not None), (cfg["c_in"],), None, None, 1e-6).permute(0, 3, 1, 2)
        h = _ln_nchw(F.conv2d(F.pixel_unshuffle(h, patch), emb.weight, emb.bias))

    if plan.dw:  # the trunk is made channels_last once, here, so that the blocks hand each other NHWC memory
        h = h.contiguous(memory_format=torch.channels_last)

    def run(blk, level, h, skip=None, z=None, defer=False):
        if blk.kind == 'C':
            return _res_block(blk, h, skip, drop(level), plan, defer)
        if blk.kind == 'A':
            return _attn_block(blk, h, c_embed, cfg["nhead"][level], cfg["self_attn"], drop(level), plan, attn_weights, z)
        if blk.kind == 'T':
            return _timestep_block(blk, h, r_embed)
        if blk.kind == 'F':
            return _ff_block(blk, h, drop(level), plan, z, defer)
        if blk.kind == 'D':  # LayerNorm2d + Conv2d(k2, s2)   (src/modules.py:153-156)
            cv = blk._modules["1"]
            return F.conv2d(_ln_nchw(h), cv.weight, cv.bias, stride=2)
        if blk.kind == 'U':  # LayerNorm2d + ConvTranspose2d(k2, s2)   (src/modules.py:172-175)
            cv = blk._modules["1"]
            return F.conv_transpose2d(_ln_nchw(h), cv.weight, cv.bias, stride=2)
        raise RuntimeError("unknown block kind %r" % blk.kind)

    def run_level(level, i, h, skip=None):
        """the blocks of one level in order; skip goes to a ResBlock that comes first.  With plan.mod, a C / F block right in front of a T block hands (MLP output,
        its input) over unadded, the T block is one `timestep_modulate` call, and when an A / F block follows in the level the op makes its LayerNorm rows too"""
        level = list(level)
        z = None
        for j, blk in enumerate(level):
            nxt = level[j + 1].kind if j + 1 < len(level) else None
            sk = skip if (j == 0 and blk.kind == 'C') else None
            if not plan.mod:
                h = run(blk, i, h, sk)
            elif blk.kind == 'T':
                x, res = h if isinstance(h, tuple) else (h, None)
                ab = F.linear(r_embed, blk.mapper.weight, blk.mapper.bias)
                if nxt in ('A', 'F'):
                    h, z = timestep_modulate(x, ab, res, True)
                else:
                    h = timestep_modulate(x, ab, res)
            else:
                h, z = run(blk, i, h, sk, z, defer=blk.kind in ('C', 'F') and nxt == 'T'), None
        return h

    encoded = {}
    for i, level, skip in _levels(model):
        h = run_level(level, i, h, encoded[i] if skip else None)
        encoded.setdefault(i, h)                           # the way down passes every level first: what is kept is the encoder's output
    clf = model.clf._modules["1"]
    h = F.pixel_shuffle(F.conv2d(_ln_nchw(h), clf.weight, clf.bias), patch)
    return _ln_nchw(h)


def forward_autograd(model, x, r, byt5, clip=None, clip_image=None, x_cat=None, attn_weights=None):
    """Paella.forward (src/modules.py:263-275) as autograd-tracked torch ops.  Returns logits [B, num_labels, H, W]."""
    return F.conv2d(_forward_features(model, x, r, byt5, clip, clip_image, x_cat, attn_weights), model.out_mapper._modules["1"].weight)


def forward_loss(model, x, r, target, byt5, clip=None, clip_image=None, x_cat=None, attn_weights=None, label_smoothing=0.1, seeds=None):
    """One training forward with the loss head fused: (loss [B, H, W], correct [B, H, W] bool) instead of logits [B, num_labels, H, W].  seeds: a `TrainSeeds` whose
    words the HIP dropout ops take as their seeds (None: every op draws its own, as always)."""
    w = model.out_mapper._modules["1"].weight
    refuse_head_widths(w.size(1), w.size(0))      # before the network runs: a refused call has drawn no seed and launched nothing
    if seeds is not None and not isinstance(seeds, TrainSeeds):
        raise ValueError("seeds must be a paella_amd.training.TrainSeeds (got %s)" % type(seeds).__name__)
    feat = _forward_features(model, x, r, byt5, clip, clip_image, x_cat, attn_weights, seeds)
    loss, argmax = head_cross_entropy(feat.permute(0, 2, 3, 1), model.out_mapper._modules["1"].weight, target, label_smoothing)
    return loss, argmax == target


def dropout_sites(model):
    """How many words of a `TrainSeeds` one train-mode forward of `model` on a cuda device consumes under its PRESENT switches and `model.dropout`: one per
    `gelu_grn_dropout` call (every C / F block, with set_training_activation("hip")) and one per `attention_dropout` call (every A block, with
    set_training_attention("hip")) whose level has p > 0.  The torch routes draw through torch's generator and count nothing."""
    plan, drop = _plan(model, True), _level_dropout(model)
    return sum(1 for i, level, _ in _levels(model) for blk in level if _draws(plan, blk.kind, drop(i)))


_STEP_INPUTS = ("noised", "t", "latents", "byt5", "clip", "clip_image", "x_cat", "loss_weight")


class GraphTrainStep(GraphOwner):
    """One whole training iteration of src/train.py:59-69 -- `forward_loss`, the loss reduction, `backward()`, clip_grad_norm_ + AdamW (`ClippedAdamW`) -- captured
    ONCE into a HIP graph for fixed shapes and replayed per call: the same kernels as the eager iteration plus one launch that advances the dropout seeds, submitted
    as one graph instead of some two thousand launches.

        step = GraphTrainStep(model, opt, dict(noised=, t=, latents=, byt5=[, clip=, clip_image=, x_cat=, loss_weight=]))
        loss, accuracy, grad_norm = step(noised=..., t=..., latents=..., byt5=..., ...)        # 0-dim device tensors owned by the graph, valid until the next call

    Loss: with `loss_weight` ((loss * lw).sum([1, 2]) / lw.sum([1, 2])).mean() (src_distributed/train.py:107), without it loss.mean() (src/train.py); accuracy is
    (argmax == latents).float().mean().  The model must be in train mode on a cuda device and the optimizer a `ClippedAdamW` over its parameters: anything else raises.
    What changes from replay to replay although the graph is fixed:
      * the inputs -- copied into the graph's static buffers (a shape or dtype that differs from the example's raises ValueError; an input left out keeps its buffer);
      * the dropout masks -- `.seeds` (a `TrainSeeds` sized by `dropout_sites`) is advanced INSIDE the graph, so replay k draws the words of iteration k;
        `seed=` is its base (None: one draw from torch's CPU generator, so torch.manual_seed reproduces a run); `.seeds` stays ONE object for the life of the step --
        a recapture that needs more sites grows it in place (`TrainSeeds.grow`);
      * the hyperparameters -- the optimizer's table is rebuilt from `param_groups` and uploaded eagerly on the current stream before every replay (only the three
        launches of the step sit in the graph), so a scheduler's `lr` acts as in the eager loop.
    A call does not synchronise with the device.  Every updated parameter's version is raised, so the HIP engine and captured sampling graphs notice the new weights.
    Construction: optimizer state is materialised, ONE warm-up forward + backward runs on a side stream without an optimizer step (timestep-frequency table, allocator
    pools, library selections), the gradients are set to None and the iteration is captured (capture_error_mode="thread_local", one stream: the graph has no parallel
    branches); the seed table is put back to its state from before the warm-up after both.  Weights, optimizer state and step counts are untouched, and the first
    replay draws the words of iteration 1.  After the capture p.grad of every parameter is a tensor owned by the graph that each replay rewrites: there is no
    zero_grad in the loop (a p.grad that was replaced or set to None is put back before the next replay).
    Staleness, as `GraphSampler`: before a replay the data_ptr of every parameter and optimizer state tensor, the six training switches, `model.dropout`
    and train mode are compared with what the capture saw; on a difference the step is captured again (on_stale="recapture"; `.captures` counts) or a RuntimeError
    names the cause (on_stale="raise").  The call counters of the ops (ATTN_COUNTERS, MOD_COUNTERS, LINEAR_COUNTERS, ...) and ADAMW_COUNTERS count Python calls: they
    move at capture time only, never at a replay.
    The token embedding: under the default `set_training_embedding("torch")` a captured forward of more than EMBEDDING_CHUNK tokens looks the tokens up in pieces
    (`_token_embedding`); under `set_training_embedding("hip")` the stem is `token_embed_layernorm` -- one forward and one backward launch at any token count, no
    pieces and no torch embedding backward in the graph.
    Not offered: gradient accumulation inside the graph, DDP, GradScaler / autocast, the `attn_weights` branch."""

    _noun = "captured iteration"

    def __init__(self, model, optimizer, example_inputs, *, label_smoothing=0.1, seed=None, on_stale="recapture"):
        self._init_owner(on_stale)
        if not isinstance(optimizer, ClippedAdamW):
            raise TypeError("GraphTrainStep captures the HIP optimizer step: the optimizer must be a paella_amd.training.ClippedAdamW (got %s)" % type(optimizer).__name__)
        params = [p for p in model.parameters()]
        if not params or not all(p.is_cuda for p in params):
            raise ValueError("GraphTrainStep runs on the HIP device only: move the model to a cuda device first")
        self.model, self.optimizer, self.label_smoothing = model, optimizer, float(label_smoothing)
        self.device = params[0].device
        self._refuse_eval()
        unknown = sorted(set(example_inputs) - set(_STEP_INPUTS))
        if unknown:
            raise ValueError("example_inputs takes %s (got also %s)" % (", ".join(_STEP_INPUTS), ", ".join(unknown)))
        for k in ("noised", "t", "latents", "byt5"):
            if example_inputs.get(k) is None:
                raise ValueError("example_inputs needs %s" % k)
        clone = lambda v: [t.detach().to(self.device).clone() for t in v] if isinstance(v, (list, tuple)) else v.detach().to(self.device).clone()
        self.inputs = {k: clone(v) for k, v in example_inputs.items() if v is not None}
        self.seeds = TrainSeeds(max(dropout_sites(model), 1), seed, self.device)
        self.graph = self.out = None
        self._capture()

    def _refuse_eval(self):
        if not self.model.training:
            raise RuntimeError("GraphTrainStep captures the training path and this module is in eval mode: call model.train() first")

    # ---- what a capture depends on besides the shapes
    def _state(self):
        m, opt = self.model, self.optimizer
        ps = list(m.parameters())
        state = []
        for p in ps:
            st = opt.state.get(p) or {}
            state.append(tuple(None if st.get(k) is None else st[k].data_ptr() for k in ("step", "exp_avg", "exp_avg_sq")))
        return [("parameter storage", tuple(p.data_ptr() for p in ps)), ("parameters that require a gradient", tuple(p.requires_grad for p in ps)),
                ("optimizer state storage", (tuple(state), None if opt._rows_dev is None else opt._rows_dev.data_ptr(), None if opt._ws is None else opt._ws.data_ptr(),
                                             tuple(id(p) for p in opt._params()), opt.max_norm))] + \
               [(s.label, s.read(m)) for s in TRAIN_SWITCHES] + \
               [("model.dropout", tuple(m.dropout) if isinstance(m.dropout, (list, tuple)) else float(m.dropout)), ("train mode", bool(m.training))]

    def _iteration(self, optimize):
        """seeds.advance -> forward_loss -> reduction -> backward [-> the optimizer's launch part]; -> (loss, accuracy, norm or None)"""
        i = self.inputs
        self.seeds.advance()
        per_pos, correct = forward_loss(self.model, i["noised"], i["t"], i["latents"], i["byt5"], i.get("clip"), i.get("clip_image"), i.get("x_cat"), None,
                                        self.label_smoothing, self.seeds)
        lw = i.get("loss_weight")
        loss = per_pos.mean() if lw is None else ((per_pos * lw).sum(dim=[1, 2]) / lw.sum(dim=[1, 2])).mean()
        loss.backward()
        acc = correct.float().mean()
        norm = None
        if optimize:
            with torch.no_grad():
                # the plan reads the addresses of the gradients this capture's backward made, so it runs here; it is host code and enqueues nothing, because the state,
                # the table and the workspace exist (materialize_state) and the gradients are dense fp32 -- `_capture` refuses a plan that had to make a temporary
                self._plan = self.optimizer._plan()
                norm = self.optimizer._launch(self._plan)
        return loss.detach(), acc, norm

    def _capture(self):
        self._refuse_eval()
        opt, m = self.optimizer, self.model
        if self.seeds.n_sites < dropout_sites(m):           # a switch or model.dropout added drawing calls since the table was sized: `.seeds` grows in place
            self.seeds.grow(dropout_sites(m))
        before = getattr(self, "_captured_state", None), self.captures
        self.graph = self.out = self._plan = None
        self._grads = []
        opt.materialize_state()
        snap = self.seeds.snapshot()

        def after_warmup():                                 # the seed table as before the warm-up, and no gradient tensor for the capture's backward to add to
            self.seeds.restore(snap)
            m.zero_grad(set_to_none=True)
        # warm-up: ONE iteration without the optimizer step, nothing but gradients is written
        out = self._capture_graph(lambda: self._iteration(optimize=True), warmup=lambda: self._iteration(optimize=False), n_warmup=1, after_warmup=after_warmup,
                                  after_capture=lambda: self.seeds.restore(snap))
        if self._plan["keep"] and any(g is not p.grad for g, p in zip(self._plan["keep"], self._plan["updated"])):
            self.graph, (self._captured_state, self.captures) = None, before   # not a capture to replay: the step is as stale as it was
            raise RuntimeError("GraphTrainStep: a gradient is not dense fp32 on the parameters' device; the captured optimizer step would read a temporary")
        self._grads = [(p, p.grad) for p in self._plan["updated"]]
        self.out = out

    def _copy_inputs(self, given):
        unknown = sorted(set(given) - set(_STEP_INPUTS))
        if unknown:
            raise ValueError("GraphTrainStep takes %s (got also %s)" % (", ".join(_STEP_INPUTS), ", ".join(unknown)))
        todo = []
        for k, src in given.items():
            if src is None:
                continue
            dst = self.inputs.get(k)
            if dst is None:
                raise ValueError("the iteration was captured without %s" % k)
            pairs = list(zip(dst, src)) if isinstance(dst, list) and isinstance(src, (list, tuple)) and len(src) == len(dst) else None if isinstance(dst, list) or \
                isinstance(src, (list, tuple)) else [(dst, src)]
            if pairs is None:
                raise ValueError("%s: the captured iteration takes %s" % (k, "a list of %d tensors" % len(dst) if isinstance(dst, list) else "one tensor"))
            for d, s in pairs:
                if not torch.is_tensor(s) or tuple(s.shape) != tuple(d.shape) or s.dtype != d.dtype:
                    raise ValueError("%s: the captured iteration takes %s %s (got %s)" % (k, d.dtype, tuple(d.shape), "%s %s" % (s.dtype, tuple(s.shape))
                                                                                             if torch.is_tensor(s) else type(s).__name__))
                todo.append((d, s))
        for d, s in todo:       # only after every input was accepted
            d.copy_(s, non_blocking=True)

    def __call__(self, inputs=None, **more):
        given = dict(inputs or {}, **more)
        self._check_fresh()
        self._copy_inputs(given)
        opt = self.optimizer
        for p, g in self._grads:                         # (a loop that still calls zero_grad(set_to_none=True): the graph writes these tensors, so they are what p.grad is)
            if p.grad is not g:
                p.grad = g
        with torch.no_grad():
            opt._plan_hyper(self._plan["rows"])          # lr, betas, eps, weight_decay as param_groups hold them NOW
            opt._upload(self._plan)                      # eager, on the stream the replay follows on
        self.graph.replay()
        opt.grad_norm = self.out[2]
        if self._plan["updated"]:
            torch.autograd.graph.increment_version(self._plan["updated"])
        return self.out

"""The training ops: stretches of the train-mode network (paella_amd/training.py) that run as ONE HIP op in both directions, each a `torch.autograd.Function`
over a pair of C entry points plus the public function that validates its arguments and hands dense, aligned tensors over.  HIP only: there is no torch fallback.

Every op is written against the same scaffold, the helpers right below (the host side of the same scaffold is paella_amd/csrc/train_common.h):
    _call          one checked library call under the tensors' device, with a fresh workspace of plain bytes -- the ops keep no state in it and initialise nothing
    _grad_outputs  the backward's outputs from `needs_input_grad`: a NULL output is not computed, and when none is wanted the call is skipped
    _refuse_*      the refusals every op makes -- not tensors, not the right dtype, not one cuda device, a scalar outside its range -- each op in its own order
`paella_amd.training` imports the public names into its own namespace and the network calls them through those module globals."""
import numpy as np
import torch

from . import _lib


def _call(entry, dev, ws_bytes, *args):
    """lib.<entry>(*args, workspace, its size, the current stream of dev): tensors go as their addresses (None as NULL), a non-zero return raises"""
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(getattr(lib, entry)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev)))


def _grad_outputs(ctx, *like):
    """one entry per input of the Function, in order: an empty tensor like like[i] (a shape: of that shape, otherwise like like[0]) where autograd wants that
    gradient, else None; like[i] = None for an input that has no gradient.  -> (the list, whether anything is wanted at all)"""
    outs = [None if t is None or not need else torch.empty_like(t) if isinstance(t, torch.Tensor) else like[0].new_empty(t) for t, need in zip(like, ctx.needs_input_grad)]
    return outs, any(o is not None for o in outs)


def _refuse_non_tensors(op, *tensors):
    if not all(torch.is_tensor(t) for t in tensors):
        raise ValueError("%s takes tensors" % op)


def _got(tensors, field):
    return ", ".join(str(None if t is None else getattr(t, field)) for t in tensors)


def _refuse_dtypes(op, what, tensors, dtypes=None):
    """tensors (None = an absent optional one) must have the given dtypes, fp32 unless said otherwise; `what` reads "fp32 u, gamma and beta" """
    if any(t is not None and t.dtype != d for t, d in zip(tensors, dtypes or [torch.float32] * len(tensors))):
        raise ValueError("%s takes %s (got %s)" % (op, what, _got(tensors, "dtype")))


def _refuse_off_device(op, what, tensors):
    """the first tensor must be on a cuda device and the others (None = absent) on the same one; `what` reads "u, gamma and beta" """
    if not tensors[0].is_cuda or any(t is not None and t.device != tensors[0].device for t in tensors[1:]):
        raise ValueError("%s runs on the HIP device only: %s must live on the same cuda device (got %s)" % (op, what, _got(tensors, "device")))


def _refuse_out_of_range(name, shown, ok, rule):
    if not ok:  # (a comparison chain is false for NaN)
        raise ValueError("%s = %r: %s" % (name, shown, rule))


def _aligned(t):
    """the kernels move 16-byte vectors: a contiguous view that starts off that grain is copied"""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _dropout_seed(op, seed, p, dev):
    """the `seed=` argument of the two dropout ops -> what the Function carries: 0 at p = 0 (nothing is drawn, nothing is consumed); an int as its low 64 bits;
    a one-element int64 tensor on dev (a `TrainSeeds.site()`: the kernels load the word when they run) as it is; None: one draw from torch's default CPU generator
    -- refused while the current stream is capturing, where that host value would be frozen into the graph and every replay would repeat its masks"""
    if p == 0.0:
        return 0
    if torch.is_tensor(seed):
        if seed.device != dev:
            raise ValueError("%s: a tensor seed must live on the op's device %s (got %s)" % (op, dev, seed.device))
        return seed.detach()
    if seed is None:
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("%s: seed=None with p > 0 while the stream is capturing: the seed would be drawn on the host once and frozen into the graph. "
                               "Pass seed=<a device word> (paella_amd.training.TrainSeeds.site())" % op)
        seed = int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def _refuse_seed_tensor(op, seed):
    """a tensor handed over as `seed=` is one dense int64 element (asked before the device checks, whatever p is)"""
    if torch.is_tensor(seed) and (seed.dtype != torch.int64 or seed.numel() != 1 or seed.layout != torch.strided or not seed.is_contiguous()):
        raise ValueError("%s: a tensor seed must be one dense int64 element (got %s %s, %s)" % (op, seed.dtype, tuple(seed.shape), seed.layout))


def _seed_entry(entry, seed):
    """the entry point that takes this seed: by value, or `<entry>_seed_dev` for a device word"""
    return entry + "_seed_dev" if torch.is_tensor(seed) else entry


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Training loss head: out_mapper's convolution + label-smoothed cross-entropy as ONE HIP op, forward and backward (paella_amd/csrc/loss.hip,
# include/paella_hip.h "Training loss head").  The [rows, num_labels] logits, their log-softmax and their gradient are never stored: the forward keeps
# five numbers per row, the backward recomputes the logit tiles from h, the weight and the saved lse.
# ---------------------------------------------------------------------------------------------------------------------------------------------------
HEAD_MAX_K, HEAD_MAX_LABELS, HEAD_MAX_ROWS = 256, 65536, 1 << 24


def refuse_head_widths(K, N):
    """the widths the fused head takes: K features and N labels, multiples of 16 (`head_cross_entropy`; `training.forward_loss` asks before it runs the network)"""
    if K % 16 or not 16 <= K <= HEAD_MAX_K:
        raise ValueError("K = %d: the fused head takes a multiple of 16 in 16...%d" % (K, HEAD_MAX_K))
    if N % 16 or not 16 <= N <= HEAD_MAX_LABELS:
        raise ValueError("N = %d labels: the fused head takes a multiple of 16 in 16...%d" % (N, HEAD_MAX_LABELS))


class _HeadCrossEntropy(torch.autograd.Function):
    """(h [rows, K], weight [N, K], target [rows]) -> (loss fp32 [rows], argmax int32 [rows]); saves h, weight, target and lse [rows]."""

    @staticmethod
    def forward(ctx, h, weight, target, eps):
        rows, K = h.shape
        N = weight.size(0)
        loss = h.new_empty(rows)
        lse = h.new_empty(rows)
        argmax = torch.empty(rows, dtype=torch.int32, device=h.device)
        _call("paella_head_loss_forward", h.device, _lib.load().paella_head_loss_workspace_bytes(rows, N, K), h, weight, target, rows, N, K, eps, loss, lse, argmax)
        ctx.save_for_backward(h, weight, target, lse)
        ctx.eps = eps
        ctx.mark_non_differentiable(argmax)
        return loss, argmax

    @staticmethod
    def backward(ctx, grad_loss, _grad_argmax):
        h, weight, target, lse = ctx.saved_tensors
        rows, K = h.shape
        N = weight.size(0)
        g = grad_loss.to(torch.float32).contiguous()
        (dh, dw, _, _), wanted = _grad_outputs(ctx, h, weight, None, None)
        if wanted:
            _call("paella_head_loss_backward", h.device, _lib.load().paella_head_loss_workspace_bytes(rows, N, K), h, weight, target, lse, g, rows, N, K, ctx.eps, dh, dw)
        return dh, dw, None, None


def head_cross_entropy(h, weight, target, label_smoothing=0.0):
    """Classifier head + cross-entropy without a logits tensor: with l = h @ weight^T,
        loss   = nn.CrossEntropyLoss(label_smoothing=label_smoothing, reduction='none')(l, target)     (fp32, the shape of `target`; differentiable in h and weight)
        argmax = l.argmax(-1), the lowest label on ties                                                  (int32, not differentiable)
    h fp32 [..., K]; weight fp32 [N, K] or [N, K, 1, 1] (out_mapper.1.weight); target int64 with the leading shape of h.  A target outside [0, N) marks an
    ignored position (loss 0, no gradient), as ignore_index does.  K a multiple of 16 up to 256, N a multiple of 16 up to 65536, at most 2^24 positions.
    HIP only and exact fp32 only: anything else raises ValueError -- there is no torch fallback."""
    _refuse_non_tensors("head_cross_entropy", h, weight, target)
    _refuse_off_device("head_cross_entropy", "h, weight and target", (h, weight, target))
    _refuse_dtypes("head_cross_entropy", "fp32 h and weight and int64 target", (h, weight, target), (torch.float32, torch.float32, torch.int64))
    if weight.dim() == 4 and weight.size(2) == 1 and weight.size(3) == 1:
        weight = weight.reshape(weight.size(0), weight.size(1))
    if weight.dim() != 2 or h.dim() < 1 or h.size(-1) != weight.size(1):
        raise ValueError("weight must be [N, K] or [N, K, 1, 1] with K = h.size(-1) (got h %s, weight %s)" % (tuple(h.shape), tuple(weight.shape)))
    N, K = weight.shape
    lead = h.shape[:-1]
    if tuple(target.shape) != tuple(lead):
        raise ValueError("target must have the leading shape of h, %s (got %s)" % (tuple(lead), tuple(target.shape)))
    rows = target.numel()
    refuse_head_widths(K, N)
    if not 1 <= rows <= HEAD_MAX_ROWS:
        raise ValueError("%d positions: the fused head takes 1...%d" % (rows, HEAD_MAX_ROWS))
    eps = float(label_smoothing)
    _refuse_out_of_range("label_smoothing", label_smoothing, 0.0 <= eps < 1.0, "must lie in [0, 1)")
    # rows must be contiguous; the NHWC view behind `_ln_nchw`'s result already is (no copy)
    h2 = h.view(rows, K) if h.is_contiguous() else h.contiguous().view(rows, K)
    loss, argmax = _HeadCrossEntropy.apply(h2, weight.contiguous(), target.contiguous().view(rows), eps)
    return loss.view(lead), argmax.view(lead)


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
        B, P, C = u.shape
        z = torch.empty_like(u)
        gx = u.new_empty(B, C)
        _call(_seed_entry("paella_grn_act_forward", seed), u.device, _lib.load().paella_grn_act_workspace_bytes(B, P, C), u, gamma, beta, B, P, C, p, seed, z, gx)
        ctx.save_for_backward(u, gamma, gx)
        ctx.p, ctx.seed = p, seed
        return z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dz):
        u, gamma, gx = ctx.saved_tensors
        B, P, C = u.shape
        dz = _aligned(dz.to(torch.float32).contiguous())
        (du, dgamma, dbeta, _, _), wanted = _grad_outputs(ctx, u, gamma, gamma, None, None)
        if wanted:
            _call(_seed_entry("paella_grn_act_backward", ctx.seed), u.device, _lib.load().paella_grn_act_workspace_bytes(B, P, C), u, gamma, gx, dz, B, P, C, ctx.p, ctx.seed, du, dgamma, dbeta)
        return du, dgamma, dbeta, None, None


def gelu_grn_dropout(u, gamma, beta, p=0.0, seed=None):
    """The middle of a ResBlock / FeedForwardBlock MLP in train mode as one op: with h = gelu(u),
        z = dropout(gamma * (h * nx) + beta + h, p),   nx = Gx / (mean_c Gx + 1e-6),   Gx = ||h||_2 over the positions of a sample
    (src/modules.py:30-40, 49-53).  u fp32 [B, ..., C] (the dimensions between the first and the last are the positions of a sample); gamma, beta fp32 with C
    elements (the module's [1, 1, 1, C] parameters as they are).  Once differentiable in u, gamma and beta; autograd keeps u, gamma and Gx [B, C] only.  p in
    [0, 1); p = 0 draws nothing.  The dropout mask is a function of (seed, element index): seed = None with p > 0 draws one 64-bit seed from torch's default CPU
    generator, so torch.manual_seed reproduces a run (refused with RuntimeError while the stream is capturing: that value would be frozen into the graph).  seed may also be a
    one-element int64 tensor on u's device: the kernels load the word when they run, in both directions -- a word that holds s gives the bits of seed = s, and the
    backward must find the word its forward found (`TrainSeeds`).  C a multiple of 4 up to 16384, at most 2^20 positions per sample, B up to 65535.  HIP only and exact fp32
    only: anything else raises ValueError -- there is no torch fallback."""
    _refuse_non_tensors("gelu_grn_dropout", u, gamma, beta)
    _refuse_dtypes("gelu_grn_dropout", "fp32 u, gamma and beta", (u, gamma, beta))
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
    _refuse_out_of_range("p", p, 0.0 <= p < 1.0, "must lie in [0, 1)")
    _refuse_seed_tensor("gelu_grn_dropout", seed)
    _refuse_off_device("gelu_grn_dropout", "u, gamma and beta", (u, gamma, beta))
    seed = _dropout_seed("gelu_grn_dropout", seed, p, u.device)
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
        B, H, W, C = x.shape
        y = torch.empty_like(x)
        rstd = x.new_empty(B, H, W)
        # the forward asks for the repacked weights only, which is what the sizing call returns for one position
        _call("paella_dwconv_ln_train_forward", x.device, _lib.load().paella_dwconv_ln_train_workspace_bytes(1, 1, 1, C, int(skip is not None)), x, skip, weight, bias,
              B, H, W, C, eps, y, rstd)
        ctx.save_for_backward(x, skip, weight, y, rstd)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, skip, weight, y, rstd = ctx.saved_tensors
        B, H, W, C = x.shape
        dy = _aligned(dy.to(torch.float32).contiguous())
        (dx, dskip, dw, dbias, _), wanted = _grad_outputs(ctx, x, skip, weight, (C,), None)
        if wanted:
            _call("paella_dwconv_ln_train_backward", x.device, _lib.load().paella_dwconv_ln_train_workspace_bytes(B, H, W, C, int(skip is not None)), x, skip, weight, y,
                  rstd, dy, B, H, W, C, dx, dskip, dw, dbias)
        return dx, dskip, dw, dbias, None


def _nhwc(t, counters=DW_COUNTERS):
    """[B, C, H, W] of any strides -> its [B, H, W, C] view when the memory is already dense NHWC and 16-byte aligned, else one copy (counted in counters["copied"])"""
    v = t.permute(0, 2, 3, 1)
    if v.is_contiguous() and v.data_ptr() % 16 == 0:
        return v
    counters["copied"] += 1
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
    _refuse_non_tensors("dwconv_layernorm", x, weight, bias, *(() if skip is None else (skip,)))
    _refuse_dtypes("dwconv_layernorm", "fp32 x, skip, weight and bias", (x, skip, weight, bias))
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
    _refuse_out_of_range("eps", eps, 0.0 < eps < 1e30, "must be positive and finite")
    _refuse_off_device("dwconv_layernorm", "x, skip, weight and bias", (x, skip, weight, bias))
    DW_COUNTERS["calls"] += 1
    return _DwconvLayerNorm.apply(_nhwc(x), None if skip is None else _nhwc(skip), _aligned(weight.contiguous()), _aligned(bias.contiguous().view(C)), eps)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Training attention: softmax(q k^T / sqrt(D)) v with dropout on the probabilities as ONE HIP op, forward and backward, flash style
# (paella_amd/csrc/attn_train.hip, include/paella_hip.h "Training attention").  Besides its inputs and its output autograd keeps one float per (sample, head,
# query): the [B, nhead, P, L] scores, probabilities and dropout mask of the torch chain never exist -- the backward recomputes the probabilities from q, k and
# lse, the mask from a (seed, element index) counter.
# ---------------------------------------------------------------------------------------------------------------------------------------------------
ATTN_MAX_B, ATTN_MAX_HEADS, ATTN_MAX_P, ATTN_MAX_L, ATTN_MAX_ROWS = 65535, 65535, 1 << 20, 1 << 20, 2 ** 31 - 1
# diagnostic: how often `attention_dropout` ran (tests, tools/bench_train_attention.py)
ATTN_COUNTERS = {"calls": 0}


class _AttentionDropout(torch.autograd.Function):
    """(q [B, P, C], kv [B, L, 2C]) -> o [B, P, C]; saves q, kv, o and lse [B, nhead, P].  k and v are the two halves of kv's rows and dk, dv the two halves of
    dkv's: the strides of the C entry points take them in place."""

    @staticmethod
    def forward(ctx, q, kv, nhead, p, seed):
        B, P, C = q.shape
        L, D = kv.size(1), C // nhead
        o = torch.empty_like(q)
        lse = q.new_empty(B, nhead, P)
        _call(_seed_entry("paella_attn_train_forward", seed), q.device, _lib.load().paella_attn_train_workspace_bytes(B, nhead, P, L, D), q, C, kv[..., :C], 2 * C, kv[..., C:], 2 * C,
              B, nhead, P, L, D, p, seed, o, lse)
        ctx.save_for_backward(q, kv, o, lse)
        ctx.nhead, ctx.p, ctx.seed = nhead, p, seed
        return o

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, do):
        q, kv, o, lse = ctx.saved_tensors
        B, P, C = q.shape
        nhead, L, D = ctx.nhead, kv.size(1), C // ctx.nhead
        do = _aligned(do.to(torch.float32).contiguous())
        (dq, dkv, _, _, _), wanted = _grad_outputs(ctx, q, kv, None, None, None)
        if wanted:
            dk, dv = (None, None) if dkv is None else (dkv[..., :C], dkv[..., C:])
            _call(_seed_entry("paella_attn_train_backward", ctx.seed), q.device, _lib.load().paella_attn_train_workspace_bytes(B, nhead, P, L, D), q, C, kv[..., :C], 2 * C, kv[..., C:], 2 * C,
                  o, lse, do, B, nhead, P, L, D, ctx.p, ctx.seed, dq, C, dk, 2 * C, dv, 2 * C)
        return dq, dkv, None, None, None


def attention_dropout(q, kv, nhead, p=0.0, seed=None):
    """The attention core of an AttnBlock in train mode as one op (nn.MultiheadAttention between its in-projection and its out-projection): per head h, with
    D = C / nhead, qh = q[..., hD:(h+1)D], kh = kv[..., hD:(h+1)D], vh = kv[..., C + hD:C + (h+1)D],
        o[..., hD:(h+1)D] = dropout(softmax(qh kh^T / sqrt(D)), p) vh
    q fp32 [B, P, C]; kv fp32 [B, L, 2C], keys in channels [0, C) and values in [C, 2C) -- what one F.linear(rows, in_proj_weight[C:], in_proj_bias[C:]) produces.
    Returns o [B, P, C], contiguous.  Once differentiable in q and kv; the gradient of kv comes back as one [B, L, 2C] tensor.  Besides q, kv and o autograd keeps
    lse [B, nhead, P] only.  p in [0, 1); p = 0 draws nothing.  The dropout mask is a function of (seed, element index): seed = None with p > 0 draws one 64-bit seed
    from torch's default CPU generator, so torch.manual_seed reproduces a run (refused with RuntimeError while the stream is capturing).  seed may also be a one-element
    int64 tensor on q's device, read by the kernels when they run, as `gelu_grn_dropout` takes it.  D a multiple of 16 in 16...128, B and nhead up to 65535, P and L up to 2^20,
    B nhead P up to 2^31 - 1.  HIP only and exact fp32 only: anything else raises ValueError -- there is no torch fallback."""
    _refuse_non_tensors("attention_dropout", q, kv)
    _refuse_dtypes("attention_dropout", "fp32 q and kv", (q, kv))
    if q.dim() != 3 or kv.dim() != 3 or kv.size(0) != q.size(0) or kv.size(2) != 2 * q.size(2):
        raise ValueError("q must be [B, P, C] and kv [B, L, 2C] (got %s, %s)" % (tuple(q.shape), tuple(kv.shape)))
    B, P, C = q.shape
    L = kv.size(1)
    if isinstance(nhead, bool) or not isinstance(nhead, int) or not 1 <= nhead <= ATTN_MAX_HEADS or C % nhead:
        raise ValueError("nhead = %r: must be an integer in 1...%d that divides C = %d" % (nhead, ATTN_MAX_HEADS, C))
    D = C // nhead
    if D % 16 or not 16 <= D <= 128:
        raise ValueError("head width D = C / nhead = %d: the fused attention takes a multiple of 16 in 16...128" % D)
    if not 1 <= B <= ATTN_MAX_B or not 1 <= P <= ATTN_MAX_P or not 1 <= L <= ATTN_MAX_L or B * nhead * P > ATTN_MAX_ROWS:
        raise ValueError("q %s, kv %s: the fused attention takes 1...%d samples, 1...%d queries and 1...%d keys per sample, B nhead P <= 2^31 - 1"
                         % (tuple(q.shape), tuple(kv.shape), ATTN_MAX_B, ATTN_MAX_P, ATTN_MAX_L))
    p = float(p)
    _refuse_out_of_range("p", p, 0.0 <= p < 1.0, "must lie in [0, 1)")
    _refuse_seed_tensor("attention_dropout", seed)
    _refuse_off_device("attention_dropout", "q and kv", (q, kv))
    seed = _dropout_seed("attention_dropout", seed, p, q.device)
    ATTN_COUNTERS["calls"] += 1
    return _AttentionDropout.apply(_aligned(q.contiguous()), _aligned(kv.contiguous()), nhead, p, seed)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Training seed table: the dropout seeds of one forward as DEVICE words, re-derived by one launch per iteration (paella_amd/csrc/train_seeds.hip,
# include/paella_hip.h "Training seed table").  The two ops above take such a word as `seed=`; a captured iteration (`training.GraphTrainStep`) then draws other
# masks at every replay, because the launch that advances the table is part of the graph.
# ---------------------------------------------------------------------------------------------------------------------------------------------------
SEEDS_MAX_SITES = 65536
_MASK64 = 0xFFFFFFFFFFFFFFFF


def _as_int64(v):
    """the low 64 bits of a Python int as the int64 that holds those bits"""
    v = int(v) & _MASK64
    return v - (1 << 64) if v >> 63 else v


class TrainSeeds:
    """`n_sites` 64-bit seeds on `device`, one per drawing op call of a forward, as one int64 array (base, iteration, word[0 .. n_sites)):
        advance()   ONE launch, no synchronisation, capturable: iteration += 1, word[s] = the first two words of philox4x32(key = base, counter (s, iteration))
        begin()     a forward starts: the next `site()` is word 0
        site()      the next word as a one-element int64 view -- what `gelu_grn_dropout(..., seed=)` / `attention_dropout(..., seed=)` take; raises when the table
                    is too small.  Forward and backward of an op read the same word: nothing may advance the table between them
        values()    the words as Python ints (unsigned), `iteration` / `base` those two entries; they synchronise -- tests and tools
        set_base(seed)          rewrites the base word (the iteration stays)
        snapshot() / restore()  (base, iteration) as a device copy, and back: without synchronising
        grow(n_sites)           a larger table in this same object, base and iteration kept; views handed out by `site()` before it are dead
    seed = None draws the base once from torch's default CPU generator, so torch.manual_seed reproduces a run.  The words are zero until the first advance()."""

    def __init__(self, n_sites, seed=None, device="cuda"):
        if isinstance(n_sites, bool) or not isinstance(n_sites, int) or not 1 <= n_sites <= SEEDS_MAX_SITES:
            raise ValueError("n_sites = %r: a seed table takes 1...%d sites" % (n_sites, SEEDS_MAX_SITES))
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("a seed table lives on the HIP device (got %s)" % device)
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
            raise ValueError("seed = %r: an integer or None" % (seed,))
        if seed is None:
            seed = int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        self.n_sites, self.device = n_sites, torch.device(device.type, torch.cuda.current_device() if device.index is None else device.index)
        host = torch.zeros(2 + n_sites, dtype=torch.int64)
        host[0] = _as_int64(seed)
        self.state = host.to(self.device)
        self._next = 0

    def advance(self):
        lib = _lib.load()
        with torch.cuda.device(self.device):
            _lib.check(lib.paella_train_seeds_advance(self.state.data_ptr(), self.n_sites, _lib.stream_ptr(self.device)))
        return self

    def begin(self):
        self._next = 0
        return self

    def site(self):
        i = self._next
        if i >= self.n_sites:
            raise RuntimeError("the seed table has %d sites and this forward asks for one more: size it with training.dropout_sites(model)" % self.n_sites)
        self._next = i + 1
        return self.state[2 + i:3 + i]

    @property
    def used(self):
        """how many sites were handed out since `begin()`"""
        return self._next

    def values(self):
        return [int(v) & _MASK64 for v in self.state[2:].tolist()]

    @property
    def base(self):
        return int(self.state[0].item()) & _MASK64

    @property
    def iteration(self):
        return int(self.state[1].item()) & _MASK64

    def set_base(self, seed):
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError("seed = %r: an integer" % (seed,))
        self.state[:1].copy_(torch.tensor([_as_int64(seed)], dtype=torch.int64))
        return self

    def snapshot(self):
        return self.state[:2].clone()

    def grow(self, n_sites):
        if isinstance(n_sites, bool) or not isinstance(n_sites, int) or not self.n_sites <= n_sites <= SEEDS_MAX_SITES:
            raise ValueError("n_sites = %r: a seed table of %d sites grows to at most %d" % (n_sites, self.n_sites, SEEDS_MAX_SITES))
        if n_sites > self.n_sites:
            state = torch.zeros(2 + n_sites, dtype=torch.int64, device=self.device)
            state[:2 + self.n_sites].copy_(self.state)
            self.state, self.n_sites, self._next = state, n_sites, 0
        return self

    def restore(self, snap):
        self.state[:2].copy_(snap)
        return self


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Training timestep modulation: the joint between two blocks of a `C T [A]` unit -- the residual add that ends a ResBlock / FeedForwardBlock, the TimestepBlock's
# x (1 + a) + b and the LayerNorm2d that begins an AttnBlock / FeedForwardBlock -- as ONE HIP op, forward and backward (paella_amd/csrc/mod_train.hip,
# include/paella_hip.h "Training timestep modulation").  x and residual are read in place, ab is the mapper's [B, 2C] output as it is and its gradient comes back
# as one [B, 2C] tensor (no chunk), and besides its inputs and z autograd keeps one float per position (rstd): x + residual, x' and 1 + a are recomputed.
# ---------------------------------------------------------------------------------------------------------------------------------------------------
MOD_MAX_B, MOD_MAX_P, MOD_MAX_C, MOD_MAX_POSITIONS = 65535, 1 << 20, 8192, 2 ** 31 - 1
# diagnostic: how often `timestep_modulate` ran, with a residual, with the LayerNorm, and how many of its x / residual arguments were not dense NHWC memory and had
# to be copied (tests, tools/bench_train_modulation.py)
MOD_COUNTERS = {"calls": 0, "residual": 0, "layernorm": 0, "copied": 0}


class _TimestepModulate(torch.autograd.Function):
    """(x [B, H, W, C], residual [B, H, W, C] or None, ab [B, 2C]) -> x' [B, H, W, C], with layernorm (x', z [B, H W, C]); saves x, residual, ab, z and
    rstd [B, H W].  An output nobody used arrives in the backward as None and goes to C as NULL."""

    @staticmethod
    def forward(ctx, x, residual, ab, layernorm, eps):
        B, H, W, C = x.shape
        P = H * W
        xp = torch.empty_like(x)
        z = x.new_empty(B, P, C) if layernorm else None
        rstd = x.new_empty(B, P) if layernorm else None
        _call("paella_mod_ln_train_forward", x.device, 0, x, residual, ab, B, P, C, eps, xp, z, rstd)   # the forward uses no workspace
        ctx.save_for_backward(x, residual, ab, z, rstd)
        ctx.set_materialize_grads(False)
        return (xp, z) if layernorm else xp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dxp, dz=None):
        x, residual, ab, z, rstd = ctx.saved_tensors
        B, H, W, C = x.shape
        P = H * W
        need_x, need_res, need_ab = ctx.needs_input_grad[:3]
        if (dxp is None and dz is None) or not (need_x or need_res or need_ab):
            return None, None, None, None, None
        dxp, dz = (None if g is None else _aligned(g.to(torch.float32).contiguous()) for g in (dxp, dz))
        dx = torch.empty_like(x) if need_x or need_res else None      # ONE tensor: the gradients of x and of residual are the same values
        dab = torch.empty_like(ab) if need_ab else None
        _call("paella_mod_ln_train_backward", x.device, _lib.load().paella_mod_ln_train_workspace_bytes(B, P, C, int(dz is not None)), x, residual, ab,
              None if dz is None else z, None if dz is None else rstd, dxp, dz, B, P, C, dx, dab)
        return dx if need_x else None, dx if need_res else None, dab, None, None


def timestep_modulate(x, ab, residual=None, layernorm=False, eps=1e-6):
    """The joint between two blocks of a `C T [A]` unit in train mode as one op (src/modules.py:62 / 96, 99-106, 22-27): with a = ab[:, :C], b = ab[:, C:],
        x' = (x + residual) * (1 + a[:, :, None, None]) + b[:, :, None, None]                 and, with layernorm,
        z  = layer_norm(x'.permute(0, 2, 3, 1), (C,), eps=eps).reshape(B, H * W, C)
    x and residual fp32 with logical shape [B, C, H, W] and any strides: memory that is already dense NHWC and 16-byte aligned is used in place, anything else is
    copied once.  ab fp32 [B, 2C]: the TimestepBlock mapper's F.linear output as it is.  Returns x' with logical shape [B, C, H, W] over NHWC memory; with
    layernorm (x', z), z contiguous [B, H W, C] -- what `_attn_block` and `_channelwise` consume.  Once differentiable in x, residual and ab: the gradients of x
    and residual are one tensor (logical [B, C, H, W] over NHWC memory), the gradient of ab comes back as one [B, 2C] tensor.  Besides its inputs and z autograd
    keeps one float per position; x + residual, x' and 1 + a are recomputed, and the backward never divides by 1 + a.  C a multiple of 4 in 4...8192, 1...2^20
    positions per sample, B up to 65535, B H W up to 2^31 - 1.  HIP only and exact fp32 only: anything else raises ValueError -- there is no torch fallback."""
    _refuse_non_tensors("timestep_modulate", x, ab, *(() if residual is None else (residual,)))
    _refuse_dtypes("timestep_modulate", "fp32 x, ab and residual", (x, ab, residual))
    if x.dim() != 4:
        raise ValueError("x must be [B, C, H, W] (got %s)" % (tuple(x.shape),))
    B, C, H, W = x.shape
    if residual is not None and tuple(residual.shape) != tuple(x.shape):
        raise ValueError("residual must have the shape of x, %s (got %s)" % (tuple(x.shape), tuple(residual.shape)))
    if tuple(ab.shape) != (B, 2 * C):
        raise ValueError("ab must be [B, 2C] = [%d, %d] (got %s)" % (B, 2 * C, tuple(ab.shape)))
    if C % 4 or not 4 <= C <= MOD_MAX_C:
        raise ValueError("C = %d: the fused timestep modulation takes a multiple of 4 in 4...%d" % (C, MOD_MAX_C))
    if not 1 <= B <= MOD_MAX_B or not 1 <= H * W <= MOD_MAX_P or B * H * W > MOD_MAX_POSITIONS:
        raise ValueError("x %s: the fused timestep modulation takes 1...%d samples of 1...%d positions, B H W <= 2^31 - 1" % (tuple(x.shape), MOD_MAX_B, MOD_MAX_P))
    eps = float(eps)
    _refuse_out_of_range("eps", eps, 0.0 < eps < 1e30, "must be positive and finite")
    _refuse_off_device("timestep_modulate", "x, ab and residual", (x, ab, residual))
    layernorm = bool(layernorm)
    MOD_COUNTERS["calls"] += 1
    MOD_COUNTERS["residual"] += int(residual is not None)
    MOD_COUNTERS["layernorm"] += int(layernorm)
    out = _TimestepModulate.apply(_nhwc(x, MOD_COUNTERS), None if residual is None else _nhwc(residual, MOD_COUNTERS), _aligned(ab.contiguous()), layernorm, eps)
    return (out[0].permute(0, 3, 1, 2), out[1]) if layernorm else out.permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Training linear on bf16 operands: y = x W^T + b with the forward, dgrad and wgrad GEMMs on the bf16 matrix cores and fp32 accumulation
# (paella_amd/csrc/linear_train.hip, include/paella_hip.h "Training linear on bf16 operands").  OPT-IN and outside the fp32 parity contract
# (Paella.set_training_gemm("bf16")).  x, the weight, the bias, y and every gradient stay fp32 in memory: the op rounds the GEMM operands into its workspace, in
# one pass per tensor, and autograd keeps x and the weight as they are -- what F.linear keeps.
# ---------------------------------------------------------------------------------------------------------------------------------------------------
LINEAR_GRAIN, LINEAR_MAX_DIM = 64, 65535 * 64
# diagnostic: how often `linear_bf16` ran, how many backward calls reached the library, how many sites of the network fell back to F.linear because
# `linear_shapes_ok` does not hold there, and how many inputs / gradients were not dense and had to be copied (tests, tools/bench_train_linear.py)
LINEAR_COUNTERS = {"calls": 0, "backward": 0, "fallbacks": 0, "copied": 0}
_WANT_DX, _WANT_DW, _WANT_DB = 1, 2, 4


def linear_shapes_ok(M, N, K):
    """the shapes `linear_bf16` takes: M rows, N output and K input features, each a positive multiple of 64 up to 65535 x 64 (the extent of the pack's grid) -- each of them is the reduction of one
    of the three GEMMs (K forward, N dgrad, M wgrad), and the bf16 kernels step 64 elements of it at a time"""
    return all(isinstance(v, int) and LINEAR_GRAIN <= v <= LINEAR_MAX_DIM and v % LINEAR_GRAIN == 0 for v in (M, N, K))


def _dense(t):
    """t itself when it is dense row-major memory on the 16-byte grain, else one copy (counted in LINEAR_COUNTERS["copied"])"""
    if t.is_contiguous() and t.data_ptr() % 16 == 0:
        return t
    LINEAR_COUNTERS["copied"] += 1
    return t.contiguous() if not t.is_contiguous() else t.clone()


class _LinearBf16(torch.autograd.Function):
    """(x [M, K], weight [N, K], bias [N] or None) -> y [M, N]; saves x and weight, fp32 as they are."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        M, K = x.shape
        N = weight.size(0)
        y = x.new_empty(M, N)
        _call("paella_linear_train_forward", x.device, _lib.load().paella_linear_train_workspace_bytes(M, N, K, 0, 0), x, weight, bias, y, M, N, K)
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        M, K = x.shape
        N = weight.size(0)
        (dx, dw, db), wanted = _grad_outputs(ctx, x, weight, (N,))
        if not wanted:
            return None, None, None
        dy = _dense(dy.to(torch.float32))
        wants = (_WANT_DX if dx is not None else 0) | (_WANT_DW if dw is not None else 0) | (_WANT_DB if db is not None else 0)
        LINEAR_COUNTERS["backward"] += 1
        _call("paella_linear_train_backward", x.device, _lib.load().paella_linear_train_workspace_bytes(M, N, K, 1, wants), x, weight, dy, dx, dw, db, M, N, K)
        return dx, dw, db


def linear_bf16(x, weight, bias=None):
    """F.linear(x, weight, bias) in train mode with its three GEMMs on the bf16 matrix cores:
        y  = bf16(x) bf16(weight)^T + bias                                   (fp32 accumulation; y fp32)
        dx = bf16(dy) bf16(weight),   dweight = bf16(dy)^T bf16(x),   dbias = dy.sum(0) of the unrounded dy, carried in fp64
    x fp32 [..., K], flattened to M rows; weight fp32 [N, K]; bias fp32 [N] or None.  Returns y [..., N], contiguous.  Once differentiable in x, weight and bias; a
    gradient autograd does not want is neither packed for nor computed.  Autograd keeps x and weight as they are, fp32 -- what F.linear keeps; the backward rounds
    them again.  bf16(.) is round to nearest even, the bits of torch's .bfloat16().  OUTSIDE the fp32 parity contract: a result differs from F.linear's by the
    rounding of the operands (relative 2^-9 per operand element).  Parameters, gradients and every tensor in memory stay fp32.  M, N and K multiples of 64 up to
    65535 x 64 (`linear_shapes_ok`); an x or an arriving gradient that is not dense is copied once (counted).  HIP only: anything else raises ValueError -- there is no torch
    fallback."""
    tensors = (x, weight) if bias is None else (x, weight, bias)
    _refuse_non_tensors("linear_bf16", *tensors)
    _refuse_dtypes("linear_bf16", "fp32 x, weight and bias", (x, weight, bias))
    if weight.dim() != 2 or x.dim() < 1 or x.size(-1) != weight.size(1):
        raise ValueError("weight must be [N, K] with K = x.size(-1) (got x %s, weight %s)" % (tuple(x.shape), tuple(weight.shape)))
    N, K = weight.shape
    if bias is not None and tuple(bias.shape) != (N,):
        raise ValueError("bias must be [N] = [%d] (got %s)" % (N, tuple(bias.shape)))
    M = x.numel() // K if K else 0
    for name, v in (("M", M), ("N", N), ("K", K)):
        if not linear_shapes_ok(v, LINEAR_GRAIN, LINEAR_GRAIN):
            raise ValueError("%s = %d (x %s, weight %s): the bf16 linear takes a multiple of %d in %d...%d"
                             % (name, v, tuple(x.shape), tuple(weight.shape), LINEAR_GRAIN, LINEAR_GRAIN, LINEAR_MAX_DIM))
    _refuse_off_device("linear_bf16", "x, weight and bias", (x, weight, bias))
    LINEAR_COUNTERS["calls"] += 1
    y = _LinearBf16.apply(_dense(x).view(M, K), _dense(weight), None if bias is None else _dense(bias))
    return y.view(x.shape[:-1] + (N,))


def pack_bf16(x, transposed=False, colsum=False):
    """The pass that makes `linear_bf16`'s operands, alone: x fp32 [rows, cols] on a cuda device, rows and cols multiples of 64, read once.  Returns
    (x.bfloat16() [rows, cols][, x.t().contiguous().bfloat16() [cols, rows] with transposed][, x.sum(0) fp32 [cols] with colsum, carried in fp64]); the bf16 tensors
    have the bits of torch's conversion (`.view(torch.int16)` compares them).  HIP only: anything else raises ValueError."""
    _refuse_non_tensors("pack_bf16", x)
    _refuse_dtypes("pack_bf16", "fp32 x", (x,))
    if x.dim() != 2 or not linear_shapes_ok(x.size(0), x.size(1), LINEAR_GRAIN):
        raise ValueError("x %s: the pack takes [rows, cols], both multiples of %d in %d...%d" % (tuple(x.shape), LINEAR_GRAIN, LINEAR_GRAIN, LINEAR_MAX_DIM))
    _refuse_off_device("pack_bf16", "x", (x,))
    rows, cols = x.shape
    x = _aligned(x.contiguous())
    row = torch.empty(rows, cols, dtype=torch.bfloat16, device=x.device)
    tr = torch.empty(cols, rows, dtype=torch.bfloat16, device=x.device) if transposed else None
    cs = x.new_empty(cols) if colsum else None
    # the partials of the column sums: one double per (strip, column), at most one strip per row tile
    _call("paella_pack_bf16", x.device, 256 + (rows // LINEAR_GRAIN) * cols * 8 if colsum else 0, x, rows, cols, row, tr, cs)
    return (row,) + (() if tr is None else (tr,)) + (() if cs is None else (cs,))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Training token stem: F.embedding -> layer_norm -> pixel_unshuffle -> NHWC rows at the top of the network as ONE HIP op, forward and backward
# (paella_amd/csrc/embed_train.hip, include/paella_hip.h "Training token stem").  The forward is the eval engine's launch; the backward writes the table's whole
# gradient in one launch without atomics, sorts or library calls -- which is what lets a captured iteration hold it.  Autograd keeps the tokens and the reference
# to the table and NOTHING per token: the statistics of a table row are recomputed once per label in the backward (saving two floats per token would buy nothing,
# since the LayerNorm backward runs per label and not per token).
# ---------------------------------------------------------------------------------------------------------------------------------------------------
EMBED_MAX_C, EMBED_MAX_LABELS, EMBED_MAX_POSITIONS = 1024, 65536, 2 ** 31 - 1
# diagnostic: how often `token_embed_layernorm` ran and how many backward calls reached the library (tests, tools/bench_train_embedding.py)
EMBED_COUNTERS = {"calls": 0, "backward": 0}


class _TokenEmbedLayerNorm(torch.autograd.Function):
    """(x int64 [B, H, W], weight [num_labels, c_in]) -> rows [B, H/p, W/p, c_in p^2]; saves x and weight."""

    @staticmethod
    def forward(ctx, x, weight, patch, eps):
        B, H, W = x.shape
        L, C = weight.shape
        rows = weight.new_empty(B, H // patch, W // patch, C * patch * patch)
        _call("paella_embed_ln_train_forward", weight.device, _lib.load().paella_embed_ln_train_workspace_bytes(B, H, W, C, patch, L), x, weight, B, H, W, C, patch, L, eps, rows)
        ctx.save_for_backward(x, weight)
        ctx.patch, ctx.eps = patch, eps
        return rows

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_rows):
        x, weight = ctx.saved_tensors
        B, H, W = x.shape
        L, C = weight.shape
        (_, dw, _, _), wanted = _grad_outputs(ctx, None, weight, None, None)
        if wanted:
            d_rows = _aligned(d_rows.to(torch.float32).contiguous())
            EMBED_COUNTERS["backward"] += 1
            _call("paella_embed_ln_train_backward", weight.device, _lib.load().paella_embed_ln_train_workspace_bytes(B, H, W, C, ctx.patch, L), x, weight, d_rows,
                  B, H, W, C, ctx.patch, L, ctx.eps, dw)
        return None, dw, None, None


def token_embed_layernorm(x, weight, patch=1, eps=1e-6):
    """The token stem of the network in train mode as one op (src/modules.py:126-131, 271): the rows
        rows[b, oy, ox, c p^2 + dy p + dx] = layer_norm(weight[x[b, oy p + dy, ox p + dx]], (c_in,), eps=eps)[c],        p = patch
    i.e. F.pixel_unshuffle(F.layer_norm(F.embedding(x, weight), (c_in,), eps=eps).permute(0, 3, 1, 2), p) in NHWC memory -- the A operand of the 1x1 convolution
    behind it as a linear.  x int64 [B, H, W], H and W multiples of patch, patch 1 or 2; weight fp32 [num_labels, c_in], `in_mapper.0.weight` used in place.  Returns
    rows fp32 [B, H/p, W/p, c_in p^2], contiguous, bit for bit what the inference engine's stem launch gives.  Once differentiable in weight (x has no gradient):
    the gradient is WRITTEN whole by the op, exact zeros in the rows of labels that do not occur, summed in ascending position order without atomics -- its bits depend on
    (x, weight, the arriving gradient, the shape) alone.  Autograd keeps x and the reference to weight, nothing the size of the activations.  A token outside
    [0, num_labels) is clamped into it in both directions, as the inference kernel clamps it.  c_in a multiple of 4 in 4...1024, num_labels in 1...65536, at most
    2^31 - 1 output positions.  HIP only and exact fp32 only: anything else raises ValueError -- there is no torch fallback."""
    _refuse_non_tensors("token_embed_layernorm", x, weight)
    _refuse_dtypes("token_embed_layernorm", "int64 x and fp32 weight", (x, weight), (torch.int64, torch.float32))
    _refuse_out_of_range("patch", patch, not isinstance(patch, bool) and isinstance(patch, int) and patch in (1, 2), "the fused token stem takes patch 1 or 2")
    if x.dim() != 3 or weight.dim() != 2:
        raise ValueError("x must be [B, H, W] and weight [num_labels, c_in] (got %s, %s)" % (tuple(x.shape), tuple(weight.shape)))
    B, H, W = x.shape
    L, C = weight.shape
    if C % 4 or not 4 <= C <= EMBED_MAX_C:
        raise ValueError("c_in = %d: the fused token stem takes a multiple of 4 in 4...%d" % (C, EMBED_MAX_C))
    if not 1 <= L <= EMBED_MAX_LABELS:
        raise ValueError("num_labels = %d: the fused token stem takes 1...%d" % (L, EMBED_MAX_LABELS))
    if B < 1 or H < 1 or W < 1 or H % patch or W % patch or B * (H // patch) * (W // patch) > EMBED_MAX_POSITIONS:
        raise ValueError("x %s: the fused token stem takes H and W multiples of patch = %d and 1...2^31 - 1 output positions" % (tuple(x.shape), patch))
    eps = float(eps)
    _refuse_out_of_range("eps", eps, 0.0 < eps < 1e30, "must be positive and finite")
    _refuse_off_device("token_embed_layernorm", "x and weight", (x, weight))
    EMBED_COUNTERS["calls"] += 1
    return _TokenEmbedLayerNorm.apply(_aligned(x.contiguous()), _aligned(weight.contiguous()), patch, eps)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Training optimizer step: clip_grad_norm_ + AdamW of every parameter as THREE launches over a device table of tensors (paella_amd/csrc/optim.hip,
# include/paella_hip.h "Training optimizer step"): the gradients are read once for the norm, then p, g, m, v are read once and p, m, v written once.  The gradients
# are never rewritten and nothing the size of the parameters is allocated.
# ---------------------------------------------------------------------------------------------------------------------------------------------------
# one row of the table = include/paella_hip.h: paella_adamw_tensor = _lib.AdamwTensor (88 bytes, every field 8 wide)
ADAMW_ROW = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("chunk_begin", "<i8"),
                      ("lr", "<f8"), ("beta1", "<f8"), ("beta2", "<f8"), ("eps", "<f8"), ("weight_decay", "<f8")])
# diagnostic: how often `ClippedAdamW.step` ran and how often it had to wait for a staging buffer's earlier upload (tests, tools/bench_train_optimizer.py)
ADAMW_COUNTERS = {"steps": 0, "staging_waits": 0}
# what torch.optim.AdamW keeps in a parameter group besides lr, betas, eps and weight_decay, at the only values this optimizer has: a state dict of either class
# then loads into the other
_ADAMW_TORCH_KEYS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)


def adamw_chunk_plan(counts, chunk):
    """element counts of the tensors, in order (0 for a tensor without elements or without a gradient) -> (the index of each tensor's first chunk, the number of
    chunks): a tensor owns ceil(count / chunk) consecutive chunks of `chunk` elements, the last one possibly short"""
    begins, c = [], 0
    for n in counts:
        if n < 0:
            raise ValueError("a tensor of %d elements" % n)
        begins.append(c)
        c += -(-n // chunk)
    return begins, c


def _refuse_adamw_hyper(lr, betas, eps, weight_decay):
    """torch.optim.AdamW's ranges"""
    _refuse_out_of_range("lr", lr, isinstance(lr, (int, float)) and 0.0 <= lr, "must be a non-negative number (a tensor lr is not taken)")
    _refuse_out_of_range("eps", eps, isinstance(eps, (int, float)) and 0.0 <= eps, "must be a non-negative number")
    ok = isinstance(betas, (tuple, list)) and len(betas) == 2 and all(isinstance(b, (int, float)) for b in betas)
    _refuse_out_of_range("betas", betas, ok and 0.0 <= betas[0] < 1.0, "betas[0] must lie in [0, 1)")
    _refuse_out_of_range("betas", betas, 0.0 <= betas[1] < 1.0, "betas[1] must lie in [0, 1)")
    _refuse_out_of_range("weight_decay", weight_decay, isinstance(weight_decay, (int, float)) and 0.0 <= weight_decay, "must be a non-negative number")


def _dense_fp32_grad(g, dev):
    """the gradient as the kernels read it: dense fp32 on dev -- itself, or a temporary copy / cast"""
    if g.is_sparse or g.layout != torch.strided:
        raise ValueError("sparse gradients are not taken (got layout %s)" % g.layout)
    if g.dtype != torch.float32 or g.device != dev:
        g = g.to(device=dev, dtype=torch.float32)
    return g if g.is_contiguous() else g.contiguous()


class ClippedAdamW(torch.optim.Optimizer):
    """`nn.utils.clip_grad_norm_(params, max_norm); torch.optim.AdamW(params, ...).step()` as one HIP op of three launches (the reference's update,
    src/train.py:66-69), for fp32 parameters on one cuda device:
        norm = ||all gradients||_2 (summed in fp64);  coef = min(1, max_norm / (norm + 1e-6));  g' = g coef
        p *= 1 - lr wd;  m += (g' - m)(1 - beta1);  v = v beta2 + (1 - beta2) g' g';  p -= lr / (1 - beta1^step) m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
    Parameter groups are honoured: lr, betas, eps and weight_decay per group, lr read from `param_groups` at every step (schedulers work as with torch's class).
    max_norm is one value for the optimizer and the norm is global over every parameter that has a gradient; max_norm = None: no clipping -- the norm is still
    computed.  After `step()`, `opt.grad_norm` is a 0-dim device tensor with the norm BEFORE clipping: what clip_grad_norm_ returns.
    Two differences from the torch pair, both on purpose:
      * the gradients are left UNCLIPPED: g' exists in registers only (p.grad after the step is what backward() wrote);
      * a step whose norm is not finite (an inf or NaN gradient anywhere) is SKIPPED on the device: p, exp_avg, exp_avg_sq and step stay bit for bit, where torch
        would write NaN into every weight.  `opt.grad_norm` is then inf or NaN, which is how a loop learns of it.
    The state is torch AdamW's: state[p] = {"step", "exp_avg", "exp_avg_sq"}, created at a parameter's first gradient; "step" is a 0-dim float32 view into one flat
    device array.  `state_dict()` loads into torch.optim.AdamW and a torch.optim.AdamW state dict (CPU "step" tensors included) loads into this class.
    `step()` does not synchronise with the device: the table goes up from one of two pinned staging buffers, each guarded by an event, on the current stream; every
    updated parameter's version is raised, which is what `Paella._signature` and hence the HIP engine and captured graphs notice.  Call it on ONE stream.
    HIP only: amsgrad, maximize, foreach= / fused=, non-fp32 or non-contiguous parameters, parameters off the one cuda device, sparse gradients and hyperparameters
    outside torch's ranges raise ValueError -- there is no torch fallback.  A non-contiguous or non-fp32 gradient is copied / cast to a dense fp32 temporary."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=1.0, **unsupported):
        for k, v in unsupported.items():
            if k not in ("amsgrad", "maximize", "foreach", "fused", "capturable", "differentiable"):
                raise TypeError("ClippedAdamW() got an unexpected keyword argument %r" % k)
            if k in ("foreach", "fused") or v:
                raise ValueError("ClippedAdamW is one HIP implementation: %s=%r is not taken (amsgrad, maximize, capturable and differentiable are not implemented, "
                                 "foreach / fused select torch implementations)" % (k, v))
        _refuse_adamw_hyper(lr, betas, eps, weight_decay)
        if max_norm is not None:
            _refuse_out_of_range("max_norm", max_norm, isinstance(max_norm, (int, float)) and 0.0 < max_norm < float("inf"), "must be positive and finite, or None")
        self.max_norm = max_norm
        self.grad_norm = None
        self._device = None
        self._steps = None              # flat float32 [number of parameters]: state[p]["step"] is a view of its element
        self._index = {}                # parameter -> its row
        self._rows_dev = self._ws = None
        self._staging, self._events, self._turn = [None, None], [None, None], 0
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, **_ADAMW_TORCH_KEYS))

    def add_param_group(self, param_group):
        g = dict(getattr(self, "defaults", {}), **{k: v for k, v in param_group.items() if k != "params"})
        _refuse_adamw_hyper(g["lr"], g["betas"], g["eps"], g["weight_decay"])
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("ClippedAdamW does not implement amsgrad or maximize")
        ps = param_group["params"]
        ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
        param_group = dict(param_group, params=ps)
        _refuse_non_tensors("ClippedAdamW", *ps)
        _refuse_dtypes("ClippedAdamW", "fp32 parameters", ps)
        dev = self._device
        for p in ps:
            if not p.is_cuda or (dev is not None and p.device != dev):
                raise ValueError("ClippedAdamW runs on the HIP device only: every parameter must live on the same cuda device (got %s%s)"
                                 % (p.device, "" if dev is None else " after %s" % dev))
            dev = p.device
            if not p.is_contiguous():
                raise ValueError("ClippedAdamW takes contiguous parameters (got shape %s with strides %s)" % (tuple(p.shape), tuple(p.stride())))
        super().add_param_group(param_group)
        self._device = dev

    # -- the flat step array ------------------------------------------------------------------------------------------------------------------------
    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _layout(self):
        """the parameters in group order with their rows; grows the flat step array (and moves the views) when a group was added"""
        ps = self._params()
        if self._steps is None or self._steps.numel() != len(ps) or any(self._index.get(p) != i for i, p in enumerate(ps)):
            old, old_index = self._steps, self._index
            self._steps = torch.zeros(len(ps), dtype=torch.float32, device=self._device)
            self._index = {p: i for i, p in enumerate(ps)}
            for p, i in self._index.items():
                if p in self.state and "step" in self.state[p]:
                    if old is not None and p in old_index:
                        self._steps[i].copy_(old[old_index[p]])
                    self.state[p]["step"] = self._steps[i]
        return ps

    def state_dict(self):
        """torch's layout; every "step" is a copy (0-dim float32 on the device), never a view of the flat array: an optimizer that loads it shares nothing with this one"""
        sd = super().state_dict()
        sd["state"] = {k: dict(st, step=st["step"].clone()) if torch.is_tensor(st.get("step")) else st for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """takes a ClippedAdamW or a torch.optim.AdamW state dict (its "step" a CPU or device tensor of any float dtype, or a number) and re-packs the steps into
        the flat device array; exp_avg / exp_avg_sq are made dense fp32 on the parameters' device"""
        for g in state_dict["param_groups"]:
            if g.get("amsgrad") or g.get("maximize"):
                raise ValueError("ClippedAdamW does not implement amsgrad or maximize: this state dict was written with one of them")
            _refuse_adamw_hyper(g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"])
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            g["betas"] = tuple(g["betas"])
            for k, v in _ADAMW_TORCH_KEYS.items():
                g[k] = v
        self._steps, self._index = None, {}
        loaded = {p: st.pop("step") for p, st in self.state.items() if "step" in st}
        self._layout()
        values = torch.zeros(self._steps.numel(), dtype=torch.float32)
        on_device = []
        for p, s in loaded.items():
            i = self._index[p]
            if torch.is_tensor(s) and s.is_cuda:
                on_device.append((i, s))
            else:
                values[i] = float(s)
        self._steps.copy_(values)
        for i, s in on_device:
            self._steps[i].copy_(s.detach().to(torch.float32).reshape(()))
        for p, st in self.state.items():
            st["step"] = self._steps[self._index[p]]
            for k in ("exp_avg", "exp_avg_sq"):
                st[k] = _aligned(st[k].detach().to(device=p.device, dtype=torch.float32).contiguous())

    # -- the step -----------------------------------------------------------------------------------------------------------------------------------
    def _stage(self, rows):
        """rows (numpy, ADAMW_ROW) -> the device table.  A staging buffer is rewritten only after the upload that last read it has finished: two buffers, used in
        turn, each with the event recorded behind its upload -- waiting for it is waiting for the step before the previous one"""
        nbytes = rows.nbytes
        t = self._turn = self._turn ^ 1
        if self._events[t] is not None and not self._events[t].query():
            ADAMW_COUNTERS["staging_waits"] += 1
            self._events[t].synchronize()
        if self._staging[t] is None or self._staging[t].numel() < nbytes:
            self._staging[t] = torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=True)
        self._reserve(nbytes, 0)
        self._staging[t].numpy()[:nbytes] = rows.view(np.uint8).reshape(-1)
        self._rows_dev[:nbytes].copy_(self._staging[t][:nbytes], non_blocking=True)
        if self._events[t] is None:
            self._events[t] = torch.cuda.Event()
        self._events[t].record()
        return self._rows_dev

    def materialize_state(self):
        """state[p] = {"step", "exp_avg", "exp_avg_sq"} for every parameter that requires a gradient, now instead of at its first gradient -- the zeros lazy creation
        makes -- plus the device table and the workspace at the size a step over all of them needs.  After it a step allocates nothing but its norm: what a stream
        capture of the launch part needs (`training.GraphTrainStep`).  A parameter that never gets a gradient keeps its row with count 0, as without this call."""
        lib = _lib.load()
        ps = self._layout()
        dev = self._device
        if not ps:
            return self
        with torch.cuda.device(dev):
            for p in ps:
                if not p.requires_grad:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = self._steps[self._index[p]]
                    st["exp_avg"] = torch.zeros(p.shape, dtype=torch.float32, device=dev)
                    st["exp_avg_sq"] = torch.zeros(p.shape, dtype=torch.float32, device=dev)
            _, n_chunks = adamw_chunk_plan([p.numel() for p in ps], lib.paella_adamw_chunk_elems())
            self._reserve(len(ps) * ADAMW_ROW.itemsize, lib.paella_adamw_workspace_bytes(len(ps), n_chunks))
        return self

    def _reserve(self, table_bytes, ws_bytes):
        """the device table and the workspace, grown when a step needs more (never shrunk: their addresses stay while the parameter set does)"""
        if self._rows_dev is None or self._rows_dev.numel() < table_bytes:
            self._rows_dev = torch.empty(max(table_bytes, 1), dtype=torch.uint8, device=self._device)
        if self._ws is None or self._ws.numel() < ws_bytes:
            self._ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self._device)

    # `step()` in three parts.  Only the LAUNCH part puts work on the stream that a capture may hold: the upload goes through a pinned staging copy guarded by
    # event.query() / synchronize() and never sits inside one.  The PLAN is host code -- it reads addresses and `param_groups` -- and enqueues nothing ONCE the state
    # is materialised and every gradient is dense fp32 on the device: then it may run while a stream is capturing, which a captured iteration needs, because the
    # gradients whose addresses it reads are made by the captured backward.  Otherwise it allocates (first-gradient state, a temporary for a gradient that is not dense
    # fp32): `GraphTrainStep` materialises the state before it captures and refuses a plan that kept a temporary.  The hyperparameter values a plan made at capture
    # time holds are stale by the first replay: before every replay the iteration refreshes those columns (`_plan_hyper`) and uploads eagerly on the same stream --
    # which is how a scheduler's `lr` reaches a captured step.
    def _plan_hyper(self, rows):
        """the hyperparameter columns of the host rows from `param_groups` as they are NOW"""
        hyper = []
        for group in self.param_groups:
            lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            _refuse_adamw_hyper(lr, (b1, b2), eps, wd)
            hyper.extend([(lr, b1, b2, eps, wd)] * len(group["params"]))
        hyper = np.array(hyper, dtype=np.float64).reshape(len(rows), 5)
        for j, k in enumerate(("lr", "beta1", "beta2", "eps", "weight_decay")):
            rows[k] = hyper[:, j]
        return rows

    def _plan(self):
        """part 1, host only apart from a temporary for a gradient that is not dense fp32 and the state of a parameter's first gradient: -> dict(rows = the host table
        (numpy, ADAMW_ROW), n, n_chunks, keep = temporaries that must outlive the launch, updated = the parameters the step will write); sizes table and workspace"""
        lib = _lib.load()
        ps = self._layout()
        dev = self._device
        chunk = lib.paella_adamw_chunk_elems()
        rows = np.zeros(len(ps), dtype=ADAMW_ROW)
        cols = {k: [] for k in ("p", "g", "m", "v", "n")}     # by column: one numpy assignment each
        counts, keep, updated = [], [], []                    # keep: the temporaries stay alive until the call is enqueued
        with torch.cuda.device(dev):
            for group in self.param_groups:
                _refuse_adamw_hyper(group["lr"], group["betas"], group["eps"], group["weight_decay"])   # per group, before its state is created: the order step() always had
                for p in group["params"]:
                    n = p.numel()
                    cols["n"].append(n)
                    if p.grad is None:
                        counts.append(0)
                        for k in "pgmv":
                            cols[k].append(0)
                        continue
                    g = _dense_fp32_grad(p.grad, dev)
                    keep.append(g)
                    st = self.state[p]
                    if not st:
                        st["step"] = self._steps[self._index[p]]
                        st["exp_avg"] = torch.zeros(p.shape, dtype=torch.float32, device=dev)
                        st["exp_avg_sq"] = torch.zeros(p.shape, dtype=torch.float32, device=dev)
                    cols["p"].append(p.data_ptr())
                    cols["g"].append(g.data_ptr())
                    cols["m"].append(st["exp_avg"].data_ptr())
                    cols["v"].append(st["exp_avg_sq"].data_ptr())
                    counts.append(n)
                    updated.append(p)
            for k, col in cols.items():
                rows[k] = col
            self._plan_hyper(rows)
            begins, n_chunks = adamw_chunk_plan(counts, chunk)
            rows["chunk_begin"] = begins
            self._reserve(rows.nbytes, lib.paella_adamw_workspace_bytes(len(ps), n_chunks))
        return dict(rows=rows, n=len(ps), n_chunks=n_chunks, keep=keep, updated=updated)

    def _upload(self, plan):
        """part 2: the host rows -> the device table, through a pinned staging buffer on the current stream.  Never inside a capture."""
        with torch.cuda.device(self._device):
            return self._stage(plan["rows"])

    def _launch(self, plan):
        """part 3: the three launches of paella_adamw_step over the device table at its fixed address; -> the norm (0-dim, made here).  Capturable."""
        dev = self._device
        with torch.cuda.device(dev):
            norm = torch.empty((), dtype=torch.float32, device=dev)
            _lib.check(_lib.load().paella_adamw_step(self._rows_dev.data_ptr(), plan["n"], plan["n_chunks"], 0.0 if self.max_norm is None else float(self.max_norm),
                                                     self._steps.data_ptr(), norm.data_ptr(), self._ws.data_ptr(), self._ws.numel(), _lib.stream_ptr(dev)))
        return norm

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not self._params():
            return loss
        plan = self._plan()
        self._upload(plan)
        self.grad_norm = self._launch(plan)
        if plan["updated"]:
            torch.autograd.graph.increment_version(plan["updated"])   # the kernels wrote through raw pointers: this is what Paella._signature sees
        ADAMW_COUNTERS["steps"] += 1
        return loss


def grad_norm(parameters):
    """The 2-norm of all gradients of `parameters` (a tensor or an iterable; those without a gradient are left out) as a 0-dim fp32 device tensor, summed in fp64
    in a fixed order: what `nn.utils.clip_grad_norm_` returns, without clipping anything.  HIP only: the gradients live on one cuda device; non-fp32 or
    non-contiguous ones are cast / copied to a dense fp32 temporary, sparse ones raise ValueError."""
    ps = [parameters] if isinstance(parameters, torch.Tensor) else list(parameters)
    _refuse_non_tensors("grad_norm", *ps)
    grads = [p.grad for p in ps if p.grad is not None]
    if not grads:
        raise ValueError("grad_norm: no parameter has a gradient")
    _refuse_off_device("grad_norm", "the gradients", grads)
    dev = grads[0].device
    lib = _lib.load()
    with torch.no_grad():
        grads = [_dense_fp32_grad(g, dev) for g in grads]
        rows = np.zeros(len(grads), dtype=ADAMW_ROW)
        rows["g"] = [g.data_ptr() for g in grads]
        rows["n"] = [g.numel() for g in grads]
        rows["chunk_begin"], n_chunks = adamw_chunk_plan([g.numel() for g in grads], lib.paella_adamw_chunk_elems())
        table = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(dev)
        norm = torch.empty((), dtype=torch.float32, device=dev)
        _call("paella_adamw_grad_norm", dev, lib.paella_adamw_workspace_bytes(len(grads), n_chunks), table, len(grads), n_chunks, norm)
    return norm

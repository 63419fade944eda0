"""GPU: the training attention op (paella_amd/csrc/attn_train.hip) against the fp64 model of tests/attn_train_model.py.

The yardstick of every accuracy check is MEASURED in the same test, as tests/test_gpu_grn_act.py does: the torch fp32 chain (scores -> softmax -> times the SAME dropout
mask -> @ v, autograd's backward) runs on the same device and inputs, its max abs error against the fp64 model is taken for each of o, dq, dk and dv, and the fused
op must stay within 4x max(that error, one fp32 ulp at the largest reference magnitude) -- the ulp floor is the rounding no fp32 result can avoid.  The measured pairs
are kept in profiles/train_attention_parity.txt."""
import functools
import math

import numpy as np
import pytest
import torch

from paella_amd import _lib, training
from tests import attn_train_model as M
from tests import train_op_checks as T
from tests.test_gpu_training import _train_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (B, nhead, P, L, D): one score; tails in both tile axes with L off the quad grain; the tiny network's level; keys independent of P over several key tiles; one past
# a tile both ways at the released head width; the 570M level-1 geometry; the widest head with few queries against many key tiles
SHAPES = [(1, 1, 1, 1, 16), (2, 2, 7, 9, 16), (1, 4, 64, 68, 16), (2, 2, 33, 100, 32), (1, 2, 65, 131, 80), (2, 16, 64, 84, 80), (1, 1, 16, 1040, 128)]
FACTOR = T.FACTOR
_err, _ulp = T.err, T.ulp
SEED = (0xC0FFEE << 40) + 977   # high key word in use
ids = lambda s: "x".join(map(str, s))
U = 2.0 ** -24                  # the unit roundoff of fp32


@functools.lru_cache(maxsize=None)
def _inputs(B, nhead, P, L, D, qscale=1.0):
    gen = torch.Generator().manual_seed(1000003 * B + 10007 * nhead + 101 * P + 7 * L + D)
    C = nhead * D
    q = (torch.randn(B, P, C, generator=gen) * qscale).to(DEV)
    kv = torch.randn(B, L, 2 * C, generator=gen).to(DEV)
    do = torch.randn(B, P, C, generator=gen).to(DEV)
    return q, kv[..., :C].contiguous(), kv[..., C:].contiguous(), do, kv


@functools.lru_cache(maxsize=None)
def _keep(shape, p, seed=SEED):
    return torch.from_numpy(M.keep_mask(shape[:4], p, seed)).to(DEV) if p else None


@functools.lru_cache(maxsize=None)
def _model(shape, p, qscale=1.0):
    q, k, v, do, _ = _inputs(*shape, qscale)
    return M.forward(q, k, v, shape[1], _keep(shape, p), p) + M.backward(q, k, v, do, shape[1], _keep(shape, p), p)


def _ld(t):
    """the row pitch of a [B, rows, C] tensor or view whose rows are dense and whose samples follow each other (0 for an output that is not wanted)"""
    if t is None:
        return 0
    assert t.stride(2) == 1 and t.stride(0) == t.size(1) * t.stride(1)
    return t.stride(1)


def fused(q, k, v, nhead, p=0.0, seed=0, do=None, want=(True, True, True), poison=True, grads=None):
    """the raw op: forward, and backward when do is given -> dict of outputs.  q, k, v and the gradients may be strided views (rows `ld` floats apart).  Outputs and
    workspace start as NaN: they are WRITTEN, and the workspace needs no set-up.  grads: (dq, dk, dv) buffers to write into instead of fresh dense ones."""
    lib = _lib.load()
    B, P, C = q.shape
    L, D = k.size(1), C // nhead
    new = (lambda *s: torch.full(s, float("nan"), device=DEV)) if poison else (lambda *s: torch.empty(s, device=DEV))
    nb = lib.paella_attn_train_workspace_bytes(B, nhead, P, L, D)
    assert nb > 0
    ws = torch.full((nb,), 255, dtype=torch.uint8, device=DEV) if poison else torch.empty(nb, dtype=torch.uint8, device=DEV)
    out = dict(o=new(B, P, C), lse=new(B, nhead, P))
    st = _lib.stream_ptr(q.device)
    _lib.check(lib.paella_attn_train_forward(_lib.ptr(q), _ld(q), _lib.ptr(k), _ld(k), _lib.ptr(v), _ld(v), B, nhead, P, L, D, p, seed, _lib.ptr(out["o"]),
                                             _lib.ptr(out["lse"]), _lib.ptr(ws), nb, st))
    if do is not None:
        if grads is None:
            grads = (new(B, P, C), new(B, L, C), new(B, L, C))
        dq, dk, dv = (g if w else None for g, w in zip(grads, want))
        out.update(dq=dq, dk=dk, dv=dv)
        _lib.check(lib.paella_attn_train_backward(_lib.ptr(q), _ld(q), _lib.ptr(k), _ld(k), _lib.ptr(v), _ld(v), _lib.ptr(out["o"]), _lib.ptr(out["lse"]), _lib.ptr(do),
                                                  B, nhead, P, L, D, p, seed, _lib.ptr(dq), _ld(dq), _lib.ptr(dk), _ld(dk), _lib.ptr(dv), _ld(dv), _lib.ptr(ws), nb, st))
    return out


def torch_chain(q, k, v, do, nhead, keep, p):
    """the attention core as torch runs it in fp32, written out: scores -> softmax -> times the given mask -> @ v, autograd's backward -> (o, dq, dk, dv)"""
    B, P, C = q.shape
    D = C // nhead
    qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
    qh, kh, vh = (t.view(B, -1, nhead, D).transpose(1, 2) for t in (qq, kk, vv))
    w = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(D), dim=-1)
    if keep is not None:
        w = w * (keep.float() * np.float32(M.scale_of(p)))
    o = (w @ vh).transpose(1, 2).reshape(B, P, C)
    o.backward(do)
    return o.detach(), qq.grad, kk.grad, vv.grad


def lse_bound(q, k, nhead, lse64):
    """|lse - fp64 lse| of the kernel's forms.  A score is a chain of D fp32 fmas (the exact-fp32 matrix core), off by at most D u A with A the largest
    sum_c |q_c k_c| / sqrt(D), plus one rounding for the product with 1 / sqrt(D) (itself rounded): 2 u |s|.  The running maximum is one of these scores.  Each term of
    the sum is exp2((s - m) log2 e): the subtraction and the product round the argument x <= 0 by at most 2 u |x|, which moves the term e^x by at most 2 u |x| e^x <=
    0.74 u (|x| e^x <= 1 / e), the hardware exp2 adds 1 ulp = 2 u of the term, and the largest term is 1, so relative to the sum l >= 1 every term is off by less than
    3 u.  The sum itself: a lane adds its 4 terms of each of the ceil(L / 16) tiles one by one and rescales once per tile, then two shuffle adds: at most L / 16 + 8
    roundings, u each, relative.  log l turns the relative error of l into an absolute one and adds 1 ulp of its own; m + log l is rounded once: 2 u |lse| covers both."""
    D = q.size(-1) // nhead
    A = float((M.heads(q, nhead).abs().unsqueeze(3) * M.heads(k, nhead).abs().unsqueeze(2)).sum(-1).max()) / math.sqrt(D)
    L = k.size(1)
    return U * (D * A + 2 * A + 3 + (L / 16 + 8) + 2 * float(lse64.abs().max()))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_accuracy_against_the_fp64_model(built_lib, shape, p):
    """Measured pairs (fused / torch, MI355X): all of them in profiles/train_attention_parity.txt."""
    q, k, v, do, _ = _inputs(*shape)
    nhead = shape[1]
    o64, lse64, dq64, dk64, dv64 = _model(shape, p)
    out = fused(q, k, v, nhead, p, SEED, do)
    ref = torch_chain(q, k, v, do, nhead, _keep(shape, p), p)
    pairs = []
    for name, a, b, m in zip(("o", "dq", "dk", "dv"), (out["o"], out["dq"], out["dk"], out["dv"]), ref, (o64, dq64, dk64, dv64)):
        assert torch.isfinite(a).all(), "%s: not finite" % name
        pairs.append((name, _err(a, m), _err(b, m), _ulp(m)))
    e_lse, b_lse = _err(out["lse"], lse64), lse_bound(q, k, nhead, lse64)
    print("train_attention parity %s p=%g: " % (shape, p) + "  ".join("%s fused %.3e torch %.3e ulp %.3e" % t for t in pairs) + "  lse fused %.3e bound %.3e" % (e_lse, b_lse))
    assert torch.isfinite(out["lse"]).all() and e_lse <= b_lse, "%s p=%g lse: error %.3e exceeds the derived bound %.3e" % (shape, p, e_lse, b_lse)
    for name, e_fused, e_torch, ulp in pairs:
        assert T.within_yardstick(e_fused, e_torch, ulp), "%s p=%g %s: fused error %.3e exceeds %gx max(torch fp32 chain %.3e, ulp %.3e)" % (shape, p, name, e_fused, FACTOR, e_torch, ulp)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_large_scores(built_lib, p):
    """q scaled so that |s| reaches about 80: exp(s) overflows fp32 at 88.7 and a sum of a few such terms well before, so the outputs are finite and right only if
    the row maximum really is subtracted"""
    shape = (2, 2, 33, 100, 32)
    qscale = 20.0
    q, k, v, do, _ = _inputs(*shape, qscale)
    nhead = shape[1]
    o64, lse64, dq64, dk64, dv64 = _model(shape, p, qscale)
    smax = float((M.heads(q, nhead) @ M.heads(k, nhead).transpose(-1, -2)).abs().max()) / math.sqrt(shape[4])
    assert 60.0 < smax < 110.0, smax
    out = fused(q, k, v, nhead, p, SEED, do)
    ref = torch_chain(q, k, v, do, nhead, _keep(shape, p), p)
    for name, b, m in zip(("o", "dq", "dk", "dv"), ref, (o64, dq64, dk64, dv64)):
        assert torch.isfinite(out[name]).all(), name
        e_fused, e_torch, ulp = _err(out[name], m), _err(b, m), _ulp(m)
        print("train_attention large scores (|s| <= %.1f) p=%g %s: fused %.3e torch %.3e ulp %.3e" % (smax, p, name, e_fused, e_torch, ulp))
        assert T.within_yardstick(e_fused, e_torch, ulp), "%s p=%g: fused error %.3e exceeds %gx max(torch %.3e, ulp %.3e)" % (name, p, e_fused, FACTOR, e_torch, ulp)
    assert torch.isfinite(out["lse"]).all() and _err(out["lse"], lse64) <= lse_bound(q, k, nhead, lse64)


@pytest.mark.parametrize("shape", [(2, 2, 33, 100, 32), (1, 2, 65, 131, 80), (2, 3, 21, 90, 128)], ids=ids)
def test_dropout_mask_is_the_cpu_philox_models(built_lib, shape):
    B, nhead, P, L, D = shape
    q, k, v, do, kv = _inputs(*shape)
    p = 0.1
    keep = _keep(shape, p)
    assert 0.05 < 1.0 - float(keep.float().mean()) < 0.15
    # v = 1: o (1 - p) is the kept probability mass of the row, the same in every channel of the head
    ones = torch.ones_like(v)
    o64, _ = M.forward(q, k, ones, nhead, keep, p)
    out = fused(q, k, ones, nhead, p, SEED)
    torch.testing.assert_close(out["o"].double(), o64, rtol=1e-5, atol=1e-6)
    full64, _ = M.forward(q, k, ones, nhead, None, 0.0)
    assert float((o64 - full64).abs().max()) > 0.05        # ... and the mask is visible in it
    # two seeds differ, and differ as the model says
    keep2 = _keep(shape, p, SEED + 1)
    o64b, _ = M.forward(q, k, ones, nhead, keep2, p)
    other = fused(q, k, ones, nhead, p, SEED + 1)
    assert float((o64b - o64).abs().max()) > 0.05
    torch.testing.assert_close(other["o"].double(), o64b, rtol=1e-5, atol=1e-6)
    if L <= D:
        # every element of the mask, exactly: with q = 0 every probability is 1 / L, and with v[key] = the unit vector of channel `key` o[q, key] = keep / ((1 - p) L)
        eye = torch.eye(L, D, device=DEV).repeat(1, nhead).expand(B, L, nhead * D).contiguous()
        for seed, km in ((SEED, keep), (SEED + 1, keep2)):
            got = fused(torch.zeros_like(q), k, eye, nhead, p, seed)["o"].view(B, P, nhead, D)[..., :L].permute(0, 2, 1, 3)
            assert torch.equal(got > 0.5 / L, km)
            assert torch.all(got[~km] == 0)
    # the backward regenerates the same mask: its gradients are the model's under that mask (and not those of the other seed's)
    ref = _model(shape, p)
    b = fused(q, k, v, nhead, p, SEED, do)
    for name, m in zip(("dq", "dk", "dv"), ref[2:]):
        torch.testing.assert_close(b[name].double(), m, rtol=1e-4, atol=1e-5)
    # without dropout the seed is without meaning, and the call that never mentions dropout gives the same bits
    a = fused(q, k, v, nhead, 0.0, SEED, do)
    c = fused(q, k, v, nhead, 0.0, 0, do)
    for name in ("o", "lse", "dq", "dk", "dv"):
        assert torch.equal(a[name], c[name]), name
    # the public function: its default call is the raw call at p = 0; with a seed, the raw call with that seed
    assert torch.equal(training.attention_dropout(q, kv, nhead), a["o"])
    assert torch.equal(training.attention_dropout(q, kv, nhead, p=0.0, seed=SEED), a["o"])
    assert torch.equal(training.attention_dropout(q, kv, nhead, p=p, seed=SEED), b["o"])


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_strided_operands(built_lib, p):
    """k / v as the halves of one [B, L, 2C] buffer and dk / dv written into one have the bits of the dense call; the padding floats of a wider pitch stay untouched"""
    shape = (2, 2, 33, 100, 32)
    B, nhead, P, L, D = shape
    C = nhead * D
    q, k, v, do, kv = _inputs(*shape)
    dense = fused(q, k, v, nhead, p, SEED, do)
    dkv = torch.full((B, L, 2 * C), float("nan"), device=DEV)
    halves = fused(q, kv[..., :C], kv[..., C:], nhead, p, SEED, do, grads=(torch.full((B, P, C), float("nan"), device=DEV), dkv[..., :C], dkv[..., C:]))
    assert torch.equal(halves["o"], dense["o"]) and torch.equal(halves["lse"], dense["lse"]) and torch.equal(halves["dq"], dense["dq"])
    assert torch.equal(dkv[..., :C], dense["dk"]) and torch.equal(dkv[..., C:], dense["dv"])
    # every pitch wider than the row, each by another amount; the floats between the rows hold NaN before and after
    pad = lambda t, extra: torch.cat([t, torch.full(t.shape[:2] + (extra,), float("nan"), device=DEV)], dim=2)
    qw, kw, vw = pad(q, 8), pad(k, 4), pad(v, 12)
    gq, gk, gv = (torch.full((B, n, C + e), float("nan"), device=DEV) for n, e in ((P, 4), (L, 8), (L, 16)))
    wide = fused(qw[..., :C], kw[..., :C], vw[..., :C], nhead, p, SEED, do, grads=(gq[..., :C], gk[..., :C], gv[..., :C]))
    assert torch.equal(wide["o"], dense["o"]) and torch.equal(wide["lse"], dense["lse"])
    for g, name in ((gq, "dq"), (gk, "dk"), (gv, "dv")):
        assert torch.equal(g[..., :C], dense[name]), name
        assert torch.isnan(g[..., C:]).all(), name


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("shape", [(2, 2, 7, 9, 16), (1, 2, 65, 131, 80), (1, 1, 16, 1040, 128)], ids=ids)
def test_null_outputs_and_determinism(built_lib, shape, p):
    q, k, v, do, _ = _inputs(*shape)
    nhead = shape[1]
    full = fused(q, k, v, nhead, p, SEED, do)
    for name in ("o", "lse", "dq", "dk", "dv"):
        assert torch.isfinite(full[name]).all(), name   # the NaN the outputs and the workspace were filled with is gone
    for _ in range(2):                                  # three calls in all, the later ones over uninitialised memory
        again = fused(q, k, v, nhead, p, SEED, do, poison=False)
        for name in ("o", "lse", "dq", "dk", "dv"):
            assert torch.equal(full[name], again[name]), name
    for want in [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True), (True, False, True)]:
        part = fused(q, k, v, nhead, p, SEED, do, want)
        for name, w in zip(("dq", "dk", "dv"), want):
            if w:
                assert torch.equal(part[name], full[name]), (want, name)
            else:
                assert part[name] is None
    none = fused(q, k, v, nhead, p, SEED, do, (False, False, False))
    assert torch.equal(none["o"], full["o"]) and torch.equal(none["lse"], full["lse"])


def test_samples_are_independent(built_lib):
    """p = 0: each sample of a batch of 3 has the bits of a one-sample call"""
    shape = (3, 2, 33, 100, 32)
    q, k, v, do, _ = _inputs(*shape)
    full = fused(q, k, v, shape[1], 0.0, 0, do)
    for b in range(3):
        one = fused(q[b:b + 1], k[b:b + 1], v[b:b + 1], shape[1], 0.0, 0, do[b:b + 1])
        for name in ("o", "lse", "dq", "dk", "dv"):
            assert torch.equal(full[name][b:b + 1], one[name]), (b, name)


def test_offsets_past_4_gib(built_lib):
    """q, o, do and dq of more than 2^32 bytes each against a short key set (so that the arithmetic stays cheap): the last 8192 rows of the last sample lie past
    byte 2^32, and that sample equals the one-sample call bit for bit"""
    B, nhead, P, L, D = 2, 8, (1 << 19) + 4096, 16, 128
    C = nhead * D
    assert B * P * C * 4 > 2 ** 32 and B * P * C - 2 ** 30 == 8192 * C
    gen = torch.Generator(device=DEV).manual_seed(5)
    q = torch.randn(B, P, C, device=DEV, generator=gen)
    do = torch.randn(B, P, C, device=DEV, generator=gen)
    k = torch.randn(B, L, C, device=DEV, generator=gen)
    v = torch.randn(B, L, C, device=DEV, generator=gen)
    big = fused(q, k, v, nhead, 0.0, 0, do, poison=False)
    one = fused(q[1:], k[1:], v[1:], nhead, 0.0, 0, do[1:])
    try:
        for name in ("o", "lse", "dq", "dk", "dv"):
            assert torch.isfinite(one[name]).all(), name
            assert torch.equal(big[name][1:], one[name]), name
        # and the one-sample call is right on its last rows (fp32 chain, loose: the accuracy tests hold the op to the fp64 model)
        ro, rdq, _, _ = torch_chain(q[1:, -64:], k[1:], v[1:], do[1:, -64:], nhead, None, 0.0)
        torch.testing.assert_close(one["o"][:, -64:], ro, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(one["dq"][:, -64:], rdq, rtol=1e-4, atol=1e-4)
        assert torch.isfinite(big["o"][0]).all() and torch.isfinite(big["dq"][0]).all() and not torch.equal(big["o"][0, :64], one["o"][0, :64])
    finally:
        del big, one, q, do
        torch.cuda.empty_cache()


def test_autograd_function_and_saved_state(built_lib):
    shape = (2, 2, 33, 100, 32)
    B, nhead, P, L, D = shape
    C = nhead * D
    q3, k3, v3, do, kv3 = _inputs(*shape)
    p = 0.1
    raw = fused(q3, k3, v3, nhead, p, SEED, do)
    q, kv = q3.clone().requires_grad_(True), kv3.clone().requires_grad_(True)
    packed = []

    def pack(t):
        packed.append(t.numel() * t.element_size())
        return t

    calls = training.ATTN_COUNTERS["calls"]
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        o = training.attention_dropout(q, kv, nhead, p, seed=SEED)
    assert training.ATTN_COUNTERS["calls"] == calls + 1
    assert o.shape == (B, P, C) and o.requires_grad and o.is_contiguous()
    # inputs, output and lse [B, nhead, P]: nothing of [P, L]
    assert sum(packed) == (q.numel() + kv.numel() + o.numel() + B * nhead * P) * 4, packed
    o.backward(do)
    assert torch.equal(o.detach(), raw["o"])
    assert torch.equal(q.grad, raw["dq"]) and kv.grad.shape == (B, L, 2 * C)
    assert torch.equal(kv.grad[..., :C], raw["dk"]) and torch.equal(kv.grad[..., C:], raw["dv"])
    # once differentiable: the gradient comes back without a graph of its own, so a second differentiation cannot silently use a wrong one
    qq = q3.clone().requires_grad_(True)
    (gq,) = torch.autograd.grad(training.attention_dropout(qq, kv3, nhead).sum(), qq, create_graph=True)
    assert not gq.requires_grad
    # needs_input_grad subsets: only q, only kv -- the same bits
    qz = q3.clone().requires_grad_(True)
    training.attention_dropout(qz, kv3, nhead, p, seed=SEED).backward(do)
    assert torch.equal(qz.grad, raw["dq"])
    kz = kv3.clone().requires_grad_(True)
    training.attention_dropout(q3, kz, nhead, p, seed=SEED).backward(do)
    assert torch.equal(kz.grad[..., :C], raw["dk"]) and torch.equal(kz.grad[..., C:], raw["dv"])
    assert not training.attention_dropout(q3, kv3, nhead, p, seed=SEED).requires_grad
    # views whose rows are not contiguous are copied, not misread; seed=None draws from torch's default CPU generator
    wide = torch.randn(B, P, 2 * C, device=DEV)
    assert torch.equal(training.attention_dropout(wide[..., :C], kv3, nhead), training.attention_dropout(wide[..., :C].contiguous(), kv3, nhead))
    torch.manual_seed(3)
    a = training.attention_dropout(q3, kv3, nhead, p)
    c = training.attention_dropout(q3, kv3, nhead, p)
    torch.manual_seed(3)
    b = training.attention_dropout(q3, kv3, nhead, p)
    assert torch.equal(a, b) and not torch.equal(a, c)
    with pytest.raises(ValueError, match="multiple of 16"):
        training.attention_dropout(torch.zeros(1, 2, 48, device=DEV), torch.zeros(1, 2, 96, device=DEV), 2)


@pytest.mark.parametrize("others", ["torch", "hip"])
@pytest.mark.parametrize("which", ["tiny", "variant"])
def test_train_step_with_hip_attention_reproduces_the_reference(golden, built_lib, which, others):
    """_train_step of tests/test_gpu_training.py under set_training_attention("hip"), alone and together with the other two switches, against the reference's recorded
    step (tiny: self_attn, D = 16; variant: conditioning keys only, D = 32) and under that test's tolerances: one call of the op per `A` block per forward, none in eval
    mode; then the hand-over to the HIP engine, which never sees the switch.  A train-mode call with attn_weights takes the torch branch under either setting."""
    cfg, m = T.model_for(which, golden, DEV)
    m.set_training_attention("hip").set_training_activation(others).set_training_depthwise(others)
    a_blocks = [b for lv in list(m.down_blocks) + list(m.up_blocks) for b in lv if b.kind == "A"]
    assert a_blocks and cfg["c_hidden"][-1] // cfg["nhead"][-1] == (16 if which == "tiny" else 32) and bool(cfg["self_attn"]) == (which == "tiny")
    n0 = training.ATTN_COUNTERS["calls"]
    pred, loss = _train_step(m, cfg)
    assert training.ATTN_COUNTERS["calls"] == n0 + len(a_blocks), "the train-mode forward did not route every AttnBlock through the HIP op"
    # with a key-weight vector the torch branch runs, switch or no switch: the counter stays, and the logits are those of the default route
    latents, t, mask, random_x, c = T.G.train_step_inputs(cfg)
    noised = (latents * (1 - mask) + random_x * mask).to(DEV)
    aw = torch.tensor([0.5, 2.0], device=DEV)
    with torch.no_grad():
        n1 = training.ATTN_COUNTERS["calls"]
        weighted = m(noised, t.to(DEV), **T.to_dev(c, DEV), attn_weights=aw)
        assert training.ATTN_COUNTERS["calls"] == n1
        m.set_training_attention("torch")
        assert torch.equal(weighted, m(noised, t.to(DEV), **T.to_dev(c, DEV), attn_weights=aw))
        m.set_training_attention("hip")
        assert training.ATTN_COUNTERS["calls"] == n1
    T.assert_switched_step_and_handover(m, cfg, golden("train_%s_step" % which), pred, loss, lambda: m.set_training_attention("torch"),
                                        op_calls=lambda: training.ATTN_COUNTERS["calls"], calls_per_forward=len(a_blocks))

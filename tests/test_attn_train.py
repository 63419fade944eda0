"""Training attention without a GPU: the fp64 model the GPU tests measure against (tests/attn_train_model.py, explicit exp / sum and a closed-form backward) equals
fp64 torch autograd of the plain torch formulation (scores -> softmax -> a dropout mask -> @ v); the mask follows the documented L4 counter rule; the C entry points
validate their arguments on the host before anything is enqueued; the Python surface refuses what the op cannot do instead of falling back; the network switch."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

import paella_amd
from oracle import golden_configs as G
from paella_amd import training
from tests import attn_train_model as M
from tests import counter_noise as CN
from tests import train_op_checks as T

ERR_ARG, ERR_WORKSPACE = -1, -3


def _inputs(B=2, nhead=3, P=7, L=9, D=4, seed=5):
    g = torch.Generator().manual_seed(seed)
    C = nhead * D
    q = torch.randn(B, P, C, generator=g, dtype=torch.float64)
    k = torch.randn(B, L, C, generator=g, dtype=torch.float64)
    v = torch.randn(B, L, C, generator=g, dtype=torch.float64)
    do = torch.randn(B, P, C, generator=g, dtype=torch.float64)
    return q, k, v, do


def reference_expression(q, k, v, nhead, keep, scale):
    """what `training._attn_block` computes between the projections, as plain torch ops with the dropout as an explicit mask"""
    B, P, C = q.shape
    D = C // nhead
    qh, kh, vh = (t.view(B, -1, nhead, D).transpose(1, 2) for t in (q, k, v))
    w = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(D), dim=-1) * keep * scale
    return (w @ vh).transpose(1, 2).reshape(B, P, C)


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_model_equals_fp64_autograd_of_the_plain_torch_formulation(p):
    B, nhead, P, L, D = 2, 3, 7, 9, 4
    q, k, v, do = _inputs(B, nhead, P, L, D)
    keep = M.keep_mask((B, nhead, P, L), p, 1234) if p else None
    k64 = torch.ones(B, nhead, P, L, dtype=torch.float64) if keep is None else torch.from_numpy(keep).double()
    if p:
        assert 0 < int(keep.sum()) < keep.size
    qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref = reference_expression(qq, kk, vv, nhead, k64, M.scale_of(p))
    ref.backward(do)
    o, lse = M.forward(q, k, v, nhead, keep, p)
    dq, dk, dv = M.backward(q, k, v, do, nhead, keep, p)
    torch.testing.assert_close(o, ref.detach(), rtol=1e-13, atol=1e-13)
    s = torch.einsum("bphd,blhd->bhpl", q.view(B, P, nhead, D), k.view(B, L, nhead, D)) / math.sqrt(D)
    torch.testing.assert_close(lse, torch.logsumexp(s, dim=-1), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(dq, qq.grad, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(dk, kk.grad, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(dv, vv.grad, rtol=1e-12, atol=1e-13)


def test_keep_mask_follows_the_l4_rule():
    """a row of L keys owns L4 / 4 = ceil(L / 4) whole Philox calls: element (row, key) is word key & 3 of counter row * L4 / 4 + key / 4, and no call is shared
    between two rows"""
    p, seed = 0.3, (1 << 63) + 12345
    key = (seed ^ M.ATTN_DROPOUT_SALT) & CN.M64
    for L in (5, 8):
        shape = (2, 2, 3, L)
        quads = (L + 3) // 4
        keep = M.keep_mask(shape, p, seed).reshape(-1, L)
        counters = set()
        for row in range(keep.shape[0]):
            mine = {row * quads + j // 4 for j in range(L)}
            assert not counters & mine
            counters |= mine
            for j in range(L):
                w = CN.philox4x32_scalar(key, row * quads + j // 4, 0)[j & 3]
                assert bool(keep[row, j]) == ((w >> 8) * 2.0 ** -24 >= float(np.float32(p))), (L, row, j)
        assert len(counters) == keep.shape[0] * quads
        assert not np.array_equal(keep, M.keep_mask(shape, p, seed + 1).reshape(-1, L))
    # L = 5 pads its rows to 8 elements: row 1 starts at counter 2, where a dense [rows, 5] numbering would put it at element 5 of counter 1
    assert bool(M.keep_mask((1, 1, 2, 5), p, seed)[0, 0, 1, 0]) == ((CN.philox4x32_scalar(key, 2, 0)[0] >> 8) * 2.0 ** -24 >= float(np.float32(p)))
    assert M.scale_of(0.0) == 1.0 and M.scale_of(0.5) == 2.0
    from tests import grn_act_model
    assert M.ATTN_DROPOUT_SALT != grn_act_model.DROPOUT_SALT   # the two ops under one seed draw unrelated masks


def test_argument_validation_without_gpu(built_lib):
    """every refusal comes from the host checks, before any device work: the pointers below are never dereferenced"""
    lib = built_lib
    ok = ctypes.c_void_p(4096)  # stands for any non-NULL, 16-byte aligned device pointer
    off = ctypes.c_void_p(4100)
    B, nhead, P, L, D = 2, 4, 64, 68, 16
    C = nhead * D
    need = lib.paella_attn_train_workspace_bytes(B, nhead, P, L, D)
    assert need >= B * nhead * P * 4

    def fwd(B=B, nhead=nhead, P=P, L=L, D=D, p_drop=0.1, q=ok, k=ok, v=ok, ldq=C, ldk=2 * C, ldv=2 * C, o=ok, ws=ok, ws_bytes=need):
        return lib.paella_attn_train_forward(q, ldq, k, ldk, v, ldv, B, nhead, P, L, D, p_drop, 7, o, ok, ws, ws_bytes, None)

    def bwd(B=B, nhead=nhead, P=P, L=L, D=D, p_drop=0.1, q=ok, k=ok, v=ok, ldq=C, ldk=2 * C, ldv=2 * C, o=ok, ws=ok, ws_bytes=need, dq=ok, dk=ok, dv=ok, lddq=C,
            lddk=2 * C, lddv=2 * C):
        return lib.paella_attn_train_backward(q, ldq, k, ldk, v, ldv, o, ok, ok, B, nhead, P, L, D, p_drop, 7, dq, lddq, dk, lddk, dv, lddv, ws, ws_bytes, None)

    def refused(call, named, **bad):
        assert call(**bad) == ERR_ARG, bad
        assert named.encode() in lib.paella_last_error(), (bad, lib.paella_last_error())

    for call in (fwd, bwd):
        for D_ in (8, 24, 144, 0):
            refused(call, "D=%d" % D_, D=D_)
        for bad in (dict(B=0), dict(B=65536), dict(nhead=0), dict(P=0), dict(P=(1 << 20) + 1), dict(L=0), dict(L=(1 << 20) + 1), dict(B=65535, nhead=64, P=1 << 20)):
            refused(call, "unsupported shape", **bad)
        for name in ("ldq", "ldk", "ldv"):
            refused(call, name, **{name: C + 2})      # not a multiple of 4
            refused(call, name, **{name: C - 4})      # below nhead * D
        for name in ("q", "k", "v", "o"):
            refused(call, "16-byte aligned", **{name: off})
            refused(call, name, **{name: None})
        for p_drop in (1.0, -0.1, float("nan")):
            refused(call, "p_drop", p_drop=p_drop)
        assert call(ws_bytes=need - 1) == ERR_WORKSPACE
        assert b"workspace" in lib.paella_last_error() and str(need).encode() in lib.paella_last_error()
        assert call(ws=None) == ERR_WORKSPACE
        refused(call, "workspace must be 16-byte aligned", ws=off)
    # the backward's own arguments: a gradient is wanted but an operand it needs is missing; the pitches and the alignment of the gradients
    refused(bwd, "k", k=None, dq=None, dv=None)
    for name in ("lddq", "lddk", "lddv"):
        refused(bwd, name, **{name: C + 2})
        refused(bwd, name, **{name: C - 4})
    for name in ("dq", "dk", "dv"):
        refused(bwd, "16-byte aligned", **{name: off})
    # the pitch of a gradient that is not wanted is not looked at, and with no gradient wanted nothing is launched
    assert bwd(dq=None, dk=None, dv=None, lddq=0, lddk=1, lddv=-5) == 0


def test_workspace_bytes(built_lib):
    ws = built_lib.paella_attn_train_workspace_bytes
    for bad in [(2, 4, 64, 68, 8), (2, 4, 64, 68, 24), (2, 4, 64, 68, 144), (0, 4, 64, 68, 16), (2, 0, 64, 68, 16), (2, 4, 0, 68, 16), (2, 4, 64, 0, 16),
                (65536, 4, 64, 68, 16), (2, 4, (1 << 20) + 1, 68, 16), (2, 4, 64, (1 << 20) + 1, 16), (65535, 64, 1 << 20, 68, 16)]:
        assert ws(*bad) == 0, bad
    for D in range(16, 129, 16):
        assert ws(2, 4, 64, 68, D) > 0
    # monotone in B, P and L, and one float per (sample, head, query)
    base = (3, 4, 65, 131, 80)
    for axis in (0, 2, 3):
        last = 0
        for n in (1, 2, 15, 16, 17, 100, 1000, 4097):
            shape = list(base)
            shape[axis] = n
            b = ws(*shape)
            assert b >= last > -1 and b % 256 == 0
            last = b
            assert shape[0] * shape[1] * shape[2] * 4 <= b < shape[0] * shape[1] * shape[2] * 4 + 256
    # the largest geometry the eval path is tested at, and the extremes of the range, are sized without overflow
    assert ws(64, 32, 128 * 128, 128 * 128 + 776, 80) == 64 * 32 * 128 * 128 * 4
    assert ws(1, 1, 1 << 20, 1 << 20, 128) > 0 and ws(65535, 1, 1 << 15, 1 << 20, 16) > 0
    assert training.ATTN_MAX_B >= 64 and training.ATTN_MAX_HEADS >= 32 and training.ATTN_MAX_P >= 128 * 128 and training.ATTN_MAX_L >= 128 * 128 + 776
    assert ws(training.ATTN_MAX_B, 1, 1, training.ATTN_MAX_L, 16) > 0 and ws(1, training.ATTN_MAX_HEADS, training.ATTN_MAX_P // 65536, 1, 16) > 0
    assert ws(1, 1, training.ATTN_MAX_P, 1, 16) > 0 and ws(training.ATTN_MAX_B + 1, 1, 1, 1, 16) == 0 and ws(1, 1, training.ATTN_MAX_P + 1, 1, 16) == 0
    assert ws(1, training.ATTN_MAX_HEADS + 1, 1, 1, 16) == 0 and ws(1, 1, 1, training.ATTN_MAX_L + 1, 16) == 0
    assert ws(1, 1 << 11, 1 << 20, 1, 16) == 0 and (1 << 31) - 1 == training.ATTN_MAX_ROWS


def test_attention_dropout_refuses_what_the_op_cannot_do():
    q = torch.zeros(2, 5, 32)
    kv = torch.zeros(2, 7, 64)
    with pytest.raises(ValueError, match="HIP device"):     # cpu tensors: there is no torch fallback
        training.attention_dropout(q, kv, 2, 0.1)
    with pytest.raises(ValueError, match="fp32"):
        training.attention_dropout(q.double(), kv, 2)
    with pytest.raises(ValueError, match="fp32"):
        training.attention_dropout(q, kv.half(), 2)
    with pytest.raises(ValueError, match="tensors"):
        training.attention_dropout(q, None, 2)
    for bad_q, bad_kv in ((q[0], kv), (q, kv[0]), (q, kv[:1]), (q, kv[..., :32]), (q, torch.zeros(2, 7, 96))):
        with pytest.raises(ValueError, match=r"\[B, L, 2C\]"):
            training.attention_dropout(bad_q, bad_kv, 2)
    for nhead in (0, 3, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="nhead"):
            training.attention_dropout(q, kv, nhead)
    with pytest.raises(ValueError, match="multiple of 16"):      # D = 8
        training.attention_dropout(q, kv, 4)
    with pytest.raises(ValueError, match="multiple of 16"):      # D = 24
        training.attention_dropout(torch.zeros(1, 2, 48), torch.zeros(1, 2, 96), 2)
    with pytest.raises(ValueError, match="multiple of 16"):      # D = 144
        training.attention_dropout(torch.zeros(1, 2, 144), torch.zeros(1, 2, 288), 1)
    with pytest.raises(ValueError, match="queries"):
        training.attention_dropout(torch.zeros(2, 0, 32), kv, 2)
    with pytest.raises(ValueError, match="keys"):
        training.attention_dropout(q, torch.zeros(2, 0, 64), 2)
    for p in (1.0, -0.1, float("nan"), 1.5):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            training.attention_dropout(q, kv, 2, p)


def test_set_training_attention():
    """(what every switch's setter does: tests/test_training.py::test_training_switch)"""
    m = paella_amd.Paella(**G.UNET_TINY).set_training_attention("hip")
    # the plan of a forward carries one field per row of the table, in its order
    assert training._plan(m, True)._fields[:len(training.TRAIN_SWITCHES)] == tuple(s.field for s in training.TRAIN_SWITCHES)
    assert training.ATTN_COUNTERS == {"calls": training.ATTN_COUNTERS["calls"]}
    # nothing new at the package root beyond the method
    assert not [n for n in dir(paella_amd) if "attention_dropout" in n or n.startswith("ATTN")]


@pytest.mark.parametrize("act,dw", list(itertools.product(("torch", "hip"), repeat=2)))
def test_the_switch_leaves_a_cpu_train_step_alone(act, dw):
    calls = training.ATTN_COUNTERS["calls"]
    T.assert_switch_leaves_a_cpu_train_step_alone(lambda m: m.set_training_attention("hip"), before=lambda m: m.set_training_activation(act).set_training_depthwise(dw))
    assert training.ATTN_COUNTERS["calls"] == calls

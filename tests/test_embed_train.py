"""Training token stem without a GPU: the fp64 model the GPU tests measure against (tests/embed_train_model.py: torch fp64 autograd through F.embedding ->
layer_norm -> pixel_unshuffle) against a case worked by hand and against F.pixel_unshuffle's channel order, clamped tokens included; the C entry points validate
their arguments on the host before anything is enqueued; the Python surface refuses what the op cannot do instead of falling back; the sixth switch."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import paella_amd
from oracle import golden_configs as G
from paella_amd import training
from tests import embed_train_model as M
from tests import train_op_checks as T

ERR_ARG, ERR_WORKSPACE = -1, -3


def _ln(row, eps=1e-6):
    mean = row.mean()
    var = ((row - mean) ** 2).mean()
    return (row - mean) / torch.sqrt(var + eps), 1.0 / torch.sqrt(var + eps)


def _ln_backward(row, g, eps=1e-6):
    """the LayerNorm backward of one row by hand: rstd ((g - mean g) - xhat mean(g xhat))"""
    xhat, rstd = _ln(row, eps)
    return rstd * ((g - g.mean()) - xhat * (g * xhat).mean())


def test_model_against_a_case_by_hand():
    """2 x 2 tokens over 3 labels, patch 1, one label twice, one never, one token below the range and one above it (clamped to labels 0 and 2)"""
    w = torch.tensor([[1.0, 2.0, 4.0, -3.0], [0.5, 0.25, -1.0, 8.0], [3.0, -2.0, 0.0, 1.5]], dtype=torch.float64)
    x = torch.tensor([[[-1, 2], [3, 0]]])             # labels 0, 2, 2, 0 after the clamp; label 1 never
    d = torch.arange(16, dtype=torch.float64).view(1, 2, 2, 4) * 0.25 - 1.0
    rows, dw = M.model(x, w, d, patch=1)
    want = torch.stack([_ln(w[l])[0] for l in (0, 2, 2, 0)]).view(1, 2, 2, 4)
    torch.testing.assert_close(rows, want, rtol=1e-13, atol=1e-13)
    g = d.view(4, 4)
    by_hand = torch.stack([_ln_backward(w[0], g[0] + g[3]), torch.zeros(4, dtype=torch.float64), _ln_backward(w[2], g[1] + g[2])])
    torch.testing.assert_close(dw, by_hand, rtol=1e-12, atol=1e-12)
    assert torch.all(dw[1] == 0)
    # the same with patch 2: ONE output position whose channel c p^2 + dy p + dx holds token (dy, dx)'s channel c
    rows2, dw2 = M.model(x, w, d.view(1, 1, 1, 16), patch=2)
    tok = [[0, 2], [2, 0]]
    for c in range(4):
        for dy in range(2):
            for dx in range(2):
                assert abs(float(rows2[0, 0, 0, c * 4 + dy * 2 + dx]) - float(_ln(w[tok[dy][dx]])[0][c])) < 1e-13
    g2 = d.view(4, 2, 2)                               # [c, dy, dx]
    by_hand2 = torch.stack([_ln_backward(w[0], g2[:, 0, 0] + g2[:, 1, 1]), torch.zeros(4, dtype=torch.float64), _ln_backward(w[2], g2[:, 0, 1] + g2[:, 1, 0])])
    torch.testing.assert_close(dw2, by_hand2, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("patch", [1, 2])
def test_model_channel_order_is_pixel_unshuffles(patch):
    x, w, _ = M.inputs(2, 4, 6, patch, 8, 11, seed=3)
    rows, _ = M.model(x, w, patch=patch)
    ln = F.layer_norm(w.double()[x], (8,), None, None, 1e-6)              # [B, H, W, c]
    want = F.pixel_unshuffle(ln.permute(0, 3, 1, 2), patch)                # [B, c p^2, H/p, W/p]
    assert torch.equal(rows, want.permute(0, 2, 3, 1))
    p = patch
    for (b, oy, ox, c, dy, dx) in [(0, 0, 0, 0, 0, 0), (1, 4 // p - 1, 6 // p - 1, 7, p - 1, p - 1), (1, 0, 1, 3, p - 1, 0)]:
        assert rows[b, oy, ox, c * p * p + dy * p + dx] == ln[b, oy * p + dy, ox * p + dx, c]


def test_model_clamps_out_of_range_tokens():
    x, w, d = M.inputs(2, 2, 4, 2, 8, 5, seed=4)
    x[0, 0, 0], x[1, 1, 3], x[0, 1, 2] = -1, 5, 1 << 40
    rows, dw = M.model(x, w, d, patch=2)
    rows_c, dw_c = M.model(x.clamp(0, 4), w, d, patch=2)
    assert torch.equal(rows, rows_c) and torch.equal(dw, dw_c) and torch.isfinite(dw).all()
    assert torch.all(dw[torch.bincount(x.clamp(0, 4).view(-1), minlength=5) == 0] == 0)


def test_argument_validation_without_gpu(built_lib):
    """every refusal comes from the host checks, before any device work: the pointers below are never dereferenced"""
    lib = built_lib
    p = ctypes.c_void_p(4096)  # stands for any non-NULL, 16-byte aligned device pointer
    off = ctypes.c_void_p(4100)
    B, H, W, C, patch, L = 2, 8, 8, 32, 2, 64
    need = lib.paella_embed_ln_train_workspace_bytes(B, H, W, C, patch, L)
    assert need == 256

    def fwd(B=B, H=H, W=W, C=C, patch=patch, L=L, tokens=p, table=p, rows=p, eps=1e-6, ws=p, ws_bytes=need):
        return lib.paella_embed_ln_train_forward(tokens, table, B, H, W, C, patch, L, eps, rows, ws, ws_bytes, None)

    def bwd(B=B, H=H, W=W, C=C, patch=patch, L=L, tokens=p, table=p, d_rows=p, eps=1e-6, dtable=p, ws=p, ws_bytes=need):
        return lib.paella_embed_ln_train_backward(tokens, table, d_rows, B, H, W, C, patch, L, eps, dtable, ws, ws_bytes, None)

    for call in (fwd, bwd):
        for bad in (dict(C=0), dict(C=6), dict(C=1028), dict(C=-4), dict(L=0), dict(L=65537), dict(B=0), dict(B=-1), dict(H=0), dict(H=7), dict(W=9), dict(patch=0),
                    dict(patch=3), dict(patch=4), dict(B=1 << 11, H=1 << 11, W=1 << 11, patch=1), dict(tokens=None), dict(table=None), dict(tokens=off), dict(table=off),
                    dict(ws=off)):
            assert call(**bad) == ERR_ARG, (call.__name__, bad)
            assert lib.paella_last_error()
        for eps in (0.0, -1.0, float("nan"), float("inf")):
            assert call(eps=eps) == ERR_ARG and b"eps" in lib.paella_last_error(), eps
        assert call(ws_bytes=need - 1) == ERR_WORKSPACE and b"paella_embed_ln_train_workspace_bytes" in lib.paella_last_error()
        assert call(ws=None) == ERR_WORKSPACE
    assert fwd(rows=None) == ERR_ARG and b"required" in lib.paella_last_error()
    assert fwd(rows=off) == ERR_ARG
    for bad in (dict(d_rows=None), dict(dtable=None)):
        assert bwd(**bad) == ERR_ARG and b"required" in lib.paella_last_error()
    for bad in (dict(d_rows=off), dict(dtable=off)):
        assert bwd(**bad) == ERR_ARG and b"aligned" in lib.paella_last_error()


def test_workspace_bytes(built_lib):
    size = built_lib.paella_embed_ln_train_workspace_bytes
    for bad in [(1, 1, 1, 0, 1, 3), (1, 1, 1, 6, 1, 3), (1, 1, 1, 1028, 1, 3), (1, 1, 1, 4, 1, 0), (1, 1, 1, 4, 1, 65537), (0, 2, 2, 4, 1, 3), (1, 3, 2, 4, 2, 3),
                (1, 2, 2, 4, 3, 3), (1 << 11, 1 << 11, 1 << 11, 4, 1, 3)]:
        assert size(*bad) == 0, bad
    for ok in [(1, 1, 1, 4, 1, 1), (2, 4, 6, 32, 2, 64), (16, 64, 64, 256, 2, 8192), (1, 2, 2, 1024, 2, 65536), ((1 << 11) - 1, 1 << 11, 1 << 11, 4, 2, 3)]:
        assert size(*ok) == 256, ok
    assert (training.EMBED_MAX_C, training.EMBED_MAX_LABELS, training.EMBED_MAX_POSITIONS) == (1024, 65536, 2 ** 31 - 1)


def test_token_embed_layernorm_refuses_what_the_op_cannot_do():
    x, w, _ = M.inputs(2, 4, 6, 2, 8, 11)
    op = training.token_embed_layernorm
    with pytest.raises(ValueError, match="HIP device"):     # cpu tensors: there is no torch fallback
        op(x, w, 2)
    with pytest.raises(ValueError, match="tensors"):
        op(x, None)
    with pytest.raises(ValueError, match="tensors"):
        op([[1]], w)
    for bad in ((x.int(), w), (x.float(), w), (x, w.double()), (x, w.half())):
        with pytest.raises(ValueError, match="int64 x and fp32 weight"):
            op(*bad)
    for patch in (0, 3, 4, 2.0, True, None):
        with pytest.raises(ValueError, match="patch"):
            op(x, w, patch)
    with pytest.raises(ValueError, match=r"\[B, H, W\]"):
        op(x[0], w)
    with pytest.raises(ValueError, match=r"\[num_labels, c_in\]"):
        op(x, w[0])
    for c_in in (6, 2, 1028):
        with pytest.raises(ValueError, match="multiple of 4"):
            op(x, torch.zeros(11, c_in))
    with pytest.raises(ValueError, match="num_labels"):
        op(x, torch.zeros(0, 8))
    with pytest.raises(ValueError, match="num_labels"):
        op(x, torch.zeros(1, 8).expand(65537, 8))
    with pytest.raises(ValueError, match="multiples of patch"):
        op(x[:, :3], w, 2)
    with pytest.raises(ValueError, match="multiples of patch"):
        op(x[:, :, :5], w, 2)
    with pytest.raises(ValueError, match="positions"):
        op(x[:0], w)
    with pytest.raises(ValueError, match="positions"):       # 2^31 output positions, one more than the kernels index
        op(torch.zeros(1, 1, 1, dtype=torch.int64).expand(1 << 11, 1 << 10, 1 << 10), w, 1)
    for eps in (0.0, -1e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            op(x, w, 2, eps)
    assert set(training.EMBED_COUNTERS) == {"calls", "backward"}


def test_the_sixth_switch():
    """(what every switch's setter does: tests/test_training.py::test_training_switch)"""
    S = training.Switch
    assert training.TRAIN_SWITCHES[-1] == S("stem", "embedding", "torch", "hip") and training.TRAIN_SWITCHES[-1].name == "embedding"
    assert training.TRAIN_SWITCHES[:5] == (S("act", "activation", "torch", "hip"), S("dw", "depthwise", "torch", "hip"), S("attn", "attention", "torch", "hip"),
                                           S("mod", "modulation", "torch", "hip"), S("gemm", "gemm", "fp32", "bf16"))
    names = set(dir(paella_amd))
    m = paella_amd.Paella(**G.UNET_TINY)
    assert m._train_embedding == "torch" and m.training_route()["embedding"] == "torch"
    m.train()
    assert not training._plan(m, True).stem
    assert m.set_training_embedding("hip") is m and m.training_route()["embedding"] == "hip"
    assert training._plan(m, True).stem and not training._plan(m, False).stem
    assert m.set_training_route(embedding="torch").training_route()["embedding"] == "torch"
    with pytest.raises(ValueError, match="training embedding must be 'torch' or 'hip'"):
        m.set_training_embedding("bf16")
    assert training.TRAIN_SWITCHES[-1].label == "training embedding"
    assert "token_embed_layernorm" in (paella_amd.Paella.set_training_embedding.__doc__ or "")
    # nothing new at the package root beyond the method
    assert set(dir(paella_amd)) == names and not [n for n in dir(paella_amd) if "token_embed" in n or n.startswith("EMBED")]


@pytest.mark.parametrize("others", ["torch", "hip"])
def test_the_switch_leaves_a_cpu_train_step_alone(others):
    calls = dict(training.EMBED_COUNTERS)
    T.assert_switch_leaves_a_cpu_train_step_alone(lambda m: m.set_training_embedding("hip"),
                                                  before=lambda m: m.set_training_route(activation=others, depthwise=others, attention=others, modulation=others))
    assert training.EMBED_COUNTERS == calls

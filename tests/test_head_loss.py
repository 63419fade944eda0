"""Training loss head without a GPU: the fp64 model the GPU tests measure against equals torch's own cross-entropy and its autograd gradients; the three C entry
points validate their arguments on the host before anything is enqueued; the Python surface refuses what the op cannot do instead of falling back."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import paella_amd
from oracle import golden_configs as G
from paella_amd import training
from tests import head_loss_model as M

ERR_ARG, ERR_WORKSPACE = -1, -3


def _inputs(rows=37, N=48, K=16, seed=5):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(rows, K, generator=g, dtype=torch.float64)
    w = torch.randn(N, K, generator=g, dtype=torch.float64) / K ** 0.5
    t = torch.randint(0, N, (rows,), generator=g)
    gl = torch.rand(rows, generator=g, dtype=torch.float64) * 2
    return h, w, t, gl


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_model_equals_torch_cross_entropy_and_its_gradients(eps):
    h, w, t, gl = _inputs()
    h.requires_grad_(True)
    w.requires_grad_(True)
    l = h @ w.t()
    ref = F.cross_entropy(l, t, label_smoothing=eps, reduction='none')
    (ref * gl).sum().backward()
    loss, lse, argmax, _ = M.forward(h.detach(), w.detach(), t, eps)
    dh, dw = M.backward(h.detach(), w.detach(), t, eps, gl)
    torch.testing.assert_close(loss, ref.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(lse, torch.logsumexp(l.detach(), 1), rtol=1e-12, atol=1e-12)
    assert torch.equal(argmax, l.detach().argmax(1))
    torch.testing.assert_close(dh, h.grad, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(dw, w.grad, rtol=1e-11, atol=1e-13)


def test_model_argmax_takes_the_lowest_label_of_a_tie():
    h, w, t, _ = _inputs()
    w[40] = w[3]
    w[47] = w[3]
    h = h * 0 + w[3] * 4  # every row aligned with the three identical weight rows
    _, _, argmax, l = M.forward(h, w, t, 0.0)
    assert torch.equal(l[:, 3], l[:, 40]) and torch.equal(l[:, 3], l[:, 47])
    assert torch.equal(argmax, torch.full_like(argmax, 3))


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_model_ignored_row_equals_torch_ignore_index(eps):
    h, w, t, gl = _inputs()
    t[::5] = -100
    h.requires_grad_(True)
    w.requires_grad_(True)
    ref = F.cross_entropy(h @ w.t(), t, label_smoothing=eps, reduction='none', ignore_index=-100)
    (ref * gl).sum().backward()
    loss, _, _, _ = M.forward(h.detach(), w.detach(), t, eps)
    dh, dw = M.backward(h.detach(), w.detach(), t, eps, gl)
    assert torch.all(loss[::5] == 0) and torch.all(dh[::5] == 0)
    torch.testing.assert_close(loss, ref.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dh, h.grad, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(dw, w.grad, rtol=1e-11, atol=1e-13)
    # any other target outside [0, N) is the same ignored row
    t2 = t.clone()
    t2[::5] = torch.tensor([-1, 48, 2 ** 40, -100] * 2)[: t2[::5].numel()]
    assert torch.equal(M.forward(h.detach(), w.detach(), t2, eps)[0], loss)
    assert torch.equal(M.backward(h.detach(), w.detach(), t2, eps, gl)[1], dw)


def test_argument_validation_without_gpu(built_lib):
    """every refusal comes from the host checks, before any device work: the pointers below are never dereferenced"""
    lib = built_lib
    p = ctypes.c_void_p(4096)  # stands for any non-NULL device pointer
    rows, N, K = 512, 128, 64
    need = lib.paella_head_loss_workspace_bytes(rows, N, K)
    assert need > 0

    def fwd(rows=rows, N=N, K=K, eps=0.1, h=p, ws_bytes=need):
        return lib.paella_head_loss_forward(h, p, p, rows, N, K, eps, p, p, None, p, ws_bytes, None)

    def bwd(rows=rows, N=N, K=K, eps=0.1, h=p, ws_bytes=need):
        return lib.paella_head_loss_backward(h, p, p, p, p, rows, N, K, eps, p, p, p, ws_bytes, None)

    for call in (fwd, bwd):
        for bad in (dict(K=8), dict(K=272), dict(N=24), dict(rows=0), dict(eps=1.0), dict(eps=float("nan")), dict(h=None), dict(eps=-0.1), dict(rows=(1 << 24) + 1),
                    dict(N=65536 + 16)):
            assert call(**bad) == ERR_ARG, bad
            assert lib.paella_last_error()
        assert call(ws_bytes=need - 1) == ERR_WORKSPACE
        assert b"workspace" in lib.paella_last_error()
    for rows_, N_, K_ in [(rows, N, 8), (rows, N, 272), (rows, 24, K), (0, N, K), (rows, 8, K), ((1 << 24) + 1, N, K)]:
        assert lib.paella_head_loss_workspace_bytes(rows_, N_, K_) == 0
    # the workspace stays under a quarter of ONE fp32 logits tensor (rows * N * 4 / 4 bytes)
    for rows_ in (4096, 16384, 65536):
        b = lib.paella_head_loss_workspace_bytes(rows_, 8192, 256)
        assert 0 < b < rows_ * 8192 * 4 // 4, (rows_, b)


def test_forward_loss_refuses_eval_mode():
    m = paella_amd.Paella(**G.UNET_TINY)
    assert not m.training
    x = torch.zeros(1, 16, 16, dtype=torch.long)
    with pytest.raises(RuntimeError, match=r"model\.train\(\)"):
        m.forward_loss(x, torch.zeros(1), x, torch.zeros(1, 2, G.UNET_TINY["byt5_embd"]))


def test_head_cross_entropy_has_no_cpu_fallback():
    h, w, t, _ = _inputs(K=32)
    with pytest.raises(ValueError, match="HIP device"):
        training.head_cross_entropy(h.float(), w.float(), t, 0.1)

"""fp64 model of the training loss head (include/paella_hip.h "Training loss head"): the classifier head with the label-smoothed cross-entropy, its argmax with the
lowest label on ties, ignored rows (a target outside [0, N)), and both gradients for a given gradient g of the per-row loss.  Plain torch on whatever device the
inputs live on; shared by tests/test_head_loss.py (against torch's own cross_entropy) and tests/test_gpu_head_loss.py (against the HIP op)."""
import torch


def logits64(h, w):
    return h.double() @ w.double().t()


def forward(h, w, target, eps):
    """-> (loss [rows], lse [rows], argmax [rows] int64, logits [rows, N]), all fp64 but argmax"""
    l = logits64(h, w)
    N = l.size(1)
    lse = torch.logsumexp(l, dim=1)
    valid = (target >= 0) & (target < N)
    lt = l.gather(1, target.clamp(0, N - 1)[:, None])[:, 0]
    loss = (1 - eps) * (lse - lt) + eps * (lse - l.mean(dim=1))
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    idx = torch.arange(N, device=l.device)[None, :].expand_as(l)
    argmax = torch.where(l == l.max(dim=1, keepdim=True).values, idx, torch.full_like(idx, N)).min(dim=1).values  # the lowest label of a tie
    return loss, lse, argmax, l


def backward(h, w, target, eps, g):
    """-> (dh [rows, K], dw [N, K]) in fp64 for the gradient g [rows] arriving at the per-row loss"""
    l = logits64(h, w)
    N = l.size(1)
    valid = (target >= 0) & (target < N)
    d = torch.exp(l - torch.logsumexp(l, dim=1, keepdim=True)) - eps / N
    d.scatter_add_(1, target.clamp(0, N - 1)[:, None], torch.full((l.size(0), 1), -(1 - eps), dtype=d.dtype, device=d.device))
    d = d * (g.double() * valid.double())[:, None]
    return d @ w.double(), d.t() @ h.double()


def top2_gap(l):
    t = l.topk(2, dim=1).values
    return t[:, 0] - t[:, 1]

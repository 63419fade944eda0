"""GPU: the training optimizer step (paella_amd.training.ClippedAdamW, paella_amd/csrc/optim.hip) against the fp64 model of tests/adamw_model.py.

The accuracy rule (train_op_checks.within_yardstick): `clip_grad_norm_` + `torch.optim.AdamW` run on the same device from the same inputs; its max abs error
against the fp64 model is measured for each tensor's p, exp_avg, exp_avg_sq and for the norm, and the fused op stays within 4 x max(that error, one fp32 ulp at the
model's largest magnitude).  Three consecutive steps with fresh seeded gradients, checked after each; every check prints its worst pair (kept in
profiles/train_optimizer_parity.txt).  C below is the exported chunk size."""
import copy
import math
import warnings

import numpy as np
import pytest
import torch
from torch import nn

from oracle import paella_oracle as O
from oracle import golden_configs as G
from paella_amd import _lib, train_ops, training
from tests import adamw_model as A
from tests import train_op_checks as T
from tests.helpers import cond_for, to_dev
from tests.test_gpu_training import _train_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
ERR_ARG, ERR_WORKSPACE = -1, -3


def chunk():
    return _lib.load().paella_adamw_chunk_elems()


def off_grain(t):
    """t's values in device memory that is 4-byte aligned only: a view at storage offset 1"""
    base = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = base[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 or t.numel() == 0
    return v


def tensors(sizes, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen) * scale for n in sizes]


class Trio:
    """The same parameters three times: under ClippedAdamW on the device ("f"), under clip_grad_norm_ + torch.optim.AdamW on the device ("t") and as the fp64 model
    on the CPU ("m").  init: fp32 CPU tensors; groups: [(indices, hyperparameters of the group)], default one group; off_grain: indices whose fused parameter AND
    gradient sit at a 4-byte aligned address."""

    def __init__(self, name, init, groups=None, max_norm=1.0, off_grain_at=(), **hyper):
        self.name, self.max_norm, self.off = name, max_norm, set(off_grain_at)
        groups = groups or [(range(len(init)), {})]
        base = dict(HYPER, **hyper)
        self.hyper = [None] * len(init)
        for idx, h in groups:
            for i in idx:
                self.hyper[i] = dict(base, **h)
        self.fp = [nn.Parameter(off_grain(t) if i in self.off else t.to(DEV)) for i, t in enumerate(init)]
        self.tp = [nn.Parameter(t.to(DEV)) for t in init]
        self.opt_f = training.ClippedAdamW([dict(params=[self.fp[i] for i in idx], **h) for idx, h in groups], max_norm=max_norm, **base)
        self.opt_t = torch.optim.AdamW([dict(params=[self.tp[i] for i in idx], **h) for idx, h in groups], **base)
        self.p64 = [t.double() for t in init]
        self.m64 = [torch.zeros_like(p) for p in self.p64]
        self.v64 = [torch.zeros_like(p) for p in self.p64]
        self.steps = [0] * len(init)
        self.norm64 = self.norm_t = None
        self.n_checked = 0

    def set_lr(self, lr):
        for opt in (self.opt_f, self.opt_t):
            for g in opt.param_groups:
                g["lr"] = lr
        for h in self.hyper:
            h["lr"] = lr

    def step(self, grads, run="ftm"):
        """grads: per tensor an fp32 CPU tensor or None (no gradient this step)"""
        if "f" in run:
            for i, (p, g) in enumerate(zip(self.fp, grads)):
                p.grad = None if g is None else off_grain(g) if i in self.off else g.to(DEV)
            self.opt_f.step()
        if "t" in run:
            for p, g in zip(self.tp, grads):
                p.grad = None if g is None else g.to(DEV)
            with_g = [p for p in self.tp if p.grad is not None]
            if self.max_norm is None:
                self.norm_t = nn.utils.get_total_norm([p.grad for p in with_g])
            else:
                self.norm_t = nn.utils.clip_grad_norm_(with_g, self.max_norm)
            self.opt_t.step()
        if "m" in run:
            self.norm64 = A.model_norm([g for g in grads if g is not None])
            coef = A.model_coef(self.norm64, self.max_norm)
            for i, g in enumerate(grads):
                if g is not None:
                    self.steps[i] += 1
                    self.p64[i], self.m64[i], self.v64[i] = A.model_step(self.p64[i], g.double(), self.m64[i], self.v64[i], self.steps[i], self.hyper[i], coef)
        return self

    def check(self, what, norm=True):
        """the accuracy rule for every tensor's p, exp_avg and exp_avg_sq and for the norm; a tensor that never had a gradient has no state on either side"""
        worst, fails = (-1.0, None), []
        for i, (pf, pt) in enumerate(zip(self.fp, self.tp)):
            if self.steps[i] == 0:
                assert pf not in self.opt_f.state and torch.equal(pf.detach().cpu().double(), self.p64[i])
                continue
            sf, st = self.opt_f.state[pf], self.opt_t.state[pt]
            assert sf["step"].dtype == torch.float32 and sf["step"].dim() == 0 and sf["step"].is_cuda
            if pf.numel():
                assert float(sf["step"]) == float(st["step"]) == self.steps[i], (i, float(sf["step"]), float(st["step"]), self.steps[i])
            for name, gf, gt, ref in (("p", pf.detach(), pt.detach(), self.p64[i]), ("exp_avg", sf["exp_avg"], st["exp_avg"], self.m64[i]),
                                      ("exp_avg_sq", sf["exp_avg_sq"], st["exp_avg_sq"], self.v64[i])):
                if not ref.numel():
                    continue
                assert torch.isfinite(gf).all(), (i, name)
                ef, et, u = T.err(gf.cpu(), ref), T.err(gt.cpu(), ref), T.ulp(ref)
                if ef / max(et, u) > worst[0]:
                    worst = (ef / max(et, u), "tensor %d (%d elements) %s: e(fused) %.3e e(torch) %.3e ulp %.3e" % (i, ref.numel(), name, ef, et, u))
                if not T.within_yardstick(ef, et, u):
                    fails.append("tensor %d (%d elements) %s: error %.3e exceeds %gx max(torch %.3e, ulp %.3e)" % (i, ref.numel(), name, ef, T.FACTOR, et, u))
        line = "train_optimizer parity %s %s: largest e(fused) / max(e(torch), ulp) = %.3f in %s" % (self.name, what, worst[0], worst[1])
        if norm:
            nf = float(self.opt_f.grad_norm)
            ef, et, u = abs(nf - self.norm64), abs(float(self.norm_t) - self.norm64), float(np.spacing(np.float32(self.norm64)))
            line += "; norm %.9g: e(fused) %.3e e(torch) %.3e ulp %.3e" % (self.norm64, ef, et, u)
            if not T.within_yardstick(ef, et, u):
                fails.append("norm: error %.3e exceeds %gx max(torch %.3e, ulp %.3e)" % (ef, T.FACTOR, et, u))
        print(line)
        assert not fails, "%s %s: outside the yardstick:\n%s" % (self.name, what, "\n".join(fails))
        self.n_checked += 1

    def three_steps(self, sizes, seed, scale=1.0):
        for k in (1, 2, 3):
            self.step(tensors(sizes, seed + k, scale)).check("step %d" % k)
        return self

    def fused_bits(self):
        out = [self.opt_f.grad_norm.clone()]
        for p in self.fp:
            st = self.opt_f.state.get(p, {})
            out += [p.detach().clone()] + [st[k].clone() for k in ("step", "exp_avg", "exp_avg_sq") if k in st]
        return out


def same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_grains(built_lib):
    """every size at which a kernel takes another path: below / at / above a 16-byte vector, a wave, a workgroup, a chunk; several chunks with a short last one; no
    element at all; and one tensor -- C + 1 elements, two chunks -- whose parameter and gradient are 4-byte aligned only (the scalar path)"""
    C = chunk()
    sizes = [1, 3, 4, 5, 255, 256, 257, 1023, C - 1, C, C + 1, 2 * C + 3, 0, C + 1]
    t = Trio("grains", tensors(sizes, 100, 0.5), off_grain_at=(len(sizes) - 1,)).three_steps(sizes, 200)
    assert t.n_checked == 3 and t.fp[-1].data_ptr() % 16 == 4


def test_many_tensors(built_lib):
    """300 tensors of 1...2000 elements: more rows than the finalize workgroup has threads would need one each -- its loops over the rows take several rounds"""
    sizes = [int(v) for v in torch.randint(1, 2001, (300,), generator=torch.Generator().manual_seed(5))]
    Trio("many", tensors(sizes, 101, 0.5)).three_steps(sizes, 300)


def test_more_rows_than_finalize_threads(built_lib):
    """1100 tensors of 1...40 elements: more rows than the 1024 threads of the finalize workgroup"""
    sizes = [int(v) for v in torch.randint(1, 41, (1100,), generator=torch.Generator().manual_seed(6))]
    Trio("rows>1024", tensors(sizes, 102, 0.5)).three_steps(sizes, 400)


def test_groups(built_lib):
    """two parameter groups with different lr, weight decay, betas and eps under one global norm"""
    C = chunk()
    sizes = [1000, C + 77, 77, 4097, 300]
    groups = [((0, 1, 2), dict(lr=3e-3, weight_decay=0.1, betas=(0.8, 0.95), eps=1e-6)), ((3, 4), dict(lr=5e-4, weight_decay=0.0, betas=(0.95, 0.9999), eps=1e-10))]
    t = Trio("groups", tensors(sizes, 103, 0.5), groups=groups).three_steps(sizes, 500)
    assert [g["lr"] for g in t.opt_f.param_groups] == [3e-3, 5e-4]


def test_clipping(built_lib):
    """active (norm >> max_norm), max_norm = None on the same gradients, and inactive (norm << max_norm): then the result equals the run without clipping bit for bit"""
    C = chunk()
    sizes = [C + 9, 513, 64]
    init = tensors(sizes, 104, 0.5)
    active = Trio("clip-active", init).three_steps(sizes, 600, scale=30.0)
    assert active.norm64 > 1000.0
    none = Trio("clip-none", init, max_norm=None).three_steps(sizes, 600, scale=30.0)
    assert not same_bits(active.fused_bits()[1:], none.fused_bits()[1:]) and torch.equal(active.opt_f.grad_norm, none.opt_f.grad_norm)
    small = Trio("clip-inactive", init).three_steps(sizes, 600, scale=1e-4)
    assert small.norm64 < 0.01
    small_none = Trio("clip-inactive-none", init, max_norm=None).three_steps(sizes, 600, scale=1e-4)
    assert same_bits(small.fused_bits(), small_none.fused_bits())


def test_missing_gradients(built_lib):
    """tensor 1 has no gradient for two steps: untouched, no state entry, not in the norm (the model's norm leaves it out).  At step 3 it gets one: its step is 1
    while the others are at 3, and it is held to the model with its own bias correction"""
    C = chunk()
    sizes = [300, C + 5, 77]
    t = Trio("missing", tensors(sizes, 105, 0.5))
    before = t.fp[1].detach().clone()
    for k in (1, 2):
        g = tensors(sizes, 700 + k)
        g[1] = None
        t.step(g).check("step %d" % k)
        assert t.fp[1] not in t.opt_f.state and torch.equal(t.fp[1].detach(), before)
    t.step(tensors(sizes, 703)).check("step 3")
    assert t.steps == [3, 1, 3] and [float(t.opt_f.state[p]["step"]) for p in t.fp] == [3.0, 1.0, 3.0]


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_step_is_skipped(built_lib, bad):
    """one bad element: p, exp_avg, exp_avg_sq and the steps stay bit for bit, grad_norm is not finite, and the next finite step equals a run in which the bad step
    never happened"""
    C = chunk()
    sizes = [C + 3, 100]
    init = tensors(sizes, 106, 0.5)
    g1, g2, g3 = (tensors(sizes, 800 + k) for k in (1, 2, 3))
    g2[0][C + 1] = bad
    a, b = Trio("nonfinite", init), Trio("nonfinite-never", init)
    a.step(g1, run="f")
    held = a.fused_bits()[1:]
    version = a.fp[0]._version
    a.step(g2, run="f")
    assert not math.isfinite(float(a.opt_f.grad_norm))
    assert same_bits(a.fused_bits()[1:], held) and [float(s) for s in a.opt_f._steps] == [1.0, 1.0]
    assert a.fp[0]._version > version                # a version bump without a change costs the engine a reload and nothing else
    a.step(g3, run="f")
    b.step(g1, run="f").step(g3, run="f")
    assert same_bits(a.fused_bits(), b.fused_bits()) and [float(s) for s in a.opt_f._steps] == [2.0, 2.0]


def test_large_magnitudes(built_lib):
    """gradients of 1e25: squared in fp32 they overflow; widened to fp64 first they do not.  The norm is ONE rounding to fp32 of an fp64 sum (relative 2^-23),
    clipping brings g' to order 1 / sqrt(n) and the parameters stay finite"""
    C = chunk()
    sizes = [C + 17, 300]
    t = Trio("1e25", tensors(sizes, 107, 0.5))
    g = [x * 1e25 for x in tensors(sizes, 900)]
    t.step(g, run="fm")
    got = float(t.opt_f.grad_norm)
    print("train_optimizer parity 1e25: norm %.9g, model %.9g, relative error %.3e" % (got, t.norm64, abs(got - t.norm64) / t.norm64))
    assert math.isfinite(got) and got > 1e26 and abs(got - t.norm64) <= 2.0 ** -23 * t.norm64
    for i, p in enumerate(t.fp):
        assert torch.isfinite(p).all() and all(torch.isfinite(t.opt_f.state[p][k]).all() for k in ("exp_avg", "exp_avg_sq"))
        assert T.err(p.detach().cpu(), t.p64[i]) <= T.FACTOR * T.ulp(t.p64[i])


def test_determinism(built_lib):
    """the same inputs twice give the same bits in p, exp_avg, exp_avg_sq and the norm -- with more chunks (2100) than the grid has workgroups, so a workgroup takes
    several chunks and the finalize workgroup several partials per thread"""
    C = chunk()
    sizes = [2100 * C + 7, 1000, C]
    init, g = tensors(sizes, 108, 0.5), [tensors(sizes, 1000 + k) for k in (1, 2)]
    runs = []
    for _ in range(2):
        t = Trio("determinism", init)
        t.step(g[0], run="f").step(g[1], run="f")
        runs.append(t.fused_bits())
    assert same_bits(*runs)
    t.step(g[0], run="m").step(g[1], run="m")
    assert abs(float(t.opt_f.grad_norm) - t.norm64) <= float(np.spacing(np.float32(t.norm64)))


def test_no_sync_sequence(built_lib):
    """20 steps issued back to back with another lr each, the gradients already on the device, under torch's synchronisation detector: no step waits for the
    device, no step reads a table that a later step has overwritten (each row carries its step's lr), and the result obeys the accuracy rule"""
    C = chunk()
    sizes = [C + 33, 700, 5]
    t = Trio("no-sync", tensors(sizes, 109, 0.5))
    grads = [tensors(sizes, 1100 + k) for k in range(20)]
    lrs = [1e-3 * (1 + k % 7) for k in range(20)]
    on_dev = [[g.to(DEV) for g in gs] for gs in grads]
    waits = train_ops.ADAMW_COUNTERS["staging_waits"]
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for gs, lr in zip(on_dev, lrs):
                for g in t.opt_f.param_groups:
                    g["lr"] = lr
                for p, g in zip(t.fp, gs):
                    p.grad = g
                t.opt_f.step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert not [str(w.message) for w in caught if "synchronizing" in str(w.message).lower()], [str(w.message) for w in caught]
    print("train_optimizer parity no-sync: %d waits for a staging buffer in 20 steps" % (train_ops.ADAMW_COUNTERS["staging_waits"] - waits))
    for gs, lr in zip(grads, lrs):
        t.set_lr(lr)
        t.step(gs, run="tm")
    t.check("20 steps")


def test_state_dict_from_torch(built_lib):
    """two steps of torch AdamW (its "step" tensors live on the CPU, as in the reference's checkpoints), load_state_dict into ClippedAdamW, one more step each"""
    C = chunk()
    sizes = [C + 3, 500, 9]
    t = Trio("state-from-torch", tensors(sizes, 110, 0.5))
    for k in (1, 2):
        t.step(tensors(sizes, 1200 + k), run="tm")
    sd = copy.deepcopy(t.opt_t.state_dict())
    assert all(not st["step"].is_cuda for st in sd["state"].values())
    t.opt_f.load_state_dict(sd)
    with torch.no_grad():
        for pf, pt in zip(t.fp, t.tp):
            pf.copy_(pt)
    assert [float(t.opt_f.state[p]["step"]) for p in t.fp] == [2.0] * 3 and all(t.opt_f.state[p]["step"].is_cuda for p in t.fp)
    t.step(tensors(sizes, 1203)).check("step 3 after load")


def test_state_dict_into_torch(built_lib):
    """two steps of ClippedAdamW, its state_dict() into torch.optim.AdamW, one more step each; the loaded dict shares nothing with the optimizer that wrote it"""
    C = chunk()
    sizes = [C + 3, 500, 9]
    t = Trio("state-into-torch", tensors(sizes, 111, 0.5))
    for k in (1, 2):
        t.step(tensors(sizes, 1300 + k), run="fm")
    sd = t.opt_f.state_dict()
    assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    assert all(st["step"].data_ptr() != t.opt_f.state[p]["step"].data_ptr() for st, p in zip(sd["state"].values(), t.fp))
    t.opt_t.load_state_dict(copy.deepcopy(sd))
    with torch.no_grad():
        for pf, pt in zip(t.fp, t.tp):
            pt.copy_(pf)
    t.step(tensors(sizes, 1303)).check("step 3 after load")
    # and round: the dict of this class loads into this class
    other = training.ClippedAdamW([nn.Parameter(p.detach().clone()) for p in t.fp])
    other.load_state_dict(copy.deepcopy(t.opt_f.state_dict()))
    assert [float(s) for s in other._steps] == [3.0] * 3


def test_grad_norm_alone(built_lib):
    """training.grad_norm: the norm through paella_adamw_grad_norm, one rounding of the fp64 sum; gradients are not touched, a parameter without one is left out"""
    C = chunk()
    sizes = [C + 3, 500, 9, 40]
    ps = [nn.Parameter(t.to(DEV)) for t in tensors(sizes, 112)]
    gs = tensors(sizes, 1400, 3.0)
    for p, g in zip(ps[:3], gs):
        p.grad = g.to(DEV)
    ps[1].grad_dtype = None                            # (torch asks for this before a gradient of another dtype may be assigned)
    ps[1].grad = gs[1].to(DEV, torch.float64)          # cast to a dense fp32 temporary
    ps[2].grad = gs[2].to(DEV).repeat_interleave(2)[::2]    # not contiguous: copied
    got = training.grad_norm(ps)
    ref = A.model_norm(gs[:3])
    assert got.shape == () and got.is_cuda and got.dtype == torch.float32
    assert abs(float(got) - ref) <= float(np.spacing(np.float32(ref)))
    assert torch.equal(ps[0].grad.cpu(), gs[0])


def test_refusals_on_the_device(built_lib):
    base = torch.zeros(8, 6, device=DEV)
    with pytest.raises(ValueError, match="contiguous"):
        training.ClippedAdamW([nn.Parameter(base.t())])
    p = nn.Parameter(torch.zeros(10, 4, device=DEV))
    opt = training.ClippedAdamW([p])
    p.grad = torch.sparse_coo_tensor(torch.tensor([[1], [2]]), torch.tensor([1.0]), (10, 4)).to(DEV)
    with pytest.raises(ValueError, match="sparse"):
        opt.step()
    p.grad_dtype = None                                                    # (torch asks for this before a gradient of another dtype may be assigned)
    p.grad = torch.ones(4, 10, device=DEV, dtype=torch.float64).t()        # neither fp32 nor contiguous: a dense fp32 temporary
    opt.step()
    assert float(opt.grad_norm) == pytest.approx(math.sqrt(40.0), rel=1e-6) and float(opt.state[p]["step"]) == 1.0
    opt.param_groups[0]["lr"] = -1.0
    with pytest.raises(ValueError, match="lr"):
        opt.step()


def test_handover_to_the_engine(golden, built_lib):
    """`_train_step` of tests/test_gpu_training.py on the "tiny" network, then ClippedAdamW(lr=2e-3).step(): the parameters obey the accuracy rule against the
    torch pair run on a second copy from the same gradients; `_signature` changed; after eval() the HIP engine's logits equal the oracle on the updated state
    dict within the existing test's bound and moved by more than 50 x that difference"""
    cfg, m = T.model_for("tiny", golden, DEV)
    _, m2 = T.model_for("tiny", golden, DEV)
    gen = torch.Generator().manual_seed(17)
    x = torch.randint(0, cfg["num_labels"], (2, 16, 16), generator=gen)
    r = torch.tensor([0.8, 0.3])
    c = cond_for(cfg, 2, 3, 1, G.COND_SEED + 3)
    before = m(x.to(DEV), r.to(DEV), **to_dev(c, DEV)).float().cpu().clone()
    _train_step(m, cfg)
    names = [k for k, _ in m.named_parameters()]
    p0 = {k: p.detach().cpu().double() for k, p in m.named_parameters()}
    g0 = {k: p.grad.detach().cpu().double() for k, p in m.named_parameters()}
    for (k, p), (k2, p2) in zip(m.named_parameters(), m2.named_parameters()):
        assert k == k2 and torch.equal(p, p2)
        p2.grad = p.grad.detach().clone()
    sig = m._signature()
    opt = training.ClippedAdamW(m.parameters(), lr=2e-3)
    opt.step()
    assert m._signature() != sig
    norm_t = nn.utils.clip_grad_norm_(m2.parameters(), 1.0)
    torch.optim.AdamW(m2.parameters(), lr=2e-3).step()
    norm64 = A.model_norm(g0.values())
    coef = A.model_coef(norm64, 1.0)
    hyper = dict(HYPER, lr=2e-3)
    worst, fails, tp = (-1.0, None), [], dict(m2.named_parameters())
    for k, p in m.named_parameters():
        ref, _, _ = A.model_step(p0[k], g0[k], torch.zeros_like(p0[k]), torch.zeros_like(p0[k]), 1, hyper, coef)
        ef, et, u = T.err(p.detach().cpu(), ref), T.err(tp[k].detach().cpu(), ref), T.ulp(ref)
        if ef / max(et, u) > worst[0]:
            worst = (ef / max(et, u), "%s: e(fused) %.3e e(torch) %.3e ulp %.3e" % (k, ef, et, u))
        if not T.within_yardstick(ef, et, u):
            fails.append("%s: error %.3e exceeds %gx max(torch %.3e, ulp %.3e)" % (k, ef, T.FACTOR, et, u))
    ef, et, u = abs(float(opt.grad_norm) - norm64), abs(float(norm_t) - norm64), float(np.spacing(np.float32(norm64)))
    print("train_optimizer parity handover-tiny (%d tensors): largest e(fused) / max(e(torch), ulp) = %.3f in %s; norm %.9g: e(fused) %.3e e(torch) %.3e ulp %.3e"
          % (len(names), worst[0], worst[1], norm64, ef, et, u))
    assert not fails, "\n".join(fails)
    assert T.within_yardstick(ef, et, u)
    m.eval()
    after = m(x.to(DEV), r.to(DEV), **to_dev(c, DEV)).float().cpu()
    sd_new = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref = O.unet_forward(sd_new, cfg, x, r, **c)
    diff = (after - ref).abs().max().item()
    moved = (after - before).abs().max().item()
    print("train_optimizer parity handover-tiny: HIP engine vs oracle(updated state dict) max|diff| %.2e, logits moved by %.2e" % (diff, moved))
    assert diff <= 2e-5 * max(1.0, ref.std().item())
    assert moved > 50 * diff, "the engine still serves the pre-step weights"


def test_offsets_beyond_2_to_31(built_lib):
    """a single tensor of 2^31 + C + 5 elements: constant but for a seeded slice over the last 2C elements, which straddles element 2^31.  The norm against the
    closed form; every element in front of the slice against the one value a constant input gives; the head and the slice against the model and, under the accuracy
    rule, against torch.optim.AdamW run on copies of those two pieces (max_norm = None: the coefficient is 1 on both sides)."""
    C = chunk()
    n, tail = 2 ** 31 + C + 5, 2 * C
    free = torch.cuda.mem_get_info()[0]
    if free < 48 * 2 ** 30:
        print("test_offsets_beyond_2_to_31 needs about 35 GiB and asks for 48 GiB free: %.1f GiB are" % (free / 2 ** 30))
        pytest.skip("needs 48 GiB of free device memory, %.1f GiB are free" % (free / 2 ** 30))
    gen = torch.Generator().manual_seed(113)
    p_tail, g_tail = torch.randn(tail, generator=gen) * 0.5, torch.randn(tail, generator=gen)
    p = nn.Parameter(torch.full((n,), 0.5, device=DEV))
    g = torch.full((n,), 0.25, device=DEV)
    with torch.no_grad():
        p[n - tail:] = p_tail.to(DEV)
    g[n - tail:] = g_tail.to(DEV)
    p.grad = g
    opt = training.ClippedAdamW([p], max_norm=None, **HYPER)
    opt.step()
    norm64 = math.sqrt((n - tail) * 0.25 ** 2 + float((g_tail.double() ** 2).sum()))
    assert abs(float(opt.grad_norm) - norm64) <= float(np.spacing(np.float32(norm64)))
    st = opt.state[p]
    head = 1000
    pieces = {"head": (slice(0, head), torch.full((head,), 0.5), torch.full((head,), 0.25)), "tail": (slice(n - tail, n), p_tail, g_tail)}
    for name, (sl, p0, g0) in pieces.items():
        pt = nn.Parameter(p0.to(DEV))
        pt.grad = g0.to(DEV)
        ot = torch.optim.AdamW([pt], **HYPER)
        ot.step()
        refs = A.model_step(p0.double(), g0.double(), torch.zeros(p0.numel(), dtype=torch.float64), torch.zeros(p0.numel(), dtype=torch.float64), 1, HYPER, 1.0)
        for what, gf, gt, ref in zip(("p", "exp_avg", "exp_avg_sq"), (p.detach()[sl], st["exp_avg"][sl], st["exp_avg_sq"][sl]),
                                     (pt.detach(), ot.state[pt]["exp_avg"], ot.state[pt]["exp_avg_sq"]), refs):
            ef, et, u = T.err(gf.cpu(), ref), T.err(gt.cpu(), ref), T.ulp(ref)
            print("train_optimizer parity 2^31 %s %s: e(fused) %.3e e(torch) %.3e ulp %.3e" % (name, what, ef, et, u))
            assert T.within_yardstick(ef, et, u), (name, what, ef, et, u)
    for t in (p.detach(), st["exp_avg"], st["exp_avg_sq"]):
        assert bool((t[:n - tail] == t[0]).all()), "an element in front of the seeded slice differs from element 0"
    assert bool((g[:n - tail] == 0.25).all()) and torch.equal(g[n - tail:].cpu(), g_tail)      # g is never written
    del p, g, st, opt, t
    torch.cuda.empty_cache()


def _raw_setup(sizes, seed):
    lib = _lib.load()
    C = chunk()
    init, grads = tensors(sizes, seed, 0.5), tensors(sizes, seed + 1)
    p, g = [t.to(DEV) for t in init], [t.to(DEV) for t in grads]
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    rows = np.zeros(len(sizes), dtype=train_ops.ADAMW_ROW)
    for k, ts in (("p", p), ("g", g), ("m", m), ("v", v)):
        rows[k] = [t.data_ptr() for t in ts]
    rows["n"] = sizes
    begins, n_chunks = train_ops.adamw_chunk_plan(sizes, C)
    rows["chunk_begin"] = begins
    rows["lr"], rows["beta1"], rows["beta2"], rows["eps"], rows["weight_decay"] = HYPER["lr"], *HYPER["betas"], HYPER["eps"], HYPER["weight_decay"]
    return lib, init, grads, p, g, m, v, rows, n_chunks


def _table(rows, pinned=False):
    t = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy())
    return t.pin_memory() if pinned else t.to(DEV)


def _poisoned(nbytes):
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)       # every float and double in it reads as NaN


def test_raw_abi(built_lib):
    """the C entry points on a hand-made table: norm_out and the workspace are poisoned with NaN bytes and need no set-up; a workspace one byte short and a plan
    whose chunk_begin does not ascend are refused before anything is enqueued (the plan where the host can read the table: pinned memory); the same plan in
    device memory is caught by the finalize launch and treated as a non-finite step"""
    C = chunk()
    sizes = [C + 5, 300, 2 * C]
    lib, init, grads, p, g, m, v, rows, n_chunks = _raw_setup(sizes, 114)
    need = lib.paella_adamw_workspace_bytes(len(sizes), n_chunks)
    ws, norm, steps = _poisoned(need), _poisoned(4).view(torch.float32), torch.zeros(len(sizes), device=DEV)
    stream = _lib.stream_ptr(torch.device(DEV))
    table = _table(rows)
    norm64 = A.model_norm(grads)
    # the norm alone: written, nothing else touched
    assert lib.paella_adamw_grad_norm(table.data_ptr(), len(sizes), n_chunks, norm.data_ptr(), ws.data_ptr(), need, stream) == 0
    assert abs(float(norm[0]) - norm64) <= float(np.spacing(np.float32(norm64)))
    assert [float(s) for s in steps] == [0.0] * 3 and all(torch.equal(a.cpu(), b) for a, b in zip(p, init)) and not any(bool(t.any()) for t in m + v)
    # refusals, before anything is enqueued
    ws.fill_(0xFF)
    norm.view(torch.uint8).fill_(0xFF)
    args = (len(sizes), n_chunks, 1.0, steps.data_ptr(), norm.data_ptr(), ws.data_ptr())
    assert lib.paella_adamw_step(table.data_ptr(), *args, need - 1, stream) == ERR_WORKSPACE
    bad = rows.copy()
    bad["chunk_begin"][1], bad["chunk_begin"][2] = bad["chunk_begin"][2], bad["chunk_begin"][1]
    pinned = _table(bad, pinned=True)
    assert lib.paella_adamw_step(pinned.data_ptr(), *args, need, stream) == ERR_ARG and b"chunk_begin" in lib.paella_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(norm).all()) and [float(s) for s in steps] == [0.0] * 3
    # the same plan from device memory: the finalize launch refuses it -- norm NaN, nothing updated
    assert lib.paella_adamw_step(_table(bad).data_ptr(), *args, need, stream) == 0
    assert math.isnan(float(norm[0])) and [float(s) for s in steps] == [0.0] * 3
    assert all(torch.equal(a.cpu(), b) for a, b in zip(p, init)) and not any(bool(t.any()) for t in m + v)
    # the step
    ws.fill_(0xFF)
    assert lib.paella_adamw_step(table.data_ptr(), *args, need, stream) == 0
    torch.cuda.synchronize()
    assert abs(float(norm[0]) - norm64) <= float(np.spacing(np.float32(norm64))) and [float(s) for s in steps] == [1.0] * 3
    coef = A.model_coef(norm64, 1.0)
    for i in range(len(sizes)):
        refs = A.model_step(init[i].double(), grads[i].double(), torch.zeros(sizes[i], dtype=torch.float64), torch.zeros(sizes[i], dtype=torch.float64), 1, HYPER, coef)
        for got, ref in zip((p[i], m[i], v[i]), refs):
            assert T.err(got.cpu(), ref) <= T.FACTOR * T.ulp(ref)
        assert torch.equal(g[i].cpu(), grads[i])
    # no tensor at all: the norm of nothing is 0
    assert lib.paella_adamw_step(table.data_ptr(), 0, 0, 1.0, steps.data_ptr(), norm.data_ptr(), ws.data_ptr(), need, stream) == 0
    assert float(norm[0]) == 0.0

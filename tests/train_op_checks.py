"""What the tests of the training ops (paella_amd/train_ops.py) check the same way: the error figures and the yardstick rule of the accuracy tests, and the
model-level block -- the reference's recorded training step under the tolerances of tests/test_gpu_training.py, `forward_loss` on the same route, and the hand-over
to the HIP engine, which never sees a training switch."""
import contextlib

import numpy as np
import torch
from torch import nn

import paella_amd
from oracle import golden_configs as G
from paella_amd import train_ops, training
from tests import train_step_model as S
from tests.helpers import cond_for, to_dev, weights_for

FACTOR = 4.0


def err(a, ref):
    """max abs error of a against the fp64 values ref"""
    return float((a.double() - ref).abs().max())


def ulp(ref):
    """one fp32 ulp at the largest magnitude of ref: the rounding no fp32 result can avoid"""
    return float(np.spacing(np.float32(float(ref.abs().max()))))


def within_yardstick(e_fused, e_torch, floor=0.0):
    """the accuracy rule: the fused op's error stays within FACTOR x the error MEASURED for the torch fp32 path on the same inputs, or x `floor` where that is larger"""
    return e_fused <= FACTOR * max(e_torch, floor)


def model_for(which, golden, dev):
    """(cfg, the "tiny" or "variant" network with the weights of the recorded step, on dev)"""
    cfg = G.UNET_TINY if which == "tiny" else G.UNET_VARIANT
    m = paella_amd.Paella(**cfg)
    weights_for(m, sum(cfg["blocks"]), golden("unet_%s_forward" % which))
    return cfg, m.to(dev)


def assert_recorded_step(m, g, loss, pred=None):
    """loss (and the logits, where the step has them) and the gradients m holds after one step without dropout, against the reference's record g"""
    np.testing.assert_allclose(float(loss), float(g["nodrop_loss"]), rtol=2e-5)
    if pred is not None:
        np.testing.assert_allclose(pred[:, ::4, ::2, ::2].cpu().numpy(), g["nodrop_pred_sub"], atol=5e-5, rtol=1e-4)
    params = dict(m.named_parameters())
    names = g["names"].tolist()
    norms = np.array([float(params[k].grad.norm()) for k in names])
    np.testing.assert_allclose(norms, g["nodrop_grad_norms"], rtol=5e-4, atol=1e-6)
    for k in [k for k in g.files if k.startswith("nodrop_grad:")]:
        ref = g[k]
        np.testing.assert_allclose(params[k.split(":", 1)[1]].grad.cpu().numpy(), ref, rtol=5e-4, atol=5e-4 * max(float(np.abs(ref).max()), 1e-6), err_msg=k)


def assert_switched_step_and_handover(m, cfg, g, pred, loss, flip_back, op_calls=None, calls_per_forward=0):
    """After `_train_step` of tests/test_gpu_training.py under a training switch gave (pred, loss): the recorded step; `forward_loss` takes the same route; then an
    optimizer step, back to eval, and the engine's logits are the same bits after flip_back() has put the switch back.  op_calls() reads a call counter of the op:
    forward_loss raises it by calls_per_forward, eval mode never reaches the op."""
    dev = pred.device
    assert_recorded_step(m, g, loss, pred)
    latents, t, mask, random_x, c = G.train_step_inputs(cfg)
    latents, t, mask, random_x = latents.to(dev), t.to(dev), mask.to(dev), random_x.to(dev)
    noised = latents * (1 - mask) + random_x * mask
    lw = m.get_loss_weight(t, mask)
    n0 = op_calls() if op_calls else 0
    fl, _ = m.forward_loss(noised, t, latents, **to_dev(c, dev))
    assert not op_calls or op_calls() == n0 + calls_per_forward
    np.testing.assert_allclose(float(((fl.detach() * lw).sum(dim=[1, 2]) / lw.sum(dim=[1, 2])).mean()), float(g["nodrop_loss"]), rtol=2e-5)
    opt = torch.optim.AdamW(m.parameters(), lr=2e-3)
    nn.utils.clip_grad_norm_(m.parameters(), 1.0)
    opt.step()
    m.eval()
    gen = torch.Generator().manual_seed(17)
    x = torch.randint(0, cfg["num_labels"], (2, 16, 16), generator=gen).to(dev)
    r = torch.tensor([0.8, 0.3]).to(dev)
    cc = to_dev(cond_for(cfg, 2, 3, 1, G.COND_SEED + 3), dev)
    with torch.no_grad():
        n0 = op_calls() if op_calls else 0
        with_hip = m(x, r, **cc).clone()
        flip_back()
        with_torch = m(x, r, **cc)
        assert not op_calls or op_calls() == n0
    assert torch.isfinite(with_hip).all() and torch.equal(with_hip, with_torch)


def assert_switch_leaves_a_cpu_train_step_alone(flip, before=None):
    """the switches act on a cuda device only: on the CPU a train-mode forward is the torch chain before and after flip(m), bit for bit"""
    m = paella_amd.Paella(**G.UNET_TINY)
    weights_for(m, sum(G.UNET_TINY["blocks"]))
    latents, t, mask, random_x, c = G.train_step_inputs(G.UNET_TINY)
    noised = latents * (1 - mask) + random_x * mask
    m.train()
    m.dropout = 0.0
    if before:
        before(m)
    a = m(noised, t, **c)
    flip(m)
    b = m(noised, t, **c)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# One training step on the HIP route against the fp64 mirror of tests/train_step_model.py: what tests/test_gpu_train_step_dropout.py, tests/test_gpu_mod_train.py and
# tests/test_gpu_unet_geometries.py share -- the harness that injects seeds and records the library calls, the network with its references, the step itself and
# the assertions.  The rule is stated in the docstring of tests/test_gpu_train_step_dropout.py.
# ---------------------------------------------------------------------------------------------------------------------
DEV = "cuda"
HIP, TORCH = ("hip", "hip", "hip"), ("torch", "torch", "torch")
S0 = (0xC0FFEE << 40) + 977      # high key word in use, as SEED of tests/test_gpu_attn_train.py
S1 = (0xFACADE << 40) + 31337
# name -> (config, B x H x W tokens, model.dropout): the cases of tests/test_gpu_train_step_dropout.py (tests/test_gpu_mod_train.py runs three of them)
STEP_CASES = {"recorded-tiny": ("tiny", (2, 16, 16), 0.1),                # the recorded geometry
              "recorded-variant": ("variant", (2, 16, 16), 0.1),          # F blocks, cross-attention only, patch 1
              "per-level": ("tiny", (3, 8, 24), [0.0, 0.1, 0.2]),         # B odd, P = 3 against 16 keys, a level that draws nothing
              "one-position": ("tiny", (1, 8, 8), 0.1),                   # P = 1 with C = 256, attention of 1 query against 14 keys
              "odd-variant": ("variant", (3, 4, 12), 0.1),                # P = 48 / 12, L = 9
              "head-80": ("mid", (2, 16, 16), 0.1)}                       # D = 80 with L = 17 / 29, C = 640 / 1280, skip C = 320
LOGITS, PER_POS = "<logits>", "<loss per position>"
# library entry -> (kind, direction, where (B, P, C) / (B, nhead, P, L) sit among the arguments after (entry, device, workspace bytes), where p sits; the seed follows p)
ENTRIES = {"paella_grn_act_forward": ("act", "fwd", slice(3, 6), 6), "paella_grn_act_backward": ("act", "bwd", slice(4, 7), 7),
           "paella_attn_train_forward": ("attn", "fwd", slice(6, 10), 11), "paella_attn_train_backward": ("attn", "bwd", slice(9, 13), 14)}


@contextlib.contextmanager
def deterministic_torch():
    """torch.use_deterministic_algorithms(True, warn_only=True) while it is entered.  The HIP ops use no float atomics, but what torch runs around them does in its
    default mode (its BLAS calls may combine partial sums atomically): the same step with the same seeds then gives other bits from run to run, and a gradient that
    is ONE row -- a bias at a level of one position per sample, B = 1 -- moved between 2 and 4.3 x the yardstick (measured, no_timestep at dropout 0.1:
    down_blocks.2.1.channelwise.0.bias, e 1.8e-8 ... 3.0e-8 in the default mode against 5.8e-9 in every repeat in this mode, e32 6.9e-9)."""
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)


class Harness:
    """While it is entered: the network's two dropout ops (the module globals of paella_amd.training) get seed = next(seeds) injected where p > 0 (seeds = None:
    nothing is injected, the ops draw their own), and every library call of train_ops._call is recorded as (kind, direction, dims, p, seed, address of its first
    tensor) -- the first tensor is the saved input u / q, the same object in both directions, which pairs a backward call with its forward."""

    def __init__(self, seeds=None):
        self.seeds = None if seeds is None else iter(seeds)
        self.lib_calls = []

    def __enter__(self):
        self.real = (training.gelu_grn_dropout, training.attention_dropout, train_ops._call)
        act, attn, call = self.real

        def seed_for(p, seed):
            return next(self.seeds) if self.seeds is not None and float(p) > 0.0 else seed

        def act_w(u, gamma, beta, p=0.0, seed=None):
            return act(u, gamma, beta, p, seed_for(p, seed))

        def attn_w(q, kv, nhead, p=0.0, seed=None):
            return attn(q, kv, nhead, p, seed_for(p, seed))

        def call_w(entry, dev, ws_bytes, *args):
            if entry in ENTRIES:
                kind, direction, dims, ip = ENTRIES[entry]
                self.lib_calls.append((kind, direction, tuple(int(v) for v in args[dims]), float(args[ip]), int(args[ip + 1]), args[0].data_ptr()))
            return call(entry, dev, ws_bytes, *args)

        training.gelu_grn_dropout, training.attention_dropout, train_ops._call = act_w, attn_w, call_w
        return self

    def __exit__(self, *exc):
        training.gelu_grn_dropout, training.attention_dropout, train_ops._call = self.real
        return False

    def forwards(self):
        return [c for c in self.lib_calls if c[1] == "fwd"]

    def forward_seeds(self):
        """the seeds of the forward calls that drew a mask, in call order"""
        return [c[4] for c in self.forwards() if c[3] > 0.0]


class Case:
    """One network on the device, its inputs on both sides, and what is measured once -- the fp64 mirror without dropout and the error of the "torch" route on the
    GPU at dropout 0 against it (eT).  spec: (which, (B, H, W), model.dropout) with which = "tiny" / "variant" (the weights of the recorded step) or "mid", on the
    inputs of the recorded recipe; or a dict(cfg=constructor arguments, B=, H=, W=, S_byt5=, n_img=, seed=, dropout=) -- any configuration, synthetic weights."""

    def __init__(self, name, spec, golden=None, dev=DEV):
        self.name = name
        if isinstance(spec, dict):
            self.cfg, (B, H, W), self.dropout = spec["cfg"], (spec["B"], spec["H"], spec["W"]), spec["dropout"]
            self.m = paella_amd.Paella(**self.cfg)
            self.sd = weights_for(self.m, sum(self.cfg["blocks"]))
            self.m = self.m.to(dev)
            self.inp = S.inputs(self.cfg, B, H, W, seed=spec["seed"], S_byt5=spec["S_byt5"], n_img=spec["n_img"])
        else:
            which, (B, H, W), self.dropout = spec
            if which == "mid":
                self.cfg = G.UNET_MID
                self.m = paella_amd.Paella(**self.cfg)
                self.sd = weights_for(self.m, sum(self.cfg["blocks"]))
                self.m = self.m.to(dev)
            else:
                self.cfg, self.m = model_for(which, golden, dev)
                self.sd = {k: v.detach().cpu().clone() for k, v in self.m.state_dict().items()}
            self.inp = S.inputs(self.cfg, B, H, W)
        self.grid = (H, W)
        n = len(self.cfg["c_hidden"])
        self.p_of_level = [float(v) for v in self.dropout] if isinstance(self.dropout, list) else [float(self.dropout)] * n
        latents, t, mask, random_x, c = self.inp
        self.latents, self.t, self.mask = latents.to(dev), t.to(dev), mask.to(dev)
        self.noised = (latents * (1 - mask) + random_x * mask).to(dev)
        self.c = to_dev(c, dev)
        self.mirrors, self.n_drawing = {}, None
        self.ref0 = as_dict(S.step(self.sd, self.cfg, self.inp, None, torch.float64))
        # the parameters the step reaches (all of them, unless the inputs carry no CLIP-image entry or the network has no AttnBlock: such a mapper gets no gradient
        # on either side, and assert_step_against_mirror holds the HIP route to exactly this set)
        self.names = [k for k, _ in self.m.named_parameters() if k in self.ref0]
        if not isinstance(spec, dict):      # the recorded family has a CLIP-image entry and attention: EVERY parameter must have a gradient
            assert self.names == [k for k, _ in self.m.named_parameters()], "parameters without a gradient in the mirror: %s" % sorted(
                k for k, _ in self.m.named_parameters() if k not in self.ref0)
        out = run_step(self, TORCH, dropout=0.0)
        assert not out["harness"].lib_calls, "the torch route reached a training op"
        self.eT = {k: err(out["values"][k].cpu(), self.ref0[k]) for k in self.ref0}

    def mirror(self, seeds, p_of_level=None):
        """(fp64 mirror under the models' masks for these seeds, error of the fp32 mirror under the same masks per tensor, the fp64 mirror's call record);
        p_of_level: another dropout per level than the case's own (a step run with run_step(..., dropout=...))"""
        seeds = tuple(seeds)
        p_of_level = self.p_of_level if p_of_level is None else [float(v) for v in p_of_level]
        key = (seeds, tuple(p_of_level))
        if key not in self.mirrors:
            d64 = S.model_masks(seeds, p_of_level, self.cfg, self.grid)
            ref = as_dict(S.step(self.sd, self.cfg, self.inp, d64, torch.float64))
            got32 = as_dict(S.step(self.sd, self.cfg, self.inp, S.model_masks(seeds, p_of_level, self.cfg, self.grid), torch.float32))
            assert len(seeds) == sum(1 for c in d64.calls if c[3] > 0.0), "the mirror consumed %d of %d seeds" % (sum(1 for c in d64.calls if c[3] > 0.0), len(seeds))
            self.mirrors[key] = (ref, {k: err(got32[k], ref[k]) for k in ref}, list(d64.calls))
        return self.mirrors[key]

    def n_drawing_calls(self):
        """how many op calls of one forward draw a mask: the plan is that of the mirror, whatever the seeds"""
        if self.n_drawing is None:
            d = S.model_masks(iter(range(1, 1000)), self.p_of_level, self.cfg, self.grid)
            with torch.no_grad():
                latents, t, mask, random_x, c = self.inp
                S.O.unet_forward(self.sd, self.cfg, latents * (1 - mask) + random_x * mask, t, drop=d, **c)
            self.n_drawing = sum(1 for c in d.calls if c[3] > 0.0)
        return self.n_drawing


def as_dict(stepped):
    """(pred, loss per position, loss, grads) of S.step -> one dict: the gradients by parameter name, plus LOGITS, PER_POS and "loss" """
    pred, per_pos, loss, grads = stepped
    return dict(grads, **{LOGITS: pred, PER_POS: per_pos, "loss": loss})


def run_step(case, route=HIP, dropout=None, seeds=None, fused_loss=False, zero=True, backward=True):
    """one training step of case.m under the switches `route` = (activation, depthwise, attention[, modulation]), the leading rows of training.TRAIN_SWITCHES (a
    switch the route does not reach stays as it is):
    `model(...)` + CrossEntropyLoss as _train_step of tests/test_gpu_training.py, or `forward_loss`; -> dict(values = {parameter name: its .grad, LOGITS, PER_POS,
    "loss"}, correct, harness)"""
    m = case.m
    assert len(route) in (3, 4)
    m.set_training_route(**{s.name: mode for s, mode in zip(training.TRAIN_SWITCHES, route)})
    m.train()
    m.dropout = case.dropout if dropout is None else dropout
    if zero:
        m.zero_grad(set_to_none=True)
    lw = m.get_loss_weight(case.t, case.mask)
    pred = correct = None
    with Harness(seeds) as h, torch.set_grad_enabled(backward):
        if fused_loss:
            per_pos, correct = m.forward_loss(case.noised, case.t, case.latents, **case.c)
        else:
            pred = m(case.noised, case.t, **case.c)
            per_pos = nn.CrossEntropyLoss(label_smoothing=0.1, reduction='none')(pred, case.latents)
        loss = ((per_pos * lw).sum(dim=[1, 2]) / lw.sum(dim=[1, 2])).mean()
        if backward:
            loss.backward()
    m.eval()
    values = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None} if backward else {}
    values.update({PER_POS: per_pos.detach(), "loss": loss.detach()}, **({} if pred is None else {LOGITS: pred.detach()}))
    return dict(values=values, correct=correct, harness=h)


def assert_call_protocol(case, h, mirror_calls, directions=("fwd", "bwd")):
    """the recorded library calls against the mirror's call record: number, order, kind, geometry, p and seed of the forward calls; p = 0 calls carry seed 0; and
    every forward call has exactly one backward call, with its (p, seed)"""
    fw = h.forwards()
    assert [(k, d, p) for k, _, d, p, _, _ in fw] == [(k, (s[0], s[1] * s[2], s[3]) if k == "act" else s, p) for k, s, _, p, _ in mirror_calls], \
        "the HIP route's forward calls are not the call plan of the mirror"
    assert [s for _, _, _, _, s, _ in fw] == [0 if s is None else s for _, _, _, _, s in mirror_calls], "a forward call carries another seed than the one handed out for it"
    if "bwd" in directions:
        bw = [c for c in h.lib_calls if c[1] == "bwd"]
        assert len(bw) == len(fw) and len({(c[0], c[5]) for c in fw}) == len(fw)
        by_input = {(c[0], c[5]): c for c in fw}
        for kind, _, dims, p, seed, ptr in bw:
            f = by_input.pop((kind, ptr))      # KeyError: a backward call without a forward call on that saved input, or two for one
            assert (dims, p, seed) == (f[2], f[3], f[4]), "%s backward carries (dims, p, seed) = %s, its forward %s" % (kind, (dims, p, seed), f[2:5])
        assert not by_input


def assert_within_yardstick(case, what, got, ref, e32, eT=None, keys=None, label="train_step_dropout parity"):
    """the rule of tests/test_gpu_train_step_dropout.py, e(hip route) <= FACTOR max(e32, eT, ulp), for every tensor in keys (default: every parameter and the
    logits); prints the two ratios the parity file keeps"""
    eT = case.eT if eT is None else eT
    keys = case.names + [LOGITS] if keys is None else keys
    worst, spread, fails = (0.0, None, ()), (0.0, None), []
    for k in keys:
        assert k in got, "%s %s: no value for %s" % (case.name, what, k)
        assert torch.isfinite(got[k]).all(), "%s %s %s: not finite" % (case.name, what, k)
        assert tuple(got[k].shape) == tuple(ref[k].shape), k
        e, u = err(got[k].cpu(), ref[k]), ulp(ref[k])
        yard = max(e32[k], eT[k], u)
        if e / yard > worst[0]:
            worst = (e / yard, k, (e, e32[k], eT[k], u))
        if e32[k] > 0 and eT[k] / e32[k] > spread[0]:
            spread = (eT[k] / e32[k], k)
        if not within_yardstick(e, max(e32[k], eT[k]), u):
            fails.append("%s: error %.3e exceeds %gx max(fp32 mirror %.3e, torch route %.3e, ulp %.3e)" % (k, e, FACTOR, e32[k], eT[k], u))
    rel = abs(float(got["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    print(label + " %s %s: largest e(hip) / max(e32, eT, ulp) = %.3f in %s (e %.3e e32 %.3e eT %.3e ulp %.3e); largest eT / e32 = %.2f in %s; "
          "loss %.6f, rel err %.2e" % ((case.name, what, worst[0], worst[1]) + worst[2] + (spread[0], spread[1], float(got["loss"]), rel)))
    assert not fails, "%s %s: %d tensors outside the yardstick:\n" % (case.name, what, len(fails)) + "\n".join(fails)
    np.testing.assert_allclose(float(got["loss"]), float(ref["loss"]), rtol=2e-5)


def assert_fixed_tolerances(case, got, ref):
    """train_op_checks.assert_recorded_step's tolerances, with the fp64 mirror in the place of the reference's record and every gradient in full"""
    np.testing.assert_allclose(float(got["loss"]), float(ref["loss"]), rtol=2e-5)
    if LOGITS in got:
        np.testing.assert_allclose(got[LOGITS][:, ::4, ::2, ::2].cpu().numpy(), ref[LOGITS][:, ::4, ::2, ::2].numpy(), atol=5e-5, rtol=1e-4)
    np.testing.assert_allclose(np.array([float(got[k].norm()) for k in case.names]), np.array([float(ref[k].norm()) for k in case.names]), rtol=5e-4, atol=1e-6)
    for k in case.names:
        r = ref[k].numpy()
        np.testing.assert_allclose(got[k].cpu().numpy(), r, rtol=5e-4, atol=5e-4 * max(float(np.abs(r).max()), 1e-6), err_msg=k)


def assert_step_against_mirror(case, out, seeds, what, keys=None, directions=("fwd", "bwd"), label="train_step_dropout parity", p_of_level=None):
    ref, e32, calls = case.mirror(seeds, p_of_level)
    assert_call_protocol(case, out["harness"], calls, directions)
    assert set(k for k in out["values"] if not k.startswith("<") and k != "loss") == set(case.names) == set(k for k in ref if not k.startswith("<") and k != "loss")
    assert_within_yardstick(case, what, out["values"], ref, e32, keys=keys, label=label)
    if case.name.startswith("recorded"):
        assert_fixed_tolerances(case, out["values"], ref)
    return ref


def injected(case, s0=S0):
    return [s0 + i for i in range(case.n_drawing_calls())]

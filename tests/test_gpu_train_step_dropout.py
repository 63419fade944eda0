"""GPU: one training step WITH dropout on the HIP route -- all three training switches on "hip", which is how the reference always trains (dropout 0.1) -- against
the fp64 mirror of tests/train_step_model.py, which takes its dropout masks from the CPU Philox models of the ops under the seeds the HIP route used.  The mirror
itself is pinned against the reference's recorded steps on the CPU (tests/test_train_step_model.py).

What the step is held to (training section): one seed per op call with p > 0, drawn in forward order from torch's default CPU generator; none at p = 0; the
backward call carries its forward's (p, seed); a per-level `dropout` list reaches the level it names; the 1 / (1 - p) scale is applied once.

The accuracy rule is tests/train_op_checks.within_yardstick, per parameter tensor k (and for the logits and the per-position loss), e(x) = max|x - fp64 mirror|:
    e(hip route) <= 4 max(e32_k, eT_k, ulp_k)
e32_k: the fp32 CPU mirror under the SAME masks; eT_k: this model's "torch" route on the GPU at dropout 0 against the fp64 mirror without dropout at the same geometry
(measured once per case); ulp_k: one fp32 ulp at max|ref_k|.  Both yardsticks are references, never the code under test.  The loss scalar keeps rtol 2e-5, and at the
recorded geometries the fixed tolerances of train_op_checks.assert_recorded_step hold against the mirror as well.  The measured ratios are kept in
profiles/train_step_dropout_parity.txt."""
import numpy as np
import pytest
import torch
from torch import nn

import paella_amd
from oracle import golden_configs as G
from paella_amd import train_ops, training
from tests import train_op_checks as T
from tests import train_step_model as S
from tests.helpers import cond_for, to_dev, weights_for

pytestmark = pytest.mark.gpu
DEV = "cuda"
HIP, TORCH = ("hip", "hip", "hip"), ("torch", "torch", "torch")
S0 = (0xC0FFEE << 40) + 977      # high key word in use, as SEED of tests/test_gpu_attn_train.py
S1 = (0xFACADE << 40) + 31337
# name -> (config, B x H x W tokens, model.dropout)
CASES = {"recorded-tiny": ("tiny", (2, 16, 16), 0.1),                # the recorded geometry
         "recorded-variant": ("variant", (2, 16, 16), 0.1),          # F blocks, cross-attention only, patch 1
         "per-level": ("tiny", (3, 8, 24), [0.0, 0.1, 0.2]),         # B odd, P = 3 against 16 keys, a level that draws nothing
         "one-position": ("tiny", (1, 8, 8), 0.1),                   # P = 1 with C = 256, attention of 1 query against 14 keys
         "odd-variant": ("variant", (3, 4, 12), 0.1),                # P = 48 / 12, L = 9
         "head-80": ("mid", (2, 16, 16), 0.1)}                       # D = 80 with L = 17 / 29, C = 640 / 1280, skip C = 320
ALL = list(CASES)
LOGITS, PER_POS = "<logits>", "<loss per position>"
# library entry -> (kind, direction, where (B, P, C) / (B, nhead, P, L) sit among the arguments after (entry, device, workspace bytes), where p sits; the seed follows p)
ENTRIES = {"paella_grn_act_forward": ("act", "fwd", slice(3, 6), 6), "paella_grn_act_backward": ("act", "bwd", slice(4, 7), 7),
           "paella_attn_train_forward": ("attn", "fwd", slice(6, 10), 11), "paella_attn_train_backward": ("attn", "bwd", slice(9, 13), 14)}


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
    """One row of CASES: the network on the device, its inputs on both sides, and what is measured once -- the fp64 mirror without dropout and the error of the
    "torch" route on the GPU at dropout 0 against it (eT)."""

    def __init__(self, name, golden):
        which, (B, H, W), self.dropout = CASES[name]
        self.name, self.grid = name, (H, W)
        if which == "mid":
            self.cfg = G.UNET_MID
            self.m = paella_amd.Paella(**self.cfg)
            self.sd = weights_for(self.m, sum(self.cfg["blocks"]))
            self.m = self.m.to(DEV)
        else:
            self.cfg, self.m = T.model_for(which, golden, DEV)
            self.sd = {k: v.detach().cpu().clone() for k, v in self.m.state_dict().items()}
        n = len(self.cfg["c_hidden"])
        self.p_of_level = [float(v) for v in self.dropout] if isinstance(self.dropout, list) else [float(self.dropout)] * n
        self.names = [k for k, _ in self.m.named_parameters()]
        self.inp = S.inputs(self.cfg, B, H, W)
        latents, t, mask, random_x, c = self.inp
        self.latents, self.t, self.mask = latents.to(DEV), t.to(DEV), mask.to(DEV)
        self.noised = (latents * (1 - mask) + random_x * mask).to(DEV)
        self.c = to_dev(c, DEV)
        self.mirrors, self.n_drawing = {}, None
        self.ref0 = as_dict(S.step(self.sd, self.cfg, self.inp, None, torch.float64))
        out = run_step(self, TORCH, dropout=0.0)
        assert not out["harness"].lib_calls, "the torch route reached a training op"
        self.eT = {k: T.err(out["values"][k].cpu(), self.ref0[k]) for k in self.ref0}

    def mirror(self, seeds):
        """(fp64 mirror under the models' masks for these seeds, error of the fp32 mirror under the same masks per tensor, the fp64 mirror's call record)"""
        seeds = tuple(seeds)
        if seeds not in self.mirrors:
            d64 = S.model_masks(seeds, self.p_of_level, self.cfg, self.grid)
            ref = as_dict(S.step(self.sd, self.cfg, self.inp, d64, torch.float64))
            got32 = as_dict(S.step(self.sd, self.cfg, self.inp, S.model_masks(seeds, self.p_of_level, self.cfg, self.grid), torch.float32))
            assert len(seeds) == sum(1 for c in d64.calls if c[3] > 0.0), "the mirror consumed %d of %d seeds" % (sum(1 for c in d64.calls if c[3] > 0.0), len(seeds))
            self.mirrors[seeds] = (ref, {k: T.err(got32[k], ref[k]) for k in ref}, list(d64.calls))
        return self.mirrors[seeds]

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
    """one training step of case.m under the three switches `route` = (activation, depthwise, attention): `model(...)` + CrossEntropyLoss as _train_step of
    tests/test_gpu_training.py, or `forward_loss`; -> dict(values = {parameter name: its .grad, LOGITS, PER_POS, "loss"}, correct, harness)"""
    m = case.m
    m.set_training_activation(route[0]).set_training_depthwise(route[1]).set_training_attention(route[2])
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


def assert_within_yardstick(case, what, got, ref, e32, eT=None, keys=None):
    """the module docstring's rule for every tensor in keys (default: every parameter and the logits); prints the two ratios the parity file keeps"""
    eT = case.eT if eT is None else eT
    keys = case.names + [LOGITS] if keys is None else keys
    worst, spread, fails = (0.0, None, ()), (0.0, None), []
    for k in keys:
        assert k in got, "%s %s: no value for %s" % (case.name, what, k)
        assert torch.isfinite(got[k]).all(), "%s %s %s: not finite" % (case.name, what, k)
        assert tuple(got[k].shape) == tuple(ref[k].shape), k
        e, ulp = T.err(got[k].cpu(), ref[k]), T.ulp(ref[k])
        yard = max(e32[k], eT[k], ulp)
        if e / yard > worst[0]:
            worst = (e / yard, k, (e, e32[k], eT[k], ulp))
        if e32[k] > 0 and eT[k] / e32[k] > spread[0]:
            spread = (eT[k] / e32[k], k)
        if not T.within_yardstick(e, max(e32[k], eT[k]), ulp):
            fails.append("%s: error %.3e exceeds %gx max(fp32 mirror %.3e, torch route %.3e, ulp %.3e)" % (k, e, T.FACTOR, e32[k], eT[k], ulp))
    rel = abs(float(got["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    print("train_step_dropout parity %s %s: largest e(hip) / max(e32, eT, ulp) = %.3f in %s (e %.3e e32 %.3e eT %.3e ulp %.3e); largest eT / e32 = %.2f in %s; "
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


def assert_step_against_mirror(case, out, seeds, what, keys=None, directions=("fwd", "bwd")):
    ref, e32, calls = case.mirror(seeds)
    assert_call_protocol(case, out["harness"], calls, directions)
    assert set(k for k in out["values"] if not k.startswith("<") and k != "loss") == set(case.names) == set(k for k in ref if not k.startswith("<") and k != "loss")
    assert_within_yardstick(case, what, out["values"], ref, e32, keys=keys)
    if case.name.startswith("recorded"):
        assert_fixed_tolerances(case, out["values"], ref)
    return ref


@pytest.fixture(scope="module")
def cases(golden, built_lib):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, golden)
        return made[name]

    yield get
    made.clear()
    torch.cuda.empty_cache()


def injected(case, s0=S0):
    return [s0 + i for i in range(case.n_drawing_calls())]


@pytest.mark.parametrize("name", ALL)
def test_step_with_injected_seeds_matches_the_fp64_mirror(cases, name):
    """model(...) + CrossEntropyLoss with seed S0 + i handed to the i-th op call that draws: loss, all logits and every gradient against the mirror under the
    models' masks for those seeds; the library calls are the mirror's call plan, and each backward call carries the (p, seed) of its forward."""
    case = cases(name)
    seeds = injected(case)
    assert len(seeds) >= 3
    out = run_step(case, seeds=iter(seeds))
    ref = assert_step_against_mirror(case, out, seeds, "injected seeds")
    # dropout is visible in what was compared: the mirror without it is far outside the same yardstick (so the masks, not just the network, were checked)
    _, e32, _ = case.mirror(seeds)
    moved = [k for k in case.names if T.err(case.ref0[k], ref[k]) > 10 * T.FACTOR * max(e32[k], case.eT[k], T.ulp(ref[k]))]
    assert len(moved) > 0.9 * len(case.names), "dropout moved only %d of %d gradients clearly" % (len(moved), len(case.names))


@pytest.mark.parametrize("name", ["recorded-tiny", "per-level"])
def test_step_with_default_seeds(cases, name):
    """Nothing injected: the ops draw their seeds from torch's default CPU generator.  The seeds of the calls that draw are pairwise distinct, p = 0 calls carry seed
    0, and the mirror fed with the CAPTURED seeds agrees as under injected ones; torch.manual_seed reproduces seeds and gradients bit for bit (torch's own backward
    kernels under use_deterministic_algorithms, as test_train_step_with_dropout_is_reproducible_under_manual_seed), another seed gives other seeds."""
    case = cases(name)
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        torch.manual_seed(11)
        a = run_step(case)
        torch.manual_seed(11)
        b = run_step(case)
        torch.manual_seed(12)
        c = run_step(case, backward=False)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)
    seeds = a["harness"].forward_seeds()
    assert len(seeds) == case.n_drawing_calls() and len(set(seeds)) == len(seeds), "two op calls of one step share a seed"
    assert all(s == 0 for _, _, _, p, s, _ in a["harness"].forwards() if p == 0.0)
    assert_step_against_mirror(case, a, seeds, "default seeds")
    assert b["harness"].forward_seeds() == seeds
    assert a["values"].keys() == b["values"].keys()
    for k, v in a["values"].items():
        assert torch.equal(v, b["values"][k]), k
    other = c["harness"].forward_seeds()
    assert len(other) == len(seeds) and not set(other) & set(seeds)


@pytest.mark.parametrize("name", ["recorded-tiny", "head-80"])
def test_forward_loss_with_injected_seeds_matches_the_fp64_mirror(cases, name):
    """forward_loss -- all four training ops in one graph -- under the same seeds: the per-position loss and, after backward of the weighted mean, every gradient
    against the mirror; `correct` is the mirror's pred.argmax(1) == target except where the mirror's top-2 margin is below 1e-4 (counted, helpers.argmax_report)."""
    case = cases(name)
    seeds = injected(case)
    out = run_step(case, seeds=iter(seeds), fused_loss=True)
    ref = assert_step_against_mirror(case, out, seeds, "forward_loss", keys=case.names + [PER_POS])
    top2 = ref[LOGITS].topk(2, dim=1).values
    near = (top2[:, 0] - top2[:, 1]) < 1e-4
    mism = out["correct"].cpu() != (ref[LOGITS].argmax(1) == case.inp[0])
    print("%s forward_loss: `correct` differs at %d positions with a clear margin and %d of %d near-ties" % (name, int((mism & ~near).sum()), int((mism & near).sum()), int(near.sum())))
    assert out["correct"].dtype == torch.bool and int((mism & ~near).sum()) == 0


def test_partial_route_matches_the_fp64_mirror(cases):
    """activation and attention on "hip", the ResBlock front on "torch": the front draws nothing, so the same mirror applies (bit equality with the full route is
    not asked for)"""
    case = cases("recorded-tiny")
    seeds = injected(case)
    out = run_step(case, ("hip", "torch", "hip"), seeds=iter(seeds))
    assert_step_against_mirror(case, out, seeds, "depthwise on torch")


def test_accumulation_over_two_micro_steps(cases):
    """two backward passes under two seed sets without zero_grad in between: the ops WRITE their gradients and autograd accumulates them, so every .grad is the sum
    of the two mirrors' gradients; the yardsticks of the two steps are added"""
    case = cases("recorded-tiny")
    sa, sb = injected(case, S0), injected(case, S1)
    first = run_step(case, seeds=iter(sa))
    second = run_step(case, seeds=iter(sb), zero=False)
    (ra, ea, calls_a), (rb, eb, calls_b) = case.mirror(sa), case.mirror(sb)
    assert_call_protocol(case, first["harness"], calls_a)
    assert_call_protocol(case, second["harness"], calls_b)
    ref = {k: ra[k] + rb[k] for k in case.names}
    ref["loss"] = rb["loss"]
    assert min(T.err(ra[k], rb[k]) / float(ra[k].abs().max()) for k in case.names) > 1e-3      # the two steps differ in every gradient
    assert_within_yardstick(case, "two micro-steps", second["values"], ref, {k: ea[k] + eb[k] for k in case.names}, {k: 2 * case.eT[k] for k in case.names}, keys=case.names)


def test_back_to_eval_after_dropout_steps(golden, built_lib):
    """after a step with dropout on the HIP route and an optimizer step, eval-mode logits are finite and the same bits before and after the three switches go back:
    the HIP inference engine never sees them (the tail of train_op_checks.assert_switched_step_and_handover)"""
    case = Case("recorded-tiny", golden)
    m, cfg = case.m, case.cfg
    run_step(case, seeds=iter(injected(case)))
    opt = torch.optim.AdamW(m.parameters(), lr=2e-3)
    nn.utils.clip_grad_norm_(m.parameters(), 1.0)
    opt.step()
    m.eval()
    m.set_training_activation("hip").set_training_depthwise("hip").set_training_attention("hip")
    gen = torch.Generator().manual_seed(17)
    x = torch.randint(0, cfg["num_labels"], (2, 16, 16), generator=gen).to(DEV)
    r = torch.tensor([0.8, 0.3]).to(DEV)
    cc = to_dev(cond_for(cfg, 2, 3, 1, G.COND_SEED + 3), DEV)
    with torch.no_grad(), Harness() as h:
        with_hip = m(x, r, **cc).clone()
        m.set_training_activation("torch").set_training_depthwise("torch").set_training_attention("torch")
        with_torch = m(x, r, **cc)
    assert not h.lib_calls, "eval mode reached a training op"
    assert torch.isfinite(with_hip).all() and torch.equal(with_hip, with_torch)

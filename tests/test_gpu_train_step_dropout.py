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
import pytest
import torch
from torch import nn

from oracle import golden_configs as G
from tests import train_op_checks as T
from tests.helpers import cond_for, to_dev
from tests.train_op_checks import DEV, LOGITS, PER_POS, S0, S1, Case, Harness, assert_call_protocol, assert_step_against_mirror, assert_within_yardstick, injected, run_step

pytestmark = pytest.mark.gpu
CASES = T.STEP_CASES
ALL = list(CASES)


@pytest.fixture(scope="module")
def cases(golden, built_lib):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, CASES[name], golden)
        return made[name]

    yield get
    made.clear()
    torch.cuda.empty_cache()


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
    case = Case("recorded-tiny", CASES["recorded-tiny"], golden)
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

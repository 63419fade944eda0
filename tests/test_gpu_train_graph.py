"""GPU: the captured training iteration -- the device-side seed table (`TrainSeeds`), the two dropout ops under a device seed, `forward_loss(seeds=)`,
`ClippedAdamW` in three parts and `GraphTrainStep` -- against the CPU model of the table (tests/train_seeds_model.py) and against the EAGER iteration, which is the
reference everywhere below and never the other way round.

The parity rule of a replayed run (test_replay_equals_eager, test_staleness_recaptures): the eager side -- `forward_loss` under a `Harness` that injects the ints of
the same table state, backward, `ClippedAdamW.step()`, `scheduler.step()`, `zero_grad` -- is run TWICE.  Where it repeats itself bit for bit, every replayed
parameter, exp_avg, exp_avg_sq, step count, loss and grad_norm must be torch.equal to it; otherwise the relative L2 distance of replay to eager is at most
4 x max(eager-to-eager distance, 2^-24) per tensor (4: train_op_checks.FACTOR).  The branch that held and the largest ratio are printed
("train_graph parity ...") and kept in profiles/train_graph_parity.txt."""
import warnings

import pytest
import torch

import paella_amd
from oracle import golden_configs as G
from paella_amd import train_ops, training
from tests import train_op_checks as T
from tests import train_seeds_model as M
from tests.helpers import cond_for, to_dev
from tests.train_op_checks import DEV, S0, S1, Case, Harness

pytestmark = pytest.mark.gpu
ALL_ON = dict(activation="hip", depthwise="hip", attention="hip", modulation="hip", gemm="bf16")
FP32 = dict(ALL_ON, gemm="fp32")
MASK64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def cases(golden, built_lib):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, T.STEP_CASES[name], golden)
        return made[name]

    yield get
    made.clear()
    torch.cuda.empty_cache()


def word_tensor(s):
    s &= MASK64
    return torch.tensor([s - (1 << 64) if s >> 63 else s], dtype=torch.int64, device=DEV)


def switch(m, **kw):
    return m.set_training_route(**kw)


def fresh_model(case, switches=ALL_ON, dropout=None):
    """a new module with the case's weights, in train mode under the given switches: the tests below write to it"""
    m = paella_amd.Paella(**case.cfg)
    m.load_state_dict(case.sd)
    m = switch(m.to(DEV), **switches)
    m.train()
    m.dropout = case.dropout if dropout is None else dropout
    return m


def loss_weight(case, m):
    return m.get_loss_weight(case.t, case.mask)


def reduce_loss(per_pos, lw):
    return per_pos.mean() if lw is None else ((per_pos * lw).sum(dim=[1, 2]) / lw.sum(dim=[1, 2])).mean()


def forward_backward(m, case, lw, seeds=None, ints=None):
    """one eager forward_loss + backward of m: under a seed table, or under a Harness that injects ints; -> (per-position loss, loss, harness)"""
    with Harness(None if ints is None else iter(ints)) as h:
        per_pos, _ = m.forward_loss(case.noised, case.t, case.latents, **case.c, seeds=seeds)
        loss = reduce_loss(per_pos, lw)
        loss.backward()
    return per_pos.detach(), loss.detach(), h


def example_inputs(case, lw):
    return dict(dict(noised=case.noised, t=case.t, latents=case.latents, **case.c), **({} if lw is None else dict(loss_weight=lw)))


def snapshot(m, opt, extra=()):
    out = {}
    for k, p in m.named_parameters():
        out["p:" + k] = p.detach().clone()
        for s in ("exp_avg", "exp_avg_sq", "step"):
            if s in opt.state.get(p, {}):
                out[s + ":" + k] = opt.state[p][s].detach().clone()
    out.update(extra)
    return out


def make_optimizer(m, lr=1e-3):
    opt = training.ClippedAdamW(m.parameters(), lr=lr, weight_decay=0.01)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: 1.0 / (1 + k))
    return opt, sched


def eager_run(case, switches, base, n_iter, with_lw, hooks=None, table=False):
    """n_iter eager iterations from the case's weights; iteration k (from 1) draws under the ints of the table state (base, k) -- table: under a `TrainSeeds` of that
    base, advanced once per iteration, instead; hooks[k](m) runs before it"""
    m = fresh_model(case, switches)
    opt, sched = make_optimizer(m)
    lw = loss_weight(case, m) if with_lw else None
    extra = {}
    seeds = training.TrainSeeds(training.dropout_sites(m), base, DEV) if table else None
    for k in range(1, n_iter + 1):
        if hooks and k in hooks:
            hooks[k](m)
        if table:
            _, loss, _ = forward_backward(m, case, lw, seeds=seeds.advance())
        else:
            _, loss, _ = forward_backward(m, case, lw, ints=M.words(base, k, training.dropout_sites(m)))
        opt.step()
        extra["loss%d" % k], extra["norm%d" % k] = loss.clone(), opt.grad_norm.clone()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sched.step()
        m.zero_grad(set_to_none=True)
    return snapshot(m, opt, extra)


def graph_run(case, switches, base, n_iter, with_lw, hooks=None):
    m = fresh_model(case, switches)
    opt, sched = make_optimizer(m)
    lw = loss_weight(case, m) if with_lw else None
    step = training.GraphTrainStep(m, opt, example_inputs(case, lw), seed=base)
    extra = {}
    for k in range(1, n_iter + 1):
        if hooks and k in hooks:
            hooks[k](m)
        loss, _, norm = step(noised=case.noised, t=case.t, latents=case.latents)
        extra["loss%d" % k], extra["norm%d" % k] = loss.clone(), norm.clone()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sched.step()
    assert step.seeds.iteration == n_iter
    return snapshot(m, opt, extra), step


def rel_l2(a, ref):
    a, ref = a.double().flatten(), ref.double().flatten()
    d, n = float((a - ref).norm()), float(ref.norm())
    return 0.0 if d == 0.0 else d / n if n > 0.0 else float("inf")


def assert_replay_matches_eager(what, replay, eager_a, eager_b):
    """the rule of the module docstring"""
    assert replay.keys() == eager_a.keys() == eager_b.keys()
    for k, v in eager_a.items():
        assert torch.isfinite(v).all(), k
    repeats = all(torch.equal(eager_a[k], eager_b[k]) for k in eager_a)
    if repeats:
        diff = [k for k in eager_a if not torch.equal(replay[k], eager_a[k])]
        print("train_graph parity %s: the eager side repeats itself bit for bit; %d of %d tensors of the replayed run differ from it%s"
              % (what, len(diff), len(eager_a), "" if not diff else " (largest relative L2 distance %.3e in %s)" % max((rel_l2(replay[k], eager_a[k]), k) for k in diff)))
        assert not diff, "%s: %d tensors differ from the eager run, e.g. %s" % (what, len(diff), diff[:4])
        return
    worst, fails = (0.0, None), []
    for k in eager_a:
        yard = max(rel_l2(eager_b[k], eager_a[k]), 2.0 ** -24)
        e = rel_l2(replay[k], eager_a[k])
        if e / yard > worst[0]:
            worst = (e / yard, "%s (replay-to-eager %.3e, eager-to-eager %.3e)" % (k, e, rel_l2(eager_b[k], eager_a[k])))
        if e > T.FACTOR * yard:
            fails.append("%s: %.3e > %g x %.3e" % (k, e, T.FACTOR, yard))
    print("train_graph parity %s: the eager side does NOT repeat itself bit for bit; largest replay-to-eager / max(eager-to-eager, 2^-24) = %.3f in %s" % ((what,) + worst))
    assert not fails, "%s: %d tensors outside the rule:\n%s" % (what, len(fails), "\n".join(fails[:10]))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the seed table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sites", [1, 5, 300, 4096])
def test_seed_table_equals_the_cpu_model(built_lib, n_sites):
    t = training.TrainSeeds(n_sites, S0, DEV)
    model = M.Table(n_sites, S0)
    assert t.iteration == 0 and t.base == S0 and t.values() == [0] * n_sites
    for it in (1, 2, 3):
        assert t.advance().iteration == it
        assert t.values() == model.advance().values(), "n_sites %d, iteration %d" % (n_sites, it)
    t.set_base(S1)
    assert t.base == S1 and t.iteration == 3
    assert t.advance().values() == M.words(S1, 4, n_sites) and t.iteration == 4
    snap = t.snapshot()
    t.advance().advance()
    assert t.restore(snap).iteration == 4 and t.advance().values() == M.words(S1, 5, n_sites)
    # grown in place: the same object, base and iteration kept, and a word does not depend on the size of the table
    assert t.grow(n_sites + 7) is t and t.n_sites == n_sites + 7 and t.base == S1 and t.iteration == 5
    assert t.advance().values() == M.words(S1, 6, n_sites + 7)
    with pytest.raises(ValueError, match="grows"):
        t.grow(n_sites)
    n_sites += 7
    # the sites of a forward: views of the words, in order, and a refusal past the end
    t.begin()
    first = t.site()
    assert first.dtype == torch.int64 and first.numel() == 1 and first.data_ptr() == t.state.data_ptr() + 16 and int(first) & MASK64 == t.values()[0]
    for _ in range(n_sites - 1):
        t.site()
    assert t.used == n_sites
    with pytest.raises(RuntimeError, match="sites"):
        t.site()


def test_seed_table_draws_its_base_from_torchs_cpu_generator(built_lib):
    torch.manual_seed(5)
    a = training.TrainSeeds(3, None, DEV).base
    torch.manual_seed(5)
    b = training.TrainSeeds(3, None, DEV).base
    c = training.TrainSeeds(3, None, DEV).base
    assert a == b != c


# ---------------------------------------------------------------------------------------------------------------------
# 2. the ops under a device seed
# ---------------------------------------------------------------------------------------------------------------------
def _act_call(seed, dz=None):
    g = torch.Generator().manual_seed(3)
    u, gamma, beta = (torch.randn(s, generator=g).to(DEV).requires_grad_() for s in ((2, 16, 64), (64,), (64,)))
    z = training.gelu_grn_dropout(u, gamma, beta, 0.1, seed)
    z.backward(torch.randn(z.shape, generator=g).to(DEV))
    return z.detach(), u.grad, gamma.grad, beta.grad


def _attn_call(seed):
    g = torch.Generator().manual_seed(4)
    q, kv = (torch.randn(s, generator=g).to(DEV).requires_grad_() for s in ((2, 16, 32), (2, 9, 64)))      # B=2, nhead=2, P=16, L=9, D=16
    o = training.attention_dropout(q, kv, 2, 0.1, seed)
    o.backward(torch.randn(o.shape, generator=g).to(DEV))
    return o.detach(), q.grad, kv.grad


@pytest.mark.parametrize("op", [_act_call, _attn_call], ids=["gelu_grn_dropout", "attention_dropout"])
@pytest.mark.parametrize("s", [S0, (1 << 63) | 12345], ids=["S0", "top-bit"])
def test_op_under_a_device_seed_equals_the_by_value_call(built_lib, op, s):
    by_value = op(s)
    word = word_tensor(s)
    by_word = op(word)
    for a, b in zip(by_value, by_word):
        assert torch.equal(a, b)
    # rewriting the word changes the mask: the kernels read it when they run
    word.copy_(word_tensor(s ^ 0x55))
    moved = op(word)
    assert not torch.equal(moved[0], by_word[0])
    for a, b in zip(op(s ^ 0x55), moved):
        assert torch.equal(a, b)
    # a word in the middle of a table (8-byte, not 16-byte aligned) serves as well
    table = torch.zeros(4, dtype=torch.int64, device=DEV)
    table[3:4].copy_(word_tensor(s))
    for a, b in zip(by_value, op(table[3:4])):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="device"):
        op(word.cpu())


def test_a_host_seed_is_refused_inside_a_capture(built_lib):
    u, gamma, beta = torch.randn(2, 16, 64, device=DEV), torch.randn(64, device=DEV), torch.randn(64, device=DEV)
    q, kv = torch.randn(2, 16, 32, device=DEV), torch.randn(2, 9, 64, device=DEV)
    eager = training.gelu_grn_dropout(u, gamma, beta, 0.1, S0)
    torch.cuda.synchronize()
    calls = []
    real = train_ops._call
    train_ops._call = lambda *a: calls.append(a[0]) or real(*a)
    try:
        for run in (lambda: training.gelu_grn_dropout(u, gamma, beta, 0.1), lambda: training.attention_dropout(q, kv, 2, 0.1)):
            graph = torch.cuda.CUDAGraph()
            with pytest.raises(RuntimeError, match="capturing"):
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    doubled = u * 2.0            # (something for the graph to hold: the refusal leaves it otherwise empty)
                    run()
            del graph, doubled
        assert not calls, "the refused call reached the library: %s" % calls
        # at p = 0 nothing is drawn and a capture is what it was
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            z0 = training.gelu_grn_dropout(u, gamma, beta, 0.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(z0, training.gelu_grn_dropout(u, gamma, beta, 0.0))
    finally:
        train_ops._call = real
    # the capture was abandoned cleanly: a plain eager call afterwards is what it was before
    assert torch.equal(training.gelu_grn_dropout(u, gamma, beta, 0.1, S0), eager)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the network under a seed table, eager
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,switches", [("recorded-tiny", ALL_ON), ("per-level", FP32)])
def test_network_under_a_seed_table_equals_injected_ints(cases, name, switches):
    case = cases(name)
    m = fresh_model(case, switches)
    lw = loss_weight(case, m)
    n = training.dropout_sites(m)
    assert n == case.n_drawing_calls()
    table = training.TrainSeeds(n, S1, DEV).advance()
    ints = table.values()
    assert ints == M.words(S1, 1, n)
    with T.deterministic_torch():
        per_pos_a, loss_a, h = forward_backward(m, case, lw, seeds=table)
        grads_a = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
        assert table.used == n and table.iteration == 1
        # (the Harness records the by-value entry points only: under a seed table no call that draws goes through one)
        assert all(c[3] == 0.0 for c in h.lib_calls), [c for c in h.lib_calls if c[3] > 0.0]
        m.zero_grad(set_to_none=True)
        per_pos_b, loss_b, h = forward_backward(m, case, lw, ints=ints)
    assert h.forward_seeds() == ints
    if name == "per-level":        # the level at p = 0 consumed no site: its calls went by value with seed 0, and there are such calls
        assert any(c[3] == 0.0 for c in h.forwards()) and all(c[4] == 0 for c in h.forwards() if c[3] == 0.0)
    assert torch.equal(per_pos_a, per_pos_b) and torch.equal(loss_a, loss_b)
    assert set(grads_a) == set(k for k, p in m.named_parameters() if p.grad is not None)
    for k, p in m.named_parameters():
        assert torch.equal(grads_a[k], p.grad), k
    # a table that is too small is refused
    if n > 1:
        with pytest.raises(RuntimeError, match="sites"):
            m.forward_loss(case.noised, case.t, case.latents, **case.c, seeds=training.TrainSeeds(n - 1, S1, DEV).advance())


# ---------------------------------------------------------------------------------------------------------------------
# 4. replay equals eager
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,switches,with_lw", [("recorded-tiny", ALL_ON, True), ("per-level", FP32, False)])
def test_replay_equals_eager(cases, name, switches, with_lw):
    """three GraphTrainStep calls with the lr changed by a LambdaLR between them against three eager iterations under the injected ints of the same table state"""
    case = cases(name)
    with T.deterministic_torch():
        eager_a = eager_run(case, switches, S0, 3, with_lw)
        eager_b = eager_run(case, switches, S0, 3, with_lw)
        replay, step = graph_run(case, switches, S0, 3, with_lw)
    assert step.captures == 1
    assert not torch.equal(eager_a["loss1"], eager_a["loss2"])
    assert_replay_matches_eager("%s gemm %s" % (name, switches["gemm"]), replay, eager_a, eager_b)


class _Larger:
    """the recorded-tiny network on 2 x 40x40 = 3200 tokens: above training.EMBEDDING_CHUNK, where torch's embedding backward changes form"""

    def __init__(self, case):
        from tests import train_step_model as S
        self.cfg, self.sd, self.dropout = case.cfg, case.sd, case.dropout
        latents, t, mask, random_x, c = S.inputs(case.cfg, 2, 40, 40)
        self.latents, self.t, self.mask = latents.to(DEV), t.to(DEV), mask.to(DEV)
        self.noised = (latents * (1 - mask) + random_x * mask).to(DEV)
        self.c = to_dev(c, DEV)


def test_replay_above_the_embedding_threshold(cases):
    """More than EMBEDDING_CHUNK tokens: under a seed table the token embedding is looked up in pieces, because a replay of a graph that held the sorting form of
    torch's embedding backward ended in a GPU memory fault (cause not established; training._token_embedding).  (a) Two replays against two EAGER iterations under a seed table of the same base -- the same pieces -- by the
    rule of test_replay_equals_eager.  (b) Eager, the pieces against the one-piece default under injected ints: every gradient but the embedding weight's is
    torch.equal.  (c) The embedding weight's gradient at the op, under a gradient known here: it differs from the one-piece call by summation order only, so each
    element lies within n 2^-24 sum|g_i| of the fp64 sum over the n tokens of its label (a recursive fp32 sum of n terms, in any order and any grouping, is within
    (n - 1) 2^-24 sum|g_i| to first order); a label seen once gets the same bits, a label never seen zero."""
    big = _Larger(cases("recorded-tiny"))
    assert big.noised.numel() > training.EMBEDDING_CHUNK
    with T.deterministic_torch():
        eager_a = eager_run(big, ALL_ON, S0, 2, True, table=True)
        eager_b = eager_run(big, ALL_ON, S0, 2, True, table=True)
        replay, step = graph_run(big, ALL_ON, S0, 2, True)
        assert step.captures == 1
        assert_replay_matches_eager("recorded-tiny weights at 2 x 40x40 tokens (embedding in pieces)", replay, eager_a, eager_b)
        m = fresh_model(big)
        lw = loss_weight(big, m)
        n = training.dropout_sites(m)
        table = training.TrainSeeds(n, S1, DEV).advance()
        forward_backward(m, big, lw, seeds=table)
        pieces = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
        m.zero_grad(set_to_none=True)
        forward_backward(m, big, lw, ints=table.values())
    emb = "in_mapper.0.weight"
    for k, p in m.named_parameters():
        if k != emb:
            assert torch.equal(pieces[k], p.grad), k
    assert torch.isfinite(pieces[emb]).all() and not torch.equal(pieces[emb], torch.zeros_like(pieces[emb]))
    # the embedding weight's gradient, at the op: the pieces against one piece under a gradient that is known here
    gen = torch.Generator().manual_seed(5)
    x = big.noised
    w = torch.randn(big.cfg["num_labels"], 16, generator=gen).to(DEV).requires_grad_()
    g = torch.randn(*x.shape, 16, generator=gen).to(DEV)
    out = training._token_embedding(x, w, True)
    assert torch.equal(out, torch.nn.functional.embedding(x, w)) and torch.equal(training._token_embedding(x, w, False), out)
    out.backward(g)
    got, w.grad = w.grad.clone(), None
    torch.nn.functional.embedding(x, w).backward(g)
    one = w.grad
    counts = torch.bincount(x.flatten().cpu(), minlength=w.size(0)).double()
    sum_abs = torch.zeros(w.size(0), 16, dtype=torch.float64).index_add_(0, x.flatten().cpu(), g.reshape(-1, 16).abs().double().cpu())
    exact = torch.zeros(w.size(0), 16, dtype=torch.float64).index_add_(0, x.flatten().cpu(), g.reshape(-1, 16).double().cpu())
    bound = counts[:, None] * 2.0 ** -24 * sum_abs                 # one recursive fp32 sum of n terms against the exact sum
    e_got, e_one = (got.double().cpu() - exact).abs(), (one.double().cpu() - exact).abs()
    print("train_graph parity embedding in pieces at 3200 tokens: largest error / bound %.3f in pieces, %.3f in one piece (largest count of one label %d)"
          % (float((e_got / bound.clamp_min(1e-300)).max()), float((e_one / bound.clamp_min(1e-300)).max()), int(counts.max())))
    assert bool((e_got <= bound).all())
    assert bool((got.cpu()[counts == 1] == one.cpu()[counts == 1]).all()) and bool((got.cpu()[counts == 0] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 5. - 7. masks move, construction is free of side effects, the lr is live
# ---------------------------------------------------------------------------------------------------------------------
def test_masks_move_and_lr_zero_moves_nothing(cases):
    case = cases("recorded-tiny")
    m = fresh_model(case)
    opt = training.ClippedAdamW(m.parameters(), lr=0.0, weight_decay=0.5)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    step = training.GraphTrainStep(m, opt, example_inputs(case, loss_weight(case, m)), seed=S0)
    it0 = step.seeds.iteration
    l1 = step()[0].clone()
    l2 = step()[0].clone()
    assert torch.isfinite(l1) and torch.isfinite(l2) and not torch.equal(l1, l2), "two replays on the same inputs drew the same masks"
    assert step.seeds.iteration == it0 + 2 and step.captures == 1
    for k, p in m.named_parameters():
        assert torch.equal(p, before[k]), k
        assert float(opt.state[p]["step"]) == 2.0


def test_construction_has_no_side_effects(cases):
    case = cases("recorded-tiny")
    m = fresh_model(case)
    opt = training.ClippedAdamW(m.parameters(), lr=1e-3)
    opt.materialize_state()
    before = snapshot(m, opt)
    versions = [p._version for p in m.parameters()]
    step = training.GraphTrainStep(m, opt, example_inputs(case, None), seed=S1)
    torch.cuda.synchronize()
    after = snapshot(m, opt)
    assert before.keys() == after.keys() and len(before) == 4 * len(list(m.parameters()))
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert all(float(v) == 0.0 for k, v in after.items() if k.startswith("step:"))
    assert [p._version for p in m.parameters()] == versions
    assert step.seeds.iteration == 0 and step.seeds.base == S1 and step.captures == 1
    step()
    n = training.dropout_sites(m)
    assert step.seeds.iteration == 1 and step.seeds.values()[:n] == M.words(S1, 1, n)
    assert all(p._version == v + 1 for p, v in zip(m.parameters(), versions))
    # materialize_state made what lazy creation makes
    m2 = fresh_model(case)
    lazy = training.ClippedAdamW(m2.parameters(), lr=1e-3)
    assert not lazy.state
    for p in m2.parameters():
        p.grad = torch.zeros_like(p)
    lazy.step()
    for (k, p), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        for s in ("exp_avg", "exp_avg_sq"):
            assert before[s + ":" + k].shape == lazy.state[p2][s].shape and before[s + ":" + k].dtype == lazy.state[p2][s].dtype and not before[s + ":" + k].any()


def test_lr_is_live(cases):
    case = cases("recorded-tiny")
    m = fresh_model(case)
    opt = training.ClippedAdamW(m.parameters(), lr=1e-3)
    step = training.GraphTrainStep(m, opt, example_inputs(case, None), seed=S0)
    params = lambda: [p.detach().clone() for p in m.parameters()]
    p0 = params()
    step()
    p1 = params()
    assert sum(not torch.equal(a, b) for a, b in zip(p0, p1)) > 0.9 * len(p0)
    for g in opt.param_groups:
        g["lr"] = 0.0
    step()
    p2 = params()
    assert all(torch.equal(a, b) for a, b in zip(p1, p2)), "a replay at lr = 0 moved a parameter: the table upload sits inside the graph"
    for g in opt.param_groups:
        g["lr"] = 1e-3
    step()
    assert sum(not torch.equal(a, b) for a, b in zip(p2, params())) > 0.9 * len(p0)
    assert step.captures == 1


# ---------------------------------------------------------------------------------------------------------------------
# 8. hand-over to the engine and to the captured samplers
# ---------------------------------------------------------------------------------------------------------------------
def test_handover(cases):
    case = cases("recorded-tiny")
    cfg = case.cfg
    m = fresh_model(case)
    m.eval()
    cs, us = to_dev(cond_for(cfg, 1, 3, 0, 1), DEV), to_dev(cond_for(cfg, 1, 3, 0, 2), DEV)
    sampler = paella_amd.GraphSampler(m, cs, us, (1, 16, 16), steps=2, renoise_steps=1, device=DEV)
    t0 = sampler(cs, us, seed=9).clone()
    assert sampler.captures == 1
    m.train()
    opt = training.ClippedAdamW(m.parameters(), lr=2e-3)
    step = training.GraphTrainStep(m, opt, example_inputs(case, None), seed=S0)
    step()
    step()
    m.eval()
    gen = torch.Generator().manual_seed(17)
    x = torch.randint(0, cfg["num_labels"], (2, 16, 16), generator=gen).to(DEV)
    r = torch.tensor([0.8, 0.3]).to(DEV)
    cc = to_dev(cond_for(cfg, 2, 3, 1, G.COND_SEED + 3), DEV)
    with torch.no_grad():
        got = m(x, r, **cc).clone()
        fresh = paella_amd.Paella(**cfg)
        fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
        want = fresh.to(DEV)(x, r, **cc)
    assert torch.isfinite(got).all() and torch.equal(got, want), "the engine does not serve the weights the replays wrote"
    t1 = sampler(cs, us, seed=9).clone()
    assert sampler.captures == 2 and t1.shape == t0.shape
    assert torch.equal(sampler(cs, us, seed=9), t1) and sampler.captures == 2
    m.train()
    step()
    assert step.captures == 1 and step.seeds.iteration == 3


# ---------------------------------------------------------------------------------------------------------------------
# 9. staleness and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_staleness_recaptures(cases):
    """a training switch flipped before iteration 2 and model.dropout changed before iteration 3: two recaptures, and the run still matches the eager one"""
    case = cases("recorded-tiny")
    hooks = {2: lambda m: m.set_training_modulation("torch"), 3: lambda m: setattr(m, "dropout", 0.05)}
    with T.deterministic_torch():
        eager_a = eager_run(case, ALL_ON, S1, 3, True, hooks)
        eager_b = eager_run(case, ALL_ON, S1, 3, True, hooks)
        replay, step = graph_run(case, ALL_ON, S1, 3, True, hooks)
    assert step.captures == 3
    assert_replay_matches_eager("recorded-tiny with two recaptures", replay, eager_a, eager_b)


def test_a_recapture_that_needs_more_sites_grows_the_same_table(cases):
    """model.dropout goes from a level that draws nothing to all levels drawing: `.seeds` is public, so it stays the object a caller may hold"""
    case = cases("recorded-tiny")
    m = fresh_model(case, dropout=[0.0, 0.1, 0.1])
    opt = training.ClippedAdamW(m.parameters(), lr=1e-3)
    step = training.GraphTrainStep(m, opt, example_inputs(case, None), seed=S1)
    held, n0 = step.seeds, step.seeds.n_sites
    assert n0 == training.dropout_sites(m)
    step()
    m.dropout = 0.1
    n1 = training.dropout_sites(m)
    assert n1 > n0
    loss = step()[0]
    assert step.seeds is held and held.n_sites == n1 and step.captures == 2 and held.iteration == 2 and held.base == S1
    assert held.values() == M.words(S1, 2, n1) and bool(torch.isfinite(loss))


def test_on_stale_raise_names_the_cause(cases):
    case = cases("recorded-tiny")
    m = fresh_model(case)
    opt = training.ClippedAdamW(m.parameters(), lr=1e-3)
    step = training.GraphTrainStep(m, opt, example_inputs(case, None), seed=S0, on_stale="raise")
    step()
    m.set_training_gemm("fp32")
    with pytest.raises(RuntimeError, match="training gemm"):
        step()
    m.set_training_gemm("bf16")
    m.dropout = [0.1, 0.0, 0.1]
    with pytest.raises(RuntimeError, match="model.dropout"):
        step()
    m.dropout = case.dropout
    m.eval()
    with pytest.raises(RuntimeError, match="train mode"):
        step()
    m.train()
    with torch.no_grad():
        p = next(m.parameters())
        p.data = p.data.clone()
    with pytest.raises(RuntimeError, match="parameter storage"):
        step()
    assert step.captures == 1 and step.seeds.iteration == 1


def test_refusals(cases):
    case = cases("recorded-tiny")
    m = fresh_model(case)
    opt = training.ClippedAdamW(m.parameters(), lr=1e-3)
    inputs = example_inputs(case, None)
    calls = []
    real = train_ops._call
    train_ops._call = lambda *a: calls.append(a[0]) or real(*a)
    try:
        with pytest.raises(TypeError, match="ClippedAdamW"):
            training.GraphTrainStep(m, torch.optim.AdamW(m.parameters(), lr=1e-3), inputs)
        m.eval()
        with pytest.raises(RuntimeError, match="eval mode"):
            training.GraphTrainStep(m, opt, inputs)
        m.train()
        cpu = paella_amd.Paella(**case.cfg)
        cpu.train()
        with pytest.raises(ValueError, match="HIP device"):
            training.GraphTrainStep(cpu, opt, inputs)
        with pytest.raises(ValueError, match="on_stale"):
            training.GraphTrainStep(m, opt, inputs, on_stale="ignore")
        with pytest.raises(ValueError, match="needs latents"):
            training.GraphTrainStep(m, opt, {k: v for k, v in inputs.items() if k != "latents"})
        assert not calls
        step = training.GraphTrainStep(m, opt, inputs, seed=S0)
        del calls[:]
        before = [p.detach().clone() for p in m.parameters()]
        with pytest.raises(ValueError, match="noised"):
            step(noised=case.noised[:, :8])
        with pytest.raises(ValueError, match="noised"):
            step(noised=case.noised.to(torch.int32))
        with pytest.raises(ValueError, match="loss_weight"):
            step(loss_weight=loss_weight(case, m))            # captured without one
        with pytest.raises(ValueError, match="got also"):
            step(labels=case.latents)
        torch.cuda.synchronize()
        assert not calls and step.seeds.iteration == 0 and all(torch.equal(a, b) for a, b in zip(before, m.parameters()))
    finally:
        train_ops._call = real


# ---------------------------------------------------------------------------------------------------------------------
# 10. the defaults are untouched
# ---------------------------------------------------------------------------------------------------------------------
def test_defaults_are_untouched(cases):
    case = cases("recorded-tiny")
    entries = []
    real = train_ops._call
    train_ops._call = lambda *a: entries.append(a[0]) or real(*a)
    try:
        out = T.run_step(case, T.HIP, fused_loss=True)
    finally:
        train_ops._call = real
    h = out["harness"]
    assert not [e for e in entries if e.endswith("_seed_dev")], "a default step reached a device-seed entry point"
    drawing = [c for c in h.lib_calls if c[3] > 0.0]
    assert len(h.forwards()) == case.n_drawing_calls() == len(drawing) // 2 and len(set(h.forward_seeds())) == case.n_drawing_calls()
    assert sum(e in T.ENTRIES for e in entries) == len(h.lib_calls) == 2 * case.n_drawing_calls()
    # ClippedAdamW.step(): one count per step, a state created at the first gradient, and no synchronisation with the device
    m = fresh_model(case)
    forward_backward(m, case, None, ints=T.injected(case))
    opt = training.ClippedAdamW(m.parameters(), lr=1e-3)
    assert not opt.state
    steps, waits = train_ops.ADAMW_COUNTERS["steps"], train_ops.ADAMW_COUNTERS["staging_waits"]
    # the launches of a step(): ONE paella_adamw_step call (its three kernels) and no other call into the library
    lib = train_ops._lib.load()
    real_step, real_norm, lib_calls = lib.paella_adamw_step, lib.paella_adamw_grad_norm, []
    lib.paella_adamw_step = lambda *a: lib_calls.append("step") or real_step(*a)
    lib.paella_adamw_grad_norm = lambda *a: lib_calls.append("norm") or real_norm(*a)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for _ in range(3):
                opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
        lib.paella_adamw_step, lib.paella_adamw_grad_norm = real_step, real_norm
    assert lib_calls == ["step"] * 3
    assert not [str(w.message) for w in caught if "synchronizing" in str(w.message).lower()]
    assert train_ops.ADAMW_COUNTERS["steps"] == steps + 3 and train_ops.ADAMW_COUNTERS["staging_waits"] >= waits
    assert all(float(opt.state[p]["step"]) == 3.0 for p in m.parameters()) and len(opt.state) == len(list(m.parameters()))
    # a GraphTrainStep counts nothing at a replay: the counters move at capture time only
    gopt = training.ClippedAdamW(m.parameters(), lr=1e-3)
    step = training.GraphTrainStep(m, gopt, example_inputs(case, None), seed=S0)
    counters = (dict(train_ops.ADAMW_COUNTERS), dict(train_ops.ATTN_COUNTERS), dict(train_ops.MOD_COUNTERS), dict(train_ops.LINEAR_COUNTERS), dict(train_ops.DW_COUNTERS))
    step()
    assert counters == (train_ops.ADAMW_COUNTERS, train_ops.ATTN_COUNTERS, train_ops.MOD_COUNTERS, train_ops.LINEAR_COUNTERS, train_ops.DW_COUNTERS)

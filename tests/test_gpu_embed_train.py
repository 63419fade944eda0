"""GPU: the training token stem (`paella_amd.training.token_embed_layernorm`, paella_amd/csrc/embed_train.hip) against the fp64 model of
tests/embed_train_model.py, the sixth training switch in a recorded step and against the fp64 mirror, and a captured iteration that holds the op.

The accuracy rule is the project's (tests/train_op_checks.py): error(fused) <= FACTOR x max(error of the torch fp32 chain on the same inputs, one fp32 ulp at the
reference's largest magnitude), FACTOR = 4, the torch chain run under `deterministic_torch()`.  The measured pairs are printed under "train_embedding parity" and
kept in profiles/train_embedding_parity.txt."""
import functools

import pytest
import torch

from paella_amd import _lib, training
from tests import embed_train_model as M
from tests import test_gpu_train_graph as TG
from tests import train_op_checks as T
from tests.test_gpu_train_graph import cases  # noqa: F401  (the module-scoped fixture of the step cases)
from tests.test_gpu_training import _train_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-6
# the kernel's constants (embed_train.hip): tokens per scan step, and the labels a workgroup owns = min(256, 4096 / c_in)
TOKEN_BLOCK = 1024
labels_per_block = lambda c_in: min(256, 4096 // c_in)
# name -> (B, H, W, patch, c_in, num_labels, the one label every token holds or None)
SHAPES = {
    "one-token": (1, 1, 1, 1, 4, 3, None),              # one token, one float4 per row, two labels never seen
    "tiny": (2, 4, 6, 2, 32, 64, None),                 # the tiny geometry
    "off-every-tile": (3, 2, 10, 2, 260, 70, None),     # c_in = 260: tail lanes and a second channel per thread; 70 labels = 4 blocks of 15 + a partial one of 10
    "all-equal": (2, 16, 16, 2, 32, 64, 37),            # every token the same label: one row takes all 512 gradients, 63 rows exact zero
    "block-plus-one": (1, 25, 41, 1, 32, 300, None),    # 1025 tokens = TOKEN_BLOCK + 1; 300 labels = 2 blocks of 128 + a partial one of 44
    "shipped": (2, 32, 32, 2, 256, 8192, None),         # the shipped widths
}
ALL_SIX = dict(TG.ALL_ON, embedding="hip")


def test_the_chosen_shapes_hit_what_they_name():
    B, H, W, p, c, L, _ = SHAPES["block-plus-one"]
    assert B * H * W == TOKEN_BLOCK + 1 and -(-L // labels_per_block(c)) == 3 and L % labels_per_block(c)
    B, H, W, p, c, L, _ = SHAPES["off-every-tile"]
    assert c > 256 and c % 64 and L % labels_per_block(c) and -(-L // labels_per_block(c)) > 1


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, weight, d_rows on the device; the fp64 model's rows and dweight; the torch fp32 chain's rows and dweight on the device) -- made once, left unchanged"""
    B, H, W, p, c, L, tok = SHAPES[name]
    x, w, d = M.inputs(B, H, W, p, c, L, seed=sorted(SHAPES).index(name), tokens=tok)
    ref_rows, ref_dw = M.model(x, w, d, p, EPS)
    xd, wd, dd = x.to(DEV), w.to(DEV), d.to(DEV)
    with T.deterministic_torch():
        wt = wd.clone().requires_grad_(True)
        t_rows = M.chain(xd, wt, p, EPS)
        t_rows.backward(dd)
    return xd, wd, dd, ref_rows, ref_dw, t_rows.detach(), wt.grad


def raw_forward(x, w, patch, hook=False):
    lib = _lib.load()
    B, H, W = x.shape
    L, C = w.shape
    rows = torch.full((B, H // patch, W // patch, C * patch * patch), float("nan"), device=DEV)
    if hook:
        _lib.check(lib.paella_test_embed_ln_unshuffle(_lib.ptr(x), _lib.ptr(w), _lib.ptr(rows), B, H, W, C, patch, L, EPS, _lib.stream_ptr(x.device)))
    else:
        ws = torch.empty(lib.paella_embed_ln_train_workspace_bytes(B, H, W, C, patch, L), dtype=torch.uint8, device=DEV)
        _lib.check(lib.paella_embed_ln_train_forward(_lib.ptr(x), _lib.ptr(w), B, H, W, C, patch, L, EPS, _lib.ptr(rows), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device)))
    return rows


def raw_backward(x, w, d, patch, out_fill=float("nan"), ws_fill=255):
    """the C entry point itself: dtable_out and the workspace start as garbage -- the gradient is WRITTEN and the op initialises what it reads"""
    lib = _lib.load()
    B, H, W = x.shape
    L, C = w.shape
    dw = torch.full((L, C), out_fill, device=DEV)
    ws = torch.full((lib.paella_embed_ln_train_workspace_bytes(B, H, W, C, patch, L),), ws_fill, dtype=torch.uint8, device=DEV)
    _lib.check(lib.paella_embed_ln_train_backward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(d), B, H, W, C, patch, L, EPS, _lib.ptr(dw), _lib.ptr(ws), ws.numel(),
                                                  _lib.stream_ptr(x.device)))
    return dw


def op(x, w, d, patch):
    wt = w.clone().requires_grad_(True)
    rows = training.token_embed_layernorm(x, wt, patch, EPS)
    rows.backward(d)
    return rows.detach(), wt.grad


# ---------------------------------------------------------------------------------------------------------------------
# 1. op parity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_op_against_the_fp64_model(built_lib, name):
    """Measured pairs (fused / torch, MI355X): all of them in profiles/train_embedding_parity.txt."""
    x, w, d, ref_rows, ref_dw, t_rows, t_dw = _case(name)
    p = SHAPES[name][3]
    calls = dict(training.EMBED_COUNTERS)
    rows, dw = op(x, w, d, p)
    assert training.EMBED_COUNTERS == {"calls": calls["calls"] + 1, "backward": calls["backward"] + 1}
    assert rows.is_contiguous() and tuple(rows.shape) == tuple(ref_rows.shape) and tuple(dw.shape) == tuple(w.shape)
    pairs = []
    for what, got, tor, ref in (("rows", rows, t_rows, ref_rows), ("dweight", dw, t_dw, ref_dw)):
        assert torch.isfinite(got).all(), what
        pairs.append((what, T.err(got.cpu(), ref), T.err(tor.cpu(), ref), T.ulp(ref)))
    print("train_embedding parity %s %s: " % (name, "x".join(map(str, SHAPES[name][:6]))) + "  ".join("%s fused %.3e torch %.3e ulp %.3e" % q for q in pairs))
    for what, e_fused, e_torch, ulp in pairs:
        assert T.within_yardstick(e_fused, e_torch, ulp), "%s %s: fused error %.3e exceeds %gx max(torch fp32 chain %.3e, ulp %.3e)" % (name, what, e_fused, T.FACTOR, e_torch, ulp)
    counts = torch.bincount(x.flatten().cpu(), minlength=w.size(0))
    assert bool((dw.cpu()[counts == 0] == 0).all())
    if name == "all-equal":
        assert int((counts == 0).sum()) == 63 and int(counts.max()) == 512


def test_clamped_tokens_in_both_directions(built_lib):
    """tokens below 0 and at / above num_labels: the clamped row is read and receives the gradient"""
    x, w, d = (t.clone() for t in _case("tiny")[:3])
    x[0, 0, 0], x[1, 3, 5], x[0, 2, 1], x[1, 0, 0] = -1, 64, 1 << 40, -(1 << 62)
    rows, dw = op(x, w, d, 2)
    rows_c, dw_c = op(x.clamp(0, 63), w, d, 2)
    assert torch.equal(rows, rows_c) and torch.equal(dw, dw_c) and torch.isfinite(dw).all()
    ref_rows, ref_dw = M.model(x.cpu(), w.cpu(), d.cpu(), 2, EPS)
    with T.deterministic_torch():
        wt = w.clone().requires_grad_(True)
        M.chain(x, wt, 2, EPS).backward(d)
    assert T.within_yardstick(T.err(dw.cpu(), ref_dw), T.err(wt.grad.cpu(), ref_dw), T.ulp(ref_dw))
    assert bool((dw[0] != 0).any()) and bool((dw[63] != 0).any())


# ---------------------------------------------------------------------------------------------------------------------
# 2. written, not accumulated
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one-token", "off-every-tile", "block-plus-one"])
def test_the_gradient_is_written_not_accumulated(built_lib, name):
    x, w, d, _, ref_dw, _, t_dw = _case(name)
    p = SHAPES[name][3]
    dw = raw_backward(x, w, d, p)                      # dtable_out pre-filled with NaN
    assert torch.isfinite(dw).all()
    assert torch.equal(dw, op(x, w, d, p)[1])
    counts = torch.bincount(x.flatten().cpu(), minlength=w.size(0))
    never, once = counts == 0, counts == 1
    assert bool(never.any()) and bool(once.any())
    assert bool((dw.cpu()[never] == 0.0).all())
    # a label seen once: the LayerNorm backward of its one gradient row, by hand in fp64
    C, pp = w.size(1), p * p
    g = d.double().cpu().view(-1, C, pp).permute(0, 2, 1)                    # [output position, (dy, dx), c]
    B, H, W = x.shape
    g = g.reshape(B, H // p, W // p, p, p, C).permute(0, 1, 3, 2, 4, 5).reshape(B * H * W, C)   # [token, c] in token order
    flat = x.flatten().cpu()
    labels = torch.nonzero(once).flatten()
    pos = torch.stack([torch.nonzero(flat == l).flatten()[0] for l in labels])
    row = w.double().cpu()[labels]
    mean = row.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((row - mean) ** 2).mean(1, keepdim=True) + EPS)
    xh, gg = (row - mean) * rstd, g[pos]
    by_hand = rstd * ((gg - gg.mean(1, keepdim=True)) - xh * (gg * xh).mean(1, keepdim=True))
    e_fused, e_torch, ulp = T.err(dw.cpu()[once], by_hand), T.err(t_dw.cpu()[once], by_hand), T.ulp(by_hand)
    print("train_embedding parity %s labels seen once: dweight fused %.3e torch %.3e ulp %.3e" % (name, e_fused, e_torch, ulp))
    assert T.within_yardstick(e_fused, e_torch, ulp)
    # a NaN in the table row of a label that never occurs stays out of its gradient: that row is written as zeros, not computed
    w2 = w.clone()
    w2[torch.nonzero(never).flatten()[0].item()] = float("nan")
    assert torch.equal(raw_backward(x, w2, d, p), dw)


# ---------------------------------------------------------------------------------------------------------------------
# 3. determinism
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all-equal", "block-plus-one", "shipped"])
def test_the_backward_repeats_itself_bit_for_bit(built_lib, name):
    x, w, d = _case(name)[:3]
    p = SHAPES[name][3]
    first = raw_backward(x, w, d, p)
    for out_fill, ws_fill in ((0.0, 0), (float("inf"), 0x5A), (-7.5, 0xC3)):
        assert torch.equal(raw_backward(x, w, d, p, out_fill, ws_fill), first)
    a, b = op(x, w, d, p)[1], op(x, w, d, p)[1]
    assert torch.equal(a, first) and torch.equal(b, first)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the forward is the engine's launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_rows_are_the_inference_stems_bits(built_lib, name):
    x, w, d = _case(name)[:3]
    p = SHAPES[name][3]
    engine = raw_forward(x, w, p, hook=True)
    assert torch.isfinite(engine).all()
    assert torch.equal(raw_forward(x, w, p), engine)
    with torch.no_grad():
        assert torch.equal(training.token_embed_layernorm(x, w, p, EPS), engine)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the recorded step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("others", ["torch", "hip"])
@pytest.mark.parametrize("which", ["tiny", "variant"])
def test_train_step_with_the_hip_stem_reproduces_the_reference(golden, built_lib, which, others):
    """_train_step of tests/test_gpu_training.py under set_training_embedding("hip") -- alone, and with all six switches on but gemm (kept "fp32": the recorded
    tolerances are fp32 ones) -- against the reference's recorded step; then the hand-over to the HIP engine, which never sees the switch.  tiny is patch 2,
    variant patch 1."""
    cfg, m = T.model_for(which, golden, DEV)
    m.set_training_route(activation=others, depthwise=others, attention=others, modulation=others, gemm="fp32", embedding="hip")
    assert cfg["patch_size"] == (2 if which == "tiny" else 1)
    n0 = training.EMBED_COUNTERS["calls"]
    pred, loss = _train_step(m, cfg)
    assert training.EMBED_COUNTERS["calls"] == n0 + 1, "the train-mode forward did not route the token stem through the HIP op"
    assert m.in_mapper._modules["0"].weight.grad is not None
    T.assert_switched_step_and_handover(m, cfg, golden("train_%s_step" % which), pred, loss, lambda: m.set_training_embedding("torch"),
                                        op_calls=lambda: training.EMBED_COUNTERS["calls"], calls_per_forward=1)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the fp64 mirror
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["recorded-tiny", "recorded-variant", "one-position"])
def test_step_with_dropout_against_the_fp64_mirror(cases, name):  # noqa: F811
    """tests/test_gpu_train_step_dropout.py's step with injected seeds on the route HIP + modulation + embedding, against the fp64 mirror under that file's rule.
    The stem draws no seed: the library calls of the other ops are still the mirror's call plan."""
    case = cases(name)
    seeds = T.injected(case)
    calls = training.EMBED_COUNTERS["calls"]
    assert "in_mapper.0.weight" in case.names
    case.m.set_training_embedding("hip")
    try:
        out = T.run_step(case, T.HIP + ("hip",), seeds=iter(seeds))
    finally:
        case.m.set_training_route(modulation="torch", embedding="torch")
    assert training.EMBED_COUNTERS["calls"] == calls + 1
    assert "in_mapper.0.weight" in out["values"]
    T.assert_step_against_mirror(case, out, seeds, "five switches with the stem", label="train_embedding parity")


# ---------------------------------------------------------------------------------------------------------------------
# 7. the captured iteration
# ---------------------------------------------------------------------------------------------------------------------
class _Counting:
    """while entered: `training._token_embedding` and `torch.nn.functional.embedding` count their calls"""

    def __enter__(self):
        self.pieces = self.lookups = 0
        self.real = (training._token_embedding, torch.nn.functional.embedding)
        piece, lookup = self.real

        def piece_w(*a, **k):
            self.pieces += 1
            return piece(*a, **k)

        def lookup_w(*a, **k):
            self.lookups += 1
            return lookup(*a, **k)

        training._token_embedding, torch.nn.functional.embedding = piece_w, lookup_w
        return self

    def __exit__(self, *exc):
        training._token_embedding, torch.nn.functional.embedding = self.real
        return False


def test_replay_above_the_embedding_threshold_holds_the_op(cases):  # noqa: F811
    """2 x 40x40 = 3200 tokens, above EMBEDDING_CHUNK, all six switches on: two replays against two eager iterations under a seed table of the same base, by the
    rule of tests/test_gpu_train_graph.py -- and neither side looks a token up through torch, in pieces or whole: torch's sorting backward is never put in a graph"""
    big = TG._Larger(cases("recorded-tiny"))
    assert big.noised.numel() > training.EMBEDDING_CHUNK
    calls = dict(training.EMBED_COUNTERS)
    with T.deterministic_torch(), _Counting() as counted:
        eager_a = TG.eager_run(big, ALL_SIX, T.S0, 2, True, table=True)
        eager_b = TG.eager_run(big, ALL_SIX, T.S0, 2, True, table=True)
        replay, step = TG.graph_run(big, ALL_SIX, T.S0, 2, True)
    assert counted.pieces == 0 and counted.lookups == 0
    assert step.captures == 1
    # 2 x 2 eager forwards, then the warm-up and the capture: the replays call nothing
    assert training.EMBED_COUNTERS == {"calls": calls["calls"] + 6, "backward": calls["backward"] + 6}
    TG.assert_replay_matches_eager("recorded-tiny weights at 2 x 40x40 tokens (token stem in HIP)", replay, eager_a, eager_b)


def test_flipping_the_switch_recaptures_and_the_default_keeps_its_pieces(cases):  # noqa: F811
    big = TG._Larger(cases("recorded-tiny"))
    m = TG.fresh_model(big)                              # the five earlier switches on, the stem at its default
    opt = training.ClippedAdamW(m.parameters(), lr=1e-3)
    calls = training.EMBED_COUNTERS["calls"]
    with _Counting() as counted:
        step = training.GraphTrainStep(m, opt, TG.example_inputs(big, None), seed=T.S0)
    # (c) the default is untouched: warm-up and capture each look the 3200 tokens up in two pieces
    assert counted.pieces == 2 and counted.lookups == 4 and training.EMBED_COUNTERS["calls"] == calls
    step()
    # (b) a flip on a live step recaptures once
    m.set_training_embedding("hip")
    with _Counting() as counted:
        loss = step()[0]
    assert step.captures == 2 and counted.pieces == 0 and counted.lookups == 0 and training.EMBED_COUNTERS["calls"] == calls + 2
    assert bool(torch.isfinite(loss))
    strict = training.GraphTrainStep(m, opt, TG.example_inputs(big, None), seed=T.S0, on_stale="raise")
    strict()
    m.set_training_embedding("torch")
    with pytest.raises(RuntimeError, match="training embedding"):
        strict()
    assert strict.captures == 1

"""GPU: every route by which weights change under the HIP engine -- what the engine computes after the route against a module built fresh with the same weights.

The kernels are held to fp64 elsewhere; this file is about WHICH weights they see.  A module that has run keeps a native model with its own copies of the tensors
and tables derived from them at load time (repacked and permuted weights, the LayerNorm fold's row sums, the composed conditioning projection, in the bf16 mode the
shadows and their row sums, for the VQGAN the ResBlock gammas as host constants).  A fresh module has no reload history, so the yardstick of every test is

    output of the module after the change == output of paella_amd.Paella / VQModel constructed and loaded with the same state dict, BIT FOR BIT,

in fp32 and in the bf16 mode (a fresh module in the bf16 mode is the reference there), and the output must differ from the one before the change -- a change that
cannot be seen proves nothing.  No tolerance is involved.  That the fresh engine is not equally wrong is shown once per sweep against the oracle in fp64, under
the bounds of tests/test_gpu_unet_geometries.py and tests/test_gpu_vqgan_geometries.py.

(a) the routes of tests/weight_routes.py; (b) one state-dict key at a time; (c) GraphSampler / RequestStream after the two routes that swap tensor objects;
(d) a CondCache across a reload and across set_gemm_precision; (e) copies of a module that has run."""
import copy
import functools
import gc
import io

import pytest
import torch

import paella_amd
from oracle import golden_configs as G
from oracle import paella_oracle as O
from tests import unet_cases as U
from tests import vqgan_cases as V
from tests import weight_routes as R
from tests.helpers import cond_for, to_dev, weights_for
from tests.test_gpu_unet_geometries import _parity as unet_parity
from tests.test_gpu_vqgan_geometries import _parity as vqgan_parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ["paella", "vqmodel"]
PRECISIONS = ["fp32", "bf16"]
SEED_A, SEED_B = G.WEIGHT_SEED, G.WEIGHT_SEED + 11

UNET = U.CASES["four_levels"]
UNET_CFG = UNET["cfg"]          # four levels, C T A F in four orders; here with ByT5 rows AND CLIP AND one CLIP image, so that every mapper reaches the logits
VQ_CFG = G.VQ_TINY_F8
VQ_B, VQ_H, VQ_W = 2, 3, 2


def _new(kind, sd=None, seed=SEED_A):
    """a module on the CPU holding `sd` (or the seeded synthetic weights of `seed`); returns (module, state dict)"""
    m = paella_amd.Paella(**UNET_CFG) if kind == "paella" else paella_amd.VQModel(**VQ_CFG)
    if sd is None:
        sd = weights_for(m, sum(UNET_CFG["blocks"]) if kind == "paella" else VQ_CFG["bottleneck_blocks"], seed=seed)
    else:
        m.load_state_dict(sd)
    return m, sd


def _fresh(kind, sd, precision):
    """constructed, loaded, moved, switched: a module with no reload history"""
    m = _new(kind, sd)[0].to(DEV)
    return m.set_gemm_precision(precision) if precision != "fp32" else m


@functools.lru_cache(maxsize=None)
def _sd(kind, seed):
    return _new(kind, seed=seed)[1]


@functools.lru_cache(maxsize=None)
def _inputs(kind):
    """the inputs of every run of a model kind, on the CPU, drawn once"""
    g = torch.Generator().manual_seed(UNET["seed"] + 77)
    if kind == "paella":
        B, H, W = UNET["B"], UNET["H"], UNET["W"]
        return dict(x=torch.randint(0, UNET_CFG["num_labels"], (B, H, W), generator=g), r=U.inexact_r(B, UNET["seed"] + 1077),
                    cond=cond_for(UNET_CFG, B, 3, 1, G.COND_SEED + UNET["seed"] + 77))
    f, K = 2 ** VQ_CFG["levels"], VQ_CFG["codebook_size"]
    tokens = torch.randint(0, K, (VQ_B, VQ_H, VQ_W), generator=g)
    tokens.view(-1)[0], tokens.view(-1)[-1] = 0, K - 1
    return dict(img=torch.rand(VQ_B, 3, VQ_H * f, VQ_W * f, generator=g), tokens=tokens)


@functools.lru_cache(maxsize=None)
def _dev_inputs(kind):
    i = _inputs(kind)
    return {k: (to_dev(v, DEV) if isinstance(v, dict) else v.to(DEV)) for k, v in i.items()}


def _run(kind, m):
    """what the engine computes: the logits; for the VQGAN encode (latents, codes, indices, loss) and decode_indices"""
    i = _dev_inputs(kind)
    with torch.no_grad():
        if kind == "paella":
            out = dict(logits=m(i["x"], i["r"], **i["cond"]).clone())
        else:
            qe, lat, idx, loss = m.encode(i["img"])
            out = dict(qe=qe, lat=lat, idx=idx, loss=loss.reshape(1).clone(), dec_idx=m.decode_indices(i["tokens"]))
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.contiguous().view(torch.int32) if t.is_floating_point() else t


def _same(a, b):
    return [k for k in a if not torch.equal(_bits(a[k]), _bits(b[k]))]


def _assert_same(got, want, what):
    assert got.keys() == want.keys()
    diff = _same(got, want)
    assert not diff, "%s: %s differ from the fresh module's, e.g. %s at %d of %d entries" % (
        what, diff, diff[0], int((_bits(got[diff[0]]) != _bits(want[diff[0]])).sum()), got[diff[0]].numel())


def _assert_moved(got, before, what):
    assert len(_same(got, before)) > 0, "%s: the output is, bit for bit, the one before the change" % what


@functools.lru_cache(maxsize=None)
def _fresh_output(kind, seed, precision):
    """the output of a fresh module with the seeded weights of `seed`, computed once per (kind, weights, precision); nobody writes to it"""
    return _run(kind, _fresh(kind, _sd(kind, seed), precision))


# ---------------------------------------------------------------------------------------------------------------------
# (a) the route matrix
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", R.ROUTE_NAMES)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", KINDS)
def test_route_serves_the_new_weights(built_lib, kind, precision, route):
    """load A, run once so that the engine exists, take the route to B (for the one REFRESH route: and call refresh()), run: the fresh-B output bit for bit, and
    not the A output"""
    want_a, want_b = _fresh_output(kind, SEED_A, precision), _fresh_output(kind, SEED_B, precision)
    _assert_moved(want_b, want_a, "fresh modules with the weights A and B")
    m = _fresh(kind, _sd(kind, SEED_A), precision)
    first = _run(kind, m)
    _assert_same(first, want_a, "%s %s before the route" % (kind, precision))
    handle = m._handle
    assert handle is not None
    r = R.BY_NAME[route]
    r.apply(m, _sd(kind, SEED_B))
    if r.contract == R.REFRESH:
        m.refresh()
    assert R.home(m).type == "cuda" and m.get_gemm_precision() == precision
    got = _run(kind, m)
    assert m._handle is handle, "the route built a second native model instead of reloading the first"
    _assert_same(got, want_b, "%s %s after %s" % (kind, precision, route))
    _assert_moved(got, first, "%s %s after %s" % (kind, precision, route))
    R.assert_holds(m, _sd(kind, SEED_B))


# ---------------------------------------------------------------------------------------------------------------------
# (b) one key at a time
# ---------------------------------------------------------------------------------------------------------------------
def _group_of(kind, m, key):
    """the block kind a state-dict key belongs to"""
    parts = key.split(".")
    if kind == "paella":
        if parts[0] in ("down_blocks", "up_blocks"):
            k = getattr(m, parts[0])[int(parts[1])][int(parts[2])].kind
            return "resample" if k in "DU" else k
        return "ends"               # the conditioning mappers, the token embedding, the patch embedding, clf, out_mapper
    return {"in_block": "encoder", "down_blocks": "encoder", "vquantizer": "codebook", "up_blocks": "decoder", "out_block": "decoder"}[parts[0]]


GROUPS = {"paella": ["C", "T", "A", "F", "resample", "ends"], "vqmodel": ["encoder", "codebook", "decoder"]}


def _swept_keys(kind, m):
    """every floating-point entry of the state dict by group, in state-dict order.  The one entry left is the VQGAN BatchNorm's `num_batches_tracked`, an integer
    step counter that is no weight: the engine is never given it, and 0.05 of anything cannot be added to it."""
    by_group = {g: [] for g in GROUPS[kind]}
    for key, t in m.state_dict().items():
        if t.is_floating_point():
            by_group[_group_of(kind, m, key)].append(key)
        else:
            assert key.endswith("num_batches_tracked")
    return by_group


def _anchor(kind, m, sd, what):
    """the fp32 engine on the final state dict against the oracle in fp64, under the bounds the geometry tests apply to these tensors"""
    assert m.get_gemm_precision() == "fp32"
    got = _run(kind, m)
    i = _inputs(kind)
    with torch.no_grad():
        if kind == "paella":
            r_embed = O.r_embedding(i["r"].float(), UNET_CFG["c_r"])
            f64, f32 = (O.unet_forward(sd, UNET_CFG, i["x"], i["r"], dtype=dt, r_embed=r_embed, **i["cond"]) for dt in (torch.float64, torch.float32))
            fails = unet_parity(what, "logits", got["logits"], f64, f32)
            assert not fails, "\n".join(fails)
            return got
        rc = V.ref_cfg(VQ_CFG)
        ref = {}
        for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
            s = V._as(sd, dt)
            qe, lat, idx, loss = O.vq_encode(s, rc, i["img"].to(dt))
            ref[tag] = dict(qe=qe, lat=lat, idx=idx, dec_idx=O.vq_decode_indices(s, rc, i["tokens"]))
        rows = (ref["f64"]["lat"] * rc["scale_factor"]).permute(0, 2, 3, 1).reshape(-1, VQ_CFG["c_latent"])
        near = (V.nearest_margin(rows, sd["vquantizer.codebook.weight"].double()) < V.NEAR_TIE_EPS).view(ref["f64"]["idx"].shape)
        mism = got["idx"].cpu() != ref["f64"]["idx"]
        print("PARITY %s tokens: %d of %d differ from fp64, %d near-ties" % (what, int(mism.sum()), mism.numel(), int(near.sum())))
        assert not bool((mism & ~near).any()), "%s: tokens differ from fp64 where the nearest code is unambiguous" % what
        checks = [vqgan_parity(what, k, got[k], ref["f64"][k], ref["f32"][k]) for k in ("lat", "dec_idx")] + \
                 ([vqgan_parity(what, "qe", got["qe"], ref["f64"]["qe"], ref["f32"]["qe"])] if not bool(mism.any()) else [])
        for ok, msg in checks:
            assert ok, msg
    return got


def _sweep(kind, precision, group):
    m, sd_a = _new(kind)
    keys = _swept_keys(kind, m)[group]
    assert keys, "no key in group %s" % group
    sd = {k: v.clone() for k, v in sd_a.items()}
    m = m.to(DEV)
    if precision != "fp32":
        m.set_gemm_precision(precision)
    prev = _run(kind, m)
    _assert_same(prev, _fresh_output(kind, SEED_A, precision), "%s %s before the sweep" % (kind, precision))
    live = {key: R.tensor_of(holder, name, is_buffer) for key, holder, name, is_buffer in R.slots(m)}
    g = torch.Generator().manual_seed(4242)
    for key in keys:
        t = live[key]
        std = float(sd[key].std()) if sd[key].numel() > 1 else 0.0
        delta = torch.randn(sd[key].shape, generator=g) * (0.05 * std) if std > 0 else torch.full(sd[key].shape, 0.05)
        with torch.no_grad():
            t.add_(delta.to(DEV))
        sd[key] = t.detach().cpu().clone()
        assert not torch.equal(sd[key], sd_a[key])
        got = _run(kind, m)
        what = "%s %s after a change of %s alone" % (kind, precision, key)
        _assert_same(got, _run(kind, _fresh(kind, sd, precision)), what)
        _assert_moved(got, prev, what)
        prev = got
    # the fresh engine is not equally wrong: the exact path on the final state dict against fp64 (in the bf16 sweep after the switch back, which reloads nothing:
    # the fp32 tables were rebuilt by every reload of the sweep as well)
    if precision != "fp32":
        m.set_gemm_precision("fp32")
    _anchor(kind, m, sd, "%s/%s/%s" % (kind, precision, group))
    return len(keys)


@pytest.mark.parametrize("group", GROUPS["paella"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_key_at_a_time_unet(built_lib, precision, group):
    """every floating-point state-dict key of the group in turn: + 0.05 std of seeded noise on that tensor alone (a constant tensor: + 0.05), in place under
    no_grad; after each the engine equals a fresh module of the same state dict bit for bit and differs from the step before.  Then the fp64 anchor."""
    n = _sweep("paella", precision, group)
    print("weight_routes sweep paella %s %s: %d keys" % (precision, group, n))


@pytest.mark.parametrize("group", GROUPS["vqmodel"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_key_at_a_time_vqgan(built_lib, precision, group):
    n = _sweep("vqmodel", precision, group)
    print("weight_routes sweep vqmodel %s %s: %d keys" % (precision, group, n))


@pytest.mark.parametrize("kind", KINDS)
def test_the_groups_cover_every_weight(kind):
    m, sd = _new(kind)
    swept = [k for keys in _swept_keys(kind, m).values() for k in keys]
    assert sorted(swept) == sorted(k for k, t in sd.items() if t.is_floating_point()) and len(set(swept)) == len(swept)
    assert len(sd) - len(swept) == (0 if kind == "paella" else 1)


# ---------------------------------------------------------------------------------------------------------------------
# (c) the consumers of the signature
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["load_state_dict_assign", "new_objects"])
def test_graph_sampler_and_request_stream_notice_swapped_tensors(built_lib, route):
    """after load_state_dict(assign=True) and after new Parameter objects: GraphSampler(on_stale="raise") raises, the default recaptures and equals the eager
    `sample` bit for bit, and a RequestStream with a request in flight refuses as it does after a plain load_state_dict"""
    cfg, H = G.UNET_TINY, 16
    m = paella_amd.Paella(**cfg)
    sd = weights_for(m, sum(cfg["blocks"]))
    m = m.to(DEV)
    new_sd = {k: v * 1.05 for k, v in sd.items()}
    shape = (1, H, H)
    cs, us = to_dev(cond_for(cfg, 1, 3, 0, 1), DEV), to_dev(cond_for(cfg, 1, 3, 0, 2), DEV)
    kw = dict(steps=2, renoise_steps=1, device=DEV)
    eager = lambda: paella_amd.sample(m, cs, shape, unconditional_inputs=us, noise="philox", seed=9, **kw)
    strict = paella_amd.GraphSampler(m, cs, us, shape, on_stale="raise", **kw)
    gs = paella_amd.GraphSampler(m, cs, us, shape, **kw)
    stream = paella_amd.RequestStream(m, cs, us, (2, H, H), max_steps=2, device=DEV, on_stale="raise")
    q = dict(model_inputs=cs, unconditional_inputs=us, seed=7, steps=2)
    assert stream.admit(**q) == 0
    t0 = eager().clone()
    assert torch.equal(gs(cs, us, seed=9), t0) and torch.equal(strict(cs, us, seed=9), t0) and gs.captures == 1
    R.BY_NAME[route].apply(m, new_sd)
    with pytest.raises(RuntimeError, match="denoiser weights"):
        strict(cs, us, seed=9)
    with pytest.raises(RuntimeError, match="in flight"):
        stream.tick()
    with pytest.raises(RuntimeError, match="in flight"):
        stream.admit(**q)
    t1 = eager().clone()
    assert not torch.equal(t1, t0)
    fresh = paella_amd.Paella(**cfg)
    fresh.load_state_dict(new_sd)
    fresh = fresh.to(DEV)
    assert torch.equal(t1, paella_amd.sample(fresh, cs, shape, unconditional_inputs=us, noise="philox", seed=9, **kw)), "eager sample after the route is not a fresh module's"
    assert torch.equal(gs(cs, us, seed=9), t1) and gs.captures == 2
    assert torch.equal(gs(cs, us, seed=9), t1) and gs.captures == 2
    stream.reset()
    idle = paella_amd.RequestStream(m, cs, us, (2, H, H), max_steps=2, device=DEV, on_stale="raise")
    R.BY_NAME[route].apply(m, sd)
    with pytest.raises(RuntimeError, match="stale"):
        idle.admit(**q)


# ---------------------------------------------------------------------------------------------------------------------
# (d) CondCache
# ---------------------------------------------------------------------------------------------------------------------
def test_cond_cache_is_refused_after_a_reload(built_lib):
    """prepare_cond on A, reload to B: forward_prepared and forward_sample refuse the old cache with a RuntimeError that names the weight change, before anything is
    enqueued; a cache made after the reload serves, and the logits are a fresh module's; a cache of another module is refused as well"""
    i = _dev_inputs("paella")
    x, r, c = i["x"], i["r"], i["cond"]
    m = _fresh("paella", _sd("paella", SEED_A), "fp32")
    with torch.no_grad():
        old = m.prepare_cond(**c)
        base = m.forward_prepared(x, r, old).clone()
        _assert_same(dict(logits=base), _fresh_output("paella", SEED_A, "fp32"), "forward_prepared on A")
        assert old.gen == m._load_gen and m.forward_prepared(x, r, old) is not None     # still served while nothing changed
        m.load_state_dict(_sd("paella", SEED_B))
        out = torch.full((x.size(0), x.size(1), x.size(2), UNET_CFG["num_labels"]), float("nan"), device=DEV)
        toks = torch.full_like(x, -7)
        with pytest.raises(RuntimeError, match="weights changed"):
            m.forward_prepared(x, r, old, out=out)
        with pytest.raises(RuntimeError, match="weights changed"):
            m.forward_sample(x, r, old, toks, temperature=1.0, seed=3)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and bool((toks == -7).all()), "a refused call wrote to its output"
        new = m.prepare_cond(**c)
        assert new.gen == m._load_gen != old.gen
        got = m.forward_prepared(x, r, new).clone()
        _assert_same(dict(logits=got), _fresh_output("paella", SEED_B, "fp32"), "forward_prepared with a cache made after the reload")
        m.forward_sample(x, r, new, toks, temperature=1.0, seed=3)
        assert int(toks.min()) >= 0
        other = _fresh("paella", _sd("paella", SEED_B), "fp32")
        with pytest.raises(RuntimeError, match="another module"):
            other.forward_prepared(x, r, new)
        ours = other.prepare_cond(**c)
        assert torch.equal(ours.buf, new.buf)
        with pytest.raises(RuntimeError, match="another module"):
            m.forward_prepared(x, r, ours)


def test_cond_cache_outlives_a_precision_switch(built_lib):
    """paella_unet_cond_prepare runs the conditioning mappers, the LayerNorm, the SiLU and ONE GEMM over the composed K|V projection, all on the fp32 tensors: no
    bf16 shadow is read and the mode is not looked at.  So the K/V of a cache do not depend on the mode, the switch reloads nothing, and a cache made in one mode
    serves in the other: same cache bytes, and the logits of a cache made after the switch, bit for bit, both ways."""
    i = _dev_inputs("paella")
    x, r, c = i["x"], i["r"], i["cond"]
    m = _fresh("paella", _sd("paella", SEED_A), "fp32")
    with torch.no_grad():
        c32 = m.prepare_cond(**c)
        exact = m.forward_prepared(x, r, c32).clone()
        gen = m._load_gen
        m.set_gemm_precision("bf16")
        fast_old = m.forward_prepared(x, r, c32).clone()
        c16 = m.prepare_cond(**c)
        fast_new = m.forward_prepared(x, r, c16).clone()
        assert m._load_gen == gen == c16.gen, "the precision switch reloaded the weights"
        assert torch.equal(c32.buf, c16.buf), "the conditioning cache depends on the precision mode"
        assert torch.equal(_bits(fast_old), _bits(fast_new))
        _assert_same(dict(logits=fast_new), _fresh_output("paella", SEED_A, "bf16"), "bf16 after the switch")
        assert not torch.equal(fast_new, exact)
        m.set_gemm_precision("fp32")
        assert torch.equal(_bits(m.forward_prepared(x, r, c16)), _bits(exact))


# ---------------------------------------------------------------------------------------------------------------------
# (e) copies of a module that has run
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_deepcopy_of_a_module_that_has_run(built_lib, kind):
    m = _fresh(kind, _sd(kind, SEED_A), "fp32")
    base = _run(kind, m)
    handle = m._handle
    c = copy.deepcopy(m)
    # on the host, before any device call on the copy: a copy that shared the handle would free one native model twice
    assert c._handle is None and c._loaded_sig is None and c._ws is None and c._load_gen == 0, "the copy carries the original's engine state"
    assert m._handle is handle and handle is not None
    _assert_same(_run(kind, c), base, "%s: the deep copy" % kind)
    assert c._handle is not None and c._handle is not m._handle and c._handle.value != m._handle.value and c._load_gen != m._load_gen
    R.BY_NAME["inplace_no_grad"].apply(c, _sd(kind, SEED_B))
    _assert_same(_run(kind, c), _fresh_output(kind, SEED_B, "fp32"), "%s: the deep copy after its own weights changed" % kind)
    _assert_same(_run(kind, m), base, "%s: the original after the copy's weights changed" % kind)
    del c
    gc.collect()
    _assert_same(_run(kind, m), base, "%s: the original after the copy is gone" % kind)
    R.assert_holds(m, _sd(kind, SEED_A))


def test_torch_save_round_trip_of_a_module_that_has_run(built_lib):
    m = _fresh("paella", _sd("paella", SEED_A), "fp32")
    base = _run("paella", m)
    f = io.BytesIO()
    torch.save(m, f)
    f.seek(0)
    c = torch.load(f, weights_only=False)
    assert c._handle is None and c._loaded_sig is None and R.home(c).type == "cuda"
    _assert_same(_run("paella", c), base, "the module loaded back from torch.save")
    _assert_same(_run("paella", m), base, "the original after torch.save")

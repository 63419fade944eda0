"""CPU: the seam between the nn.Module and the native engine -- which weights the engine is told to load, and what a copy of a module takes along.

`Paella._engine()` / `VQModel._engine()` reload the native model when `_signature()` differs from the signature they loaded, and `GraphSampler` / `RequestStream`
recapture on the same comparison: a route by which the weights change and the signature does not leaves the engine computing with the old weights, silently.
Every route of tests/weight_routes.py is held to its contract here, on the CPU (the signature reads pointers and versions, no kernel); what the engine then
computes is tests/test_gpu_weight_routes.py's."""
import copy
import ctypes
import gc
import io
import pickle

import pytest
import torch
from torch import nn

import paella_amd
from oracle import golden_configs as G
from paella_amd import _lib, training
from tests import weight_routes as R
from tests.helpers import weights_for

MODELS = ["paella", "vqmodel"]
SEED_B = G.WEIGHT_SEED + 11


def _new(kind, seed=G.WEIGHT_SEED):
    if kind == "paella":
        m = paella_amd.Paella(**G.UNET_TINY)
        return m, weights_for(m, sum(G.UNET_TINY["blocks"]), seed=seed)
    m = paella_amd.VQModel(**G.VQ_TINY_F8)
    return m, weights_for(m, G.VQ_TINY_F8["bottleneck_blocks"], seed=seed)


@pytest.fixture(scope="module")
def sd_b():
    """the state dicts the routes lead to, computed once (nobody writes to them: weight_routes hands the modules copies)"""
    return {kind: _new(kind, SEED_B)[1] for kind in MODELS}


@pytest.mark.parametrize("route", R.ROUTE_NAMES)
@pytest.mark.parametrize("kind", MODELS)
def test_route_against_its_contract(kind, route, sd_b):
    """the module holds the new values after the route; an AUTO route changed the signature; after the REFRESH route, refresh() leaves no loaded signature, so
    the next `_engine()` reloads whatever the signature says"""
    m, sd_a = _new(kind)
    new = sd_b[kind]
    assert any(not torch.equal(sd_a[k], new[k]) for k in new)
    before = m._signature()
    m._loaded_sig = before                      # as after a first forward (the handle itself is never looked at here)
    R.BY_NAME[route].apply(m, new)
    R.assert_holds(m, new)
    assert R.home(m).type == "cpu" and all(t.dtype == new[k].dtype for k, t in m.state_dict().items())
    after = m._signature()
    if R.BY_NAME[route].contract == R.AUTO:
        assert after != before, "%s: the weights changed and the signature did not -- the engine would keep the old weights" % route
        assert after != m._loaded_sig
    else:
        m.refresh()
        assert m._loaded_sig is None
        m._signature()


def _assert_lists_the_current_tensors(m):
    """the list the signature walks: the module's current tensors, one entry per state-dict key"""
    listed = m.__dict__["_sig_tensors"]
    assert len(listed) == len(m.state_dict()) and {id(t) for t in listed} == {id(R.tensor_of(h, n, b)) for _, h, n, b in R.slots(m)}


@pytest.mark.parametrize("kind", MODELS)
def test_untouched_module_keeps_its_signature_and_its_list(kind):
    """two calls: equal signatures and the SAME list object (the hot path walks no module tree); a registration on an unrelated module makes the next call walk
    again, which finds the same tensors and keeps list and signature"""
    m, _ = _new(kind)
    s1 = m._signature()
    cached = m.__dict__["_sig_tensors"]
    s2 = m._signature()
    assert s1 == s2 and m.__dict__["_sig_tensors"] is cached
    walks = []
    real = type(m).parameters
    try:
        type(m).parameters = lambda self, *a, **k: (walks.append(1), real(self, *a, **k))[1]
        m._signature()
        assert not walks, "a call on an untouched module walked the module tree"
        nn.Linear(2, 2)                          # registers two Parameters somewhere else in the process
        s3 = m._signature()
        assert len(walks) == 1
        m._signature()
        assert len(walks) == 1
    finally:
        del type(m).parameters
    assert s3 == s1 and m.__dict__["_sig_tensors"] is cached


@pytest.mark.parametrize("kind", MODELS)
def test_new_object_on_the_same_storage_is_a_change(kind):
    """a new Parameter object that shares the old one's storage has the old pointer: the signature differs all the same"""
    m, _ = _new(kind)
    before = m._signature()
    _, holder, name, _b = next(s for s in R.slots(m) if not s[3])
    old = holder._parameters[name]
    setattr(holder, name, nn.Parameter(old.data))
    assert holder._parameters[name] is not old and holder._parameters[name].data_ptr() == old.data_ptr()
    assert m._signature() != before
    _assert_lists_the_current_tensors(m)


def test_vqmodel_buffer_swap_is_a_change():
    """register_buffer of a new tensor over the BatchNorm statistics (the VQModel's signature covers buffers)"""
    m, _ = _new("vqmodel")
    bn = m.down_blocks[-1]._modules["1"]
    before = m._signature()
    bn.register_buffer("running_var", bn.running_var.detach().clone() * 2.0)
    mid = m._signature()
    assert mid != before
    bn.running_mean = bn.running_mean.detach().clone() + 1.0      # attribute assignment over a buffer
    assert m._signature() not in (before, mid)
    _assert_lists_the_current_tensors(m)


# ---------------------------------------------------------------------------------------------------------------------
# copies
# ---------------------------------------------------------------------------------------------------------------------
class _NoLibrary:
    """stands where the native library would be: counts the destroy calls, offers nothing else"""

    def __init__(self):
        self.destroyed = []

    def paella_unet_destroy(self, h):
        self.destroyed.append(h)

    paella_vqgan_destroy = paella_unet_destroy


def _deepcopy(m):
    return copy.deepcopy(m)


def _pickle(m):
    return pickle.loads(pickle.dumps(m))


def _torch_save(m):
    f = io.BytesIO()
    torch.save(m, f)
    f.seek(0)
    return torch.load(f, weights_only=False)


@pytest.mark.parametrize("how", [_deepcopy, _pickle, _torch_save], ids=["deepcopy", "pickle", "torch_save"])
@pytest.mark.parametrize("kind", MODELS)
def test_copy_of_a_module_that_has_run(monkeypatch, kind, how):
    """A module with a native handle (a stand-in: nothing native is touched) copies; the copy takes the tensors and the settings and none of the engine state, and
    the original keeps its own.  Deleting the copy destroys nothing."""
    gc.collect()  # modules that earlier tests left in reference cycles are finalised now, through the real library, and not by the collection below
    lib = _NoLibrary()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    m, sd = _new(kind)
    m._precision = 1
    switches = training.TRAIN_SWITCHES if kind == "paella" else ()
    if kind == "paella":
        m.set_training_route(**{s.name: s.on for s in switches})
    handle = ctypes.c_void_p(0)
    m._handle, m._loaded_sig, m._ws, m._load_gen = handle, m._signature(), torch.zeros(8, dtype=torch.uint8), 7
    try:
        c = how(m)
        assert c is not m and type(c) is type(m)
        assert c._handle is None and c._loaded_sig is None and c._ws is None and c._load_gen == 0
        assert not any(k.startswith("_sig_") for k in c.__dict__), "the copy carries the original's tensor list"
        got = c.state_dict()
        assert sorted(got.keys()) == sorted(sd.keys())
        for k, v in got.items():
            assert torch.equal(v, sd[k]) and v.data_ptr() != m.state_dict()[k].data_ptr(), k
        assert c._cfg == m._cfg and c._cfg is not m._cfg and c._precision == 1 and c.training == m.training
        for s in switches:
            assert getattr(c, s.attr) == s.on
        if kind == "vqmodel":
            assert c.vquantizer._owner[0] is c, "the copy's quantiser still calls the original"
        assert len(c._signature()) == len(m._signature()) and c._signature() != m._signature()
        # the original is as it was
        assert m._handle is handle and m._loaded_sig == m._signature() and m._ws is not None and m._load_gen == 7
        del c, got
        gc.collect()
        assert lib.destroyed == [], "deleting the copy destroyed a native model"
    finally:
        m._handle = None


# ---------------------------------------------------------------------------------------------------------------------
# the engine's life, as far as a module without a device shows it (`paella_amd.modules._NativeModel`, one implementation for both classes)
# ---------------------------------------------------------------------------------------------------------------------
def _engine_fields(m):
    return m._handle, m._loaded_sig, m._load_gen, m._ws, m._precision


@pytest.mark.parametrize("kind", MODELS)
def test_gemm_precision_without_an_engine(kind):
    """set_gemm_precision stores the mode, drops the module's workspace (the fast mode needs another size) and returns the module; get_gemm_precision reads it
    back; anything but the two modes is refused and changes nothing.  No native model is made on the way."""
    m, _ = _new(kind)
    assert _engine_fields(m) == (None, None, 0, None, 0) and m.get_gemm_precision() == "fp32"
    for mode, stored in (("bf16", 1), ("fp32", 0), ("bf16", 1), ("f32", 0), ("bf16", 1)):
        m._ws = torch.zeros(8, dtype=torch.uint8)
        assert m.set_gemm_precision(mode) is m
        assert m._precision == stored and m._ws is None and m.get_gemm_precision() == ("bf16" if stored else "fp32")
    m._ws = ws = torch.zeros(8, dtype=torch.uint8)
    for bad in ("fp16", "BF16", "", None, 1):
        with pytest.raises(ValueError, match="^gemm precision must be 'fp32' or 'bf16'$"):
            m.set_gemm_precision(bad)
        assert m._precision == 1 and m._ws is ws and m.get_gemm_precision() == "bf16"
    assert m._handle is None and m._loaded_sig is None and m._load_gen == 0
    # each class documents what ITS fast mode covers
    assert "paella_%s_set_precision" % ("unet" if kind == "paella" else "vqgan") in type(m).set_gemm_precision.__doc__


@pytest.mark.parametrize("kind", MODELS)
def test_engine_refuses_a_cpu_module_and_names_the_class(kind):
    m, _ = _new(kind)
    want = r"^paella_amd\.%s executes only on a HIP device \(module is on 'cpu'\); move it with \.to\('cuda'\)\. There is no CPU fallback\.$" % type(m).__name__
    for _ in range(2):
        with pytest.raises(RuntimeError, match=want):
            m._engine()
        assert _engine_fields(m) == (None, None, 0, None, 0)

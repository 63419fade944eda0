"""CPU: per-request prompt weights -- the `KeyWeights` table, the normalisation and validation of `attn_weights` per request (vector / list / pair / None), and
the new entry points of the built library."""
import re

import pytest
import torch

from oracle import golden_configs as G
from paella_amd import KeyWeights, sampling


def test_key_weights_set_writes_in_place():
    kw = KeyWeights(4, 6, "cpu")
    assert kw.buf.shape == (4, 6) and kw.buf.dtype == torch.float32 and kw.lens.dtype == torch.int32 and kw.lens.tolist() == [0] * 4
    assert (kw.nb, kw.pitch) == (4, 6)
    buf, lens = kw.buf.data_ptr(), kw.lens.data_ptr()
    kw.set(1, torch.tensor([2.0, 0.5, 1.0])).set(3, [0.25] * 6).set(2, torch.tensor([1, 2]))      # any dtype, any sequence
    assert kw.lens.tolist() == [0, 3, 2, 6] and kw.buf[1, :3].tolist() == [2.0, 0.5, 1.0] and kw.buf[2, :2].tolist() == [1.0, 2.0]
    kw.set(1, None)                       # the count alone says "unweighted": the row keeps whatever it held
    assert kw.lens.tolist() == [0, 0, 2, 6] and kw.buf[1, 0] == 2.0
    kw.set(3, torch.zeros(0))
    assert kw.lens.tolist() == [0, 0, 2, 0]
    assert (kw.buf.data_ptr(), kw.lens.data_ptr()) == (buf, lens)
    kw.clear()
    assert kw.lens.tolist() == [0] * 4
    with pytest.raises(ValueError, match="attn_weights"):
        kw.set(0, torch.ones(7))
    with pytest.raises(ValueError, match="1-D"):
        kw.set(0, torch.ones(2, 2))
    with pytest.raises(IndexError):
        kw.set(4, None)
    with pytest.raises(ValueError):
        KeyWeights(0, 4, "cpu")
    with pytest.raises(ValueError):
        KeyWeights(2, 0, "cpu")


def test_request_weight_forms():
    w, v = torch.tensor([1.0, 2.0]), torch.tensor([0.5])
    assert sampling.request_weight_pair(None) == (None, None)
    c, u = sampling.request_weight_pair(w)
    assert torch.equal(c, w) and u is c
    c, u = sampling.request_weight_pair((w, None))
    assert torch.equal(c, w) and u is None
    c, u = sampling.request_weight_pair([None, v.double()])
    assert c is None and u.dtype == torch.float32 and torch.equal(u, v)
    for bad in (3.0, (w,), (w, v, v), (w, 2.0), "w", torch.ones(2, 2), (torch.ones(2, 2), None)):
        with pytest.raises(ValueError, match="attn_weights"):
            sampling.request_weight_pair(bad)
    # the argument of a whole batch: one vector keeps the shared path, a list becomes one pair per request
    assert sampling.split_request_weights(None, 3) == (None, None)
    shared, pairs = sampling.split_request_weights(w, 3)
    assert shared is w and pairs is None
    shared, pairs = sampling.split_request_weights([w, None, (v, None)], 3)
    assert shared is None and len(pairs) == 3 and pairs[1] == (None, None) and pairs[2][1] is None and torch.equal(pairs[0][1], w)
    for bad, n in (([w, None], 3), ((w, None, None), 3), ([], 1), (torch.ones(2, 2), 2)):
        with pytest.raises(ValueError, match="attn_weights"):
            sampling.split_request_weights(bad, n)


def test_weight_pair_validation():
    w4, w9 = torch.ones(4), torch.ones(9)
    ok = sampling.check_weight_pair((w4, None), (11, 9), True, 8)
    assert ok[0] is w4 and ok[1] is None
    assert sampling.check_weight_pair((w9, w9), (11, 9), True) == (w9, w9)
    with pytest.raises(ValueError, match="attn_weights.*max_attn_weights"):
        sampling.check_weight_pair((w9, None), (11, 11), True, 8)
    with pytest.raises(ValueError, match="attn_weights.*unconditional.*8 keys"):
        sampling.check_weight_pair((None, w9), (11, 8), True)
    with pytest.raises(ValueError, match="attn_weights.*conditional"):
        sampling.check_weight_pair((w9, None), (8, 11), True)
    # an unguided request has one side; the vector given for "both" weighs it
    assert sampling.check_weight_pair((w4, w4), (11, None), False) == (w4, None)
    with pytest.raises(ValueError, match="unguided"):
        sampling.check_weight_pair((w4, torch.ones(2)), (11, None), False)
    assert sampling.check_weight_pair((w9, w9), (None, None), True) == (w9, w9)      # a model without attention: nothing to exceed
    # the side's shortest key sequence: the smallest attention level's self keys + that side's rows
    assert sampling.min_attention_keys(G.UNET_TINY, 16, 16, 7) == 4 + 7 and sampling.min_attention_keys(G.UNET_TINY, 32, 32, 5) == 16 + 5
    for bad in (0, -1, 2.0, True, "8"):
        with pytest.raises(ValueError, match="max_attn_weights"):
            sampling.check_max_attn_weights(bad)
    assert sampling.check_max_attn_weights(8) == 8


def test_load_key_weights_fills_both_halves():
    kw = KeyWeights(6, 8, "cpu")
    kw.lens.fill_(5)
    a, b = torch.tensor([2.0, 3.0]), torch.tensor([0.5])
    sampling._load_key_weights(kw, [(a, a), (None, None), (b, None)], (11, 11), True, 8)
    assert kw.lens.tolist() == [2, 0, 1, 2, 0, 0] and kw.buf[3, :2].tolist() == [2.0, 3.0]
    one = KeyWeights(3, 8, "cpu")
    sampling._load_key_weights(one, [(a, a), (None, None), (b, None)], (11, None), False, 8)
    assert one.lens.tolist() == [2, 0, 1]
    with pytest.raises(ValueError, match=r"attn_weights\[2\]"):
        sampling._load_key_weights(kw, [(a, a), (None, None), (torch.ones(12), None)], (11, 11), True, 64)


def test_new_symbols_and_argument_counts(built_lib):
    """the new entry points are exported, and the binding declares as many arguments as the header / the hook header"""
    import os
    from paella_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "paella_hip.h")).read() + open(os.path.join(root, "paella_amd", "csrc", "test_hooks.h")).read(), flags=re.S)
    want = {"paella_op_attention_kw": 17, "paella_unet_forward_shared_req_kw": 18, "paella_unet_forward_sample_req_kw": 27, "paella_unet_forward_sample_stream_kw": 28,
            "paella_test_attention_bf16_kw": 17}
    for name, n in want.items():
        assert hasattr(built_lib, name), name
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert m, name + " is not declared"
        assert len(m.group(1).split(",")) == n, name
        table = _lib.SIGNATURES if name in _lib.SIGNATURES else _lib.TEST_HOOKS
        assert len(table[name][1]) == n, name
    assert built_lib.paella_abi_version() == 8
    # host-side argument validation of the op entry point: a count table without the weight table (nothing is launched)
    assert built_lib.paella_op_attention_kw(None, None, None, None, None, None, 1, 4, 16, 16, 16, 16, None, None, 1, 4, None) == -1
    assert b"kw_table" in built_lib.paella_last_error()


def test_mutual_exclusion_and_batch_shape_without_a_gpu():
    """the refusals that come before any device work: a stream / a captured sampler takes max_attn_weights (the per-request table) or attn_weights (one vector
    for its life), never both; a guided list call needs both conditioning sets at the batch size (one table row per conditioning slot)"""
    import paella_amd
    from tests.helpers import cond_for
    cfg = G.UNET_TINY
    m = paella_amd.Paella(**cfg)
    c, u = cond_for(cfg, 1, 3, 0, 1), cond_for(cfg, 1, 3, 0, 2)
    w = torch.ones(4)
    with pytest.raises(ValueError, match="max_attn_weights.*attn_weights.*mutually exclusive"):
        paella_amd.RequestStream(m, c, u, (2, 16, 16), max_steps=4, device="cuda", max_attn_weights=8, attn_weights=w)
    with pytest.raises(ValueError, match="max_attn_weights.*attn_weights.*mutually exclusive"):
        paella_amd.GraphRequestSampler(m, c, u, (1, 16, 16), steps=3, device="cuda", max_attn_weights=8, attn_weights=w)
    with pytest.raises(ValueError, match="max_attn_weights"):
        paella_amd.RequestStream(m, c, u, (2, 16, 16), max_steps=4, device="cuda", max_attn_weights=0)
    with pytest.raises(ValueError, match="max_attn_weights"):
        paella_amd.GraphRequestSampler(m, c, u, (1, 16, 16), steps=3, device="cuda", max_attn_weights=-2)
    with pytest.raises(ValueError, match="attn_weights.*2B conditioning slots"):
        paella_amd.sample_requests(m, c, u, (2, 16, 16), [1, 2], steps=3, device="cuda", attn_weights=[w, None])       # conditioning of ONE sample for two requests
    with pytest.raises(ValueError, match="attn_weights"):
        paella_amd.sample_requests(m, c, u, (1, 16, 16), [1], steps=3, device="cuda", attn_weights=[w, None])          # wrong list length

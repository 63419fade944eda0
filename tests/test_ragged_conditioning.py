"""CPU: ragged conditioning (ABI 8) -- the header, the ctypes table and the library agree on the new entry points; the host arithmetic of the 2B-slot cache
and the host validation of `RequestStream(max_cond_rows=...)` against hand-computed cases."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_PUBLIC = ["paella_unet_cond_prepare_slots", "paella_op_attention_ragged", "paella_unet_forward_shared_ragged", "paella_unet_forward_sample_ragged",
              "paella_unet_forward_shared_req_ragged", "paella_unet_forward_sample_req_ragged", "paella_unet_forward_sample_stream_ragged"]
NEW_HOOKS = ["paella_test_attention_bf16_ragged"]


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, path)).read(), flags=re.S)
    return src, set(re.findall(r"\b(paella_[a-z0-9_]+)\s*\(", src))


def test_abi_version_is_8(built_lib):
    from paella_amd import _lib
    src, _ = _declared("include/paella_hip.h")
    assert re.search(r"#define\s+PAELLA_ABI_VERSION\s+8\b", src)
    assert _lib.ABI_VERSION == 8 and built_lib.paella_abi_version() == 8


def test_new_symbols_declared_bound_and_exported(built_lib):
    from paella_amd import _lib
    _, public = _declared("include/paella_hip.h")
    _, hooks = _declared("paella_amd/csrc/test_hooks.h")
    raw = ctypes.CDLL(os.path.join(ROOT, "paella_amd", "csrc", "libpaella_hip.so"))
    for n in NEW_PUBLIC:
        assert n in public and n in _lib.SIGNATURES and hasattr(raw, n), n
    for n in NEW_HOOKS:
        assert n in hooks and n not in public and n in _lib.TEST_HOOKS and hasattr(raw, n), n


def test_ragged_twins_take_cond_len_right_after_S():
    """every twin's ctypes signature is its plain form's with ONE pointer inserted after S (argument 10 of the forward forms, after Lcond for the op)"""
    from paella_amd import _lib
    for plain, at in [("paella_unet_forward_shared", 11), ("paella_unet_forward_sample", 11), ("paella_unet_forward_shared_req", 10),
                      ("paella_unet_forward_sample_req", 10), ("paella_unet_forward_sample_stream", 10), ("paella_op_attention", 12)]:
        res, args = _lib.SIGNATURES[plain]
        rres, rargs = _lib.SIGNATURES[plain + "_ragged"]
        assert rres is res and list(rargs) == list(args[:at]) + [ctypes.c_void_p] + list(args[at:]), plain
        assert args[at - 1] is ctypes.c_int  # S / Lcond
    res, args = _lib.TEST_HOOKS["paella_test_attention_bf16"]
    assert list(_lib.TEST_HOOKS["paella_test_attention_bf16_ragged"][1]) == list(args[:12]) + [ctypes.c_void_p] + list(args[12:])
    # the slot form of cond_prepare: (S_slot, slot0) after B, the cond_len table after the cache and its size
    plain = list(_lib.SIGNATURES["paella_unet_cond_prepare"][1])
    assert list(_lib.SIGNATURES["paella_unet_cond_prepare_slots"][1]) == plain[:7] + [ctypes.c_int, ctypes.c_int] + plain[7:9] + [ctypes.c_void_p] + plain[9:]


def test_header_declares_cond_len_after_S():
    src, _ = _declared("include/paella_hip.h")
    for n in NEW_PUBLIC[2:]:
        proto = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % n, src).group(1)
        assert re.search(r"int\s+S\s*,\s*const\s+int\s*\*\s*cond_len\s*,", proto), n
    proto = re.search(r"\bpaella_op_attention_ragged\s*\(([^;]*)\)\s*;", src).group(1)
    assert re.search(r"int\s+Lcond\s*,\s*const\s+int\s*\*\s*cond_len\s*,", proto)


def test_slot_plan_hand_computed():
    from paella_amd.sampling import ragged_slot_plan
    # 13 conditional rows against 6 unconditional, B = 2, 256 bytes per cache row: pitch 13, slots of 3328 bytes
    p = ragged_slot_plan(13, 6, 2, 256)
    assert p["pitch"] == 13 and p["lens"] == [13, 13, 6, 6]
    assert p["slot_bytes"] == 3328 and p["offsets"] == [0, 3328, 6656, 9984] and p["group_offsets"] == (0, 6656) and p["nbytes"] == 13312
    # the unconditional side is the longer one; B = 1
    p = ragged_slot_plan(5, 72, 1, 4 * 2560)
    assert p["pitch"] == 72 and p["lens"] == [5, 72] and p["offsets"] == [0, 737280] and p["group_offsets"] == (0, 737280) and p["nbytes"] == 1474560
    # equal lengths degenerate to the plain layout: B * S rows per group
    p = ragged_slot_plan(7, 7, 3, 64)
    assert p["pitch"] == 7 and p["lens"] == [7] * 6 and p["offsets"] == [448 * b for b in range(6)] and p["group_offsets"] == (0, 1344) and p["nbytes"] == 2688
    for bad in [(0, 6, 2, 256), (13, 0, 2, 256), (13, 6, 0, 256)]:
        with pytest.raises(ValueError):
            ragged_slot_plan(*bad)


def test_cond_seq_len_counts_every_clip_image():
    """rows of a request = ByT5 length + clip_seq_len * [clip] + clip_seq_len * #clip_image"""
    from types import SimpleNamespace
    from paella_amd.sampling import _cond_batch, _cond_seq_len
    m = SimpleNamespace(_cfg={"clip_seq_len": 4})
    z = lambda *s: torch.zeros(*s)
    assert _cond_seq_len(m, {"byt5": z(2, 5, 8), "clip": z(2, 6), "clip_image": z(2, 6)}) == 13
    assert _cond_seq_len(m, {"byt5": z(2, 2, 8), "clip": z(2, 6), "clip_image": None}) == 6
    assert _cond_seq_len(m, {"byt5": z(1, 64, 8), "clip": z(1, 6), "clip_image": [z(1, 6), z(1, 6)]}) == 76
    assert _cond_batch({"byt5": z(3, 1, 8), "clip": None, "clip_image": None}) == 3 and _cond_batch(None) is None


def test_max_cond_rows_and_attn_weights_validation():
    from paella_amd.sampling import check_ragged_stream_args, check_request_rows, min_attention_keys
    assert check_ragged_stream_args(16, 0, 17) == 16
    for bad in (0, -3, 2.5, True, "16"):
        with pytest.raises(ValueError, match="max_cond_rows"):
            check_ragged_stream_args(bad, 0, 17)
    # the two-level toy model: attention on level 1 only, patch 2 -> a 32x32 grid has 8x8 = 64 self keys there; with one conditioning row, 65 keys
    cfg = dict(patch_size=2, level_config=["CT", "CTA"], self_attn=True)
    assert min_attention_keys(cfg, 32, 32, 1) == 65
    assert min_attention_keys(dict(cfg, self_attn=False), 32, 32, 1) == 1
    assert min_attention_keys(dict(cfg, level_config=["CTA", "CTA", "CTA"]), 32, 16, 2) == 4 * 2 + 2
    assert min_attention_keys(dict(cfg, level_config=["CT", "CT"]), 32, 32, 1) is None
    assert check_ragged_stream_args(16, 65, 65) == 16
    with pytest.raises(ValueError, match="attn_weights"):
        check_ragged_stream_args(16, 66, 65)
    with pytest.raises(ValueError, match="attn_weights"):
        check_ragged_stream_args(16, 2, 1)
    assert check_request_rows(1, 16, "x") == 1 and check_request_rows(16, 16, "x") == 16
    for rows in (0, 17, 100):
        with pytest.raises(ValueError, match="max_cond_rows"):
            check_request_rows(rows, 16, "model_inputs")


def test_cond_cache_has_lens():
    from paella_amd import CondCache
    assert CondCache(None, 2, 5).lens is None
    t = torch.zeros(2, dtype=torch.int32)
    assert CondCache(None, 2, 5, t).lens is t and CondCache(None, 2, 5, lens=t).S == 5

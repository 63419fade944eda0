"""CPU: the host side of editing requests in the request stream -- a numpy transcription of request_step_kernel's pin-policy rule (the model
tests/test_gpu_request_edit.py holds the kernel against), `paella_amd.canvas`, and the header / binding / export lists."""
import os
import re

import numpy as np
import pytest
import torch

import paella_amd
from paella_amd import _lib, editing, sampling
from tests.test_request_stream import IDLE, request_step_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIN_ENTRY_POINTS = ["paella_request_step_pin", "paella_sample_tail_pin", "paella_sample_tail_stream_pin", "paella_unet_forward_sample_pin",
                    "paella_unet_forward_sample_stream_pin"]


def request_step_pin_model(program, pos, length, policy):
    """tail.hip: request_step_kernel with a policy table.  The flat tables are those of `request_step_model` (pos is advanced in place); on top of them
    pin_on[b] = 1 for a running slot under policy 1, under policy 2 exactly when this tick is the request's last (p + 1 == len[b]), else 0 -- idle slots 0."""
    before = pos.copy()
    tables = request_step_model(program, pos, length)
    active = tables[5]
    pin_on = np.zeros(len(pos), np.int32)
    for b in range(len(pos)):
        pol = int(policy[b])
        pin_on[b] = int(bool(active[b]) and (pol == 1 or (pol == 2 and int(before[b]) + 1 == int(length[b]))))
    return tables + (pin_on,)


@pytest.mark.parametrize("max_steps", [1, 4])
def test_pin_policy_model(max_steps):
    """every policy against every slot state: lengths 1 and max_steps, a slot at its last step, one mid-flight, an idle slot (length 0) and a cursor already at
    its length"""
    states = [(0, 1), (0, max_steps), (max_steps - 1, max_steps), (0, 0), (max_steps, max_steps), (1, 1)]
    if max_steps > 2:
        states.append((1, max_steps))  # mid-flight
    for pol in (0, 1, 2):
        B = len(states)
        program = np.arange(B * max_steps * 5, dtype=np.float32).reshape(B, max_steps, 5)
        pos, length = np.int32([s[0] for s in states]), np.int32([s[1] for s in states])
        before = pos.copy()
        out = request_step_pin_model(program, pos, length, np.full(B, pol, np.int32))
        active, pin_on = out[5], out[6]
        for b, (p, n) in enumerate(states):
            running = p < n
            assert active[b] == int(running)
            want = {0: 0, 1: int(running), 2: int(running and p + 1 == n)}[pol]
            assert pin_on[b] == want, (pol, p, n)
            assert pos[b] == before[b] + int(running)
            if not running:
                assert np.array_equal(np.float32([out[0][b], out[1][b], out[2][b, 0], out[2][b, 1], out[3][b]]), IDLE)


def test_pin_policy_model_over_a_request_life():
    """a 3-step request per policy, driven to the end and two ticks beyond: policy 1 pins at every one of its steps, policy 2 at the third only, nobody afterwards"""
    max_steps = 4
    program = np.tile(IDLE, (3, max_steps, 1))
    pos, length = np.zeros(3, np.int32), np.int32([3, 3, 3])
    policy = np.int32([0, 1, 2])
    seen = [request_step_pin_model(program, pos, length, policy)[6].tolist() for _ in range(5)]
    assert seen == [[0, 1, 0], [0, 1, 0], [0, 1, 1], [0, 0, 0], [0, 0, 0]]
    assert sampling.PIN_POLICY == {"never": 0, "step": 1, "final": 2}


def test_canvas():
    g = torch.Generator().manual_seed(0)
    tok = torch.randint(0, 100, (3, 5), generator=g)
    for off in [(0, 0), (0, 3), (5, 0), (5, 3), (2, 1)]:  # the four corners and the interior of an 8 x 8 canvas
        known, mask = paella_amd.canvas(tok, (8, 8), off)
        assert known.dtype == torch.int64 and mask.dtype == torch.int64 and tuple(known.shape) == (8, 8) == tuple(mask.shape)
        y, x = off
        assert torch.equal(known[y:y + 3, x:x + 5], tok)
        want = torch.ones(8, 8, dtype=torch.int64)
        want[y:y + 3, x:x + 5] = 0
        assert torch.equal(mask, want) and int((known * mask).abs().sum()) == 0
    known, mask = paella_amd.canvas(tok, (3, 5), (0, 0))  # a full-canvas grid: nothing to regenerate
    assert torch.equal(known, tok) and int(mask.sum()) == 0
    kb, mb = paella_amd.canvas(tok[None].repeat(2, 1, 1), (4, 6), (1, 1))  # batched grids
    assert tuple(kb.shape) == (2, 4, 6) and torch.equal(kb[1, 1:, 1:], tok) and int(mb[0].sum()) == 24 - 15
    for bad in [(-1, 0), (0, -1), (6, 0), (0, 4), (8, 8)]:
        with pytest.raises(ValueError, match="canvas"):
            paella_amd.canvas(tok, (8, 8), bad)
    with pytest.raises(ValueError, match="canvas"):
        paella_amd.canvas(tok, (2, 8), (0, 0))
    with pytest.raises(ValueError, match="int64"):
        paella_amd.canvas(tok.float(), (8, 8), (0, 0))


def test_pin_mode_validation():
    assert editing.check_pin_mode("final", True, None) == "final" and editing.check_pin_mode("final", False, "torch") == "final"
    assert editing.check_pin_mode("step", True, "philox") == "step"
    with pytest.raises(ValueError, match="philox"):
        editing.check_pin_mode("step", True, "torch")
    with pytest.raises(ValueError, match="philox"):
        editing.check_pin_mode("step", True, None)
    with pytest.raises(ValueError, match="keep_known"):
        editing.check_pin_mode("step", False, "philox")
    with pytest.raises(ValueError, match="pin must be"):
        editing.check_pin_mode("always", True, "philox")
    # inpaint refuses before it touches its model or the device
    with pytest.raises(ValueError, match="philox"):
        paella_amd.inpaint(None, None, None, None, None, None, pin="step")
    with pytest.raises(ValueError, match="pin must be"):
        paella_amd.inpaint(None, None, None, None, None, None, pin="every", noise="philox")


def test_header_binding_and_exports_name_the_pin_entry_points():
    src = open(os.path.join(ROOT, "include", "paella_hip.h")).read()
    assert re.search(r"#define PAELLA_ABI_VERSION 8\b", src) and _lib.ABI_VERSION == 8
    assert "ADDITIVELY" in src  # the header says that ABI 8 was extended without a version change
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in PIN_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in the header"
        assert name in _lib.SIGNATURES, name + " is not in the binding table"
    assert "canvas" in paella_amd.__all__ and paella_amd.canvas is editing.canvas
    import inspect
    assert inspect.signature(paella_amd.RequestStream.__init__).parameters["editing"].default is False
    adm = inspect.signature(paella_amd.RequestStream.admit).parameters
    assert [adm[k].default for k in ("known", "mask", "image", "pin")] == [None, None, None, "step"]
    assert inspect.signature(paella_amd.inpaint).parameters["pin"].default == "final"
    assert inspect.signature(paella_amd.GraphInpainter.__init__).parameters["pin"].default == "final"
    fs = inspect.signature(paella_amd.Paella.forward_sample).parameters["pin"]
    assert fs.default is None and fs.kind is inspect.Parameter.KEYWORD_ONLY


def test_library_exports_the_pin_entry_points_and_keeps_abi_8(built_lib):
    for name in PIN_ENTRY_POINTS:
        assert hasattr(built_lib, name)
    assert built_lib.paella_abi_version() == 8
    # host-side argument checks of the step entry point run before any device work
    assert built_lib.paella_request_step_pin(None, 4, None, None, 2, None, None, None, None, None, None, None, None, None) == -1

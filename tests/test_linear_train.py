"""Training linear on bf16 operands without a GPU: the switch validates its argument and leaves a CPU train step alone, bit for bit; `linear_shapes_ok` states the
rule the C entry points enforce; the ABI exports the four new symbols; the C entry points validate their arguments on the host before anything is enqueued; the
Python surface refuses what the op cannot do instead of falling back."""
import itertools
import os
import re

import pytest
import torch

import paella_amd
from oracle import golden_configs as G
from paella_amd import _lib, training
from tests import train_op_checks as T

ERR_ARG, ERR_WORKSPACE = -1, -3
SYMBOLS = ("paella_linear_train_workspace_bytes", "paella_linear_train_forward", "paella_linear_train_backward", "paella_pack_bf16")
HEADER = 1 << 18            # the ticket header of a split-K region
SPLIT = HEADER + (64 << 20)  # the split-K region at the start of a linear's workspace


def test_set_training_gemm():
    """(what every switch's setter does: tests/test_training.py::test_training_switch)  Its own: independent of the inference precision, in both directions"""
    names = set(dir(paella_amd))
    m = paella_amd.Paella(**G.UNET_TINY)
    assert m.set_training_gemm("bf16")._train_gemm == "bf16" and m.get_gemm_precision() == "fp32"
    m.set_gemm_precision("bf16")
    assert m._train_gemm == "bf16"
    assert m.set_training_gemm("fp32")._train_gemm == "fp32" and m.get_gemm_precision() == "bf16"
    assert set(training.LINEAR_COUNTERS) == {"calls", "backward", "fallbacks", "copied"}
    # nothing new at the package root beyond the method
    assert set(dir(paella_amd)) == names and not [n for n in dir(paella_amd) if "linear_bf16" in n or n.startswith("LINEAR")]


@pytest.mark.parametrize("others", ["torch", "hip"])
def test_the_switch_leaves_a_cpu_train_step_alone(others):
    before = dict(training.LINEAR_COUNTERS)
    T.assert_switch_leaves_a_cpu_train_step_alone(
        lambda m: m.set_training_gemm("bf16"),
        before=lambda m: m.set_training_activation(others).set_training_depthwise(others).set_training_attention(others).set_training_modulation(others))
    assert training.LINEAR_COUNTERS == before


def test_linear_shapes_ok_matches_the_c_rule(built_lib):
    size = built_lib.paella_linear_train_workspace_bytes
    values = (-64, 0, 1, 32, 63, 64, 65, 96, 128, 192, 320, 1280, 4160, (1 << 22) - 128, (1 << 22) - 64, 1 << 22, (1 << 22) + 64)
    for M, N, K in itertools.product(values, (0, 32, 64, 96, 1280, (1 << 22) + 64), (0, 32, 64, 100, 5120)):
        ok = training.linear_shapes_ok(M, N, K)
        assert ok == (M > 0 and N > 0 and K > 0 and M % 64 == 0 and N % 64 == 0 and K % 64 == 0 and max(M, N, K) <= 65535 * 64), (M, N, K)
        for direction, wants in ((0, 0), (1, 7), (1, 1)):
            assert (size(M, N, K, direction, wants) > 0) == ok, (M, N, K, direction, wants)
    assert not training.linear_shapes_ok(64.0, 64, 64)
    assert (training.LINEAR_GRAIN, training.LINEAR_MAX_DIM) == (64, 65535 * 64)       # 65535 tiles: the largest y extent of a grid, where the pack puts its column tiles
    assert size(64, 64, 64, 2, 0) == 0 and size(64, 64, 64, 1, 8) == 0


def test_abi_exports_the_new_symbols(built_lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "paella_hip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and callable(getattr(built_lib, name))
        assert re.search(r"\b%s\(" % name, header), name
    assert built_lib.paella_abi_version() == 8


def test_workspace_layout(built_lib):
    size = built_lib.paella_linear_train_workspace_bytes
    r256 = lambda n: (n + 255) // 256 * 256
    for M, N, K in [(64, 64, 64), (128, 192, 320), (8192, 64, 64), (256, 1280, 320), (16384, 5120, 1280), (4160, 128, 64)]:
        assert size(M, N, K, 0, 0) == size(M, N, K, 0, 7) == SPLIT + r256(M * K * 2) + r256(N * K * 2)
        tiles = M // 64
        per = max(4, -(-tiles // 256))
        strips = -(-tiles // per)
        part = r256(strips * N * 8) if strips > 1 else 0
        dy16, x16t, w16t = r256(M * N * 2), r256(M * K * 2), r256(N * K * 2)
        assert size(M, N, K, 1, 0) == SPLIT
        assert size(M, N, K, 1, 1) == SPLIT + dy16 + w16t                    # dx alone: neither x, nor the transposed dy, nor the partials of db
        assert size(M, N, K, 1, 2) == SPLIT + dy16 + x16t
        assert size(M, N, K, 1, 4) == SPLIT + part
        assert size(M, N, K, 1, 7) == SPLIT + 2 * dy16 + x16t + w16t + part


def test_entry_points_validate_on_the_host(built_lib):
    """every refusal below returns before anything is enqueued: the pointers are made-up addresses that no kernel may touch"""
    lib = built_lib
    good, off = 1 << 20, (1 << 20) + 8
    M, N, K = 128, 192, 320

    def fwd(M=M, N=N, K=K, x=good, w=good, bias=good, y=good, ws=good, ws_bytes=None):
        ws_bytes = lib.paella_linear_train_workspace_bytes(128, 192, 320, 0, 0) if ws_bytes is None else ws_bytes
        return lib.paella_linear_train_forward(x, w, bias, y, M, N, K, ws, ws_bytes, None)

    def bwd(M=M, N=N, K=K, x=good, w=good, dy=good, dx=good, dw=good, db=good, ws=good, ws_bytes=None):
        ws_bytes = lib.paella_linear_train_workspace_bytes(128, 192, 320, 1, 7) if ws_bytes is None else ws_bytes
        return lib.paella_linear_train_backward(x, w, dy, dx, dw, db, M, N, K, ws, ws_bytes, None)

    def pack(rows=128, cols=192, src=good, row=good, tr=good, cs=good, ws=good, ws_bytes=1 << 20):
        return lib.paella_pack_bf16(src, rows, cols, row, tr, cs, ws, ws_bytes, None)

    for call in (fwd, bwd):
        for bad in (dict(M=96), dict(M=0), dict(M=-64), dict(N=32), dict(N=100), dict(K=32), dict(K=0), dict(K=1 << 22), dict(M=(1 << 22) + 64)):
            assert call(**bad) == ERR_ARG, (call.__name__, bad)
            msg = lib.paella_last_error()
            assert b"M=" in msg and b"N=" in msg and b"K=" in msg and b"multiples of 64" in msg, msg
        for bad in (dict(x=off), dict(w=off), dict(ws=off)):
            assert call(**bad) == ERR_ARG and b"16-byte aligned" in lib.paella_last_error(), (call.__name__, bad)
        assert call(ws=None) == ERR_WORKSPACE and call(ws_bytes=SPLIT) == ERR_WORKSPACE and b"workspace" in lib.paella_last_error()
    for bad in (dict(x=None), dict(w=None), dict(y=None)):
        assert fwd(**bad) == ERR_ARG and b"x, w and y are required" in lib.paella_last_error(), bad
    assert fwd(bias=off) == ERR_ARG and fwd(y=off) == ERR_ARG
    for bad in (dict(dy=None), dict(w=None), dict(x=None)):
        assert bwd(**bad) == ERR_ARG and b"dy is required, and w for dx_out, x for dw_out" in lib.paella_last_error(), bad
    for bad in (dict(dy=off), dict(dx=off), dict(dw=off), dict(db=off)):
        assert bwd(**bad) == ERR_ARG, bad
    # what passes the checks and asks for no output launches nothing; an operand only a skipped gradient needs may be absent
    assert bwd(dx=None, dw=None, db=None, ws_bytes=SPLIT) == 0
    assert bwd(x=None, w=None, dx=None, dw=None, db=None, ws_bytes=SPLIT) == 0
    # the pack
    for bad in (dict(rows=96), dict(rows=0), dict(cols=32), dict(cols=-64), dict(rows=1 << 22), dict(cols=1 << 22)):
        assert pack(**bad) == ERR_ARG and b"rows=" in lib.paella_last_error(), bad
    assert pack(src=None) == ERR_ARG and b"src is required" in lib.paella_last_error()
    assert pack(row=None, tr=None, cs=None) == ERR_ARG and b"at least one" in lib.paella_last_error()
    for bad in (dict(src=off), dict(row=off), dict(tr=off), dict(cs=off)):
        assert pack(**bad) == ERR_ARG and b"16-byte aligned" in lib.paella_last_error(), bad
    # 4160 rows are 65 row tiles = 17 strips of 4: the column sums need 17 x cols doubles, and nothing without them
    assert pack(rows=4160, cols=128, ws=None, ws_bytes=0) == ERR_WORKSPACE
    assert pack(rows=4160, cols=128, ws_bytes=17 * 128 * 8 - 1) == ERR_WORKSPACE and b"workspace" in lib.paella_last_error()
    assert pack(rows=4160, cols=128, ws=off, ws_bytes=1 << 20) == ERR_ARG


def test_linear_bf16_refuses_what_the_op_cannot_do():
    before = dict(training.LINEAR_COUNTERS)
    x, w, b = torch.zeros(2, 64, 128), torch.zeros(192, 128), torch.zeros(192)
    with pytest.raises(ValueError, match="HIP device.*x, weight and bias"):     # cpu tensors: there is no torch fallback
        training.linear_bf16(x, w, b)
    with pytest.raises(ValueError, match="HIP device"):
        training.linear_bf16(x, w)
    for bad in ((x.half(), w, b), (x, w.bfloat16(), b), (x, w, b.double()), (x.long(), w, None)):
        with pytest.raises(ValueError, match="fp32 x, weight and bias"):
            training.linear_bf16(*bad)
    for bad in ((None, w, b), (x, 1.0, b), (x, w, 0.0)):
        with pytest.raises(ValueError, match="tensors"):
            training.linear_bf16(*bad)
    for bad in ((x, w[:, :64], b), (x, w[0], b), (x, w[None], b), (torch.zeros(()), w, b)):
        with pytest.raises(ValueError, match=r"\[N, K\]"):
            training.linear_bf16(*bad)
    for bad_b in (b[:64], b[None], torch.zeros(128)):
        with pytest.raises(ValueError, match=r"bias must be \[N\]"):
            training.linear_bf16(x, w, bad_b)
    with pytest.raises(ValueError, match="M = 96"):
        training.linear_bf16(torch.zeros(96, 128), w, b)
    with pytest.raises(ValueError, match="M = 0"):
        training.linear_bf16(torch.zeros(0, 128), w, b)
    with pytest.raises(ValueError, match="K = 32"):
        training.linear_bf16(torch.zeros(128, 32), torch.zeros(192, 32), b)
    with pytest.raises(ValueError, match="N = 100"):
        training.linear_bf16(x, torch.zeros(100, 128))
    for bad in (torch.zeros(64), torch.zeros(96, 64), torch.zeros(64, 32), torch.zeros(2, 64, 64)):
        with pytest.raises(ValueError, match="multiples of 64"):
            training.pack_bf16(bad)
    with pytest.raises(ValueError, match="fp32"):
        training.pack_bf16(torch.zeros(64, 64).half())
    with pytest.raises(ValueError, match="HIP device"):
        training.pack_bf16(torch.zeros(64, 64))
    assert training.LINEAR_COUNTERS == before

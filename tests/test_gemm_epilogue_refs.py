"""CPU: the references tests/test_gpu_gemm_epilogue_features.py holds the GEMM epilogue against (tests/gemm_epilogue_refs.py) agree with independent torch
operators in fp64, and the test hook that launches a described GEMM refuses, on the host, a launch that could store outside its buffers."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_epilogue_refs as R


def _gen(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)


def _nhwc_rows(x):
    """NCHW -> the project's row-major [B * H * W, C]"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def test_d2s_two_segments_per_row_is_conv_transpose_k2_s2():
    """ConvTranspose2d(k2, s2) as one GEMM with N = 4 co and the depth-to-space store (model.hip: BT_UP)."""
    d = _gen(0)
    B, ci, co, h, w, ldc = 3, 8, 12, 4, 6, 16  # sH != sW, ldc > co
    x, wt, bias = d(B, ci, h, w), d(ci, co, 2, 2), d(co)
    plain = _nhwc_rows(x) @ R.convT2_weight(wt).t() + bias.repeat(4)  # (bias tiled per segment: RP_TILE4)
    idx = R.d2s_index(B * h * w, 4 * co, ldc, h, w, co, 2)
    out = R.scatter(torch.full((B, 2 * h, 2 * w, ldc), float("nan"), dtype=torch.float64), idx, plain)
    ref = F.conv_transpose2d(x, wt, bias, stride=2)
    torch.testing.assert_close(out[..., :co].permute(0, 3, 1, 2), ref, atol=1e-12, rtol=0)
    assert torch.isnan(out[..., co:]).all() and idx.unique().numel() == idx.numel()


def test_d2s_phases_with_the_four_tap_gather_are_conv_transpose_k4_s2_p1():
    """The four output phases of ConvTranspose2d(k4, s2, p1): gather of 2 x 2 taps (tsign = -1) + GEMM + phase store (vqmodel.hip: VQ_CONVT4)."""
    d = _gen(1)
    B, ci, co, h, w = 3, 5, 8, 6, 10
    x, wt, bias = d(B, ci, h, w), d(ci, co, 4, 4), d(co)
    out = torch.full((B, 2 * h, 2 * w, co), float("nan"), dtype=torch.float64)
    seen = torch.zeros(out.numel(), dtype=torch.int64)
    for py in (0, 1):
        for px in (0, 1):
            A = R.conv_gather(x.permute(0, 2, 3, 1).contiguous(), h, w, 1, 4, 1, py, px, -1)
            plain = A @ R.convT4_phase_weight(wt, py, px).t() + bias
            idx = R.d2s_index(B * h * w, co, co, h, w, co, 1, py, px)
            out = R.scatter(out, idx, plain)
            seen[idx.reshape(-1)] += 1
    assert (seen == 1).all()  # the phases tile the output: every element exactly once
    torch.testing.assert_close(out.permute(0, 3, 1, 2), F.conv_transpose2d(x, wt, bias, stride=2, padding=1), atol=1e-12, rtol=0)


def test_sixteen_tap_gather_is_conv_k4_s2_p1():
    d = _gen(2)
    B, ci, co, h, w = 3, 5, 7, 6, 10
    x, wt, bias = d(B, ci, h, w), d(co, ci, 4, 4), d(co)
    A = R.conv_gather(x.permute(0, 2, 3, 1).contiguous(), h // 2, w // 2, 2, 16, 2, -1, -1, 1)
    assert A.shape == (B * (h // 2) * (w // 2), 16 * ci)
    got = (A @ R.conv4s2_weight(wt).t() + bias).reshape(B, h // 2, w // 2, co).permute(0, 3, 1, 2)
    torch.testing.assert_close(got, F.conv2d(x, wt, bias, stride=2, padding=1), atol=1e-12, rtol=0)


def test_pixel_shuffle_nchw_store_is_pixel_shuffle():
    d = _gen(3)
    B, h, w = 3, 5, 7
    plain = d(B * h * w, 12)
    idx = R.pixshuf_index(B * h * w, 12, h, w, 3)
    out = R.scatter(torch.full((B, 3, 2 * h, 2 * w), float("nan"), dtype=torch.float64), idx, plain)
    assert torch.equal(out, F.pixel_shuffle(plain.reshape(B, h, w, 12).permute(0, 3, 1, 2), 2))


@pytest.mark.parametrize("M,rin,rout,roff", [(216, 24, 40, 3), (216, 24, 64, 2 * 64), (50, 7, 7, 0), (10, 0, 0, 0)])
def test_row_remap_against_a_plain_loop(M, rin, rout, roff):
    want = [m if rin == 0 else (m // rin) * rout + m % rin + roff for m in range(M)]
    assert R.remap_rows(M, rin, rout, roff).tolist() == want
    N, ldc = 8, 12
    idx = R.plain_index(M, N, ldc, (rin, rout, roff))
    for m in (0, M // 2, M - 1):
        assert idx[m].tolist() == [want[m] * ldc + n for n in range(N)]


def test_rowstat_partials_and_their_combination_are_mean_and_variance():
    d = _gen(4)
    x = d(37, 336) * 1.7 + 0.6 + torch.arange(336, dtype=torch.float64) * 0.01
    st = R.rowstat_partials(x)
    blk = x.reshape(37, 21, 16)
    torch.testing.assert_close(st[..., 0], blk.sum(-1), atol=1e-12, rtol=0)
    torch.testing.assert_close(st[..., 1], blk.var(-1, unbiased=False) * 16, atol=1e-11, rtol=0)
    mean, rstd = R.rowstat_combine(st, eps=1e-6)
    torch.testing.assert_close(mean, x.mean(-1), atol=1e-13, rtol=0)
    torch.testing.assert_close(rstd, 1.0 / torch.sqrt(x.var(-1, unbiased=False) + 1e-6), atol=0, rtol=1e-12)
    y = (x - mean[:, None]) * rstd[:, None]
    torch.testing.assert_close(y, F.layer_norm(x, (336,), None, None, 1e-6), atol=1e-12, rtol=0)


def test_sumsq_groups_count_the_rows_the_last_group_has():
    d = _gen(5)
    x = d(216, 20)
    q = R.sumsq_groups(x)
    assert q.shape == (14, 20)
    for gi in (0, 7):
        torch.testing.assert_close(q[gi], (x[gi * 16:(gi + 1) * 16] ** 2).sum(0), atol=1e-12, rtol=0)
    torch.testing.assert_close(q[13], (x[208:216] ** 2).sum(0), atol=1e-12, rtol=0)  # the last group: 8 rows


def test_epilogue_value_order():
    d = _gen(6)
    acc, bias, res, a, b = d(48, 8), d(8), d(48, 8), d(2, 8), d(2, 8)
    got = R.epilogue_value(acc, bias, True, 0.37, res, (a, b), 24)
    want = (F.gelu(acc + bias) * 0.37 + res) * (1 + a.repeat_interleave(24, 0)) + b.repeat_interleave(24, 0)
    torch.testing.assert_close(got, want, atol=1e-14, rtol=0)


# ---- the hook's argument block and its host-side capacity check (no device call is reached) ----
def _args(**kw):
    from paella_amd import _lib
    a = _lib.TestGemmArgs()
    a.alpha, a.n_seg_x = 1.0, 2
    a.A = a.W = a.C = 0x1000  # never dereferenced: every case below is refused on the host
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_block_has_the_size_the_library_compiled(built_lib):
    from paella_amd import _lib
    assert ctypes.sizeof(_lib.TestGemmArgs) == built_lib.paella_test_gemm_args_size()


CAPACITY_CASES = [
    # (fields, the capacity field under test, elements the launch needs there)
    (dict(M=216, N=336, K=416, ldc=336), "c_capacity", 216 * 336),
    (dict(M=216, N=336, K=416, ldc=344), "c_capacity", 215 * 344 + 336),
    (dict(M=216, N=336, K=416, ldc=336, remap_in=24, remap_out=40, remap_off=3), "c_capacity", (8 * 40 + 23 + 3) * 336 + 336),
    (dict(M=30, N=16, K=32, ldc=16, remap_in=24, remap_out=8, remap_off=0), "c_capacity", 23 * 16 + 16),  # remap_out < remap_in: the first group ends last
    (dict(M=216, N=336, K=416, ldc=336, c16=0x1000, c_capacity=1 << 30), "c16_capacity", 216 * 336),
    (dict(M=216, N=336, K=416, ldc=336, C=None, c16=0x1000), "c16_capacity", 216 * 336),
    (dict(M=216, N=336, K=416, ldc=96, store_mode=1, sH=4, sW=6, sC=84, n_seg_x=2), "c_capacity", (9 * 8 * 12 - 1) * 96 + 84),
    (dict(M=216, N=336, K=416, ldc=336, store_mode=1, sH=4, sW=6, sC=336, n_seg_x=1, py=1, px=1), "c_capacity", 9 * 8 * 12 * 336),
    (dict(M=216, N=336, K=416, ldc=336, store_mode=1, sH=4, sW=6, sC=336, n_seg_x=1, py=0, px=0), "c_capacity", (9 * 8 * 12 - 1 - 12 - 1) * 336 + 336),
    (dict(M=105, N=12, K=416, ldc=6, store_mode=2, sH=5, sW=7, sC=3), "c_capacity", 3 * 3 * 10 * 14),
    (dict(M=216, N=336, K=416, ldc=336, c_capacity=1 << 30, rowstat_out=0x1000), "rowstat_capacity", 216 * 21 * 2),
    (dict(M=216, N=336, K=416, ldc=336, c_capacity=1 << 30, sumsq_out=0x1000), "sumsq_capacity", 14 * 336),
]


@pytest.mark.parametrize("fields,cap,need", CAPACITY_CASES)
def test_hook_refuses_a_store_past_the_stated_capacity_on_the_host(built_lib, fields, cap, need):
    """One element too few is an error code; with exactly enough the capacity check passes and the NEXT host check refuses (tile id out of range), so no case reaches a device call."""
    a = _args(**fields)
    setattr(a, cap, need - 1)
    assert built_lib.paella_test_gemm_desc(ctypes.byref(a), 5, 1, None, 0, None) == -1
    assert b"capacity" in built_lib.paella_last_error()
    setattr(a, cap, need)
    assert built_lib.paella_test_gemm_desc(ctypes.byref(a), 1000, 1, None, 0, None) == -1
    assert b"bad tile config" in built_lib.paella_last_error()


def test_hook_capacity_bound_is_the_largest_index_of_the_store_references(built_lib):
    """The hook's bound and the index references are written independently: over a seeded sweep of store descriptions the smallest capacity the hook accepts is
    exactly 1 + the largest index the reference names."""
    import random
    rnd = random.Random(7)
    for _ in range(200):
        kind = rnd.choice(["plain", "remap", "d2s", "phase", "pixshuf"])
        sH, sW, B = rnd.randint(1, 5), rnd.randint(1, 6), rnd.randint(1, 4)
        f = dict(K=32)
        if kind in ("plain", "remap"):
            Mv, Nv = rnd.randint(1, 70), 4 * rnd.randint(1, 10)
            f.update(M=Mv, N=Nv, ldc=Nv + 4 * rnd.randint(0, 3))
            remap = (rnd.randint(1, 30), rnd.randint(0, 40), rnd.randint(0, 9)) if kind == "remap" else (0, 0, 0)
            f.update(remap_in=remap[0], remap_out=remap[1], remap_off=remap[2])
            idx = R.plain_index(Mv, Nv, f["ldc"], remap)
        elif kind == "pixshuf":
            sC = rnd.randint(1, 4)
            f.update(M=B * sH * sW, N=4 * sC, ldc=6, store_mode=R.STORE_PIXSHUF_NCHW, sH=sH, sW=sW, sC=sC)
            idx = R.pixshuf_index(f["M"], f["N"], sH, sW, sC)
        else:
            sC, nx = 4 * rnd.randint(1, 5), 2 if kind == "d2s" else 1
            nseg = 4 if kind == "d2s" else 1
            py, px = (0, 0) if kind == "d2s" else (rnd.randint(0, 1), rnd.randint(0, 1))
            f.update(M=B * sH * sW, N=nseg * sC, ldc=sC + 4 * rnd.randint(0, 2), store_mode=R.STORE_D2S, sH=sH, sW=sW, sC=sC, n_seg_x=nx, py=py, px=px)
            idx = R.d2s_index(f["M"], f["N"], f["ldc"], sH, sW, sC, nx, py, px)
        need = int(idx.max()) + 1
        a = _args(**f)
        a.c_capacity = need - 1
        assert built_lib.paella_test_gemm_desc(ctypes.byref(a), 5, 1, None, 0, None) == -1 and b"capacity" in built_lib.paella_last_error(), (kind, f)
        a.c_capacity = need
        assert built_lib.paella_test_gemm_desc(ctypes.byref(a), 1000, 1, None, 0, None) == -1 and b"bad tile config" in built_lib.paella_last_error(), (kind, f)


@pytest.mark.parametrize("fields,msg", [
    (dict(M=216, N=336, K=416, ldc=336, store_mode=1, sH=5, sW=6, sC=84), b"multiple of sH * sW"),
    (dict(M=216, N=336, K=416, ldc=336, store_mode=1, sH=4, sW=6, sC=80), b"bad depth-to-space"),
    (dict(M=216, N=336, K=416, ldc=336, store_mode=2, sH=4, sW=6, sC=3, c16=0x1000), b"belong to the plain store"),
    (dict(M=216, N=336, K=416, ldc=336, store_mode=3), b"unknown store mode"),
    (dict(M=216, N=336, K=416, ldc=336, C=None), b"null argument"),
    (dict(M=216, N=336, K=416, ldc=336, remap_in=24, remap_out=40, remap_off=-1), b"negative row remap"),
    (dict(M=216, N=336, K=416, ldc=336, c_capacity=1 << 30, mode=3), b"prologue mode"),
])
def test_hook_refuses_a_malformed_description_on_the_host(built_lib, fields, msg):
    a = _args(c_capacity=1 << 30, c16_capacity=1 << 30)
    for k, v in fields.items():
        setattr(a, k, v)
    assert built_lib.paella_test_gemm_desc(ctypes.byref(a), 5, 1, None, 0, None) == -1
    assert msg in built_lib.paella_last_error(), built_lib.paella_last_error()

"""GPU: every feature of the fp32 GEMM epilogue (common.h: Epilogue) and every store mode, on every tile config and on one-tile-per-workgroup / split-K /
stream-K launches, through the test hook paella_test_gemm_desc.

 * value families (ts, ts behind the GRN prologue, alpha, rowstat_out, sumsq_out): against fp64 torch math on the CPU;
 * placement families (row remap, ldc > N, bf16 copy, D2S, D2S phases, pixel-shuffle NCHW): bit for bit against the STORE_PLAIN launch of the same tile and split --
   itself compared with fp64 -- moved by the index references of tests/gemm_epilogue_refs.py (checked on the CPU by tests/test_gemm_epilogue_refs.py); every element the
   reference does not name keeps the bits it was pre-filled with;
 * the implicit-convolution prologue on the tiles that carry it, against F.conv2d / F.conv_transpose2d in fp64;
 * the specialised epilogue classes BGS / BRS / BRT / BRST of tiles 30 and 31: taken, and bit-identical to the run-time epilogue.

Shapes (the per-tile tests of tests/test_gpu_ops.py): M = 9 samples x 24 rows = 216 (no multiple of a tile height, the last 16-row group has 8 rows, samples
straddle tiles), N = 336 (a multiple of 16, of no tile width), K = 416 = 13 x 32.  Operands have asymmetric ramps and give outputs of unit scale.

Tolerances.  Values of C: the plain-GEMM bound of test_gemm_heuristic, atol = 2e-5 * max(1, sqrt(K) / 8), rtol = 1e-5, atol times the factor by which the feature
scales the value.  Statistics: the yardstick is the error of the same formula evaluated in fp32 on the CPU on the same stored values (rowstat: test_gpu_ops._ln_partials,
sumsq: fp32 pow(2).sum) against fp64, taken relative to the block's scale (sum |v| for the block sum; sum v^2 for M2 and for the sums of squares) and maximised over all
blocks; the kernel's maximum of the same relative error must stay within 4 x the yardstick's (the margin covers another summation order).  The maximum and not the
element: one fp32 evaluation can be exact on a block where another order is one rounding off.  The yardstick itself must lie within 32 roundings (32 * 2^-24) of
the fp64 reference, so that a wrong reference cannot widen its own bound.  Measured maxima are printed (pytest -s, lines starting with
"epi-parity") and kept in profiles/gemm_epilogue_features_parity.txt."""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from paella_amd import _lib
from tests import gemm_epilogue_refs as R
from tests.test_gpu_gemm_epilogue_specialisation import EPI_BIAS, EPI_GELU, EPI_RESID, EPI_RUNTIME, _both
from tests.test_gpu_ops import N_TILE_CONFIGS, _ln_partials

pytestmark = pytest.mark.gpu

EPI_TS, EPI_ROWSTAT, EPI_SUMSQ = 8, 16, 32
RPS, NB, N, K = 24, 9, 336, 416
M = RPS * NB
SPLITS = (1, 3, -7, -61)
ATOL = 2e-5 * max(1.0, K ** 0.5 / 8)
RTOL = 1e-5
FILL32, FILL16 = 0x7FC0BEEF, 0x7FC1  # pre-fill bit patterns (quiet NaNs as fp32 / bf16)
GUARD = 64                           # extra pre-filled elements behind every output
TS_OFF, TS_STRIDE = 12, 2 * N + 52   # the TimestepBlock table as the model passes it: a column block of a wider per-sample table
CONV_TILES = (2, 5, 9, 10, 14, 18, 19)  # gemm.hip: V_CONV
DMA_TILES = (0, 10, 18, 19)             # gemm.hip: V_DMA

# (family, tile) pairs launch_gemm_cfg refuses by its documented rules, with the message it gives.  Every other pair of this file is launched and checked: at these
# shapes the ring tiles' rules (K % 32 == 0, <= 8 samples per tile behind the GRN prologue) refuse nothing, so only the implicit convolution consults the table.
REFUSED = {("conv", c): b"has no implicit-convolution variant (2, 5, 9, 10, 14, 18, 19 do)" for c in range(N_TILE_CONFIGS) if c not in CONV_TILES}


def _tile_class(cfg):
    return "ring" if cfg >= 30 else ("lds-dma" if cfg in DMA_TILES else "register")


_REPORT = {}


def _record(family, quantity, cfg, splitk, value, bound):
    key = (family, quantity, _tile_class(cfg), splitk)
    old = _REPORT.get(key, (0.0, 0.0))
    _REPORT[key] = (max(old[0], float(value)), max(old[1], float(bound)))


@pytest.fixture(scope="module")
def lib(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    yield built_lib
    built_lib.paella_test_gemm_epi_specialise(1)
    built_lib.paella_test_gemm_dma(1)
    print()  # (the report starts on a line of its own, behind pytest's progress dots)
    for (family, quantity, cls, splitk), (v, b) in sorted(_REPORT.items()):
        print("epi-parity %-8s %-12s %-8s splitk %4d  max %.3e  bound %.3e" % (family, quantity, cls, splitk, v, b))


@pytest.fixture(scope="module")
def ws(lib):
    return _lib.new_workspace(64 << 20, "cuda")


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _addr(t):
    """tensor, (tensor, element offset) or None -> address"""
    if t is None:
        return None
    if isinstance(t, tuple):
        return t[0].data_ptr() + t[1] * t[0].element_size()
    return t.data_ptr()


def _room(t):
    return 0 if t is None else (t[0].numel() - t[1] if isinstance(t, tuple) else t.numel())


_POINTERS = ("A", "W", "C", "bias", "residual", "ts", "rowstat_out", "sumsq_out", "c16", "scale", "shift", "ln_stats")


def _launch(lib, ws, cfg, splitk, **kw):
    """One paella_test_gemm_desc launch; tensors (or (tensor, element offset)) for the pointer fields, the capacities taken from the tensors behind the outputs."""
    a = _lib.TestGemmArgs()
    a.alpha, a.n_seg_x = 1.0, 2
    a.c_capacity, a.c16_capacity, a.rowstat_capacity, a.sumsq_capacity = (_room(kw.get(k)) for k in ("C", "c16", "rowstat_out", "sumsq_out"))
    for k, v in kw.items():
        setattr(a, k, _addr(v) if k in _POINTERS else v)
    return lib.paella_test_gemm_desc(ctypes.byref(a), cfg, splitk, ctypes.c_void_p(ws.data_ptr()), ws.numel(), _st())


def _ok(lib, rc):
    assert rc == 0, lib.paella_last_error()


def _refused(lib, family, cfg, launch):
    """True (after asserting the refusal and its message) when (family, cfg) is in the table of refused pairs."""
    msg = REFUSED.get((family, cfg))
    if msg is None:
        return False
    assert launch() == -1, "tile %d was expected to refuse the %s launch" % (cfg, family)
    assert msg in lib.paella_last_error(), lib.paella_last_error()
    return True


def _filled(n, bf16=False):
    return torch.full((n + GUARD,), FILL16 if bf16 else FILL32, dtype=torch.int16 if bf16 else torch.int32, device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _assert_placed(buf, index, values, what):
    """buf (pre-filled int tensor the launch stored into) == its pre-fill with `values` scattered to `index`, bit for bit: placement AND untouched elements."""
    fill = FILL16 if buf.element_size() == 2 else FILL32
    want = R.scatter(torch.full((buf.numel(),), fill, dtype=buf.dtype), index, _bits(values))
    got = buf.cpu()
    if not torch.equal(got, want):
        bad = (got != want).nonzero().flatten()
        named = torch.zeros(buf.numel(), dtype=torch.bool)
        named[index.reshape(-1)] = True
        raise AssertionError("%s: %d elements differ (%d of them outside the reference's targets), first at flat index %d"
                             % (what, bad.numel(), int((~named[bad]).sum()), int(bad[0])))


def _assert_close(got, ref64, atol, what):
    np.testing.assert_allclose(got.double().numpy(), ref64.numpy(), atol=atol, rtol=RTOL, err_msg=what)


@pytest.fixture(scope="module")
def d(lib):
    """Operands, on both sides, and the fp64 contractions every case of the common shape shares."""
    g = torch.Generator().manual_seed(20)
    rn = lambda *s: torch.randn(*s, generator=g)
    o = types.SimpleNamespace()
    o.A = rn(M, K) + torch.arange(K)[None, :] * 0.001 - 0.1
    o.W = rn(N, K) / K ** 0.5 + torch.arange(N)[:, None] * 2e-5
    o.bias, o.res = 0.5 * rn(N), rn(M, N)
    o.scale, o.shift = 1.0 + 0.3 * rn(NB, K), 0.2 * rn(K)
    o.ts = 0.3 * rn(TS_OFF + NB * TS_STRIDE)
    tsv = o.ts[TS_OFF:].view(NB, TS_STRIDE)
    o.ts_a, o.ts_b = tsv[:, :N].double(), tsv[:, N:2 * N].double()
    o.W2 = rn(80, N) / N ** 0.5 + torch.arange(80)[:, None] * 1e-4  # the LayerNorm-consuming GEMM behind rowstat_out
    o.acc = o.A.double() @ o.W.double().t()
    o.acc_grn = (o.A.double() * o.scale.double().repeat_interleave(RPS, 0) + o.shift.double()) @ o.W.double().t()
    o.ref_plain = R.epilogue_value(o.acc, o.bias.double(), residual=o.res.double())
    # pixel-shuffle head: 3 channels, a 5 x 7 source grid
    o.pB, o.pH, o.pW = 3, 5, 7
    o.pM = o.pB * o.pH * o.pW
    o.pA = rn(o.pM, K) + torch.arange(K)[None, :] * 0.001
    o.pWt = rn(12, K) / K ** 0.5 + torch.arange(12)[:, None] * 1e-3
    o.pbias = 0.5 * rn(12)
    o.pref = o.pA.double() @ o.pWt.double().t() + o.pbias.double()
    o.gpu = types.SimpleNamespace(**{k: v.cuda() for k, v in vars(o).items() if torch.is_tensor(v) and v.dtype == torch.float32})
    return o


_PLAIN = {}


def _plain(lib, ws, d, cfg, splitk):
    """The STORE_PLAIN launch (bias + residual) of tile cfg and this split: compared with fp64 once, then the bit-exact standard of the placement families."""
    key = (cfg, splitk)
    if key not in _PLAIN:
        buf = _filled(M * N)
        _ok(lib, _launch(lib, ws, cfg, splitk, A=d.gpu.A, lda=K, W=d.gpu.W, ldw=K, C=buf, ldc=N, M=M, N=N, K=K, bias=d.gpu.bias, residual=d.gpu.res, ldr=N))
        got = buf.cpu()
        assert (got[M * N:] == FILL32).all(), "plain store wrote behind its last row"
        C = got[:M * N].view(torch.float32).view(M, N)
        _assert_close(C, d.ref_plain, ATOL, "plain launch, tile %d split %d" % (cfg, splitk))
        _PLAIN[key] = C
    return _PLAIN[key]


def _common(d, **kw):
    return dict(dict(A=d.gpu.A, lda=K, W=d.gpu.W, ldw=K, ldc=N, M=M, N=N, K=K, bias=d.gpu.bias, residual=d.gpu.res, ldr=N), **kw)


# ---------------------------------------------------------------------------------------------------------------------
# placement families
# ---------------------------------------------------------------------------------------------------------------------
def _place_remap(lib, ws, d, cfg, splitk, plain):
    # (remap_in, remap_out, remap_off): a plain offset form, and the conditioning-slot form remap_off = slot0 * S_slot (S = 24 rows into slots of 64, from slot 2)
    for remap in ((24, 40, 3), (RPS, 64, 2 * 64)):
        rows = int(R.remap_rows(M, *remap).max()) + 1
        buf = _filled(rows * N)
        _ok(lib, _launch(lib, ws, cfg, splitk, **_common(d, C=buf, remap_in=remap[0], remap_out=remap[1], remap_off=remap[2])))
        _assert_placed(buf, R.plain_index(M, N, N, remap), plain, "row remap %s" % (remap,))


def _place_ldc(lib, ws, d, cfg, splitk, plain):
    ldc, off = N + 24, 8  # a column block of a wider matrix, from a base inside the buffer
    buf = _filled(off + M * ldc)
    _ok(lib, _launch(lib, ws, cfg, splitk, **_common(d, C=(buf, off), ldc=ldc)))
    _assert_placed(buf, R.plain_index(M, N, ldc) + off, plain, "ldc > N")


def _place_c16(lib, ws, d, cfg, splitk, plain):
    want16 = plain.to(torch.bfloat16)  # round to nearest even
    for with_c in (True, False):
        buf, buf16 = _filled(M * N), _filled(M * N, bf16=True)
        _ok(lib, _launch(lib, ws, cfg, splitk, **_common(d, C=buf if with_c else None, c16=buf16)))
        _assert_placed(buf16, R.plain_index(M, N, N), want16, "bf16 copy (C %s)" % ("set" if with_c else "NULL"))
        if with_c:
            _assert_placed(buf, R.plain_index(M, N, N), plain, "fp32 output next to the bf16 copy")
        else:
            assert (buf.cpu() == FILL32).all()


def _place_d2s(lib, ws, d, cfg, splitk, plain):
    sH, sW, sC, ldc = 4, 6, N // 4, N // 4 + 12  # ConvTranspose2d(k2, s2): N = 4 segments (dy, dx) of 84 channels into rows of pitch 96
    buf = _filled(NB * 2 * sH * 2 * sW * ldc)
    _ok(lib, _launch(lib, ws, cfg, splitk, **_common(d, C=buf, ldc=ldc, store_mode=R.STORE_D2S, sH=sH, sW=sW, sC=sC, n_seg_x=2)))
    _assert_placed(buf, R.d2s_index(M, N, ldc, sH, sW, sC, 2), plain, "D2S, two segments per row")


def _place_phases(lib, ws, d, cfg, splitk, plain):
    sH, sW = 4, 6  # one phase of ConvTranspose2d(k4, s2, p1) per launch: the other three phases' positions stay untouched
    for py in (0, 1):
        for px in (0, 1):
            buf = _filled(NB * 2 * sH * 2 * sW * N)
            _ok(lib, _launch(lib, ws, cfg, splitk, **_common(d, C=buf, store_mode=R.STORE_D2S, sH=sH, sW=sW, sC=N, n_seg_x=1, py=py, px=px)))
            _assert_placed(buf, R.d2s_index(M, N, N, sH, sW, N, 1, py, px), plain, "D2S phase (%d, %d)" % (py, px))


def _place_pixshuf(lib, ws, d, cfg, splitk, plain_unused):
    base = dict(A=d.gpu.pA, lda=K, W=d.gpu.pWt, ldw=K, M=d.pM, N=12, K=K, bias=d.gpu.pbias)
    buf = _filled(d.pM * 12)
    _ok(lib, _launch(lib, ws, cfg, splitk, C=buf, ldc=12, **base))
    plain = buf.cpu()[:d.pM * 12].view(torch.float32).view(d.pM, 12)
    _assert_close(plain, d.pref, ATOL, "plain launch of the pixel-shuffle head, tile %d split %d" % (cfg, splitk))
    out = _filled(d.pB * 3 * 2 * d.pH * 2 * d.pW)
    _ok(lib, _launch(lib, ws, cfg, splitk, C=out, ldc=6, store_mode=R.STORE_PIXSHUF_NCHW, sH=d.pH, sW=d.pW, sC=3, **base))  # (ldc is not used by this store: no multiple of 4)
    _assert_placed(out, R.pixshuf_index(d.pM, 12, d.pH, d.pW, 3), plain, "pixel-shuffle NCHW")


PLACEMENT = {"remap": _place_remap, "ldc": _place_ldc, "c16": _place_c16, "d2s": _place_d2s, "d2s-phase": _place_phases, "pixshuf": _place_pixshuf}


@pytest.mark.parametrize("cfg", range(N_TILE_CONFIGS))
@pytest.mark.parametrize("family", sorted(PLACEMENT))
def test_store_placement_is_the_plain_launch_moved(lib, ws, d, family, cfg):
    for splitk in SPLITS:
        PLACEMENT[family](lib, ws, d, cfg, splitk, None if family == "pixshuf" else _plain(lib, ws, d, cfg, splitk))


# ---------------------------------------------------------------------------------------------------------------------
# value families
# ---------------------------------------------------------------------------------------------------------------------
def _stored(buf, rows=M, cols=N):
    got = buf.cpu()
    assert (got[rows * cols:] == FILL32).all(), "store behind the last row"
    assert (got[:rows * cols] != FILL32).all(), "elements of C left unwritten"
    return got[:rows * cols].view(torch.float32).view(rows, cols)


def _value_ts(lib, ws, d, cfg, splitk, grn=False):
    buf = _filled(M * N)
    pro = dict(mode=1, scale=d.gpu.scale, shift=d.gpu.shift, a_rows_per_sample=RPS) if grn else {}
    _ok(lib, _launch(lib, ws, cfg, splitk, **_common(d, C=buf, ts=(d.gpu.ts, TS_OFF), ts_stride=TS_STRIDE, rows_per_sample=RPS, **pro)))
    ref = R.epilogue_value(d.acc_grn if grn else d.acc, d.bias.double(), residual=d.res.double(), ts=(d.ts_a, d.ts_b), rps=RPS)
    C = _stored(buf)
    factor = float((1 + d.ts_a).abs().max())
    _record("ts-grn" if grn else "ts", "C abs", cfg, splitk, (C.double() - ref).abs().max(), ATOL * factor)
    _assert_close(C, ref, ATOL * factor, "ts")


def _value_alpha(lib, ws, d, cfg, splitk):
    buf = _filled(M * N)
    _ok(lib, _launch(lib, ws, cfg, splitk, **_common(d, C=buf, act=1, alpha=0.37)))
    ref = R.epilogue_value(d.acc, d.bias.double(), gelu=True, alpha=0.37, residual=d.res.double())
    C = _stored(buf)
    _record("alpha", "C abs", cfg, splitk, (C.double() - ref).abs().max(), ATOL * 0.37)
    _assert_close(C, ref, ATOL * 0.37, "alpha")


def _stat_check(family, quantity, cfg, splitk, got, yard, ref64, scale):
    """max over all blocks of |got - fp64| / scale within 4 x the same maximum of the fp32 CPU evaluation `yard`"""
    err = ((got.double() - ref64).abs() / scale).max().item()
    yard_err = ((yard.double() - ref64).abs() / scale).max().item()
    # the yardstick must itself sit where the number format puts it, or the bound below would follow a wrong reference: a 16-term fp32 sum in any order is within 15
    # roundings of sum |v|; the centred squares add <= 8 (two roundings per deviation, doubled by the square, and 16 mean^2 <= sum v^2) -- 32 roundings cover both
    assert yard_err <= 32 * 2.0 ** -24, "%s %s: the fp32 CPU evaluation is %.3e off the fp64 reference -- reference and yardstick disagree" % (family, quantity, yard_err)
    bound = 4 * yard_err
    print("epi-parity-case %s %s tile %d splitk %d: max rel err %.3e, bound (4 x fp32 CPU) %.3e" % (family, quantity, cfg, splitk, err, bound))
    _record(family, quantity, cfg, splitk, err, bound)
    assert bound > 0 and err <= bound, "%s %s, tile %d split %d: %.3e > %.3e" % (family, quantity, cfg, splitk, err, bound)


def _value_rowstat(lib, ws, d, cfg, splitk):
    buf, st = _filled(M * N), _filled(M * (N // 16) * 2)
    _ok(lib, _launch(lib, ws, cfg, splitk, **_common(d, C=buf, rowstat_out=st)))
    C = _stored(buf)
    _assert_close(C, d.ref_plain, ATOL, "C next to rowstat_out")
    S = _stored(st, M, (N // 16) * 2).view(M, N // 16, 2)
    # the contract: statistics OF THE STORED VALUES, all M x N / 16 of them
    ref, yard = R.rowstat_partials(C), _ln_partials(C.view(M, N // 16, 16))
    blk = C.double().view(M, N // 16, 16)
    _stat_check("rowstat", "block sum", cfg, splitk, S[..., 0], yard[..., 0], ref[..., 0], blk.abs().sum(-1))
    _stat_check("rowstat", "block M2", cfg, splitk, S[..., 1], yard[..., 1], ref[..., 1], blk.pow(2).sum(-1))
    # the consumer: LayerNorm of the stored rows folded into the next GEMM from these statistics (ring tiles need K % 32 == 0 and K = 336 here: the 32x32 tile)
    out = _filled(M * 80)
    _ok(lib, _launch(lib, ws, cfg if cfg < 30 else 5, splitk, A=(buf, 0), lda=N, W=d.gpu.W2, ldw=N, C=out, ldc=80, M=M, N=80, K=N, mode=2, ln_stats=(st, 0)))
    ref2 = F.layer_norm(C.double(), (N,), None, None, 1e-6) @ d.W2.double().t()
    got2 = _stored(out, M, 80)
    _record("rowstat", "consumer abs", cfg, splitk, (got2.double() - ref2).abs().max(), 2e-4)
    np.testing.assert_allclose(got2.double().numpy(), ref2.numpy(), atol=2e-4, rtol=2e-5)  # the bound of test_gemm_operand_prologues_every_tile_config, mode 2


def _value_sumsq(lib, ws, d, cfg, splitk):
    G = (M + 15) // 16
    buf, sq = _filled(M * N), _filled(G * N)
    _ok(lib, _launch(lib, ws, cfg, splitk, **_common(d, C=buf, residual=None, act=1, sumsq_out=sq)))
    C = _stored(buf)
    _assert_close(C, R.epilogue_value(d.acc, d.bias.double(), gelu=True), ATOL, "C next to sumsq_out")
    Q = _stored(sq, G, N)
    ref = R.sumsq_groups(C)  # the last group counts its 8 rows
    _stat_check("sumsq", "column sums", cfg, splitk, Q, R.sumsq_groups(C, torch.float32), ref, ref)


VALUE = {"ts": _value_ts, "ts-grn": lambda *a: _value_ts(*a, grn=True), "alpha": _value_alpha, "rowstat": _value_rowstat, "sumsq": _value_sumsq}


@pytest.mark.parametrize("cfg", range(N_TILE_CONFIGS))
@pytest.mark.parametrize("family", sorted(VALUE))
def test_epilogue_values_against_fp64(lib, ws, d, family, cfg):
    for splitk in SPLITS:
        VALUE[family](lib, ws, d, cfg, splitk)


# ---------------------------------------------------------------------------------------------------------------------
# implicit convolution (VQGAN, C = 32): both descriptors of vqmodel.hip on a 3 x 6 x 10 input, where zero-padded border taps are a large share of all taps
# ---------------------------------------------------------------------------------------------------------------------
CV_B, CV_H, CV_W, CV_C, CV_CO = 3, 6, 10, 32, 48


@pytest.fixture(scope="module")
def cv(lib):
    g = torch.Generator().manual_seed(21)
    rn = lambda *s: torch.randn(*s, generator=g)
    o = types.SimpleNamespace()
    o.x = rn(CV_B, CV_C, CV_H, CV_W) + torch.arange(CV_W)[None, None, None, :] * 0.05 + torch.arange(CV_C)[None, :, None, None] * 0.01  # NCHW, as torch takes it
    o.w_conv = rn(CV_CO, CV_C, 4, 4) / (16 * CV_C) ** 0.5
    o.w_convT = rn(CV_C, CV_CO, 4, 4) / (4 * CV_C) ** 0.5
    o.bias = 0.5 * rn(CV_CO)
    o.ref_conv = F.conv2d(o.x.double(), o.w_conv.double(), o.bias.double(), stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, CV_CO)          # [45, 48]
    o.ref_convT = F.conv_transpose2d(o.x.double(), o.w_convT.double(), o.bias.double(), stride=2, padding=1).permute(0, 2, 3, 1).contiguous()  # [3, 12, 20, 48]
    o.x_nhwc = o.x.permute(0, 2, 3, 1).contiguous().cuda()
    o.W = R.conv4s2_weight(o.w_conv).cuda()
    o.Wph = {(py, px): R.convT4_phase_weight(o.w_convT, py, px).cuda() for py in (0, 1) for px in (0, 1)}
    o.bias_gpu = o.bias.cuda()
    return o


def _conv_launch(lib, ws, cv, cfg, splitk, out):
    Mo, Kc = CV_B * (CV_H // 2) * (CV_W // 2), 16 * CV_C
    return _launch(lib, ws, cfg, splitk, A=cv.x_nhwc, lda=Kc, W=cv.W, ldw=Kc, C=out, ldc=CV_CO, M=Mo, N=CV_CO, K=Kc, bias=cv.bias_gpu, cv_enabled=1, cv_Hi=CV_H, cv_Wi=CV_W,
                   cv_C=CV_C, cv_Ho=CV_H // 2, cv_Wo=CV_W // 2, cv_stride=2, cv_ntaps=16, cv_tw_log2=2, cv_oy0=-1, cv_ox0=-1, cv_tsign=1)


def _convT_launch(lib, ws, cv, cfg, splitk, out, py, px):
    Mo, Kc = CV_B * CV_H * CV_W, 4 * CV_C
    return _launch(lib, ws, cfg, splitk, A=cv.x_nhwc, lda=Kc, W=cv.Wph[(py, px)], ldw=Kc, C=out, ldc=CV_CO, M=Mo, N=CV_CO, K=Kc, bias=cv.bias_gpu, cv_enabled=1, cv_Hi=CV_H,
                   cv_Wi=CV_W, cv_C=CV_C, cv_Ho=CV_H, cv_Wo=CV_W, cv_stride=1, cv_ntaps=4, cv_tw_log2=1, cv_oy0=py, cv_ox0=px, cv_tsign=-1,
                   store_mode=R.STORE_D2S, sH=CV_H, sW=CV_W, sC=CV_CO, n_seg_x=1, py=py, px=px)


@pytest.mark.parametrize("cfg", range(N_TILE_CONFIGS))
def test_implicit_convolution_against_torch_conv(lib, ws, cv, cfg):
    n_conv, n_convT = CV_B * (CV_H // 2) * (CV_W // 2) * CV_CO, CV_B * 2 * CV_H * 2 * CV_W * CV_CO
    if _refused(lib, "conv", cfg, lambda: _conv_launch(lib, ws, cv, cfg, 1, _filled(n_conv))):
        assert _refused(lib, "conv", cfg, lambda: _convT_launch(lib, ws, cv, cfg, 1, _filled(n_convT), 0, 0))
        return
    try:
        for dma in ((1, 0) if cfg in DMA_TILES else (1,)):
            _ok(lib, lib.paella_test_gemm_dma(dma))
            for splitk in SPLITS:
                out = _filled(n_conv)
                _ok(lib, _conv_launch(lib, ws, cv, cfg, splitk, out))
                got = _stored(out, n_conv // CV_CO, CV_CO)
                atol = 2e-5 * max(1.0, (16 * CV_C) ** 0.5 / 8)
                _record("conv", "k4 s2 abs", cfg, splitk, (got.double() - cv.ref_conv).abs().max(), atol)
                np.testing.assert_allclose(got.double().numpy(), cv.ref_conv.numpy(), atol=atol, rtol=RTOL)
                out = _filled(n_convT)  # the four phases into ONE buffer: together they write the full 12 x 20 output, each element once
                for py in (0, 1):
                    for px in (0, 1):
                        _ok(lib, _convT_launch(lib, ws, cv, cfg, splitk, out, py, px))
                got = _stored(out, n_convT // CV_CO, CV_CO)
                atol = 2e-5 * max(1.0, (4 * CV_C) ** 0.5 / 8)
                _record("conv", "convT abs", cfg, splitk, (got.double() - cv.ref_convT.view(-1, CV_CO)).abs().max(), atol)
                np.testing.assert_allclose(got.double().numpy(), cv.ref_convT.view(-1, CV_CO).numpy(), atol=atol, rtol=RTOL)
    finally:
        lib.paella_test_gemm_dma(1)


# ---------------------------------------------------------------------------------------------------------------------
# specialised epilogue classes of the 32x32 ring tiles (gemm.hip: RingEpi) that the op-level suite did not reach
# ---------------------------------------------------------------------------------------------------------------------
EPI_BGS = EPI_BIAS | EPI_GELU | EPI_SUMSQ
EPI_BR = EPI_BIAS | EPI_RESID
EPI_BRS, EPI_BRT, EPI_BRST = EPI_BR | EPI_ROWSTAT, EPI_BR | EPI_TS, EPI_BR | EPI_ROWSTAT | EPI_TS
# (class, GRN prologue, specialised instantiation exists): RingEpi<0> = {B, BGF, BGS, BR, BRS}, RingEpi<1> = {BR, BRS, BRT, BRST}
CLASSES = [(EPI_BGS, False, True), (EPI_BRS, False, True), (EPI_BRS, True, True), (EPI_BRT, True, True), (EPI_BRST, True, True),
           (EPI_BRT, False, False), (EPI_BRST, False, False)]


@pytest.mark.parametrize("cfg", [30, 31])
@pytest.mark.parametrize("cls,grn,specialised", CLASSES)
def test_ring_tile_classes_with_side_outputs_match_runtime_bit_for_bit(lib, ws, d, cfg, cls, grn, specialised):
    G = (M + 15) // 16

    def run():
        outs = []
        for splitk in (1, -61):
            buf, st, sq = _filled(M * N), _filled(M * (N // 16) * 2), _filled(G * N)
            kw = _common(d, C=buf)
            if cls & EPI_GELU:
                kw.update(act=1, residual=None)
            if cls & EPI_SUMSQ:
                kw.update(sumsq_out=sq)
            if cls & EPI_ROWSTAT:
                kw.update(rowstat_out=st)
            if cls & EPI_TS:
                kw.update(ts=(d.gpu.ts, TS_OFF), ts_stride=TS_STRIDE, rows_per_sample=RPS)
            if grn:
                kw.update(mode=1, scale=d.gpu.scale, shift=d.gpu.shift, a_rows_per_sample=RPS)
            _ok(lib, _launch(lib, ws, cfg, splitk, **kw))
            outs += [buf, st, sq]
        return outs

    (o_on, r_on), (o_off, r_off) = _both(lib, run)
    taken = cls if specialised else EPI_RUNTIME
    assert r_on == [(cfg, taken, cls)] * 2 and r_off == [(cfg, EPI_RUNTIME, cls)] * 2, (r_on, r_off)
    assert (o_on[0][:M * N] != FILL32).all()
    for a, b in zip(o_on, o_off):
        assert torch.equal(a, b)

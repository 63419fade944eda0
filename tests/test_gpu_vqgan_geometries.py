"""GPU: the VQGAN stack against fp64 beyond the shipped geometry (tests/vqgan_cases.py): 1 / 2 / 3 / 4 levels, widths 24 ... 1280, c_latent 4 ... 64,
codebooks of 37 ... 8193 codes, odd latent grids with B > 1; then the quantiser and the codebook gather on their own at every dispatch edge, and the
refusals that must happen before anything is enqueued.

Tolerance of every float tensor compared with fp64: with e_hip = max|HIP - fp64| and e_cpu = max|fp32 CPU oracle - fp64| on the same inputs,
    e_hip <= max(4 * e_cpu, 2^-21 * max|ref|).
4 is the margin the project uses for "no worse than the torch path" (a different accumulation order in the GEMMs); the floor, 4 ulp of the largest value,
keeps a lucky e_cpu from failing a correct kernel.  Both numbers are printed per case (profiles/vqgan_geometry_parity.txt is that output)."""
import ctypes

import pytest
import torch

from paella_amd import _lib
from paella_amd import vqgan as vqgan_module
from tests import vqgan_cases as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_ARG, ERR_WORKSPACE, ERR_STATE = -1, -3, -4
TAIL, PATTERN = 4096, 0xA5


def _parity(case, what, got, f64, f32):
    ref = f64.double()
    e_hip = float((got.double().cpu() - ref).abs().max())
    e_cpu = float((f32.double() - ref).abs().max())
    bound = max(4.0 * e_cpu, 2.0 ** -21 * float(ref.abs().max()))
    print("PARITY %-9s %-14s max|ref| %9.3e  e_cpu %9.3e  e_hip %9.3e  e_hip/e_cpu %6.2f  bound %9.3e"
          % (case, what, float(ref.abs().max()), e_cpu, e_hip, e_hip / e_cpu if e_cpu else float("inf"), bound))
    assert torch.isfinite(got).all(), "%s %s: non-finite output" % (case, what)
    return e_hip <= bound, "%s %s: e_hip %.3e > max(4 * e_cpu %.3e, floor) = %.3e" % (case, what, e_hip, e_cpu, bound)


class _NanTorch:
    """torch, as paella_amd/vqgan.py sees it, with empty / empty_like returning NaN-filled tensors (ints: the most negative value)."""

    def __getattr__(self, attr):
        return getattr(torch, attr)

    @staticmethod
    def _fill(t):
        return t.fill_(float("nan")) if t.is_floating_point() else t.fill_(torch.iinfo(t.dtype).min)

    def empty(self, *a, **k):
        return self._fill(torch.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._fill(torch.empty_like(*a, **k))


def _nan_filled_outputs(monkeypatch):
    """The wrapper allocates its outputs with torch.empty / empty_like; inside paella_amd.vqgan they now come back pre-filled with NaN, so a kernel that leaves
    part of an output unwritten cannot pass by luck."""
    monkeypatch.setattr(vqgan_module, "torch", _NanTorch())


def _exact_workspace(v, B, h, w):
    """workspace_bytes + TAIL bytes, all PATTERN, header initialised on the first workspace_bytes only: (the exact-size view, the tail view)."""
    n = v.workspace_bytes(B, h, w)
    buf = torch.full((n + TAIL,), PATTERN, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().paella_workspace_init(_lib.ptr(buf), n, _lib.stream_ptr(buf.device)))
    return buf[:n], buf[n:]


def _run_all(v, r, ws=None):
    img, tok = r["img"].to(DEV), r["tokens"].to(DEV)
    qe, lat, idx, loss = v.encode(img, ws=ws)
    return dict(qe=qe, lat=lat, idx=idx, loss=loss.reshape(1), dec_idx=v.decode_indices(tok, ws=ws))


@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_geometry_vs_fp64(built_lib, monkeypatch, name):
    r = V.reference(name)
    cfg, B, h, w = r["cfg"], r["B"], r["h"], r["w"]
    f64, f32 = r["f64"], r["f32"]
    assert int((r["margin"] < V.NEAR_TIE_EPS).sum()) == 0  # (tests/test_vqgan_cases.py): exact token equality is a fair demand
    v, _ = V.new_model(name)
    v = v.to(DEV)
    _nan_filled_outputs(monkeypatch)
    got = _run_all(v, r)
    got["dec"] = v.decode(r["lat_in"].to(DEV))
    torch.cuda.synchronize()
    checks = [_parity(name, k, got[k], f64[k], f32[k]) for k in ("lat", "qe", "dec_idx", "dec")]
    # tokens: exactly the fp64 reference's
    mism = int((got["idx"].cpu() != f64["idx"]).sum())
    print("PARITY %-9s tokens         %d of %d differ from fp64 (min nearest-code margin %.3e)" % (name, mism, f64["idx"].numel(), float(r["margin"].min())))
    assert mism == 0
    # qe = codebook[idx] / scale_factor, to the one rounding of the division (relative half an ulp: 2^-24), on the fp32 scale factor the ABI carries
    cb = r["sd"]["vquantizer.codebook.weight"].double()
    sf = V.ref_cfg(cfg)["scale_factor"]
    exact = (cb[got["idx"].cpu()] / sf).permute(0, 3, 1, 2)
    assert bool(((got["qe"].double().cpu() - exact).abs() <= 2.0 ** -24 * exact.abs()).all()), "qe is not the correctly rounded codebook[idx] / scale_factor"
    # loss = 1.25 * mse.  The kernel accumulates in fp64 and rounds three times (the mean, the quarter, the sum), so it is within rtol 5e-7 of the same
    # expression in fp64 ON WHAT IT WAS GIVEN: the codes codebook[idx] (exact) and the library's own latents (lat * sf: exact for a power-of-two scale
    # factor, otherwise to the one rounding of the division).  Against the fp64 PIPELINE the loss also carries the error of the fp32 latents, which is not the
    # loss kernel's and does not average out over the 80 values of the smallest case (measured 5.3e-7 on L2_c640, where the latents are within 0.9 x the CPU
    # oracle's error): to first order |d loss| / loss <= 2 * max|d x| / rms(q - x), and the loss is held to that with the latents' own tolerance as max|d x|.
    hip_loss, loss64 = float(got["loss"]), float(f64["loss"])
    own = 1.25 * float((cb[got["idx"].cpu()].permute(0, 3, 1, 2) - got["lat"].double().cpu() * sf).pow(2).mean())
    rel_own, rel_pipe = abs(hip_loss - own) / own, abs(hip_loss - loss64) / loss64
    tol_lat = max(4.0 * float((f32["lat"].double() - f64["lat"]).abs().max()), 2.0 ** -21 * float(f64["lat"].abs().max()))
    pipe_bound = 5e-7 + 2.0 * tol_lat * sf / (loss64 / 1.25) ** 0.5
    print("PARITY %-9s loss           hip %.9e  fp64 of its own latents %.9e rel %.2e (bound 5e-7)  fp64 pipeline %.9e rel %.2e (fp32 oracle %.2e, bound %.2e)"
          % (name, hip_loss, own, rel_own, loss64, rel_pipe, abs(float(f32["loss"]) - loss64) / loss64, pipe_bound))
    assert rel_own <= 5e-7, "loss %.9e vs fp64 1.25 * mse %.9e: rel %.2e > 5e-7" % (hip_loss, own, rel_own)
    assert rel_pipe <= pipe_bound, "loss %.9e vs the fp64 pipeline's %.9e: rel %.2e > %.2e" % (hip_loss, loss64, rel_pipe, pipe_bound)
    for ok, msg in checks:
        assert ok, msg
    # decode(codebook[tokens] / sf) and decode_indices(tokens) differ only by the rounding of / sf * sf at the decoder's input: held to the same rule against
    # the difference of the fp32 oracle's two decodes, and where the round trip is exact (a power-of-two scale factor) to bit equality
    d_hip = float((got["dec"] - got["dec_idx"]).abs().max())
    d_cpu = float((f32["dec"] - f32["dec_idx"]).abs().max())
    floor = 2.0 ** -21 * float(f64["dec_idx"].abs().max())
    print("PARITY %-9s dec-dec_idx    hip %.3e  fp32 oracle %.3e  floor %.3e" % (name, d_hip, d_cpu, floor))
    assert d_hip <= max(4.0 * d_cpu, floor)
    if sf in (0.5, 1.0):
        assert torch.equal(got["dec"], got["dec_idx"])

    # exactly paella_vqgan_workspace_bytes: same bits as with the module's own (grown, reused) scratch, and not one byte past the end is written
    ws, tail = _exact_workspace(v, B, h, w)
    again = _run_all(v, r, ws=ws)
    torch.cuda.synchronize()
    for k, t in again.items():
        assert torch.equal(t.view(torch.int32) if t.is_floating_point() else t, got[k].view(torch.int32) if t.is_floating_point() else got[k]), \
            "%s: %s differs with a workspace of exactly workspace_bytes" % (name, k)
    assert bool((tail == PATTERN).all()), "%s: %d byte(s) past workspace_bytes were written" % (name, int((tail != PATTERN).sum()))


def test_bf16_mode_is_fp32_where_no_width_is_a_multiple_of_64(built_lib, monkeypatch):
    """L2_c48: widths 24 / 48, so every ResBlock must take the fp32 branch in the bf16 mode too -- outputs bit-identical, workspace sized after the switch."""
    name = "L2_c48"
    r = V.reference(name)
    v, _ = V.new_model(name)
    v = v.to(DEV)
    _nan_filled_outputs(monkeypatch)
    base = _run_all(v, r)
    try:
        v.set_gemm_precision("bf16")
        assert v.get_gemm_precision() == "bf16"
        fast = _run_all(v, r)
        ws, tail = _exact_workspace(v, r["B"], r["h"], r["w"])
        fast_ws = _run_all(v, r, ws=ws)
        torch.cuda.synchronize()
        for k in base:
            for other in (fast, fast_ws):
                a, b = base[k], other[k]
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.is_floating_point() else torch.equal(a, b), "bf16 mode changed %s" % k
        assert bool((tail == PATTERN).all())
    finally:
        v.set_gemm_precision("fp32")
    back = _run_all(v, r)
    assert all(torch.equal(base[k], back[k]) for k in base)


# ---------------------------------------------------------------------------------------------------------------------
# the quantiser and the gather on their own
# ---------------------------------------------------------------------------------------------------------------------
def _quant(D, K, codebook=None):
    v, cb = V.new_quant_model(D, K)
    if codebook is not None:
        with torch.no_grad():
            v.vquantizer.codebook.weight.copy_(codebook)
        cb = codebook
    return v.to(DEV), cb


def _forward(v, x):
    zq, _, idx = v.vquantizer.forward(x, get_losses=False)
    return zq, idx


@pytest.mark.parametrize("D,K,rows", V.QUANT_SHAPES)
def test_quantiser_vs_fp64_brute_force(built_lib, monkeypatch, D, K, rows):
    q = V.quant_reference(D, K, rows)
    v, cb = _quant(D, K)
    _nan_filled_outputs(monkeypatch)
    x = q["x"].to(DEV)
    zq, idx = _forward(v, x)
    near = q["margin"] < V.NEAR_TIE_EPS
    mism = idx.cpu() != q["idx"]
    print("quantiser D=%d K=%d rows=%d vs fp64 brute force: %d indices differ, %d near-tie rows, all mismatches at near-ties: %s"
          % (D, K, rows, int(mism.sum()), int(near.sum()), not bool((mism & ~near).any())))
    assert int(near.sum()) <= V.QUANT_NEAR_TIE_CAP * rows
    assert int(idx.min()) >= 0 and int(idx.max()) < K
    assert not (mism & ~near).any(), "%d index(es) differ where the nearest code was unambiguous" % int((mism & ~near).sum())
    assert torch.equal(zq.cpu().view(torch.int32), cb[idx.cpu()].view(torch.int32)), "qe is not codebook[idx] bit for bit"
    if D == 4 and rows >= 4096:
        # one call (codebook in LDS when K <= 8192) against calls on chunks of 1000 rows (one wave per row): bit for bit
        parts = [_forward(v, x[i:i + 1000]) for i in range(0, rows, 1000)]
        assert torch.equal(idx, torch.cat([p[1] for p in parts])), "indices differ between one call and 1000-row chunks"
        assert torch.equal(zq.view(torch.int32), torch.cat([p[0] for p in parts]).view(torch.int32))
        # either side of the rows >= 4096 switch, on the same data
        z5, i5 = _forward(v, x[:4095])
        z6, i6 = _forward(v, x[:4096])
        assert torch.equal(i5, i6[:4095]) and torch.equal(i5, idx[:4095]) and torch.equal(z5.view(torch.int32), z6[:4095].view(torch.int32))


@pytest.mark.parametrize("D,K,rows", [(4, 8192, 4160), (4, 8192, 130), (4, 100, 4096), (4, 37, 4099), (4, 37, 9),(16, 257, 70), (64, 37, 9)])
def test_quantiser_ties_hits_and_non_finite_rows(built_lib, monkeypatch, D, K, rows):
    """Exact ties go to the lowest index (a duplicated code on the same lane, the next lane and -- K permitting -- the same lane's next turn), an exact hit of
    the last code is returned, and a row holding NaN or inf gets some valid index, that code as qe, and leaves its neighbours alone; in both kernels."""
    _, cb = V.new_quant_model(D, K)
    cb = cb.clone()
    k = 5
    dups = [k + 1, k + 64] if k + 64 < K else [k + 1, K - 2]
    for d in dups:
        cb[d] = cb[k]
    v, cb = _quant(D, K, cb)
    g = torch.Generator().manual_seed(7 * D + K)
    x = torch.randn(rows, D, generator=g) * 1.2 * cb.std()
    assert rows >= 9
    tie_rows, hit_row, nan_rows, inf_row = [0, rows // 2, rows - 1], 1, [3] + ([rows - 2] if rows > 20 else []), 5  # rows 2 and 6 stay ordinary neighbours
    for t in tie_rows:
        x[t] = cb[k]
    x[hit_row] = cb[K - 1]
    clean = x.clone()
    for t in nan_rows:
        x[t, D // 2] = float("nan")
    x[inf_row, 0] = float("inf")
    x[inf_row, D - 1] = float("-inf")
    _nan_filled_outputs(monkeypatch)
    zq, idx = _forward(v, x.to(DEV))
    zq_c, idx_c = _forward(v, clean.to(DEV))
    idx, zq = idx.cpu(), zq.cpu()
    ref, margin = V.brute_force(clean, cb)
    assert float(margin[hit_row]) > V.NEAR_TIE_EPS
    assert [int(idx[t]) for t in tie_rows] == [k] * 3, "an exact tie between codes %s did not go to the lowest index: %s" % ([k] + dups, [int(idx[t]) for t in tie_rows])
    assert int(idx[hit_row]) == K - 1
    assert all(0 <= int(idx[t]) < K for t in nan_rows + [inf_row])
    assert torch.equal(zq.view(torch.int32), cb[idx].view(torch.int32))
    keep = torch.ones(rows, dtype=torch.bool)
    keep[nan_rows + [inf_row]] = False
    assert torch.equal(idx[keep], idx_c.cpu()[keep]) and torch.equal(zq[keep].view(torch.int32), zq_c.cpu()[keep].view(torch.int32))
    ok = (idx == ref) | (margin < V.NEAR_TIE_EPS)
    assert bool(ok[keep].all())


def test_out_of_range_indices_are_clamped(built_lib, monkeypatch):
    """include/paella_hip.h, paella_vqgan_lookup_rows: an index outside [0, K) reads the nearest valid row, in idx2vq and in decode_indices."""
    name = "L1"
    r = V.reference(name)
    K = r["cfg"]["codebook_size"]
    v, sd = V.new_model(name)
    v = v.to(DEV)
    _nan_filled_outputs(monkeypatch)
    cb = sd["vquantizer.codebook.weight"]
    bad = torch.tensor([-5, K + 3, 0, K - 1, 17, -(2 ** 40), 2 ** 40], dtype=torch.int64)
    rows = v.vquantizer.idx2vq(bad.to(DEV)).cpu()
    assert torch.equal(rows.view(torch.int32), cb[bad.clamp(0, K - 1)].view(torch.int32))
    tok = r["tokens"].clone()
    tok.view(-1)[1], tok.view(-1)[-2], tok[1, 2, 3] = -5, K + 3, 2 ** 33
    out = v.decode_indices(tok.to(DEV))
    assert torch.equal(out.view(torch.int32), v.decode_indices(tok.clamp(0, K - 1).to(DEV)).view(torch.int32))


@pytest.mark.parametrize("D,K,rows", [(8, 1000, 333), (4, 8192, 4097), (64, 37, 67)])
def test_quantiser_mse_vs_fp64(built_lib, monkeypatch, D, K, rows):
    """paella_vqgan_quantize_rows with mse_out: mean((qe - x)^2), accumulated in fp64 by the kernel and rounded twice; rows * D is no multiple of 256."""
    assert (rows * D) % 256
    q = V.quant_reference(D, K, rows)
    v, cb = _quant(D, K)
    _nan_filled_outputs(monkeypatch)
    zq, (vq_loss, commit), idx = v.vquantizer.forward(q["x"].to(DEV), get_losses=True)
    ref = float((cb[idx.cpu()].double() - q["x"].double()).pow(2).mean())
    rel = abs(float(vq_loss) - ref) / ref
    print("quantiser mse D=%d K=%d rows=%d: hip %.9e fp64 %.9e rel %.2e" % (D, K, rows, float(vq_loss), ref, rel))
    assert rel <= 5e-7 and float(commit) == float(vq_loss)
    assert torch.equal(idx, _forward(v, q["x"].to(DEV))[1])


# ---------------------------------------------------------------------------------------------------------------------
# refusals: host-side returns, before anything is enqueued -- outputs pre-filled with NaN stay NaN
# ---------------------------------------------------------------------------------------------------------------------
def _refused(lib, rc, expected, outputs=()):
    torch.cuda.synchronize()
    assert rc == expected, "returned %d, expected %d (%s)" % (rc, expected, lib.paella_last_error())
    assert lib.paella_last_error(), "paella_last_error() is empty after a refusal"
    for t in outputs:
        assert bool(torch.isnan(t).all()) if t.is_floating_point() else bool((t == torch.iinfo(t.dtype).min).all()), "a refused call wrote to an output"


def test_refusals_happen_before_anything_is_enqueued(built_lib):
    lib = built_lib
    name = "L2_c48"
    r = V.reference(name)
    cfg, B, h, w = r["cfg"], r["B"], r["h"], r["w"]
    v, _ = V.new_model(name)
    v = v.to(DEV)
    hnd = v._engine()
    st = _lib.stream_ptr(torch.device(DEV))
    f, cl = 2 ** cfg["levels"], cfg["c_latent"]
    n = v.workspace_bytes(B, h, w)
    ws = _lib.new_workspace(n, torch.device(DEV))
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    qe, lat, loss, img_out = nan(B, cl, h, w), nan(B, cl, h, w), nan(1), nan(B, 3, h * f, w * f)
    idx = torch.full((B, h, w), torch.iinfo(torch.int64).min, dtype=torch.int64, device=DEV)
    img = r["img"].to(DEV)
    # an image height that is no multiple of 2^levels (the buffer is the full image: nothing is read past it either way)
    rc = lib.paella_vqgan_encode(hnd, _lib.ptr(img), B, h * f - 1, w * f, _lib.ptr(qe), _lib.ptr(lat), _lib.ptr(idx), _lib.ptr(loss), _lib.ptr(ws), n, st)
    _refused(lib, rc, ERR_ARG, (qe, lat, idx, loss))
    # a workspace one byte short of workspace_bytes
    rc = lib.paella_vqgan_encode(hnd, _lib.ptr(img), B, h * f, w * f, _lib.ptr(qe), _lib.ptr(lat), _lib.ptr(idx), _lib.ptr(loss), _lib.ptr(ws), n - 1, st)
    _refused(lib, rc, ERR_WORKSPACE, (qe, lat, idx, loss))
    tok = r["tokens"].to(DEV)
    rc = lib.paella_vqgan_decode_indices(hnd, _lib.ptr(tok), B, h, w, _lib.ptr(img_out), _lib.ptr(ws), n - 1, st)
    _refused(lib, rc, ERR_WORKSPACE, (img_out,))
    rc = lib.paella_vqgan_decode(hnd, _lib.ptr(r["lat_in"].to(DEV)), B, h, w, _lib.ptr(img_out), _lib.ptr(ws), n - 1, st)
    _refused(lib, rc, ERR_WORKSPACE, (img_out,))
    # quantize_rows with mse_out but no qe_out
    x = torch.randn(10, cl, device=DEV)
    qidx = torch.full((10,), torch.iinfo(torch.int64).min, dtype=torch.int64, device=DEV)
    rc = lib.paella_vqgan_quantize_rows(hnd, _lib.ptr(x), 10, _lib.ptr(qidx), None, _lib.ptr(loss), st)
    _refused(lib, rc, ERR_ARG, (qidx, loss))
    # the same calls, allowed: the handle and the buffers were fine all along
    _lib.check(lib.paella_vqgan_encode(hnd, _lib.ptr(img), B, h * f, w * f, _lib.ptr(qe), _lib.ptr(lat), _lib.ptr(idx), _lib.ptr(loss), _lib.ptr(ws), n, st))
    torch.cuda.synchronize()
    assert torch.equal(idx.cpu(), r["f64"]["idx"]) and bool(torch.isfinite(lat).all())

    # decode on a created but unfinalized handle
    c = _lib.VqganConfig()
    for key in ("levels", "bottleneck_blocks", "c_hidden", "c_latent", "codebook_size"):
        setattr(c, key, int(cfg[key]))
    c.scale_factor = float(cfg["scale_factor"])
    raw = ctypes.c_void_p()
    _lib.check(lib.paella_vqgan_create(ctypes.byref(c), ctypes.byref(raw)))
    try:
        rc = lib.paella_vqgan_decode(raw, _lib.ptr(r["lat_in"].to(DEV)), B, h, w, _lib.ptr(img_out), _lib.ptr(ws), n, st)
        _refused(lib, rc, ERR_STATE, (img_out,))
    finally:
        lib.paella_vqgan_destroy(raw)


@pytest.mark.parametrize("change", [dict(c_latent=68), dict(c_latent=6), dict(levels=7), dict(levels=3, c_hidden=40)])
def test_create_refuses_unsupported_configurations(built_lib, change):
    lib = built_lib
    cfg = dict(levels=2, bottleneck_blocks=1, c_hidden=64, c_latent=4, codebook_size=64, scale_factor=1.0)
    cfg.update(change)
    c = _lib.VqganConfig()
    for key in ("levels", "bottleneck_blocks", "c_hidden", "c_latent", "codebook_size"):
        setattr(c, key, int(cfg[key]))
    c.scale_factor = float(cfg["scale_factor"])
    raw = ctypes.c_void_p()
    rc = lib.paella_vqgan_create(ctypes.byref(c), ctypes.byref(raw))
    assert rc == ERR_ARG and not raw.value, "create(%s) returned %d" % (change, rc)
    assert lib.paella_last_error()

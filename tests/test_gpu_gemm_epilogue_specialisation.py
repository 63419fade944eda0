"""GPU: the compile-time-specialised epilogue classes of the GEMM (gemm_device.h: EPI_*) compute exactly what the run-time epilogue computes.
Every case runs twice in one process -- specialisation on (the product) and off (paella_test_gemm_epi_specialise(0): every launch takes EPI_RUNTIME) --
and compares bit for bit.  The per-launch records of the GEMM timing hook (paella_prof_epi) show which instantiation every launch took."""
import ctypes

import pytest
import torch

from paella_amd import _lib

pytestmark = pytest.mark.gpu

EPI_RUNTIME = 1 << 30
EPI_BIAS, EPI_GELU, EPI_RESID = 1, 2, 4


@pytest.fixture(scope="module")
def lib(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    yield built_lib
    built_lib.paella_test_gemm_epi_specialise(1)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(lib, rc):
    assert rc == 0, lib.paella_last_error()


def _recorded(lib, run):
    """run() with the GEMM timing hook on; returns [(tile config, class taken, class of the arguments)] of its launches."""
    torch.cuda.synchronize()
    _check(lib, lib.paella_prof_enable(1))
    try:
        run()
        torch.cuda.synchronize()
        cap = 1 << 16
        buf = (ctypes.c_int * (3 * cap))()
        n = lib.paella_prof_epi(buf, cap)
        assert n >= 0
        return [tuple(buf[3 * i: 3 * i + 3]) for i in range(min(n, cap))]
    finally:
        lib.paella_prof_enable(0)


def _both(lib, run):
    """(outputs, records) with specialisation on, then off."""
    out = {}
    for on in (1, 0):
        _check(lib, lib.paella_test_gemm_epi_specialise(on))
        try:
            recs = _recorded(lib, lambda: out.__setitem__(on, run()))
        finally:
            lib.paella_test_gemm_epi_specialise(1)
        out[on] = (out[on], recs)
    return out[1], out[0]


# skinny (batch-1) shapes with stream-K ranges that split tiles across workgroups, and a throughput shape with one tile per workgroup
SHAPES = [(32, 1280, 1280, -160), (32, 640, 2560, -77), (1024, 512, 256, 1)]


@pytest.mark.parametrize("cfg", [30, 31])
@pytest.mark.parametrize("M,N,K,splitk", SHAPES)
@pytest.mark.parametrize("resid", [False, True])
def test_ring_tile_classes_match_runtime_bit_for_bit(lib, cfg, M, N, K, splitk, resid):
    g = torch.Generator().manual_seed(cfg * 7 + M + N + K + resid)
    A = torch.randn(M, K, generator=g).cuda()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()
    b = torch.randn(N, generator=g).cuda()
    R = torch.randn(M, N, generator=g).cuda() if resid else None
    ws = _lib.new_workspace(64 << 20, "cuda")

    def run():
        C = torch.full((M, N), float("nan"), device="cuda")
        _check(lib, lib.paella_op_gemm(_p(A), _p(W), _p(b), _p(R), _p(C), M, N, K, 0, cfg, splitk, _p(ws), ws.numel(), _st()))
        return C

    (c_on, r_on), (c_off, r_off) = _both(lib, run)
    cls = EPI_BIAS | (EPI_RESID if resid else 0)
    assert r_on == [(cfg, cls, cls)] and r_off == [(cfg, EPI_RUNTIME, cls)], (r_on, r_off)
    assert not torch.isnan(c_on).any()
    assert torch.equal(c_on, c_off)


@pytest.mark.parametrize("B,rps,c", [(2, 64, 1280), (2, 16, 1280), (1, 64, 64)])
def test_mlp_pair_with_grn_finished_inside_the_gemms_matches_runtime(lib, B, rps, c):
    """MLP GEMM 1 (bias + GELU + GRN Gx in the epilogue) and GEMM 2 (GRN from the raw statistics, bias + residual) of the batch-1 path."""
    M = B * rps
    g = torch.Generator().manual_seed(B * 100 + rps + c)
    d = lambda *s, scale=1.0: (scale * torch.randn(*s, generator=g)).cuda()
    h, W1, b1 = d(M, c), d(4 * c, c, scale=c ** -0.5), d(4 * c, scale=0.1)
    gamma, beta, W2 = d(4 * c, scale=0.5), d(4 * c, scale=0.3), d(c, 4 * c, scale=(4 * c) ** -0.5)
    ws = _lib.new_workspace(64 << 20, "cuda")

    def run():
        hidden = torch.full((M, 4 * c), float("nan"), device="cuda")
        gx = torch.full((B, 4 * c), float("nan"), device="cuda")
        part = torch.full((B, 4 * c // 16), float("nan"), device="cuda")
        out = torch.full((M, c), float("nan"), device="cuda")
        _check(lib, lib.paella_test_mlp_grn_fused(_p(h), _p(W1), _p(b1), _p(gamma), _p(beta), _p(W2), _p(hidden), _p(gx), _p(part), _p(out), M, c, rps,
                                                  _p(ws), ws.numel(), _st()))
        return hidden, gx, part, out

    (o_on, r_on), (o_off, r_off) = _both(lib, run)
    assert all(t == EPI_RUNTIME for _, t, _ in r_off), r_off
    for a, b in zip(o_on, o_off):
        assert torch.equal(a, b)


def test_unet_forward_and_sampled_tokens_match_runtime(lib):
    """The whole network at batch 1 (every class the model launches, the fused head's tokens included): specialised == run-time bit for bit."""
    import paella_amd
    from oracle import golden_configs as G
    from oracle import paella_oracle as O
    from paella_amd import synth

    dev = "cuda:0"
    cfg = G.UNET_TINY
    c = synth.synth_conditioning(1, 4, cfg["byt5_embd"], cfg["clip_embd"], seed=2)
    u = synth.synth_conditioning(1, 4, cfg["byt5_embd"], cfg["clip_embd"], seed=7)
    mv = lambda dd: {k: (v.to(dev) if v is not None else None) for k, v in dd.items()}
    x = torch.randint(0, cfg["num_labels"], (1, 16, 16), generator=torch.Generator().manual_seed(1))
    r = torch.tensor([0.5])
    noise = O.replay_torch_noise(42, (1, 16, 16), cfg["num_labels"], 4, 3)

    def run():
        m = paella_amd.Paella(**cfg)
        synth.randomize_(m, seed=0)
        m = m.to(dev)
        logits = m(x.to(dev), r.to(dev), **mv(c)).float().clone()
        toks = paella_amd.sample(m, mv(c), (1, 16, 16), unconditional_inputs=mv(u), steps=4, renoise_steps=3, device=dev, noise=noise).clone()
        torch.cuda.synchronize()
        return logits, toks

    ((l_on, t_on), r_on), ((l_off, t_off), r_off) = _both(lib, run)
    assert all(t == EPI_RUNTIME for _, t, _ in r_off), r_off
    assert torch.equal(l_on, l_off)
    assert torch.equal(t_on, t_off)

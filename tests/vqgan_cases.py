"""Case table and fp64 reference for the VQGAN geometry tests (test infrastructure; a plain module, not a conftest).

`paella_vqgan_create` accepts levels 1 to 6, any c_hidden that is a multiple of 8 << (levels - 1), c_latent 4 to 64 and any codebook size; the goldens
cover one family (2 / 3 levels, widths 16 ... 384, c_latent 4, codebooks that are multiples of 64).  The cases below walk the rest, each as small as the
path it is there for allows:

  L1        no strided / transposed convolution at all; a codebook that is no multiple of 64; B > 1
  L2_c48    widths 24 / 48 (6 and 12 float4 lanes of 64, GEMM K = 24, the materialised im2col / transposed-conv gathers at such C, no width a multiple
            of 64); c_latent 8; an odd 3 x 5 grid with B = 3 (sample boundaries are most of the image)
  L3        c_latent 16, codebook 257 = 4 * 64 + 1, a 3 x 2 grid with B = 2
  L4        four levels, c_latent 64 (every lane of the quantiser's `lane < D` store), a codebook of 37 < 64 (lanes that own no code), a 1 x 3 grid
  L2_c640   width 640: LayerNorm / depthwise with NV = 3 float4 per lane (and 320: NV = 2), the shipped 8192 x 4 codebook
  L1_c1280  width 1280: NV = 5

The reference is the project's own oracle (oracle/paella_oracle.py: vq_encode, vq_decode, vq_decode_indices, vector_quantize), which is dtype-generic,
evaluated on the state dict cast to torch.float64; the same functions on the fp32 state dict give the error a plain fp32 implementation makes on the same
inputs, which is what the HIP stack is measured against.  Everything is computed once per process and shared.
"""
import functools

import numpy as np
import torch

import paella_amd
from oracle import paella_oracle as O
from tests.helpers import weights_for

NEAR_TIE_EPS = 1e-5  # squared-distance margin between the two nearest codes below which a token is a near-tie (the suite's definition, tests/test_gpu_vqgan.py)


def _case(levels, bottleneck_blocks, c_hidden, c_latent, codebook_size, scale_factor, B, h, w, seed):
    return dict(cfg=dict(levels=levels, bottleneck_blocks=bottleneck_blocks, c_hidden=c_hidden, c_latent=c_latent, codebook_size=codebook_size,
                         scale_factor=scale_factor), B=B, h=h, w=w, seed=seed)


CASES = {
    "L1": _case(1, 1, 64, 4, 100, 0.3764, 2, 6, 10, 101),
    "L2_c48": _case(2, 2, 48, 8, 1000, 0.5, 3, 3, 5, 102),
    "L3": _case(3, 1, 128, 16, 257, 0.3764, 2, 3, 2, 103),
    "L4": _case(4, 1, 256, 64, 37, 1.0, 1, 1, 3, 104),
    "L2_c640": _case(2, 1, 640, 4, 8192, 0.3764, 1, 5, 4, 105),
    "L1_c1280": _case(1, 1, 1280, 4, 64, 0.3764, 1, 2, 3, 106),
}
CASE_NAMES = list(CASES)


def new_model(name):
    """A fresh paella_amd.VQModel of the case with the suite's seeded synthetic weights loaded (on the CPU); returns (module, fp32 state dict)."""
    cfg = CASES[name]["cfg"]
    v = paella_amd.VQModel(**cfg)
    sd = weights_for(v, cfg["bottleneck_blocks"])
    return v, sd


def _as(sd, dtype):
    return {k: (t.to(dtype) if t.is_floating_point() else t) for k, t in sd.items()}


def ref_cfg(cfg):
    """The configuration the references are evaluated with: scale_factor as the fp32 value the C ABI carries (paella_vqgan_config.scale_factor is a float),
    so the fp64 reference divides by the number the library divides by."""
    return dict(cfg, scale_factor=float(np.float32(cfg["scale_factor"])))


def nearest_margin(rows64, codebook64):
    """Squared-distance margin between the two nearest codes of every row, in fp64."""
    top = torch.cdist(rows64, codebook64).pow(2).topk(2, dim=1, largest=False).values
    return top[:, 1] - top[:, 0]


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs and references of one case, computed once: the image, the decode tokens (index 0 and K - 1 forced in: encoded tokens collapse onto a few
    codes and would not exercise the gather), the decode latents codebook[tokens] / sf, and for each of fp64 / fp32 the oracle's encode and both decodes."""
    c = CASES[name]
    cfg, B, h, w = c["cfg"], c["B"], c["h"], c["w"]
    rc = ref_cfg(cfg)
    f = 2 ** cfg["levels"]
    K = cfg["codebook_size"]
    _, sd = new_model(name)
    g = torch.Generator().manual_seed(c["seed"])
    img = torch.rand(B, 3, h * f, w * f, generator=g)
    tokens = torch.randint(0, K, (B, h, w), generator=g)
    tokens.view(-1)[0] = 0
    tokens.view(-1)[-1] = K - 1
    cb = sd["vquantizer.codebook.weight"]
    sf32 = torch.tensor(rc["scale_factor"], dtype=torch.float32)
    lat_in = (cb[tokens] / sf32).permute(0, 3, 1, 2).contiguous()  # what encode returns as qe for these tokens
    out = dict(cfg=cfg, B=B, h=h, w=w, sd=sd, img=img, tokens=tokens, lat_in=lat_in)
    with torch.no_grad():
        for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
            s = _as(sd, dt)
            qe, lat, idx, loss = O.vq_encode(s, rc, img.to(dt))
            out[tag] = dict(qe=qe, lat=lat, idx=idx, loss=loss, dec_idx=O.vq_decode_indices(s, rc, tokens), dec=O.vq_decode(s, rc, lat_in.to(dt)))
        r64 = out["f64"]
        rows = (r64["lat"] * rc["scale_factor"]).permute(0, 2, 3, 1).reshape(-1, cfg["c_latent"])
        out["margin"] = nearest_margin(rows, cb.double())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The quantiser on its own: (D, K, rows).  D = 4 with K <= 8192 and rows >= 4096 takes the kernel that keeps the codebook in LDS, everything else one
# wave per row; 4097 / 4160 / 5000 / 4096 rows sit on and past the switch with a partial last 64-row chunk, 8193 codes must fall back to the row kernel,
# 8191 / 100 / 37 / 257 / 1000 codes give the lanes of a wave unequal (or no) shares of the codebook, D = 8 ... 64 run the row kernel at general D.
# ---------------------------------------------------------------------------------------------------------------------
QUANT_SHAPES = [(4, 8192, 4097), (4, 8191, 4160), (4, 100, 5000), (4, 37, 4096), (4, 8193, 4100), (8, 1000, 333), (16, 257, 130), (64, 37, 67), (12, 64, 5)]
QUANT_NEAR_TIE_CAP = 1e-3  # near-tie rows of a shape, as a fraction of its rows


def quant_cfg(D, K):
    return dict(levels=1, bottleneck_blocks=1, c_hidden=8, c_latent=D, codebook_size=K, scale_factor=1.0)


def new_quant_model(D, K):
    """The cheapest model that owns a [K, D] codebook; returns (module, fp32 codebook)."""
    cfg = quant_cfg(D, K)
    v = paella_amd.VQModel(**cfg)
    sd = weights_for(v, 1)
    return v, sd["vquantizer.codebook.weight"]


def brute_force(x, codebook):
    """fp64 nearest code by |e|^2 + |x|^2 - 2 x.e, first minimum: (indices, margin between the two smallest distances)."""
    cb, xd = codebook.double(), x.double()
    d = (cb * cb).sum(1)[None, :] + (xd * xd).sum(1)[:, None] - 2.0 * xd @ cb.t()
    top = d.topk(2, dim=1, largest=False).values
    return d.argmin(1), top[:, 1] - top[:, 0]


@functools.lru_cache(maxsize=None)
def quant_reference(D, K, rows):
    _, cb = new_quant_model(D, K)
    g = torch.Generator().manual_seed(D * 1000 + K)
    x = torch.randn(rows, D, generator=g) * 1.2 * cb.std()
    idx, margin = brute_force(x, cb)
    return dict(codebook=cb, x=x, idx=idx, margin=margin)

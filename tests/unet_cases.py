"""Case table and fp64 reference for the UNet geometry tests (test infrastructure; a plain module, not a conftest).

`paella_unet_create` accepts 1 to 8 levels, any c_hidden that is a multiple of 8, any level_config over C T A F, attention at any level, patch 1 or 2, self-attention
on or off and any c_r; the shipped configurations (oracle/golden_configs.py) are one family: 2 / 3 levels of widths that are multiples of 32 and never shrink going
down, nhead[0] = -1, CT / CTA levels.  The cases below walk the rest, each as small as the path it is there for allows (the `why` of a case says what that is, and
tests/test_unet_cases.py derives it from the configuration):

  one_level     no DOWN / UP; attention at level 0 with D = 16; clf fed by an AttnBlock's row statistics (3 blocks of 16 columns); 15 positions per sample with
                B = 3: the per-sample GRN kernel, and 16-row blocks that straddle samples
  attn_level0   256 queries at level 0 with D = 32 (the LDS-staged attention kernel inside a network); the split at level 0: one level is replicated
  c_not_16      widths = 8 mod 16: no statistics fold for UP 72 -> 40 or for clf, a fold for UP 96 -> 72; GEMM K = 40 / 72 / 160 / 288; D = 48; labels and widths
                that are multiples of 4 only; odd B
  four_levels   four levels; a width that shrinks going down (64 -> 48); A right after DOWN (no producer); T first in a level (standalone); F in front of UP;
                2 positions per sample at the bottom; S_byt5 = 0 with two CLIP-image entries
  orders        the split at block 0; T after A; a C that is not first in an up level (no skip reaches it); two T in a row; D = 64; odd c_r; patch 1; no
                self-attention
  no_timestep   ts_total == 0; a level that is one AttnBlock; 96 -> 32 -> 64
  no_attention  n_attn == 0: the split falls back to 0 and the conditioning is unused
  heads         D = 112 and 128 between real projections; 224 is no multiple of 64 next to 256, which is

The reference is the project's own oracle (oracle/paella_oracle.unet_forward, dtype-generic) on the state dict cast to torch.float64; the same function in fp32 gives
the error a plain fp32 implementation makes on the same inputs, which is what the HIP engine is measured against.  Both receive the timestep embedding as the fp32
evaluation O.r_embedding(r.float(), c_r): the angles fl(fl(r * 1e4) * freq) are what every fp32 route computes, bit for bit, so they are an input of the network and
not an error of it (tests/train_step_model.step).  Everything is computed once per process and shared; nobody writes to what `reference` returns.
"""
import functools

import torch

import paella_amd
from oracle import golden_configs as G
from oracle import paella_oracle as O
from tests import train_step_model as S
from tests.helpers import cond_for, weights_for

NEAR_TIE_EPS = 1e-4     # fp64 top-1 / top-2 margin below which a position is a near-tie (the suite's definition: tests/helpers.argmax_report)
NEAR_TIE_CAP = 0.01     # near-ties of a case, as a fraction of its positions


def _case(c_hidden, nhead, blocks, level_config, B, H, W, S_byt5, n_img, seed, **over):
    cfg = dict(c_in=32, c_out=32, num_labels=64, c_r=16, patch_size=2, c_cond=64, c_hidden=c_hidden, nhead=nhead, blocks=blocks, level_config=level_config,
               clip_embd=48, byt5_embd=40, clip_seq_len=4, kernel_size=3, self_attn=True)
    cfg.update(over)
    return dict(cfg=cfg, B=B, H=H, W=W, S_byt5=S_byt5, n_img=n_img, seed=seed)


CASES = {
    "one_level": _case([48], [3], [2], ["CTA"], 3, 6, 10, 5, 1, 201),
    "attn_level0": _case([64, 64], [2, 4], [1, 1], ["CTA", "CTA"], 1, 32, 32, 3, 0, 202),
    "c_not_16": _case([40, 72, 96], [-1, -1, 2], [1, 2, 1], ["CT", "CTF", "CTA"], 3, 8, 24, 3, 1, 203, c_in=20, c_out=20, num_labels=36, c_cond=24, clip_seq_len=1),
    "four_levels": _case([32, 64, 48, 96], [-1, 4, 3, 2], [1, 1, 2, 1], ["CT", "CTA", "ACT", "TAF"], 2, 16, 32, 0, 2, 204),
    "orders": _case([64, 128], [1, 2], [2, 1], ["ATC", "TTFA"], 2, 4, 6, 7, 0, 205, patch_size=1, self_attn=False, c_r=17),
    "no_timestep": _case([96, 32, 64], [-1, 2, 1], [1, 1, 1], ["C", "A", "CA"], 1, 8, 8, 2, 1, 206, c_r=8),
    "no_attention": _case([40, 56], [-1, -1], [1, 2], ["CT", "FTC"], 2, 4, 12, 2, 0, 207),
    "heads": _case([64, 224, 256], [-1, 2, 2], [1, 1, 1], ["CT", "CTA", "CTA"], 2, 8, 8, 9, 1, 208),
}
CASE_NAMES = list(CASES)


# ---------------------------------------------------------------------------------------------------------------------
# what a configuration IS, from its fields alone (nothing here reads the library or paella_amd.training)
# ---------------------------------------------------------------------------------------------------------------------
def level_sequences(cfg):
    """the block kinds of every level list in forward order: down levels ('D' first below level 0), then up levels ('U' last above level 0) -> [(level, str)]"""
    n = len(cfg["c_hidden"])
    down = [(i, ("D" if i > 0 else "") + cfg["level_config"][i] * cfg["blocks"][i]) for i in range(n)]
    up = [(i, cfg["level_config"][i] * cfg["blocks"][i] + ("U" if i > 0 else "")) for i in reversed(range(n))]
    return down + up


def positions_per_sample(cfg, H, W):
    """positions of one sample at every level"""
    return [(H // (cfg["patch_size"] << l)) * (W // (cfg["patch_size"] << l)) for l in range(len(cfg["c_hidden"]))]


def first_attention(cfg):
    """(level, index in that down level's own blocks) of the first AttnBlock on the way down, or None"""
    for level, seq in level_sequences(cfg)[:len(cfg["c_hidden"])]:
        blocks = seq.lstrip("D")
        if "A" in blocks:
            return level, blocks.index("A")
    return None


def ts_total(cfg):
    """the [a | b] columns of all TimestepBlocks together"""
    return sum(2 * cfg["c_hidden"][level] * seq.count("T") for level, seq in level_sequences(cfg))


def modulation_plan(cfg):
    """What the train-mode forward under set_training_modulation("hip") must ask of `timestep_modulate`, one (residual, layernorm) per TimestepBlock in forward
    order: the residual comes from a C / F block right in front of it in the same level (not from an A, a D, or another T -- the second of T T takes none, and a T
    that opens a level takes none), the LayerNorm rows are asked for when an A / F block follows in the same level (not for a C, a U, or the level's end)."""
    plan = []
    for _, seq in level_sequences(cfg):
        for j, k in enumerate(seq):
            if k == "T":
                plan.append((j > 0 and seq[j - 1] in "CF", j + 1 < len(seq) and seq[j + 1] in "AF"))
    return plan


def new_model(name):
    """A fresh paella_amd.Paella of the case with the suite's seeded synthetic weights loaded (on the CPU); returns (module, fp32 state dict)."""
    cfg = CASES[name]["cfg"]
    m = paella_amd.Paella(**cfg)
    sd = weights_for(m, sum(cfg["blocks"]))
    return m, sd


def inexact_r(B, seed):
    """B timesteps in (0, 1] whose product with 1e4 is inexact in fp32 (seeded; checked)"""
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(B, generator=g).mul(0.998).add(0.001)
    assert bool(((r.double() * 10000.0) != (r * 10000.0).double()).all())
    return r


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs and eval-mode references of one case, computed once: tokens x, timesteps r, the conditional and the unconditional set (different seeds), the fp32
    timestep embedding both dtypes receive, and for each of fp64 / fp32 the oracle's logits and conditioning embeddings of both sets."""
    c = CASES[name]
    cfg, B, H, W = c["cfg"], c["B"], c["H"], c["W"]
    _, sd = new_model(name)
    g = torch.Generator().manual_seed(c["seed"])
    x = torch.randint(0, cfg["num_labels"], (B, H, W), generator=g)
    r = inexact_r(B, c["seed"] + 1000)
    cond = cond_for(cfg, B, c["S_byt5"], c["n_img"], G.COND_SEED + c["seed"])
    uncond = cond_for(cfg, B, c["S_byt5"], c["n_img"], G.COND_SEED + c["seed"] + 500)
    r_embed = O.r_embedding(r.float(), cfg["c_r"])
    out = dict(cfg=cfg, B=B, H=H, W=W, sd=sd, x=x, r=r, cond=cond, uncond=uncond, r_embed=r_embed)
    with torch.no_grad():
        for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
            res = {}
            for which, cc in (("c", cond), ("u", uncond)):
                taps = {}
                res["logits_" + which] = O.unet_forward(sd, cfg, x, r, dtype=dt, taps=taps, r_embed=r_embed, **cc)
                res["c_embed_" + which] = taps["c_embed"]
            out[tag] = res
    top2 = out["f64"]["logits_c"].topk(2, dim=1).values
    out["near"] = (top2[:, 0] - top2[:, 1]) < NEAR_TIE_EPS
    return out


def train_inputs(name):
    """S.inputs of the case: its grid, its conditioning rows, its seed"""
    c = CASES[name]
    return S.inputs(c["cfg"], c["B"], c["H"], c["W"], seed=c["seed"], S_byt5=c["S_byt5"], n_img=c["n_img"])

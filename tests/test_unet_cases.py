"""CPU: the case table of the UNet geometry tests (tests/unet_cases.py) -- that every case IS what it is listed for, derived from its configuration; that the
argmax check of the GPU tests is a fair demand (few fp64 near-ties); that handing the timestep embedding to the oracle changes nothing when it is not handed over;
and that with it handed over the fp32 and the fp64 reference agree as closely as the arithmetic of the network alone warrants."""
import pytest
import torch

import paella_amd
from oracle import paella_oracle as O
from tests import train_step_model as S
from tests import unet_cases as U


def _cfg(name):
    return U.CASES[name]["cfg"]


def _pps(name):
    c = U.CASES[name]
    return U.positions_per_sample(c["cfg"], c["H"], c["W"])


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_case_constructs_and_its_grid_divides(name):
    c = U.CASES[name]
    cfg = c["cfg"]
    m, sd = U.new_model(name)
    assert isinstance(m, paella_amd.Paella) and cfg["c_in"] == cfg["c_out"]
    assert (cfg["clip_embd"], cfg["byt5_embd"], cfg["kernel_size"]) == (48, 40, 3)
    div = cfg["patch_size"] << (len(cfg["c_hidden"]) - 1)
    assert c["H"] % div == 0 and c["W"] % div == 0
    assert all(w % 8 == 0 for w in cfg["c_hidden"])
    assert sum(v.numel() for v in sd.values()) <= 3.7e6
    assert c["B"] * c["H"] * c["W"] <= 1024
    S.levels_of(cfg, (c["H"], c["W"]))      # the levels' geometries are pairwise distinct: the mirror's masks can tell the level from a tensor


def test_what_each_case_is_there_for():
    pps = {n: _pps(n) for n in U.CASE_NAMES}
    not16 = {n: [l for l, p in enumerate(pps[n]) if p % 16] for n in U.CASE_NAMES}
    c_not16 = {n: [l for l, w in enumerate(_cfg(n)["c_hidden"]) if w % 16] for n in U.CASE_NAMES}
    seqs = {n: U.level_sequences(_cfg(n)) for n in U.CASE_NAMES}
    # positions per sample, and the levels where a 16-row block straddles two samples (B > 1) or the per-sample GRN kernel runs
    assert pps["one_level"] == [15] and U.CASES["one_level"]["B"] == 3 and not16["one_level"] == [0]
    assert pps["attn_level0"] == [256, 64] and not16["attn_level0"] == []
    assert pps["c_not_16"] == [48, 12, 3] and not16["c_not_16"] == [1, 2] and U.CASES["c_not_16"]["B"] % 2 == 1
    assert pps["four_levels"] == [128, 32, 8, 2] and not16["four_levels"] == [2, 3]
    assert pps["orders"] == [24, 6] and not16["orders"] == [0, 1]
    assert pps["no_timestep"] == [16, 4, 1] and pps["no_attention"] == [12, 3] and pps["heads"] == [16, 4, 1]
    # widths that are no multiple of 16: no LayerNorm statistics can be folded from a producer of that width
    assert c_not16["c_not_16"] == [0, 1] and c_not16["no_attention"] == [0, 1]
    assert all(not c_not16[n] for n in ("one_level", "attn_level0", "four_levels", "orders", "no_timestep", "heads"))
    # where the first AttnBlock sits: the block at which a shared prefix ends
    assert U.first_attention(_cfg("one_level")) == (0, 2) and U.first_attention(_cfg("attn_level0")) == (0, 2)
    assert U.first_attention(_cfg("orders")) == (0, 0) and U.first_attention(_cfg("no_attention")) is None
    assert U.first_attention(_cfg("c_not_16")) == (2, 2) and U.first_attention(_cfg("four_levels")) == (1, 2)
    assert U.first_attention(_cfg("no_timestep")) == (1, 0) and U.first_attention(_cfg("heads")) == (1, 2)
    # TimestepBlocks
    assert U.ts_total(_cfg("no_timestep")) == 0 and all(U.ts_total(_cfg(n)) > 0 for n in U.CASE_NAMES if n != "no_timestep")
    assert U.ts_total(_cfg("orders")) == 2 * (2 * 2 * 64 + 2 * 2 * 128)
    # head widths
    heads = {n: sorted({w // h for w, h, lc in zip(_cfg(n)["c_hidden"], _cfg(n)["nhead"], _cfg(n)["level_config"]) if "A" in lc}) for n in U.CASE_NAMES}
    assert heads == {"one_level": [16], "attn_level0": [16, 32], "c_not_16": [48], "four_levels": [16, 48], "orders": [64], "no_timestep": [16, 64],
                     "no_attention": [], "heads": [112, 128]}
    # block orders: A right after DOWN, T first in a level, F in front of UP, a width that shrinks; T after A, T T, a C that is not first in an up level
    four = dict((i, s) for i, s in seqs["four_levels"][:4])
    assert four[2].startswith("DA") and four[3].startswith("DT") and seqs["four_levels"][4] == (3, "TAFU")
    assert _cfg("four_levels")["c_hidden"][2] < _cfg("four_levels")["c_hidden"][1]
    assert seqs["orders"] == [(0, "ATCATC"), (1, "DTTFA"), (1, "TTFAU"), (0, "ATCATC")]
    assert seqs["one_level"] == [(0, "CTACTA"), (0, "CTACTA")]
    # the conditioning rows
    assert U.CASES["four_levels"]["S_byt5"] == 0 and U.CASES["four_levels"]["n_img"] == 2


def test_modulation_plans():
    """(residual, layernorm) per TimestepBlock, written out by hand for the orders the cases are there for"""
    assert U.modulation_plan(_cfg("no_timestep")) == []
    # ATC ATC | D TTFA | TTFA U | ATC ATC: T after A takes no residual and is followed by C: (F, F); T T F: the first opens the level or follows D, the second
    # follows a T and stands in front of F
    assert U.modulation_plan(_cfg("orders")) == [(False, False)] * 2 + [(False, False), (False, True)] * 2 + [(False, False)] * 2
    # CT | D CTA | D ACT ACT | D TAF | TAF U | ACT ACT U | CTA U | CT: a T that opens a level (after D, and first of the up path) takes no residual
    Y, N = True, False
    assert U.modulation_plan(_cfg("four_levels")) == [(Y, N), (Y, Y), (Y, Y), (Y, N), (N, Y), (N, Y), (Y, Y), (Y, N), (Y, Y), (Y, N)]
    # CT | D FTC FTC | FTC FTC U | CT
    assert U.modulation_plan(_cfg("no_attention")) == [(Y, N)] * 6
    # CT | D CTF CTF | D CTA | CTA U | CTF CTF U | CT
    assert U.modulation_plan(_cfg("c_not_16")) == [(Y, N)] + [(Y, Y)] * 6 + [(Y, N)]
    assert U.modulation_plan(_cfg("one_level")) == [(Y, Y)] * 4


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_near_ties_are_rare(name):
    r = U.reference(name)
    n, total = int(r["near"].sum()), r["near"].numel()
    print("%s: %d of %d positions are fp64 near-ties (margin < %g)" % (name, n, total, U.NEAR_TIE_EPS))
    assert n <= U.NEAR_TIE_CAP * total


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_r_embed_none_leaves_the_oracle_unchanged(name):
    """unet_forward(..., r_embed=None) and the call without the argument give the same bits, in fp32 and fp64; and in fp32 handing over the oracle's own embedding
    gives them too (it IS what the default computes)"""
    r = U.reference(name)
    cfg, sd, x, t = r["cfg"], r["sd"], r["x"], r["r"]
    with torch.no_grad():
        for dt in (torch.float32, torch.float64):
            a = O.unet_forward(sd, cfg, x, t, dtype=dt, **r["cond"])
            b = O.unet_forward(sd, cfg, x, t, dtype=dt, r_embed=None, **r["cond"])
            assert torch.equal(a, b) and a.dtype == dt
        given = O.unet_forward(sd, cfg, x, t, dtype=torch.float32, r_embed=r["r_embed"], **r["cond"])
        assert torch.equal(given, O.unet_forward(sd, cfg, x, t, dtype=torch.float32, **r["cond"]))
        assert torch.equal(given, r["f32"]["logits_c"])
        # the embedding is cast to the dtype of the evaluation, whatever it arrives as
        assert torch.equal(O.unet_forward(sd, cfg, x, t, dtype=torch.float64, r_embed=r["r_embed"].double(), **r["cond"]), r["f64"]["logits_c"])
        taps = {}
        O.unet_forward(sd, cfg, x, t, dtype=torch.float64, r_embed=r["r_embed"], taps=taps, **r["cond"])
        assert taps["r_embed"].dtype == torch.float64 and torch.equal(taps["r_embed"], r["r_embed"].double())


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_fp32_reference_is_close_to_fp64_with_the_embedding_given(name):
    """A guard on the reference, not on the kernels: 2e-5 is the bound tests/test_gpu_unet.py applies to networks of this size (measured 2.3e-6 ... 5.2e-6); with the
    embedding redone in fp64 the same gap is 6e-5 ... 1.3e-4"""
    r = U.reference(name)
    gap = max(float((r["f32"]["logits_" + w].double() - r["f64"]["logits_" + w]).abs().max()) for w in "cu")
    print("%s: max|fp32 oracle - fp64 oracle| over the logits = %.3e" % (name, gap))
    assert gap < 2e-5
    if name != "no_attention":
        assert not torch.equal(r["f64"]["logits_c"], r["f64"]["logits_u"])
    else:
        assert torch.equal(r["f64"]["logits_c"], r["f64"]["logits_u"])


def test_train_mirror_runs_on_every_case():
    """train_step_model.step in fp64 and fp32 on every case: finite, a gradient for every parameter, and the fp32 mirror within 2e-5 of the fp64 one in the logits"""
    for name in U.CASE_NAMES:
        r = U.reference(name)
        inp = U.train_inputs(name)
        p64, _, l64, g64 = S.step(r["sd"], r["cfg"], inp, None, torch.float64)
        p32, _, l32, g32 = S.step(r["sd"], r["cfg"], inp, None, torch.float32)
        m, _ = U.new_model(name)
        # every parameter the step reaches has a gradient: all but the CLIP-image mapper without a CLIP-image entry, and the three mappers without an AttnBlock
        unused = [] if U.CASES[name]["n_img"] else ["clip_image_mapper."]
        unused += [] if U.first_attention(r["cfg"]) or any("A" in lc for lc in r["cfg"]["level_config"]) else ["byt5_mapper.", "clip_mapper.", "clip_image_mapper."]
        assert set(g64) == set(g32) == {k for k, _ in m.named_parameters() if not any(k.startswith(u) for u in unused)}
        assert all(bool(torch.isfinite(v).all()) for v in g64.values())
        gap = float((p32.double() - p64).abs().max())
        print("%s: training mirror, max|fp32 - fp64| over the logits = %.3e" % (name, gap))
        assert gap < 2e-5

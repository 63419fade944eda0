"""CPU: the VQGAN geometry cases (tests/vqgan_cases.py) are usable -- exact token equality is a fair demand of tests/test_gpu_vqgan_geometries.py only
where the fp64 reference has no nearest-code near-tie, and the quantiser inputs may have near-ties on at most 0.1 % of their rows."""
import pytest
import torch

from tests import vqgan_cases as V


@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_case_has_no_near_tie(name):
    r = V.reference(name)
    cfg = r["cfg"]
    margin = r["margin"]
    f64, f32 = r["f64"], r["f32"]
    e_lat = float((f32["lat"].double() - f64["lat"]).abs().max())
    e_dec = max(float((f32[k].double() - f64[k]).abs().max()) for k in ("dec", "dec_idx"))
    print("%s: %d positions, min nearest-code margin %.3e, %d distinct tokens of %d codes; fp32 oracle vs fp64: tokens equal %s, latents %.2e at max |latent| %.2f, "
          "decodes %.2e" % (name, margin.numel(), float(margin.min()), f64["idx"].unique().numel(), cfg["codebook_size"], torch.equal(f32["idx"], f64["idx"]),
                            e_lat, float(f64["lat"].abs().max()), e_dec))
    assert r["img"].shape == (r["B"], 3, r["h"] << cfg["levels"], r["w"] << cfg["levels"])
    assert f64["idx"].shape == (r["B"], r["h"], r["w"]) and f64["lat"].dtype == torch.float64
    for k in ("qe", "lat", "dec", "dec_idx"):
        assert torch.isfinite(f64[k]).all()
    assert int((margin < V.NEAR_TIE_EPS).sum()) == 0, "a nearest-code near-tie in the fp64 reference: change the case's seed or size, not this condition"
    assert int(r["tokens"].min()) == 0 and int(r["tokens"].max()) == cfg["codebook_size"] - 1


@pytest.mark.parametrize("D,K,rows", V.QUANT_SHAPES)
def test_quantiser_inputs_have_few_near_ties(D, K, rows):
    q = V.quant_reference(D, K, rows)
    near = int((q["margin"] < V.NEAR_TIE_EPS).sum())
    print("quantiser input D=%d K=%d rows=%d: %d near-tie rows (margin < %g), %d distinct nearest codes" % (D, K, rows, near, V.NEAR_TIE_EPS, q["idx"].unique().numel()))
    assert q["x"].shape == (rows, D) and q["codebook"].shape == (K, D)
    assert near <= V.QUANT_NEAR_TIE_CAP * rows
    # the brute force is the oracle's search: same distance expression, same first minimum
    assert torch.equal(q["idx"], V.O.vector_quantize(q["x"].double(), q["codebook"].double())[1])

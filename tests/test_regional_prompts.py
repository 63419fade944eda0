"""CPU: regional prompts -- the query-group builder against a brute-force loop, the masked model by hand, every host refusal of RequestStream / admit, and the
argument checks of the C entry points (all of which return before any HIP call)."""
import ctypes

import pytest
import torch

import paella_amd
from oracle import golden_configs as G
from paella_amd import modules, sampling
from tests import region_model as RM


# ---------------------------------------------------------------------------------------------------------------- region_query_groups
def _masks(R, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(R, H, W, dtype=torch.bool)
    if R > 0:
        m[0, :, : W // 2] = True                              # a half image
    if R > 1:
        m[1, 1:H - 3, 3:W - 2] = True                         # cuts through 2x2 (and 4x4, 8x8) blocks
    if R > 2:
        m[2] = torch.rand(H, W, generator=g) < 0.05           # scattered single positions: OR-pooling spreads them on the coarse levels
    return m


@pytest.mark.parametrize("cfg_name", ["UNET_TINY", "UNET_VARIANT"])
@pytest.mark.parametrize("H,W", [(32, 32), (16, 32)])
def test_region_query_groups_against_brute_force(cfg_name, H, W):
    cfg = getattr(G, cfg_name)
    p, n = cfg["patch_size"], len(cfg["c_hidden"])
    Qtot = sum(((H // p) >> l) * ((W // p) >> l) for l in range(n))
    assert modules.region_query_total(cfg, H, W) == Qtot
    for R in (0, 1, 3):
        masks = _masks(R, H, W, 11 * R + H)
        got = paella_amd.region_query_groups(masks, cfg, H, W)
        assert got.dtype == torch.int32 and tuple(got.shape) == (Qtot,)
        assert got.tolist() == RM.query_groups_bruteforce(masks.tolist(), cfg, H, W)
        assert bool((got & 1).all())                          # bit 0 everywhere
    # integer masks count as bool; an all-zero mask leaves bit 0 alone
    assert torch.equal(paella_amd.region_query_groups(_masks(2, H, W, 5).to(torch.int64) * 7, cfg, H, W), paella_amd.region_query_groups(_masks(2, H, W, 5), cfg, H, W))
    assert paella_amd.region_query_groups(torch.zeros(2, H, W, dtype=torch.bool), cfg, H, W).tolist() == [1] * Qtot
    with pytest.raises(ValueError, match="regions"):
        paella_amd.region_query_groups(torch.zeros(1, H, W), cfg, H, W)                       # floating dtype
    with pytest.raises(ValueError, match="regions"):
        paella_amd.region_query_groups(torch.zeros(1, H + 1, W, dtype=torch.bool), cfg, H, W)
    with pytest.raises(ValueError, match="regions"):
        paella_amd.region_query_groups(torch.zeros(31, H, W, dtype=torch.bool), cfg, H, W)


def test_region_bits_use_thirty_regions_and_never_the_sign_bit():
    cfg, H, W = G.UNET_VARIANT, 8, 8
    masks = torch.zeros(30, H, W, dtype=torch.bool)
    masks[29, 0, 0] = True
    got = paella_amd.region_query_groups(masks, cfg, H, W)
    assert int(got[0]) == 1 | (1 << 30) and int(got.min()) > 0


# ---------------------------------------------------------------------------------------------------------------- the model by hand
def test_masked_attention_by_hand():
    """2 queries, 3 keys (1 self + 2 conditioning), D = 1: query 0 sees the self key and conditioning key 1, query 1 everything"""
    q = torch.tensor([[1.0], [2.0]])
    k = torch.tensor([[0.0], [1.0], [-1.0]])
    v = torch.tensor([[10.0], [20.0], [30.0]])
    vis = RM.visibility([0b101, 0b111], [0b010, 0b100], Lself=1)
    assert vis.tolist() == [[True, False, True], [True, True, True]]
    out = RM.masked_attention(q, k, v, vis, scale=1.0)
    e = lambda x: float(torch.tensor(x, dtype=torch.float64).exp())
    row0 = (10 * e(0.0) + 30 * e(-1.0)) / (e(0.0) + e(-1.0))
    row1 = (10 * e(0.0) + 20 * e(2.0) + 30 * e(-2.0)) / (e(0.0) + e(2.0) + e(-2.0))
    assert out.dtype == torch.float64 and torch.allclose(out, torch.tensor([[row0], [row1]], dtype=torch.float64), rtol=1e-14, atol=0)
    # key weights act after the softmax on the last keys by INDEX, visible or not, without renormalisation
    outw = RM.masked_attention(q, k, v, vis, scale=1.0, weights=torch.tensor([2.0, 0.5]))
    row0w = (10 * e(0.0) + 0.5 * 30 * e(-1.0)) / (e(0.0) + e(-1.0))
    row1w = (10 * e(0.0) + 2.0 * 20 * e(2.0) + 0.5 * 30 * e(-2.0)) / (e(0.0) + e(2.0) + e(-2.0))
    assert torch.allclose(outw, torch.tensor([[row0w], [row1w]], dtype=torch.float64), rtol=1e-14, atol=0)
    # a query that sees nothing: a zero row, not NaN
    none = RM.masked_attention(q, k[1:], v[1:], RM.visibility([0b001, 0b010], [0b010, 0b100], Lself=0), scale=1.0)
    assert none[0].tolist() == [0.0] and float(none[1]) == 20.0


def test_regional_forward_with_everything_visible_is_the_oracle_forward(monkeypatch):
    """the substituted mha / c_embeddings reproduce the oracle's own forward when nothing is masked, and two prompts concatenate as one longer prompt does"""
    from oracle import paella_oracle as O
    from paella_amd import synth
    from tests.helpers import cond_for
    cfg, H, W = G.UNET_VARIANT, 8, 8
    m = paella_amd.Paella(**cfg)
    sd = synth.synth_state_dict(m.state_dict(), seed=G.WEIGHT_SEED, n_blocks=sum(cfg["blocks"]))
    g = torch.Generator().manual_seed(1)
    x, r = torch.randint(0, cfg["num_labels"], (1, H, W), generator=g), torch.tensor([0.4])
    c = cond_for(cfg, 1, 3, 0, 7)
    Qtot = modules.region_query_total(cfg, H, W)
    with torch.no_grad():
        ref = O.unet_forward(sd, cfg, x, r, **c, dtype=torch.float64)
    got = RM.regional_forward(monkeypatch, sd, cfg, x, r, [c], [1] * Qtot, [1] * 5, dtype=torch.float64)
    assert float((got - ref).abs().max()) < 1e-12
    assert O.mha.__module__ == "oracle.paella_oracle"            # the substitution is undone
    # hiding the clip rows (the last 2) from every query == the forward without clip
    with torch.no_grad():
        ref_noclip = O.unet_forward(sd, cfg, x, r, byt5=c["byt5"], dtype=torch.float64)
    got = RM.regional_forward(monkeypatch, sd, cfg, x, r, [c], [1] * Qtot, [1, 1, 1, 2, 2], dtype=torch.float64)
    assert float((got - ref_noclip).abs().max()) < 1e-12 and float((got - ref).abs().max()) > 1e-6


# ---------------------------------------------------------------------------------------------------------------- host refusals
class _FakeModel:
    _cfg = G.UNET_TINY

    def __init__(self, precision="fp32"):
        self.precision = precision

    def get_gemm_precision(self):
        return self.precision


def _cond(B=1, n_byt5=2, clip=True):
    cfg = G.UNET_TINY
    return dict(byt5=torch.zeros(B, n_byt5, cfg["byt5_embd"]), clip=torch.zeros(B, cfg["clip_embd"]) if clip else None, clip_image=None)


def test_max_regions_is_validated_before_anything_touches_a_device():
    m = _FakeModel()
    assert sampling.check_max_regions(2, 16, None, m) == 2 and sampling.check_max_regions(30, 16, None, m) == 30
    for bad in (0, 31, -1, 2.0, True, "2"):
        with pytest.raises(ValueError, match="max_regions"):
            sampling.check_max_regions(bad, 16, None, m)
    with pytest.raises(ValueError, match="max_regions needs max_cond_rows"):
        sampling.check_max_regions(2, None, None, m)
    with pytest.raises(ValueError, match="max_regions excludes the stream-wide attn_weights"):
        sampling.check_max_regions(2, 16, torch.ones(3), m)
    with pytest.raises(ValueError, match="bf16"):
        sampling.check_max_regions(2, 16, None, _FakeModel("bf16"))


def _bare_stream(max_regions=2, max_cond_rows=16, precision="fp32"):
    """the checks sit in front of any device work: exercised on an instance that was never constructed"""
    st = object.__new__(paella_amd.RequestStream)
    st.shape, st.filtering, st.editing, st.max_regions, st.max_cond_rows, st.model = (2, 32, 32), False, False, max_regions, max_cond_rows, _FakeModel(precision)
    return st


def test_admit_refuses_regions_before_touching_the_stream():
    H = W = 32
    ok_mask = torch.zeros(H, W, dtype=torch.bool)
    base = _cond()                                    # 2 ByT5 rows + 4 clip rows = 6
    with pytest.raises(ValueError, match="regions need a stream built with max_regions"):
        _bare_stream(max_regions=None).admit(base, regions=[(_cond(), ok_mask)])
    st = _bare_stream()
    with pytest.raises(ValueError, match="regions: 3 given, the stream admits at most 2"):
        st.admit(base, regions=[(_cond(), ok_mask)] * 3)
    with pytest.raises(ValueError, match="regions: the mask of region 0"):
        st.admit(base, regions=[(_cond(), torch.zeros(H, W + 1, dtype=torch.bool))])
    with pytest.raises(ValueError, match="regions: the mask of region 1"):
        st.admit(base, regions=[(_cond(), ok_mask), (_cond(), torch.zeros(H, W))])          # floating dtype
    with pytest.raises(ValueError, match="regions: region 0 takes the inputs of ONE prompt"):
        st.admit(base, regions=[(_cond(B=2), ok_mask)])
    with pytest.raises(ValueError, match="regions: 18 base \\+ region conditioning rows, the stream's slots hold 16"):
        st.admit(base, regions=[(_cond(), ok_mask), (_cond(), ok_mask)])                    # 6 + 6 + 6
    with pytest.raises(ValueError, match="regions are not offered in the bf16"):
        _bare_stream(precision="bf16").admit(base, regions=[(_cond(), ok_mask)])
    with pytest.raises(ValueError, match="regions: entry 0"):
        st.admit(base, regions=[ok_mask])
    # the checks accept what they should: integer masks, overlapping masks, an all-zero mask, no clip
    plan, masks = st._check_regions([(_cond(n_byt5=1, clip=False), ok_mask.to(torch.int64)), (_cond(), ~ok_mask)], base)
    assert [rows for _, rows in plan] == [1, 6] and masks.dtype == torch.bool and tuple(masks.shape) == (2, H, W)
    assert st._check_regions(None, base) == (None, None)


def test_region_tables_refuse_bad_shapes():
    with pytest.raises(ValueError, match="RegionTables"):
        paella_amd.RegionTables(0, 4, 4, device="cpu")
    t = paella_amd.RegionTables(2, 5, 3, device="cpu")
    assert t.q_groups.tolist() == [[1] * 5] * 2 and t.k_groups.tolist() == [[1] * 3] * 2 and t.q_groups.dtype == torch.int32
    t.set(1, torch.tensor([1, 3, 5, 1, 1], dtype=torch.int32), torch.tensor([1, 2], dtype=torch.int32))
    assert t.q_groups.tolist() == [[1] * 5, [1, 3, 5, 1, 1]] and t.k_groups.tolist() == [[1, 1, 1], [1, 2, 1]]
    t.set(1)
    assert t.q_groups[1].tolist() == [1] * 5 and t.k_groups[1].tolist() == [1] * 3
    with pytest.raises(ValueError, match="regions"):
        t.set(0, torch.ones(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="regions"):
        t.set(0, None, torch.ones(4, dtype=torch.int32))
    with pytest.raises(IndexError):
        t.set(2)
    t.set(0, torch.full((5,), 3, dtype=torch.int32), torch.full((3,), 2, dtype=torch.int32)).clear()
    assert bool((t.q_groups == 1).all()) and bool((t.k_groups == 1).all())


# ---------------------------------------------------------------------------------------------------------------- the C ABI, without a GPU
def test_group_table_argument_validation_without_gpu(built_lib):
    """every refusal below returns before any HIP call: the pointers are host arrays that are never dereferenced"""
    lib = built_lib
    buf = (ctypes.c_float * 64)()
    tab = (ctypes.c_int32 * 64)()
    out = (ctypes.c_int64 * 64)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    B, nhead, D, Lq, Lself, Lcond = 2, 4, 16, 16, 16, 8

    def op(qg, qp, kg, kp):
        return lib.paella_op_attention_rg(p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), B, nhead, D, Lq, Lself, Lcond, None, None, None, 0, qg, qp, kg, kp, None)

    assert op(p(tab), Lq, None, Lcond) == -1 and b"q_groups and k_groups must be given together" in lib.paella_last_error()
    assert op(None, Lq, p(tab), Lcond) == -1 and b"q_groups and k_groups must be given together" in lib.paella_last_error()
    assert op(p(tab), Lq - 1, p(tab), Lcond) == -1 and b"pitches too small" in lib.paella_last_error()
    assert op(p(tab), Lq, p(tab), Lcond - 1) == -1 and b"pitches too small" in lib.paella_last_error()

    H = W = 8
    S = 6

    def logits(qg, qp, kg, kp, m=None):
        return lib.paella_unet_forward_shared_req_rg(m, p(out), p(buf), p(buf), 2, 1, p(buf), H, W, S, p(tab), None, None, 0, qg, qp, kg, kp, p(buf), p(buf), 256, None)

    def tick(qg, qp, kg, kp, m=None):
        return lib.paella_unet_forward_sample_stream_rg(m, p(out), p(buf), p(buf), 2, 1, p(buf), H, W, S, p(tab), None, None, 0, qg, qp, kg, kp, p(out), p(buf), H * W,
                                                        p(tab), p(buf), p(tab), p(out), None, None, None, p(out), p(buf), 256, None)

    for fn, name in ((logits, b"forward_shared_req_rg"), (tick, b"forward_sample_stream_rg")):
        assert fn(p(tab), 100, None, S) == -1 and name + b": q_groups and k_groups must be given together" in lib.paella_last_error()
        assert fn(None, 100, p(tab), S) == -1 and name + b": q_groups and k_groups must be given together" in lib.paella_last_error()
        assert fn(p(tab), 100, p(tab), S - 1) == -1 and name + b": key-group pitches too small" in lib.paella_last_error()
        assert fn(p(tab), 0, p(tab), S) == -1 and name + b": key-group pitches too small" in lib.paella_last_error()
        # both tables NULL: the _kw entry point it extends answers (here: no model)
        assert fn(None, 0, None, 0) != 0 and name not in lib.paella_last_error()

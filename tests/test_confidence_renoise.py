"""CPU: confidence-ordered renoise -- the numpy model of tests/confidence_model.py by hand on small rows, every Python refusal, and every PAELLA_ERR_ARG of the four
new entry points (none of them touches a device)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import paella_amd
from paella_amd import sampling
from tests import confidence_model as CM
from tests import counter_noise as C

INF, NAN = np.float32(np.inf), np.float32(np.nan)


def _sel(scores, t_next, free=None):
    scores = np.float32(scores)
    free = np.ones(scores.size, bool) if free is None else np.asarray(free, bool)
    return np.nonzero(CM.select(scores, free, t_next))[0].tolist()


# ---------------------------------------------------------------------------------------------------------------- the model, by hand
def test_key_orders_scores_and_puts_nan_first():
    s = np.float32([NAN, -INF, -3.0, -1e-30, -0.0, 0.0, 1e-30, 2.0, INF])
    k = CM.score_key(s).astype(np.int64)
    assert k[0] == 0 and (np.diff(k[:4]) > 0).all() and k[4] == k[5] and (np.diff(k[5:]) > 0).all()
    assert k.max() < 0xFFFFFFFF, "no score maps to the key that marks an excluded position"
    assert CM.score_key(np.float32([-NAN]))[0] == 0


def test_ties_go_to_the_lower_index():
    assert _sel([-1.0, -2.0, -2.0, -2.0, -0.5, -2.0], 0.5) == [1, 2, 3]          # n = 3 of the four tied at -2: the three lowest indices
    assert _sel([0.0, -0.0, 0.0, -0.0], 0.5) == [0, 1]                           # -0 == +0: one tie group, by index
    assert _sel([-2.0, -1.0, -2.0, -1.0], 0.75) == [0, 1, 2]                     # the whole group below, then the tie by index: 1, not 3


def test_nan_and_minus_inf_come_first():
    s = [-1.0, -INF, -5.0, NAN, -2.0, NAN, -INF, -0.1]
    assert _sel(s, 0.125) == [3]
    assert _sel(s, 0.25) == [3, 5]
    assert _sel(s, 0.5) == [1, 3, 5, 6]
    assert _sel(s, 0.625) == [1, 2, 3, 5, 6]


def test_count_rounds_half_to_even_in_fp32():
    assert CM.renoise_count(0.25, 10) == 2      # 2.5 -> 2
    assert CM.renoise_count(0.35, 10) == 4      # fp32(0.35) * 10 = 3.5 exactly in fp32 -> 4
    assert float(np.float32(0.35) * np.float32(10)) == 3.5
    assert CM.renoise_count(0.5, 5) == 2 and CM.renoise_count(0.5, 7) == 4
    assert len(_sel(np.arange(10, dtype=np.float32), 0.25)) == 2 and len(_sel(np.arange(10, dtype=np.float32), 0.35)) == 4


def test_threshold_edges():
    s = -np.arange(7, dtype=np.float32)
    assert _sel(s, -1.0) == [] and _sel(s, 0.0) == [] and _sel(s, -0.0) == []
    assert sorted(_sel(s, 1.0)) == list(range(7))
    assert sorted(_sel(s, 3.0)) == list(range(7)), "the count is clamped to the free positions"
    assert _sel(s, NAN) == [] and sorted(_sel(s, INF)) == list(range(7))
    assert _sel([-1.0], 0.5) == [] and _sel([-1.0], 0.51) == [0]                  # one position: rint(0.5) = 0, rint(0.51) = 1


def test_pinned_positions_are_never_chosen_and_the_count_is_over_the_free_ones():
    s = np.float32([-9.0, -8.0, -7.0, -6.0, -5.0, -4.0, -3.0, -2.0])
    free = np.array([0, 1, 0, 1, 1, 0, 1, 1], bool)
    assert _sel(s, 0.5, free) == [1, 3]   # n = rint(0.5 * 5) = 2 (2.5 -> 2), the least confident FREE positions
    assert sorted(_sel(s, 1.0, free)) == [1, 3, 4, 6, 7]
    assert _sel(s, 1.0, np.zeros(8, bool)) == []
    assert _sel(np.float32([NAN, NAN, -1.0]), 0.5, [False, True, True]) == [1]


def test_row_stats_by_hand():
    z = np.log(np.float32([0.5, 0.25, 0.125, 0.125]))
    r = CM.row_stats(z)
    assert r["filtered"] and np.allclose(r["logprob"], np.log([0.5, 0.25, 0.125, 0.125]), atol=1e-6)
    assert abs(r["entropy"] - 1.75 * math.log(2)) < 1e-6
    assert 0 < r["eps_H"] < 1e-5 and (r["eps_logp"] > 0).all() and (r["eps_logp"] < 1e-5).all()
    k = CM.row_stats(z, top_k=2)                                                    # A = the two largest: p = (2/3, 1/3)
    assert np.allclose(k["logprob"][:2], np.log([2 / 3, 1 / 3]), atol=1e-6) and np.isinf(k["logprob"][2:]).all()
    assert abs(k["entropy"] - (math.log(3) - 2 / 3 * math.log(2))) < 1e-6
    t = CM.row_stats(np.float32([1.0, 1.0, 0.0, 0.0]), top_k=1)                     # ties at the k-th value stay in A
    assert np.isfinite(t["logprob"]).sum() == 2
    for bad in (np.float32([0.0, NAN, 1.0]), np.float32([-INF, -INF]), np.float32([0.0, INF])):
        b = CM.row_stats(bad)
        assert not b["filtered"] and np.isneginf(b["logprob"]).all() and math.isnan(b["entropy"])
    m = CM.row_stats(np.float32([0.0, -INF, -1.0]))                                 # a label of probability 0 adds 0 to the entropy
    assert m["filtered"] and np.isneginf(m["logprob"][1]) and math.isfinite(m["entropy"])


def test_score64_uses_word_one_of_the_renoise_call():
    seed, step = 0xC3A5C85C97CB3127, 3
    w0, w1 = CM.renoise_words(seed, np.arange(5), step)
    ref = [C.philox4x32_scalar(seed ^ C.RENOISE_SALT, i, step) for i in range(5)]
    assert w0.tolist() == [r[0] for r in ref] and w1.tolist() == [r[1] for r in ref]
    lp = np.float32([-1.0, -2.0, -INF, NAN, -0.5])
    s, bound = CM.score64(lp, 0.0, 0.4, w1)
    assert np.array_equal(s[[0, 1, 4]], [-1.0, -2.0, -0.5]) and not bound.any()
    s, bound = CM.score64(lp, 4.5, 0.4, w1)
    gt = float(np.float32(4.5) * np.float32(0.4))
    assert np.allclose(s[[0, 1, 4]], lp[[0, 1, 4]] - gt * C.log_exp1(w1)[[0, 1, 4]]) and np.isneginf(s[2]) and np.isnan(s[3])
    assert (bound[[0, 1, 4]] > 0).all() and (bound[[0, 1, 4]] < 1e-4).all()


# ---------------------------------------------------------------------------------------------------------------- host validation
def test_check_renoise():
    assert sampling.check_renoise() == (0, 0.0)
    assert sampling.check_renoise("confidence", 4.5) == (1, 4.5) and sampling.check_renoise("random", 2) == (0, 2.0)
    assert paella_amd.check_renoise is sampling.check_renoise
    for kw, word in [(dict(renoise="greedy"), "renoise"), (dict(renoise=None), "renoise"), (dict(renoise=1), "renoise"), (dict(confidence_noise=-0.5), "confidence_noise"),
                     (dict(confidence_noise=float("nan")), "confidence_noise"), (dict(confidence_noise=float("inf")), "confidence_noise"),
                     (dict(confidence_noise="1"), "confidence_noise"), (dict(confidence_noise=True), "confidence_noise")]:
        with pytest.raises(ValueError, match=word):
            sampling.check_renoise(**kw)


def test_request_renoise():
    pol, g, on = sampling.request_renoise(3, renoise=["random", "confidence", "random"], confidence_noise=[0.0, 4.5, 1.0])
    assert pol.tolist() == [0, 1, 0] and pol.dtype == torch.int32 and g.tolist() == [0.0, 4.5, 1.0] and g.dtype == torch.float32 and on
    assert not sampling.request_renoise(2)[2] and sampling.request_renoise(2, "confidence")[0].tolist() == [1, 1]
    with pytest.raises(ValueError, match="renoise must be one value or a list of 2"):
        sampling.request_renoise(2, renoise=["random"] * 3)
    with pytest.raises(ValueError, match="confidence_noise must be one value or a list of 3"):
        sampling.request_renoise(3, confidence_noise=[0.0, 1.0])
    with pytest.raises(ValueError, match="request 1: confidence_noise"):
        sampling.request_renoise(2, "confidence", [0.0, -1.0])
    with pytest.raises(ValueError, match="request 0: renoise"):
        sampling.request_renoise(2, ["sorted", "random"])


def test_calls_refuse_before_touching_a_device():
    args = (object(), {}, (1, 8, 8))
    with pytest.raises(ValueError, match="renoise='confidence' needs noise='philox'"):
        paella_amd.sample(*args, cfg=None, renoise="confidence")
    with pytest.raises(ValueError, match="renoise='confidence' needs noise='philox'"):
        paella_amd.sample(*args, cfg=None, noise="torch", renoise="confidence", confidence_noise=1.0)
    with pytest.raises(ValueError, match="return_stats needs noise='philox'"):
        paella_amd.sample(*args, cfg=None, return_stats=True)
    with pytest.raises(ValueError, match="renoise='confidence' needs noise='philox'"):
        paella_amd.sample(*args, cfg=None, noise={"init_noise": None}, renoise="confidence")
    with pytest.raises(ValueError, match="renoise='confidence' is not offered with a step temperature of 0"):
        paella_amd.sample(*args, cfg=None, noise="philox", temperature=(1.0, 0.0), renoise="confidence")
    with pytest.raises(ValueError, match="return_stats is not offered with a step temperature of 0"):
        paella_amd.sample(*args, cfg=None, noise="philox", temperature=(1.0, 0.0), return_stats=True)
    with pytest.raises(ValueError, match="renoise must be 'random' or 'confidence'"):
        paella_amd.sample(*args, cfg=None, noise="philox", renoise="Confidence")
    with pytest.raises(ValueError, match="confidence_noise"):
        paella_amd.sample(*args, cfg=None, noise="philox", renoise="confidence", confidence_noise=-1.0)
    u = {"byt5": torch.zeros(1)}
    with pytest.raises(ValueError, match="renoise='confidence' needs noise='philox'"):
        paella_amd.sample_distributed(object(), {}, u, (1, 8, 8), renoise="confidence")
    with pytest.raises(ValueError, match="step temperature of 0"):
        paella_amd.sample_distributed(object(), {}, u, (1, 8, 8), noise="philox", temperature=(0.5, 0.0), renoise="confidence")
    with pytest.raises(ValueError, match="confidence_noise"):
        paella_amd.sample_distributed(object(), {}, u, (1, 8, 8), noise="philox", confidence_noise=-2)
    with pytest.raises(ValueError, match="renoise must be one value or a list of 2"):
        paella_amd.sample_requests(object(), {}, None, (2, 8, 8), [1, 2], cfg=None, renoise=["confidence"])
    with pytest.raises(ValueError, match="request 1: renoise"):
        paella_amd.sample_requests(object(), {}, None, (2, 8, 8), [1, 2], cfg=None, renoise=["confidence", "no"])
    with pytest.raises(ValueError, match="renoise"):
        paella_amd.GraphSampler(object(), {}, None, (1, 8, 8), cfg=None, renoise="best")
    with pytest.raises(ValueError, match="step temperature of 0"):
        paella_amd.GraphSampler(object(), {}, None, (1, 8, 8), cfg=None, temperature=(1.0, 0.0), return_stats=True)


def test_stream_refuses_a_confidence_request_it_was_not_built_for():
    """the check sits in front of any device work: exercised on an instance that was never constructed"""
    st = object.__new__(paella_amd.RequestStream)
    st.shape, st.filtering, st.editing, st.confidence = (2, 8, 8), False, False, False
    with pytest.raises(ValueError, match="renoise='confidence' needs a stream built with confidence=True"):
        st.admit({}, renoise="confidence")
    with pytest.raises(ValueError, match="renoise must be"):
        st.admit({}, renoise="ranked")
    with pytest.raises(ValueError, match="confidence_noise"):
        st.admit({}, confidence_noise=-1.0)
    st._held, st._pos, st._len = [True, False], [1, 0], [1, 0]
    with pytest.raises(ValueError, match="stats=True needs a stream built with confidence=True"):
        st.result(0, stats=True)


# ---------------------------------------------------------------------------------------------------------------- the C ABI, without a GPU
def test_argument_validation_without_gpu(built_lib):
    """every refusal below returns before any HIP call: the pointers are host arrays that are never dereferenced"""
    lib = built_lib
    L, rows = 16, 4
    buf = (ctypes.c_float * (rows * L))()
    out = (ctypes.c_int64 * rows)()
    tab = (ctypes.c_int32 * 8)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    err = lambda: lib.paella_last_error()

    def stats(L=L, mode=0, temperature=1.0, top_k=0, top_p=1.0, typical=1.0, min_tokens=1, keep=None, known=None, lp=p(buf), ent=None):
        return lib.paella_sample_tail_stats(p(buf), None, rows, L, 1.0, 0.0, temperature, mode, 1, None, 0, 0, None, None, 0.0, keep, known, top_k, top_p, typical, min_tokens,
                                            p(out), None, lp, ent, None)

    for kw, word in [(dict(top_p=0.5, typical=0.5), b"mutually exclusive"), (dict(top_p=0.0), b"top_p"), (dict(typical=-0.5), b"typical_mass"), (dict(min_tokens=0), b"min_tokens"),
                     (dict(mode=1), b"argmax"), (dict(temperature=0.0), b"temperature"), (dict(L=16388), b"16384"), (dict(L=18), b"% 4"),
                     (dict(keep=p(out)), b"pin_keep and pin_tokens"), (dict(lp=None, ent=p(buf), L=16388), b"16384")]:
        assert stats(**kw) == -1, kw
        assert word in err(), (kw, err())
    assert stats(lp=None, ent=None, mode=1, top_k=3) == -1 and b"sample_tail_filter:" in err()      # no output: the entry point it extends answers

    def sstats(fk=None, fm=None, L=L, step=p(tab), init=p(out), rps=2, lp=p(buf), ent=p(buf), keep=None):
        return lib.paella_sample_tail_stream_stats(p(buf), None, rows, L, None, p(buf), p(out), rps, step, p(buf), p(tab), init, keep, None, None, fk, fm, p(out), None, lp, ent,
                                                   None)

    assert sstats(p(tab), None) == -1 and b"filter_k and filter_mass" in err()
    assert sstats(None, p(buf)) == -1 and b"filter_k and filter_mass" in err()
    assert sstats(step=None) == -1 and b"required" in err()
    assert sstats(init=None) == -1 and b"required" in err()
    assert sstats(L=16388) == -1 and b"16384" in err()
    assert sstats(rps=3) == -1 and b"rows_per_sample" in err()
    assert sstats(rps=0) == -1 and b"rows_per_sample" in err()
    assert sstats(keep=p(out)) == -1 and b"pin_keep and pin_tokens" in err()
    assert sstats(lp=None, ent=None, step=None) == -1 and b"sample_tail_stream:" in err()             # no output, no tables: the entry points it extends answer

    lp = (ctypes.c_float * rows)()

    def sel(rows=rows, rps=2, policy=1, g=0.0, logprob=p(lp), keep=None, known=None, drawn=p(out), init=p(out), row_offset=0):
        return lib.paella_renoise_select(drawn, logprob, init, rows, rps, 1, None, 0, row_offset, None, 0.5, policy, g, keep, known, p(out), None)

    for kw, word in [(dict(rps=3), b"multiple of rows_per_sample"), (dict(rps=0), b"1 ... 16384"), (dict(rps=-4), b"1 ... 16384"), (dict(rows=16385, rps=16385), b"1 ... 16384"),
                     (dict(g=-1.0), b"confidence_noise"), (dict(g=float("nan")), b"confidence_noise"), (dict(g=float("inf")), b"confidence_noise"),
                     (dict(policy=2), b"policy"), (dict(policy=-1), b"policy"), (dict(logprob=None), b"needs logprob"), (dict(keep=p(out)), b"pin_keep and pin_tokens"),
                     (dict(known=p(out)), b"pin_keep and pin_tokens"), (dict(drawn=None), b"null argument"), (dict(init=None), b"null argument"),
                     (dict(row_offset=-2), b"row_offset")]:
        assert sel(**kw) == -1, kw
        assert word in err(), (kw, err())

    def ssel(rows=rows, rps=2, policy=p(tab), logprob=p(lp), keep=None, known=None, pin_on=None, seeds=p(out), step=p(tab), t_next=p(buf), active=p(tab)):
        return lib.paella_renoise_select_stream(p(out), logprob, p(out), rows, rps, seeds, step, t_next, active, policy, p(buf), keep, known, pin_on, p(out), None)

    for kw, word in [(dict(rps=3), b"multiple of rows_per_sample"), (dict(rps=0), b"1 ... 16384"), (dict(rows=2 * 16385, rps=16385), b"1 ... 16384"),
                     (dict(logprob=None), b"needs logprob"), (dict(keep=p(out)), b"pin_keep and pin_tokens"), (dict(known=p(out)), b"pin_keep and pin_tokens"),
                     (dict(pin_on=p(tab)), b"pin_on"), (dict(seeds=None), b"required"), (dict(step=None), b"required"), (dict(t_next=None), b"required"),
                     (dict(active=None), b"required")]:
        assert ssel(**kw) == -1, kw
        assert word in err(), (kw, err())
    hook = lib.paella_test_renoise_scores
    assert hook(p(out), p(lp), p(out), rows, 2, 1, 0, 0, 0.5, 1, 0.0, None, None, None, None, None, None, None, None, None, p(out), None, None) == -1 and b"scores_out" in err()
    assert hook(p(out), p(lp), p(out), rows, 3, 1, 0, 0, 0.5, 1, 0.0, None, None, None, None, None, None, None, None, None, p(out), p(lp), None) == -1

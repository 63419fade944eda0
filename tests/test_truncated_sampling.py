"""CPU: truncated sampling (top-k, nucleus, typical filtering) -- hand-worked cases of the fp64 model (tests/truncation_model.py), every host-side refusal, the
argument checks of the two C entry points (no device work before them) and the cap on how many candidate rows the GPU tests may reject."""
import ctypes
import math

import numpy as np
import pytest
import torch

import paella_amd
from paella_amd import _lib, sampling
from tests import truncation_model as TM

# a 6-label row: p = softmax(z) = (0.4, 0.25, 0.15, 0.1, 0.06, 0.04)
P6 = np.array([0.4, 0.25, 0.15, 0.1, 0.06, 0.04])
Z6 = np.log(P6).astype(np.float32)


def _kept(z, **kw):
    r = TM.truncate_row(z, **kw)
    return sorted(np.nonzero(r["kept"])[0].tolist()), r


# ---------------------------------------------------------------------------------------------------------------- the model, by hand
def test_six_labels_top_k():
    assert _kept(Z6, top_k=3)[0] == [0, 1, 2]
    assert _kept(Z6[::-1].copy(), top_k=2)[0] == [4, 5]
    assert not _kept(Z6, top_k=3)[1]["band"].any()


def test_six_labels_top_p():
    # cumulative mass 0.4, 0.65, 0.8, 0.9: the first value whose mass reaches 0.7 is the third
    assert _kept(Z6, top_p=0.7)[0] == [0, 1, 2]
    assert _kept(Z6, top_p=0.3)[0] == [0]
    assert _kept(Z6, top_p=0.95)[0] == [0, 1, 2, 3, 4]
    k, r = _kept(Z6, top_k=3, top_p=0.7)  # p renormalised over the three: 0.5, 0.3125, 0.1875 -> 0.5, 0.8125
    assert k == [0, 1] and abs(r["threshold"] - math.log(0.25)) < 1e-6


def test_six_labels_typical():
    H = -(P6 * np.log(P6)).sum()                      # 1.5396
    d = np.abs(-np.log(P6) - H)                       # 0.623, 0.153, 0.358, 0.763, 1.274, 1.679
    order = np.argsort(d)                             # 1, 2, 0, 3, 4, 5: masses 0.25, 0.40, 0.80, ...
    assert order.tolist() == [1, 2, 0, 3, 4, 5]
    k, r = _kept(Z6, typical_mass=0.2)
    assert k == [1] and abs(r["H"] - H) < 1e-6 and abs(r["threshold"] - d[1]) < 1e-6
    assert _kept(Z6, typical_mass=0.3)[0] == [1, 2]
    assert _kept(Z6, typical_mass=0.5)[0] == [0, 1, 2]
    assert _kept(Z6, typical_mass=0.85)[0] == [0, 1, 2, 3]
    # after top_k = 3 the probabilities are 0.5, 0.3125, 0.1875 with H = 1.0239: d = 0.331, 0.139, 0.650
    assert _kept(Z6, top_k=3, typical_mass=0.4)[0] == [0, 1]


def test_ties_at_the_threshold_are_all_kept():
    z = np.log(np.array([0.3, 0.2, 0.2, 0.2, 0.05, 0.05])).astype(np.float32)
    assert _kept(z, top_k=2)[0] == [0, 1, 2, 3]
    assert _kept(z, top_p=0.4)[0] == [0, 1, 2, 3]      # 0.3 < 0.4 <= 0.9: the whole tie group
    assert _kept(z, top_k=5)[0] == [0, 1, 2, 3, 4, 5]
    assert _kept(np.zeros(8, np.float32), typical_mass=0.1)[0] == list(range(8))   # all equal: d = 0 everywhere
    assert _kept(np.zeros(8, np.float32), top_p=0.1)[0] == list(range(8))
    z = np.float32([0.0, -0.0, -1.0, -2.0])            # -0 == +0
    assert _kept(z, top_k=1)[0] == [0, 1]


def test_min_tokens():
    assert _kept(Z6, top_p=0.3, min_tokens=3)[0] == [0, 1, 2]
    assert _kept(Z6, top_p=0.7, min_tokens=2)[0] == [0, 1, 2]                    # below the filter's own count: nothing changes
    assert _kept(Z6, typical_mass=0.2, min_tokens=3)[0] == [0, 1, 2]             # the three first in typical order: 1, 2, 0
    assert _kept(Z6, top_k=2, min_tokens=5)[0] == [0, 1]                          # no mass filter: ignored
    assert _kept(Z6, top_k=3, top_p=0.1, min_tokens=9)[0] == [0, 1, 2]            # more than A holds: A
    z = np.log(np.array([0.3, 0.2, 0.2, 0.2, 0.05, 0.05])).astype(np.float32)
    assert _kept(z, top_p=0.1, min_tokens=2)[0] == [0, 1, 2, 3]                   # ties at the n-th value


def test_off_values():
    everything = list(range(6))
    for kw in (dict(), dict(top_k=0), dict(top_k=-3), dict(top_k=6), dict(top_k=99), dict(top_p=1.0), dict(top_p=1.5), dict(typical_mass=1.0),
               dict(top_k=None, top_p=None, typical_mass=None), dict(top_p=1.0, typical_mass=1.0, min_tokens=4)):
        assert _kept(Z6, **kw)[0] == everything, kw
    assert _kept(Z6, top_p=1.0, typical_mass=0.2)[0] == [1]                          # an "off" mass combines with the other filter
    with pytest.raises(ValueError):
        TM.truncate_row(Z6, top_p=0.5, typical_mass=0.5)


def test_minus_infinity_labels_and_non_finite_rows():
    z = Z6.copy()
    z[[1, 4]] = -np.inf                                  # p = 0.4, 0.15, 0.1, 0.04 over 0.69
    assert _kept(z, top_p=0.5)[0] == [0]
    assert _kept(z, top_p=0.99)[0] == [0, 2, 3, 5]       # a label of probability 0 is never needed
    assert _kept(z, top_k=5)[0] == [0, 1, 2, 3, 4, 5]    # ... but it ties at the k-th value
    k, r = _kept(z, typical_mass=0.99)
    assert k == [0, 2, 3, 5] and np.isfinite(r["H"])     # p log p = 0 for the two
    for bad in (np.float32([0.0, np.nan, 1.0, 2.0]), np.full(4, -np.inf, np.float32), np.float32([0.0, np.inf, 1.0, 2.0])):
        k, r = _kept(bad, top_k=1, top_p=0.1)
        assert k == [0, 1, 2, 3] and not r["filtered"] and not r["band"].any()


def test_unreachable_mass_keeps_a():
    P = float(np.nextafter(1.0, 0.0))
    p = np.full(7, 1.0 / 7.0)
    assert p.sum() < P                                   # seven equal labels: their fp64 masses sum to 1 - 2^-52 < P, the target is never reached
    k, r = _kept(np.zeros(7, np.float32), top_p=P)
    assert k == list(range(7))
    z = np.concatenate([np.zeros(7), [-1.0, -2.0]]).astype(np.float32)
    assert _kept(z, top_k=7, typical_mass=P)[0] == list(range(7))


def test_band_flags_a_cut_inside_the_kernel_error():
    # two labels whose cumulative mass reaches the target within eps_mass: the model cannot promise the kernel's side
    z = np.log(np.array([0.5, 0.25, 0.25])).astype(np.float32)
    assert TM.truncate_row(z, top_p=0.5)["band"].any()
    assert not TM.truncate_row(z, top_p=0.4)["band"].any()
    # typical: labels 1 and 2 are one ulp apart, their distances differ by less than the kernel's error in H, and the cut falls on one of them
    z = np.float32([0.0, -1.0, np.nextafter(np.float32(-1.0), np.float32(-2.0)), -3.0])
    assert TM.truncate_row(z, typical_mass=0.95)["band"].any()
    assert not TM.truncate_row(np.float32([0.0, -1.0, -1.0, -3.0]), typical_mass=0.95)["band"].any()   # equal z: equal keys in the kernel too


def test_derived_bounds_at_8192():
    assert TM.gamma(8192) == (32 - 1 + 10) * 2.0 ** -24
    assert TM.delta_e(0.0) == 2 * TM.U and TM.delta_e(-10.0) == 32 * TM.U


@pytest.mark.parametrize("L", TM.GPU_SHAPES)
@pytest.mark.parametrize("name", sorted(TM.GPU_FILTERS))
def test_input_selection_rejects_at_most_half(L, name):
    for with_u in (False, True):
        lc, lu, cfg, omc, T, kept, rejected = TM.select_rows(L, name, with_u, 48)
        assert rejected <= 0.5, "L=%d %s: %.0f%% of the candidate rows have a non-empty band" % (L, name, 100 * rejected)
        assert lc.shape[0] == 48 and kept.shape == (48, L)


# ---------------------------------------------------------------------------------------------------------------- host validation
def test_check_filter():
    assert sampling.check_filter() == sampling.FILTER_OFF == (0, 1.0, 1.0, 1)
    assert sampling.check_filter(5, 0.9, None, 2) == (5, 0.9, 1.0, 2)
    assert sampling.check_filter(None, 1.0, 0.2) == (0, 1.0, 0.2, 1)
    assert not sampling.filter_on(sampling.check_filter(0, 1.0, 1.0, 7)) and sampling.filter_on(sampling.check_filter(typical_mass=0.2))
    for kw, word in [(dict(top_p=0.9, typical_mass=0.2), "mutually exclusive"), (dict(top_p=0.0), "top_p"), (dict(top_p=1.2), "top_p"), (dict(top_p=-0.1), "top_p"),
                     (dict(typical_mass=0.0), "typical_mass"), (dict(typical_mass=2), "typical_mass"), (dict(top_k=-1), "top_k"), (dict(top_k=2.5), "top_k"),
                     (dict(min_tokens=0), "min_tokens"), (dict(min_tokens=1.5), "min_tokens"), (dict(top_p=float("nan")), "top_p")]:
        with pytest.raises(ValueError, match=word):
            sampling.check_filter(**kw)


def test_request_filters():
    k, mass, on = sampling.request_filters(3, top_k=[0, 5, 0], typical_mass=[None, None, 0.2], min_tokens=2)
    assert k.tolist() == [[0, 2], [5, 2], [0, 2]] and k.dtype == torch.int32
    assert torch.equal(mass, torch.tensor([[1.0, 1.0], [1.0, 1.0], [1.0, 0.2]])) and on
    assert not sampling.request_filters(2)[2]
    with pytest.raises(ValueError, match="request 1.*mutually exclusive"):
        sampling.request_filters(2, top_p=[None, 0.5], typical_mass=0.3)
    with pytest.raises(ValueError, match="top_k must be one value or a list of 2"):
        sampling.request_filters(2, top_k=[1, 2, 3])


def test_calls_refuse_a_filter_before_touching_a_device():
    args = (object(), {}, (1, 8, 8))
    with pytest.raises(ValueError, match="typical_mass needs noise='philox'"):
        paella_amd.sample(*args, cfg=None, typical_mass=0.2)
    with pytest.raises(ValueError, match="top_k / top_p needs noise='philox'"):
        paella_amd.sample(*args, cfg=None, noise="torch", top_k=4, top_p=0.5)
    with pytest.raises(ValueError, match="top_p is not offered with a step temperature of 0"):
        paella_amd.sample(*args, cfg=None, noise="philox", temperature=(1.0, 0.0), top_p=0.5)
    with pytest.raises(ValueError, match="mutually exclusive"):
        paella_amd.sample(*args, cfg=None, noise="philox", top_p=0.5, typical_mass=0.5)
    with pytest.raises(ValueError, match="min_tokens"):
        paella_amd.sample(*args, cfg=None, noise="philox", min_tokens=0)
    with pytest.raises(ValueError, match="top_k"):
        paella_amd.sample_distributed(object(), {}, {"byt5": torch.zeros(1)}, (1, 8, 8), noise="philox", top_k=-2)
    with pytest.raises(ValueError, match="typical_mass needs noise='philox'"):
        paella_amd.sample_distributed(object(), {}, {"byt5": torch.zeros(1)}, (1, 8, 8), typical_mass=0.5)
    with pytest.raises(ValueError, match="request 0: top_p"):
        paella_amd.sample_requests(object(), {}, None, (1, 8, 8), [1], cfg=None, top_p=3.0)


def test_stream_and_graph_sampler_refuse_filters_they_were_not_built_for():
    """the check sits in front of any device work: exercised on instances that were never constructed"""
    st = object.__new__(paella_amd.RequestStream)
    st.shape, st.filtering, st.editing = (2, 8, 8), False, False
    with pytest.raises(ValueError, match="top_k needs a stream built with filtering=True"):
        st.admit({}, top_k=5)
    with pytest.raises(ValueError, match="mutually exclusive"):
        st.admit({}, top_p=0.5, typical_mass=0.5)
    gr = object.__new__(paella_amd.GraphRequestSampler)
    gr.shape, gr.kw, gr.req_defaults, gr.filt = (1, 8, 8), dict(steps=2), dict(cfg=None, temperature=(1.0, 0.5)), None
    with pytest.raises(ValueError, match="typical_mass per replay needs a sampler built with filtering=True"):
        gr([1], typical_mass=0.3)


# ---------------------------------------------------------------------------------------------------------------- the C ABI, without a GPU
def test_filter_argument_validation_without_gpu(built_lib):
    """every refusal below returns before any HIP call: the pointers are host arrays that are never dereferenced"""
    L, rows = 16, 4
    buf = (ctypes.c_float * (rows * L))()
    out = (ctypes.c_int64 * rows)()
    tab = (ctypes.c_int32 * 8)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)

    def scalar(L=L, mode=0, temperature=1.0, top_k=0, top_p=1.0, typical=1.0, min_tokens=1, keep=None, known=None):
        return built_lib.paella_sample_tail_filter(p(buf), None, rows, L, 1.0, 0.0, temperature, mode, 1, None, 0, 0, None, None, 0.0, keep, known, top_k, top_p, typical,
                                                   min_tokens, p(out), None, None)

    for kw, word in [(dict(top_p=0.5, typical=0.5), b"mutually exclusive"), (dict(top_p=0.0), b"top_p"), (dict(top_p=1.5), b"top_p"), (dict(top_p=float("nan")), b"top_p"),
                     (dict(typical=-0.5), b"typical_mass"), (dict(min_tokens=0), b"min_tokens"), (dict(mode=1, top_k=3), b"argmax"), (dict(temperature=0.0), b"temperature"),
                     (dict(L=16388, top_k=3), b"16384"), (dict(L=18), b"% 4"), (dict(keep=p(out)), b"pin_keep and pin_tokens")]:
        assert scalar(**kw) == -1, kw
        assert word in built_lib.paella_last_error(), (kw, built_lib.paella_last_error())

    def stream(fk, fm, L=L, step=p(tab), init=p(out), rps=2):
        return built_lib.paella_sample_tail_stream_filter(p(buf), None, rows, L, None, p(buf), p(out), rps, step, p(buf), p(tab), init, None, None, None, fk, fm, p(out),
                                                          None, None)

    assert stream(p(tab), None) == -1 and b"filter_k and filter_mass" in built_lib.paella_last_error()
    assert stream(None, p(buf)) == -1 and b"filter_k and filter_mass" in built_lib.paella_last_error()
    assert stream(p(tab), p(buf), step=None) == -1 and b"required" in built_lib.paella_last_error()
    assert stream(p(tab), p(buf), init=None) == -1 and b"required" in built_lib.paella_last_error()
    assert stream(p(tab), p(buf), L=16388) == -1 and b"16384" in built_lib.paella_last_error()
    assert stream(p(tab), p(buf), rps=3) == -1 and b"rows_per_sample" in built_lib.paella_last_error()
    assert stream(p(tab), p(buf), rps=0) == -1
    assert stream(None, None, step=None) == -1 and b"sample_tail_stream:" in built_lib.paella_last_error()   # no tables: the entry point it extends answers
    hook = built_lib.paella_test_tail_filter_keep
    assert hook(p(buf), None, rows, L, 1.0, 0.0, 1.0, 0, 0.5, 0.5, 1, None, None, None, 0, None, None, p(out), None, None) == -1
    assert hook(p(buf), None, rows, L, 1.0, 0.0, 1.0, 0, 1.0, 1.0, 1, None, None, None, 2, None, None, p(out), None, None) == -1

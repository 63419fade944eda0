"""CPU: the host side of a request batch (paella_amd.sample_requests / GraphRequestSampler): the table builder, the keying contract stated with
tests/counter_noise.py (request b draws what `sample(latent_shape=(1, H, W), seed=seeds[b])` draws: row_offset 0, its own seed), argument errors."""
import numpy as np
import pytest
import torch

import paella_amd
from paella_amd import sampling
from tests import counter_noise as C

SEED_HI = 0xC3A5C85C97CB3127  # bit 63 set


def _bits(t):
    return t.numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint64)


def test_tables_equal_the_scalar_samplers_values_bit_for_bit():
    steps, B = 5, 3
    seeds = [7, SEED_HI, (1 << 64) - 1]
    cfgs = [3.0, 7.5, (9.0, 5.0)]
    temps = [(1.0, 0.2), (0.7, 0.3), (0.05, 1.3)]
    seed_t, temp_t, pair_t = sampling.request_tables(B, steps, seeds, cfgs, temps)
    assert seed_t.dtype == torch.int64 and temp_t.shape == (steps, B) and pair_t.shape == (steps, B, 2)
    assert [int(v) & C.M64 for v in seed_t] == seeds and [int(v) for v in seed_t] == [sampling.seed_word(s) for s in seeds]
    f32 = lambda v: np.array([v], dtype=np.float32).view(np.uint32)[0]
    for b in range(B):
        want_t = sampling.linspace_schedule(temps[b][0], temps[b][1], steps)  # what sample() / sample_distributed pass per step
        assert [_bits(temp_t)[i, b] for i in range(steps)] == [f32(v) for v in want_t]
        if isinstance(cfgs[b], tuple):  # sample_distributed: linspace, 1 - cfg in fp32
            sched = torch.linspace(cfgs[b][0], cfgs[b][1], steps)
            want = [(float(sched[i]), float(1 - sched[i])) for i in range(steps)]
        else:                           # sample(): fp32(cfg), fp32(1.0 - cfg)
            want = [(float(torch.tensor(float(cfgs[b]), dtype=torch.float32)), float(torch.tensor(1.0 - float(cfgs[b]), dtype=torch.float32)))] * steps
        for i in range(steps):
            assert (_bits(pair_t)[i, b, 0], _bits(pair_t)[i, b, 1]) == (f32(want[i][0]), f32(want[i][1]))
    # one value for all requests; cfg=None gives no pair table
    s2, t2, p2 = sampling.request_tables(2, steps, [1, 2], 8.0, (1.0, 0.2))
    assert torch.equal(t2[:, 0], t2[:, 1]) and torch.equal(p2[:, 0], p2[:, 1]) and p2[0, 0].tolist() == [8.0, -7.0]
    assert sampling.request_tables(2, steps, [1, 2], None, (1.0, 0.2))[2] is None
    # B == 2 stays unambiguous: a pair of pairs is per request, a pair of numbers is one range
    t3 = sampling.request_tables(2, steps, [1, 2], None, [(1.0, 0.2), (0.5, 0.4)])[1]
    assert t3[0].tolist() == [1.0, 0.5]


def _request_streams(seeds, H, W, L, steps, renoise_steps):
    """every (key, ctr_lo, ctr_hi) a request batch draws: request b is one single-sample run under its own seed, row offset 0"""
    runs = [C.sample_run_streams(s, 1, H, W, L, steps, renoise_steps) for s in seeds]
    return [np.concatenate([r["start"], r["categorical"], r["renoise"]]) for r in runs]


def test_no_counter_is_drawn_twice_and_equal_seeds_draw_equal_words():
    H, W, L, steps = 4, 6, 1028, 6
    seeds = [11, 12, SEED_HI, SEED_HI + 1, (1 << 64) - 1]
    per = _request_streams(seeds, H, W, L, steps, steps - 1)
    allw = np.ascontiguousarray(np.concatenate(per)).view([("k", np.uint64), ("lo", np.uint64), ("hi", np.uint64)]).reshape(-1)
    assert np.unique(allw).size == allw.size, "a (key, counter) pair is drawn twice inside one request batch"
    # no global row, no slot: the counters of every request are the same set, only the keys differ
    assert all(np.array_equal(p[:, 1:], per[0][:, 1:]) for p in per)
    # The keying is the single call's, so it inherits its one caveat: the three streams of a request are told apart by XOR-ing a salt into the key, and two
    # seeds that differ by exactly such a salt share a key across streams (as two separate sample() calls with those seeds already do).  Stated, not hidden:
    ka, kb = _request_streams([SEED_HI, SEED_HI ^ C.RENOISE_SALT], H, W, L, 2, 1)
    assert int(kb[H * W, 0]) == C.renoise_key(SEED_HI) == int(ka[-1, 0])
    # documented: equal seeds -> identical words (start tokens, categorical words, renoise mask)
    assert np.array_equal(C.start_tokens(SEED_HI, H * W, L), C.start_tokens(SEED_HI, H * W, L, row_offset=0))
    a, b = _request_streams([SEED_HI, SEED_HI], H, W, L, 2, 1)
    assert np.array_equal(a, b)
    assert np.array_equal(C.categorical_words(SEED_HI, H * W, L, 3), C.categorical_words(SEED_HI, H * W, L, 3, row_offset=0))


@pytest.mark.parametrize("kw,exc", [
    (dict(seeds=[1, 2]), ValueError),                                        # wrong number of seeds
    (dict(seeds=5), ValueError),
    (dict(temperature=[(1.0, 0.2)] * 2), ValueError),                        # wrong number of temperature ranges
    (dict(temperature=(1.0, 0.0)), ValueError),                              # reaches temperature 0
    (dict(temperature=[(1.0, 0.2), (0.5, -0.1), (1.0, 0.2)]), ValueError),
    (dict(temperature=1.0), ValueError),
    (dict(cfg=[8.0, 3.0]), ValueError),                                      # wrong number of guidance entries
    (dict(cfg=[8.0, None, 3.0]), ValueError),                                # mixed cfg=None
    (dict(cfg=(9.0, 5.0)), TypeError),                                       # a bare tuple is ambiguous
    (dict(cfg=[8.0, "x", 3.0]), ValueError),
])
def test_argument_errors_raise_before_any_device_work(kw, exc):
    args = dict(seeds=[1, 2, 3], cfg=8.0, temperature=(1.0, 0.2))
    args.update(kw)
    with pytest.raises(exc):
        sampling.request_tables(3, 4, args["seeds"], args["cfg"], args["temperature"])
    # the public entry point validates first: it raises the same error with a model that could not run and a device that does not exist
    with pytest.raises(exc):
        paella_amd.sample_requests(None, {}, {}, (3, 8, 8), args["seeds"], cfg=args["cfg"], temperature=args["temperature"], steps=4, renoise_steps=3, device="cuda:99")


def test_guidance_needs_unconditional_inputs_and_a_hip_device():
    with pytest.raises(TypeError, match="unconditional_inputs"):
        paella_amd.sample_requests(None, {}, None, (2, 8, 8), [1, 2], cfg=8.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        paella_amd.sample_requests(None, {}, {}, (2, 8, 8), [1, 2], device="cpu")
    assert "sample_requests" in paella_amd.__all__ and "GraphRequestSampler" in paella_amd.__all__

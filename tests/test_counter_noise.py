"""CPU: the numpy model of the counter-based noise (tests/counter_noise.py) -- Philox4x32-10 known answers, the vectorised
form against a scalar transcription, the uniform grids, and injectivity of the keying.  The GPU kernels are checked against the
same model in tests/test_gpu_counter_noise.py."""
import numpy as np
import pytest

from tests import counter_noise as C


def _words(ctr, key):
    lo, hi = ctr[0] | ctr[1] << 32, ctr[2] | ctr[3] << 32
    return lo, hi, key[0] | key[1] << 32


# Random123's published known-answer vectors for Philox4x32-10 (counter c0..c3, key k0 k1 -> output words)
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    lo, hi, k = _words(ctr, key)
    assert tuple(int(v) for v in C.philox4x32(k, lo, hi)) == want
    assert C.philox4x32_scalar(k, lo, hi) == want


def test_vectorised_philox_equals_scalar_transcription():
    rng = np.random.default_rng(7)
    n = 4000
    keys = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    lo = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    hi = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    hi[:8] = np.uint64(C.M64)
    lo[8:16] = np.uint64(C.M64)
    got = np.stack(C.philox4x32(keys, lo, hi), 1)
    for i in range(n):
        assert tuple(int(v) for v in got[i]) == C.philox4x32_scalar(int(keys[i]), int(lo[i]), int(hi[i])), i


def test_uniform_grids():
    w = np.array([0, 1, 511, 512, 2 ** 31, 2 ** 32 - 513, 2 ** 32 - 512, 2 ** 32 - 1], dtype=np.uint64)
    u = C.u01_open(w)
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24
    assert (u > 0).all() and (u < 1).all()
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u), "u01_open must be exact in fp32"
    lq = C.log_exp1(w)
    assert np.isfinite(lq).all()
    # the end points: u = 2^-24 -> log(24 ln 2) = 2.8115, u = 1 - 2^-24 -> log(2^-24) + O(2^-25) = -16.6355
    assert abs(lq[0] - np.log(24 * np.log(2.0))) < 1e-12 and abs(lq[-1] - (-24 * np.log(2.0) + 2.0 ** -25)) < 1e-12
    h = C.u01_half_open(w)
    assert h.min() == 0.0 and h.max() == 1.0 - 2.0 ** -24 and (h < 1).all()
    assert np.array_equal(h.astype(np.float32).astype(np.float64), h)
    # the grids are uniform: every 2^-23 (open) / 2^-24 (half open) step is taken by exactly 2^9 / 2^8 words
    ws = np.arange(0, 2 ** 12, dtype=np.uint64)
    assert np.array_equal(np.unique(C.u01_open(ws), return_counts=True)[1], np.full(8, 512))
    assert np.array_equal(np.unique(C.u01_half_open(ws), return_counts=True)[1], np.full(16, 256))


def test_gumbel_bound_is_stated_in_ulps():
    assert C.gumbel_bound(np.array([16.0]))[0] == C.GUMBEL_ULPS * 2.0 ** -19 + C.GUMBEL_ABS
    assert C.gumbel_bound(np.array([0.0]))[0] >= C.GUMBEL_ABS
    assert C.ulp32(np.array([1.0]))[0] == 2.0 ** -23


def test_mix_is_two_roundings_without_fma():
    lc = np.array([1.0000001, 3.3, -2.7], dtype=np.float32)
    lu = np.array([0.9999999, 3.1, -2.9], dtype=np.float32)
    got = C.mix_logits(lc, lu, 8.0, -7.0)
    want = np.array([np.float32(np.float32(a * np.float32(8.0)) + np.float32(b * np.float32(-7.0))) for a, b in zip(lc, lu)])
    assert np.array_equal(got, want) and got.dtype == np.float32
    assert C.inv_temperature(0.2) == np.float32(1.0) / np.float32(0.2)


def test_first_index_wins_ties():
    s = np.array([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0]])
    idx, margin = C.top2_margin(s)
    assert idx.tolist() == [1, 0] and margin.tolist() == [0.0, 0.0]


def test_tail_model_small_case_by_hand():
    """One row worked through the scalar transcription: the chunked, vectorised tail model must reproduce it."""
    L, seed, step, row_off = 12, 0xDEADBEEF12345678, 3, (1 << 32) // 3 + 5
    rng = np.random.default_rng(1)
    lc = rng.standard_normal((5, L)).astype(np.float32)
    lu = rng.standard_normal((5, L)).astype(np.float32)
    init = np.arange(5) + 100
    pre, final, margin = C.sample_tail(lc, 0.7, seed, step, lu=lu, cfg=8.0, omc=-7.0, row_offset=row_off, init_noise=init, t_next=0.5, chunk_rows=2)
    inv_t = np.float32(1.0) / np.float32(0.7)
    for r in range(5):
        scores = []
        for q in range(L // 4):
            w = C.philox4x32_scalar(seed, (r + row_off) * (L // 4) + q, step)
            for e in range(4):
                i = 4 * q + e
                mix = np.float32(np.float32(lc[r, i] * np.float32(8.0)) + np.float32(lu[r, i] * np.float32(-7.0)))
                u = ((w[e] >> 9) + 0.5) / 2 ** 23
                scores.append(float(mix) * float(inv_t) - np.log(-np.log(u)))  # one rounding on the device: model exact
        best = int(np.argmax(scores))
        assert pre[r] == best
        assert abs(margin[r] - (sorted(scores)[-1] - sorted(scores)[-2])) < 1e-12
        w0 = C.philox4x32_scalar(seed ^ C.RENOISE_SALT, r + row_off, step)[0]
        assert final[r] == (init[r] if (w0 >> 8) / 2 ** 24 <= 0.5 else best)


def test_start_tokens_and_add_noise_by_hand():
    seed, L, off = (1 << 63) | 12345, 1000, (1 << 33) + 7
    tok = C.start_tokens(seed, 6, L, row_offset=off)
    for i in range(6):
        w = C.philox4x32_scalar(seed ^ C.START_SALT, i + off, C.M64)
        assert tok[i] == ((w[0] << 32) | w[1]) % L
    rx = C.random_x_tokens(C.M64 - 3, 4, L)
    assert np.array_equal(rx, C.start_tokens((C.M64 - 3 + C.RANDOM_X_SALT) & C.M64, 4, L))
    x = np.arange(8).reshape(2, 4)
    xo, m = C.add_noise_philox(x, np.array([0.3, 0.9], dtype=np.float32), 99, 4, L)
    for i in range(8):
        w = C.philox4x32_scalar(99, i, 4)
        mi = int((w[0] >> 8) / 2 ** 24 <= float(np.float32([0.3, 0.9][i // 4])))
        assert m.reshape(-1)[i] == mi and xo.reshape(-1)[i] == (((w[1] << 32) | w[2]) % L if mi else i)


def test_seed_and_row_words_add_with_wraparound():
    # key = seed + word mod 2^64: a device-resident word that wraps the seed gives the stream of the wrapped seed
    a = C.categorical_words(C.M64 - 2, 3, 8, 1, seed_word=5)
    b = C.categorical_words(2, 3, 8, 1)
    assert np.array_equal(a, b)
    assert np.array_equal(C.start_tokens(C.M64, 10, 77, seed_word=1), C.start_tokens(0, 10, 77))
    assert np.array_equal(C.renoise_mask(C.M64 - 1, 16, 2, 0.5, seed_word=3), C.renoise_mask(1, 16, 2, 0.5))
    # row_offset + row_offset_word = the global row
    assert np.array_equal(C.categorical_words(9, 4, 16, 0, row_offset=10, row_offset_word=20), C.categorical_words(9, 34, 16, 0)[30:])


def _assert_unique(rows, what):
    v = np.ascontiguousarray(rows).view([("k", np.uint64), ("lo", np.uint64), ("hi", np.uint64)]).reshape(-1)
    n_unique = np.unique(v).size
    assert n_unique == v.size, "%s: %d of %d (key, counter) triples collide" % (what, v.size - n_unique, v.size)


@pytest.mark.parametrize("L", [8192, 1028, 4])
def test_keying_is_injective_within_one_call(L):
    """One tail call: no two (row, label quad) pairs share a counter -- rows whose (row * L/4) passes 2^32 included."""
    L4 = L // 4
    rows = 64
    row_off = (1 << 32) // L4 - rows // 2  # the block straddles the 2^32 boundary of the low counter word
    ctr = C.categorical_counters(rows, L, row_off)
    assert int(ctr.min()) < 2 ** 32 <= int(ctr.max())
    assert np.unique(ctr).size == ctr.size
    # and the counter is the global one: the same positions drawn as two shards use the same counters
    assert np.array_equal(np.concatenate([C.categorical_counters(10, L, row_off), C.categorical_counters(rows - 10, L, row_off + 10)]), ctr)


@pytest.mark.parametrize("seed,seed_word,shard", [(5, 0, None), ((1 << 63) | 0xABCDEF, 0, (3, 8)), (C.M64 - 1, 9, (1, 4))])
def test_keying_is_injective_within_one_sample_run(seed, seed_word, shard):
    """One sample() call: start tokens, every step's categorical draws and every renoise draw use distinct (key, counter) pairs,
    across streams and steps; with a large row offset the categorical counters pass 2^32."""
    B, H, W, L, steps = 2, 4, 4, 1028, 12
    st = C.sample_run_streams(seed, B, H, W, L, steps, steps - 1, shard=shard, seed_word=seed_word)
    allw = np.concatenate([st["start"], st["categorical"], st["renoise"]])
    _assert_unique(allw, "sample run")
    assert len({int(k) for k in allw[:, 0]}) == 3, "three streams, three keys"
    # rows past 2^32 / (L/4) through the row-offset word of a shard
    st = C.sample_run_streams(seed, B, H, W, L, 3, 2, shard=shard, seed_word=seed_word, row_offset_word=(1 << 32) // (L // 4) - 8)
    assert int(st["categorical"][:, 1].max()) >= 2 ** 32
    _assert_unique(np.concatenate([st["start"], st["categorical"], st["renoise"]]), "sample run past 2^32")


def test_sample_run_keys_follow_the_seed_and_shards_tile_the_batch():
    """Two seeds never share a (key, counter) pair by construction of the key; the shards of one batch draw disjoint counters whose
    union is the unsharded call's."""
    B, H, W, L = 4, 2, 2, 8
    full = C.sample_run_streams(77, B, H, W, L, 2, 1)
    parts = [C.sample_run_streams(77, 1, H, W, L, 2, 1, shard=(lo, B)) for lo in range(B)]
    for name in ("start", "categorical", "renoise"):
        cat = np.concatenate([p[name] for p in parts])
        a = np.ascontiguousarray(cat).view([("k", np.uint64), ("lo", np.uint64), ("hi", np.uint64)]).reshape(-1)
        b = np.ascontiguousarray(full[name]).view([("k", np.uint64), ("lo", np.uint64), ("hi", np.uint64)]).reshape(-1)
        assert np.array_equal(np.sort(a), np.sort(b)), name


def test_seed_words_keep_the_bit_pattern():
    """Device-resident seed words are int64 tensors the kernels read as uint64: a seed with bit 63 set must fit and keep its bits
    (GraphSampler's seed word, the seed packed into the conditioning broadcast)."""
    import torch
    from paella_amd import dist, sampling
    for seed in (0, 5, (1 << 63) - 1, 1 << 63, 0xC3A5C85C97CB3127, C.M64):
        w = sampling.seed_word(seed)
        t = torch.tensor([w], dtype=torch.int64)
        assert int(t.numpy().view(np.uint64)[0]) == seed
        packed = dist._pack_seed(seed, "cpu")
        assert packed.dtype == torch.float32 and int(packed.view(torch.int64).numpy().view(np.uint64)[0]) == seed

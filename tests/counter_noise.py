"""CPU model of the counter-based noise (`noise="philox"`), written independently of the kernels (paella_amd/csrc/philox.h,
tail.hip, the head GEMM's fused tail epilogue in gemm.hip) and of paella_amd: plain numpy, vectorised over uint64.

The contract it states:
  * Philox4x32-10: round (c0, c1, c2, c3) -> (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)),
    M0 = 0xD2511F53, M1 = 0xCD9E8D57; the key advances by the Weyl constants (0x9E3779B9, 0xBB67AE85) after every round.
    key = (lo, hi) 32-bit halves of a 64-bit seed; counter = the 64-bit words (ctr_lo, ctr_hi) split the same way.
  * u01_open(w) = ((w >> 9) + 1/2) * 2^-23 in (0, 1); u01_half_open(w) = (w >> 8) * 2^-24 in [0, 1).
  * categorical draw (Gumbel-max): score_i = mix_i * fp32(1/T) - log(-log u01_open(w_i)), token = first argmax; the kernels round
    the score ONCE (an fma of the fp32 log), so the model keeps the product exact (fp64) and the logarithms in fp64;
    mix = fp32(fp32(lc * cfg) + fp32(lu * omc)) (two roundings, no FMA) with guidance, lc without.
    key seed + seed_word (mod 2^64); counter ((row + row_offset + row_offset_word) * (L/4) + label/4, step); word e -> label 4q + e.
  * renoise: key seed' ^ RENOISE_SALT, counter (global row, step); replaced by init_noise[row] where u01_half_open(w0) <= t_next.
  * start tokens: key seed' ^ START_SALT, counter (i + row_offset', 2^64 - 1); token ((w0 << 32) | w1) mod L.
    Inpainting's random_x: the start tokens of seed (seed + RANDOM_X_SALT) mod 2^64.
  * paella_add_noise's Philox branch (C ABI only): key seed, counter (i, offset); mask u01_half_open(w0) <= t[b],
    random_x ((w1 << 32) | w2) mod L.
  * the sampler: step i draws with step offset i; a batch shard (lo, total) uses row offset lo * H * W.
The device's log(-log u) is an fp32 approximation of the fp64 value computed here: the tests bound that difference
(GUMBEL_ULPS / GUMBEL_ABS below), and a device score may differ from the model's by that bound plus half an ulp of the score;
everything else in the stream is integer or exact and is compared bit for bit."""
import numpy as np

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
RENOISE_SALT = 0x5BD1E9955BD1E995
START_SALT = 0x9E3779B97F4A7C15
RANDOM_X_SALT = 0x5851F42D4C957F2D
START_CTR_HI = M64

# Bound of |device log(-log u) - fp64 log(-log u)|: GUMBEL_ULPS fp32 ulps of |log E| plus GUMBEL_ABS.  Each logarithm lowers to
# v_log_f32 (log2, a denormal rescale) and a two-part ln 2 product, i.e. log2 within ~1 ulp, then ~0.5 ulp for the product:
# <= 2 ulp per logarithm.  The inner one, -log u, is then off by <= 2 * 2^-23 RELATIVELY (one fp32 ulp is <= 2^-23 of the value),
# which the outer logarithm turns into an ABSOLUTE error of the same size; the outer one adds its own <= 2 ulp of |log E|.
# Measured on MI355X over 2^27 draws covering both ends of the u grid: worst error / bound 0.89 (u = 0.99758, log E = -6.024, error
# 1.06e-6); worst absolute error 1.88e-6 at u = 0.9999878 (log E = -11.31, 2 ulp), no larger toward u -> 1 than elsewhere.
GUMBEL_ULPS = 2.0
GUMBEL_ABS = 2.0 * 2.0 ** -23

_U64 = np.uint64


def ulp32(x):
    """fp32 ulp of |x| (the spacing above |x|; 2^-149 for 0 and subnormals)."""
    a = np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def gumbel_bound(log_e):
    """The stated bound on |device log_exp1 - fp64 log(-log u)| at fp64 value log_e."""
    return GUMBEL_ULPS * ulp32(log_e) + GUMBEL_ABS


# ------------------------------------------------------------------------------------------------------------------ Philox
def philox4x32(key, ctr_lo, ctr_hi):
    """Philox4x32-10; key, ctr_lo, ctr_hi: 64-bit words (python ints or uint64 arrays, broadcast).  Returns four uint64 arrays
    holding the 32-bit output words."""
    key, ctr_lo, ctr_hi = (np.asarray(v, dtype=np.uint64) if not isinstance(v, int) else np.uint64(v & M64) for v in (key, ctr_lo, ctr_hi))
    m32, s32 = _U64(M32), _U64(32)
    c0, c1 = ctr_lo & m32, ctr_lo >> s32
    c2, c3 = ctr_hi & m32, ctr_hi >> s32
    k0, k1 = key & m32, key >> s32
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    m0, m1, w0, w1 = _U64(PHILOX_M0), _U64(PHILOX_M1), _U64(PHILOX_W0), _U64(PHILOX_W1)
    for _ in range(10):
        p0 = m0 * c0
        p1 = m1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + w0) & m32
        k1 = (k1 + w1) & m32
    return c0, c1, c2, c3


def philox4x32_scalar(key, ctr_lo, ctr_hi):
    """The same function as plain python integers, one call at a time (the transcription the vectorised form is checked against)."""
    c = [ctr_lo & M32, (ctr_lo >> 32) & M32, ctr_hi & M32, (ctr_hi >> 32) & M32]
    k0, k1 = key & M32, (key >> 32) & M32
    for _ in range(10):
        p0 = PHILOX_M0 * c[0]
        p1 = PHILOX_M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + PHILOX_W0) & M32
        k1 = (k1 + PHILOX_W1) & M32
    return tuple(c)


# ------------------------------------------------------------------------------------------------------------------ transforms
def u01_open(w):
    """((w >> 9) + 1/2) * 2^-23: the 2^23-point grid strictly inside (0, 1) (exact in fp32 and fp64)."""
    return ((np.asarray(w, dtype=np.uint64) >> _U64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def u01_half_open(w):
    """(w >> 8) * 2^-24 in [0, 1) (exact in fp32 and fp64)."""
    return (np.asarray(w, dtype=np.uint64) >> _U64(8)).astype(np.float64) * 2.0 ** -24


def log_exp1(w):
    """fp64 log(-log u01_open(w)): the value the device's fp32 log_exp1 approximates.  -log u = -log1p(u - 1), u - 1 exact in fp64."""
    return np.log(-np.log1p(u01_open(w) - 1.0))


def mix_logits(lc, lu=None, cfg=1.0, omc=0.0):
    """fp32(fp32(lc * cfg) + fp32(lu * omc)) -- two roundings, never fused; lc alone without guidance."""
    lc = np.asarray(lc, dtype=np.float32)
    if lu is None:
        return lc
    return (lc * np.float32(cfg)) + (np.asarray(lu, dtype=np.float32) * np.float32(omc))


def inv_temperature(temperature):
    """fp32(1 / T), correctly rounded."""
    return np.float32(1.0) / np.float32(temperature)


def scaled_logits(mix, temperature):
    """mix * fp32(1/T), exact in fp64 (a product of two fp32 values): the logit part of the Gumbel score, which the kernels do not round
    on its own (tail_score_gumbel is one fma)."""
    return np.asarray(mix, dtype=np.float32).astype(np.float64) * float(inv_temperature(temperature))


# ------------------------------------------------------------------------------------------------------------------ keying
def categorical_key(seed, seed_word=0):
    return (int(seed) + int(seed_word)) & M64


def renoise_key(seed, seed_word=0):
    return categorical_key(seed, seed_word) ^ RENOISE_SALT


def start_key(seed, seed_word=0):
    return categorical_key(seed, seed_word) ^ START_SALT


def categorical_counters(rows, L, row_offset=0, row_offset_word=0):
    """[rows, L/4] uint64 low counter words ((row + row_offset + row_offset_word) * L/4 + quad) mod 2^64; rows: int or array of row indices."""
    L4 = L // 4
    r = np.arange(rows, dtype=np.uint64) if isinstance(rows, (int, np.integer)) else np.asarray(rows, dtype=np.uint64)
    g = r + _U64((int(row_offset) + int(row_offset_word)) & M64)
    return g[:, None] * _U64(L4) + np.arange(L4, dtype=np.uint64)[None, :]


def sample_run_streams(seed, B, H, W, L, steps, renoise_steps, shard=None, seed_word=0, row_offset_word=0):
    """Every (stream, key, ctr_lo, ctr_hi) one sample(noise="philox") call draws, as uint64 arrays [n, 3] per stream:
    the start tokens, per step the categorical draw of every (row, label quad) and, for renoised steps, the renoise word."""
    lo = 0 if shard is None else int(shard[0])
    row_off = lo * H * W
    rows = B * H * W
    g = np.arange(rows, dtype=np.uint64) + _U64((row_off + int(row_offset_word)) & M64)
    out = {"start": np.stack([np.full(rows, start_key(seed, seed_word), dtype=np.uint64), g, np.full(rows, START_CTR_HI, dtype=np.uint64)], 1)}
    cat, ren = [], []
    for i in range(steps):
        c = categorical_counters(rows, L, row_off, row_offset_word).reshape(-1)
        cat.append(np.stack([np.full(c.size, categorical_key(seed, seed_word), dtype=np.uint64), c, np.full(c.size, i, dtype=np.uint64)], 1))
        if i < renoise_steps:
            ren.append(np.stack([np.full(rows, renoise_key(seed, seed_word), dtype=np.uint64), g, np.full(rows, i, dtype=np.uint64)], 1))
    out["categorical"] = np.concatenate(cat)
    out["renoise"] = np.concatenate(ren) if ren else np.zeros((0, 3), dtype=np.uint64)
    return out


# ------------------------------------------------------------------------------------------------------------------ draws
def categorical_words(seed, rows, L, step, row_offset=0, seed_word=0, row_offset_word=0):
    """[rows, L] uint64: the Philox word of every (row, label) -- word e of quad q belongs to label 4q + e."""
    ctr = categorical_counters(rows, L, row_offset, row_offset_word)
    w = philox4x32(categorical_key(seed, seed_word), ctr, int(step))
    return np.stack(w, axis=-1).reshape(ctr.shape[0], L)


def gumbel_scores(mix, temperature, words):
    """fp64 Gumbel-max scores mix * fp32(1/T) - log(-log u) of [rows, L] mixed logits and their Philox words."""
    return scaled_logits(mix, temperature) - log_exp1(words)


def top2_margin(scores):
    """(first argmax, top-1 minus top-2) per row of an fp64 score matrix."""
    idx = np.argmax(scores, axis=1)
    part = np.partition(scores, scores.shape[1] - 2, axis=1)[:, -2:] if scores.shape[1] > 1 else np.concatenate([scores, np.full_like(scores, -np.inf)], 1)
    return idx, part[:, 1] - part[:, 0]


def renoise_mask(seed, rows, step, t_next, row_offset=0, seed_word=0, row_offset_word=0):
    """[rows] bool: u01_half_open(w0) <= t_next (t_next rounded to fp32, as the kernels receive it)."""
    g = np.arange(rows, dtype=np.uint64) + _U64((int(row_offset) + int(row_offset_word)) & M64)
    w0 = philox4x32(renoise_key(seed, seed_word), g, int(step))[0]
    return u01_half_open(w0) <= float(np.float32(t_next))


def start_tokens(seed, n, L, row_offset=0, seed_word=0, row_offset_word=0):
    """[n] int64 start tokens of the global positions row_offset + row_offset_word + [0, n)."""
    g = np.arange(n, dtype=np.uint64) + _U64((int(row_offset) + int(row_offset_word)) & M64)
    w = philox4x32(start_key(seed, seed_word), g, START_CTR_HI)
    return (((w[0] << _U64(32)) | w[1]) % _U64(L)).astype(np.int64)


def random_x_tokens(seed, n, L, row_offset=0, seed_word=0, row_offset_word=0):
    """Inpainting's random_x in the counter-based mode: the start tokens of the salted seed."""
    return start_tokens((int(seed) + RANDOM_X_SALT) & M64, n, L, row_offset, seed_word, row_offset_word)


def add_noise_philox(x, t, seed, offset, L):
    """paella_add_noise with neither mask, rand_u nor random_x given: x [B, ...] int64, t [B] fp32 -> (x_out, mask)."""
    x = np.asarray(x, dtype=np.int64)
    B = x.shape[0]
    per = x.size // B
    i = np.arange(x.size, dtype=np.uint64)
    w0, w1, w2, _ = philox4x32(int(seed), i, int(offset))
    tb = np.repeat(np.asarray(t, dtype=np.float32).astype(np.float64), per)
    m = (u01_half_open(w0) <= tb).astype(np.int64)
    rx = (((w1 << _U64(32)) | w2) % _U64(L)).astype(np.int64)
    flat = x.reshape(-1)
    return (flat * (1 - m) + rx * m).reshape(x.shape), m.reshape(x.shape)


def sample_tail(lc, temperature, seed, step, lu=None, cfg=1.0, omc=0.0, row_offset=0, seed_word=0, row_offset_word=0, init_noise=None,
                t_next=0.0, argmax=False, chunk_rows=256):
    """Reference of one tail step on [rows, L] logits: returns (pre-renoise tokens, final tokens, fp64 top-1 minus top-2 score margin).
    argmax=True: first argmax of the fp32 mix (margin in the same units).  Rows are processed in chunks to bound host memory."""
    lc = np.asarray(lc, dtype=np.float32)
    rows, L = lc.shape
    pre = np.empty(rows, dtype=np.int64)
    margin = np.empty(rows, dtype=np.float64)
    for a in range(0, rows, chunk_rows):
        b = min(rows, a + chunk_rows)
        mix = mix_logits(lc[a:b], None if lu is None else np.asarray(lu, dtype=np.float32)[a:b], cfg, omc)
        if argmax:
            s = mix.astype(np.float64)
        else:
            s = gumbel_scores(mix, temperature, categorical_words(seed, b - a, L, step, int(row_offset) + a, seed_word, row_offset_word))
        pre[a:b], margin[a:b] = top2_margin(s)
    final = pre.copy()
    if init_noise is not None:
        m = renoise_mask(seed, rows, step, t_next, row_offset, seed_word, row_offset_word)
        final[m] = np.asarray(init_noise, dtype=np.int64).reshape(-1)[m]
    return pre, final, margin

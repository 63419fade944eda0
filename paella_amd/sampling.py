"""Paella's iterative token-denoising sampler on MI355X.

Host mirror of the reference's two `sample()` functions:
  * `sample`             -- src/utils.py:35-55          (model, model_inputs, latent_shape, unconditional_inputs=None, ...)
  * `sample_distributed` -- src_distributed/utils.py:97-126 (model, model_inputs, unconditional_inputs, latent_shape, init_x=None, ...)
Both drive the same core loop.  The loop itself is host code (a dozen lines, as in the reference); everything
it calls is a HIP kernel: `Paella.prepare_cond` once per call (step-invariant conditioning work hoisted out of
the loop), `Paella.forward_prepared` per step with the conditional and unconditional rows batched into one
2B-row evaluation when their conditioning shapes agree (the reference runs two forwards, src/utils.py:44,46),
and one fused tail kernel per step for CFG mix -> temperature -> softmax -> categorical draw -> renoise.

Noise: with `noise="torch"` (default) the random numbers are drawn from torch's generator with the same calls in
the same order as the reference (randint for the start tokens; per step `exponential_` for the multinomial draw
-- torch.multinomial(p, 1) is argmax(p / Exp(1)) -- and `rand` for the renoise mask), so under the same seed the
result equals the reference's whenever the logits agree.  `noise="philox"` generates all per-step noise inside
the tail kernel (Philox4x32-10 keyed by `seed`), which removes the [B*H*W, num_labels] noise tensor.

Extension (not reference behaviour): a step temperature of 0 selects argmax of the mixed logits.
"""
import ctypes

import torch

from . import _lib
from ._graph import GraphOwner
from .modules import MAX_REGIONS, CondCache, KeyWeights, Paella, RegionTables, region_query_groups, region_query_total


def linspace_schedule(start, end, n):
    """torch.linspace(start, end, n) as python floats of the fp32 values (what the reference multiplies by)."""
    return [float(v) for v in torch.linspace(start, end, n)]


def _same_cond_layout(a, b):
    if a is None or b is None:
        return False
    for k in ("byt5", "clip", "clip_image"):
        va, vb = a.get(k), b.get(k)
        if (va is None) != (vb is None):
            return False
        if va is None:
            continue
        if isinstance(va, (list, tuple)) != isinstance(vb, (list, tuple)):
            return False
        if isinstance(va, (list, tuple)):
            if len(va) != len(vb) or any(x.shape != y.shape for x, y in zip(va, vb)):
                return False
        elif va.shape != vb.shape:
            return False
    return True


def _cond_batch(inputs):
    """samples in a conditioning dict (None when it has no tensor)"""
    for k in ("byt5", "clip", "clip_image"):
        v = inputs.get(k) if inputs is not None else None
        if isinstance(v, (list, tuple)):
            v = v[0] if v else None
        if v is not None:
            return int(v.size(0))
    return None


def _cond_seq_len(model, inputs):
    """Conditioning rows per sample: S_byt5 + clip_seq_len * [clip] + clip_seq_len * #clip_image (src/modules.py:223-232)."""
    if inputs is None:
        return 0
    n = model._cfg["clip_seq_len"]
    S = inputs["byt5"].size(1) if inputs.get("byt5") is not None else 0
    if inputs.get("clip") is not None:
        S += n
    ci = inputs.get("clip_image")
    if ci is not None:
        S += n * (len(ci) if isinstance(ci, (list, tuple)) else 1)
    return S


def ragged_slot_plan(S_c, S_u, B, row_bytes):
    """The ONE 2B-slot cache of a guided call whose conditional and unconditional sets have S_c and S_u conditioning rows: the slot pitch max(S_c, S_u), the row
    count of every slot (conditional group in slots [0, B), unconditional in [B, 2B)), the byte offset of each slot and of the two groups, and the cache size;
    row_bytes = bytes of one cache row (`Paella.cond_bytes(1, 1)`).  Pure host arithmetic."""
    S_c, S_u, B, row_bytes = int(S_c), int(S_u), int(B), int(row_bytes)
    if S_c <= 0 or S_u <= 0 or B <= 0:
        raise ValueError("a ragged cache needs B > 0 and at least one conditioning row on each side")
    pitch = max(S_c, S_u)
    slot_bytes = pitch * row_bytes
    return dict(pitch=pitch, lens=[S_c] * B + [S_u] * B, slot_bytes=slot_bytes, offsets=[b * slot_bytes for b in range(2 * B)],
                group_offsets=(0, B * slot_bytes), nbytes=2 * B * slot_bytes)


def _prepare_ragged_pair(model, model_inputs, unconditional_inputs, B, ws):
    """conditional and unconditional sets of different layouts as ONE ragged 2B-slot cache (`ragged_slot_plan`): each group is prepared straight into its slots
    at its own length, with the GEMM shapes of the plain `prepare_cond` call"""
    dev = model._device()
    plan = ragged_slot_plan(_cond_seq_len(model, model_inputs), _cond_seq_len(model, unconditional_inputs), B, model.cond_bytes(1, 1))
    buf = torch.empty(plan["nbytes"], dtype=torch.uint8, device=dev)
    lens = torch.empty(2 * B, dtype=torch.int32, device=dev)
    half = plan["group_offsets"][1]
    model.prepare_cond(**model_inputs, ws=ws, out=buf[:half], slot_rows=plan["pitch"], lens_out=lens[:B])
    model.prepare_cond(**unconditional_inputs, ws=ws, out=buf[half:], slot_rows=plan["pitch"], lens_out=lens[B:])
    return CondCache(buf, 2 * B, plan["pitch"], lens)


def _cat_inputs(a, b):
    out = {}
    for k in ("byt5", "clip", "clip_image"):
        va, vb = a.get(k), b.get(k)
        if va is None:
            out[k] = None
        elif isinstance(va, (list, tuple)):
            out[k] = [torch.cat([x, y], dim=0) for x, y in zip(va, vb)]
        else:
            out[k] = torch.cat([va, vb], dim=0)
    return out


def _run_tail(lc, lu, rows, L, out, *, scalar=None, req=None, stream=None, offset=0, init_noise=None, t_next=0.0, pin=None, filt=None, stats=None):
    """ONE sampling tail on materialised logits through its argument block (include/paella_hip.h: paella_tail_args); None = not given, and which tail runs follows
    from what is given.  scalar=(cfg, omc, temperature, mode, seed, seed_dev, row_offset, row_offset_dev, noise_q, mask_u) or req=(pairs, temps, seeds,
    rows_per_sample) DEVICE tables, with stream=(step, t_next, active) tables in place of `offset` / `t_next`; pin=(keep, known[, pin_on]);
    filt=(top_k, top_p, typical_mass, min_tokens) of `check_filter` next to `scalar`, the (filter_k, filter_mass) tables next to `req`; stats=(logprob, entropy)"""
    t = _lib.TailArgs(rows=rows, L=L, offset=offset, t_next=t_next)
    _lib.tensor_fields(t, logits_c=lc, logits_u=lu, init_noise=init_noise, tokens_out=out)
    if req is None:
        t.cfg, t.one_minus_cfg, t.temperature, t.mode, t.seed, seed_dev, t.row_offset, row_offset_dev, noise_q, mask_u = scalar
        _lib.tensor_fields(t, seed_ptr=seed_dev, row_offset_ptr=row_offset_dev, noise_q=noise_q, mask_u=mask_u)
        if filt is not None:
            t.top_k, t.top_p, t.typical_mass, t.min_tokens = filt
    else:
        _lib.tensor_fields(t, cfg_pairs=None if lu is None else req[0], temperature_tab=req[1], seeds=req[2]).rows_per_sample = req[3]
        if filt is not None:
            _lib.tensor_fields(t, filter_k=filt[0], filter_mass=filt[1])
    if stream is not None:
        _lib.tensor_fields(t, step=stream[0], t_next_tab=stream[1], active=stream[2])
    if pin is not None:
        _lib.tensor_fields(t, pin_keep=pin[0], pin_tokens=pin[1], pin_on=pin[2] if len(pin) > 2 else None)
    if stats is not None:
        _lib.tensor_fields(t, logprob_out=stats[0], entropy_out=stats[1])
    with torch.cuda.device(lc.device):
        _lib.check(_lib.load().paella_sample_tail_args(ctypes.byref(t), ctypes.sizeof(t), _lib.stream_ptr(lc.device)))


def _tail(logits_c, logits_u, rows, L, cfg, omc, temperature, mode, noise_q, seed, offset, init_noise, mask_u, t_next, out,
          seed_dev=None, row_offset=0, row_offset_dev=None, pin=None, filt=None):
    """the scalar form; pin=(keep, known): the tail writes known[row] wherever keep[row] == 0, after the draw and the renoise; filt: truncated sampling"""
    _run_tail(logits_c, logits_u, rows, L, out, scalar=(cfg, omc, temperature, mode, seed, seed_dev, row_offset, row_offset_dev, noise_q, mask_u), offset=offset,
              init_noise=init_noise, t_next=t_next, pin=pin, filt=filt)


def _tail_req(lc, lu, rows, L, rows_per_sample, req, step, init_noise, t_next, out, filt=None):
    """the request form of `_tail`: seed, guidance pair and temperature per sample from the device tables of `req` (RequestTables); filt (FilterTables): the
    filtered stream tail, fed with that step's constant step / renoise-threshold tables (the words the scalar arguments carry otherwise)"""
    tabs = (None if lu is None else req.pairs[step], req.temps[step], req.seeds, rows_per_sample)
    if filt is not None:
        _stream_draw(lc, lu, rows, L, out, tabs, filt.step[step], filt.t_next[step], filt.active, init_noise, (filt.k, filt.mass))
    else:
        _run_tail(lc, lu, rows, L, out, req=tabs, offset=step, init_noise=init_noise, t_next=t_next)


def _stream_draw(lc, lu, rows, L, out, req, step, t_next, active, init_noise, filt, pin=None, conf=None, renoise=True):
    """The tail sequences of the stream-table form, issued here for the request batch (`_sample_core`) and for the request stream's tick alike.  req=(pairs, temps,
    seeds, rows_per_sample), step / t_next / active and filt=(filter_k, filter_mass) are DEVICE tables, pin=(keep, known, pin_on).  conf=None: the filtered stream
    tail, the pin riding in it.  conf=(never, policy, noise, logprob, entropy): the statistics tail in the stream form, never renoising (threshold table `never` =
    -1) and unpinned, then -- unless renoise=False: a step of a request batch past its renoising ones -- the renoise stage with the real thresholds `t_next`,
    every sample by its own policy, which also applies the pin (`out` in place)."""
    if conf is None:
        _run_tail(lc, lu, rows, L, out, req=req, stream=(step, t_next, active), init_noise=init_noise, pin=pin, filt=filt)
        return
    never, policy, noise, logprob, entropy = conf
    _run_tail(lc, lu, rows, L, out, req=req, stream=(step, never, active), init_noise=init_noise, filt=filt, stats=(logprob, entropy))
    if renoise:
        pk, pt, po = (None, None, None) if pin is None else pin
        with torch.cuda.device(out.device):
            _lib.check(_lib.load().paella_renoise_select_stream(_lib.ptr(out), _lib.ptr(logprob), _lib.ptr(init_noise), rows, req[3], _lib.ptr(req[2]), _lib.ptr(step),
                                                                _lib.ptr(t_next), _lib.ptr(active), _lib.ptr(policy), _lib.ptr(noise), _lib.ptr(pk), _lib.ptr(pt),
                                                                _lib.ptr(po), _lib.ptr(out), _lib.stream_ptr(out.device)))


def fresh_seed():
    """A 62-bit seed drawn from torch's default (CPU) generator: reproducible under torch.manual_seed, different on every
    call otherwise -- what `seed=None` means in the counter-based (Philox) noise mode.  NOTE: this consumes one draw of torch's
    global CPU generator per call (the reference's sample() consumes the global DEVICE generator instead, src/utils.py:37)."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def seed_word(seed):
    """The int64 with the bit pattern of a 64-bit seed: what a device-resident seed word holds (the kernels read it as uint64), so seeds
    with bit 63 set fit an int64 tensor."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s - (1 << 64) if s >> 63 else s


def start_tokens(num_labels, shape, seed, device, shard=None, out=None, seed_dev=None, row_offset_dev=None):
    """The start tokens of the counter-based noise mode (the reference draws torch.randint on the global generator,
    src/utils.py:37 -- a stream that cannot be sharded): token i of the GLOBAL [total, H, W] grid is Philox(seed, i) mod
    num_labels (paella_start_tokens), so a batch shard draws exactly its rows of the unsharded draw at O(shard) cost.
    seed_dev / row_offset_dev: optional device-resident words added to seed / the row offset (a captured graph draws fresh
    tokens for any seed and shard without host work)."""
    B, H, W = shape
    lo = 0 if shard is None else int(shard[0])
    device = torch.device(device)
    if out is None:
        out = torch.empty(B, H, W, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().paella_start_tokens(int(seed), _lib.ptr(seed_dev), lo * H * W, _lib.ptr(row_offset_dev), int(num_labels),
                                                   B * H * W, _lib.ptr(out), _lib.stream_ptr(device)))
    return out


def start_tokens_requests(num_labels, shape, seeds_dev, out=None):
    """Start tokens of a request batch: sample b of [B, H, W] gets the start tokens `start_tokens(num_labels, (1, H, W), seeds[b])` draws; seeds_dev is the
    int64 DEVICE tensor [B] of seed bit patterns (paella_start_tokens_req: graph-capturable, no host work)."""
    B, H, W = shape
    device = seeds_dev.device
    if out is None:
        out = torch.empty(B, H, W, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().paella_start_tokens_req(_lib.ptr(seeds_dev), B, H * W, int(num_labels), _lib.ptr(out), _lib.stream_ptr(device)))
    return out


def _per_request(v, B, message, one=None, seq=(list, tuple)):
    """an argument that is one value for all requests or a sequence of B, as a list of B.  one(v): is v a single value (default: anything that is no `seq`);
    message(v): the caller's text for anything else"""
    if one(v) if one is not None else not isinstance(v, seq):
        return [v] * B
    if not isinstance(v, seq) or len(v) != B:
        raise ValueError(message(v))
    return list(v)


def _request_rows(B, check, **columns):
    """[check(request b's values) for every b], each keyword one value for all requests or a list of B; an error names the argument and the request"""
    cols = [_per_request(v, B, lambda v, name=name: "%s must be one value or a list of %d (one per request), got %d" % (name, B, len(v))) for name, v in columns.items()]
    rows = []
    for b, values in enumerate(zip(*cols)):
        try:
            rows.append(check(*values))
        except ValueError as e:
            raise ValueError("request %d: %s" % (b, e)) from None
    return rows


def request_tables(B, steps, seeds, cfg, temperature):
    """HOST tables of a request batch, validated before anything touches a device:
        seeds int64 [B] (bit patterns, `seed_word`), temps fp32 [steps, B], pairs fp32 [steps, B, 2] or None (cfg=None: no guidance for anyone).
    Row b holds, bit for bit, the scalars the scalar samplers compute for that request's values: temperatures `linspace_schedule(start, end, steps)`;
    a float guidance scale as `sample()` rounds it (fp32(cfg), fp32(1.0 - cfg), the same for every step), a (start, end) tuple as `sample_distributed`
    does (torch.linspace, 1 - cfg in fp32).  temperature: one (start, end) pair or a list of B pairs.  cfg: None, a float (all requests), or a LIST of B
    entries, each a float or a (start, end) tuple -- a bare tuple is refused (with B = 2 it could mean either).  Guidance is on for every request or for
    none: a request that wants none inside a guided batch passes 1.0, which mixes with (1, 0) -- exact while the unconditional activations are finite."""
    B, steps = int(B), int(steps)
    if B <= 0 or steps <= 0:
        raise ValueError("a request batch needs B > 0 and steps > 0")
    seeds = list(seeds) if isinstance(seeds, (list, tuple)) or torch.is_tensor(seeds) else None
    if seeds is None or len(seeds) != B:
        raise ValueError("seeds must be a sequence of %d integers (one per request)" % B)
    seed_t = torch.tensor([seed_word(int(v)) for v in seeds], dtype=torch.int64)
    is_num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
    is_pair = lambda v: isinstance(v, (list, tuple)) and len(v) == 2 and all(is_num(x) for x in v)
    t_message = lambda v: "temperature must be one (start, end) pair or a list of %d such pairs" % B
    t_pairs = _per_request(temperature, B, t_message, one=is_pair)
    if not all(is_pair(v) for v in t_pairs):
        raise ValueError(t_message(temperature))
    temps = torch.tensor([linspace_schedule(float(a), float(b), steps) for a, b in t_pairs], dtype=torch.float32).t().contiguous()
    if not bool((temps > 0).all()):
        raise ValueError("every step temperature of a request batch must be > 0 (temperature 0, the argmax extension, is not offered per request)")
    if cfg is None:
        return seed_t, temps, None
    if isinstance(cfg, tuple):
        raise TypeError("cfg must be None, a float or a LIST with one entry per request (a float or a (start, end) tuple each); a bare tuple is ambiguous")
    rows = []
    for e in _per_request(cfg, B, lambda v: "cfg must be None, a float or a list of %d entries" % B, one=is_num, seq=list):
        if e is None:
            raise ValueError("guidance is on for every request of a batch or for none: cfg=None cannot be mixed with guided requests (pass 1.0 for 'no guidance')")
        if is_num(e):
            rows.append([[float(torch.tensor(float(e), dtype=torch.float32)), float(torch.tensor(1.0 - float(e), dtype=torch.float32))]] * steps)
        elif isinstance(e, tuple) and is_pair(e):
            sched = torch.linspace(e[0], e[1], steps)
            rows.append([[float(sched[i]), float(1 - sched[i])] for i in range(steps)])
        else:
            raise ValueError("a cfg entry must be a float or a (start, end) tuple, got %r" % (e,))
    pairs = torch.tensor(rows, dtype=torch.float32).permute(1, 0, 2).contiguous()
    return seed_t, temps, pairs


class RequestTables:
    """the DEVICE tables of a request batch (seeds int64 [B], temps fp32 [steps, B], pairs fp32 [steps, B, 2] or None); `load` rewrites them in place, which is
    all a captured graph needs to serve other seeds, guidance scales and temperatures"""

    def __init__(self, host, device):
        self.seeds, self.temps, self.pairs = (None if t is None else t.to(device) for t in host)

    def load(self, host):
        if (host[2] is None) != (self.pairs is None):
            raise ValueError("guidance cannot be switched %s for a captured request batch" % ("off" if host[2] is None else "on"))
        for dst, src in zip((self.seeds, self.temps, self.pairs), host):
            if dst is not None:
                dst.copy_(src)

    def step(self, i):
        """what forward_sample(req=...) takes at step i"""
        return (self.seeds, self.temps[i], None if self.pairs is None else self.pairs[i])


# ---------------------------------------------------------------------------------------------------------------- truncated sampling
FILTER_OFF = (0, 1.0, 1.0, 1)  # (top_k, top_p, typical_mass, min_tokens) as the kernels read them: top_k <= 0, a mass of 1 = off


def check_filter(top_k=None, top_p=None, typical_mass=None, min_tokens=1):
    """One truncation setting -> (top_k, top_p, typical_mass, min_tokens) in the kernels' encoding (None becomes 0 / 1.0 / 1.0).  Raises a ValueError that names
    the argument: a negative top_k, a mass outside (0, 1], min_tokens < 1, both mass filters at once (top_p=1 / typical_mass=1 are "off" and combine with anything)."""
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
    is_num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
    if top_k is not None and (not is_int(top_k) or top_k < 0):
        raise ValueError("top_k must be None or an integer >= 0 (0 = off), got %r" % (top_k,))
    for name, v in (("top_p", top_p), ("typical_mass", typical_mass)):
        if v is not None and (not is_num(v) or not 0.0 < float(v) <= 1.0):
            raise ValueError("%s must be None or a mass in (0, 1] (1 = off), got %r" % (name, v))
    if not is_int(min_tokens) or min_tokens < 1:
        raise ValueError("min_tokens must be an integer >= 1, got %r" % (min_tokens,))
    p, m = 1.0 if top_p is None else float(top_p), 1.0 if typical_mass is None else float(typical_mass)
    if p < 1.0 and m < 1.0:
        raise ValueError("top_p and typical_mass are mutually exclusive: one mass filter at most (got top_p=%r, typical_mass=%r)" % (top_p, typical_mass))
    return (0 if top_k is None else int(top_k), p, m, int(min_tokens))


def filter_on(f):
    """does a `check_filter` tuple restrict anything (a top_k >= num_labels still counts: the kernel finds it off)"""
    return f[0] > 0 or f[1] < 1.0 or f[2] < 1.0


def _filter_names(top_k, top_p, typical_mass):
    return " / ".join(n for n, v in (("top_k", top_k), ("top_p", top_p), ("typical_mass", typical_mass)) if v is not None) or "top_k / top_p / typical_mass"


def _philox_only(names, why, noise, temperatures):
    """the two refusals of a whole call's filter and renoise settings: every call that can carry one passes `_call_filter` / `_call_renoise` on its way to `_sample_core`"""
    if noise != "philox":
        raise ValueError("%s needs noise='philox' (the counter-based sampling tail %s)" % (names, why))
    if any(t == 0 for t in temperatures):
        raise ValueError("%s is not offered with a step temperature of 0 (the argmax extension)" % names)


def request_filters(B, top_k=None, top_p=None, typical_mass=None, min_tokens=1):
    """HOST tables of a request batch's filters: each argument one value for all requests or a list of B -> (k int32 [B, 2] = (top_k, min_tokens), mass fp32 [B, 2]
    = (top_p, typical_mass), any_on); every row validated by `check_filter` (the message names the argument and the request)."""
    rows = _request_rows(int(B), check_filter, top_k=top_k, top_p=top_p, typical_mass=typical_mass, min_tokens=min_tokens)
    k = torch.tensor([[r[0], r[3]] for r in rows], dtype=torch.int32)
    mass = torch.tensor([[r[1], r[2]] for r in rows], dtype=torch.float32)
    return k, mass, any(filter_on(r) for r in rows)


class FilterTables:
    """the DEVICE tables of a filtered request batch: k int32 [B, 2], mass fp32 [B, 2] (`request_filters`; `load` rewrites them in place, all a captured graph needs
    to serve other filters) and, because the filtered tail of the request family is the stream form, the constant stream tables of every step of a batch whose
    requests march in step: step [steps, B] = i, t_next [steps, B] = t_list[i + 1] (-1 from renoise_steps on: never renoises), active [B] = 1."""

    def __init__(self, host, device, steps, renoise_steps, t_list):
        B = host[0].size(0)
        self.k, self.mass = host[0].to(device), host[1].to(device)
        self.step = torch.arange(steps, dtype=torch.int32)[:, None].repeat(1, B).contiguous().to(device)
        self.t_next = torch.tensor([float(t_list[i + 1]) if i < renoise_steps else -1.0 for i in range(steps)], dtype=torch.float32)[:, None].repeat(1, B).contiguous().to(device)
        self.active = torch.ones(B, dtype=torch.int32, device=device)

    def load(self, host):
        self.k.copy_(host[0])
        self.mass.copy_(host[1])


# ---------------------------------------------------------------------------------------------------------------- confidence-ordered renoise
RENOISE_POLICY = {"random": 0, "confidence": 1}  # as the renoise stage reads it (tail.hip: renoise_select_kernel)


def check_renoise(renoise="random", confidence_noise=0.0):
    """One renoise setting -> (policy, confidence_noise) in the kernels' encoding.  renoise: "random" (an independent coin u <= t_next per position, the
    reference's policy) or "confidence" (after each step exactly rint(t_next * free positions) tokens go back to noise, the least confident first);
    confidence_noise g >= 0: the scale of the annealed Gumbel perturbation of the confidence scores (score = logprob + g * t_next * Gumbel; 0 = none), which only
    acts under "confidence".  Raises a ValueError that names the argument."""
    if not isinstance(renoise, str) or renoise not in RENOISE_POLICY:
        raise ValueError("renoise must be 'random' or 'confidence', got %r" % (renoise,))
    g = confidence_noise
    if isinstance(g, bool) or not isinstance(g, (int, float)) or not 0.0 <= float(g) < float("inf"):
        raise ValueError("confidence_noise must be a finite number >= 0, got %r" % (g,))
    return RENOISE_POLICY[renoise], float(g)


def _call_renoise(noise, temperatures, renoise, confidence_noise, return_stats):
    """the renoise setting of a whole call: validated, None with the defaults (the call then takes exactly the path it takes without these arguments), else
    (policy, confidence_noise, return_stats)"""
    policy, g = check_renoise(renoise, confidence_noise)
    if policy == 0 and not return_stats:
        return None
    _philox_only("renoise='confidence'" if policy else "return_stats", "reports the statistics the selection ranks", noise, temperatures)
    return policy, g, bool(return_stats)


def request_renoise(B, renoise="random", confidence_noise=0.0):
    """HOST tables of a request batch's renoise settings: each argument one value for all requests or a list of B -> (policy int32 [B], confidence_noise fp32 [B],
    any_confidence); every entry validated by `check_renoise` (the message names the argument and the request)."""
    rows = _request_rows(int(B), check_renoise, renoise=renoise, confidence_noise=confidence_noise)
    return torch.tensor([r[0] for r in rows], dtype=torch.int32), torch.tensor([r[1] for r in rows], dtype=torch.float32), any(r[0] for r in rows)


class ConfidenceTables:
    """the DEVICE tables of a request batch that renoises per request: policy int32 [B], noise fp32 [B] (`request_renoise`) and `never` fp32 [B] = -1, the renoise
    threshold the statistics tail runs with (the renoise stage after it does the renoising)"""

    def __init__(self, host, device):
        self.policy, self.noise = host[0].to(device), host[1].to(device)
        self.never = torch.full((host[0].numel(),), -1.0, dtype=torch.float32, device=device)


def _renoise_stage(drawn, logprob, init_noise, rows, rows_per_sample, seed, offset, t_next, policy, g, out, seed_dev=None, row_offset=0, row_offset_dev=None, pin=None):
    """the renoise stage, scalar form (`out` may be `drawn`)"""
    pk, pt = (None, None) if pin is None else pin
    dev = drawn.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().paella_renoise_select(_lib.ptr(drawn), _lib.ptr(logprob), _lib.ptr(init_noise), rows, rows_per_sample, seed, _lib.ptr(seed_dev), offset,
                                                     row_offset, _lib.ptr(row_offset_dev), t_next, policy, g, _lib.ptr(pk), _lib.ptr(pt), _lib.ptr(out),
                                                     _lib.stream_ptr(dev)))


def _weights_vector(v):
    if v is None:
        return None
    if not torch.is_tensor(v) or v.dim() != 1:
        raise ValueError("attn_weights: every vector must be a 1-D tensor (utils/alter_attention.py:27), got %r" % (type(v).__name__ if not torch.is_tensor(v) else tuple(v.shape),))
    return v.detach().to(torch.float32)


def request_weight_pair(entry):
    """one request's `attn_weights` -> (conditional, unconditional), each a 1-D fp32 tensor or None: None = unweighted; a vector weighs both sides (what the one
    vector of a whole call does); a pair (conditional, unconditional), either member None, weighs each side of the guided step on its own -- "my image rows times
    2" addresses the conditional side only, whose last rows they are."""
    if entry is None or torch.is_tensor(entry):
        v = _weights_vector(entry)
        return v, v
    if isinstance(entry, (tuple, list)) and len(entry) == 2 and all(m is None or torch.is_tensor(m) for m in entry):
        return _weights_vector(entry[0]), _weights_vector(entry[1])
    raise ValueError("attn_weights: a request's entry must be None, a 1-D tensor or a pair (conditional, unconditional) of those, got %r" % (type(entry).__name__,))


def split_request_weights(attn_weights, B):
    """the `attn_weights` argument of a request batch -> (shared, pairs): a 1-D tensor (or None) is ONE vector for all requests, returned as `shared` -- the
    path and the bits of a call without per-request weights; a list with one entry per request (`request_weight_pair`) comes back as `pairs`, B (conditional,
    unconditional) pairs.  Exactly one of the two is not None, or both are for attn_weights=None."""
    if attn_weights is None or torch.is_tensor(attn_weights):
        if attn_weights is not None and attn_weights.dim() != 1:
            raise ValueError("attn_weights must be 1-D (utils/alter_attention.py:27)")
        return attn_weights, None
    if not isinstance(attn_weights, list) or len(attn_weights) != int(B):
        raise ValueError("attn_weights must be None, one 1-D tensor for all requests or a LIST with one entry per request (%d), got %s" %
                         (int(B), "a list of %d" % len(attn_weights) if isinstance(attn_weights, list) else type(attn_weights).__name__))
    return None, [request_weight_pair(e) for e in attn_weights]


def check_weight_pair(pair, keys, guided, max_n=None, what="attn_weights"):
    """host validation of one request's (conditional, unconditional) weights: each vector at most `max_n` long (the table's row, None = no limit) and at most
    as long as that side's own key sequence, keys = (conditional, unconditional) from `min_attention_keys` (None = the model has no attention) -- a longer one
    would be clamped by the kernels, which shifts what every entry means.  An unguided request has no unconditional side."""
    c, u = pair
    if not guided:
        if u is not None and u is not c:
            raise ValueError("%s: an unguided request has no unconditional side to weigh (pass one vector, or (conditional, None))" % what)
        u = None
    for v, k, side in ((c, keys[0], "conditional"), (u, keys[1], "unconditional")):
        if v is None:
            continue
        if max_n is not None and v.numel() > max_n:
            raise ValueError("%s: %d %s weights, the table holds at most %d per slot (max_attn_weights)" % (what, v.numel(), side, max_n))
        if k is not None and v.numel() > k:
            raise ValueError("%s: %d %s weights, more than the %d keys of that side's shortest key sequence" % (what, v.numel(), side, k))
    return c, u


def _load_key_weights(kw, pairs, keys, guided, max_n=None):
    """validate every request's pair, then write the table in place: conditional rows in slots [0, B), unconditional ones in [B, 2B)"""
    B = len(pairs)
    pairs = [check_weight_pair(p, keys, guided, max_n, "attn_weights[%d]" % b) for b, p in enumerate(pairs)]
    for b, (c, u) in enumerate(pairs):
        kw.set(b, c)
        if guided:
            kw.set(B + b, u)
    return kw


def _request_keys(model, H, W, model_inputs, unconditional_inputs):
    """(conditional, unconditional) shortest key sequence of a request with these conditioning sets"""
    return (min_attention_keys(model._cfg, H, W, _cond_seq_len(model, model_inputs)),
            min_attention_keys(model._cfg, H, W, _cond_seq_len(model, unconditional_inputs)) if unconditional_inputs is not None else None)


def timestep_table(t_list, steps, B, device):
    """[steps, B] fp32: row i = the timestep of step i for every sample (one upload instead of a fill kernel per step)."""
    return torch.tensor([float(v) for v in t_list[:steps]], dtype=torch.float32).to(device)[:, None].repeat(1, B).contiguous()


def select_tokens(a, b=None, mask=None, flag=None, fill=-1, out=None):
    """out[i] = keep(i) ? a[i] : (b[i] if b is given else fill), keep(i) = (mask is None or mask[i] != 0) and (flag is None or flag[0] == 1.0) -- int64 token
    grids, `flag` a 1-element fp32 DEVICE tensor (paella_select_tokens: one HIP kernel, no host synchronisation, graph-capturable).  Used by the inpainting
    wrapper (re-impose the known tokens) and by the batch-sharded sampler (-1 tokens when the conditioning broadcast was flagged invalid)."""
    dev = a.device
    if dev.type != "cuda" or a.dtype != torch.int64:
        raise ValueError("select_tokens needs int64 HIP tensors")
    a = a.contiguous()
    for name, t in (("b", b), ("mask", mask)):
        if t is not None and (t.dtype != torch.int64 or t.shape != a.shape or t.device != dev):
            raise ValueError("select_tokens: %s must be an int64 tensor of a's shape on a's device" % name)
    if flag is not None and (flag.dtype != torch.float32 or flag.numel() != 1 or flag.device != dev):
        raise ValueError("select_tokens: flag must be a 1-element fp32 tensor on a's device")
    if out is None:
        out = torch.empty_like(a)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().paella_select_tokens(_lib.ptr(a), _lib.ptr(None if b is None else b.contiguous()), _lib.ptr(None if mask is None else mask.contiguous()),
                                                    _lib.ptr(flag), int(fill), a.numel(), _lib.ptr(out), _lib.stream_ptr(dev)))
    return out


def _sample_core(model, model_inputs, unconditional_inputs, latent_shape, init_x, steps, renoise_steps, t_list, temperatures,
                 cfgs, device, noise="torch", seed=None, attn_weights=None, seed_dev=None, init_noise_buf=None, r_all=None, shard=None,
                 ws=None, fused_tail=True, row_offset_dev=None, req=None, pin=None, filt=None, conf=None):
    """cfgs: per-step list of (cfg_fp32, one_minus_cfg_fp32) or None (no guidance at that step).
    seed_dev / row_offset_dev / init_noise_buf / r_all: device-resident seed and row-offset words, a buffer for the start tokens
    and the [steps, B] timestep table (HIP-graph capture cannot upload from the host, see GraphSampler); ws: caller-owned
    workspace for every library call.
    shard = (lo, total): this call samples rows [lo, lo + B) of a global batch of `total`; with noise="philox" every random
    number is keyed by the GLOBAL row, so the shard reproduces those rows of the unsharded call bit for bit.
    req (RequestTables; noise="philox" only): the B samples are independent requests -- seed, guidance pair and temperature per sample come from its device
    tables, `seed` / `shard` are unused, `temperatures` must be positive placeholders and `cfgs` only says whether guidance is on.
    pin=(keep, known) (noise="philox" only; int64 [B, H, W] each): after EVERY step's draw and renoise the tail writes known[row] wherever keep[row] == 0 -- the
    known region of an editing request stays clean while the model denoises (paella_amd.editing.inpaint(pin="step")).
    filt (noise="philox" only): truncated sampling -- a `check_filter` tuple (one setting for the call) or, with `req`, a `FilterTables`.  Every step then takes the
    logits forward plus the filtered tail: `fused_tail` is ignored, rows * L * 4 bytes of logits are written and read back per step.
    conf (noise="philox" only): confidence-ordered renoise / statistics -- (policy, confidence_noise, return_stats) of `_call_renoise` or, with `req`, a
    `ConfidenceTables` (then `filt` carries the stream tables).  Every step is then the logits forward, the statistics tail (the filtered tail's draw plus log p(token)
    and the row entropy, no renoise) and, on a renoising step, the renoise stage; `fused_tail` is ignored.  With return_stats the result is (tokens, {"logprob",
    "entropy"}), fp32 [B, H, W] maps of the final step's draw."""
    device = torch.device(device)
    B, H, W = shape = tuple(int(v) for v in latent_shape)
    L = model.num_labels
    native = isinstance(model, Paella)
    _refuse_core_args(noise, device, native, shape, temperatures[:steps], init_x, shard, req, pin)
    philox = noise == "philox"
    if seed is None:
        # GraphSampler keeps the live seed in device memory; without the counter-based generator it is unused: every random number comes from torch's generator
        # or from explicit tensors
        seed = fresh_seed() if philox and seed_dev is None else 0
    row_offset = 0 if shard is None else int(shard[0]) * H * W
    with torch.inference_mode():
        init_noise = _start_noise(noise, L, shape, seed, device, shard, req, init_noise_buf, seed_dev, row_offset_dev)
        sampled = init_noise.clone() if init_x is None else init_x.to(device=device, dtype=torch.int64).contiguous()
        cond_c, cond_u, cond_both, batched = _prepare_conditioning(model, model_inputs, unconditional_inputs, B, cfgs, philox, ws) if native else (None, None, None, False)
        bufs = {}  # logits buffers exist only for steps that take the unfused path (allocated on first use: 8.6 GB each at BASELINE configs[2])
        out = torch.empty(B, H, W, dtype=torch.int64, device=device)
        if r_all is None:
            r_all = timestep_table(t_list, steps, B, device)
        fuse = philox and native and fused_tail and filt is None and conf is None  # head GEMM + tail in one launch: no logits tensor at all (a filter needs the whole row)
        stats = None if conf is None else tuple(torch.empty(B, H, W, dtype=torch.float32, device=device) for _ in range(2))  # (logprob, entropy)
        for i in range(steps):
            cfg, temp = cfgs[i], temperatures[i]  # cfg None: no guidance at this step; temp 0: argmax
            t_next = t_list[i + 1] if i < renoise_steps else None  # None: this step does not renoise
            if fuse and (cfg is None or (batched and temp != 0)):
                # in place is safe: the token gather at the head of the forward and the token store at its tail are different kernels
                # of one stream
                model.forward_sample(sampled, r_all[i], cond_c if cfg is None else cond_both, out, temperature=temp if temp != 0 else 1.0, argmax=temp == 0,
                                     seed=seed, seed_dev=seed_dev, offset=i, row_offset=row_offset, row_offset_dev=row_offset_dev,
                                     init_noise=None if t_next is None else init_noise, t_next=0.0 if t_next is None else t_next,
                                     cfg_mix=cfg if req is None else None, attn_weights=attn_weights, ws=ws,
                                     req=None if req is None else req.step(i), **({} if pin is None else {"pin": pin}))
            else:
                lc, lu = _step_logits(model, sampled, r_all[i], i, cfg, philox and temp != 0, (cond_c, cond_u, cond_both, batched), bufs,
                                      (model_inputs, unconditional_inputs), attn_weights, ws, req)
                noise_q, mask_u = _step_noise(noise, i, shape, L, device, temp != 0, t_next is not None)
                _draw(lc, lu, out, i, temp, cfg, t_next, init_noise, (seed, seed_dev, row_offset, row_offset_dev), noise_q, mask_u, req, pin, filt, conf, stats)
            sampled = out  # no tail reads `sampled`, so one output buffer is enough (stream-ordered reuse)
    if conf is not None and req is None and conf[2]:
        return sampled, {"logprob": stats[0], "entropy": stats[1]}
    return sampled


def _refuse_core_args(noise, device, native, shape, temperatures, init_x, shard, req, pin):
    """what `_sample_core` refuses, before anything touches the device (the library is loaded on the way).  `filt` and `conf` are not looked at: a whole call's
    settings were checked against the noise mode and the temperatures where they were built (`_philox_only`), the tables of a request batch need neither check."""
    explicit = isinstance(noise, dict)  # parity tests: {"init_noise": [B,H,W], "q": [rows,L] per step, "u": [B,H,W] per step}
    if not explicit and noise not in ("torch", "philox"):
        raise ValueError("noise must be 'torch', 'philox' or a dict of explicit noise tensors")
    if device.type != "cuda":
        raise RuntimeError("paella_amd.sample runs on a HIP device only (got device=%s); there is no CPU path" % device)
    _lib.load()
    philox = noise == "philox"
    if shard is not None and not (philox or explicit):
        raise ValueError("shard=(lo, total) needs noise='philox' (or explicit noise tensors): torch's generator stream cannot be sharded")
    if req is not None and not (philox and native and shard is None and init_x is None):
        raise ValueError("a request batch needs noise='philox', a paella_amd.Paella model, no shard and no init_x")
    if pin is not None:
        if not philox or req is not None:
            raise ValueError("pin=(keep, known) needs noise='philox' (the counter-based sampling tail re-imposes the known tokens) and no request tables")
        if any(t == 0 for t in temperatures):
            raise ValueError("pin=(keep, known) is not offered with a step temperature of 0 (the argmax extension)")
        for name, t in zip(("keep", "known"), pin):
            if not torch.is_tensor(t) or t.dtype != torch.int64 or tuple(t.shape) != shape or t.device.type != "cuda" or not t.is_contiguous():
                raise ValueError("pin: %s must be a contiguous int64 HIP tensor of shape %s" % (name, shape))


def _start_noise(noise, L, shape, seed, device, shard, req, buf, seed_dev, row_offset_dev):
    """the start tokens of a call, which are also the renoise source of its steps; buf: where a captured graph keeps them (GraphSampler)"""
    if req is not None:
        return start_tokens_requests(L, shape, req.seeds, out=buf)
    if noise == "philox":
        return start_tokens(L, shape, seed, device, shard, out=buf, seed_dev=seed_dev, row_offset_dev=row_offset_dev)
    if buf is not None:
        return buf
    if isinstance(noise, dict):
        return noise["init_noise"].to(device=device, dtype=torch.int64).contiguous()
    return torch.randint(0, L, size=shape, device=device)


def _prepare_conditioning(model, model_inputs, unconditional_inputs, B, cfgs, philox, ws):
    """the step-invariant conditioning work of a call -> (cond_c, cond_u, cond_both, batched): the prepared conditional and unconditional caches (None where no
    step needs one), the 2B-slot cache that holds both, and whether guided steps run as ONE forward against it"""
    any_cfg = any(c is not None for c in cfgs)
    cond_c = cond_u = cond_both = None
    if any_cfg and _same_cond_layout(model_inputs, unconditional_inputs):
        cond_both = model.prepare_cond(**_cat_inputs(model_inputs, unconditional_inputs), ws=ws)
    elif any_cfg and philox and _cond_batch(model_inputs) == B and _cond_batch(unconditional_inputs) == B \
            and min(_cond_seq_len(model, model_inputs), _cond_seq_len(model, unconditional_inputs)) > 0:
        # layouts differ (what conditioning.embed_prompts produces on real prompts): one ragged 2B-slot cache, every sample bounded by its own row count
        # in the attention kernels -- the same one-forward path as above.  noise="torch" / explicit noise keep the two forwards: their tokens are pinned
        # to the reference's, whose rounding is that of two separate evaluations
        cond_both = _prepare_ragged_pair(model, model_inputs, unconditional_inputs, B, ws)
    batched = cond_both is not None
    if not batched or not all(c is not None for c in cfgs):
        cond_c = model.prepare_cond(**model_inputs, ws=ws)
        cond_u = model.prepare_cond(**unconditional_inputs, ws=ws) if any_cfg and not batched else None
    return cond_c, cond_u, cond_both, batched


def _step_logits(model, sampled, r, i, cfg, fold, conds, bufs, inputs, attn_weights, ws, req):
    """the logits forward of ONE unfused step -> (lc, lu), fp32 [B, H, W, L] each; lu None: the step is unguided or its guidance mix is already in lc.
    conds: what `_prepare_conditioning` returned; bufs: the call's logits buffers by name, allocated here on first use; inputs: the two conditioning dicts"""
    cond_c, cond_u, cond_both, batched = conds
    B, H, W = sampled.shape

    def logits_buf(name, rows_b):
        if name not in bufs:
            bufs[name] = torch.empty(rows_b, H, W, model.num_labels, dtype=torch.float32, device=sampled.device)
        return bufs[name]
    if not isinstance(model, Paella):  # any other callable with the reference's signature; logits come back [B, L, H, W]
        lc = model(sampled, r, **inputs[0]).permute(0, 2, 3, 1).float().contiguous()
        return lc, (model(sampled, r, **inputs[1]).permute(0, 2, 3, 1).float().contiguous() if cfg is not None else None)
    if cfg is not None and batched:
        # one evaluation against the 2B-row conditioning cache: tokens / r are passed once, the library computes
        # the conditioning-free prefix for them and replicates it where the two passes diverge.  With the
        # counter-based generator (no bit-parity promise towards torch's RNG stream) a categorical step (`fold`) also lets
        # the guidance mix ride through the linear head: one mixed logits tensor comes back.
        logits2 = logits_buf("both", 2 * B)
        model.forward_prepared(sampled, r, cond_both, attn_weights=attn_weights, out=logits2[:B] if fold else logits2,
                               cfg_mix=cfg if fold and req is None else None, ws=ws, **({} if req is None else {"req_mix": req.pairs[i]}))
        return logits2[:B], (None if fold else logits2[B:])
    lc, lu = logits_buf("c", B), None
    model.forward_prepared(sampled, r, cond_c, attn_weights=attn_weights, out=lc, ws=ws)
    if cfg is not None:
        lu = logits_buf("u", B)
        model.forward_prepared(sampled, r, cond_u, attn_weights=attn_weights, out=lu, ws=ws)
    return lc, lu


def _step_noise(noise, i, shape, L, device, categorical, renoise):
    """the noise tensors of ONE unfused step that the tail does not generate itself -> (noise_q, mask_u), both None with noise="philox"; drawn in the reference's order"""
    if noise == "philox":
        return None, None
    if isinstance(noise, dict):
        given = lambda t: t.to(device=device, dtype=torch.float32).contiguous()
        return given(noise["q"][i]) if categorical else None, given(noise["u"][i]) if renoise else None
    B, H, W = shape
    rows = B * H * W
    noise_q = mask_u = None
    if categorical:
        # what torch.multinomial(scores, 1) draws internally: q = empty_like(scores).exponential_(1)
        # in the memory order of the reference's `scores.permute(0,2,3,1).reshape(-1, L)`: row-major copy for
        # B > 1, but a column-major VIEW of the NCHW softmax output for B == 1
        if B == 1:
            noise_q = torch.empty(L, rows, dtype=torch.float32, device=device).exponential_(1).t().contiguous()
        else:
            noise_q = torch.empty(rows, L, dtype=torch.float32, device=device).exponential_(1)
    if renoise:
        mask_u = torch.rand(B, H, W, dtype=torch.float32, device=device)  # == torch.rand_like(x.float())
    return noise_q, mask_u


def _draw(lc, lu, out, i, temp, cfg, t_next, init_noise, words, noise_q, mask_u, req, pin, filt, conf, stats):
    """The tail launches of ONE unfused step on its logits, in the one of the four tail forms the call has: scalar (`_tail`); scalar with statistics, then
    `_renoise_stage` (conf a tuple); request (`_tail_req`); request with statistics, then the stream form of the renoise stage (conf a ConfidenceTables).
    t_next None: the step does not renoise; words = (seed, seed_dev, row_offset, row_offset_dev); stats = (logprob, entropy) with conf."""
    rows, L = out.numel(), lc.size(-1)
    hw = rows // out.size(0)
    renoise = t_next is not None
    seed, seed_dev, row_offset, row_offset_dev = words
    cfg, omc = (1.0, 0.0) if cfg is None else cfg
    if conf is not None and req is not None:
        _stream_draw(lc, lu, rows, L, out, (None if lu is None else req.pairs[i], req.temps[i], req.seeds, hw), filt.step[i], filt.t_next[i] if renoise else None,
                     filt.active, init_noise, (filt.k, filt.mass), conf=(conf.never, conf.policy, conf.noise, *stats), renoise=renoise)
    elif conf is not None:
        # a renoising step: the raw draw and its statistics, then the renoise stage (which also applies the pin); the last steps: the pin rides in the tail
        _run_tail(lc, lu, rows, L, out, scalar=(cfg, omc, temp, 0, seed, seed_dev, row_offset, row_offset_dev, None, None), offset=i, pin=None if renoise else pin,
                  filt=FILTER_OFF if filt is None else filt, stats=stats)
        if renoise:
            _renoise_stage(out, stats[0], init_noise, rows, hw, seed, i, t_next, conf[0], conf[1], out, seed_dev=seed_dev, row_offset=row_offset,
                           row_offset_dev=row_offset_dev, pin=pin)
    elif req is not None:
        # (the stream form of the filtered tail wants its renoise source at every step; a step that does not renoise -- threshold -1 -- never reads it)
        _tail_req(lc, lu, rows, L, hw, req, i, init_noise if renoise or filt is not None else None, t_next if renoise else 0.0, out, filt=filt)
    else:
        _tail(lc, lu, rows, L, cfg, omc, temp if temp != 0 else 1.0, int(temp == 0), noise_q, seed, i, init_noise if renoise else None, mask_u,
              t_next if renoise else 0.0, out, seed_dev=seed_dev, row_offset=row_offset, row_offset_dev=row_offset_dev, pin=pin, filt=filt)


def _call_filter(noise, temperatures, top_k, top_p, typical_mass, min_tokens):
    """the filter of a whole call: validated, None when nothing is on (the call then takes exactly the path it takes without these arguments)"""
    f = check_filter(top_k, top_p, typical_mass, min_tokens)
    if not filter_on(f):
        return None
    _philox_only(_filter_names(top_k, top_p, typical_mass), "filters the draw", noise, temperatures)
    return f


def sample(model, model_inputs, latent_shape, unconditional_inputs=None, steps=12, renoise_steps=11, temperature=(1.0, 0.2),
           cfg=8.0, t_start=1.0, t_end=0.0, device="cuda", *, noise="torch", seed=None, seed_dev=None, attn_weights=None, shard=None, fused_tail=True,
           top_k=None, top_p=None, typical_mass=None, min_tokens=1, renoise="random", confidence_noise=0.0, return_stats=False):
    """Drop-in for reference src/utils.py:35 `sample` (same positional order and defaults).
    top_k / top_p / typical_mass / min_tokens (noise="philox" only; `check_filter`): truncated sampling, one setting for the call -- see `_sample_core`.
    renoise / confidence_noise / return_stats (noise="philox" only; `check_renoise`): renoise="confidence" sends exactly rint(t_next * free positions) tokens per
    sample back to noise after each renoising step, the least confident first (confidence_noise: the annealed Gumbel perturbation of the ranking); return_stats=True
    returns (tokens, {"logprob", "entropy"}), fp32 [B, H, W] maps of the final step's draw.  With the defaults the call is today's call -- see `_sample_core`.
    Keyword-only extensions: noise ("torch" = consume torch's generator exactly like the reference; "philox" = counter-based
    noise generated in the kernels, keyed by `seed` -- None draws a fresh seed from torch's generator), attn_weights
    (utils/modules.py:268), shard=(lo, total) for batch-sharded sampling (paella_amd.dist.sample_sharded), fused_tail (counter-based
    mode only: take the categorical decision inside the head GEMM so the logits are never written; False keeps the two-kernel
    path -- same tokens bit for bit, for A/B measurements), seed_dev (counter-based mode: a 1-element int64 DEVICE tensor added to `seed` inside
    the kernels -- a seed that arrived in a collective is used without a host round trip; pass seed=0 with it)."""
    if cfg and unconditional_inputs is None:
        # the reference raises TypeError at src/utils.py:46 (`**None`); keep the failure, make it readable
        raise TypeError("cfg=%r requires unconditional_inputs" % (cfg,))
    t_list, temperatures, cfgs = _scalar_schedule(steps, temperature, cfg, t_start, t_end)
    return _sample_core(model, model_inputs, unconditional_inputs, latent_shape, None, steps, renoise_steps, t_list, temperatures,
                        cfgs, device, noise=noise, seed=seed, seed_dev=seed_dev, attn_weights=attn_weights, shard=shard, fused_tail=fused_tail,
                        filt=_call_filter(noise, temperatures, top_k, top_p, typical_mass, min_tokens),
                        conf=_call_renoise(noise, temperatures, renoise, confidence_noise, return_stats))


def sample_distributed(model, model_inputs, unconditional_inputs, latent_shape, init_x=None, steps=12, renoise_steps=None,
                       temperature=(0.7, 0.3), cfg=(8.0, 8.0), t_start=1.0, t_end=0.0, sampling_conditional_steps=None, *,
                       noise="torch", seed=None, attn_weights=None, shard=None, fused_tail=True, pin=None, top_k=None, top_p=None, typical_mass=None, min_tokens=1,
                       renoise="random", confidence_noise=0.0, return_stats=False):
    """Drop-in for reference src_distributed/utils.py:97 `sample` (init_x, cfg schedule, conditional-step cutoff).
    top_k / top_p / typical_mass / min_tokens (noise="philox" only): truncated sampling, as `sample`.
    renoise / confidence_noise / return_stats (noise="philox" only): confidence-ordered renoise and the statistics maps, as `sample`; with pin= the count is taken over
    the positions the pin does not own.
    Keyword-only extension pin=(keep, known) (noise="philox" only): every step's tail re-imposes known where keep == 0, see `_sample_core`."""
    device = unconditional_inputs["byt5"].device
    if sampling_conditional_steps is None:
        sampling_conditional_steps = steps
    if renoise_steps is None:
        renoise_steps = steps - 1
    t_list = linspace_schedule(t_start, t_end, steps + 1)
    temperatures = linspace_schedule(temperature[0], temperature[1], steps)
    cfgs = [None] * steps
    if cfg is not None:
        sched = torch.linspace(cfg[0], cfg[1], steps)
        for i in range(min(steps, sampling_conditional_steps)):
            # `logits * cfgs[i] + logits_u * (1 - cfgs[i])` with a 0-dim fp32 tensor: (1 - cfg) is computed in fp32
            cfgs[i] = (float(sched[i]), float(1 - sched[i]))
    return _sample_core(model, model_inputs, unconditional_inputs, latent_shape, init_x, steps, renoise_steps, t_list, temperatures,
                        cfgs, device, noise=noise, seed=seed, attn_weights=attn_weights, shard=shard, fused_tail=fused_tail, pin=pin,
                        filt=_call_filter(noise, temperatures, top_k, top_p, typical_mass, min_tokens),
                        conf=_call_renoise(noise, temperatures, renoise, confidence_noise, return_stats))


def _scalar_schedule(steps, temperature, cfg, t_start, t_end):
    """(t_list, temperatures, per-step guidance pairs) of the src/utils.py:35 signature, for `sample` and for the capture of it (GraphSampler)"""
    pair = None
    if cfg:
        # `logits * cfg + logits_u * (1 - cfg)` with python-float cfg: both scalars are rounded to fp32 by torch
        pair = (float(torch.tensor(float(cfg), dtype=torch.float32)), float(torch.tensor(1.0 - float(cfg), dtype=torch.float32)))
    return linspace_schedule(t_start, t_end, steps + 1), linspace_schedule(temperature[0], temperature[1], steps), [pair] * steps


def _request_schedule(steps, t_start, t_end, guided):
    """what `_sample_core` takes for a request batch: the common timestep list, placeholder temperatures (the real ones are in the tables) and whether guidance is on"""
    return linspace_schedule(t_start, t_end, steps + 1), [1.0] * steps, [(1.0, 0.0) if guided else None] * steps


def sample_requests(model, model_inputs, unconditional_inputs, latent_shape, seeds, cfg=8.0, temperature=(1.0, 0.2), steps=12, renoise_steps=11,
                    t_start=1.0, t_end=0.0, device="cuda", attn_weights=None, fused_tail=True, *, top_k=None, top_p=None, typical_mass=None, min_tokens=1,
                    renoise="random", confidence_noise=0.0):
    """B independent REQUESTS sampled as one batch (counter-based noise): request b has its own seed `seeds[b]`, guidance and temperature range, and its
    tokens are a function of the request alone -- every random number it draws is the one `sample(..., latent_shape=(1, H, W), noise="philox", seed=seeds[b])`
    draws, whatever slot it sits in and whoever shares the batch (the logits may still differ in their last bits with the batch size: the GEMMs split their
    work by tile index).  `cfg` / `temperature`: one value for all requests or one per request, see `request_tables`.  `steps`, `renoise_steps`, `t_start` /
    `t_end`, the grid and the conditioning layout are common to the batch.  Two requests with equal seeds draw identical noise.  Returns tokens [B, H, W].
    attn_weights: one 1-D tensor for all requests (one vector per launch, as `sample`), or a LIST with one entry per request -- None, a vector (both sides of
    the guided step) or a pair (conditional, unconditional), either member None (`request_weight_pair`).  The list form runs on a `KeyWeights` table with one row
    per conditioning slot: request b's tokens are those of a call in which every request carries request b's weights, bit for bit, whatever its batch-mates
    carry.  A guided list call needs the one-forward path (both conditioning sets with B samples each).
    top_k / top_p / typical_mass / min_tokens: truncated sampling, each one value for all requests or a list with one per request (`request_filters`); request b
    is filtered as `sample(..., seed=seeds[b], <its values>)` filters it.  With a filter on for anyone every step takes the logits forward plus the filtered tail.
    renoise / confidence_noise: each one value for all requests or a list with one per request (`request_renoise`); request b renoises as
    `sample(..., seed=seeds[b], <its values>)` does, whatever its batch-mates carry.  With renoise="confidence" for anyone every step takes the logits forward, the
    statistics tail and the renoise stage, all in their request form."""
    B, H, W = (int(v) for v in latent_shape)
    host = request_tables(B, steps, seeds, cfg, temperature)
    fhost = request_filters(B, top_k, top_p, typical_mass, min_tokens)
    chost = request_renoise(B, renoise, confidence_noise)
    if host[2] is not None and unconditional_inputs is None:
        raise TypeError("cfg=%r requires unconditional_inputs" % (cfg,))
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("paella_amd.sample_requests runs on a HIP device only (got device=%s); there is no CPU path" % device)
    t_list, temps, cfgs = _request_schedule(steps, t_start, t_end, host[2] is not None)
    attn_weights, pairs = split_request_weights(attn_weights, B)
    if pairs is not None:
        guided = host[2] is not None
        if guided and not (_cond_batch(model_inputs) == B and _cond_batch(unconditional_inputs) == B
                           and min(_cond_seq_len(model, model_inputs), _cond_seq_len(model, unconditional_inputs)) > 0):
            raise ValueError("attn_weights per request in a guided batch run as ONE forward over 2B conditioning slots (one table row each): model_inputs and "
                             "unconditional_inputs must each hold %d samples with at least one conditioning row (got %r and %r samples)"
                             % (B, _cond_batch(model_inputs), _cond_batch(unconditional_inputs)))
        n_max = max([1] + [v.numel() for p in pairs for v in p if v is not None])
        attn_weights = _load_key_weights(KeyWeights(2 * B if guided else B, n_max, device), pairs,
                                         _request_keys(model, H, W, model_inputs, unconditional_inputs if guided else None), guided)
    return _sample_core(model, model_inputs, unconditional_inputs, (B, H, W), None, steps, renoise_steps, t_list, temps, cfgs, device, noise="philox", seed=0,
                        attn_weights=attn_weights, fused_tail=fused_tail, req=RequestTables(host, device),
                        filt=FilterTables(fhost, device, steps, renoise_steps, t_list) if fhost[2] or chost[2] else None,
                        conf=ConfidenceTables(chost, device) if chost[2] else None)


class _EngineGraph(GraphOwner):
    """A captured graph of the inference engines' launches (`GraphSampler`, `RequestStream`): besides the shapes it depends on the weights and the precision mode
    of `self.model` and, where there is one, of `self.vqgan`."""

    _stale_hint = "load_state_dict / optimizer step / .to() / set_gemm_precision"

    def _state(self):
        st = [("denoiser weights", self.model._signature()), ("denoiser gemm precision", self.model._precision)]
        if self.vqgan is not None:
            st += [("VQGAN weights", self.vqgan._signature()), ("VQGAN gemm precision", self.vqgan._precision)]
        return st


class GraphSampler(_EngineGraph):
    """The whole `sample()` call (conditioning prep, all denoising steps, sampling tails; optionally the VQGAN
    decode) captured ONCE into a HIP graph for fixed shapes and replayed per request.

    Why: at batch 1 the path is ~3000 short kernels per image and eager launches are host-bound at ~2.8 us per kernel
    on this platform (tools/launch_floor.py), a graph replays the same kernels at ~1.6-1.8 us.  Arithmetic, kernels and
    results are identical to `sample(..., noise="philox")`; only the submission mechanism changes.  Per request the
    conditioning tensors are copied into the graph's static input buffers and two device words are rewritten: the Philox seed
    and the GLOBAL row offset of this replay's batch shard.  Start tokens, categorical draws and renoise masks are all drawn
    inside the graph as functions of (seed, global row, step): `sampler(seed=s, shard=(lo, total))` returns exactly rows
    [lo, lo + B) of `sample(..., noise="philox", seed=s)` over the global batch (tests/test_gpu_sample.py).
    seed=None draws a fresh seed from torch's global CPU generator (one draw per call; see fresh_seed).
    top_k / top_p / typical_mass / min_tokens (keyword-only): one truncation setting baked into the capture, as `sample` takes it.
    renoise / confidence_noise / return_stats (keyword-only): one renoise setting baked into the capture, as `sample` takes it; with return_stats a replay returns
    (tokens, {"logprob", "entropy"}) -- with a VQGAN (tokens, image, {...}) -- in graph-owned buffers.

    Staleness (the call site that reloads weights between sampling calls is src/train.py:40,64-69,76): a capture bakes raw pointers,
    host-side constants read from the weights (the VQGAN's ResBlock gammas) and the precision mode's kernel choice.  Every replay first compares the models'
    parameter signature (data_ptr + version of every tensor) and precision with what the capture saw; on a difference it RECAPTURES (on_stale="recapture",
    default: the replay then equals a fresh eager call bit for bit) or raises a RuntimeError naming the cause (on_stale="raise")."""

    def __init__(self, model, model_inputs, unconditional_inputs, latent_shape, steps=12, renoise_steps=11, temperature=(1.0, 0.2),
                 cfg=8.0, t_start=1.0, t_end=0.0, device="cuda", vqgan=None, attn_weights=None, on_stale="recapture", *, top_k=None, top_p=None, typical_mass=None,
                 min_tokens=1, renoise="random", confidence_noise=0.0, return_stats=False):
        self._init_owner(on_stale)
        # confidence-ordered renoise / statistics, one setting baked into the capture (None = today's capture)
        self.conf = _call_renoise("philox", linspace_schedule(temperature[0], temperature[1], steps), renoise, confidence_noise, return_stats)
        if not hasattr(self, "filt"):  # truncated sampling, one setting baked into the capture (GraphRequestSampler keeps device tables here instead)
            self.filt = _call_filter("philox", linspace_schedule(temperature[0], temperature[1], steps), top_k, top_p, typical_mass, min_tokens)
        self.model, self.vqgan, self.device = model, vqgan, torch.device(device)
        self.shape = tuple(int(v) for v in latent_shape)
        self.kw = dict(steps=steps, renoise_steps=renoise_steps, temperature=temperature, cfg=cfg, t_start=t_start, t_end=t_end)
        self.attn_weights = attn_weights
        clone = lambda d: None if d is None else {k: (None if v is None else ([t.clone() for t in v] if isinstance(v, (list, tuple)) else v.clone()))
                                                  for k, v in d.items()}
        self.cond, self.uncond = clone(model_inputs), clone(unconditional_inputs)
        self.seed_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.row_offset_dev = torch.zeros(1, dtype=torch.int64, device=self.device)  # lo * H * W of the shard being sampled
        self.init_noise = torch.zeros(self.shape, dtype=torch.int64, device=self.device)
        self.r_all = timestep_table(linspace_schedule(t_start, t_end, steps + 1), steps, self.shape[0], self.device)
        self._capture()

    def _capture(self):
        # The graph bakes raw pointers: it owns its workspaces (the modules' own scratch is dropped and reallocated whenever a
        # later eager call needs a bigger one) and it is the only user of their split-K tickets.  Sized here: the fast mode needs more room.
        B, H, W = self.shape
        S = max(_cond_seq_len(self.model, self.cond), _cond_seq_len(self.model, self.uncond), 1)
        self.graph = self.out = None
        self.ws = _lib.new_workspace(self.model.workspace_bytes(2 * B, H, W, S), self.device)
        self.vq_ws = None if self.vqgan is None else _lib.new_workspace(self.vqgan.workspace_bytes(B, H, W), self.device)
        self.out = self._capture_graph(self._run)

    def _schedule(self):
        """(t_list, temperatures, per-step guidance pairs) of the src/utils.py:35 signature"""
        k = self.kw
        return _scalar_schedule(k["steps"], k["temperature"], k["cfg"], k["t_start"], k["t_end"])

    def _init_x(self):
        """tokens the loop starts from (None = the Philox start tokens); GraphInpainter encodes + renoises an image here"""
        return None

    def _pin(self):
        """(keep, known) the tail of every step re-imposes (called after `_init_x`), or None; GraphInpainter(pin="step") returns its mask and encoded tokens"""
        return None

    def _finish(self, toks):
        return toks

    def _run(self):
        k = self.kw
        t_list, temps, cfgs = self._schedule()
        init_x = self._init_x()
        toks = _sample_core(self.model, self.cond, self.uncond, self.shape, init_x, k["steps"], k["renoise_steps"], t_list, temps, cfgs,
                            self.device, noise="philox", seed=0, attn_weights=self.attn_weights, seed_dev=self.seed_dev,
                            init_noise_buf=self.init_noise, r_all=self.r_all, ws=self.ws, row_offset_dev=self.row_offset_dev, pin=self._pin(), filt=self.filt,
                            conf=self.conf)
        stats = ()
        if self.conf is not None and self.conf[2]:
            toks, stats = toks[0], (toks[1],)
        toks = self._finish(toks)
        if self.vqgan is None:
            return (toks, *stats) if stats else toks
        return (toks, self.vqgan.decode_indices(toks, ws=self.vq_ws), *stats)

    @staticmethod
    def _match_inputs(dst, src):
        """a call's conditioning set `src` against the captured one `dst` -> the (buffer, tensor) pairs to copy.  Nothing is copied here: a refused set raises
        ValueError and leaves every buffer as it was"""
        if dst is None:
            if src is not None:
                raise ValueError("the graph was captured without this conditioning set")
            return []
        todo = []
        for key, d in dst.items():
            s = src.get(key) if src is not None else None
            if d is None:
                if s is not None:
                    raise ValueError("conditioning layout differs from the captured one (%s)" % key)
                continue
            if isinstance(d, (list, tuple)):
                if not isinstance(s, (list, tuple)) or len(s) != len(d) or any(a.shape != b.shape for a, b in zip(d, s)):
                    raise ValueError("conditioning layout differs from the captured one (%s: list length / shapes)" % key)
                todo.extend(zip(d, s))
            else:
                if s is None or isinstance(s, (list, tuple)) or s.shape != d.shape:
                    raise ValueError("conditioning shape differs from the captured one (%s)" % key)
                todo.append((d, s))
        return todo

    def _refresh(self, model_inputs, unconditional_inputs, grids=()):
        """what every replay starts with: a capture that matches the weights, then this call's inputs in the graph's input buffers (None = keep).  grids: (name,
        buffer, tensor or None) of what the capture holds besides the conditioning (GraphInpainter: images and mask).  Every given input is matched against
        the captured layout before any is copied: a refused call leaves the buffers as they were."""
        self._check_fresh()
        todo = []
        for name, d, s in grids:
            if s is not None:
                if tuple(s.shape) != tuple(d.shape):
                    raise ValueError("%s shape differs from the captured one" % name)
                todo.append((d, s))
        if model_inputs is not None:
            todo += self._match_inputs(self.cond, model_inputs)
        if unconditional_inputs is not None:
            todo += self._match_inputs(self.uncond, unconditional_inputs)
        for d, s in todo:  # only after every input was accepted
            d.copy_(s)

    def _set_words(self, seed, shard):
        if seed is None:
            seed = fresh_seed()
        lo = 0
        if shard is not None:
            lo, total = int(shard[0]), int(shard[1])
            if lo < 0 or lo + self.shape[0] > total:
                raise ValueError("shard=(lo, total): rows [lo, lo + %d) must lie inside the global batch" % self.shape[0])
        self.row_offset_dev.fill_(lo * self.shape[1] * self.shape[2])
        self.seed_dev.fill_(seed_word(seed))

    def __call__(self, model_inputs=None, unconditional_inputs=None, seed=None, shard=None):
        """Replay. Returns tokens (and the decoded image if a VQGAN was given); outputs live in graph-owned buffers that
        the next replay overwrites.  seed=None draws a fresh seed from torch's CPU generator; the start tokens and all per-step
        noise are functions of the seed and of the GLOBAL row: shard=(lo, total) makes this replay rows [lo, lo + B) of a
        global batch of `total` (bit-identical to those rows of the unsharded call with the same seed).  Conditioning that does not match the captured layout
        raises ValueError before anything is copied: the graph's buffers stay as the last accepted call left them."""
        self._refresh(model_inputs, unconditional_inputs)
        self._set_words(seed, shard)
        self.graph.replay()
        return self.out


class GraphRequestSampler(GraphSampler):
    """`sample_requests` (optionally + the VQGAN decode) captured ONCE per shape and step count and replayed per batch of requests: the seeds, guidance
    pairs and temperatures live in device tables the kernels read, so a replay with other values rewrites the tables and never recaptures (`captures`
    stays 1); GraphSampler's staleness check (weights, precision) applies unchanged.  `cfg` / `temperature` given here are the defaults of a call that
    passes none, and `cfg=None` captures an unguided batch (guidance cannot be switched per replay: it decides the launch sequence).  Replays equal the
    eager `sample_requests` bit for bit.
    max_attn_weights=N (mutually exclusive with `attn_weights`, the one vector baked into the capture): the graph reads a `KeyWeights` table of N weights per
    conditioning slot, and `__call__(attn_weights=...)` rewrites it in place -- None (nobody weighted), one vector for all requests or a list with one entry
    per request, as `sample_requests`; `captures` stays 1.
    filtering=True: the capture holds the logits forward plus the filtered tail and two device tables of per-request filters, every request off until
    `__call__(top_k=, top_p=, typical_mass=, min_tokens=)` (one value or one per request) rewrites them in place; `captures` stays 1."""

    def __init__(self, model, model_inputs, unconditional_inputs, latent_shape, steps=12, renoise_steps=11, temperature=(1.0, 0.2), cfg=8.0, t_start=1.0,
                 t_end=0.0, device="cuda", vqgan=None, attn_weights=None, on_stale="recapture", max_attn_weights=None, filtering=False):
        B = int(latent_shape[0])
        # filtering=True: the capture holds the logits forward plus the filtered tail and two device tables (every request off until a call says otherwise)
        self.filt = FilterTables(request_filters(B), torch.device(device), steps, renoise_steps, linspace_schedule(t_start, t_end, steps + 1)) if filtering else None
        if max_attn_weights is not None:  # (validated before anything touches a device)
            if attn_weights is not None:
                raise ValueError("max_attn_weights (a per-request table) and attn_weights (one vector for the life of the capture) are mutually exclusive")
            check_max_attn_weights(max_attn_weights)
        self.req_defaults = dict(cfg=cfg, temperature=temperature)
        self.req = RequestTables(request_tables(B, steps, [0] * B, cfg, temperature), torch.device(device))
        self.key_weights = None
        if max_attn_weights is not None:
            attn_weights = self.key_weights = KeyWeights(2 * B if self.req.pairs is not None else B, max_attn_weights, device)
        super().__init__(model, model_inputs, unconditional_inputs, latent_shape, steps=steps, renoise_steps=renoise_steps, temperature=temperature, cfg=cfg,
                         t_start=t_start, t_end=t_end, device=device, vqgan=vqgan, attn_weights=attn_weights, on_stale=on_stale)

    def _run(self):
        k = self.kw
        t_list, temps, cfgs = _request_schedule(k["steps"], k["t_start"], k["t_end"], self.req.pairs is not None)
        toks = _sample_core(self.model, self.cond, self.uncond, self.shape, None, k["steps"], k["renoise_steps"], t_list, temps, cfgs, self.device,
                            noise="philox", seed=0, attn_weights=self.attn_weights, init_noise_buf=self.init_noise, r_all=self.r_all, ws=self.ws, req=self.req,
                            filt=self.filt)
        return toks if self.vqgan is None else (toks, self.vqgan.decode_indices(toks, ws=self.vq_ws))

    def __call__(self, seeds, cfg=None, temperature=None, model_inputs=None, unconditional_inputs=None, attn_weights=None, *, top_k=None, top_p=None,
                 typical_mass=None, min_tokens=1):
        """Replay for the requests `seeds[b]` (cfg / temperature: as `sample_requests`; None = the constructor's).  Outputs live in graph-owned buffers that the
        next replay overwrites.  attn_weights (a sampler built with max_attn_weights only): this replay's prompt weights, as `sample_requests` takes them; None =
        nobody is weighted.  top_k / top_p / typical_mass / min_tokens (a sampler built with filtering=True only): this replay's filters, as `sample_requests`
        takes them; the tables are rewritten in place, `captures` stays 1."""
        B, H, W = self.shape
        host = request_tables(B, self.kw["steps"], seeds, self.req_defaults["cfg"] if cfg is None else cfg,
                              self.req_defaults["temperature"] if temperature is None else temperature)
        fhost = request_filters(B, top_k, top_p, typical_mass, min_tokens)
        if self.filt is None and fhost[2]:
            raise ValueError("%s per replay needs a sampler built with filtering=True" % _filter_names(top_k, top_p, typical_mass))
        if self.key_weights is None:
            if attn_weights is not None:
                raise ValueError("attn_weights per replay needs a sampler built with max_attn_weights=N (this one baked the constructor's attn_weights into its capture)")
        else:
            shared, pairs = split_request_weights(attn_weights, B)
            guided = self.req.pairs is not None
            _load_key_weights(self.key_weights, [request_weight_pair(shared)] * B if pairs is None else pairs,
                              _request_keys(self.model, H, W, self.cond, self.uncond if guided else None), guided, self.key_weights.pitch)
        self._refresh(model_inputs, unconditional_inputs)
        self.req.load(host)
        if self.filt is not None:
            self.filt.load(fhost)
        self.graph.replay()
        return self.out


# ---------------------------------------------------------------------------------------------------------------- continuous request batching
_IDLE_ROW = (0.0, 1.0, 1.0, 0.0, -1.0)  # what an idle slot runs with: finite, never renoising (tail.hip: request_step_kernel fills the same values)
# pin policy of a slot of an editing stream (tail.hip: request_step_kernel): when the tail re-imposes the slot's known tokens
PIN_POLICY = {"never": 0, "step": 1, "final": 2}


def request_program(steps, renoise_steps=None, temperature=(1.0, 0.2), cfg=8.0, t_start=1.0, t_end=0.0, max_steps=None, *, guided=None):
    """The schedule of ONE request of a `RequestStream` as a HOST table: (program fp32 [max_steps, 5], steps).  Row j = (r_j, temperature_j, cfg_j, 1 - cfg_j,
    t_next_j) is what the request runs its step j with, bit for bit the scalars the scalar samplers compute: r and the temperatures from `linspace_schedule`
    (t_list = linspace(t_start, t_end, steps + 1)); a float `cfg` rounded as `sample()` rounds it (fp32(cfg), fp32(1.0 - cfg), every step), a (start, end) tuple
    as `sample_distributed` does (torch.linspace, 1 - cfg in fp32), None = the pair (1, 0) of a request without guidance; t_next_j = t_list[j + 1] for
    j < renoise_steps (None: steps - 1, as `sample_distributed`), else -1.0 -- a negative threshold never renoises.  Rows from `steps` on are padding (the idle
    values) and never run: the slot's length is `steps`.  max_steps None = steps.
    guided (keyword-only; what `RequestStream.admit` passes): True refuses cfg=None, False refuses any other cfg -- guidance is on for every request of a stream
    or for none.  Raises ValueError unless 1 <= steps <= max_steps, 0 <= renoise_steps and every step temperature > 0."""
    steps = int(steps)
    max_steps = steps if max_steps is None else int(max_steps)
    if not 1 <= steps <= max_steps:
        raise ValueError("a request needs 1 <= steps <= max_steps (steps=%d, max_steps=%d)" % (steps, max_steps))
    renoise_steps = steps - 1 if renoise_steps is None else int(renoise_steps)
    if renoise_steps < 0:
        raise ValueError("renoise_steps must be >= 0")
    is_num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
    if not (isinstance(temperature, (list, tuple)) and len(temperature) == 2 and all(is_num(v) for v in temperature)):
        raise ValueError("temperature must be a (start, end) pair")
    t_list = linspace_schedule(t_start, t_end, steps + 1)
    temps = linspace_schedule(float(temperature[0]), float(temperature[1]), steps)
    if not all(t > 0 for t in temps):
        raise ValueError("every step temperature of a request must be > 0 (temperature 0, the argmax extension, is not offered per request)")
    if guided is not None and bool(guided) != (cfg is not None):
        raise ValueError("guidance is on for every request of a stream or for none: " +
                         ("cfg=None in a guided stream (pass 1.0 for 'no guidance')" if guided else "cfg=%r in an unguided stream (pass cfg=None)" % (cfg,)))
    if cfg is None:
        pairs = [(1.0, 0.0)] * steps
    elif is_num(cfg):
        pairs = [(float(torch.tensor(float(cfg), dtype=torch.float32)), float(torch.tensor(1.0 - float(cfg), dtype=torch.float32)))] * steps
    elif isinstance(cfg, (list, tuple)) and len(cfg) == 2 and all(is_num(v) for v in cfg):
        sched = torch.linspace(cfg[0], cfg[1], steps)
        pairs = [(float(sched[i]), float(1 - sched[i])) for i in range(steps)]
    else:
        raise ValueError("cfg must be None, a float or a (start, end) tuple, got %r" % (cfg,))
    rows = [(t_list[j], temps[j], pairs[j][0], pairs[j][1], t_list[j + 1] if j < renoise_steps else -1.0) for j in range(steps)]
    rows += [_IDLE_ROW] * (max_steps - steps)
    return torch.tensor(rows, dtype=torch.float32), steps


def _cond_layout(inputs):
    """what a conditioning dict looks like per request: key -> None, the trailing shape, or the list of trailing shapes"""
    return {k: (None if inputs.get(k) is None else [tuple(t.shape[1:]) for t in inputs[k]] if isinstance(inputs[k], (list, tuple)) else tuple(inputs[k].shape[1:]))
            for k in ("byt5", "clip", "clip_image")}


def min_attention_keys(cfg, H, W, cond_rows):
    """the shortest key sequence any attention block of a model with constructor arguments `cfg` sees on an H x W token grid when a sample has `cond_rows`
    conditioning rows: self keys of the smallest grid that has an AttnBlock (none without self_attn) + cond_rows; None for a model without attention"""
    p, best = int(cfg["patch_size"]), None
    for l, lc in enumerate(cfg["level_config"]):
        if "A" in lc:
            n = (((H // p) >> l) * ((W // p) >> l) if cfg["self_attn"] else 0) + int(cond_rows)
            best = n if best is None else min(best, n)
    return best


def check_ragged_stream_args(max_cond_rows, n_attn_weights, min_keys):
    """host validation of `RequestStream(max_cond_rows=N)`: N a positive integer; attn_weights (n_attn_weights of them, 0 = none) weigh the LAST keys of every
    request's own key sequence, so they must fit the shortest admissible one (min_keys = `min_attention_keys(..., cond_rows=1)`)"""
    if isinstance(max_cond_rows, bool) or not isinstance(max_cond_rows, int) or max_cond_rows < 1:
        raise ValueError("max_cond_rows must be None or a positive integer, got %r" % (max_cond_rows,))
    if n_attn_weights and min_keys is not None and n_attn_weights > min_keys:
        raise ValueError("attn_weights has %d entries, more than the %d keys of the shortest request a stream with max_cond_rows admits" % (n_attn_weights, min_keys))
    return max_cond_rows


def check_max_attn_weights(n):
    """`max_attn_weights=N` of a stream / a captured request sampler: the row length of its key-weight table, a positive integer"""
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError("max_attn_weights must be None or a positive integer, got %r" % (n,))
    return n


def check_max_regions(n, max_cond_rows, attn_weights, model):
    """`max_regions=R` of a stream: 1 ... 30 region prompts per request, on a ragged stream (the region rows sit behind the base rows of a slot), without the
    stream-wide weight vector (the entry points that take the group tables take prompt weights as a table) and outside the bf16 precision mode"""
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= MAX_REGIONS:
        raise ValueError("max_regions must be None or an integer 1 ... %d, got %r" % (MAX_REGIONS, n))
    if max_cond_rows is None:
        raise ValueError("max_regions needs max_cond_rows: the rows of a request's regions go behind its base rows in a slot of max_cond_rows rows")
    if attn_weights is not None:
        raise ValueError("max_regions excludes the stream-wide attn_weights vector: give prompt weights per request (max_attn_weights=N)")
    if model.get_gemm_precision() == "bf16":
        raise ValueError("max_regions is not offered in the bf16 precision mode (the bf16 attention core has no masked form)")
    return n


def check_request_rows(rows, max_cond_rows, what):
    """a request's conditioning rows (ByT5 length + clip + any number of clip_image) must be 1 ... max_cond_rows"""
    if not 1 <= rows <= max_cond_rows:
        raise ValueError("%s: %d conditioning rows, the stream admits 1 ... %d (max_cond_rows)" % (what, rows, max_cond_rows))
    return rows


class RequestStream(_EngineGraph):
    """Continuous request batching: a fixed-shape batch of B SLOTS whose requests join and leave at step boundaries.  Every request has its own seed, step count,
    renoise count, temperature and guidance schedule, timestep range and optionally its own start tokens (`init_x` with `t_start` -- the denoising part of an
    image-to-image request); ONE captured graph of a single tick (`request_step` -> the stream form of `forward_sample`) is replayed while they come and go.

    `model_inputs` / `unconditional_inputs` given here are EXAMPLES: they fix the conditioning layout and the number of conditioning rows S for the life of the
    stream (callers pad prompts to that S, as they pad a batch).  guided: guidance is on for every request or for none -- it decides the launch sequence.

    Contract: a request admitted to a stream draws, at its step j, exactly the random words of `sample_distributed(..., latent_shape=(1, H, W), init_x=init_x,
    steps=steps, ..., noise="philox", seed=seed)` at step j; and whoever else is in the batch and whatever tick it was admitted at, its tokens at a given slot
    and B are the same bit for bit.  An idle slot costs a full slot of compute: a stream with k of B slots busy runs at the speed of batch B.

    The stream's device state: the in-place token grid and the start-token grid [B, H, W], the 2B-slot (unguided: B-slot) conditioning cache, per slot a program
    (`request_program`), a cursor and a length, the seed words and the flat per-tick tables.  The host mirrors the cursors: no read-back per tick.
    Staleness (as GraphSampler): a changed weight or precision recaptures (on_stale="recapture") or raises (on_stale="raise") while no request is in flight; with
    requests in flight it always raises -- their conditioning was prepared with the old weights; `reset()` abandons them.

    max_cond_rows=N (ragged conditioning; None keeps the strict layout check above): the cache has slots of N rows and `admit` takes ANY request whose conditional
    and unconditional rows (ByT5 length + clip + any number of clip_image) are each 1 ... N -- the two sides need not share a layout, prompts are not padded.  A
    request is prepared straight into its slots at its own length and attends exactly its own rows: its tokens at a given slot do not depend on the lengths of
    its batch-mates.  `attn_weights` longer than the shortest admissible key sequence are refused.

    editing=True (default False: today's launches and state, with or without max_cond_rows): the stream also serves inpainting / outpainting / structural-editing
    requests next to text-to-image ones, in the same batch and the same captured graph.  It then owns two more grids [B, H, W] int64 -- `keep` (1 = regenerate,
    0 = known; all ones for a plain request) and `known` -- and per slot a pin policy (`PIN_POLICY`: never / every step / final step only); its tick is
    `paella_request_step_pin`, which turns the policies into this tick's per-slot flags `pin_on`, plus the pinned stream forward, whose tail writes known[row]
    over the draw wherever the slot's flag is set and keep[row] == 0.  `admit(known=, mask=)` or `admit(image=, mask=)` (encoded with the stream's VQGAN at
    admission) starts the request from `add_noise(known, t_start, mask=mask, random_x=R)`, R the salted Philox start tokens of the request's seed, as
    `paella_amd.inpaint(noise="philox")` does.  Contract: an editing request with pin="final" produces the tokens of `inpaint(..., keep_known=True, noise="philox",
    seed=seed, decode=False)` at batch 1, with pin="step" those of `inpaint(..., pin="step", ...)` (both for a stream of B = 1; the logits of a larger B may differ
    in their last bits, as for every request of a stream); in both cases the tokens at a given slot and B are independent of the batch-mates and of the admission
    tick, bit for bit.  `captures` stays 1 while text-to-image and editing requests of either policy come and go.

    max_attn_weights=N (per-request prompt weights; mutually exclusive with the stream-wide `attn_weights`, which stays one vector for the life of the stream):
    the stream owns a `KeyWeights` table -- N weights per conditioning slot, 2B slots when guided, so the two sides of a request carry independent rows -- that
    the tick reads, and `admit(attn_weights=)` takes None, one vector for both sides or a pair (conditional, unconditional), either member None.  Every admit
    writes both of its slots' rows, count 0 included: a slot never inherits its predecessor's weights; `reset()` zeroes the counts.  A vector longer than N, or
    longer than that side's own shortest key sequence, is refused at admission.  Contract: a request admitted with weights `w` produces, at a given slot and B,
    exactly the tokens of a stream of the same shape built with stream-wide `attn_weights=w` serving that request -- bit for bit, independent of its
    batch-mates' weights and of the tick it joined at.  With editing and / or max_cond_rows as well it is still one tick, one graph: `captures` stays 1.

    filtering=True (truncated sampling; default False: exactly the entry points of today): the stream owns the two filter tables (int32 [B, 2] = (top_k, min_tokens),
    fp32 [B, 2] = (top_p, typical_mass), every slot off) and a [B, H, W, num_labels] logits buffer; its captured tick is `request_step` -> the logits forward (guidance
    folded through the head) -> the filtered stream tail, and `admit(top_k=, top_p=, typical_mass=, min_tokens=)` writes the slot's row, "off" included, so a slot
    never inherits its predecessor's filter; `reset()` writes off everywhere.  A request admitted with a filter produces, at a given slot and B, the same tokens whatever
    its batch-mates carry and whatever tick it joined at; one admitted with every filter off produces the tokens of a filtering=False stream (fused == unfused).  The
    price is the materialised logits: B * H * W * num_labels * 4 bytes written and read back per tick.  Editing, max_cond_rows and prompt weights combine unchanged.

    max_regions=R (regional prompts, 1 ... 30; needs max_cond_rows, and excludes the stream-wide `attn_weights` vector -- use max_attn_weights): the stream owns a
    `RegionTables` for its conditioning slots and its tick -- fused or filtered -- runs the masked attention kernels through the `_rg` entry points.
    `admit(regions=[(inputs_r, mask_r), ...])` gives the request up to R more prompts next to `model_inputs`, which stays the base prompt, visible everywhere:
    region r's rows are prepared into the conditional slot behind the base rows (and behind the regions before it), carry group bit r + 1, and are visible to the
    positions of every level whose patch * 2^level block of token positions touches mask_r (`region_query_groups`).  Base rows, every row of the unconditional
    side and every query carry bit 0.  Base + region rows must fit max_cond_rows.  Every admit writes both of its slots' rows of both tables, the all-visible
    default included, so a slot never inherits its predecessor's regions; `reset()` restores the default.  Contracts: a request's tokens at a given slot and B do
    not depend on its batch-mates' regions or on the tick it joined at; a request admitted with regions=None produces the tokens of the same stream built
    without max_regions; a region whose mask is all zero changes nothing.  `captures` stays 1.  Not offered in the bf16 precision mode.

    confidence=True (confidence-ordered renoise and statistics maps; default False: today's entry points and state): the stream owns policy int32 [B] and
    confidence_noise fp32 [B] (every slot random), the logprob / entropy maps fp32 [B, H, W] and a [B, H, W, num_labels] logits buffer; its captured tick is
    `request_step[_pin]` -> the logits forward -> the statistics tail (the filtered tail's draw plus the two maps; no renoise, no pin) -> the renoise stage, which
    renoises every slot by its own policy and applies the pin.  `admit(renoise=, confidence_noise=)` writes the slot's row of both tables every time, the random
    default included, so a slot never inherits its predecessor's policy; `reset()` writes the default everywhere; `result(slot, stats=True)` also returns the slot's
    maps of its final draw.  A request's tokens and maps at a given slot and B do not depend on its batch-mates' policies or on the tick it joined at; a
    renoise="random" request produces the tokens of a confidence=False stream.  Editing, filtering, max_cond_rows, max_attn_weights and max_regions combine unchanged."""

    def __init__(self, model, model_inputs, unconditional_inputs, latent_shape, max_steps=12, guided=True, device="cuda", vqgan=None, attn_weights=None,
                 on_stale="recapture", max_cond_rows=None, editing=False, max_attn_weights=None, filtering=False, max_regions=None, confidence=False):
        self._init_owner(on_stale)
        if not isinstance(model, Paella):
            raise TypeError("RequestStream needs a paella_amd.Paella model")
        self.model, self.vqgan, self.device = model, vqgan, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("paella_amd.RequestStream runs on a HIP device only (got device=%s); there is no CPU path" % self.device)
        self.shape = tuple(int(v) for v in latent_shape)
        B, H, W = self.shape
        self.max_steps, self.guided, self.attn_weights = int(max_steps), bool(guided), attn_weights
        if max_attn_weights is not None and attn_weights is not None:
            raise ValueError("max_attn_weights (per-request weights, given to admit) and attn_weights (one vector for the life of the stream) are mutually exclusive")
        self.max_attn_weights = None if max_attn_weights is None else check_max_attn_weights(max_attn_weights)
        self.max_regions = None if max_regions is None else check_max_regions(max_regions, max_cond_rows, attn_weights, model)
        if B <= 0 or self.max_steps <= 0:
            raise ValueError("a request stream needs B > 0 and max_steps > 0")
        if model_inputs is None or (self.guided and unconditional_inputs is None):
            raise TypeError("a %s stream needs model_inputs%s" % ("guided" if self.guided else "unguided", " and unconditional_inputs" if self.guided else ""))
        self.layout = _cond_layout(model_inputs)
        self.max_cond_rows = max_cond_rows
        if max_cond_rows is not None:
            check_ragged_stream_args(max_cond_rows, 0 if attn_weights is None else int(attn_weights.numel()), min_attention_keys(model._cfg, H, W, 1))
            for inputs, what in ((model_inputs, "model_inputs"), (unconditional_inputs, "unconditional_inputs"))[:2 if self.guided else 1]:
                check_request_rows(_cond_seq_len(model, inputs), max_cond_rows, what)
            self.S = max_cond_rows
        else:
            if self.guided and _cond_layout(unconditional_inputs) != self.layout:
                raise ValueError("the conditional and unconditional inputs of a guided stream must share one layout (they are evaluated as one 2B-row batch)")
            self.S = _cond_seq_len(model, model_inputs)
        if self.S <= 0:
            raise ValueError("conditioning sequence is empty")
        dev, nb = self.device, (2 * B if self.guided else B)
        self._slot_bytes = model.cond_bytes(1, self.S)
        # (zero K/V rows: finite work for slots never filled; a ragged stream's never-filled slots attend all N of them)
        lens = None if max_cond_rows is None else torch.full((nb,), self.S, dtype=torch.int32, device=dev)
        self.cache = CondCache(torch.zeros(nb * self._slot_bytes, dtype=torch.uint8, device=dev), nb, self.S, lens)
        assert self.cache.buf.numel() == model.cond_bytes(nb, self.S)
        self.tokens = torch.zeros(self.shape, dtype=torch.int64, device=dev)    # the in-place grid: a tick reads and writes it
        self.random_x = torch.zeros(self.shape, dtype=torch.int64, device=dev)  # per slot the start tokens of its seed: the renoise source
        self.seeds = torch.zeros(B, dtype=torch.int64, device=dev)
        self.program = torch.tensor(_IDLE_ROW, dtype=torch.float32).repeat(B, self.max_steps, 1).to(dev)
        self.pos = torch.zeros(B, dtype=torch.int32, device=dev)
        self.len = torch.zeros(B, dtype=torch.int32, device=dev)
        self.r = torch.zeros(B, dtype=torch.float32, device=dev)
        self.temps = torch.ones(B, dtype=torch.float32, device=dev)
        self.pairs = torch.tensor([1.0, 0.0]).repeat(B, 1).to(dev) if self.guided else None
        self.t_next = torch.full((B,), -1.0, dtype=torch.float32, device=dev)
        self.step = torch.zeros(B, dtype=torch.int32, device=dev)
        self.active_dev = torch.zeros(B, dtype=torch.int32, device=dev)
        self._pos, self._len, self._held = [0] * B, [0] * B, [False] * B  # host mirror: cursor, length, slot taken (admitted and not yet collected)
        self.editing = bool(editing)
        self.keep = self.known = self.pin_policy = self.pin_on = None
        if self.editing:
            self.keep = torch.ones(self.shape, dtype=torch.int64, device=dev)    # 1 = regenerate, 0 = known (the project's mask type)
            self.known = torch.zeros(self.shape, dtype=torch.int64, device=dev)
            self.pin_policy = torch.zeros(B, dtype=torch.int32, device=dev)      # PIN_POLICY per slot
            self.pin_on = torch.zeros(B, dtype=torch.int32, device=dev)          # this tick's flags, written by the step kernel
        # per-request prompt weights: one row per conditioning slot, all counts 0 until a request brings weights; the tick reads the table instead of a vector
        self.key_weights = None if self.max_attn_weights is None else KeyWeights(nb, self.max_attn_weights, dev)
        if self.key_weights is not None:
            self.attn_weights = self.key_weights
        # regional prompts: the key-group tables are stream state (everything visible until a request brings regions); the tick reads them through the _rg entry points
        self.regions = None if self.max_regions is None else RegionTables(nb, region_query_total(model._cfg, H, W), self.S, dev)
        # truncated sampling: the filter tables are stream state (every slot off), and the tick materialises the logits for the filtered stream tail
        self.filtering = bool(filtering)
        self.filter_k = self.filter_mass = self.logits = None
        if self.filtering:
            self.filter_k = torch.tensor([FILTER_OFF[0], FILTER_OFF[3]], dtype=torch.int32).repeat(B, 1).to(dev)
            self.filter_mass = torch.tensor([FILTER_OFF[1], FILTER_OFF[2]], dtype=torch.float32).repeat(B, 1).to(dev)
            self.logits = torch.empty(B, H, W, model.num_labels, dtype=torch.float32, device=dev)
        # confidence-ordered renoise: the policy tables and the statistics maps are stream state (every slot random); the tick materialises the logits as well
        self.confidence = bool(confidence)
        self.policy = self.confidence_noise = self.logprob = self.entropy = self._never = None
        if self.confidence:
            self.policy = torch.zeros(B, dtype=torch.int32, device=dev)
            self.confidence_noise = torch.zeros(B, dtype=torch.float32, device=dev)
            self.logprob, self.entropy = (torch.zeros(self.shape, dtype=torch.float32, device=dev) for _ in range(2))
            self._never = torch.full((B,), -1.0, dtype=torch.float32, device=dev)  # the threshold table of the statistics tail: the renoise stage renoises
            if self.logits is None:
                self.logits = torch.empty(B, H, W, model.num_labels, dtype=torch.float32, device=dev)
        self._capture()

    # ---- slots
    @property
    def free_slots(self):
        """slots that hold no request (neither running nor finished and waiting for `result`)"""
        return [b for b, held in enumerate(self._held) if not held]

    @property
    def active(self):
        """slots whose request still has steps to run"""
        return [b for b in range(self.shape[0]) if self._held[b] and self._pos[b] < self._len[b]]

    # ---- one tick on the current stream: the launches the graph holds
    def _tick_launches(self):
        B = self.shape[0]
        tables = (_lib.ptr(self.program), self.max_steps, _lib.ptr(self.pos), _lib.ptr(self.len), B, _lib.ptr(self.r), _lib.ptr(self.temps), _lib.ptr(self.pairs),
                  _lib.ptr(self.t_next), _lib.ptr(self.step), _lib.ptr(self.active_dev))
        with torch.cuda.device(self.device):
            if self.editing:
                _lib.check(_lib.load().paella_request_step_pin(*tables, _lib.ptr(self.pin_policy), _lib.ptr(self.pin_on), _lib.stream_ptr(self.device)))
            else:
                _lib.check(_lib.load().paella_request_step(*tables, _lib.stream_ptr(self.device)))
        pin = (self.keep, self.known, self.pin_on) if self.editing else None
        if not (self.confidence or self.filtering):
            # in place: the token gather at the head of the forward and the token store at its tail are different kernels of one stream (as in _sample_core)
            self.model.forward_sample(self.tokens, self.r, self.cache, self.tokens, temperature=1.0, init_noise=self.random_x, attn_weights=self.attn_weights, ws=self.ws,
                                      req=(self.seeds, self.temps, self.pairs), stream=(self.step, self.t_next, self.active_dev),
                                      **({} if pin is None else {"pin": pin}), **({} if self.regions is None else {"regions": self.regions}))
            return
        # the logits forward (the guidance mix folded through the head: ONE [rows, L] tensor), then in place as above the filtered stream tail, the pin riding in it --
        # or, in a confidence stream, the statistics tail (raw draw, no pin) + the renoise stage (every slot's own policy, then the pin)
        self.model.forward_prepared(self.tokens, self.r, self.cache, attn_weights=self.attn_weights, out=self.logits, ws=self.ws,
                                    **({} if self.pairs is None else {"req_mix": self.pairs}), **({} if self.regions is None else {"regions": self.regions}))
        hw = self.shape[1] * self.shape[2]
        _stream_draw(self.logits, None, B * hw, self.model.num_labels, self.tokens, (None, self.temps, self.seeds, hw), self.step, self.t_next, self.active_dev,
                     self.random_x, (self.filter_k, self.filter_mass), pin=pin,
                     conf=(self._never, self.policy, self.confidence_noise, self.logprob, self.entropy) if self.confidence else None)

    def _capture(self):
        """only with no request in flight: every slot is then idle on the device, and an idle tick stores nothing and moves no cursor -- the warm-up ticks and the
        capture itself leave the state (finished tokens waiting for `result` included) as it is"""
        assert not self.active
        B, H, W = self.shape
        self.graph = None
        self.ws = _lib.new_workspace(self.model.workspace_bytes(self.cache.B, H, W, self.S), self.device)
        self.vq_ws = None if self.vqgan is None else _lib.new_workspace(self.vqgan.workspace_bytes(1, H, W), self.device)
        self._capture_graph(torch.inference_mode()(self._tick_launches))

    def _refuse_recapture(self, causes):
        if self.active:
            raise RuntimeError("RequestStream: %s changed with %d request(s) in flight -- their conditioning was prepared with the old state; let the stream run "
                               "empty before load_state_dict / set_gemm_precision, or abandon them with reset()" % (", ".join(causes), len(self.active)))

    # ---- requests
    def _check_inputs(self, inputs, what):
        if self.max_cond_rows is not None:
            if inputs is None:
                raise ValueError("%s: missing" % what)
            check_request_rows(_cond_seq_len(self.model, inputs), self.max_cond_rows, what)
        elif inputs is None or _cond_layout(inputs) != self.layout:
            raise ValueError("%s: conditioning layout or sequence length differs from the stream's (%r)" % (what, self.layout))
        for k in ("byt5", "clip", "clip_image"):
            v = inputs.get(k)
            for t in ([] if v is None else v if isinstance(v, (list, tuple)) else [v]):
                if t.size(0) != 1:
                    raise ValueError("%s: admit takes the inputs of ONE request (leading dimension 1), got %d for %s" % (what, t.size(0), k))

    def _check_edit(self, known, mask, image, pin):
        """the editing arguments of `admit`, validated before anything touches the stream: (known or image, mask int64 0/1) on the device, or (None, None)"""
        B, H, W = self.shape
        if pin not in PIN_POLICY or pin == "never":
            raise ValueError("pin must be 'step' or 'final', got %r" % (pin,))
        if known is None and mask is None and image is None:
            return None, None, None
        if not self.editing:
            raise ValueError("known / mask / image need an editing stream: construct RequestStream(..., editing=True)")
        if image is not None and known is not None:
            raise ValueError("image and known are mutually exclusive (image is encoded into known at admission)")
        if mask is None or (known is None and image is None):
            raise ValueError("an editing request needs a mask together with known tokens or an image (got %s)" % ("a mask alone" if mask is not None else "no mask"))
        if not torch.is_tensor(mask) or tuple(mask.shape) != (H, W) or mask.dtype.is_floating_point or mask.dtype.is_complex:
            raise ValueError("mask must be an integer or bool tensor [%d, %d] on the token grid (1 = regenerate)" % (H, W))
        if known is not None and (not torch.is_tensor(known) or tuple(known.shape) != (H, W) or known.dtype != torch.int64):
            raise ValueError("known must be an int64 tensor [%d, %d]" % (H, W))
        if image is not None:
            if self.vqgan is None:
                raise ValueError("image= needs a stream with a VQGAN (RequestStream(..., vqgan=...)): it is encoded at admission")
            f = 2 ** self.vqgan.levels
            if not torch.is_tensor(image) or tuple(image.shape) != (3, f * H, f * W) or image.dtype != torch.float32:
                raise ValueError("image must be an fp32 tensor [3, %d, %d] in [0, 1]" % (f * H, f * W))
        return known, (mask != 0).to(device=self.device, dtype=torch.int64), image

    def _check_weights(self, attn_weights, model_inputs, unconditional_inputs):
        """the `attn_weights` of `admit`, validated before anything touches the stream -> (conditional, unconditional) vectors or None each"""
        if self.key_weights is None:
            if attn_weights is not None:
                raise ValueError("attn_weights per request need a stream built with max_attn_weights=N (this one has %s)" %
                                 ("no prompt weights" if self.attn_weights is None else "one stream-wide attn_weights vector"))
            return None
        H, W = self.shape[1:]
        rows = lambda inputs: _cond_seq_len(self.model, inputs) if self.max_cond_rows is not None else self.S
        keys = (min_attention_keys(self.model._cfg, H, W, rows(model_inputs)), min_attention_keys(self.model._cfg, H, W, rows(unconditional_inputs)) if self.guided else None)
        return check_weight_pair(request_weight_pair(attn_weights), keys, self.guided, self.max_attn_weights)

    def _check_regions(self, regions, model_inputs):
        """the `regions` of `admit`, validated before anything touches the stream -> [(inputs_r, rows_r)], bool masks [R, H, W] on the host (None, None without)"""
        if regions is None:
            return None, None
        B, H, W = self.shape
        if self.max_regions is None:
            raise ValueError("regions need a stream built with max_regions=R (and max_cond_rows)")
        if self.model.get_gemm_precision() == "bf16":
            raise ValueError("regions are not offered in the bf16 precision mode")
        regions = list(regions)
        if len(regions) > self.max_regions:
            raise ValueError("regions: %d given, the stream admits at most %d (max_regions)" % (len(regions), self.max_regions))
        total, plan, masks = _cond_seq_len(self.model, model_inputs), [], []
        for i, item in enumerate(regions):
            if not isinstance(item, (tuple, list)) or len(item) != 2 or not isinstance(item[0], dict):
                raise ValueError("regions: entry %d must be a pair (inputs, mask)" % i)
            inputs, m = item
            if not torch.is_tensor(m) or tuple(m.shape) != (H, W) or m.dtype.is_floating_point or m.dtype.is_complex:
                raise ValueError("regions: the mask of region %d must be an integer or bool tensor [%d, %d] on the token grid (1 = the prompt applies here)" % (i, H, W))
            for k in ("byt5", "clip", "clip_image"):
                v = inputs.get(k)
                for t in ([] if v is None else v if isinstance(v, (list, tuple)) else [v]):
                    if t.size(0) != 1:
                        raise ValueError("regions: region %d takes the inputs of ONE prompt (leading dimension 1), got %d for %s" % (i, t.size(0), k))
            rows = _cond_seq_len(self.model, inputs)
            if rows < 1:
                raise ValueError("regions: region %d has no conditioning rows" % i)
            total += rows
            plan.append((inputs, rows))
            masks.append((m != 0).cpu())
        if total > self.max_cond_rows:
            raise ValueError("regions: %d base + region conditioning rows, the stream's slots hold %d (max_cond_rows)" % (total, self.max_cond_rows))
        return plan, (torch.stack(masks) if masks else torch.zeros(0, H, W, dtype=torch.bool))

    def admit(self, model_inputs, unconditional_inputs=None, seed=None, steps=12, renoise_steps=None, temperature=(1.0, 0.2), cfg=8.0, t_start=1.0, t_end=0.0,
              init_x=None, known=None, mask=None, image=None, pin="step", attn_weights=None, *, top_k=None, top_p=None, typical_mass=None, min_tokens=1, regions=None,
              renoise="random", confidence_noise=0.0):
        """Put ONE request into a free slot; it runs from the next tick on.  Inputs: leading dimension 1, the stream's layout.  Schedule arguments as
        `request_program` (an unguided stream takes cfg=None); init_x int64 [H, W]: the tokens the request starts from instead of its seed's start tokens.
        Everything here is eager work on the current stream, ordered before the next tick: the conditioning of the one request is prepared straight into the
        slot's rows of the cache.  Raises RuntimeError when no slot is free.  Returns the slot.
        Editing stream: known int64 [H, W] tokens (or image fp32 [3, f*H, f*W] in [0, 1], encoded here with the stream's VQGAN) and mask [H, W] on the token grid
        (1 = regenerate) make this an editing request -- unless init_x is given it starts from add_noise(known, t_start, mask=mask, random_x=R), R the salted Philox
        start tokens of `seed`; pin="step" re-imposes the known tokens after every step, pin="final" after the request's last step only.  A request without them
        is a plain one: policy never, keep = ones.
        attn_weights (a stream built with max_attn_weights): this request's prompt weights -- None, one 1-D tensor for both sides, or a pair (conditional,
        unconditional), either member None; written to the request's two rows of the stream's table (count 0 for an unweighted side).
        top_k / top_p / typical_mass / min_tokens (a stream built with filtering=True): this request's truncation filter (`check_filter`); every admit writes its
        slot's row of the stream's filter tables, "off" included.
        regions (a stream built with max_regions): [(inputs_r, mask_r), ...] -- more prompts of this request, each a conditioning dict of ONE prompt and a bool /
        integer mask [H, W] (1 = the prompt applies here); `model_inputs` stays the base prompt, visible everywhere.  Masks may overlap; an all-zero mask is a
        no-op.  The unconditional side is never regional.
        renoise / confidence_noise (`check_renoise`; renoise="confidence" needs a stream built with confidence=True): this request's renoise policy; every admit
        writes its slot's row of the stream's two tables, the random default included."""
        B, H, W = self.shape
        region_plan, region_masks = self._check_regions(regions, model_inputs)
        known, mask, image = self._check_edit(known, mask, image, pin)
        filt = check_filter(top_k, top_p, typical_mass, min_tokens)
        if filter_on(filt) and not self.filtering:
            raise ValueError("%s needs a stream built with filtering=True (this one runs the fused tail, which sees no whole row)" % _filter_names(top_k, top_p, typical_mass))
        policy, conf_g = check_renoise(renoise, confidence_noise)
        if policy and not getattr(self, "confidence", False):
            raise ValueError("renoise='confidence' needs a stream built with confidence=True (this one renoises inside its tail, one coin per position)")
        program, n = request_program(steps, renoise_steps, temperature, cfg, t_start, t_end, max_steps=self.max_steps, guided=self.guided)
        self._check_inputs(model_inputs, "model_inputs")
        if self.guided:
            self._check_inputs(unconditional_inputs, "unconditional_inputs")
        weights = self._check_weights(attn_weights, model_inputs, unconditional_inputs)
        if init_x is not None:
            init_x = init_x.reshape(H, W) if torch.is_tensor(init_x) and init_x.numel() == H * W else init_x
            if not torch.is_tensor(init_x) or tuple(init_x.shape) != (H, W) or init_x.dtype != torch.int64:
                raise ValueError("init_x must be an int64 tensor [%d, %d]" % (H, W))
        free = self.free_slots
        if not free:
            raise RuntimeError("RequestStream: no free slot (%d running, %d finished and waiting for result())" % (len(self.active), B - len(self.active)))
        self._check_fresh()
        if seed is None:
            seed = fresh_seed()
        b, nbytes = free[0], self._slot_bytes
        with torch.inference_mode():
            # the conditioning GEMMs run on the TICK's workspace (self.ws, whose split-K tickets the captured graph also uses).  That is safe on two grounds: admit and
            # every replay are enqueued on the same (current) stream, so the two users never run concurrently and each launch leaves the tickets zero; and the
            # workspace was sized for the 2B-row forward, which covers the conditioning preparation of one request (prepare_cond checks the size and raises otherwise)
            for row, inputs in ((b, model_inputs), (B + b, unconditional_inputs))[:2 if self.guided else 1]:
                # ragged stream: at the request's own length into the front of its slot, and its `lens` entry with it (stream-ordered before the next tick)
                slot = {} if self.cache.lens is None else dict(slot_rows=self.S, lens_out=self.cache.lens[row:row + 1])
                self.model.prepare_cond(**{k: inputs.get(k) for k in ("byt5", "clip", "clip_image")}, ws=self.ws, out=self.cache.buf[row * nbytes:(row + 1) * nbytes],
                                        **slot)
            if self.regions is not None:  # both slots' rows of both tables, the all-visible default included: nothing is inherited
                k_row = None
                if region_plan:
                    # region r's rows behind the base rows (and the regions before it): the preparation writes S rows from ANY row offset of the slot, and the slot's
                    # count becomes the total.  Conditioning rows are per-row functions of their inputs, so these are the rows of the prompt prepared alone
                    row_bytes, off = nbytes // self.S, _cond_seq_len(self.model, model_inputs)
                    k_row = [1] * off
                    scratch_len = torch.zeros(1, dtype=torch.int32, device=self.device)
                    for i, (inputs, rows) in enumerate(region_plan):
                        self.model.prepare_cond(**{k: inputs.get(k) for k in ("byt5", "clip", "clip_image")}, ws=self.ws,
                                                out=self.cache.buf[b * nbytes + off * row_bytes:b * nbytes + (off + rows) * row_bytes], slot_rows=rows, lens_out=scratch_len)
                        k_row += [1 << (i + 1)] * rows
                        off += rows
                    self.cache.lens[b].fill_(off)
                    k_row = torch.tensor(k_row, dtype=torch.int32)
                self.regions.set(b, None if not region_plan else region_query_groups(region_masks, self.model._cfg, H, W), k_row)
                if self.guided:
                    self.regions.set(B + b)
            start_tokens(self.model.num_labels, (1, H, W), seed, self.device, out=self.random_x[b:b + 1])
            if self.key_weights is not None:  # both rows, count 0 included: the slot's previous request leaves nothing behind
                self.key_weights.set(b, weights[0])
                if self.guided:
                    self.key_weights.set(B + b, weights[1])
            if self.filtering:  # the slot's row, "off" included: its previous request leaves nothing behind
                self.filter_k[b].copy_(torch.tensor([filt[0], filt[3]], dtype=torch.int32))
                self.filter_mass[b].copy_(torch.tensor([filt[1], filt[2]], dtype=torch.float32))
            if self.confidence:  # the slot's row, the random default included: its previous request leaves nothing behind
                self.policy[b].fill_(policy)
                self.confidence_noise[b].fill_(conf_g)
            if self.editing:
                if mask is None:
                    self.keep[b].fill_(1)
                    self.pin_policy[b].fill_(PIN_POLICY["never"])
                else:
                    if image is not None:
                        known = self.vqgan.encode(image[None].to(self.device), ws=self.vq_ws)[2][0]
                    self.known[b].copy_(known)
                    self.keep[b].copy_(mask)
                    self.pin_policy[b].fill_(PIN_POLICY[pin])
                    if init_x is None:  # what inpaint(noise="philox") starts a batch of one from (editing.py: _philox_random_x)
                        from .editing import RANDOM_X_SALT
                        rx = start_tokens(self.model.num_labels, (1, H, W), (int(seed) + RANDOM_X_SALT) & 0xFFFFFFFFFFFFFFFF, self.device)
                        init_x = self.model.add_noise(self.known[b:b + 1], torch.full((1,), float(t_start), device=self.device), mask=self.keep[b:b + 1], random_x=rx)[0][0]
            self.tokens[b].copy_(self.random_x[b] if init_x is None else init_x)
            self.seeds[b].fill_(seed_word(seed))
            self.program[b].copy_(program)
            self.len[b].fill_(n)
            self.pos[b].fill_(0)
        self._pos[b], self._len[b], self._held[b] = 0, n, True
        return b

    def reset(self):
        """Abandon every request the stream holds, running or finished: all slots become free and idle (cursors and lengths zeroed on the device, stream-ordered
        before the next tick); nothing is returned for them.  The way out after a weight or precision change with requests in flight -- the next admit / tick then
        finds the stream empty and recaptures (or raises, with on_stale="raise")."""
        B = self.shape[0]
        self.len.zero_()
        self.pos.zero_()
        if self.editing:
            self.pin_policy.zero_()
        if self.key_weights is not None:
            self.key_weights.clear()
        if self.regions is not None:
            self.regions.clear()
        if self.filtering:
            self.filter_k[:, 0].fill_(FILTER_OFF[0])
            self.filter_k[:, 1].fill_(FILTER_OFF[3])
            self.filter_mass.fill_(1.0)
        if self.confidence:
            self.policy.zero_()
            self.confidence_noise.zero_()
        self._pos, self._len, self._held = [0] * B, [0] * B, [False] * B

    def tick(self, graph=True):
        """One denoising step of every running request (one graph replay; graph=False: the same launches eagerly).  Returns the slots whose request finished with
        this tick -- collect them with `result`.  With no running request nothing is launched."""
        running = self.active
        if not running:
            return []
        self._check_fresh()
        if graph:
            self.graph.replay()
        else:
            with torch.inference_mode():
                self._tick_launches()
        done = []
        for b in running:
            self._pos[b] += 1
            if self._pos[b] == self._len[b]:
                done.append(b)
        return done

    def result(self, slot, stats=False):
        """The finished request of `slot`: its tokens [H, W] (a clone), with a VQGAN (tokens, image [3, f*H, f*W]) -- an eager decode of the one slot.  Frees the slot.
        stats=True (a stream built with confidence=True): the slot's {"logprob", "entropy"} maps fp32 [H, W] of its final draw (clones) come last in the result."""
        slot = int(slot)
        if not (0 <= slot < self.shape[0]) or not self._held[slot]:
            raise ValueError("slot %d holds no request" % slot)
        if self._pos[slot] < self._len[slot]:
            raise RuntimeError("the request of slot %d has %d step(s) to run" % (slot, self._len[slot] - self._pos[slot]))
        if stats and not self.confidence:
            raise ValueError("stats=True needs a stream built with confidence=True")
        toks = self.tokens[slot].clone()
        maps = ({"logprob": self.logprob[slot].clone(), "entropy": self.entropy[slot].clone()},) if stats else ()
        self._held[slot] = False
        if self.vqgan is None:
            return (toks, *maps) if maps else toks
        with torch.inference_mode():
            return (toks, self.vqgan.decode_indices(toks[None], ws=self.vq_ws)[0].clone(), *maps)

    def drain(self, requests, graph=True):
        """Serve an iterable of requests (keyword dicts for `admit`): admit as slots free up, tick until everything is collected; yields (index, tokens) -- with a
        VQGAN (index, tokens, image) -- in completion order.  The stream must be empty: a request admitted outside this call would finish among its ticks."""
        if any(self._held):
            raise RuntimeError("RequestStream.drain needs an empty stream (%d slot(s) hold requests admitted elsewhere: collect them with result() first)" % sum(self._held))
        it, index_of, more = iter(enumerate(requests)), {}, True
        while True:
            while more and self.free_slots:
                nxt = next(it, None)
                if nxt is None:
                    more = False
                else:
                    index_of[self.admit(**nxt[1])] = nxt[0]
            if not index_of:
                return
            for b in self.tick(graph=graph):
                res = self.result(b)
                yield (index_of.pop(b), *res) if isinstance(res, tuple) else (index_of.pop(b), res)

"""`Paella` -- the denoising UNet of dome272/Paella, executed by hand-written HIP kernels on MI355X.

This module is the host-side mirror of the reference's `src/modules.py` (class `Paella`, :109-283; kwargs /
list-valued `clip_image` superset of `utils/modules.py`; `get_loss_weight` of `src_distributed/modules.py:283`).
It keeps the constructor, `forward`, `add_noise`, `gen_r_embedding`, `gen_c_embeddings` signatures and the exact
state-dict key names, so reference checkpoints load unchanged -- but it contains no arithmetic: parameters are
plain `nn.Parameter` holders, and every call goes through the C ABI of libpaella_hip.so (include/paella_hip.h).
There is no CPU / eager fallback: using the module off a HIP device raises.

Beyond the reference surface it exposes the two calls `sample()` uses to hoist step-invariant work:
`prepare_cond()` (conditioning embeddings + per-AttnBlock K/V of the conditioning rows, once per sample() call)
and `forward_prepared()` (one denoising evaluation against that cache).
"""
import ctypes
import itertools
import math

import torch
from torch import nn
from torch.nn.modules import module as _nn_module

from . import _lib
from .training import TRAIN_SWITCHES

_TRAIN_SWITCH = {sw.name: sw for sw in TRAIN_SWITCHES}


# Every registration of a Parameter, buffer or child module on ANY nn.Module of the process counts here (torch's process-wide registration hooks: they fire for
# `holder.weight = nn.Parameter(t)`, `register_parameter` / `register_buffer`, and `load_state_dict(assign=True)`, which assigns).  `_NativeModel._signature`
# compares the count with the one it saw when it listed its tensors, so a swapped tensor OBJECT is noticed for one integer compare per call.
_REGISTRATIONS = [0]
# Load generations: every (re)load of a native model draws the next one, so a generation names one load of one module ("Load generation").
_LOAD_GENS = itertools.count(1)


def _count_registration(module, name, value):
    _REGISTRATIONS[0] += 1


_nn_module.register_module_parameter_registration_hook(_count_registration)
_nn_module.register_module_buffer_registration_hook(_count_registration)
_nn_module.register_module_module_registration_hook(_count_registration)


class _NativeModel:
    """What `Paella` and `VQModel` share around their native handle (mixed in before nn.Module): the engine's life -- created on first use, reloaded when the
    weight signature changed, switched between the precision modes, destroyed with the module -- its scratch workspace, the weight signature, `refresh()`, and
    copy / pickle semantics.  A class brings `_abi`, the prefix of its entry-point family in libpaella_hip.so, `_device()`, where its device is read from, and
    `_create()`, which makes the native model from the class's configuration."""

    _abi = None

    def _init_engine(self):
        """no native model yet: `_engine()` builds it on first use"""
        self._handle = None
        self._loaded_sig = None
        self._load_gen = 0
        self._ws = None
        self._precision = 0

    def _native(self, name):
        """the entry point `<_abi>_<name>` of the library"""
        return getattr(_lib.load(), "%s_%s" % (self._abi, name))

    def _require_hip(self):
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("paella_amd.%s executes only on a HIP device (module is on '%s'); move it with .to('cuda'). There is no CPU fallback."
                               % (type(self).__name__, dev))
        return dev

    def _engine(self):
        """Create / refresh the native model: (re)load every tensor when parameters moved or changed."""
        dev = self._require_hip()
        _lib.load()
        sig = self._signature()
        if self._handle is not None and sig == self._loaded_sig:
            return self._handle
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            if self._handle is None:
                self._handle = self._create()
                if self._precision:
                    _lib.check(self._native("set_precision")(self._handle, self._precision, st))
            load_tensor = self._native("load_tensor")
            for key, t in self.state_dict().items():
                if key.endswith("num_batches_tracked"):  # (torch's BatchNorm counter: no weight)
                    continue
                t = t.detach()
                if t.dtype != torch.float32 or not t.is_contiguous():
                    t = t.float().contiguous()
                shape = (ctypes.c_int64 * t.dim())(*t.shape)
                _lib.check(load_tensor(self._handle, key.encode(), _lib.ptr(t), shape, t.dim(), st))
            _lib.check(self._native("finalize")(self._handle, st))
            torch.cuda.current_stream(dev).synchronize()  # staging copies above may be temporaries
        self._loaded_sig = sig
        self._load_gen = next(_LOAD_GENS)
        return self._handle

    def set_gemm_precision(self, mode):
        modes = {"fp32": 0, "f32": 0, "bf16": 1}
        if mode not in modes:
            raise ValueError("gemm precision must be 'fp32' or 'bf16'")
        self._precision = modes[mode]
        if self._handle is not None:
            dev = self._require_hip()
            with torch.cuda.device(dev):
                _lib.check(self._native("set_precision")(self._handle, self._precision, _lib.stream_ptr(dev)))
        self._ws = None
        return self

    def get_gemm_precision(self):
        return "bf16" if self._precision == 1 else "fp32"

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None:
            try:
                self._native("destroy")(h)
            except Exception:
                pass

    def _workspace(self, nbytes, ws=None):
        """The module's own scratch workspace (grown on demand), or a caller-owned one (`ws`, from `new_workspace`): anything
        that outlives the call -- a captured HIP graph above all -- must bring its own, because growing the module's
        workspace frees the old buffer."""
        dev = self._device()
        if ws is not None:
            if ws.device != dev or ws.dtype != torch.uint8 or ws.numel() < nbytes:
                raise ValueError("workspace too small or on the wrong device (%d bytes needed)" % nbytes)
            return ws
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != dev:
            self._ws = None
            self._ws = _lib.new_workspace(nbytes, dev)
        return self._ws

    def _signature(self):
        """What `_engine`, `GraphSampler` and `RequestStream` compare to notice a weight change: (data_ptr, version) of every parameter and buffer, behind a count
        of how often the SET of tensor objects changed.  Noticed with no further call: `load_state_dict` (with or without `assign=True`, from any device),
        optimizer steps and ordinary in-place ops (the version), `.to()` / `.cuda()` / `.float()` and `p.data = t` (the pointer), a new Parameter or buffer object
        under an existing name (the registration count above).  NOT noticed: in-place edits through `.data` (`p.data.mul_(2)`), which torch does not version --
        call `refresh()` after those.
        The tensor LIST is cached (walking the module tree costs ~0.7 ms at the 570M size, the comparison itself ~0.08 ms) and walked again only after a
        registration somewhere in the process, an `_apply` or a `refresh()`; a walk that finds the same objects keeps the list."""
        d = self.__dict__
        ts = d.get("_sig_tensors")
        if ts is None or d.get("_sig_seen") != _REGISTRATIONS[0]:
            seen = _REGISTRATIONS[0]
            new = list(self.parameters()) + list(self.buffers())
            if ts is None:
                ts = d["_sig_tensors"] = new
            elif len(new) != len(ts) or any(a is not b for a, b in zip(new, ts)):
                ts = d["_sig_tensors"] = new
                d["_sig_swaps"] = d.get("_sig_swaps", 0) + 1  # (a new object may sit where a freed one sat, at version 0: the pointers alone do not tell)
            d["_sig_seen"] = seen
        sig = [(d.get("_sig_swaps", 0), -1)]
        sig.extend([(t.data_ptr(), t._version) for t in ts])
        return tuple(sig)

    def _apply(self, fn, *args, **kwargs):
        self.__dict__["_sig_seen"] = None
        return super()._apply(fn, *args, **kwargs)

    def refresh(self):
        """Force the native engine to reload every tensor on the next call.  Needed only after in-place edits through `.data` (`p.data *= ...`, the idiom the
        reference itself uses at init; `p.data.copy_(t)`), which torch does not version; every other route by which weights change is noticed (`_signature`)."""
        self._loaded_sig = None
        self.__dict__["_sig_seen"] = None

    def __getstate__(self):
        """A copy (`copy.deepcopy`, pickle, `torch.save` of the module) takes the tensors and the settings, never the native model: it starts without a handle,
        a loaded signature, a workspace or a tensor list, and builds its own engine on first use."""
        state = dict(self.__dict__)
        state.update(_handle=None, _loaded_sig=None, _ws=None, _load_gen=0)
        for k in ("_sig_tensors", "_sig_seen", "_sig_swaps"):
            state.pop(k, None)
        return state


class _Holder(nn.Module):
    """Parameter container; children / parameters are registered under the reference's attribute names."""

    def __init__(self, **items):
        super().__init__()
        for name, v in items.items():
            if isinstance(v, nn.Module):
                self.add_module(name, v)
            else:
                self.register_parameter(name, v)


def _p(*shape):
    return nn.Parameter(torch.empty(*shape, dtype=torch.float32))


def _wb(w_shape, bias=True):
    return _Holder(weight=_p(*w_shape), **({"bias": _p(w_shape[0])} if bias else {}))


def _seq(**children):  # nn.Sequential-like numbering ("0", "1", ...), only the parametrised slots exist
    return _Holder(**children)


def _channelwise(c):
    return _seq(**{"0": _wb((4 * c, c)), "2": _Holder(gamma=_p(1, 1, 1, 4 * c), beta=_p(1, 1, 1, 4 * c)), "4": _wb((c, 4 * c))})


class _Block(_Holder):
    def __init__(self, kind, **items):
        super().__init__(**items)
        self.kind = kind


class _InferenceOnly(torch.autograd.Function):
    """Marks an eval-mode result of the HIP engine as non-differentiable WITH a readable failure: the engine keeps no activations
    and has no backward kernels, so `loss.backward()` through an eval-mode forward raises here and names the fix."""

    @staticmethod
    def forward(ctx, anchor, run):
        # the engine runs INSIDE the Function, so the result is a fresh tensor of this node (not a view of an input): in-place edits of the
        # logits work as on the reference's output, and nothing is copied
        return run()

    @staticmethod
    def backward(ctx, grad):  # (gradients for: anchor, run)
        raise RuntimeError("paella_amd.Paella was evaluated in eval mode (the hand-written HIP inference engine, which has no backward); "
                           "call model.train() before the forward for the differentiable path (paella_amd/training.py)")


class CondCache:
    """Device-resident result of `Paella.prepare_cond` (K/V of the conditioning rows for every AttnBlock).
    lens (ragged conditioning): None, or an int32 DEVICE tensor [B] -- the cache is then B slots of S rows, sample b's real rows sit at the front of slot b and
    lens[b] says how many there are; the attention kernels bound every sample by its own count and never read the rest of a slot.
    gen: the load generation of the module whose weights made the K/V (`prepare_cond` records it; one integer names one load of one module), or None for a cache
    put together by a caller that watches the weights itself (`GraphSampler`, `RequestStream`).  `forward_prepared` / `forward_sample` refuse a cache whose
    generation is not the module's current one: its K/V come from other weights.  The K/V do not depend on the gemm precision mode (the conditioning mappers and
    the composed K|V projection run in fp32 in either mode), so a cache outlives `set_gemm_precision`."""

    def __init__(self, buf, B, S, lens=None, gen=None):
        self.buf, self.B, self.S, self.lens, self.gen = buf, B, S, lens, gen


class KeyWeights:
    """Per-request prompt weights: one row of post-softmax key multipliers (`attn_weights` of utils/alter_attention.py:23-34) per conditioning SLOT of a launch
    instead of one vector for all of them -- `buf` fp32 [nb, pitch], row b = slot b's multipliers at its front, and `lens` int32 [nb], how many there are (0 = the
    slot is unweighted).  nb is the conditioning batch of the forward it is passed to (`cond.B`: 2 * Bx for a guided step, conditional slots first, so the two
    halves carry independent rows).  Slot b weighs the last lens[b] keys of its OWN key sequence; entries beyond the count are never read.  `Paella.forward_prepared`
    and `Paella.forward_sample` take a KeyWeights wherever they take a 1-D `attn_weights` tensor.  `set` writes in place, so a captured graph that reads the table
    serves other weights without a recapture."""

    def __init__(self, nb, pitch, device="cuda"):
        nb, pitch = int(nb), int(pitch)
        if nb < 1 or pitch < 1:
            raise ValueError("KeyWeights needs nb >= 1 slots and pitch >= 1 weights per slot")
        self.buf = torch.zeros(nb, pitch, dtype=torch.float32, device=device)
        self.lens = torch.zeros(nb, dtype=torch.int32, device=device)

    @property
    def nb(self):
        return self.buf.size(0)

    @property
    def pitch(self):
        return self.buf.size(1)

    def set(self, slot, weights):
        """slot's weights: None (or an empty vector) = unweighted, else a 1-D tensor / sequence of at most `pitch` multipliers.  In place, stream-ordered."""
        slot = int(slot)
        if not 0 <= slot < self.nb:
            raise IndexError("KeyWeights: slot %d outside 0 ... %d" % (slot, self.nb - 1))
        n = 0
        if weights is not None:
            w = torch.as_tensor(weights).detach().to(torch.float32)
            if w.dim() != 1:
                raise ValueError("attn_weights must be 1-D (utils/alter_attention.py:27)")
            n = w.numel()
            if n > self.pitch:
                raise ValueError("attn_weights has %d entries, the table holds at most %d per slot" % (n, self.pitch))
            if n:
                self.buf[slot, :n].copy_(w)
        self.lens[slot].fill_(n)
        return self

    def clear(self):
        """every slot unweighted"""
        self.lens.zero_()
        return self


MAX_REGIONS = 30  # bit 0 = "everywhere", bit r + 1 = region r; the sign bit of the int32 masks stays unused


def region_query_total(cfg, H, W):
    """Qtot: the queries of every level of a model with constructor arguments `cfg` on an H x W token grid -- the row length of `RegionTables.q_groups`"""
    p = int(cfg["patch_size"])
    return sum(((H // p) >> l) * ((W // p) >> l) for l in range(len(cfg["c_hidden"])))


def region_query_groups(masks, cfg, H, W):
    """The query-side group masks of one request: bool masks [R, H, W] on the token grid (mask r = where region r's prompt applies) -> int32 [Qtot], level-major
    (level l: the (H/patch >> l) x (W/patch >> l) positions row-major, after all finer levels).  Position (y, x) of level l stands for the patch * 2^l square
    block of token positions under it and carries bit r + 1 iff ANY of them lies in mask r (OR-pooling), and always bit 0 ("everywhere").  Pure, runs anywhere."""
    masks = torch.as_tensor(masks)
    if masks.dim() != 3 or tuple(masks.shape[1:]) != (H, W) or masks.dtype.is_floating_point or masks.dtype.is_complex:
        raise ValueError("regions: masks must be a bool / integer tensor [R, %d, %d] on the token grid" % (H, W))
    R, p, n_levels = masks.size(0), int(cfg["patch_size"]), len(cfg["c_hidden"])
    if R > MAX_REGIONS:
        raise ValueError("regions: %d masks, at most %d fit the group bits" % (R, MAX_REGIONS))
    if H % (p << (n_levels - 1)) or W % (p << (n_levels - 1)):
        raise ValueError("regions: the token grid %dx%d must be a multiple of %d" % (H, W, p << (n_levels - 1)))
    m = (masks != 0)
    out = []
    for l in range(n_levels):
        f = p << l
        g = torch.ones((H // f) * (W // f), dtype=torch.int32, device=m.device)
        if R:
            pooled = m.reshape(R, H // f, f, W // f, f).any(dim=4).any(dim=2).reshape(R, -1).to(torch.int32)
            bits = torch.tensor([1 << (r + 1) for r in range(R)], dtype=torch.int32, device=m.device)
            g = g | (pooled * bits[:, None]).sum(dim=0, dtype=torch.int32)
        out.append(g)
    return torch.cat(out)


class RegionTables:
    """Regional prompts: per-query key groups for every attention block of a forward (include/paella_hip.h, "Regional prompts") -- `q_groups` int32 [nb, Qtot], one
    bit mask per query of every level (level-major, `region_query_groups` builds a row), and `k_groups` int32 [nb, S_slot], one per conditioning row of a slot; nb
    is the conditioning batch of the forward (cond.B, conditional slots first).  Row c of slot b is visible to query q iff q_groups[b, q] & k_groups[b, c] != 0.
    The default content is 1 everywhere: everything visible, which computes the bits of the forward without the tables.  Written in place, so a captured graph
    that reads the tables serves other regions without a recapture.  Every conditioning row below the slot's count must be finite: invisible rows are read."""

    def __init__(self, nb, Qtot, S_slot, device="cuda"):
        nb, Qtot, S_slot = int(nb), int(Qtot), int(S_slot)
        if nb < 1 or Qtot < 1 or S_slot < 1:
            raise ValueError("RegionTables needs nb >= 1 slots, Qtot >= 1 queries and S_slot >= 1 rows per slot")
        self.q_groups = torch.ones(nb, Qtot, dtype=torch.int32, device=device)
        self.k_groups = torch.ones(nb, S_slot, dtype=torch.int32, device=device)

    @property
    def nb(self):
        return self.q_groups.size(0)

    def set(self, slot, q_row=None, k_row=None):
        """slot's rows: q_row int32 [Qtot] and k_row int32 [n <= S_slot] (the rest of the row becomes 1); None = all ones.  In place, stream-ordered."""
        slot = int(slot)
        if not 0 <= slot < self.nb:
            raise IndexError("RegionTables: slot %d outside 0 ... %d" % (slot, self.nb - 1))
        if q_row is None:
            self.q_groups[slot].fill_(1)
        else:
            q_row = torch.as_tensor(q_row)
            if tuple(q_row.shape) != (self.q_groups.size(1),) or q_row.dtype != torch.int32:
                raise ValueError("regions: q_row must be an int32 tensor [%d]" % self.q_groups.size(1))
            self.q_groups[slot].copy_(q_row)
        self.k_groups[slot].fill_(1)
        if k_row is not None:
            k_row = torch.as_tensor(k_row)
            if k_row.dim() != 1 or k_row.numel() > self.k_groups.size(1) or k_row.dtype != torch.int32:
                raise ValueError("regions: k_row must be an int32 tensor of at most %d entries" % self.k_groups.size(1))
            self.k_groups[slot, :k_row.numel()].copy_(k_row)
        return self

    def clear(self):
        """every slot: everything visible"""
        self.q_groups.fill_(1)
        self.k_groups.fill_(1)
        return self


class Paella(_NativeModel, nn.Module):
    """Drop-in for reference `Paella` (src/modules.py:109). Same constructor arguments and defaults."""

    def __init__(self, c_in=256, c_out=256, num_labels=8192, c_r=64, patch_size=2, c_cond=1024,
                 c_hidden=[640, 1280, 1280], nhead=[-1, 16, 16], blocks=[6, 16, 6], level_config=['CT', 'CTA', 'CTA'],
                 clip_embd=1024, byt5_embd=1536, clip_seq_len=4, kernel_size=3, dropout=0.1, self_attn=True):
        super().__init__()
        self.c_r = c_r
        self.c_cond = c_cond
        self.num_labels = num_labels
        self._cfg = dict(c_in=c_in, c_out=c_out, num_labels=num_labels, c_r=c_r, patch_size=patch_size, c_cond=c_cond,
                         c_hidden=list(c_hidden), nhead=list(nhead), blocks=list(blocks), level_config=list(level_config),
                         clip_embd=clip_embd, byt5_embd=byt5_embd, clip_seq_len=clip_seq_len, kernel_size=kernel_size,
                         self_attn=bool(self_attn))
        # dropout acts in train mode only (paella_amd/training.py); the HIP engine serves eval mode, where it is the identity
        self.dropout = dropout
        n_levels = len(c_hidden)
        if not (len(nhead) == len(blocks) == len(level_config) == n_levels):
            raise ValueError("c_hidden, nhead, blocks, level_config must have equal lengths")
        p2 = patch_size ** 2

        self.byt5_mapper = _wb((c_cond, byt5_embd))
        self.clip_mapper = _wb((c_cond * clip_seq_len, clip_embd))
        self.clip_image_mapper = _wb((c_cond * clip_seq_len, clip_embd))
        self.in_mapper = _seq(**{"0": _Holder(weight=_p(num_labels, c_in))})
        self.embedding = _seq(**{"1": _wb((c_hidden[0], c_in * p2, 1, 1))})

        def get_block(block_type, c, c_skip=0):
            if block_type == 'C':
                return _Block('C', depthwise=_Holder(weight=_p(c, (c + c_skip) // c, kernel_size, kernel_size), bias=_p(c)),
                              channelwise=_channelwise(c))
            if block_type == 'A':
                attn = _Holder(in_proj_weight=_p(3 * c, c), in_proj_bias=_p(3 * c), out_proj=_wb((c, c)))
                return _Block('A', attention=_Holder(attn=attn), kv_mapper=_seq(**{"1": _wb((c, c_cond))}))
            if block_type == 'F':
                return _Block('F', channelwise=_channelwise(c))
            if block_type == 'T':
                return _Block('T', mapper=_wb((2 * c, c_r)))
            raise Exception(f'Block type {block_type} not supported')

        self.down_blocks = nn.ModuleList()
        for i in range(n_levels):
            level = nn.ModuleList()
            if i > 0:
                level.append(_Block('D', **{"1": _wb((c_hidden[i], c_hidden[i - 1], 2, 2))}))
            for _ in range(blocks[i]):
                for bt in level_config[i]:
                    level.append(get_block(bt, c_hidden[i]))
            self.down_blocks.append(level)
        self.up_blocks = nn.ModuleList()
        for i in reversed(range(n_levels)):
            level = nn.ModuleList()
            for j in range(blocks[i]):
                for k, bt in enumerate(level_config[i]):
                    level.append(get_block(bt, c_hidden[i], c_skip=c_hidden[i] if i < n_levels - 1 and j == k == 0 else 0))
            if i > 0:
                up = _Block('U', **{"1": _Holder(weight=_p(c_hidden[i], c_hidden[i - 1], 2, 2), bias=_p(c_hidden[i - 1]))})
                level.append(up)
            self.up_blocks.append(level)
        self.clf = _seq(**{"1": _wb((c_out * p2, c_hidden[0], 1, 1))})
        self.out_mapper = _seq(**{"1": _Holder(weight=_p(num_labels, c_out, 1, 1))})

        self.reset_parameters()
        self._init_engine()
        for sw in TRAIN_SWITCHES:
            setattr(self, sw.attr, sw.off)
        # Constructed in EVAL mode (an nn.Module normally starts in train mode): eval = the hand-written HIP engine, which is what
        # sampling needs; `model.train()` -- the switch the reference's training loops flip (src/train.py:47,
        # src_distributed/train.py:73,140,172) -- selects the differentiable torch-op evaluation of paella_amd/training.py.
        self.train(False)

    # ------------------------------------------------------------------ init (same distributions as src/modules.py:189-210)
    @torch.no_grad()
    def reset_parameters(self):
        cfg = self._cfg
        for name, p in self.named_parameters():
            if name.endswith("bias") or name.endswith("gamma") or name.endswith("beta"):
                p.zero_()
            elif p.dim() >= 2:
                nn.init.xavier_uniform_(p)
            else:
                p.zero_()
        for level in self.up_blocks:  # the reference's _init_weights touches Conv2d / Linear only: the up-samplers' ConvTranspose2d
            for b in level:           # keeps torch's default init (kaiming-uniform weight, uniform bias)
                if b.kind == 'U':
                    cv = b._modules["1"]
                    ref = nn.ConvTranspose2d(cv.weight.size(0), cv.weight.size(1), kernel_size=2, stride=2)
                    cv.weight.copy_(ref.weight)
                    cv.bias.copy_(ref.bias)
        for m in (self.byt5_mapper, self.clip_mapper, self.clip_image_mapper):
            nn.init.normal_(m.weight, std=0.02)
        nn.init.xavier_uniform_(self.embedding._modules["1"].weight, 0.02)
        self.clf._modules["1"].weight.zero_()
        emb = self.in_mapper._modules["0"].weight
        nn.init.normal_(emb, std=math.sqrt(1 / cfg["num_labels"]))
        self.out_mapper._modules["1"].weight.copy_(emb[:, :, None, None])
        scale = math.sqrt(1 / sum(cfg["blocks"]))
        for level in list(self.down_blocks) + list(self.up_blocks):
            for b in level:
                if b.kind in ('C', 'F'):
                    b.channelwise._modules["4"].weight.mul_(scale)
                elif b.kind == 'T':
                    b.mapper.weight.zero_()

    # ------------------------------------------------------------------ engine plumbing
    def _device(self):
        return self.in_mapper._modules["0"].weight.device

    _abi = "paella_unet"

    def _create(self):
        cfg = self._cfg
        c = _lib.UnetConfig()
        for k in ("c_in", "c_out", "num_labels", "c_r", "patch_size", "c_cond", "clip_embd", "byt5_embd",
                  "clip_seq_len", "kernel_size"):
            setattr(c, k, int(cfg[k]))
        c.self_attn = int(cfg["self_attn"])
        n = len(cfg["c_hidden"])
        if n > _lib.MAX_LEVELS:
            raise ValueError("too many levels")
        c.n_levels = n
        for i in range(n):
            c.c_hidden[i] = int(cfg["c_hidden"][i])
            c.nhead[i] = int(cfg["nhead"][i])
            c.blocks[i] = int(cfg["blocks"][i])
            lc = cfg["level_config"][i].encode()
            if len(lc) >= _lib.MAX_BLOCK_TYPES:
                raise ValueError("level_config entry too long")
            c.level_config[i].value = lc
        h = ctypes.c_void_p()
        _lib.check(self._native("create")(ctypes.byref(c), ctypes.byref(h)))
        # frequencies computed with torch exactly as the reference does (src/modules.py:214-216)
        half = cfg["c_r"] // 2
        emb = math.log(10000) / (half - 1)
        freqs = torch.arange(half).float().mul(-emb).exp().contiguous()
        arr = (ctypes.c_float * half)(*freqs.tolist())
        _lib.check(self._native("set_timestep_freqs")(h, arr, half))
        return h

    def set_gemm_precision(self, mode):
        """OPT-IN fast mode of THIS model, outside the fp32 parity contract (include/paella_hip.h: paella_unet_set_precision): "bf16" runs the
        forward's dense contractions on bf16-operand MFMA with fp32 accumulation (bf16 shadow weights, bf16 activations between producer and
        consumer GEMMs; residual stream, statistics, attention, logits and the sampling tail stay fp32); "fp32" (default) is the exact path,
        bit for bit.  Objects that captured the model's launches or sized a workspace before the switch (`GraphSampler`, `new_workspace`)
        must be rebuilt after it."""
        return super().set_gemm_precision(mode)

    def _set_training(self, name, mode, store=True):
        """validate `mode` against the switch's row of `paella_amd.training.TRAIN_SWITCHES` and (store) keep it"""
        sw = _TRAIN_SWITCH[name]
        if mode not in (sw.off, sw.on):
            raise ValueError(sw.refusal)
        if sw.name == "depthwise" and mode == sw.on and int(self._cfg["kernel_size"]) != 3:
            raise ValueError("training depthwise 'hip' takes kernel_size 3 only (this module has %d)" % int(self._cfg["kernel_size"]))
        if store:
            setattr(self, sw.attr, mode)
        return self

    def set_training_route(self, **settings):
        """Several training switches in one call: any of activation=, depthwise=, attention=, modulation=, embedding= ("torch" / "hip") and gemm= ("fp32" / "bf16"), each as its
        `set_training_*` method takes it.  Every given setting is validated before any is stored: a refused call changes nothing."""
        unknown = sorted(set(settings) - set(_TRAIN_SWITCH))
        if unknown:
            raise TypeError("set_training_route takes %s (got also %s)" % (", ".join(_TRAIN_SWITCH), ", ".join(unknown)))
        for store in (False, True):
            for name, mode in settings.items():
                self._set_training(name, mode, store)
        return self

    def training_route(self):
        """the present training switches, as the keywords of `set_training_route`"""
        return {sw.name: sw.read(self) for sw in TRAIN_SWITCHES}

    def set_training_activation(self, mode):
        """How the TRAIN-mode forward (`forward` and `forward_loss` after `model.train()`) runs the GELU -> GlobalResponseNorm -> Dropout stretch of every
        ResBlock / FeedForwardBlock MLP: "torch" (default) is the chain of torch ops, op for op as before; "hip" runs it as one HIP op in both directions
        (`paella_amd.training.gelu_grn_dropout`) when the module is on a cuda device -- autograd then keeps the MLP's pre-activation and one [B, 4c] table
        instead of four or five [B, H, W, 4c] tensors, and the dropout masks come from one 64-bit seed per MLP drawn from torch's default CPU generator
        (`torch.manual_seed` reproduces a run; the masks are not the torch chain's).  Eval mode -- the HIP inference engine -- never sees the switch."""
        return self._set_training("activation", mode)

    def set_training_depthwise(self, mode):
        """How the TRAIN-mode forward (`forward` and `forward_loss` after `model.train()`) runs the front of every ResBlock -- the concatenation with the skip,
        the depthwise 3x3 convolution, the LayerNorm2d and the change to NHWC: "torch" (default) is the chain of torch ops, op for op as before; "hip" runs it as
        one HIP op in both directions (`paella_amd.training.dwconv_layernorm`) when the module is on a cuda device -- x and the skip are read in place, the trunk
        is kept in channels_last memory, and besides the block's input and the MLP's input autograd keeps one float per position.  Independent of
        `set_training_activation`.  The op is 3 x 3 only: "hip" on a module built with another kernel_size raises ValueError.  Eval mode -- the HIP inference
        engine -- never sees the switch."""
        return self._set_training("depthwise", mode)

    def set_training_attention(self, mode):
        """How the TRAIN-mode forward (`forward` and `forward_loss` after `model.train()`) runs the attention core of every AttnBlock -- scores, softmax, dropout
        and the product with the values, between the in-projection and the out-projection: "torch" (default) is `F.multi_head_attention_forward`, op for op as
        before; "hip" runs it as one HIP op in both directions (`paella_amd.training.attention_dropout`) when the module is on a cuda device -- autograd then
        keeps one float per (sample, head, query) instead of the [B, nhead, P, L] probabilities and their dropout mask, and the masks come from one 64-bit seed
        per block drawn from torch's default CPU generator (`torch.manual_seed` reproduces a run; the masks are not the torch chain's).  Independent of
        `set_training_activation` and `set_training_depthwise`.  A train-mode call with `attn_weights` runs the torch ops under either setting: the key-weight
        table stays an inference feature.  Eval mode -- the HIP inference engine -- never sees the switch."""
        return self._set_training("attention", mode)

    def set_training_modulation(self, mode):
        """How the TRAIN-mode forward (`forward` and `forward_loss` after `model.train()`) runs the joint around every TimestepBlock -- the residual add that ends
        the ResBlock / FeedForwardBlock in front of it, its own x (1 + a) + b, and the LayerNorm2d that begins the AttnBlock / FeedForwardBlock behind it in the
        same level: "torch" (default) is the chain of torch ops, op for op as before; "hip" runs it as one HIP op in both directions
        (`paella_amd.training.timestep_modulate`) when the module is on a cuda device -- the two summands are handed over unadded, the mapper's [B, 2C] output goes
        in and its gradient comes back whole, and besides the op's inputs and the LayerNorm rows autograd keeps one float per position.  The op draws nothing.
        Independent of `set_training_activation`, `set_training_depthwise` and `set_training_attention`.  The LayerNorm of the down- and up-sampling blocks and
        of the classifier stays where it is.  Eval mode -- the HIP inference engine -- never sees the switch."""
        return self._set_training("modulation", mode)

    def set_training_gemm(self, mode):
        """On which operands the TRAIN-mode forward (`forward` and `forward_loss` after `model.train()`) and its backward run the routed linears -- the two of every
        ResBlock / FeedForwardBlock MLP and, on the `set_training_attention("hip")` branch, the q, kv and out projections of every AttnBlock: "fp32" (default) is
        `F.linear`, op for op as before; "bf16" runs forward, dgrad and wgrad on the bf16 matrix cores with fp32 accumulation (`paella_amd.training.linear_bf16`)
        when the module is on a cuda device.  OPT-IN and OUTSIDE the fp32 parity contract, as `set_gemm_precision("bf16")` is for inference: only the operands of
        those GEMMs are rounded, inside the op.  Activations, parameters, gradients and optimizer state stay fp32 in memory, every other training op is untouched, and
        autograd keeps what `F.linear` keeps.  A site whose shapes the op does not take (rows, input or output features not a multiple of 64) runs `F.linear`,
        counted in `paella_amd.training.LINEAR_COUNTERS["fallbacks"]`.  The torch attention branch, the `attn_weights` branch, the timestep and conditioning mappers,
        the down- / up-sampling convolutions, the embedding, the classifier and the loss head stay where they are.  Independent of the four switches above and of
        `set_gemm_precision`.  Eval mode -- the HIP inference engine -- never sees the switch."""
        return self._set_training("gemm", mode)

    def set_training_embedding(self, mode):
        """How the TRAIN-mode forward (`forward` and `forward_loss` after `model.train()`) runs the token stem -- the embedding lookup, its LayerNorm, the
        PixelUnshuffle and the 1x1 convolution behind them: "torch" (default) is the chain of torch ops, op for op as before (under a seed table in pieces of
        at most 3072 tokens, `paella_amd.training._token_embedding`); "hip" runs everything in front of the convolution as one HIP op in both directions
        (`paella_amd.training.token_embed_layernorm`) when the module is on a cuda device, and the convolution as a linear over its rows (through
        `set_training_gemm` where its shapes allow) -- the forward is the inference engine's stem launch, bit for bit, and the gradient of `in_mapper.0.weight`
        is written whole by one launch that sums in ascending token order without atomics, sorts or library calls: a captured iteration (`GraphTrainStep`) holds
        it at any token count, and its bits depend on the tensors alone.  Autograd keeps the tokens and nothing per token.  The op draws nothing.  Independent of
        the five switches above.  Eval mode -- the HIP inference engine -- never sees the switch."""
        return self._set_training("embedding", mode)

    def workspace_bytes(self, B, H, W, S):
        """Bytes of workspace one forward (and the conditioning preparation) of this shape needs."""
        return int(_lib.load().paella_unet_workspace_bytes(self._engine(), B, H, W, S))

    def new_workspace(self, B, H, W, S):
        return _lib.new_workspace(self.workspace_bytes(B, H, W, S), self._device())

    def _check_table(self, t, shape, dtype, name):
        """a request-batch table: a contiguous DEVICE tensor of exactly this shape and type (the kernels index it by sample)"""
        if not torch.is_tensor(t) or t.device != self._device() or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor of shape %s on the model's device" % (name, dtype, tuple(shape)))

    def _key_weights(self, attn_weights, nb, one_d=True):
        """`attn_weights` of a forward over `nb` conditioning slots -> (fp32 tensor or None, KeyWeights or None), checked; one_d=False takes a plain tensor of
        any shape as its numel() weights (what forward_sample has always done)"""
        if isinstance(attn_weights, KeyWeights):
            self._check_table(attn_weights.buf, (nb, attn_weights.pitch), torch.float32, "attn_weights (KeyWeights.buf: one row per conditioning slot)")
            self._check_table(attn_weights.lens, (nb,), torch.int32, "attn_weights (KeyWeights.lens: one count per conditioning slot)")
            return None, attn_weights
        aw = self._f32(attn_weights, "attn_weights")
        if one_d and aw is not None and aw.dim() != 1:
            raise ValueError("attn_weights must be 1-D (utils/alter_attention.py:27)")
        return aw, None

    def _regions(self, regions, nb, H, W, S):
        """`regions` of a forward over `nb` conditioning slots of S rows on an H x W grid, checked (None passes through)"""
        if regions is None:
            return None
        if not isinstance(regions, RegionTables):
            raise ValueError("regions must be a paella_amd.RegionTables")
        if self._precision == 1:
            raise ValueError("regions are not offered in the bf16 precision mode (the bf16 attention core has no masked form)")
        self._check_table(regions.q_groups, (nb, region_query_total(self._cfg, H, W)), torch.int32, "regions (RegionTables.q_groups: one row per conditioning slot)")
        self._check_table(regions.k_groups, (nb, S), torch.int32, "regions (RegionTables.k_groups: one row per conditioning slot)")
        return regions

    @staticmethod
    def _f32(t, name):
        if t is None:
            return None
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a HIP (cuda) tensor")
        return t.detach().to(torch.float32).contiguous()

    # ------------------------------------------------------------------ conditioning
    def _cond_args(self, byt5, clip, clip_image):
        cfg = self._cfg
        byt5 = self._f32(byt5, "byt5")
        if byt5 is None or byt5.dim() != 3 or byt5.size(2) != cfg["byt5_embd"]:
            raise ValueError("byt5 must be [B, S, %d] (use S=0 for CLIP-only conditioning)" % cfg["byt5_embd"])
        B, Sb = byt5.size(0), byt5.size(1)
        clip = self._f32(clip, "clip")
        if clip is not None and tuple(clip.shape) != (B, cfg["clip_embd"]):
            raise ValueError("clip must be [B, %d]" % cfg["clip_embd"])
        if clip_image is None:
            images = []
        elif isinstance(clip_image, (list, tuple)):  # utils/modules.py:229-233
            images = [self._f32(ci, "clip_image") for ci in clip_image]
        else:
            images = [self._f32(clip_image, "clip_image")]
        for ci in images:
            if tuple(ci.shape) != (B, cfg["clip_embd"]):
                raise ValueError("clip_image must be [B, %d]" % cfg["clip_embd"])
        S = Sb + (cfg["clip_seq_len"] if clip is not None else 0) + cfg["clip_seq_len"] * len(images)
        arr = (ctypes.c_void_p * max(len(images), 1))(*[ci.data_ptr() for ci in images]) if images else None
        return byt5, clip, images, arr, B, Sb, S

    def cond_bytes(self, B, S):
        """Bytes of the conditioning cache of B samples with S conditioning rows each: one row-major [B*S, kv_total] fp32 matrix, sample b's rows a contiguous slice."""
        return int(_lib.load().paella_unet_cond_bytes(self._engine(), B, S))

    def prepare_cond(self, byt5, clip=None, clip_image=None, ws=None, out=None, slot_rows=None, lens_out=None):
        """Hoisted conditioning work (gen_c_embeddings + kv_mapper + K/V in-projection per AttnBlock).
        out: an optional contiguous uint8 DEVICE tensor of `cond_bytes(B, S)` bytes that receives the cache instead of a fresh buffer -- e.g. the rows of one slot
        inside a larger cache (the cache is row-major by sample, so a request stream prepares ONE request straight into its slot).
        slot_rows (ragged conditioning, with lens_out): the B samples' S rows go to the front of B slots of `slot_rows` >= S rows each -- `out` (or a fresh buffer) has
        `cond_bytes(B, slot_rows)` bytes, the stored rows are those of the plain call bit for bit and no other byte of `out` is written; lens_out, a contiguous
        int32 DEVICE tensor [B] (e.g. B entries of a larger cache's table), receives S.  Returns CondCache(out, B, slot_rows, lens_out)."""
        h = self._engine()
        lib = _lib.load()
        dev = self._device()
        byt5, clip, images, arr, B, Sb, S = self._cond_args(byt5, clip, clip_image)
        if S == 0:
            raise ValueError("conditioning sequence is empty")
        if (slot_rows is None) != (lens_out is None):
            raise ValueError("slot_rows and lens_out go together")
        if slot_rows is not None:
            slot_rows = int(slot_rows)
            if S > slot_rows:
                raise ValueError("%d conditioning rows do not fit a slot of %d rows" % (S, slot_rows))
            self._check_table(lens_out, (B,), torch.int32, "lens_out")
        with torch.cuda.device(dev):
            nbytes = lib.paella_unet_cond_bytes(h, B, S if slot_rows is None else slot_rows)
            if out is None:
                buf = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
            elif out.device != dev or out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != int(nbytes):
                raise ValueError("out must be a contiguous uint8 tensor of %d bytes on the model's device" % int(nbytes))
            else:
                buf = out
            ws = self._workspace(lib.paella_unet_workspace_bytes(h, B, 0, 0, S), ws)
            if slot_rows is not None:
                _lib.check(lib.paella_unet_cond_prepare_slots(h, _lib.ptr(byt5) if Sb > 0 else None, Sb, _lib.ptr(clip), arr, len(images), B, slot_rows, 0,
                                                              _lib.ptr(buf), buf.numel(), _lib.ptr(lens_out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
                return CondCache(buf, B, slot_rows, lens_out, gen=self._load_gen)
            _lib.check(lib.paella_unet_cond_prepare(h, _lib.ptr(byt5) if Sb > 0 else None, Sb, _lib.ptr(clip), arr, len(images), B,
                                                    _lib.ptr(buf), buf.numel(), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        return CondCache(buf, B, S, gen=self._load_gen)

    def _check_cond(self, cond):
        """a cache that records its load generation must be of this module's current load (called after `_engine()`, which is what reloads)"""
        gen = getattr(cond, "gen", None)
        if gen is not None and gen != self._load_gen:
            raise RuntimeError("this CondCache holds K/V computed from other weights: the module's weights changed (and were reloaded) after prepare_cond, or the "
                               "cache was prepared by another module -- call prepare_cond again")

    def _cond_lens(self, cond):
        """the `cond_len` table of a ragged cache (None for a plain one), checked"""
        lens = getattr(cond, "lens", None)
        if lens is not None:
            self._check_table(lens, (cond.B,), torch.int32, "CondCache.lens")
        return lens

    def gen_c_embeddings(self, byt5, clip, clip_image):
        """reference src/modules.py:223-232 -> [B, S, c_cond]"""
        h = self._engine()
        lib = _lib.load()
        dev = self._device()
        byt5, clip, images, arr, B, Sb, S = self._cond_args(byt5, clip, clip_image)
        out = torch.empty(B, S, self.c_cond, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ws = self._workspace(lib.paella_unet_workspace_bytes(h, B, 0, 0, S))
            _lib.check(lib.paella_unet_c_embeddings(h, _lib.ptr(byt5) if Sb > 0 else None, Sb, _lib.ptr(clip), arr, len(images), B,
                                                    _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        return out

    def gen_r_embedding(self, r, max_positions=10000):
        """reference src/modules.py:212-221 -> [B, c_r]"""
        h = self._engine()
        dev = self._device()
        r = self._f32(r, "r")
        out = torch.empty(r.numel(), self.c_r, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().paella_unet_r_embedding(h, _lib.ptr(r), r.numel(), float(max_positions), _lib.ptr(out),
                                                           _lib.stream_ptr(dev)))
        return out

    # ------------------------------------------------------------------ forward
    def forward_prepared(self, x, r, cond, attn_weights=None, out=None, cfg_mix=None, ws=None, req_mix=None, regions=None):
        """One denoising evaluation against a `CondCache` (see `_forward_prepared_raw`): logits with the reference's shape [B, num_labels, H, W], a channels-last
        view of the position-major buffer the kernels write."""
        return self._forward_prepared_raw(x, r, cond, attn_weights=attn_weights, out=out, cfg_mix=cfg_mix, ws=ws, req_mix=req_mix, regions=regions).permute(0, 3, 1, 2)

    def _forward_prepared_raw(self, x, r, cond, attn_weights=None, out=None, cfg_mix=None, ws=None, req_mix=None, regions=None):
        """One denoising evaluation against a `CondCache`, position-major result [B, H, W, num_labels].  x int64 [Bx,H,W]; r fp32 [Bx].
        Normally Bx == cond.B.  With Bx < cond.B (cond.B a multiple of Bx) the rows b, b + Bx, ... of the conditioning
        share the tokens and timestep of row b -- classifier-free guidance batches the conditional and unconditional pass
        that way -- and the conditioning-independent prefix of the network is computed once for the Bx distinct rows.
        cfg_mix=(a, b) with cond.B == 2*Bx additionally folds the guidance mix a*logits[:Bx] + b*logits[Bx:]
        (src/utils.py:47) through the bias-free linear head and returns only those Bx mixed rows.
        Returns logits with the reference's shape [B, num_labels, H, W] (a channels-last view of the
        position-major buffer the kernels write; pass `out` = a [B,H,W,num_labels] fp32 tensor to reuse memory).
        req_mix (request batch, instead of cfg_mix): an fp32 DEVICE tensor [Bx, 2] with one guidance pair per sample.
        attn_weights: a 1-D tensor (one vector for every sample) or a `KeyWeights` table with one row per conditioning slot (cond.B of them); with the table a
        cfg_mix is uploaded as a [Bx, 2] pair table (a host-to-device copy, refused with a ValueError during a graph capture: capture such a step with req_mix).
        regions: a `RegionTables` with one row per conditioning slot (regional prompts: per-query key groups); attn_weights is then None or a `KeyWeights` table,
        and a cfg_mix is uploaded as a pair table as above.  None = the same kernels with the same arguments as the call without it."""
        h = self._engine()
        lib = _lib.load()
        dev = self._device()
        if not x.is_cuda or x.dtype != torch.int64 or x.dim() != 3:
            raise ValueError("x must be an int64 HIP tensor [B, H, W]")
        x = x.contiguous()
        nu, H, W = x.shape
        r = self._f32(r, "r")
        if r.numel() != nu:
            raise ValueError("r must have one entry per sample")
        self._check_cond(cond)
        B = cond.B
        if nu <= 0 or B % nu:
            raise ValueError("conditioning batch %d is not a multiple of the token batch %d" % (B, nu))
        aw, kw = self._key_weights(attn_weights, B)
        rg = self._regions(regions, B, H, W, cond.S)
        if rg is not None and aw is not None:
            raise ValueError("regions take prompt weights as a KeyWeights table, not as one attn_weights vector")
        mix = (0.0, 0.0) if cfg_mix is None else (float(cfg_mix[0]), float(cfg_mix[1]))
        if cfg_mix is not None and (B != 2 * nu or mix == (0.0, 0.0)):
            raise ValueError("cfg_mix needs a conditioning batch of twice the token batch and a non-zero mix")
        if req_mix is not None:
            if cfg_mix is not None or B != 2 * nu:
                raise ValueError("req_mix needs a conditioning batch of twice the token batch and no cfg_mix")
            self._check_table(req_mix, (nu, 2), torch.float32, "req_mix")
        Bo = nu if (cfg_mix is not None or req_mix is not None) else B
        if out is None:
            out = torch.empty(Bo, H, W, self.num_labels, dtype=torch.float32, device=dev)
        elif tuple(out.shape) != (Bo, H, W, self.num_labels) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous fp32 [B,H,W,num_labels] tensor")
        lens = self._cond_lens(cond)
        with torch.cuda.device(dev):
            ws = self._workspace(lib.paella_unet_workspace_bytes(h, B, H, W, cond.S), ws)
            pairs = req_mix
            if (kw is not None or rg is not None) and cfg_mix is not None:  # next to a per-slot table the guidance mix is a pair table as well
                if torch.cuda.is_current_stream_capturing():
                    raise ValueError("forward_prepared with a KeyWeights table turns cfg_mix into a pair table by a host-to-device copy, which a graph capture "
                                     "cannot hold: pass req_mix (an fp32 device tensor [Bx, 2]) instead of cfg_mix inside a capture")
                pairs, mix = torch.tensor([mix] * nu, dtype=torch.float32).to(dev), (0.0, 0.0)
            s = self._step_block(x, r, cond, mix, pairs, lens, aw, kw, rg)
            s.logits_out = out.data_ptr()
            _lib.check(lib.paella_unet_step(h, ctypes.byref(s), ctypes.sizeof(s), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        return out

    @staticmethod
    def _step_block(x, r, cond, mix, pairs, lens, aw, kw, rg):
        """the argument block of one forward (include/paella_hip.h: paella_step_args) without its output: the caller sets logits_out or tail.  It holds raw
        pointers: the tensors passed here stay alive in the caller until the call returns"""
        s = _lib.StepArgs(B=cond.B, n_unique=x.size(0), mix_c=mix[0], mix_u=mix[1], H=x.size(1), W=x.size(2), S=cond.S, n_attn_weights=0 if aw is None else aw.numel())
        _lib.tensor_fields(s, tokens=x, r=r, cond=cond.buf, mix_pairs=pairs, cond_len=lens, attn_weights=aw)
        if kw is not None:
            _lib.tensor_fields(s, kw_table=kw.buf, kw_len=kw.lens).kw_pitch = kw.pitch
        if rg is not None:
            _lib.tensor_fields(s, q_groups=rg.q_groups, k_groups=rg.k_groups)
            s.qg_pitch, s.kg_pitch = rg.q_groups.size(1), rg.k_groups.size(1)
        return s

    def forward_sample(self, x, r, cond, out, *, temperature, argmax=False, seed=0, seed_dev=None, offset=0, row_offset=0,
                       row_offset_dev=None, init_noise=None, t_next=0.0, cfg_mix=None, attn_weights=None, ws=None, req=None, stream=None, pin=None, regions=None):
        """One whole sampling step in the counter-based noise mode (src/utils.py:43-54): the denoiser evaluation with the head
        GEMM and the sampling tail FUSED -- the [B, num_labels, H, W] logits are never materialised.  x int64 [Bx,H,W], r [Bx];
        cfg_mix=(a, b) with cond.B == 2*Bx folds classifier-free guidance through the head (as forward_prepared); without it
        cond.B must equal Bx.  `out` int64 [Bx,H,W] receives the tokens (renoised against init_noise with u <= t_next when
        init_noise is given).  Bit-identical to forward_prepared + the tail kernel on the same seed.
        req=(seeds, temperature, pairs) (request batch; `temperature`, `seed`, `row_offset` and `cfg_mix` are then unused): DEVICE tables with one entry per
        sample -- int64 [Bx] seed bit patterns, fp32 [Bx] temperatures (> 0, validated by the caller), fp32 [Bx, 2] guidance pairs or None (no guidance);
        sample b draws what it draws alone under seeds[b] (counters from the position inside the sample).
        stream=(step, t_next, active) (request stream, with `req`; `offset` and `t_next` are then unused and `init_noise` is required): DEVICE tables with one entry
        per sample -- int32 [Bx] own step index (the Philox step word), fp32 [Bx] renoise threshold (negative: no renoise), int32 [Bx] active flag (0: nothing is
        stored for the sample, `out` keeps its rows) -- every request of the batch is at its own step; `out` may be `x` (the stream runs in place).
        pin=(keep, known) (scalar form) or pin=(keep, known, pin_on) (with `stream`): editing requests -- int64 [Bx,H,W] DEVICE grids, keep 1 = regenerate / 0 = known;
        after the draw and the renoise the tail stores known wherever keep == 0, with `stream` only for the samples whose int32 [Bx] flag pin_on is set.  Categorical
        mode only; not offered with `req` alone.  Without `pin` the call launches the same kernels with the same arguments as without this argument.
        attn_weights: a 1-D tensor, or (with `req`) a `KeyWeights` table with one row per conditioning slot (cond.B of them).
        regions (with `stream` only): a `RegionTables` with one row per conditioning slot -- regional prompts; attn_weights is then None or a `KeyWeights` table."""
        h = self._engine()
        lib = _lib.load()
        dev = self._device()
        if not x.is_cuda or x.dtype != torch.int64 or x.dim() != 3:
            raise ValueError("x must be an int64 HIP tensor [B, H, W]")
        x = x.contiguous()
        nu, H, W = x.shape
        r = self._f32(r, "r")
        self._check_cond(cond)
        B = cond.B
        mix = (0.0, 0.0) if cfg_mix is None else (float(cfg_mix[0]), float(cfg_mix[1]))
        if req is not None:
            seeds, temps, pairs = req
            if argmax or cfg_mix is not None or B != (nu if pairs is None else 2 * nu):
                raise ValueError("forward_sample(req=...) is categorical, takes its guidance from the pair table and needs cond.B == Bx (no pairs) or 2*Bx")
            self._check_table(seeds, (nu,), torch.int64, "req seeds")
            self._check_table(temps, (nu,), torch.float32, "req temperature")
            if pairs is not None:
                self._check_table(pairs, (nu, 2), torch.float32, "req pairs")
            if stream is not None:
                if init_noise is None:
                    raise ValueError("forward_sample(stream=...) needs init_noise: it is the renoise source of every slot")
                self._check_table(stream[0], (nu,), torch.int32, "stream step")
                self._check_table(stream[1], (nu,), torch.float32, "stream t_next")
                self._check_table(stream[2], (nu,), torch.int32, "stream active")
        elif stream is not None:
            raise ValueError("forward_sample(stream=...) needs the request tables (req=...)")
        elif (cfg_mix is None and B != nu) or (cfg_mix is not None and (B != 2 * nu or mix == (0.0, 0.0))):
            raise ValueError("forward_sample needs cond.B == Bx (no guidance) or cond.B == 2*Bx with a non-zero cfg_mix")
        if tuple(out.shape) != (nu, H, W) or out.dtype != torch.int64 or not out.is_contiguous():
            raise ValueError("out must be a contiguous int64 [B,H,W] tensor")
        if pin is not None:
            if argmax or (req is not None and stream is None) or len(pin) != (2 if stream is None else 3):
                raise ValueError("forward_sample(pin=...) is categorical and takes (keep, known), or (keep, known, pin_on) together with stream=...; "
                                 "it is not offered with req=... alone")
            self._check_table(pin[0], (nu, H, W), torch.int64, "pin keep")
            self._check_table(pin[1], (nu, H, W), torch.int64, "pin known")
            if stream is not None:
                self._check_table(pin[2], (nu,), torch.int32, "pin pin_on")
        aw, kw = self._key_weights(attn_weights, B, one_d=False)
        if kw is not None and req is None:
            raise ValueError("forward_sample takes a KeyWeights table for attn_weights only with the request tables (req=...); the scalar form takes one 1-D vector")
        rg = self._regions(regions, B, H, W, cond.S)
        if rg is not None and (stream is None or aw is not None):
            raise ValueError("forward_sample takes regions only with the stream tables (stream=...), and prompt weights next to them as a KeyWeights table")
        lens = self._cond_lens(cond)
        with torch.cuda.device(dev):
            ws = self._workspace(lib.paella_unet_workspace_bytes(h, B, H, W, cond.S), ws)
            t = _lib.TailArgs(offset=int(offset), t_next=float(t_next))  # (the stream form reads neither: its step and t_next tables carry them)
            _lib.tensor_fields(t, init_noise=init_noise, tokens_out=out)
            if req is None:
                t.temperature, t.mode, t.seed, t.row_offset = float(temperature), 1 if argmax else 0, int(seed), int(row_offset)
                _lib.tensor_fields(t, seed_ptr=seed_dev, row_offset_ptr=row_offset_dev)
            else:
                _lib.tensor_fields(t, seeds=seeds, temperature_tab=temps).rows_per_sample = H * W
            if stream is not None:
                _lib.tensor_fields(t, step=stream[0], t_next_tab=stream[1], active=stream[2])
            if pin is not None:
                _lib.tensor_fields(t, pin_keep=pin[0], pin_tokens=pin[1], pin_on=None if stream is None else pin[2])
            s = self._step_block(x, r, cond, mix, None if req is None else pairs, lens, aw, kw, rg)
            s.tail = ctypes.pointer(t)
            _lib.check(lib.paella_unet_step(h, ctypes.byref(s), ctypes.sizeof(s), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        return out

    def forward(self, x, r, byt5, clip=None, clip_image=None, x_cat=None, **kwargs):
        """reference src/modules.py:263-275 (kwargs -> attn_weights as utils/modules.py:268).
        eval mode (default): the HIP engine, no autograd graph.  train mode (`model.train()`): the differentiable torch-op
        evaluation of paella_amd/training.py, so `loss.backward()` works as in src/train.py:63-66."""
        unknown = set(kwargs) - {"attn_weights"}
        if unknown:
            raise TypeError("unsupported attention kwargs: %s" % sorted(unknown))
        if self.training:
            from .training import forward_autograd
            return forward_autograd(self, x, r, byt5, clip, clip_image, x_cat, kwargs.get("attn_weights"))
        if x_cat is not None:
            x = torch.cat([x, x_cat], dim=1)
        cond = self.prepare_cond(byt5, clip, clip_image)
        # (the engine writes position-major [B,H,W,L]; the reference's [B,L,H,W] shape is a permuted view of it -- the Function below returns the BASE tensor and
        # the permute happens outside, as an ordinary differentiable view)
        run_base = lambda: self._forward_prepared_raw(x, r, cond, attn_weights=kwargs.get("attn_weights"))
        run = lambda: run_base().permute(0, 3, 1, 2)
        if torch.is_grad_enabled():
            # like the reference module's, an eval-mode result computed with gradients enabled is attached to the parameters -- but
            # backpropagating through it fails with a message that names model.train() instead of 'does not require grad'
            anchor = getattr(self, "_grad_anchor", None)
            if anchor is None or not anchor.requires_grad:
                anchor = next((p for p in self.parameters() if p.requires_grad), None)
                object.__setattr__(self, "_grad_anchor", anchor)  # (plain attribute: not a registered parameter)
            if anchor is not None:
                return _InferenceOnly.apply(anchor, run_base).permute(0, 3, 1, 2)
        return run()

    def forward_loss(self, x, r, target, byt5, clip=None, clip_image=None, x_cat=None, attn_weights=None, label_smoothing=0.1, seeds=None):
        """Train mode only: the forward of src/train.py:63-71 with the loss head fused -- returns (loss [B, H, W], correct [B, H, W] bool) where the reference
        computes `pred = model(...)`, `criterion(pred, target)` (nn.CrossEntropyLoss(label_smoothing, reduction='none')) and `pred.argmax(1) == target`.  The network
        up to the last LayerNorm2d is the torch-op evaluation of paella_amd/training.py; out_mapper's convolution and the loss run as one HIP op in both directions
        (paella_amd.training.head_cross_entropy), so the [B, num_labels, H, W] logits never exist.  Exact fp32 whatever `set_gemm_precision` says.  seeds: a
        `paella_amd.training.TrainSeeds` -- the HIP dropout ops then read their seeds from its device words, in forward order (what a captured iteration,
        `paella_amd.training.GraphTrainStep`, needs); None: every op draws its own seed, as always."""
        if not self.training:
            raise RuntimeError("forward_loss is the training path and this module is in eval mode: call model.train() first (eval mode serves the HIP inference engine)")
        from .training import forward_loss
        return forward_loss(self, x, r, target, byt5, clip, clip_image, x_cat, attn_weights, label_smoothing, seeds)

    # ------------------------------------------------------------------ add_noise / loss weight
    def add_noise(self, x, t, mask=None, random_x=None):
        """reference src/modules.py:277-283.  Noise is drawn from torch's generator with the same calls and in the
        same order as the reference (rand_like, then randint_like), the masking arithmetic runs in the HIP kernel."""
        self._require_hip()
        dev = x.device
        if not x.is_cuda or x.dtype != torch.int64:
            raise ValueError("x must be an int64 HIP tensor")
        x = x.contiguous()
        B = x.size(0)
        per = x.numel() // max(B, 1)
        rand_u = None
        if mask is None:
            rand_u = torch.rand_like(x.float())
            t = self._f32(t, "t")
            if t.numel() != B:
                raise ValueError("t must have one entry per sample")
        else:
            mask = mask.to(torch.int64).expand_as(x).contiguous()
        if random_x is None:
            random_x = torch.randint_like(x, 0, self.num_labels)
        random_x = random_x.to(torch.int64).expand_as(x).contiguous()
        x_out = torch.empty_like(x)
        mask_out = torch.empty_like(x)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().paella_add_noise(_lib.ptr(x), _lib.ptr(t) if mask is None else None, _lib.ptr(mask),
                                                    _lib.ptr(random_x), _lib.ptr(rand_u), 0, 0, self.num_labels, B, per,
                                                    _lib.ptr(x_out), _lib.ptr(mask_out), _lib.stream_ptr(dev)))
        return x_out, mask_out

    def get_loss_weight(self, t, mask, min_val=0.3):
        """reference src_distributed/modules.py:283-284 (training-loss helper; plain tensor arithmetic)."""
        return 1 - (1 - mask) * ((1 - t) * (1 - min_val))[:, None, None]


DenoiseUNet = Paella  # name used by BASELINE.json's north_star / older upstream revisions


def replace_attention_layers(model):
    """reference utils/alter_attention.py:45-53 swaps nn.MultiheadAttention for a re-weightable copy.
    The HIP attention kernel already supports `attn_weights`, so this is a no-op kept for call-site compatibility."""
    return None

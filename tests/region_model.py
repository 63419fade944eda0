"""The specification of regional prompts (per-query key groups in attention), independent of the kernels: no GPU, no paella_amd.

Visibility: conditioning key c is visible to query q iff q_groups[q] & k_groups[c] != 0; self keys are always visible.  The softmax runs over the visible keys
only; a query that sees no key gets a zero row; key weights multiply the probabilities of the LAST n keys of the whole key sequence (visible or not) after the
softmax, without renormalisation (utils/alter_attention.py:23-34).

The whole forward is the oracle's: `regional_forward` calls oracle.paella_oracle.unet_forward with the module attributes `mha` and `c_embeddings` substituted at
run time (attn_block and unet_forward resolve both through the module's globals; the oracle's files stay as they are).  Conditioning rows are per-row functions
of their inputs (a linear map and a LayerNorm over the channels of ONE row), so the concatenation of the per-prompt c_embeddings is what preparing each prompt
at its row offset of a slot produces."""
import torch
import torch.nn.functional as F

from oracle import paella_oracle as O


def visibility(q_groups, k_groups, Lself):
    """bool [Lq, Lself + Lcond]: self keys visible, conditioning key c visible to query q iff the masks share a bit"""
    q_groups, k_groups = torch.as_tensor(q_groups, dtype=torch.int64), torch.as_tensor(k_groups, dtype=torch.int64)
    cond = (q_groups[:, None] & k_groups[None, :]) != 0
    return torch.cat([torch.ones(q_groups.numel(), Lself, dtype=torch.bool), cond], dim=1)


def masked_attention(q, k, v, vis, scale=None, weights=None):
    """fp64 attention of q [Lq, D] over k / v [Lk, D] restricted to vis bool [Lq, Lk]; weights: 1-D post-softmax multipliers of the last keys"""
    q, k, v = q.double(), k.double(), v.double()
    scale = q.size(-1) ** -0.5 if scale is None else scale
    s = (q @ k.t()) * scale
    s = s.masked_fill(~vis, float("-inf"))
    m = s.max(dim=1, keepdim=True).values
    seen = torch.isfinite(m)
    e = torch.where(vis, (s - torch.where(seen, m, torch.zeros_like(m))).exp(), torch.zeros_like(s))
    den = e.sum(dim=1, keepdim=True)
    p = torch.where(seen, e / torch.where(seen, den, torch.ones_like(den)), torch.zeros_like(e))   # nothing visible: a zero row
    if weights is not None and weights.numel():
        p = p.clone()
        p[:, -weights.numel():] *= weights.double()[None, :]
    return p @ v


def attention_batch(q, ks, vs, kc, vc, lens, nhead, Lq, Lself, q_groups, k_groups, kw=None, kw_len=None):
    """the layout of paella_op_attention_rg on the host: q [B*Lq, nhead*D], ks / vs [B*Lself, ...], kc / vc [B, S_slot, ...], lens[b] conditioning rows of sample b,
    q_groups [B, >= Lq], k_groups [B, >= S_slot], kw [B, pitch] / kw_len [B] or None -> fp64 [B*Lq, nhead*D]"""
    B, D = len(lens), q.size(1) // nhead
    out = torch.zeros(B * Lq, nhead * D, dtype=torch.float64)
    for b in range(B):
        n = int(lens[b])
        vis = visibility(q_groups[b, :Lq], k_groups[b, :n], Lself)
        w = None if kw is None else kw[b, :int(kw_len[b])]
        for h in range(nhead):
            c = slice(h * D, (h + 1) * D)
            k = torch.cat([ks[b * Lself:(b + 1) * Lself, c], kc[b, :n, c]])
            v = torch.cat([vs[b * Lself:(b + 1) * Lself, c], vc[b, :n, c]])
            out[b * Lq:(b + 1) * Lq, c] = masked_attention(q[b * Lq:(b + 1) * Lq, c], k, v, vis, weights=w)
    return out


def query_groups_bruteforce(masks, cfg, H, W):
    """`paella_amd.region_query_groups` by loops: level-major int list; position (y, x) of level l has bit r + 1 iff any token position of its patch * 2^l block is
    in mask r, and always bit 0"""
    p, out = cfg["patch_size"], []
    for l in range(len(cfg["c_hidden"])):
        f = p << l
        for y in range(H // f):
            for x in range(W // f):
                g = 1
                for r in range(len(masks)):
                    if any(bool(masks[r][yy][xx]) for yy in range(y * f, (y + 1) * f) for xx in range(x * f, (x + 1) * f)):
                        g |= 1 << (r + 1)
                out.append(g)
    return out


def level_offsets(cfg, H, W):
    """(query count -> offset inside a q_groups row) of every level"""
    p, off, table = cfg["patch_size"], 0, {}
    for l in range(len(cfg["c_hidden"])):
        n = ((H // p) >> l) * ((W // p) >> l)
        table.setdefault(n, off)
        off += n
    return table


def regional_forward(monkeypatch, sd, cfg, x, r, prompts, q_groups, k_groups, dtype=torch.float32):
    """The oracle's forward of ONE sample (x [1, H, W], r [1]) whose conditioning is the concatenation of `prompts` (conditioning dicts of one prompt each), with
    the attention of every block restricted by q_groups (int [Qtot], level-major) and k_groups (int, one per conditioning row).  dtype is the oracle's: fp32 is
    the reference's own arithmetic (the timestep embedding sin(r * 10000 * f) is an fp32 computation there; in fp64 its ARGUMENT differs by up to half an fp32 ulp
    of 10^4, which moves logits by 1e-4); the masked softmax inside is fp64 either way."""
    H, W = x.shape[1:]
    offs = level_offsets(cfg, H, W)
    self_attn = cfg.get("self_attn", True)

    def c_embeddings(sd_, cfg_, byt5, clip=None, clip_image=None):
        return torch.cat([O_c_embeddings(sd_, cfg_, p["byt5"].to(dtype), None if p.get("clip") is None else p["clip"].to(dtype),
                                         None if p.get("clip_image") is None else [c.to(dtype) for c in p["clip_image"]] if isinstance(p["clip_image"], (list, tuple))
                                         else p["clip_image"].to(dtype)) for p in prompts], dim=1)

    def mha(sd_, p, q_in, kv_in, nhead, attn_weights=None):
        assert attn_weights is None and q_in.size(0) == 1
        w, b = sd_[p + ".in_proj_weight"].chunk(3, dim=0), sd_[p + ".in_proj_bias"].chunk(3, dim=0)
        Lq, C = q_in.shape[1:]
        Lk = kv_in.size(1)
        Lself = Lq if self_attn else 0
        qg = torch.as_tensor(q_groups)[offs[Lq]:offs[Lq] + Lq]
        vis = visibility(qg, torch.as_tensor(k_groups)[:Lk - Lself], Lself)
        q, k, v = F.linear(q_in, w[0], b[0])[0], F.linear(kv_in, w[1], b[1])[0], F.linear(kv_in, w[2], b[2])[0]
        D = C // nhead
        o = torch.cat([masked_attention(q[:, h * D:(h + 1) * D], k[:, h * D:(h + 1) * D], v[:, h * D:(h + 1) * D], vis) for h in range(nhead)], dim=1).to(q_in.dtype)
        return F.linear(o[None], sd_[p + ".out_proj.weight"], sd_[p + ".out_proj.bias"])

    O_c_embeddings = O.c_embeddings
    with monkeypatch.context() as mp:
        mp.setattr(O, "mha", mha)
        mp.setattr(O, "c_embeddings", c_embeddings)
        first = prompts[0]
        with torch.no_grad():
            return O.unet_forward(sd, cfg, x, r, byt5=first["byt5"], clip=first.get("clip"), clip_image=first.get("clip_image"), dtype=dtype)

"""paella_amd -- the sampling hot path of dome272/Paella, built MI355X-first.

Public surface (mirrors the reference's Python API):
    Paella / DenoiseUNet      reference src/modules.py:109
    VQModel                   reference src/vqgan.py:45
    sample                    reference src/utils.py:35
    sample_distributed        reference src_distributed/utils.py:97
    sample_requests           (extension) B independent requests -- own seed, guidance, temperature -- in one batch; GraphRequestSampler = its captured form
    RequestStream             (extension) continuous batching: requests join and leave a fixed-shape batch at step boundaries, each with its own step count,
                              start tokens and timestep range (request_program builds one request's schedule); one captured single-step graph serves them all.
                              editing=True: inpainting / outpainting / structural-editing requests (admit(known= or image=, mask=, pin="step" | "final")) share
                              the batch and the graph with text-to-image ones; the sampling tail re-imposes their known tokens
    KeyWeights                (extension) per-request prompt weights: one row of post-softmax key multipliers per conditioning slot instead of one attn_weights
                              vector per launch; sample_requests / GraphRequestSampler / RequestStream.admit take attn_weights per request, per guidance side
    RegionTables              (extension) regional prompts: per-query key groups in attention -- RequestStream(max_regions=R).admit(regions=[(inputs, mask), ...])
                              gives a request a base prompt plus up to R prompts that apply where their mask says; region_query_groups builds the query side
    top_k / top_p / typical_mass / min_tokens
                              (extension, keyword-only) truncated sampling on sample, sample_distributed, GraphSampler, sample_requests (one value or one per
                              request), GraphRequestSampler(filtering=True) and RequestStream(filtering=True).admit: the draw is restricted to a subset of the
                              labels, the random numbers stay those of the unfiltered call (DESIGN.md 4 "Truncated sampling")
    renoise / confidence_noise / return_stats
                              (extension, keyword-only) confidence-ordered renoise and per-token confidence maps on sample, sample_distributed, GraphSampler,
                              sample_requests (renoise / confidence_noise: one value or one per request) and RequestStream(confidence=True).admit /
                              .result(stats=True): renoise="confidence" sends exactly rint(t_next * free positions) tokens per sample back to noise, the least
                              confident first; return_stats adds the log p(token) and entropy maps of the final draw; check_renoise validates one setting
                              (DESIGN.md 4 "Confidence-ordered renoise")
    inpaint / GraphInpainter  (extension) encode -> masked renoise -> sample -> decode; pin="step" keeps the known region clean at every step
    canvas                    (extension) a token grid placed on a larger canvas -> (known, mask): the outpainting set-up
    replace_attention_layers  reference utils/alter_attention.py:45
    load_conditional_models   reference src_distributed/utils.py:65 (+ embed_prompts, load_checkpoint: paella_amd/conditioning.py)
Everything executes through libpaella_hip.so (hand-written HIP for gfx950, C ABI in include/paella_hip.h).
The opt-in bf16 fast mode is a per-model switch: `Paella.set_gemm_precision("bf16")` (outside the fp32 parity contract).
"""
from .conditioning import build_paella, embed_prompts, load_checkpoint, load_conditional_models
from .editing import GraphInpainter, canvas, inpaint
from .modules import CondCache, DenoiseUNet, KeyWeights, Paella, RegionTables, region_query_groups, replace_attention_layers
from .sampling import GraphRequestSampler, GraphSampler, RequestStream, check_renoise, request_program, sample, sample_distributed, sample_requests, select_tokens
from .vqgan import VectorQuantize, VQModel


__all__ = ["Paella", "DenoiseUNet", "CondCache", "KeyWeights", "RegionTables", "region_query_groups", "VQModel", "VectorQuantize", "sample", "sample_distributed", "sample_requests", "GraphSampler", "GraphRequestSampler", "RequestStream", "request_program", "check_renoise",
           "replace_attention_layers", "inpaint", "GraphInpainter", "canvas", "select_tokens", "load_conditional_models", "embed_prompts", "load_checkpoint", "build_paella"]

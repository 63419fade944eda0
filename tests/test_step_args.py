"""CPU: the two argument blocks of include/paella_hip.h (paella_step_args / paella_tail_args) -- the ctypes structures mirror the header field by field, a wrong
args_bytes is refused, and every single-rule violation is refused by the block entry point exactly as by the fixed-form entry point of the same form.  Every refusal
below returns before any HIP call: the pointers are host arrays that are never dereferenced, the model handle is NULL."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_struct_fields(name):
    src = open(os.path.join(ROOT, "include", "paella_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), src, flags=re.S).group(1)
    return [f for decl in body.split(";") for f in re.findall(r"\b(\w+)\s*(?:,|$)", decl.strip())]


@pytest.mark.parametrize("struct,name", [("TailArgs", "paella_tail_args"), ("StepArgs", "paella_step_args")])
def test_ctypes_structures_match_the_header(struct, name):
    from paella_amd import _lib
    fields = header_struct_fields(name)
    assert len(fields) > 20
    assert [f for f, _ in getattr(_lib, struct)._fields_] == fields


def test_wrong_args_bytes_is_refused(built_lib):
    from paella_amd import _lib
    t, s = _lib.TailArgs(), _lib.StepArgs()
    for off in (-8, 8, -ctypes.sizeof(t)):
        assert built_lib.paella_sample_tail_args(ctypes.byref(t), ctypes.sizeof(t) + off, None) == -1 and b"args_bytes" in built_lib.paella_last_error()
    for off in (-8, 8, -ctypes.sizeof(s)):
        assert built_lib.paella_unet_step(None, ctypes.byref(s), ctypes.sizeof(s) + off, None, 0, None) == -1 and b"args_bytes" in built_lib.paella_last_error()
    # the library's own sizes are the structures': with the right size the block is read and its (empty) content is what is refused
    assert built_lib.paella_sample_tail_args(ctypes.byref(t), ctypes.sizeof(t), None) == -1 and b"args_bytes" not in built_lib.paella_last_error()
    assert built_lib.paella_unet_step(None, ctypes.byref(s), ctypes.sizeof(s), None, 0, None) == -1 and b"args_bytes" not in built_lib.paella_last_error()


L, ROWS, H, W, S = 16, 4, 8, 8, 6
BUF = (ctypes.c_float * 256)()
TAB = (ctypes.c_int32 * 64)()
OUT = (ctypes.c_int64 * 64)()


def p(a):
    return ctypes.cast(a, ctypes.c_void_p)


def _tail(**kw):
    """a valid scalar tail block on host arrays, then the overrides"""
    from paella_amd import _lib
    t = _lib.TailArgs(logits_c=p(BUF), rows=ROWS, L=L, cfg=1.0, temperature=1.0, seed=1, tokens_out=p(OUT))
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _stream_tail(**kw):
    """a valid stream tail block (2 samples of 2 rows)"""
    return _tail(**dict(dict(temperature_tab=p(BUF), seeds=p(OUT), rows_per_sample=2, step=p(TAB), t_next_tab=p(BUF), active=p(TAB), init_noise=p(OUT)), **kw))


def _step(tail=None, **kw):
    """a valid guided step block of 1 sample (2 conditioning slots) on host arrays, then the overrides; with `tail` the fused step"""
    from paella_amd import _lib
    s = _lib.StepArgs(tokens=p(OUT), r=p(BUF), cond=p(BUF), B=2, n_unique=1, mix_pairs=p(BUF), H=H, W=W, S=S, cond_len=p(TAB))
    if tail is None:
        s.logits_out = p(BUF)
    else:
        s.tail = ctypes.pointer(tail)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _run_tail(lib, t):
    return lib.paella_sample_tail_args(ctypes.byref(t), ctypes.sizeof(t), None)


def _run_step(lib, s):
    return lib.paella_unet_step(None, ctypes.byref(s), ctypes.sizeof(s), p(BUF), 256, None)


def _legacy_scalar_tail(lib, temperature=1.0, row_offset=0, keep=None, known=None):
    return lib.paella_sample_tail_pin(p(BUF), None, ROWS, L, 1.0, 0.0, temperature, 0, 1, None, 0, row_offset, None, None, 0.0, keep, known, p(OUT), None, None)


def _legacy_stream_tail(lib, t_next=p(BUF), keep=None, known=None, pin_on=None, fk=None, fm=None):
    return lib.paella_sample_tail_stream_filter(p(BUF), None, ROWS, L, None, p(BUF), p(OUT), 2, p(TAB), t_next, p(TAB), p(OUT), keep, known, pin_on, fk, fm, p(OUT), None, None)


def _legacy_logits(lib, kw_table=None, kw_len=None, qg=None, qp=0, kg=None, kp=0):
    return lib.paella_unet_forward_shared_req_rg(None, p(OUT), p(BUF), p(BUF), 2, 1, p(BUF), H, W, S, p(TAB), kw_table, kw_len, 4, qg, qp, kg, kp, p(BUF), p(BUF), 256, None)


def _legacy_fused_req(lib, rps):
    return lib.paella_unet_forward_sample_req(None, p(OUT), p(BUF), p(BUF), 2, 1, p(BUF), H, W, S, None, 0, p(OUT), p(BUF), rps, 0, None, 0.0, p(OUT), p(BUF), 256, None)


def _legacy_fused_pin(lib, keep, known):
    return lib.paella_unet_forward_sample_pin(None, p(OUT), p(BUF), p(BUF), 1, 1, 0.0, 0.0, H, W, S, None, None, 0, 1.0, 0, 1, None, 0, 0, None, None, 0.0, keep, known,
                                              p(OUT), p(BUF), 256, None)


# rule -> (the block call, the fixed-form entry point of the same form, the rule's key phrase)
VIOLATIONS = {
    "pin pair incomplete": (lambda lib: _run_tail(lib, _tail(pin_keep=p(OUT))), lambda lib: _legacy_scalar_tail(lib, keep=p(OUT)), b"pin_keep and pin_tokens"),
    "pin pair incomplete, stream": (lambda lib: _run_tail(lib, _stream_tail(pin_tokens=p(OUT))), lambda lib: _legacy_stream_tail(lib, known=p(OUT)), b"pin_keep and pin_tokens"),
    "pin pair incomplete, fused": (lambda lib: _run_step(lib, _step(_tail(pin_keep=p(OUT)), B=1, mix_pairs=None)), lambda lib: _legacy_fused_pin(lib, p(OUT), None),
                                   b"pin_keep and pin_tokens"),
    "pin_on without tables": (lambda lib: _run_tail(lib, _stream_tail(pin_on=p(TAB))), lambda lib: _legacy_stream_tail(lib, pin_on=p(TAB)), b"pin_on without"),
    "stream table missing": (lambda lib: _run_tail(lib, _stream_tail(t_next_tab=None)), lambda lib: _legacy_stream_tail(lib, t_next=None), b"required"),
    "filter pair incomplete": (lambda lib: _run_tail(lib, _stream_tail(filter_k=p(TAB))), lambda lib: _legacy_stream_tail(lib, fk=p(TAB)), b"filter_k and filter_mass"),
    "kw_len without kw_table": (lambda lib: _run_step(lib, _step(kw_len=p(TAB), kw_pitch=4)), lambda lib: _legacy_logits(lib, kw_len=p(TAB)), b"kw_table"),
    "key-group pair incomplete": (lambda lib: _run_step(lib, _step(q_groups=p(TAB), qg_pitch=100, kg_pitch=S)), lambda lib: _legacy_logits(lib, qg=p(TAB), qp=100, kp=S),
                                  b"q_groups and k_groups must be given together"),
    "key-group pitch too small": (lambda lib: _run_step(lib, _step(q_groups=p(TAB), qg_pitch=100, k_groups=p(TAB), kg_pitch=S - 1)),
                                  lambda lib: _legacy_logits(lib, qg=p(TAB), qp=100, kg=p(TAB), kp=S - 1), b"pitches too small"),
    "categorical temperature 0": (lambda lib: _run_tail(lib, _tail(temperature=0.0)), lambda lib: _legacy_scalar_tail(lib, temperature=0.0), b"temperature must be > 0"),
    "negative row_offset": (lambda lib: _run_tail(lib, _tail(row_offset=-1)), lambda lib: _legacy_scalar_tail(lib, row_offset=-1), b"row_offset must be >= 0"),
    "rows_per_sample != H*W": (lambda lib: _run_step(lib, _step(_tail(temperature_tab=p(BUF), seeds=p(OUT), rows_per_sample=H * W - 1))),
                               lambda lib: _legacy_fused_req(lib, H * W - 1), b"must equal H * W"),
}


@pytest.mark.parametrize("rule", sorted(VIOLATIONS))
def test_single_rule_violation_is_refused_by_block_and_fixed_form(built_lib, rule):
    """both return PAELLA_ERR_ARG (-1), and the block's message names the rule"""
    block, legacy, phrase = VIOLATIONS[rule]
    assert legacy(built_lib) == -1, built_lib.paella_last_error()
    assert phrase in built_lib.paella_last_error()
    assert block(built_lib) == -1
    assert phrase in built_lib.paella_last_error(), built_lib.paella_last_error()


def test_valid_blocks_pass_every_rule(built_lib):
    """the blocks the violations start from break no rule: without a model they get as far as the forward itself (a NULL model is PAELLA_ERR_STATE, not _ARG)"""
    for s in (_step(), _step(_stream_tail(rows_per_sample=H * W)), _step(_tail(), B=1, mix_pairs=None)):
        assert _run_step(built_lib, s) == -4, built_lib.paella_last_error()
        assert b"model not finalized" in built_lib.paella_last_error()

"""CPU: the device-side seed table of a captured training iteration -- its CPU model (tests/train_seeds_model.py) against known Philox words, the refusals of
`TrainSeeds`, of the C entry points and of the ops' `seed=` argument (all on the host, before any device work), and the declarations of the new symbols."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from paella_amd import _lib, train_ops, training
from tests import counter_noise as CN
from tests import train_op_checks as T
from tests import train_seeds_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NEW_SYMBOLS = ["paella_train_seeds_max_sites", "paella_train_seeds_advance", "paella_grn_act_forward_seed_dev", "paella_grn_act_backward_seed_dev",
               "paella_attn_train_forward_seed_dev", "paella_attn_train_backward_seed_dev"]


def test_model_words_against_known_philox_answers():
    """Philox4x32-10's published known-answer vectors (the Random123 kat_vectors: counter and key all zero, all ones, and the digits of pi) through the transcription
    the model uses; then the table's word for one (base, iteration, site): the first two output words, low word first.  With base 0, iteration 0 and site 0 that is
    the all-zero vector, 6627e8d5 e169c58d ...; and one (base, iteration, site) with a high key word in use, evaluated by the plain-integer transcription once and
    written down here, against the vectorised form that `Table.advance` uses."""
    assert CN.philox4x32_scalar(0, 0, 0) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert CN.philox4x32_scalar(CN.M64, CN.M64, CN.M64) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert CN.philox4x32_scalar(0x299F31D0A4093822, 0x85A308D3243F6A88, 0x0370734413198A2E) == (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    assert M.word(0, 0, 0) == 0xE169C58D6627E8D5
    assert M.word(T.S0, 3, 5) == 0x31F86101A6CD70B3
    t = M.Table(8, T.S0).advance().advance().advance()
    assert t.iteration == 3 and t.values()[5] == 0x31F86101A6CD70B3
    assert t.values() == [M.word(T.S0, 3, s) for s in range(8)]
    # a word does not depend on the size of the table
    assert M.Table(300, T.S0).advance().advance().advance().values()[:8] == t.values()


def test_model_words_are_pairwise_distinct():
    t = M.Table(300, T.S1)
    seen = []
    for it in range(1, 4):
        t.advance()
        assert t.iteration == it
        seen += t.values()
    assert len(seen) == 900 and len(set(seen)) == 900 and all(0 <= v <= CN.M64 for v in seen)
    # another base, other words
    assert not set(seen) & set(M.Table(300, T.S0).advance().values())


def test_train_seeds_refusals():
    for bad in (0, -1, train_ops.SEEDS_MAX_SITES + 1, 2.0, True, None):
        with pytest.raises(ValueError, match="sites"):
            training.TrainSeeds(bad, 1, "cuda")
    with pytest.raises(ValueError, match="HIP device"):
        training.TrainSeeds(4, 1, "cpu")
    with pytest.raises(ValueError, match="integer"):
        training.TrainSeeds(4, 1.5, "cuda")
    assert train_ops.SEEDS_MAX_SITES >= 4096


def test_seed_entry_points_refuse_on_the_host(built_lib):
    """the pointers below are never dereferenced: every refusal comes before anything is enqueued"""
    lib = built_lib
    p = ctypes.c_void_p(4096)  # stands for any non-NULL, 16-byte aligned device pointer
    assert lib.paella_train_seeds_max_sites() == train_ops.SEEDS_MAX_SITES
    for n in (0, -3, train_ops.SEEDS_MAX_SITES + 1):
        assert lib.paella_train_seeds_advance(p, n, None) == ERR_ARG
        assert b"n_sites" in lib.paella_last_error()
    for state in (None, ctypes.c_void_p(4100)):
        assert lib.paella_train_seeds_advance(state, 4, None) == ERR_ARG
    B, P, C = 2, 16, 64
    need = lib.paella_grn_act_workspace_bytes(B, P, C)
    for seed_dev in (None, ctypes.c_void_p(4100)):      # required, and on 8 bytes, where a mask is drawn
        assert lib.paella_grn_act_forward_seed_dev(p, p, p, B, P, C, 0.1, seed_dev, p, p, p, need, None) == ERR_ARG
        assert b"seed_dev" in lib.paella_last_error()
        assert lib.paella_grn_act_backward_seed_dev(p, p, p, p, B, P, C, 0.1, seed_dev, p, p, p, p, need, None) == ERR_ARG
    assert lib.paella_grn_act_forward_seed_dev(p, p, p, B, P, 6, 0.1, p, p, p, p, need, None) == ERR_ARG      # the shape rules of the by-value form
    nh, L, D = 2, 9, 16
    need = lib.paella_attn_train_workspace_bytes(B, nh, P, L, D)
    for seed_dev in (None, ctypes.c_void_p(4100)):
        assert lib.paella_attn_train_forward_seed_dev(p, 32, p, 64, p, 64, B, nh, P, L, D, 0.1, seed_dev, p, p, p, need, None) == ERR_ARG
        assert b"seed_dev" in lib.paella_last_error()
        assert lib.paella_attn_train_backward_seed_dev(p, 32, p, 64, p, 64, p, p, p, B, nh, P, L, D, 0.1, seed_dev, p, 32, p, 64, p, 64, p, need, None) == ERR_ARG
    assert lib.paella_attn_train_forward_seed_dev(p, 32, p, 64, p, 64, B, nh, P, L, 24, 0.1, p, p, p, p, need, None) == ERR_ARG


def test_ops_refuse_a_seed_tensor_that_is_not_one_dense_int64_word():
    """asked before the device checks, so CPU tensors reach it; a good seed tensor on CPU operands then meets the HIP-only refusal"""
    u, gamma, beta = torch.zeros(2, 4, 8), torch.zeros(8), torch.zeros(8)
    q, kv = torch.zeros(2, 4, 32), torch.zeros(2, 3, 64)
    bad = [torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.float32), torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int64),
           torch.zeros(1, dtype=torch.int64).to_sparse()]
    for s in bad:
        with pytest.raises(ValueError, match="one dense int64 element"):
            training.gelu_grn_dropout(u, gamma, beta, 0.1, s)
        with pytest.raises(ValueError, match="one dense int64 element"):
            training.attention_dropout(q, kv, 2, 0.1, seed=s)
    good = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="HIP device"):
        training.gelu_grn_dropout(u, gamma, beta, 0.1, good)
    with pytest.raises(ValueError, match="HIP device"):
        training.attention_dropout(q, kv, 2, 0.1, good)
    with pytest.raises(ValueError, match="TrainSeeds"):
        training.forward_loss(_HeadOnly(), None, None, None, None, seeds=[1, 2, 3])


class _HeadOnly:
    """what `forward_loss` looks at before it runs the network: the classifier's widths"""

    class _W:
        weight = torch.zeros(32, 16, 1, 1)
    out_mapper = type("M", (), {"_modules": {"1": _W}})


def test_new_symbols_are_declared_in_header_and_binding():
    src = open(os.path.join(ROOT, "include", "paella_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(paella_[a-z0-9_]+)\s*\(", src))
    for name in NEW_SYMBOLS:
        assert name in declared, "%s is not declared in include/paella_hip.h" % name
        assert name in _lib.SIGNATURES, "%s is not bound in paella_amd/_lib.py" % name
    assert "train_seeds.hip" in __import__("paella_amd._stamp", fromlist=["SOURCES"]).SOURCES
    # the Python surface of the feature
    for name in ("TrainSeeds", "GraphTrainStep", "dropout_sites"):
        assert hasattr(training, name)
    assert "seeds" in inspect.signature(training.forward_loss).parameters
    assert hasattr(training.ClippedAdamW, "materialize_state")

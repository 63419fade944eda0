"""CPU: the host side of continuous request batching (paella_amd.request_program, the exports) and a numpy transcription of tail.hip's request_step_kernel --
the model tests/test_gpu_request_stream.py holds the kernel against."""
import numpy as np
import pytest
import torch

import paella_amd
from paella_amd import sampling

IDLE = np.array([0.0, 1.0, 1.0, 0.0, -1.0], dtype=np.float32)


def request_step_model(program, pos, length):
    """tail.hip: request_step_kernel, one slot per loop turn.  program fp32 [B, max_steps, 5], pos / length int32 [B] (pos is advanced in place).
    Returns this tick's flat tables (r, temperature, pairs [B, 2], t_next, step, active)."""
    B, max_steps, _ = program.shape
    r, temp, t_next = np.empty(B, np.float32), np.empty(B, np.float32), np.empty(B, np.float32)
    pairs, step, active = np.empty((B, 2), np.float32), np.empty(B, np.int32), np.empty(B, np.int32)
    for b in range(B):
        p = int(pos[b])
        on = 0 <= p < int(length[b]) and p < max_steps
        row = program[b, p] if on else IDLE
        r[b], temp[b], pairs[b, 0], pairs[b, 1], t_next[b] = row
        step[b], active[b] = p, int(on)
        if on:
            pos[b] = p + 1
    return r, temp, pairs, t_next, step, active


def _bits(values):
    return np.asarray(values, dtype=np.float32).view(np.uint32)


CASES = [dict(steps=s, renoise_steps=rn, cfg=cfg, t_start=ts)
         for s in (1, 4, 12) for rn in sorted({0, s - 1, s}) for cfg, ts in ((8.0, 1.0), ((9.0, 5.0), 1.0), (3.5, 0.6), ((2.0, 6.0), 0.6))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "s%d-rn%d-cfg%s-t%s" % (c["steps"], c["renoise_steps"], c["cfg"], c["t_start"]))
def test_request_program_rows_equal_the_scalar_samplers(case):
    steps, rn, cfg, t_start = case["steps"], case["renoise_steps"], case["cfg"], case["t_start"]
    temperature, t_end, max_steps = (0.9, 0.3), 0.1, 12
    prog, n = paella_amd.request_program(steps, rn, temperature, cfg, t_start, t_end, max_steps=max_steps)
    assert n == steps and prog.dtype == torch.float32 and tuple(prog.shape) == (max_steps, 5)
    p = prog.numpy()
    t_list = sampling.linspace_schedule(t_start, t_end, steps + 1)
    temps = sampling.linspace_schedule(temperature[0], temperature[1], steps)
    assert np.array_equal(_bits(p[:steps, 0]), _bits(t_list[:steps]))
    assert np.array_equal(_bits(p[:steps, 1]), _bits(temps))
    if isinstance(cfg, tuple):  # sample_distributed: a 0-dim fp32 tensor, (1 - cfg) computed in fp32
        sched = torch.linspace(cfg[0], cfg[1], steps)
        pairs = [(float(sched[i]), float(1 - sched[i])) for i in range(steps)]
    else:  # sample(): both scalars rounded to fp32 from the python floats
        pairs = [(float(torch.tensor(float(cfg), dtype=torch.float32)), float(torch.tensor(1.0 - float(cfg), dtype=torch.float32)))] * steps
    assert np.array_equal(_bits(p[:steps, 2:4]), _bits(pairs))
    # and the request-batch tables of the same values: what GraphRequestSampler runs a lock-step batch with
    _, rt_temps, rt_pairs = sampling.request_tables(1, steps, [1], [cfg], temperature)
    assert np.array_equal(_bits(p[:steps, 1]), _bits(rt_temps[:, 0].numpy())) and np.array_equal(_bits(p[:steps, 2:4]), _bits(rt_pairs[:, 0].numpy()))
    for j in range(steps):
        if j < rn:
            assert _bits(p[j, 4]) == _bits(t_list[j + 1])
        else:
            assert p[j, 4] == -1.0
    assert np.array_equal(p[steps:], np.tile(IDLE, (max_steps - steps, 1)))
    # the padding is never run: a slot driven by the kernel model is active exactly `steps` times
    pos, length = np.zeros(1, np.int32), np.array([n], np.int32)
    act = [int(request_step_model(p[None], pos, length)[5][0]) for _ in range(max_steps + 2)]
    assert act == [1] * steps + [0] * (max_steps + 2 - steps) and int(pos[0]) == steps


def test_request_program_defaults_and_unguided():
    prog, n = paella_amd.request_program(5)
    assert n == 5 and tuple(prog.shape) == (5, 5)
    t_list = sampling.linspace_schedule(1.0, 0.0, 6)
    assert np.array_equal(_bits(prog[:4, 4].numpy()), _bits(t_list[1:5])) and float(prog[4, 4]) == -1.0  # renoise_steps None = steps - 1
    prog, _ = paella_amd.request_program(3, cfg=None, guided=False)
    assert np.array_equal(prog[:, 2:4].numpy(), np.tile(np.float32([1.0, 0.0]), (3, 1)))


def test_request_program_validation():
    with pytest.raises(ValueError, match="temperature"):
        paella_amd.request_program(4, temperature=(1.0, 0.0))
    with pytest.raises(ValueError, match="temperature"):
        paella_amd.request_program(1, temperature=(0.0, 0.5))
    with pytest.raises(ValueError, match="max_steps"):
        paella_amd.request_program(7, max_steps=6)
    with pytest.raises(ValueError, match="max_steps"):
        paella_amd.request_program(0, max_steps=6)
    with pytest.raises(ValueError, match="guided stream"):
        paella_amd.request_program(4, cfg=None, guided=True)
    with pytest.raises(ValueError, match="unguided stream"):
        paella_amd.request_program(4, cfg=8.0, guided=False)
    with pytest.raises(ValueError):
        paella_amd.request_program(4, renoise_steps=-1)
    with pytest.raises(ValueError):
        paella_amd.request_program(4, cfg=[1.0, 2.0, 3.0])


def test_request_step_model_staggered_schedule():
    """B = 4 slots, requests of 3, 1, 5 and 2 steps admitted at ticks 0, 0, 2 and 4 (slot 1 is reused at tick 4): every slot sees its own rows in order exactly
    `len` times, then idles with the idle values and a cursor that stays put"""
    B, max_steps = 4, 6
    rng = np.random.default_rng(0)
    program = np.tile(IDLE, (B, max_steps, 1))
    pos, length = np.zeros(B, np.int32), np.zeros(B, np.int32)
    admits = {0: [(0, 3), (1, 1)], 2: [(2, 5)], 4: [(1, 2)]}
    seen = {b: [] for b in range(B)}
    own = {}
    for tick in range(10):
        for b, n in admits.get(tick, []):
            rows = rng.standard_normal((n, 5)).astype(np.float32)
            program[b, :n], length[b], pos[b] = rows, n, 0
            own[b], seen[b] = rows, []
        before = pos.copy()
        r, temp, pairs, t_next, step, active = request_step_model(program, pos, length)
        for b in range(B):
            assert step[b] == before[b]
            if active[b]:
                seen[b].append(np.array([r[b], temp[b], pairs[b, 0], pairs[b, 1], t_next[b]], np.float32))
                assert pos[b] == before[b] + 1
            else:
                assert (r[b], temp[b], pairs[b, 0], pairs[b, 1], t_next[b]) == (0.0, 1.0, 1.0, 0.0, -1.0) and pos[b] == before[b]
        if tick == 3:
            assert list(active) == [0, 0, 1, 0]
    for b, rows in own.items():
        assert np.array_equal(np.array(seen[b]), rows), "slot %d did not see its rows in order exactly len times" % b
    assert seen[3] == [] and list(pos) == [3, 2, 5, 0]


def test_exports():
    for name in ("RequestStream", "request_program"):
        assert name in paella_amd.__all__ and hasattr(paella_amd, name)

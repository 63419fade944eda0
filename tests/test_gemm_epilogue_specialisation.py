"""CPU: the compile-time epilogue classes of the GEMM (gemm_device.h: EPI_*) take the uniforms of absent features out of the batch-1 ring kernels.
Parses the kernel-resource remarks build.py keeps next to every object (build/<unit>.resources.txt), as tests/test_kernel_resources.py does, and holds
the SGPR spill of every specialised instantiation to a ceiling: at most half of its run-time twin's (91-151 when the classes were introduced; the values
reached are in profiles/gemm_epilogue_isa_counts.txt).  Every specialised kernel keeps an EPI_RUNTIME twin, the fall-back of sites outside the set."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "paella_amd", "csrc", "build")
EPI_RUNTIME = 1 << 30
GEMM = re.compile(r"_Z14gemm_nt_kernelILi(\d)ELi(\d)ELi(\d)ELi(\d)ELi(\d)ELi(\d)ELb(\d)ELi(\d+)ELb(\d)ELi(\d)ELb(\d)ELi(\d+)E")
# (APRO, classes) of the 32x32 ring tiles (ids 30 / 31: RING 3 / 4) -- gemm.hip: RingEpi
B, BGF, BGS, BR, BRS, BRT, BRST = 1, 1 | 2 | 64, 1 | 2 | 32, 1 | 4, 1 | 4 | 16, 1 | 4 | 8, 1 | 4 | 16 | 8
RING_SETS = {0: {B, BGF, BGS, BR, BRS}, 1: {BR, BRS, BRT, BRST}, 2: {B}, 4: {BR, BRS, BRT, BRST}}
# highest SGPR spill reached per prologue (ring 3 and 4 alike) when the classes were introduced, and the ceiling held here (<= half of the run-time twin)
RING_SPILL_CEILING = {0: 20, 1: 25, 2: 4, 4: 36}


def _gemm_kernels(built_lib):
    path = os.path.join(BUILD, "gemm.resources.txt")
    if not os.path.exists(path):
        pytest.skip("no compiler remarks next to the objects (library reused from a snapshot without its build directory)")
    out = {}
    for blk in re.split(r"remark: Function Name: ", open(path).read())[1:]:
        m = GEMM.match(blk.split()[0])
        if not m:
            continue
        key = tuple(int(v) for v in m.groups())
        spill = re.search(r"SGPRs Spill: (\d+)", blk)
        scratch = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk)
        out[key] = dict(spill=int(spill.group(1)) if spill else 0, scratch=int(scratch.group(1)) if scratch else 0)
    return out


def test_every_ring_class_is_instantiated_with_a_runtime_twin(built_lib):
    ks = _gemm_kernels(built_lib)
    for ring in (3, 4):
        for apro, classes in RING_SETS.items():
            base = (2, 2, 1, 1, 1, apro, 0, 32, 0, ring, 0)
            assert base + (EPI_RUNTIME,) in ks, "missing run-time twin %s" % (base,)
            for c in classes:
                assert base + (c,) in ks, "missing specialised ring kernel %s class %d" % (base, c)
    specialised = [k for k in ks if k[-1] != EPI_RUNTIME]
    for k in specialised:
        assert k[:-1] + (EPI_RUNTIME,) in ks, k


def test_specialised_classes_cut_the_sgpr_spill(built_lib):
    ks = _gemm_kernels(built_lib)
    for ring in (3, 4):
        for apro, classes in RING_SETS.items():
            base = (2, 2, 1, 1, 1, apro, 0, 32, 0, ring, 0)
            twin = ks[base + (EPI_RUNTIME,)]["spill"]
            for c in classes:
                k = ks[base + (c,)]
                assert k["scratch"] == 0
                assert k["spill"] <= RING_SPILL_CEILING[apro] and 2 * k["spill"] <= twin, (base, c, k, twin)

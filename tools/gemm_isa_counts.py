"""Static ISA counts of the hot gemm_nt_kernel instantiations (profiles/gemm_epilogue_isa_counts.txt).

    python tools/gemm_isa_counts.py <gemm.o> [<gemm.resources.txt>]
    python tools/gemm_isa_counts.py --req-tail <gemm.o> <gemm.resources.txt>     the REQ (request form) fused-tail head tiles instead: per instantiation the
                                                                                 instruction count and the SGPR / VGPR / scratch figures of the remarks

    python tools/gemm_isa_counts.py --attention <attention.o> <attention.resources.txt>   the attention kernels (same columns, one row per instantiation)

Extracts the gfx950 code object from the object's .hip_fatbin (llvm-objcopy + clang-offload-bundler --unbundle), disassembles it with
`llvm-objdump -d --mcpu=gfx950`, and prints per batch-1 ring instantiation: instructions after the last MFMA, v_readlane_b32 among them,
instructions before the first buffer load, and (from the kernel-resource remarks) the SGPR spill count."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
HOT = re.compile(r"^_Z14gemm_nt_kernelILi2ELi2ELi1ELi1ELi1ELi(\d)ELb0ELi32ELb0ELi([34])ELb0E(?:Li(\d+)E)?Ev")


def code_object(obj, tmp):
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    return co


def functions(co):
    txt = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], text=True)
    out, name = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.startswith("\t"):
            out[name].append(line.strip().split()[0])
    return out


def spills(res):
    d = {}
    if res and os.path.exists(res):
        for blk in re.split(r"remark: Function Name: ", open(res).read())[1:]:
            m = re.search(r"SGPRs Spill: (\d+)", blk)
            d[blk.split()[0]] = int(m.group(1)) if m else 0
    return d


REQ_TAIL = re.compile(r"^_Z14gemm_nt_kernelI(.*)Li1073741824ELb1EEv")  # ..., EPI = EPI_RUNTIME, REQ = true


def resources(res):
    d = {}
    for blk in re.split(r"remark: Function Name: ", open(res).read())[1:]:
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
        d[blk.split()[0]] = (get("TotalSGPRs"), get("VGPRs"), get("SGPRs Spill"), get(r"ScratchSize \[bytes/lane\]"))
    return d


def req_tail(obj, res):
    rs = resources(res)
    with tempfile.TemporaryDirectory() as tmp:
        fns = functions(code_object(obj, tmp))
    print("%-64s %8s %7s %7s %7s %8s %10s" % ("REQ head tile (template arguments WM,WN,TM,TN,PD,APRO,TAIL,BK,DMA,RING,BF)", "instr", "SGPR", "VGPR", "spill", "scratch", "v_mfma"))
    for name, ins in sorted(fns.items()):
        m = REQ_TAIL.match(name)
        if m:
            args = ",".join(re.findall(r"L[ib](\d+)E", m.group(1)))
            print("%-64s %8d %7d %7d %7d %8d %10d" % ((args, len(ins)) + rs.get(name, (-1, -1, -1, -1)) + (sum(op.startswith("v_mfma") for op in ins),)))


ATTN = re.compile(r"^_Z\d+(attention(?:_lds|_bf16)?_kernel)I(.*)Ev")


def attention(obj, res):
    rs = resources(res)
    with tempfile.TemporaryDirectory() as tmp:
        fns = functions(code_object(obj, tmp))
    print("%-40s %8s %7s %7s %7s %8s %10s" % ("attention kernel <template arguments>", "instr", "SGPR", "VGPR", "spill", "scratch", "v_mfma"))
    for name, ins in sorted(fns.items()):
        m = ATTN.match(name)
        if m:
            args = ",".join(re.findall(r"L[ib](\d+)E", m.group(2)))
            print("%-40s %8d %7d %7d %7d %8d %10d" % (("%s<%s>" % (m.group(1), args), len(ins)) + rs.get(name, (-1, -1, -1, -1)) + (sum(op.startswith("v_mfma") for op in ins),)))


def main():
    if sys.argv[1] == "--req-tail":
        return req_tail(sys.argv[2], sys.argv[3])
    if sys.argv[1] == "--attention":
        return attention(sys.argv[2], sys.argv[3])
    obj = sys.argv[1]
    res = sys.argv[2] if len(sys.argv) > 2 else None
    sp = spills(res)
    with tempfile.TemporaryDirectory() as tmp:
        fns = functions(code_object(obj, tmp))
    print("%-8s %-5s %-12s %10s %14s %12s %12s" % ("prologue", "ring", "class", "SGPR spill", "instr>lastMFMA", "v_readlane", "instr<1stld"))
    rows = []
    for name, ins in fns.items():
        m = HOT.match(name)
        if not m:
            continue
        apro, ring, epi = int(m.group(1)), int(m.group(2)), int(m.group(3) or 1 << 30)
        last = max((i for i, op in enumerate(ins) if op.startswith("v_mfma")), default=-1)
        first = next((i for i, op in enumerate(ins) if op.startswith("buffer_load")), -1)
        tail = ins[last + 1:]
        rows.append((apro, ring, "RUNTIME" if epi == 1 << 30 else str(epi), sp.get(name, -1), len(tail), sum(op.startswith("v_readlane") for op in tail), first))
    for r in sorted(rows, key=lambda r: (r[0], r[1], r[2] != "RUNTIME", r[2])):
        print("%-8d %-5d %-12s %10d %14d %12d %12d" % r)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Static report from the compiler (no GPU): per kernel of the given csrc/*.hip files -- instructions, VGPRs, scratch, LDS,
and the counts of the instruction classes the round-4 ISA audit looked at (correctly rounded divisions, transcendentals,
MFMAs, LDS / buffer traffic, waits, barriers), the occupancy, and the ordered `s_waitcnt vmcnt(N)` immediates of the body (the
hand-counted LDS-DMA streams: a request or a wait that moved shows here).
usage: python scripts/isa_report.py [--root OTHER_CHECKOUT] [--timing] norm conv_halo [...]
  --root DIR   report on the sources of another checkout of the repository (e.g. the parent commit's), to compare two reports
  --timing     with -DTC_TIMING_BUILDS: the ablation / trace instances too"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tooncrafter_amd", "csrc")
EXTRA = {"attention": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]}
CLASSES = [("mfma", r"v_mfma_"), ("div_scale", r"v_div_scale_f32"), ("exp", r"v_exp_f32"), ("rcp", r"v_rcp_f32"),
           ("ds_read", r"ds_read"), ("ds_write", r"ds_write"), ("buffer/global ld", r"(buffer|global)_load"),
           ("st", r"(buffer|global)_store"), ("waitcnt", r"s_waitcnt"), ("barrier", r"s_barrier")]


def rle(seq):
    out, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        out.append(seq[i] if j - i == 1 else f"{seq[i]}x{j - i}")
        i = j
    return " ".join(out)


def main():
    global ROOT, CSRC
    args = sys.argv[1:]
    if "--root" in args:
        i = args.index("--root"); ROOT = os.path.abspath(args[i + 1]); CSRC = os.path.join(ROOT, "tooncrafter_amd", "csrc"); del args[i:i + 2]
    timing = "--timing" in args
    args = [a for a in args if a != "--timing"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    print(subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.splitlines()[0])
    for name in args or ["norm", "conv_halo"]:
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, name + ".s")
            cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", f"-I{ROOT}/include", f"-I{CSRC}",
                   *EXTRA.get(name, []), *(["-DTC_TIMING_BUILDS"] if timing else []), "-S", "--cuda-device-only", os.path.join(CSRC, name + ".hip"), "-o", out]
            subprocess.run(cmd, check=True, capture_output=True)
            asm = open(out).read()
        heads = [(m.start(), m.group(1)) for m in re.finditer(r"^(_Z\w+):", asm, re.M)]
        res = {k: re.findall(r"^; %s: (\d+)" % k, asm, re.M) for k in ("NumVgprs", "ScratchSize", "LDSByteSize", "Occupancy")}
        print(f"\n== csrc/{name}.hip: {len(res['NumVgprs'])} kernels")
        print(f"{'kernel':72s} {'instr':>6s} {'VGPR':>5s} {'scr':>4s} {'LDS':>7s} {'occ':>3s}  " + " ".join(f"{c[0]:>9s}" for c in CLASSES))
        k = 0
        for i, (pos, sym) in enumerate(heads):
            end = heads[i + 1][0] if i + 1 < len(heads) else len(asm)
            body = asm[pos:end]
            if "s_endpgm" not in body:
                continue
            body = body[:body.rindex("s_endpgm")]           # the last exit (kernels with an early return have several)
            dem = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
            dem = re.sub(r"\(anonymous namespace\)::", "", dem)
            dem = re.sub(r"\(.*$", "", dem).replace("void ", "")
            n_instr = len(re.findall(r"^\s+[a-z][a-z0-9_]+", body, re.M))
            counts = [len(re.findall(r"^\s+" + pat, body, re.M)) for _, pat in CLASSES]
            print(f"{dem[:72]:72s} {n_instr:6d} {res['NumVgprs'][k]:>5s} {res['ScratchSize'][k]:>4s} {res['LDSByteSize'][k]:>7s} {res['Occupancy'][k]:>3s}  "
                  + " ".join(f"{c:9d}" for c in counts))
            vm = re.findall(r"^\s+s_waitcnt[^\n]*?vmcnt\((\d+)\)", body, re.M)
            if vm:
                print(f"    vmcnt immediates in order ({len(vm)}): {rle(vm)}")
            k += 1


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generator of tests/golden/gemm_routes.json: what tc_gemm_bf16 launches -- kernel instance, grid, block, scalar
arguments -- for a fixed problem set under every routing-switch setting the tests and scripts use.

The launches are RECORDED from the library's own sources, not restated: the GEMM sources of a tree are compiled for the
host only with gemm_route_recorder.h force-included (every hipLaunchKernelGGL prints instead of launching), linked with
gemm_route_driver.cpp, and the printed kernel-handle addresses are resolved with `nm -C`.  No GPU is needed.

    python tests/golden/make_gemm_routes.py [--tree DIR] [--problems gemm_problems.json] [--out FILE | --check]

--tree: the source tree to record from (default: this one).  The golden was recorded from the commit BEFORE the routing
moved into csrc/gemm_route.cpp, and this tree reproduces it byte for byte (--check).  --problems: the unique
TcGemmParams of one full-size guided forward and one decode, recorded on the GPU; they are kept as data inside the
golden and read back from there when the option is absent.

98 settings x 13575 problems are 1.3 million lines, so the golden holds in full only the lines of the recorded problems
and of the refusal cases under the default setting; for every setting it holds the SHA-256 of those lines and of the
synthetic grid's, and once, over everything, a histogram of kernel instances (the coverage).  tests/test_gemm_route_cpu.py
compares the pure routing function with all of it; --text FILE writes every line, to diff two trees when a digest moves."""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "gemm_routes.json")
SOURCES = ["gemm_route.cpp", "gemm.hip", "gemm_wide.hip", "gemm16.hip", "conv_halo.hip", "gemm8.hip", "gemm_ws.hip"]
FIELDS = ["a", "w", "c", "bias", "row_bias", "residual", "m", "n", "k", "lda", "ldw", "ldc", "ldr", "ldrb", "row_div", "alpha",
          "out_scale", "act", "out_f32", "gather", "cin", "frames", "t_len", "h_out", "w_out", "h_in", "w_in", "stride", "upsample",
          "pad", "batch", "stride_a", "stride_w", "stride_c", "workspace", "workspace_bytes", "a_norm", "a_norm_eps", "gn_part"]
SWITCHES = ["TC_GEMM_TILE", "TC_GEMM_TILE16", "TC_GEMM8", "TC_GEMM_WS", "TC_GEMM_WIDE", "TC_GEMM_PIPE", "TC_GEMM_SPLITK", "TC_GEMM_ORDER",
            "TC_GEMM_ORDER_MIB", "TC_GEMM_NMAJOR", "TC_GEMM_EPI_LATE", "TC_G16_ILV", "TC_G16_TALL", "TC_G8_GRID", "TC_G8_STAGGER",
            "TC_CONV_HALO", "TC_CONV_HALO_3X3", "TC_CONV_HALO_T3", "TC_CONV_HALO_TALL", "TC_CONV_HALO_KSPLIT", "TC_GN_PART"]
# every value tests/ and scripts/ set, one switch at a time
SINGLES = {"TC_GEMM_TILE": ["w", "22", "21", "12", "11"], "TC_GEMM_TILE16": ["0", "1", "2"], "TC_GEMM8": ["0", "1", "2"],
           "TC_GEMM_WS": ["0", "2", "3", "4", "5"], "TC_GEMM_WIDE": ["0"], "TC_GEMM_PIPE": ["0", "1", "2"],
           "TC_GEMM_SPLITK": ["0", "2", "4", "8"], "TC_GEMM_ORDER": ["0", "4"], "TC_GEMM_ORDER_MIB": ["1"],
           "TC_GEMM_NMAJOR": ["0", "2"], "TC_GEMM_EPI_LATE": ["1"], "TC_G16_ILV": ["0", "1", "2"], "TC_G16_TALL": ["0", "1", "2"],
           "TC_G8_GRID": ["8", "24", "248"], "TC_G8_STAGGER": ["1", "2", "3", "4"], "TC_CONV_HALO": ["0", "1", "2"],
           "TC_CONV_HALO_3X3": ["0"], "TC_CONV_HALO_T3": ["0", "1"], "TC_CONV_HALO_TALL": ["0", "1", "2"],
           "TC_CONV_HALO_KSPLIT": ["0", "1", "2"], "TC_GN_PART": ["0", "1"]}


def settings():
    out = [{}] + [{k: v} for k in SWITCHES for v in SINGLES[k]]
    # tests/test_gpu_gemm16_ilv.py
    for ilv, tall in ((0, 0), (1, 0), (2, 0), (0, 2), (1, 2), (2, 2)):
        out.append({"TC_GEMM_TILE16": "2", "TC_G16_ILV": str(ilv), "TC_G16_TALL": str(tall), "TC_GEMM_SPLITK": "0", "TC_GEMM8": "0",
                    "TC_GEMM_WS": "0"})
        out.append({"TC_GEMM_TILE16": "2", "TC_G16_ILV": str(ilv), "TC_G16_TALL": str(tall)})
    # tests/test_gpu_gemm8.py
    out += [{"TC_GEMM8": "2", "TC_GEMM_SPLITK": "0"}, {"TC_GEMM8": "2", "TC_GEMM_SPLITK": "0", "TC_G8_GRID": "8"},
            {"TC_GEMM8": "0", "TC_GEMM_SPLITK": "0"}, {"TC_GEMM8": "2", "TC_G8_GRID": "8"}, {"TC_GEMM8": "2", "TC_G8_GRID": "24"}]
    # tests/test_gpu_conv_halo.py
    out += [{"TC_CONV_HALO": "2", "TC_CONV_HALO_TALL": t, "TC_CONV_HALO_KSPLIT": k} for t, k in (("0", "0"), ("2", "0"), ("0", "1"), ("0", "2"))]
    out += [{"TC_CONV_HALO": "2", "TC_CONV_HALO_TALL": t} for t in ("1", "2")]
    # tests/test_gpu_gn_part.py
    out += [{"TC_CONV_HALO": "0", "TC_GN_PART": "1"}, {"TC_CONV_HALO": "0", "TC_GN_PART": "0"}]
    # scripts/gemm_autotune.py, and the plain K loop on every forced tile
    for t in ("22", "21", "12", "11", "w"):
        out.append({"TC_GEMM_TILE": t, "TC_GEMM_TILE16": "0", "TC_GEMM_WS": "0"})
        out.append({"TC_GEMM_TILE": t, "TC_GEMM_PIPE": "0" if t != "w" else "2"})
    out += [{"TC_GEMM_TILE16": "2", "TC_GEMM_WS": "0"}, {"TC_GEMM_TILE16": "2", "TC_GEMM_WS": "0", "TC_GEMM_PIPE": "2"},
            {"TC_GEMM_TILE16": "2", "TC_GEMM_WS": "0", "TC_G16_ILV": "0"}, {"TC_GEMM_TILE16": "2", "TC_GEMM_WS": "0", "TC_G16_ILV": "2"},
            {"TC_GEMM_TILE16": "2", "TC_GEMM_WS": "0", "TC_G16_ILV": "0", "TC_GEMM_PIPE": "2"}]
    return [(" ".join(f"{k}={v}" for k, v in s.items()) or "default", s) for s in out]


def _base(**kw):
    d = dict.fromkeys(FIELDS, 0)
    d.update(a=1, w=1, c=1, bias=1, alpha=1.0, out_scale=1.0, batch=1, workspace=-1)
    d.update(kw)
    return d


def linear(m, n, k, variant="plain"):
    d = _base(m=m, n=n, k=k, lda=k, ldw=k, ldc=n, ldr=n, ldrb=n, row_div=1280)
    for v in variant.split("+"):
        if v == "residual":
            d["residual"] = 1
        elif v == "row_bias":
            d["row_bias"] = 1
        elif v == "geglu":
            d.update(act=3, ldc=n // 2, ldr=n // 2)
        elif v == "silu":
            d["act"] = 1
        elif v == "out_f32":
            d["out_f32"] = 1
        elif v == "a_norm":
            d.update(a_norm=1, a_norm_eps=1e-5)
        elif v == "gn_part":
            d["gn_part"] = -1
        elif v == "alpha":
            d["alpha"] = 0.125
        elif v == "batch2":
            d.update(batch=2, stride_a=m * k, stride_w=n * k, stride_c=m * n)
    return d


def conv(kind, frames, h, w, cin, n, variant="plain"):
    d = _base(n=n, cin=cin, lda=cin, ldc=n, ldr=n, ldrb=n, frames=frames, t_len=16, h_in=h, w_in=w, h_out=h, w_out=w, stride=1, pad=1)
    if kind == "t3":
        d.update(gather=2, k=3 * cin)
    else:
        d.update(gather=1, k=9 * cin)
        if kind == "s2":
            d.update(stride=2, h_out=(h - 1) // 2 + 1, w_out=(w - 1) // 2 + 1)
        elif kind == "pad0":
            d.update(stride=2, pad=0, h_out=(h - 2) // 2 + 1, w_out=(w - 2) // 2 + 1)
        elif kind == "up":
            d.update(upsample=1, h_in=h // 2, w_in=w // 2)
    d["ldw"] = d["k"]
    d["m"] = frames * d["h_out"] * d["w_out"]
    d["row_div"] = d["h_out"] * d["w_out"]
    if variant == "residual":
        d["residual"] = 1
    elif variant == "row_bias":
        d["row_bias"] = 1
    elif variant == "gn_part":
        d["gn_part"] = -1
    return d


def refusals():
    """one problem per refusal of the validation and of the route"""
    ok = linear(5120, 640, 640)
    big = conv("3x3", 32, 5, 8, 1280, 1280)          # a split-K candidate
    return [dict(ok, a=0), dict(ok, m=0), dict(ok, a=2), dict(ok, residual=2), dict(ok, k=636, lda=636, ldw=636), dict(ok, ldw=632),
            dict(ok, ldc=636), dict(ok, residual=1, ldr=636), dict(ok, bias=2), dict(ok, row_bias=1, ldrb=642), dict(ok, ldc=320),
            dict(linear(5120, 640, 640, "geglu"), n=192, ldc=96), dict(linear(5120, 640, 640, "geglu"), residual=1),
            dict(ok, row_bias=1, row_div=0), dict(ok, act=7), dict(ok, lda=320), dict(ok, gather=5),
            dict(big, cin=1248), dict(big, frames=0), dict(big, m=1279), dict(big, stride=3), dict(big, upsample=1, stride=2),
            dict(big, pad=2), dict(big, h_out=6), dict(conv("t3", 32, 5, 8, 1280, 1280), t_len=5),
            dict(ok, ldw=1 << 22, n=1024, ldc=1024),                                        # 31-bit offsets
            linear(5120, 640, 640, "a_norm"),                                              # a_norm off the weight-stationary kernel
            dict(linear(5120, 1280, 640, "geglu"), gn_part=1), dict(linear(1280, 4, 320), gn_part=1),      # statistics nobody emits
            dict(big, workspace=2, workspace_bytes=1 << 30), dict(big, workspace=1, workspace_bytes=1 << 30),
            dict(big, workspace=1, workspace_bytes=1 << 30, gn_part=1), dict(big, workspace=1, workspace_bytes=64)]


LINEAR_VARIANTS = ["plain", "residual", "row_bias", "geglu", "silu", "out_f32", "a_norm", "gn_part", "alpha", "batch2", "geglu+a_norm",
                   "residual+a_norm"]


def grid():
    out = []
    for m in (1280, 5120, 20480, 40960, 81920, 163840, 655360, 2621440):
        for n in (4, 64, 128, 256, 320, 512, 640, 960, 1280, 1920, 2560, 5120, 10240):
            for k in (64, 320, 640, 1280, 2560, 5120):
                out += [linear(m, n, k, v) for v in LINEAR_VARIANTS]
    sizes = [(32, 5, 8), (32, 10, 16), (32, 20, 32), (32, 40, 64), (16, 40, 64), (16, 80, 128), (16, 160, 256), (16, 320, 512)]
    for kind in ("3x3", "s2", "up", "pad0", "t3"):
        for frames, h, w in sizes:
            for cin in (128, 256, 320, 512, 640, 1280, 1920, 2560):
                for n in sorted({cin, 4, 128, 320, 640}):
                    out += [conv(kind, frames, h, w, cin, n, v) for v in ("plain", "residual", "row_bias", "gn_part")]
    return out


def from_recording(rec):
    """recorded TcGemmParams (rows in FIELDS order + call count) -> problems: the scratch the caller sized for the default
    setting becomes 'as ops.py fills it'"""
    out = []
    for part in ("unet", "decode"):
        for row in rec[part]:
            d = dict(zip(FIELDS, row))
            d["workspace"], d["workspace_bytes"] = -1, 0
            if d["gn_part"]:
                d["gn_part"] = -1
            out.append(d)
    return out


def text(problems):
    return "".join(" ".join(repr(float(d[f])) if f in ("alpha", "out_scale", "a_norm_eps") else str(int(d[f])) for f in FIELDS) + "\n"
                   for d in problems)


def norm_name(sym):
    """`nm -C` name of a kernel handle -> the instance name"""
    sym = re.sub(r"^void ", "", sym)
    sym = sym.replace("(anonymous namespace)::", "")
    return re.sub(r"\(TcGemmParams.*\)$", "", sym)


def build_recorder(tree, tmp):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(tree, "tooncrafter_amd", "csrc")
    inc = ["-I" + os.path.join(tree, "include"), "-I" + csrc]
    objs = []
    for s in SOURCES:
        if not os.path.exists(os.path.join(csrc, s)):
            continue                                   # a tree from before gemm_route.cpp
        o = os.path.join(tmp, s + ".o")
        cmd = [hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", *inc,
               "-include", os.path.join(HERE, "gemm_route_recorder.h"), '-DTC_SRC_DIGEST="recorder"', "-c", os.path.join(csrc, s), "-o", o]
        subprocess.check_call(cmd)
        objs.append(o)
    drv = os.path.join(tmp, "driver.o")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(tree, "include"), "-c", os.path.join(HERE, "gemm_route_driver.cpp"), "-o", drv])
    exe = os.path.join(tmp, "recorder")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-no-pie", drv, *objs, "-o", exe, "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(rocm, "lib"), "-Wl,--unresolved-symbols=ignore-all"])
    names = {}
    for line in subprocess.check_output(["nm", "-C", exe], text=True).splitlines():
        m = re.match(r"([0-9a-f]+) [dDbB] (.*_kernel.*)$", line)          # the kernel handles (data), not the host stubs
        if m and "__device_stub__" not in m.group(2):
            names[int(m.group(1), 16)] = norm_name(m.group(2))
    return exe, names


def run(exe, env, problems_text, names=None):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    out = subprocess.run([exe], input=problems_text, capture_output=True, text=True, env=e, check=True).stdout
    if names is not None:
        out = re.sub(r"@0x([0-9a-f]+)", lambda m: names[int(m.group(1), 16)], out)
    lines = out.splitlines()
    assert lines[-1].endswith("end"), lines[-1]
    return lines[:-1]


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def summarise(run_setting, rec, dump=None):
    """the golden's content from a function (env, problem text) -> lines; dump: a file that receives every line"""
    real = from_recording(rec) + refusals()
    gridp = grid()
    treal, tgrid = text(real), text(gridp)
    g = {"recorded": rec, "cus": 256, "problems": {"real": len(real), "grid": len(gridp)}, "default": None, "kernels": {}, "settings": {}}
    for name, env in settings():
        lr, lg = run_setting(env, treal), run_setting(env, tgrid)
        assert len(lr) == len(real) and len(lg) == len(gridp), (name, len(lr), len(lg))
        if g["default"] is None:
            g["default"] = lr
        for l in lr + lg:
            for k in re.findall(r"\| (\w+<[^>]*>|\w+_kernel) grid", l):
                g["kernels"][k] = g["kernels"].get(k, 0) + 1
        g["settings"][name] = [digest(lr), digest(lg)]
        if dump:
            dump.write("".join(f"[{name}] {l}\n" for l in lr + lg))
    g["kernels"] = dict(sorted(g["kernels"].items()))
    return g


def dumps(g):
    """the golden's text: one recorded problem, one default line, one setting per line"""
    def block(items, ind):
        return ",\n".join(ind + x for x in items)
    recs = ",\n".join('  "%s": [\n%s\n  ]' % (k, block([json.dumps(p) for p in v], "   ")) for k, v in g["recorded"].items())
    sets = block(["%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in g["settings"].items()], "  ")
    return ('{\n "fields": %s,\n "recorded": {\n%s\n },\n "cus": %d,\n "problems": %s,\n "default": [\n%s\n ],\n "kernels": %s,\n'
            ' "settings": {\n%s\n }\n}\n' % (json.dumps(FIELDS + ["calls"]), recs, g["cus"], json.dumps(g["problems"]),
                                          block([json.dumps(l) for l in g["default"]], "  "), json.dumps(g["kernels"]), sets))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--problems")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--check", action="store_true", help="compare with the committed golden instead of writing")
    ap.add_argument("--text", help="also write every line of every setting to this file (to diff two trees)")
    a = ap.parse_args()
    if a.problems:
        rec = {k: [[r[f] for f in FIELDS + ["calls"]] for r in v] for k, v in json.load(open(a.problems)).items()}
    else:
        rec = json.load(open(GOLDEN))["recorded"]
    with tempfile.TemporaryDirectory() as tmp:
        exe, names = build_recorder(a.tree, tmp)
        g = dumps(summarise(lambda env, t: run(exe, env, t, names), rec, open(a.text, "w") if a.text else None))
    if a.check:
        same = g == open(GOLDEN).read()
        print("identical to" if same else "DIFFERENT from", GOLDEN)
        return 0 if same else 1
    open(a.out, "w").write(g)
    print("written", a.out, len(g), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Bit compare of dc_gemm_conv between two builds of the library: this tree's and another one (the parent commit's, built
with `DC_OUT=<path> dynamicrafter_amd/csrc/build.sh` from its sources).

    python tools/gemm_bitcompare.py --other-lib <path> [--listing profiles/<name>.txt]

A seeded list of launches - the smallest shapes that reach every kernel family and template instance of the dispatcher,
crossed with the epilogue options each accepts - runs once per library, each library in its own fresh child process (the
other one selected through DC_HIP_LIB). A child saves every output with the label dc_gemm_last_variant() reports; the
parent process then compares the saved outputs with torch.equal and prints one line per case: name, shape, label, equal or
DIFFERENT; then the totals and the labels reached against the labels the dc_note_variant call sites of csrc/ can produce.
Exit status 1 if an output differs, a label differs between the libraries or a label is never reached, 2 if a child process
failed (the other library is then not run). A tool, not a test.
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamicrafter_amd", "csrc")
DEV = "cuda:0"


def source_labels():
    """Every string literal inside a dc_note_variant(...) call of csrc/."""
    labels = set()
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".h")):
            continue
        text = open(os.path.join(CSRC, f)).read()
        for m in re.finditer(r"dc_note_variant\(", text):
            depth, i = 1, m.end()
            while depth and i < len(text):
                depth += {"(": 1, ")": -1}.get(text[i], 0)
                i += 1
            labels.update(re.findall(r'"([^"]+)"', text[m.end():i]))
    return labels


# ---- the cases. plan: dc_gemm_set_plan value for the launch (19 = the default). res: None | "ring" (aligned rows) |
# "ld4" (row stride % 8 == 4) | "inplace" (the residual is the output). Shapes follow tests/test_ops_gpu.py's per family.
def G(name, M, N, K, **kw):
    return dict(kind="gemm", name=name, M=M, N=N, K=K, **kw)


def CV(name, n, C, Co, H, W, **kw):
    return dict(kind="conv", name=name, n=n, C=C, Co=Co, H=H, W=W, **kw)


def TC(name, B, T, HW, C, Co=None, **kw):
    return dict(kind="tconv", name=name, B=B, T=T, HW=HW, C=C, Co=Co or C, **kw)


EPI = [("plain", {}), ("nobias", dict(bias=False)), ("gelu", dict(gelu=True)), ("rowvec", dict(rowvec=3)),
       ("alpha", dict(alpha=0.5)), ("f32", dict(f32=True, alpha=0.25)), ("res_ring", dict(res="ring")),
       ("res_ld4", dict(res="ld4")), ("res_inplace", dict(res="inplace")),
       ("all", dict(gelu=True, rowvec=3, alpha=0.5, res="ring"))]


def cases():
    out = []
    # the 128-row kernel: 64-wide (N = 320), 128-wide (N = 448: not a multiple of the tile), geglu; M no multiple of 128
    for tag, kw in EPI:
        out.append(G(f"k128/w64/{tag}", 130, 320, 64, **kw))
        out.append(G(f"k128/w128/{tag}", 1000, 448, 192, **kw))
    out.append(G("k128/w128/N4", 513, 4, 128))
    out.append(G("k128/geglu/bias", 200, 1024, 128, geglu=True))
    out.append(G("k128/geglu/nobias", 200, 1024, 128, geglu=True, bias=False))
    out.append(CV("k128/conv/s1", 3, 64, 128, 9, 11, res="ring", rowvec=3))
    out.append(CV("k128/conv/s2", 2, 128, 320, 12, 16, stride=2))
    out.append(CV("k128/conv/s2pad0", 2, 64, 64, 12, 10, stride=2, pad=0))
    out.append(CV("k128/conv/ups", 2, 128, 192, 6, 7, ups=1))
    out.append(TC("k128/tconv", 2, 5, 37, 128, res="ring"))
    # the narrow and the window conv
    out.append(CV("narrow/bf16", 3, 128, 4, 17, 70))
    out.append(CV("narrow/f32", 4, 320, 4, 18, 32, f32=True, alpha=0.5))
    out.append(CV("window/N128", 18, 128, 128, 61, 250))
    out.append(CV("window/N128/res", 18, 128, 128, 61, 250, res="ring"))
    out.append(CV("window/N256/res", 18, 128, 256, 61, 250, res="ring", bias=False))
    # LDS-DMA tiles, 128-wide (3-stage ring): plain, conv, conv with ups, tconv
    for tag, kw in EPI:
        out.append(G(f"glds128/{tag}", 30000, 448, 192, **kw))
    out.append(CV("glds128/conv", 32, 64, 384, 40, 40, res="ring", rowvec=4))
    out.append(CV("glds128/conv/s2", 32, 64, 384, 80, 80, stride=2))
    out.append(CV("glds128/conv/ups", 32, 64, 384, 20, 20, ups=1, res="ld4"))
    out.append(TC("glds128/tconv", 2, 16, 1601, 128, Co=384, res="ring"))
    # 256-wide: plain, conv, conv with ups, tconv; split-K "whole waves + remainder" (two launches + reduce)
    out.append(G("glds256/plain", 25600, 512, 320, res="ring", rowvec=4))
    out.append(G("glds256/f32", 25600, 512, 320, f32=True, alpha=0.25))
    out.append(CV("glds256/conv", 32, 64, 256, 40, 40, res="ring"))
    out.append(CV("glds256/conv/ups", 32, 64, 256, 20, 20, ups=1))
    out.append(TC("glds256/tconv", 2, 16, 1601, 256, res="ring"))
    out.append(G("glds256/splitk", 36864, 512, 2688, res="ring", gelu=True, rowvec=4, alpha=0.5))
    out.append(CV("glds256/splitk/conv", 32, 128, 512, 32, 36, res="ld4"))
    out.append(TC("glds256/splitk/tconv", 2, 16, 1152, 512))
    # 320-wide on the 8-wave kernel (plan 0): plain (K above the persistent limit), conv, conv with ups, tconv; both split-K plans
    out.append(G("glds320/plain", 51300, 320, 2624, plan=0, res="ring", rowvec=4))
    out.append(G("glds320/f32", 51300, 320, 2624, plan=0, f32=True, alpha=0.25, gelu=True))
    out.append(CV("glds320/conv", 36, 128, 320, 33, 47, plan=0, res="ring", rowvec=36))
    out.append(CV("glds320/conv/ups", 15, 64, 320, 33, 27, plan=0, ups=1))
    out.append(TC("glds320/tconv", 2, 16, 1601, 320, plan=0, res="ld4"))
    out.append(G("glds320/splitk/few", 4641, 1280, 2560, plan=0, res="ring", rowvec=4, gelu=True, alpha=0.5))
    out.append(G("glds320/splitk/few/f32", 4641, 1280, 2560, plan=0, f32=True))
    out.append(CV("glds320/splitk/few/conv", 8, 256, 1280, 18, 32, plan=0, res="inplace"))
    out.append(CV("glds320/splitk/waves/conv", 32, 256, 1280, 18, 32, plan=0, res="ring", rowvec=32))
    out.append(TC("glds320/splitk/few/tconv", 2, 4, 576, 1280, plan=0, res="ring"))
    # geglu on the non-persistent LDS-DMA kernel (K above the persistent limit): 128- and 256-wide
    out.append(G("glds/geglu128", 45000, 384, 2624, geglu=True))
    out.append(G("glds/geglu256", 32768, 1024, 2624, geglu=True, bias=False))
    # the persistent kernels: 64-, 128-, 320-wide, geglu 128 / 256, conv and tconv 320
    for tag, kw in EPI:
        out.append(G(f"persist64/{tag}", 30000, 320, 64, **kw))
        out.append(G(f"persist320/{tag}", 140000, 320, 128, **kw))
    out.append(G("persist128/plain", 70000, 448, 64))
    out.append(G("persist128/res_ring", 70000, 448, 64, res="ring", rowvec=4))
    out.append(G("persist128/res_N480", 70000, 480, 64, res="ring"))             # N % 64 != 0: epilogue-load residual
    out.append(G("persist128/f32", 70000, 448, 64, f32=True, alpha=0.25, gelu=True))
    out.append(G("persist/geglu128", 45000, 384, 128, geglu=True))
    out.append(G("persist/geglu128/nobias", 45000, 384, 128, geglu=True, bias=False))
    out.append(G("persist/geglu256", 32768 + 21, 1024, 128, geglu=True, plan=3))
    out.append(CV("persist320/conv", 16, 64, 320, 128, 128, plan=0))
    out.append(CV("persist320/conv/ragged/res_ring", 15, 64, 320, 131, 135, plan=0, res="ring", rowvec=15))
    out.append(CV("persist320/conv/s2/res_alpha", 16, 64, 320, 256, 256, plan=0, stride=2, res="ring", alpha=0.5))
    out.append(CV("persist320/conv/s2pad0", 16, 64, 320, 256, 256, plan=0, stride=2, pad=0))
    out.append(TC("persist320/tconv", 2, 16, 4608, 320))
    out.append(TC("persist320/tconv/res_ring", 3, 5, 9830, 320, res="ring"))
    out.append(TC("persist320/tconv/res_gelu", 2, 16, 4608, 320, res="ring", gelu=True))
    # the one-wave kernel under plans 3 and 0 (0: the same launches on the 8-wave kernel), whole tiles and both split-K plans,
    # merged and as two launches (plan bit 64)
    for plan in (3, 0):
        out.append(CV(f"pipe/plan{plan}/conv", 36, 128, 320, 33, 47, plan=plan, res="ring", rowvec=36))
        out.append(CV(f"pipe/plan{plan}/conv/odd", 3, 64, 320, 130, 135, plan=plan, gelu=True, alpha=0.5))
        out.append(CV(f"pipe/plan{plan}/conv/ups", 15, 64, 320, 33, 27, plan=plan, ups=1, res="ring"))
        out.append(G(f"pipe/plan{plan}/plain", 51300, 320, 1920, plan=plan, res="ring", rowvec=4))
        out.append(TC(f"pipe/plan{plan}/tconv", 2, 16, 1024, 640, plan=plan, res="ring"))
        out.append(CV(f"pipe/plan{plan}/splitk/few/conv/ups", 8, 256, 1280, 9, 16, plan=plan, ups=1, res="ring"))
    out.append(CV("pipe/splitk/few/conv", 8, 256, 1280, 18, 32, res="ring", rowvec=8))
    out.append(G("pipe/splitk/few/plain", 4641, 1280, 2560, res="inplace"))
    out.append(TC("pipe/splitk/few/tconv", 2, 4, 576, 1280, res="ring"))
    for plan in (19, 19 | 64):
        out.append(CV(f"pipe/plan{plan}/splitk/waves/conv", 32, 256, 1280, 18, 32, plan=plan, res="ring", rowvec=32))
        out.append(CV(f"pipe/plan{plan}/splitk/waves/conv/ups", 32, 256, 640, 18, 32, plan=plan, ups=1))
    # the ping-pong kernel under plans 19 (K <= 640) and 51 (any K)
    out.append(G("pp/plan19", 32768, 1024, 128, geglu=True, plan=19))
    out.append(G("pp/plan19/ragged/nobias", 16384 + 77, 2048, 192, geglu=True, plan=19, bias=False))
    out.append(G("pp/plan51", 4608, 10240, 1280, geglu=True, plan=51))
    return out


def run_case(ops, torch, c):
    g = torch.Generator(device=DEV).manual_seed(1234)
    randn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    bias_on, geglu = c.get("bias", True), c.get("geglu", False)
    conv = tconv = None
    if c["kind"] == "gemm":
        M, N, K = c["M"], c["N"], c["K"]
        a = randn(M, K).to(torch.bfloat16)
        pw = ops.PackedWeight.linear((randn(N, K) * K ** -0.5).cpu(), randn(N).cpu() if bias_on else None, DEV)
    elif c["kind"] == "conv":
        n, C, Co, H, W = c["n"], c["C"], c["Co"], c["H"], c["W"]
        stride, pad, ups = c.get("stride", 1), c.get("pad", 1), c.get("ups", 0)
        eh, ew = H << ups, W << ups
        OH, OW = ((eh + 1) // 2, (ew + 1) // 2) if stride == 2 else (eh, ew)
        a = randn(n * H * W, C).to(torch.bfloat16)
        pw = ops.PackedWeight.conv3x3((randn(Co, C, 3, 3) * (9 * C) ** -0.5).cpu(), randn(Co).cpu() if bias_on else None, DEV,
                                      n_align=4)
        conv = dict(IH=H, IW=W, OH=OH, OW=OW, stride=stride, pad=pad, ups=ups)
        M, N = n * OH * OW, pw.N
    else:
        B, T, HW, C, Co = c["B"], c["T"], c["HW"], c["C"], c["Co"]
        a = randn(B * T * HW, C).to(torch.bfloat16)
        pw = ops.PackedWeight.tconv3((randn(Co, C, 3, 1, 1) * (3 * C) ** -0.5).cpu(), randn(Co).cpu() if bias_on else None, DEV)
        tconv = dict(T=T, HW=HW)
        M, N = B * T * HW, Co
    n_out = N // 2 if geglu else N
    out = torch.zeros(M, n_out, dtype=torch.float32 if c.get("f32") else torch.bfloat16, device=DEV)
    res = None
    if c.get("res") == "ring":
        res = randn(M, n_out).to(torch.bfloat16)
    elif c.get("res") == "ld4":
        res = randn(M, n_out + 4).to(torch.bfloat16)[:, :n_out]
    elif c.get("res") == "inplace":
        out.copy_(randn(M, n_out))
        res = out
    rowvec, rpv = None, 1
    if c.get("rowvec"):
        rpv = (M + c["rowvec"] - 1) // c["rowvec"]
        rowvec = randn(c["rowvec"], n_out)
    lib = ops._hip.lib()
    prev = lib.dc_gemm_set_plan(c.get("plan", 19))
    assert prev >= 0
    try:
        ops.gemm(a, pw, out, residual=res, rowvec=rowvec, rows_per_vec=rpv, geglu=geglu, gelu=c.get("gelu", False),
                 alpha=c.get("alpha", 1.0), conv=conv, tconv=tconv)
        label = lib.dc_gemm_last_variant().decode()
    finally:
        lib.dc_gemm_set_plan(prev)
    torch.cuda.synchronize()
    ops._hip.check_error_word(c["name"])
    return out.cpu(), label


def child(out_dir):
    sys.path.insert(0, ROOT)
    import torch
    from dynamicrafter_amd import ops
    index = []
    for i, c in enumerate(cases()):
        out, label = run_case(ops, torch, c)
        torch.save(out, os.path.join(out_dir, f"{i:03d}.pt"))
        index.append(dict(name=c["name"], shape=list(out.shape), label=label))
        print(f"{c['name']} {tuple(out.shape)} {label}", flush=True)
    json.dump(index, open(os.path.join(out_dir, "index.json"), "w"))


def run_children(script, other_lib, timeout, tmp, env_sets=(("", {}),)):
    """Runs `script --child <dir>` once per library ("this": the tree's, "other": other_lib through DC_HIP_LIB) and per named
    environment set (a set with a name gets `--env-set <name>` too), each in a fresh process. -> {"this": dir, "other": dir}, or
    None when a child failed: nothing more runs on the GPU after that."""
    dirs = {}
    for tag, lib in (("this", None), ("other", os.path.abspath(other_lib))):
        dirs[tag] = os.path.join(tmp, tag)
        os.mkdir(dirs[tag])
        for name, extra in env_sets:
            env = dict(os.environ)
            env.pop("DC_HIP_LIB", None)
            if lib:
                env["DC_HIP_LIB"] = lib
            env.update(extra)
            r = subprocess.run([sys.executable, os.path.abspath(script), "--child", dirs[tag]] + (["--env-set", name] if name else []),
                               env=env, timeout=timeout, stdout=subprocess.DEVNULL)
            if r.returncode != 0:
                print(f"the run on the {tag} library ended with status {r.returncode}", file=sys.stderr)
                return None
    return dirs


def compare_saved(dirs, index="index.json"):
    """The outputs two children saved as <dir>/<i:03d>.pt with an index of dict(name, shape, label) -> (lines, number that
    differ, labels reached, equal count of cases): one line per case, equal = same label and torch.equal."""
    import torch
    ia, ib = (json.load(open(os.path.join(dirs[t], index))) for t in ("this", "other"))
    lines, differ, reached = [], 0, set()
    for i, (ca, cb) in enumerate(zip(ia, ib)):
        a, b = (torch.load(os.path.join(dirs[t], f"{i:03d}.pt")) for t in ("this", "other"))
        same = ca["label"] == cb["label"] and torch.equal(a, b)
        differ += not same
        reached.add(ca["label"])
        label = ca["label"] if ca["label"] == cb["label"] else f"{ca['label']} != {cb['label']}"
        lines.append(f"{ca['name']} {tuple(ca['shape'])} {label} {'equal' if same else 'DIFFERENT'}")
    lines.append(f"{len(ia)} outputs, {differ} differ")
    return lines, differ, reached, len(ia) == len(ib)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--other-lib", help="the library to compare this tree's against (selected through DC_HIP_LIB)")
    ap.add_argument("--listing", help="also write the listing to this file")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=480, help="seconds per child process")
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    if not args.other_lib or not os.path.exists(args.other_lib):
        ap.error("--other-lib: no such file")
    tmp = tempfile.mkdtemp(prefix="gemm_bitcompare_")
    try:
        dirs = run_children(__file__, args.other_lib, args.timeout, tmp)
        if dirs is None:
            return 2
        lines, differ, reached, same_count = compare_saved(dirs)
        want = source_labels()
        lines.append(f"labels reached ({len(reached & want)} of the {len(want)} that dc_note_variant call sites produce):")
        lines += [f"  {l}" for l in sorted(reached)]
        missing = sorted(want - reached)
        lines.append("labels never reached: " + (", ".join(missing) if missing else "none"))
        text = "\n".join(lines) + "\n"
        sys.stdout.write(text)
        if args.listing:
            open(args.listing, "w").write(text)
        return 1 if differ or missing or not same_count else 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())

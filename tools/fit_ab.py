"""Per-launch A/B of the exact-fit GEMM (csrc/gemm_fit.hip, ops.gemm_fit) against what ops.gemm launches for the same shape,
interleaved on one box, with HIP events; plus the book-keeping of profiles/fit_ab.json.

usage: python tools/fit_ab.py [--runs 7] [--launches 20] [--sets 6] [--out profiles/fit_ab.json]
       python tools/fit_ab.py --resources [--out profiles/fit_ab.json]          (no GPU: compiles gemm_fit.hip and records the
                                                                                  code object's registers and scratch)
       python tools/fit_ab.py --step NEW.jsonl PARENT.jsonl [--dumps NEW_DIR PARENT_DIR] [--out ...]     (no GPU: adds the
                                        bench.py result lines of alternating runs, and the rel-L2 of the dumped outputs)

Shapes: the plain linears of the 1024 step whose rows are whole rounds of 288 x 320 tiles on the device, M = 72 CUs
(18432 on 256 CUs) x [1280 x 1280] plain and with residual (in place, as the model calls it), [3840 x 1280], [1280 x 5120]
with residual, the [1280 x 1920] and [1280 x 2560] skips, and M = 288 CUs x [640 x 2560] with residual. A run is `launches`
back-to-back launches between two events, rotating through `sets` operand sets (activations, outputs) so that a launch does
not find its operands in the Infinity Cache from the one before (6 sets of the level-2 shape are ~570 MB); runs of the two kernels
alternate. Reported per shape, in us per launch: every run, median, min; `win` = the new kernel's median is below the other
kernel's fastest run. Each section of the JSON file is replaced by the mode that writes it; the others are kept."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes(cus):
    l2, l1 = 72 * cus, 288 * cus
    return [("l2_lin", l2, 1280, 1280, False), ("l2_lin_res", l2, 1280, 1280, True), ("l2_qkv", l2, 3840, 1280, False),
            ("l2_ff2", l2, 1280, 5120, True), ("l1_ff2", l1, 640, 2560, True), ("l2_skip1920", l2, 1280, 1920, False),
            ("l2_skip2560", l2, 1280, 2560, False)]


def measure(args):
    import torch
    from dynamicrafter_amd import ops, _hip
    lib = _hip.lib()
    dev = "cuda:0"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    gen = torch.Generator(device=dev).manual_seed(1)
    res = {}
    for name, M, N, K, has_res in shapes(cus):
        w = torch.randn((N, K), generator=gen, device=dev) * K ** -0.5
        pw = ops.PackedWeight.linear(w, torch.randn((N,), generator=gen, device=dev), dev)
        assert ops.gemm_fits(M, pw), (name, M, N, K)
        a = [torch.randn((M, K), generator=gen, device=dev).to(torch.bfloat16) for _ in range(args.sets)]
        o = [torch.randn((M, N), generator=gen, device=dev).to(torch.bfloat16) for _ in range(args.sets)]

        def fit(i):
            ops.gemm_fit(a[i], pw, o[i], residual=o[i] if has_res else None)

        def old(i):
            ops.gemm(a[i], pw, o[i], residual=o[i] if has_res else None)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for j in range(args.launches):
                fn(j % args.sets)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / args.launches

        for fn in (fit, old):                      # warm-up: code objects, LDS attribute, workspaces
            for i in range(args.sets):
                fn(i)
        variant = lib.dc_gemm_last_variant().decode()
        torch.cuda.synchronize()
        t = {"fit": [], "gemm": []}
        for _ in range(args.runs):
            t["fit"].append(timed(fit))
            t["gemm"].append(timed(old))
        _hip.check_error_word(name)
        r = dict(M=M, N=N, K=K, residual=has_res, gemm_variant=variant,
                 fit_us=[round(x, 2) for x in t["fit"]], gemm_us=[round(x, 2) for x in t["gemm"]],
                 fit_median_us=round(statistics.median(t["fit"]), 2), gemm_median_us=round(statistics.median(t["gemm"]), 2),
                 gemm_min_us=round(min(t["gemm"]), 2))
        r["win"] = r["fit_median_us"] < r["gemm_min_us"]
        r["fit_tflops"] = round(2.0 * M * N * K / r["fit_median_us"] * 1e-6, 1)
        res[name] = r
        print(name, json.dumps(r), flush=True)
        del a, o
    return dict(device=torch.cuda.get_device_name(0), cus=cus, runs=args.runs, launches_per_run=args.launches, operand_sets=args.sets,
                shapes=res)


def resources():
    """Registers and scratch of gemm_fit_kernel, from hipcc's own remarks (-Rpass-analysis=kernel-resource-usage)."""
    src = os.path.join(ROOT, "dynamicrafter_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
           "-I" + os.path.join(ROOT, "include"), "-I" + src, "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(src, "gemm_fit.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    assert "gemm_fit_kernel" in err, err
    get = lambda key: int(re.search(key + r": (\d+)", err).group(1))
    out = dict(kernel="gemm_fit_kernel", vgprs=get(r" VGPRs"), agprs=get("AGPRs"), sgprs=get("TotalSGPRs"),
               scratch_bytes_per_lane=get(r"ScratchSize \[bytes/lane\]"), waves_per_simd=get(r"Occupancy \[waves/SIMD\]"))
    out["registers"] = out["vgprs"] + out["agprs"]
    assert out["registers"] <= 512 and out["scratch_bytes_per_lane"] == 0, out
    return out


def bench_lines(path):
    rows = []
    with open(path) as f:
        for line in f:
            if line.strip().startswith("{"):
                rows.append(json.loads(line))
    return rows


def step(args):
    import numpy as np
    new, parent = bench_lines(args.step[0]), bench_lines(args.step[1])
    ms = lambda rows: [r["ms_per_step"] for r in rows]
    out = dict(what="ms_per_step of the bench.py result lines in the two files (runs of this tree and of the parent commit, taken "
                    "alternately on one box), their medians, the gain and the spread (max - min) of the parent's runs",
               new_ms_per_step=ms(new), parent_ms_per_step=ms(parent))
    out["new_median"], out["parent_median"] = statistics.median(out["new_ms_per_step"]), statistics.median(out["parent_ms_per_step"])
    out["gain_ms"] = round(out["parent_median"] - out["new_median"], 3)
    out["parent_spread_ms"] = round(max(out["parent_ms_per_step"]) - min(out["parent_ms_per_step"]), 3)
    out["gain_exceeds_parent_spread"] = out["gain_ms"] > out["parent_spread_ms"]
    if args.dumps:
        rel = {}
        for name in ("x_prev", "pred_x0"):
            a = np.load(os.path.join(args.dumps[0], name + ".npy")).astype(np.float64)
            b = np.load(os.path.join(args.dumps[1], name + ".npy")).astype(np.float64)
            rel[name] = float(np.linalg.norm(a - b) / np.linalg.norm(b))
        out["rel_l2_new_vs_parent_after_timed_steps"] = rel
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--step", nargs=2, metavar=("NEW", "PARENT"))
    ap.add_argument("--dumps", nargs=2, metavar=("NEW_DIR", "PARENT_DIR"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_ab.json"))
    args = ap.parse_args()
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if args.resources:
        doc["code_object"] = resources()
    elif args.step:
        doc["step"] = step(args)
    else:
        doc["per_launch"] = measure(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc.get("code_object" if args.resources else "step" if args.step else "per_launch"))[:2000])


if __name__ == "__main__":
    main()

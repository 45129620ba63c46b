#!/usr/bin/env python3
"""Bit compare of the attention kernels between two builds of the library: this tree's and another one (the parent commit's,
built with `DC_OUT=<path> dynamicrafter_amd/csrc/build.sh` from its sources).

    python tools/attn_bitcompare.py --other-lib <path> [--listing profiles/<name>.txt]

A seeded list of launches - the smallest shapes that reach every instance of the kernels built on csrc/attn_parts.h and every
branch of the shared parts (the dispatch conditions of dc_flash_attn_d64, dc_cross_attn_dual_d64, dc_flash_pipe_launch and the
ln_qkv_tattn launcher decide which kernel a shape takes; the kernel named in a case is the one those conditions select) - runs
once per library, each library in its own fresh child processes (the other one selected through DC_HIP_LIB; switches that a
library reads once from its environment get a child of their own). The outputs are compared with torch.equal: one line per
case, then the totals. Exit status 1 if an output differs, 2 if a child process failed (nothing more runs then). A tool, not a
test; the child-process and compare plumbing is tools/gemm_bitcompare.py's.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_bitcompare import DEV, compare_saved, run_children  # noqa: E402

ENV_SETS = (("default", {}), ("pipe0", {"DC_FLASH_PIPE": "0"}))


def FA(kernel, Lq, Lk, **kw):
    return dict(kind="flash", kernel=kernel, Lq=Lq, Lk=Lk, **kw)


def cases():
    """B = 1, heads = 2 unless a case says otherwise."""
    out = []
    # one query block per wave (Lq < 512 or Lk < 256): a ragged single tile (masked keys, clamped rows), whole tiles, just under
    # the wide threshold; plain store and the accumulate epilogue; q / k / v as column slices with padded batch strides
    for Lq, Lk in ((40, 40), (144, 144), (530, 192)):
        out.append(FA("flash<1,false>", Lq, Lk))
        out.append(FA("flash<1,false>", Lq, Lk, acc=0.5))
    out.append(FA("flash<1,false>", 144, 144, B=2, fused=160))
    # two query blocks per wave where the pipelined kernel declines: accumulate, Lk % 64 != 0, DC_FLASH_PIPE=0
    out.append(FA("flash<2,false>", 512, 256, acc=0.5))
    out.append(FA("flash<2,false>", 530, 300))
    out.append(FA("flash<2,false>", 512, 256, env="pipe0"))
    # text + image sets, tile by tile (Lq < 512, or Lk outside (64, 96]) and resident; Lq 2304 with 45 (batch, head) pairs makes
    # the launcher choose two query tiles per workgroup (810 workgroups of one tile would need a second round of 768)
    for s2 in (1.0, 0.4):
        for Lq, Lk, Lk2 in ((300, 77, 16), (512, 64, 16), (144, 5, 3)):
            out.append(dict(kind="dual", kernel="flash<1,true>", Lq=Lq, Lk=Lk, Lk2=Lk2, s2=s2))
    for Lq, Lk, Lk2 in ((512, 77, 16), (530, 77, 16), (640, 65, 1), (1000, 96, 32)):
        out.append(dict(kind="dual", kernel="cross_resident", Lq=Lq, Lk=Lk, Lk2=Lk2, s2=0.7))
    out.append(dict(kind="dual", kernel="cross_resident", Lq=2304, Lk=77, Lk2=16, s2=1.0, B=9, heads=5))
    # the pipelined kernel: two query blocks per wave (Lq % 384 != 0), three; the tracking pass run directly (modes 1 and 3 with
    # threshold 0: every growth of a row maximum rescales the packed P); spiked keys
    for mode in ((0, 8.0), (1, 0.0), (3, 0.0)):
        for Lq, Lk in ((512, 256), (530, 320), (1000, 512)):
            out.append(FA("pipe<2>", Lq, Lk, mode=mode))
        for Lq, Lk in ((768, 256), (1152, 448)):
            out.append(FA("pipe<2>" if mode[0] & 2 else "pipe<3>", Lq, Lk, mode=mode))
        for L in (512, 768):
            out.append(FA("pipe<2>" if mode[0] & 2 or L % 384 else "pipe<3>", L, L, mode=mode, spikes=(130, 131)))
    for B, HW, C in ((1, 8, 320), (2, 72, 320), (1, 8, 640), (2, 72, 640)):
        out.append(dict(kind="tattn", kernel=f"ln_qkv_tattn<{C // 320}>", B=B, HW=HW, C=C))
    for B, T, HW, heads in ((1, 16, 7, 8), (1, 4, 33, 2)):
        out.append(dict(kind="temporal", kernel="temporal_attn", B=B, T=T, HW=HW, heads=heads))
    for c in out:
        c["name"] = c["kernel"] + "/" + ",".join(f"{k}={v}" for k, v in c.items() if k not in ("kind", "kernel"))
    return out


def run_case(ops, torch, c):
    g = torch.Generator(device=DEV).manual_seed(4321)
    randn = lambda *s: torch.randn(*s, device=DEV, generator=g).to(torch.bfloat16)
    B, heads = c.get("B", 1), c.get("heads", 2)
    Cc = heads * 64
    lib = ops._hip.lib()
    if c["kind"] == "flash":
        Lq, Lk = c["Lq"], c["Lk"]
        if c.get("fused") or c.get("spikes"):                # q | k | v columns of one buffer (Lq == Lk), rows padded per batch item
            pitch = c.get("fused", Lq)
            qkv = torch.randn(B * pitch, 3 * Cc, device=DEV, generator=g)
            for n, pos in enumerate(c.get("spikes", ())):
                qkv[pos, Cc:2 * Cc] *= 6.0 + 0.6 * n
            qkv = qkv.to(torch.bfloat16)
            q, k, v = qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:]
        else:
            pitch = None
            q, k, v = randn(B * Lq, Cc), randn(B * Lk, Cc), randn(B * Lk, Cc)
        o = randn(q.shape[0], Cc) if c.get("acc") else torch.zeros(q.shape[0], Cc, dtype=torch.bfloat16, device=DEV)
        mode = c.get("mode", (0, 8.0))
        assert lib.dc_flash_attn_set_mode(*mode) == 0
        try:
            ops.flash_attn(q, k, v, o, batch=B, heads=heads, Lq=Lq, Lk=Lk, scale=0.125, accumulate=bool(c.get("acc")),
                           acc_scale=c.get("acc", 1.0), q_bstride=pitch, kv_bstride=pitch)
        finally:
            assert lib.dc_flash_attn_set_mode(0, 8.0) == 0
    elif c["kind"] == "dual":
        Lq, nt, ni = c["Lq"], c["Lk"], c["Lk2"]
        q, kv = randn(B * Lq, Cc), randn(B * (nt + ni), 4 * Cc)
        o = torch.zeros(B * Lq, Cc, dtype=torch.bfloat16, device=DEV)
        ops.cross_attn_dual(q, kv[:, :Cc], kv[:, Cc:2 * Cc], kv[nt:, 2 * Cc:3 * Cc], kv[nt:, 3 * Cc:], o, batch=B, heads=heads,
                            Lq=Lq, Lk=nt, Lk2=ni, scale=0.125, scale2=c["s2"], kv_bstride=nt + ni)
    elif c["kind"] == "tattn":
        C, M = c["C"], c["B"] * 16 * c["HW"]
        x = (torch.randn(M, C, device=DEV, generator=g) * 1.2 + 0.3).to(torch.bfloat16)
        w = torch.randn(3 * C, C, device=DEV, generator=g) * C ** -0.5 * 1.5
        gam = 1 + 0.2 * torch.randn(C, device=DEV, generator=g)
        bet = 0.3 * torch.randn(C, device=DEV, generator=g)
        o = torch.zeros(M, C, dtype=torch.bfloat16, device=DEV)
        ops.ln_qkv_temporal_attn(x, (gam, bet), ops.PackedWeight.linear(w.cpu(), None, DEV), o, B=c["B"], T=16, HW=c["HW"], scale=0.125)
    else:
        M = c["B"] * c["T"] * c["HW"]
        Cc = c["heads"] * 64
        o = torch.zeros(M, Cc, dtype=torch.bfloat16, device=DEV)
        ops.temporal_attn(randn(M, 3 * Cc), o, B=c["B"], T=c["T"], HW=c["HW"], heads=c["heads"], scale=0.125)
    torch.cuda.synchronize()
    ops._hip.check_error_word(c["name"])
    return o.cpu()


def child(out_dir, env_set):
    sys.path.insert(0, ROOT)
    import torch
    from dynamicrafter_amd import ops
    index = []
    for i, c in enumerate(cases()):
        if c.get("env", "default") != env_set:
            continue
        out = run_case(ops, torch, c)
        torch.save(out, os.path.join(out_dir, f"{i:03d}.pt"))
        index.append(dict(i=i, name=c["name"], shape=list(out.shape), label=c["kernel"]))
        print(f"{c['name']} {tuple(out.shape)}", flush=True)
    json.dump(index, open(os.path.join(out_dir, f"index_{env_set}.json"), "w"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--other-lib", help="the library to compare this tree's against (selected through DC_HIP_LIB)")
    ap.add_argument("--listing", help="also write the listing to this file")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--env-set", default="default", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.env_set)
    if not args.other_lib or not os.path.exists(args.other_lib):
        ap.error("--other-lib: no such file")
    tmp = tempfile.mkdtemp(prefix="attn_bitcompare_")
    try:
        dirs = run_children(__file__, args.other_lib, args.timeout, tmp, ENV_SETS)
        if dirs is None:
            return 2
        for d in dirs.values():                        # one index per library, in case order
            parts = [e for name, _ in ENV_SETS for e in json.load(open(os.path.join(d, f"index_{name}.json")))]
            json.dump(sorted(parts, key=lambda e: e["i"]), open(os.path.join(d, "index.json"), "w"))
        lines, differ, _, same_count = compare_saved(dirs)
        text = "\n".join(lines) + "\n"
        sys.stdout.write(text)
        if args.listing:
            open(args.listing, "w").write(text)
        return 1 if differ or not same_count else 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())

"""Same-box effect of K/V token downsampling (UNetModel.enable_token_downsampling, csrc/token_pool.hip) on the captured DDIM
step, in one process on one MI355X, at the 512 and the 1024 config's latents with bench.py's model and inputs, two guidance
branches.

usage: python tools/todo_ab.py [--res 512 1024] [--n 5] [--blocks 4] [--out profiles/todo_ab.json] [--off_only]

Timed per config, each as n replays of a captured step from a rewound run, host clock around work that ends in a device
synchronise:
  off        token downsampling disabled (what bench.py replays)
  f2_l0      factor 2 at level 0            f2_l01   factor 2 at levels 0 and 1            f4_l0   factor 4 at level 0
  (mode "nearest"; "mean" differs by the pooling kernel alone, which the launch table prices with --mean)
One warm-up block, then --blocks alternating blocks; per-step medians and ranges. Then, per setting, ONE traced eager UNet
evaluation (ops.Tracer, HIP events around every launch): per distinct shape the launches and the mean time of
flash_attn_d64(self), the pooling kernel, and the projections around them - ln_linear (the fused LayerNorm + qkv or q
projection) and the GEMM that projects kv - so that what the attention saves stands beside what the q / kv split costs.
--off_only times the off runs alone and touches nothing the parent commit lacks: the same script runs in a checkout of the
parent for the same-job comparison. Prints one JSON object (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SETTINGS = {"f2_l0": dict(factor=2, levels=(0,)), "f2_l01": dict(factor=2, levels=(0, 1)), "f4_l0": dict(factor=4, levels=(0,))}
WATCHED = ("flash_attn_d64(self)", "ln_pool_tokens", "ln_linear")


def traced_rows(ops, _hip, fn, watch_gemm):
    """One call of fn under ops.Tracer -> rows (kernel, GFLOP and MB of one launch, launches, mean us), one per kernel family and
    distinct work size, for the watched families and for the GEMMs whose (M, N, K) is in watch_gemm."""
    l = _hip.lib()
    with ops.Tracer() as tr:
        fn()
        torch.cuda.synchronize()
        recs, tr.records = tr.records, []
    rows = {}
    for name, flops, nbytes, e0, e1, tag in recs:
        ms = C.c_float()
        _hip.check(l.dc_event_elapsed_ms(e0, e1, C.byref(ms)), "dc_event_elapsed_ms")
        l.dc_event_destroy(e0); l.dc_event_destroy(e1)
        is_gemm = isinstance(tag, tuple) and len(tag) == 4 and tag[0] == 0 and tuple(tag[1:]) in watch_gemm
        if not (name.startswith(WATCHED) or is_gemm):
            continue
        key = (name, str(tag) if tag is not None else "", round(flops / 1e9, 3), round(nbytes / 1e6, 2))
        d = rows.setdefault(key, dict(launches=0, ms=0.0))
        d["launches"] += 1; d["ms"] += ms.value
    return [dict(kernel=k[0], tag=k[1], gflop=k[2], mbytes=k[3], launches=d["launches"], us=round(d["ms"] / d["launches"] * 1e3, 2),
                 total_ms=round(d["ms"], 3)) for k, d in sorted(rows.items())]


def one_config(res, args, bench, ops, _hip):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler, FusedRun
    dev = torch.device("cuda:0")
    bench.log(f"building inference_{res} model (random init)")
    model, _ = bench.build_model(res, dev)
    net = model.model.diffusion_model
    inp = {k: v.to(dev) for k, v in bench.make_clip_inputs(res, 1).items()}
    cond = {"c_crossattn": [inp["cond_ctx"]], "c_concat": [inp["c_concat"]]}
    uc = {"c_crossattn": [inp["uc_ctx"]], "c_concat": [inp["c_concat"]]}
    x_T = inp["x_T"].float().contiguous()
    S, n = bench.S_STEPS, args.n
    noises = torch.randn((S,) + tuple(x_T.shape), generator=torch.Generator().manual_seed(100)).to(dev)
    s = DDIMSampler(model)
    s.make_schedule(S, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)

    def new_run():
        return FusedRun(s, x_T.clone(), [cond, uc], fs=inp["fs"], noises=noises, cfg_scale=7.5, guidance_rescale=0.7)

    runs = {"off": new_run().capture()}
    settings = {} if args.off_only else {k: dict(v, mode="mean" if args.mean else "nearest") for k, v in SETTINGS.items()}
    for k, cfg in settings.items():                     # the setting decides the launches: it is part of the capture
        net.enable_token_downsampling(**cfg)
        runs[k] = new_run().capture()
    if settings:
        net.disable_token_downsampling()
    bench.log("runs captured")

    def timed(run):
        run.rewind(x_T)
        t0 = time.perf_counter()
        for _ in range(n):
            run.step()
        run.sync()
        return (time.perf_counter() - t0) * 1e3 / n

    for r in runs.values():
        timed(r)
    per = {k: [] for k in runs}
    for b in range(args.blocks):
        for k, r in runs.items():
            per[k].append(timed(r))
        bench.log(f"block {b + 1} of {args.blocks}")
    med = {k: sorted(v)[len(v) // 2] for k, v in per.items()}
    out = dict(latent=list(x_T.shape), branches=2, steps_per_block=n, blocks=args.blocks,
               ms_per_step_blocks={k: [round(x, 3) for x in v] for k, v in per.items()},
               ms_per_step_median={k: round(v, 3) for k, v in med.items()},
               ms_per_step_range={k: [round(min(v), 3), round(max(v), 3)] for k, v in per.items()},
               finite={k: bool(torch.isfinite(r.img).all().item()) for k, r in runs.items()})
    if settings:
        out["settings"] = {k: dict(v, levels=list(v["levels"])) for k, v in settings.items()}
        out["on_minus_off_ms"] = {k: round(med[k] - med["off"], 3) for k in med if k != "off"}
        # one traced eager evaluation per setting; the GEMMs to watch: per level l with width C_l and rows M_l of the two-branch
        # batch the qkv GEMM [M_l, 3 C_l, C_l] (levels 2 / 3; at levels 0 / 1 qkv and q go through ln_linear) and, at a selected
        # level, the kv GEMM [M_l / f^2, 2 C_l, C_l]
        probe = new_run()
        B2, T, H, W = 2 * x_T.shape[0], x_T.shape[2], x_T.shape[3], x_T.shape[4]
        widths = [m * net.model_channels for m in net.channel_mult]
        launches = {}
        for k, cfg in dict(off=None, **settings).items():
            watch = set()
            for lvl, Cl in enumerate(widths):
                h, w = -(-H // 2 ** lvl), -(-W // 2 ** lvl)
                M = B2 * T * h * w
                watch.add((M, 3 * Cl, Cl))
                if cfg is not None and lvl in cfg["levels"]:
                    hp, wp = ops.pooled_grid(h, w, cfg["factor"])
                    watch.add((B2 * T * hp * wp, 2 * Cl, Cl))
            net.set_token_downsampling(cfg)
            ev = lambda: model.apply_model_rows(probe.img, probe.prep, probe.t_table, t_index=probe.counter)
            ev(); torch.cuda.synchronize()              # warm: buffers of this setting allocated
            launches[k] = traced_rows(ops, _hip, ev, watch)
        net.disable_token_downsampling()
        out["traced_launches"] = launches
    del runs, model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", nargs="+", default=["512", "1024"], choices=["1024", "512", "256"])
    ap.add_argument("--n", type=int, default=5, help="replays of the captured step per timed block")
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--mean", action="store_true", help="mode 'mean' instead of 'nearest'")
    ap.add_argument("--out", default=None)
    ap.add_argument("--off_only", action="store_true")
    args = ap.parse_args()
    import bench
    from dynamicrafter_amd import _hip, ops
    out = dict(mode="off only" if args.off_only else "mean" if args.mean else "nearest",
               kernel_source_hash=bench.kernel_source_hash(), device=torch.cuda.get_device_name(0), host=os.uname().nodename,
               configs={res: one_config(res, args, bench, ops, _hip) for res in args.res})
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

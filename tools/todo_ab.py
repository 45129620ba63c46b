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

import torch

import step_ab

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
    c = step_ab.setup(res)
    model, net, x_T = c.model, c.net, c.x_T
    new_run = lambda: c.new_run(guidance_rescale=0.7)

    runs = {"off": new_run().capture()}
    settings = {} if args.off_only else {k: dict(v, mode="mean" if args.mean else "nearest") for k, v in SETTINGS.items()}
    for k, cfg in settings.items():                     # the setting decides the launches: it is part of the capture
        net.enable_token_downsampling(**cfg)
        runs[k] = new_run().capture()
    if settings:
        net.disable_token_downsampling()
    bench.log("runs captured")

    per, med = step_ab.alternate({k: (lambda r=r: step_ab.timed(r, x_T, args.n)) for k, r in runs.items()}, args.blocks, bench.log)
    out = dict(latent=list(x_T.shape), branches=2, steps_per_block=args.n, blocks=args.blocks,
               **step_ab.timing_fields(per, med), finite=step_ab.finite(runs))
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
    out = dict(mode="off only" if args.off_only else "mean" if args.mean else "nearest", **step_ab.header(bench),
               configs={res: one_config(res, args, bench, ops, _hip) for res in args.res})
    step_ab.emit(out, args.out)


if __name__ == "__main__":
    main()

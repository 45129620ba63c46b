"""Same-box A/B of the captured denoising step at the trained size (bench.py's step) and the captured TILED step on a
latent of twice the trained width (samplers/tiles.py: 3 boxes of the trained size at a stride of half a box, two
branches), with all boxes in one batched UNet call and with one box per call, at one config; plus the two tile kernels
alone with their bytes, and the UNet scratch each run adds.

usage: python tools/tile_ab.py [--res 512] [--steps 5] [--blocks 4] [--parent-tree DIR] [--out FILE]
The runs share the model and the context; their captured steps are replayed in alternating blocks of --steps launches
(HIP events on the graph stream), so clock drift hits all alike. `ratio` is the tiled step over W plain steps: below 1,
batching the boxes is cheaper than denoising them as separate clips.
--parent-tree DIR: a built checkout of the commit to compare against; its plain captured step is timed by ITS
tools/sampler_ab.py in a fresh child process, once before and once after this process's blocks (window_ab.py's
parent_plain_blocks, with the coupling described there).
Prints one JSON object (and writes it to --out)."""
import argparse
import os

import torch

import step_ab
from window_ab import parent_plain_blocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="512", choices=["1024", "512", "256"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    parent, parent_hash = [], None
    if args.parent_tree:                                        # before this process opens the GPU
        blk, parent_hash = parent_plain_blocks(os.path.abspath(args.parent_tree), args.res, args.steps, args.blocks)
        parent += blk
    c = step_ab.setup(args.res)
    bench, model, net, inp, dev, s, S = c.bench, c.model, c.net, c.inp, c.dev, c.sampler, c.S
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.lvdm.models.samplers.ddim import FusedRun, tiled
    B, Cx, T, H, Wd = c.x_T.shape
    WL = 2 * Wd
    g = torch.Generator().manual_seed(101)
    x_long = torch.randn(B, Cx, T, H, WL, generator=g).to(dev)
    cc_long = torch.cat([inp["c_concat"], inp["c_concat"]], dim=4).contiguous()
    noises_long = torch.randn((S,) + tuple(x_long.shape), generator=g).to(dev)
    br_long = [{"c_crossattn": [inp["cond_ctx"]], "c_concat": [cc_long]}, {"c_crossattn": [inp["uc_ctx"]], "c_concat": [cc_long]}]
    tile = dict(T=T, h=H, w=Wd, stride=(1, H, Wd // 2), weights="triangle", shift=(0, 0, 0))
    x_T = {"plain": c.x_T, "tiled": x_long, "tiled_per_call_1": x_long}
    runs, scratch = {}, {}
    for name in x_T:
        before = net._arena.nbytes()
        if name == "plain":
            runs[name] = c.new_run(guidance_rescale=0.7).capture()
        else:
            runs[name] = tiled(FusedRun)(s, x_long.clone(), br_long, tile=dict(tile, per_call=1 if name.endswith("_1") else None),
                                         fs=inp["fs"], noises=noises_long, cfg_scale=7.5, guidance_rescale=0.7).capture()
        scratch[name] = net._arena.nbytes() - before           # the arena is shape-keyed: what this run's shapes added
    tr = runs["tiled"]
    W = tr.plan["W"]
    assert W == 3 and tr.prep["tile"]["n_w"] == 3 and runs["tiled_per_call_1"].prep["tile"]["n_w"] == 1
    bench.log(f"three steps captured: W = {W} boxes of {T} x {H} x {Wd} in {T} x {H} x {WL}")
    per, med = step_ab.alternate({k: (lambda k=k: step_ab.timed_events(runs[k], x_T[k], args.steps)) for k in runs}, args.blocks)
    finite = step_ab.finite(runs)
    if args.parent_tree:                                        # and after, with this process idle
        parent += parent_plain_blocks(os.path.abspath(args.parent_tree), args.res, args.steps, args.blocks)[0]
        bench.log(f"parent tree's plain step: {len(parent)} blocks in two fresh processes")

    # the kernels alone, eager on the current stream, on this latent: 2 branches, all W boxes in one launch
    M = B * W * T * H * Wd
    ML = B * T * H * WL
    xr = torch.empty(M, 64, dtype=torch.bfloat16, device=dev)
    e_w = torch.randn(2 * M, 4, device=dev)
    e_l = torch.empty(2 * ML, 4, device=dev)
    kern = {
        "dc_pack_latent_tiles": (lambda: ops.pack_latent_tiles(x_long, cc_long, xr, tr.plan, B=B, Cx=Cx, Cc=cc_long.shape[1]),
                                 M * (8 * 4 + 64 * 2)),
        "dc_tile_merge": (lambda: ops.tile_merge(e_w, e_l, tr.plan, nb=2, B=B, C=4), (2 * M + 2 * ML) * 16),
    }
    kern_us = {}
    for k, (fn, nbytes) in kern.items():
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(100):
            fn()
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) / 100 * 1e3
        kern_us[k] = dict(us=round(us, 1), mbytes=round(nbytes / 1e6, 2), tbs=round(nbytes / us / 1e6, 3))
    pmed = sorted(parent)[len(parent) // 2] if parent else None
    out = dict(res=args.res, latent=[T, H, WL], box=[T, H, Wd], stride=[1, H, Wd // 2], boxes=W,
               max_boxes_per_call=model.max_windows_per_call(tuple(x_long.shape), 2, T, hw=(H, Wd)),
               steps_per_block=args.steps, blocks=args.blocks, **step_ab.timing_fields(per, med, ranges=False),
               ratio_tiled_over_W_plain=round(med["tiled"] / (W * med["plain"]), 4),
               ratio_tiled_per_call_1_over_W_plain=round(med["tiled_per_call_1"] / (W * med["plain"]), 4),
               parent_plain_ms_per_step_blocks=[round(x, 3) for x in parent] or None,
               parent_plain_ms_per_step_median=round(pmed, 3) if parent else None,
               ratio_tiled_over_W_parent_plain=round(med["tiled"] / (W * pmed), 4) if parent else None,
               ratio_tiled_per_call_1_over_W_parent_plain=round(med["tiled_per_call_1"] / (W * pmed), 4) if parent else None,
               parent_kernel_source_hash=parent_hash, kernels=kern_us,
               unet_scratch_mbytes={k: round(v / 1e6, 1) for k, v in scratch.items()}, finite=finite,
               **step_ab.header(bench, host=False))
    step_ab.emit(out, args.out)


if __name__ == "__main__":
    main()

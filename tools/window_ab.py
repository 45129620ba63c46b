"""Same-box A/B of the captured denoising step on one 16-frame clip (bench.py's step) and the captured WINDOWED step on a
longer clip (samplers/windows.py: T_long frames as W overlapping 16-frame windows, one batched UNet call per chunk),
at one config, plus the two window kernels alone next to dc_pack_latent and dc_ddim_step, and the UNet scratch each
run adds.

usage: python tools/window_ab.py [--res 1024] [--frames 32] [--stride 8] [--per-call N] [--steps 5] [--blocks 4]
                                 [--parent-tree DIR] [--out FILE]
Both runs share the model and the conditioning; their captured steps are replayed in alternating blocks of --steps
launches (HIP events on the graph stream), so clock drift hits both alike. `ratio` is the windowed step over W plain
steps: below 1, batching the windows is cheaper than denoising them as separate clips.
--parent-tree DIR: a built checkout of the commit to compare against (its own library next to its sources). Its plain
captured step is timed by ITS tools/sampler_ab.py in a fresh child process, once before and once after this process's
blocks, and `ratio_windowed_over_W_parent_plain` uses the median of those blocks. This couples the tool to that
script's output: its last stdout line must be a JSON object with `ms_per_step_blocks["ddim"]` (and, optionally,
`kernel_source_hash`); a tree whose sampler_ab.py prints something else makes this tool raise, not compare silently.
The default `python bench.py` runs, parent and new alternately, are not made here: they are separate processes of the
two trees, run by hand in the same job (profiles/README.md gives the commands next to the recorded results).
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys

import torch

import step_ab


def parent_plain_blocks(tree, res, steps, blocks):
    """ms per captured DDIM step, per block, measured by the tree's own tools/sampler_ab.py in a fresh process."""
    env = dict(os.environ)
    env.pop("DC_HIP_LIB", None)                                 # the tree loads the library built next to its sources
    r = subprocess.run([sys.executable, os.path.join(tree, "tools", "sampler_ab.py"), "--res", res, "--steps", str(steps),
                        "--blocks", str(blocks)], cwd=tree, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{tree}/tools/sampler_ab.py failed ({r.returncode}): {r.stderr[-2000:]}")
    try:
        out = json.loads(r.stdout.strip().splitlines()[-1])
        return [float(v) for v in out["ms_per_step_blocks"]["ddim"]], out.get("kernel_source_hash")
    except (IndexError, KeyError, TypeError, ValueError) as e:
        raise RuntimeError(f"{tree}/tools/sampler_ab.py did not print the JSON this tool reads "
                           f"(ms_per_step_blocks['ddim']): {e!r}") from e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="1024", choices=["1024", "512", "256"])
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--shift", type=int, default=0)
    ap.add_argument("--per-call", type=int, default=None)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    parent, parent_hash = [], None
    if args.parent_tree:                                        # before this process opens the GPU
        blk, parent_hash = parent_plain_blocks(os.path.abspath(args.parent_tree), args.res, args.steps, args.blocks)
        parent += blk
    import bench
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler, FusedRun, windowed
    from dynamicrafter_amd.lvdm.models.samplers.windows import window_plan
    dev = torch.device("cuda:0")
    bench.log(f"building inference_{args.res} model (random init)")
    model, _ = bench.build_model(args.res, dev)
    net = model.model.diffusion_model
    inp = {k: v.to(dev) for k, v in bench.make_clip_inputs(args.res, 1).items()}
    T, TL = inp["x_T"].shape[2], args.frames
    S = bench.S_STEPS
    g = torch.Generator().manual_seed(100)
    x_T = {"plain": inp["x_T"].float().contiguous(),
           "windowed": torch.randn(inp["x_T"].shape[:2] + (TL,) + inp["x_T"].shape[3:], generator=g).to(dev)}
    cc = {"plain": inp["c_concat"], "windowed": inp["c_concat"][:, :, :1].repeat(1, 1, TL, 1, 1).contiguous()}
    s = DDIMSampler(model)
    s.make_schedule(S, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
    runs, scratch = {}, {}
    for name in ("plain", "windowed"):
        cond = {"c_crossattn": [inp["cond_ctx"]], "c_concat": [cc[name]]}
        uc = {"c_crossattn": [inp["uc_ctx"]], "c_concat": [cc[name]]}
        noises = torch.randn((S,) + tuple(x_T[name].shape), generator=g).to(dev)
        before = net._arena.nbytes()
        kw = dict(fs=inp["fs"], noises=noises, cfg_scale=7.5, guidance_rescale=0.7)
        if name == "plain":
            runs[name] = FusedRun(s, x_T[name].clone(), [cond, uc], **kw).capture()
        else:
            window = dict(T=T, stride=args.stride, weights="triangle", shift=args.shift, per_call=args.per_call)
            runs[name] = windowed(FusedRun)(s, x_T[name].clone(), [cond, uc], window=window, **kw).capture()
        scratch[name] = net._arena.nbytes() - before           # the arena is shape-keyed: what this run's shapes added
    wr = runs["windowed"]
    W, n_w = wr.plan["W"], wr.prep["win"]["n_w"]
    W_real = window_plan(TL, T, args.stride, "triangle", args.shift, S)[0].shape[1]

    bench.log(f"both steps captured: W = {W_real} windows ({W} with padding), {n_w} per UNet call")
    per, med = step_ab.alternate({k: (lambda k=k: step_ab.timed_events(runs[k], x_T[k], args.steps)) for k in runs}, args.blocks)
    bench.log(f"timed {args.blocks} x {args.steps} steps of each")
    finite = step_ab.finite(runs)
    if args.parent_tree:                                        # and after, with this process idle
        parent += parent_plain_blocks(os.path.abspath(args.parent_tree), args.res, args.steps, args.blocks)[0]
        bench.log(f"parent tree's plain step: {len(parent)} blocks in two fresh processes")

    # the kernels alone, eager on the current stream, on this latent: 2 branches, all W windows in one launch
    B, Cx, _, H, Wd = x_T["windowed"].shape
    HW = H * Wd
    xl, ccl = x_T["windowed"], cc["windowed"]
    xr_w = torch.empty(B * W * T * HW, 64, dtype=torch.bfloat16, device=dev)
    xr_p = torch.empty(B * T * HW, 64, dtype=torch.bfloat16, device=dev)
    e_w = torch.randn(2 * B * W * T * HW, 4, device=dev)
    e_l = torch.empty(2 * B * TL * HW, 4, device=dev)
    xp, px0 = torch.empty_like(xl), torch.empty_like(xl)
    ws = ops.step_workspace(B, dev)
    ML = B * TL * HW
    n0 = torch.randn(xl.shape, device=dev)
    kern = {
        "dc_pack_latent_windows": (lambda: ops.pack_latent_windows(xl, ccl, xr_w, wr.plan, B=B, Cx=Cx, Cc=ccl.shape[1], HW=HW),
                                   B * W * T * HW * (8 * 4 + 64 * 2)),
        "dc_pack_latent_16_frames": (lambda: ops.pack_latent(x_T["plain"], cc["plain"], xr_p, B=B, Cx=Cx, Cc=ccl.shape[1],
                                                             T=T, HW=HW), B * T * HW * (8 * 4 + 64 * 2)),
        "dc_window_merge": (lambda: ops.window_merge(e_w, e_l, wr.plan, nb=2, B=B, C=4, HW=HW),
                            (2 * B * W * T * HW + 2 * ML) * 16),
        "dc_ddim_step_long_clip": (lambda: ops.ddim_step(s._tables, e_l[:ML], e_l[ML:], None, xl, n0, xp, px0, ws, B=B, Cc=4,
                                                         THW=TL * HW, index=5, v_param=model.parameterization == "v",
                                                         cfg_scale=7.5, guidance_rescale=0.7),
                                   ML * 16 * (2 * 2 + 4)),     # e_c, e_u read twice (statistics, apply); x, noise in; two out
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
        kern_us[k] = dict(us=round(us, 1), mbytes=round(nbytes / 1e6, 2), gbs=round(nbytes / us / 1e3, 1))
    out = dict(res=args.res, frames=TL, window=T, stride=args.stride, shift=args.shift, windows=W_real, windows_padded=W,
               windows_per_call=n_w, max_windows_per_call=model.max_windows_per_call(tuple(xl.shape), 2, T),
               steps_per_block=args.steps, blocks=args.blocks,
               **step_ab.timing_fields(per, med, ranges=False),
               ratio_windowed_over_W_plain=round(med["windowed"] / (W_real * med["plain"]), 4),
               parent_plain_ms_per_step_blocks=[round(x, 3) for x in parent] or None,
               parent_plain_ms_per_step_median=round(sorted(parent)[len(parent) // 2], 3) if parent else None,
               ratio_windowed_over_W_parent_plain=(round(med["windowed"] / (W_real * sorted(parent)[len(parent) // 2]), 4)
                                                   if parent else None),
               parent_kernel_source_hash=parent_hash,
               kernels=kern_us, unet_scratch_mbytes={k: round(v / 1e6, 1) for k, v in scratch.items()},
               finite=finite, **step_ab.header(bench, host=False))
    step_ab.emit(out, args.out)


if __name__ == "__main__":
    main()

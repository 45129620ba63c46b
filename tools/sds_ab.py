"""Same-box A/B of the captured SDS optimisation step (samplers/sds.py: noising pass, batched cond + uncond UNet,
SDS + Adam update) against the captured DDIM denoising step (bench.py's) at one config, plus the update kernels alone.

usage: python tools/sds_ab.py [--res 1024] [--steps 10] [--blocks 4] [--out FILE]
Both runs share the model and the conditioning; their captured steps are replayed in alternating blocks of --steps
launches (HIP events on the graph stream), so clock drift hits both alike. Prints one JSON object (and writes it to
--out)."""
import argparse

import torch

import step_ab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="1024", choices=["1024", "512", "256"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.lvdm.models.samplers import sds
    c = step_ab.setup(args.res, S=max(bench.S_STEPS, args.steps))
    model, dev, inp, cond, uc, x_T, S, noises, s = c.model, c.dev, c.inp, c.cond, c.uc, c.x_T, c.S, c.noises, c.sampler
    width = x_T.shape[-1] * 8
    spacing, phi = sds.default_timestep_spacing(width), sds.default_guidance_rescale(width)
    s.make_schedule(S, ddim_discretize=spacing, ddim_eta=1.0, verbose=False)
    runs = {"ddim": c.new_run(guidance_rescale=phi).capture()}
    # the SDS step with the reference's defaults: t on the 50-step grid, "t" weighting, Adam lr 0.05, CFG 7.5
    grid = sds.timestep_grid(model.num_timesteps, spacing)
    lo, hi = sds.step_bounds(len(grid), 0.02, 0.98)
    torch.manual_seed(100)
    t_draws = torch.stack([sds.draw_timesteps(grid, lo, hi, x_T.shape[0]) for _ in range(S)])
    c1, c2, w = sds.noise_tables(model.alphas_cumprod, t_draws)
    step_size, bc2_sqrt = sds.adam_tables(S, 0.05, sds.OPTIMIZERS["Adam"]["betas"])
    tables = {k: v.reshape(-1).contiguous().to(dev) for k, v in
              (("c1", c1), ("c2", c2), ("w", w), ("step_size", step_size), ("bc2_sqrt", bc2_sqrt))}
    runs["sds"] = sds.SdsRun(model, x_T.clone(), [cond, uc], tables, t_draws, noises, fs=inp["fs"], cfg_scale=7.5,
                             guidance_rescale=phi).capture()

    bench.log("both steps captured")
    per, med = step_ab.alternate({k: (lambda r=r: step_ab.timed_events(r, x_T, args.steps)) for k, r in runs.items()}, args.blocks)
    bench.log(f"timed {args.blocks} x {args.steps} steps of each")
    finite = step_ab.finite(runs)

    # the update kernels alone, eager on the current stream: 2 branches as channels-last rows
    B, Cc = x_T.shape[0], x_T.shape[1]
    THW = x_T[0, 0].numel()
    e = torch.randn(2 * B * THW, Cc, device=dev)
    x, xp, px0 = x_T.clone(), torch.empty_like(x_T), torch.empty_like(x_T)
    xt, m, v = torch.empty_like(x_T), torch.zeros_like(x_T), torch.zeros_like(x_T)
    loss = torch.zeros(S, device=dev)
    ws = torch.empty(16 * B * 256, device=dev)
    M = B * THW
    kw = dict(B=B, Cc=Cc, THW=THW, index=5, cfg_scale=7.5, guidance_rescale=phi)
    upd = {"ddim": lambda: ops.ddim_step(s._tables, e[:M], e[M:], None, x, noises[0], xp, px0, ws,
                                         v_param=model.parameterization == "v", **kw),
           "sds": lambda: (ops.sds_noise(tables, x, noises[5], xt, B=B, index=5),
                           ops.sds_step(tables, e[:M], e[M:], xt, x, m, v, ws, loss, **kw))}
    kern_us = {}
    for k, fn in upd.items():
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(200):
            fn()
        b.record()
        torch.cuda.synchronize()
        kern_us[k] = a.elapsed_time(b) / 200 * 1e3
    out = dict(res=args.res, steps_per_block=args.steps, blocks=args.blocks, **step_ab.timing_fields(per, med, ranges=False),
               sds_minus_ddim_ms=round(med["sds"] - med["ddim"], 3),
               sds_over_ddim=round(med["sds"] / med["ddim"], 4),
               update_kernels_us={k: round(v, 1) for k, v in kern_us.items()},
               finite=finite, **step_ab.header(bench, host=False))
    step_ab.emit(out, args.out)


if __name__ == "__main__":
    main()

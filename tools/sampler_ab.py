"""Same-box A/B of the captured denoising step with the DDIM update (bench.py's step) and with the DPM-Solver++ 2M SDE
update (samplers/dpm_solver.py) at one config, plus the two update kernels alone on that latent.

usage: python tools/sampler_ab.py [--res 1024] [--steps 10] [--blocks 4] [--out FILE]
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
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler, DpmRun
    c = step_ab.setup(args.res)
    bench, dev, x_T, noises = c.bench, c.dev, c.x_T, c.noises
    dpm = DPMSolverSampler(c.model, solver="dpmpp_2m_sde")
    dpm.make_schedule(c.S, ddim_discretize="uniform_trailing", verbose=False)
    runs = {"ddim": c.new_run(guidance_rescale=0.7).capture(),
            "dpmpp_2m_sde": DpmRun(dpm, x_T.clone(), [c.cond, c.uc], fs=c.inp["fs"], noises=noises, cfg_scale=7.5,
                                   guidance_rescale=0.7).capture()}
    bench.log("both steps captured")
    per, med = step_ab.alternate({k: (lambda r=r: step_ab.timed_events(r, x_T, args.steps)) for k, r in runs.items()}, args.blocks)
    bench.log(f"timed {args.blocks} x {args.steps} steps of each")
    finite = step_ab.finite(runs)

    # the update kernels alone, eager on the current stream: 2 branches as channels-last rows, guidance rescale on
    B, Cc = x_T.shape[0], x_T.shape[1]
    THW = x_T[0, 0].numel()
    e = torch.randn(2 * B * THW, Cc, device=dev)
    x, xp, px0 = x_T.clone(), torch.empty_like(x_T), torch.empty_like(x_T)
    ws = torch.empty(16 * B * 256, device=dev)
    hist = torch.zeros((2,) + tuple(x_T.shape), device=dev)
    kw = dict(B=B, Cc=Cc, THW=THW, index=5, v_param=True, cfg_scale=7.5, guidance_rescale=0.7)
    M = B * THW
    upd = {"ddim": lambda: ops.ddim_step(runs["ddim"].sampler._tables, e[:M], e[M:], None, x, noises[0], xp, px0, ws,
                                         **kw),
           "dpmpp_2m_sde": lambda: ops.dpmpp_step(runs["dpmpp_2m_sde"].sampler._tables, e[:M], e[M:], None, x,
                                                  noises[0], xp, px0, ws, hist, **kw)}
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
               dpm_minus_ddim_ms=round(med["dpmpp_2m_sde"] - med["ddim"], 3),
               update_kernels_us={k: round(v, 1) for k, v in kern_us.items()},
               finite=finite, **step_ab.header(bench, host=False))
    step_ab.emit(out, args.out)


if __name__ == "__main__":
    main()

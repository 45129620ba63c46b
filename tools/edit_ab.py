"""Same-box timing of the video-editing runs (samplers/ddim.py: InvertRun, partial FusedRun) next to the DDIM step of
the same process, at one config with bench.py's model and inputs.

usage: python tools/edit_ab.py [--res 512] [--n 25] [--blocks 4] [--out profiles/edit_ab.json]

Timed, each as n steps from a rewound run, host clock around work that ends in a device synchronise:
  ddim_graph_nb{1,2}      the captured DDIM step of a full run (what bench.py replays), one and two guidance branches
  invert_eager_nb{1,2}    `encode`'s run, launched eagerly
  invert_graph_nb{1,2}    the same, captured
  decode_graph_nb2        `decode(t_start = n)` as a partial FusedRun, captured
  decode_generic_nb2      `decode(t_start = n)` through separate apply_model calls: what decode ran before the partial run
One warm-up block, then --blocks alternating blocks; per-step medians and ranges. Prints one JSON object (and writes it
to --out). The question it answers: does an inversion step cost what a DDIM step of the same branch count costs?"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Generic:
    """The model without its batched entry: the sampler takes the generic path."""

    def __init__(self, model):
        self._m = model

    def __getattr__(self, name):
        if name in ("apply_model_rows", "_m"):
            raise AttributeError(name)
        return getattr(self._m, name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="512", choices=["1024", "512", "256"])
    ap.add_argument("--n", type=int, default=25, help="steps of the inversion and of the partial denoise (of bench.S_STEPS)")
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler, FusedRun, InvertRun
    dev = torch.device("cuda:0")
    bench.log(f"building inference_{args.res} model (random init)")
    model, _ = bench.build_model(args.res, dev)
    inp = {k: v.to(dev) for k, v in bench.make_clip_inputs(args.res, 1).items()}
    cond = {"c_crossattn": [inp["cond_ctx"]], "c_concat": [inp["c_concat"]]}
    uc = {"c_crossattn": [inp["uc_ctx"]], "c_concat": [inp["c_concat"]]}
    x_T = inp["x_T"].float().contiguous()
    S, n = bench.S_STEPS, args.n
    noises = torch.randn((S,) + tuple(x_T.shape), generator=torch.Generator().manual_seed(100)).to(dev)
    s = DDIMSampler(model)
    s.make_schedule(S, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
    g2 = dict(cfg_scale=7.5, guidance_rescale=0.7)
    runs = {
        "ddim_graph_nb1": FusedRun(s, x_T.clone(), [cond], fs=inp["fs"], noises=noises).capture(),
        "ddim_graph_nb2": FusedRun(s, x_T.clone(), [cond, uc], fs=inp["fs"], noises=noises, **g2).capture(),
        "invert_eager_nb1": InvertRun(s, x_T.clone(), [cond], n, fs=inp["fs"]),
        "invert_graph_nb1": InvertRun(s, x_T.clone(), [cond], n, fs=inp["fs"]).capture(),
        "invert_eager_nb2": InvertRun(s, x_T.clone(), [cond, uc], n, fs=inp["fs"], **g2),
        "invert_graph_nb2": InvertRun(s, x_T.clone(), [cond, uc], n, fs=inp["fs"], **g2).capture(),
        "decode_graph_nb2": FusedRun(s, x_T.clone(), [cond, uc], fs=inp["fs"], noises=noises[S - n:], last=n, **g2).capture(),
    }
    bench.log("runs built and captured")
    sg = DDIMSampler(Generic(model))
    sg.make_schedule(S, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)

    def timed_run(run):
        run.rewind(x_T)
        t0 = time.perf_counter()
        for _ in range(n):
            run.step()
        run.sync()
        return (time.perf_counter() - t0) * 1e3 / n

    def timed_generic():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sg.decode(x_T, cond, n, unconditional_guidance_scale=7.5, unconditional_conditioning=uc, fs=inp["fs"],
                        guidance_rescale=0.7, noises=noises[S - n:])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, out

    timers = {k: (lambda r=r: timed_run(r)) for k, r in runs.items()}
    timers["decode_generic_nb2"] = lambda: timed_generic()[0]
    for fn in timers.values():                                 # warm-up: every shape the timed window uses
        fn()
    bench.log("warmed up")
    per = {k: [] for k in timers}
    for b in range(args.blocks):
        for k, fn in timers.items():
            per[k].append(fn())
        bench.log(f"block {b + 1} of {args.blocks}")
    # the two decode paths agree (same inputs, same noises); every run's latent is finite
    runs["decode_graph_nb2"].rewind(x_T)
    for _ in range(n):
        runs["decode_graph_nb2"].step()
    runs["decode_graph_nb2"].sync()
    gen = timed_generic()[1]
    fused = runs["decode_graph_nb2"].img
    rel = float((fused - gen).norm() / gen.norm())
    finite = {k: bool(torch.isfinite(r.img).all().item()) for k, r in runs.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in per.items()}
    out = dict(res=args.res, latent=list(x_T.shape), schedule_steps=S, steps_per_block=n, blocks=args.blocks,
               ms_per_step_blocks={k: [round(x, 3) for x in v] for k, v in per.items()},
               ms_per_step_median={k: round(v, 3) for k, v in med.items()},
               ms_per_step_range={k: [round(min(v), 3), round(max(v), 3)] for k, v in per.items()},
               invert_over_ddim_graph={f"nb{b}": round(med[f"invert_graph_nb{b}"] / med[f"ddim_graph_nb{b}"], 4) for b in (1, 2)},
               decode_generic_over_graph=round(med["decode_generic_nb2"] / med["decode_graph_nb2"], 4),
               decode_fused_vs_generic_rel_l2=rel, finite=finite, kernel_source_hash=bench.kernel_source_hash(),
               device=torch.cuda.get_device_name(0), host=os.uname().nodename)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

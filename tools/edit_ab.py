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
import time

import torch

import step_ab


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
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler, FusedRun, InvertRun
    c = step_ab.setup(args.res)
    bench, model, inp, cond, uc, x_T, S, n, noises, s = c.bench, c.model, c.inp, c.cond, c.uc, c.x_T, c.S, args.n, c.noises, c.sampler
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

    def timed_generic():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sg.decode(x_T, cond, n, unconditional_guidance_scale=7.5, unconditional_conditioning=uc, fs=inp["fs"],
                        guidance_rescale=0.7, noises=noises[S - n:])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, out

    timers = {k: (lambda r=r: step_ab.timed(r, x_T, n)) for k, r in runs.items()}
    timers["decode_generic_nb2"] = lambda: timed_generic()[0]
    per, med = step_ab.alternate(timers, args.blocks, bench.log)         # the warm-up block: every shape the timed window uses
    # the two decode paths agree (same inputs, same noises); every run's latent is finite
    runs["decode_graph_nb2"].rewind(x_T)
    for _ in range(n):
        runs["decode_graph_nb2"].step()
    runs["decode_graph_nb2"].sync()
    gen = timed_generic()[1]
    fused = runs["decode_graph_nb2"].img
    rel = float((fused - gen).norm() / gen.norm())
    out = dict(res=args.res, latent=list(x_T.shape), schedule_steps=S, steps_per_block=n, blocks=args.blocks,
               **step_ab.timing_fields(per, med),
               invert_over_ddim_graph={f"nb{b}": round(med[f"invert_graph_nb{b}"] / med[f"ddim_graph_nb{b}"], 4) for b in (1, 2)},
               decode_generic_over_graph=round(med["decode_generic_nb2"] / med["decode_graph_nb2"], 4),
               decode_fused_vs_generic_rel_l2=rel, finite=step_ab.finite(runs), **step_ab.header(bench))
    step_ab.emit(out, args.out)


if __name__ == "__main__":
    main()

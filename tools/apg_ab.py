"""Same-box cost of adaptive projected guidance (`apg=`, csrc/guidance.hip) on the captured DDIM step, at one config with
bench.py's model and inputs, two guidance branches.

usage: python tools/apg_ab.py [--res 512] [--n 10] [--blocks 5] [--out profiles/apg_ab.json] [--off_only]
                              [--merge FILE --parent_json FILE ...]

Timed, each as n replays of a captured step from a rewound run, host clock around work that ends in a device synchronise:
  off          plain CFG at 7.5 with guidance_rescale 0.7 (what bench.py replays): one partial-sum launch + the update
  off_plain    plain CFG without guidance rescale: the update alone
  apg_x0       apg=dict(eta=0, norm_threshold=15, momentum=-0.5), space "x0": dc_apg_reduce + dc_apg_apply + the update
  apg_model    the same in space "model" (x is not read)
One warm-up block, then --blocks alternating blocks; per-step medians and ranges. Then the two APG launches alone, eager under
ops.Tracer on the outputs of one UNet forward (median of 5), with the achieved bytes/s on their algorithmic traffic.
--off_only times the off run alone: the same script runs in a checkout of the parent commit for the same-session comparison,
and --merge RESULT --parent_json FILES adds the JSON lines those runs printed to an earlier result as `parent_off` (no GPU).
Prints one JSON object (and writes it to --out)."""
import argparse
import json

import torch

import step_ab

SETTING = dict(eta=0.0, norm_threshold=15.0, momentum=-0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="512", choices=["1024", "512", "256"])
    ap.add_argument("--n", type=int, default=10, help="replays of the captured step per timed block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--off_only", action="store_true")
    ap.add_argument("--merge", default=None)
    ap.add_argument("--parent_json", nargs="*", default=[])
    args = ap.parse_args()
    out = json.load(open(args.merge)) if args.merge else measure(args)
    parent = []
    for path in args.parent_json:
        with open(path) as f:
            for line in f:
                if line.strip().startswith("{"):
                    d = json.loads(line)
                    parent.append(dict(ms_per_step_median=d["ms_per_step_median"]["off"], ms_per_step_range=d["ms_per_step_range"]["off"],
                                       kernel_source_hash=d["kernel_source_hash"], host=d["host"]))
    if parent:
        out["parent_off"] = parent
    step_ab.emit(out, args.out)


def measure(args):
    from dynamicrafter_amd import ops
    c = step_ab.setup(args.res)
    bench, x_T, new_run = c.bench, c.x_T, c.new_run
    runs = {"off": new_run(guidance_rescale=0.7).capture()}
    if not args.off_only:
        runs["off_plain"] = new_run().capture()
        runs["apg_x0"] = new_run(apg=dict(SETTING, space="x0")).capture()
        runs["apg_model"] = new_run(apg=dict(SETTING, space="model")).capture()
    bench.log("runs captured")

    per, med = step_ab.alternate({k: (lambda r=r: step_ab.timed(r, x_T, args.n)) for k, r in runs.items()}, args.blocks, bench.log)
    out = dict(res=args.res, latent=list(x_T.shape), branches=2, steps_per_block=args.n, blocks=args.blocks,
               **step_ab.timing_fields(per, med), finite=step_ab.finite(runs), **step_ab.header(bench))
    if not args.off_only:
        out["setting"] = SETTING
        out["minus_off_ms"] = {k: round(med[k] - med["off"], 3) for k in med if k != "off"}
        # the two launches alone, on the outputs of one forward; the run's buffers, host index 1 of the tables
        launches = {}
        for name in ("apg_x0", "apg_model"):
            run = runs[name]
            run.rewind(x_T)
            with torch.no_grad():
                e = run._evaluate()
            M = run.kw["B"] * run.kw["THW"]
            kw = dict(run.apg_kw, index=1)
            reps = []
            for rep in range(6):
                run.apg_m.zero_()
                with ops.Tracer() as tr:
                    ops.apg_guide(run.tables, e[:M], e[M:2 * M], run.img, run.apg_m, run.apg_out, run.apg_ws, **kw)
                    torch.cuda.synchronize()
                    summ = tr.summary()
                if rep:
                    reps.append(summ)
            rows = []
            for k in ("apg_reduce", "apg_apply"):
                ms = sorted(r[k]["ms"] for r in reps)[len(reps) // 2]
                nb = reps[0][k]["bytes"]
                rows.append(dict(kernel=k, us=round(ms * 1e3, 2), mbytes=round(nb / 1e6, 2),
                                 tb_per_s=round(nb / (ms * 1e-3) / 1e12, 3)))
            launches[name] = rows
        out["apg_launches"] = launches
        out["clip_active_at_step_1"] = {k: bool((runs[k].apg_m.double().norm() > SETTING["norm_threshold"]).item())
                                        for k in ("apg_x0", "apg_model")}
    return out


if __name__ == "__main__":
    main()

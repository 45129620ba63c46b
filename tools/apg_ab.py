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
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def measure(args):
    import bench
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler, FusedRun
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

    def new_run(**kw):
        return FusedRun(s, x_T.clone(), [cond, uc], fs=inp["fs"], noises=noises, cfg_scale=7.5, **kw)

    runs = {"off": new_run(guidance_rescale=0.7).capture()}
    if not args.off_only:
        runs["off_plain"] = new_run().capture()
        runs["apg_x0"] = new_run(apg=dict(SETTING, space="x0")).capture()
        runs["apg_model"] = new_run(apg=dict(SETTING, space="model")).capture()
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
    out = dict(res=args.res, latent=list(x_T.shape), branches=2, steps_per_block=n, blocks=args.blocks,
               ms_per_step_blocks={k: [round(x, 3) for x in v] for k, v in per.items()},
               ms_per_step_median={k: round(v, 3) for k, v in med.items()},
               ms_per_step_range={k: [round(min(v), 3), round(max(v), 3)] for k, v in per.items()},
               finite={k: bool(torch.isfinite(r.img).all().item()) for k, r in runs.items()},
               kernel_source_hash=bench.kernel_source_hash(), device=torch.cuda.get_device_name(0), host=os.uname().nodename)
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

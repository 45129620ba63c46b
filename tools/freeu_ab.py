"""Same-box cost of FreeU (UNetModel.enable_freeu, csrc/freeu.hip) on the captured DDIM step, at one config with bench.py's
model and inputs, two guidance branches.

usage: python tools/freeu_ab.py [--res 512] [--n 10] [--blocks 5] [--out profiles/freeu_ab.json] [--off_only]

Timed, each as n replays of a captured step from a rewound run, host clock around work that ends in a device synchronise:
  off      FreeU disabled (what bench.py replays)
  v1, v2   enable_freeu(0.9, 0.2, 1.4, 1.6, version=1 / 2), captured with it
One warm-up block, then --blocks alternating blocks; per-step medians and ranges. Then, per FreeU version, an eager UNet
forward under ops.Tracer: every FreeU launch's time (median of 3 forwards) and achieved bytes/s on its algorithmic traffic,
in situ between the kernels that surround it in a step. `traffic_bound_ms` is the selected cat buffers' traffic (skip columns
read twice and written once, the first half of h read and written once; version 2 reads all of h once more) at 3 and 4 TB/s.
--off_only times the off run alone: the same script runs in a checkout of the parent commit for the same-session comparison.
Prints one JSON object (and writes it to --out)."""
import argparse
import re

import torch

import step_ab

SETTING = dict(s1=0.9, s2=0.2, b1=1.4, b2=1.6)


def launch_bytes(name, F, H, W, ch, cs):
    rows = F * H * W
    return {"freeu_hmean": 2.0 * rows * ch + 4.0 * rows, "freeu_skip_stats": 2.0 * rows * cs + 28.0 * F * cs,
            "freeu_apply": 4.0 * rows * (cs + ch // 2)}[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="512", choices=["1024", "512", "256"])
    ap.add_argument("--n", type=int, default=10, help="replays of the captured step per timed block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--off_only", action="store_true")
    args = ap.parse_args()
    from dynamicrafter_amd import ops
    c = step_ab.setup(args.res)
    bench, model, net, x_T = c.bench, c.model, c.net, c.x_T
    new_run = lambda: c.new_run(guidance_rescale=0.7)

    runs = {"off": new_run().capture()}
    versions = () if args.off_only else (1, 2)
    for v in versions:                                  # the setting is a host constant of the capture
        net.enable_freeu(**SETTING, version=v)
        runs[f"v{v}"] = new_run().capture()
    if versions:
        net.disable_freeu()
    bench.log("runs captured")

    per, med = step_ab.alternate({k: (lambda r=r: step_ab.timed(r, x_T, args.n)) for k, r in runs.items()}, args.blocks, bench.log)
    out = dict(res=args.res, latent=list(x_T.shape), branches=2, steps_per_block=args.n, blocks=args.blocks,
               **step_ab.timing_fields(per, med), finite=step_ab.finite(runs), **step_ab.header(bench))
    if versions:
        out["setting"] = SETTING
        out["on_minus_off_ms"] = {k: round(med[k] - med["off"], 3) for k in med if k != "off"}
        probe = new_run()
        launches, bound = {}, {}
        for v in versions:
            net.enable_freeu(**SETTING, version=v)
            reps = []
            for rep in range(4):                        # the first forward warms the FreeU scratch up
                with ops.Tracer() as tr:
                    model.apply_model_rows(probe.img, probe.prep, probe.t_table, t_index=probe.counter)
                    torch.cuda.synchronize()
                    tr.summary()
                if rep:
                    reps.append({k: (d["ms"] / d["launches"], d["launches"]) for k, d in tr.detail.items()
                                 if k[0].startswith("freeu_")})
            rows = []
            for (name, tag) in reps[0]:                 # one row per kernel and distinct buffer shape: the mean over its launches
                F, H, W, ch, cs = (int(x) for x in re.match(r"F(\d+) (\d+)x(\d+) ch(\d+) cs(\d+)", tag).groups())
                ms = sorted(r[(name, tag)][0] for r in reps)[len(reps) // 2]
                nb = launch_bytes(name, F, H, W, ch, cs)
                rows.append(dict(kernel=name, shape=tag, launches_per_forward=reps[0][(name, tag)][1], us=round(ms * 1e3, 2),
                                 mbytes=round(nb / 1e6, 2), tb_per_s=round(nb / (ms * 1e-3) / 1e12, 3)))
            launches[f"v{v}"] = rows
            # the traffic bound over the ten selected buffers (every launch of a forward, not one per distinct shape)
            with ops.Tracer() as tr:
                model.apply_model_rows(probe.img, probe.prep, probe.t_table, t_index=probe.counter)
                torch.cuda.synchronize()
                summ = tr.summary()
            fu = {k: d for k, d in summ.items() if k.startswith("freeu_")}
            nbytes = sum(d["bytes"] for d in fu.values())
            # ops.freeu counts the skip columns once in the stats pass and twice (read + write) in the apply pass = the bound's 3x
            bound[f"v{v}"] = dict(launches=sum(d["launches"] for d in fu.values()), mbytes=round(nbytes / 1e6, 1),
                                  eager_ms=round(sum(d["ms"] for d in fu.values()), 3),
                                  traffic_bound_ms={"3TB/s": round(nbytes / 3e12 * 1e3, 3), "4TB/s": round(nbytes / 4e12 * 1e3, 3)})
        net.disable_freeu()
        out["freeu_launches"] = launches
        out["freeu_traffic"] = bound
    step_ab.emit(out, args.out)


if __name__ == "__main__":
    main()

"""What the *_ab.py tools that time a captured step share (a module, not a tool): bench.py's model and inputs at a --res, the
two guidance branches, seeded step noises, a scheduled DDIMSampler, a FusedRun factory, the two ways of timing n steps of a
rewound run, the loop of one warm-up block plus alternating blocks, and the JSON line every tool ends in."""
import ctypes as C
import json
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def setup(res, S=None, spacing="uniform_trailing", seed=100):
    """bench.py's random-init model and clip inputs of config `res` on cuda:0 -> a namespace: bench, model, net (its UNet),
    inp, the conditioning dicts cond / uc, x_T (fp32), S (default bench.S_STEPS), noises [S, *x_T.shape] from `seed`, sampler
    (a DDIMSampler scheduled for S steps at eta 1) and new_run(**kw), a FusedRun of [cond, uc] at guidance scale 7.5."""
    import bench
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler, FusedRun
    dev = torch.device("cuda:0")
    bench.log(f"building inference_{res} model (random init)")
    model, _ = bench.build_model(res, dev)
    inp = {k: v.to(dev) for k, v in bench.make_clip_inputs(res, 1).items()}
    c = types.SimpleNamespace(bench=bench, model=model, net=model.model.diffusion_model, inp=inp, dev=dev,
                              cond={"c_crossattn": [inp["cond_ctx"]], "c_concat": [inp["c_concat"]]},
                              uc={"c_crossattn": [inp["uc_ctx"]], "c_concat": [inp["c_concat"]]},
                              x_T=inp["x_T"].float().contiguous(), S=bench.S_STEPS if S is None else S)
    c.noises = torch.randn((c.S,) + tuple(c.x_T.shape), generator=torch.Generator().manual_seed(seed)).to(dev)
    c.sampler = DDIMSampler(model)
    c.sampler.make_schedule(c.S, ddim_discretize=spacing, ddim_eta=1.0, verbose=False)
    c.new_run = lambda **kw: FusedRun(c.sampler, c.x_T.clone(), [c.cond, c.uc], fs=inp["fs"], noises=c.noises, cfg_scale=7.5, **kw)
    return c


def timed(run, x_T, n):
    """ms per step of n steps from a rewound run: host clock around work that ends in a device synchronise."""
    run.rewind(x_T)
    t0 = time.perf_counter()
    for _ in range(n):
        run.step()
    run.sync()
    return (time.perf_counter() - t0) * 1e3 / n


def timed_events(run, x_T, n):
    """ms per step of n replays of a captured run from a rewind: HIP events on the graph's stream."""
    from dynamicrafter_amd import _hip
    l = _hip.lib()
    run.rewind(x_T)
    e0, e1 = C.c_void_p(), C.c_void_p()
    l.dc_event_create(C.byref(e0)); l.dc_event_create(C.byref(e1))
    l.dc_event_record(e0, run.graph._stream)
    for _ in range(n):
        run.step()
    l.dc_event_record(e1, run.graph._stream)
    run.sync()
    ms = C.c_float()
    l.dc_event_elapsed_ms(e0, e1, C.byref(ms))
    l.dc_event_destroy(e0); l.dc_event_destroy(e1)
    return ms.value / n


def alternate(timers, blocks, log=None):
    """One warm-up block, then `blocks` blocks, each calling every timer ({name: () -> ms per step}) in turn, so that clock
    drift hits all alike. Returns (per: {name: the blocks' values}, med: {name: their median})."""
    for fn in timers.values():
        fn()
    per = {k: [] for k in timers}
    for b in range(blocks):
        for k, fn in timers.items():
            per[k].append(fn())
        if log:
            log(f"block {b + 1} of {blocks}")
    return per, {k: sorted(v)[len(v) // 2] for k, v in per.items()}


def timing_fields(per, med, ranges=True):
    out = dict(ms_per_step_blocks={k: [round(x, 3) for x in v] for k, v in per.items()},
               ms_per_step_median={k: round(v, 3) for k, v in med.items()})
    if ranges:
        out["ms_per_step_range"] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in per.items()}
    return out


def finite(runs):
    return {k: bool(torch.isfinite(r.img).all().item()) for k, r in runs.items()}


def header(bench, host=True):
    """What identifies the build and the machine of a result."""
    out = dict(kernel_source_hash=bench.kernel_source_hash(), device=torch.cuda.get_device_name(0))
    return dict(out, host=os.uname().nodename) if host else out


def emit(out, path=None):
    """Prints the result as one JSON line and writes it to `path` (--out)."""
    line = json.dumps(out)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")

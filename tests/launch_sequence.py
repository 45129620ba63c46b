"""The ordered (kernel name, tag) list of one eager FusedRun step and one eager InvertRun step on the tiny UNet, two guidance
branches, a 2-step schedule: with every sampling option off, and with freeu + token_downsampling (+ apg on the FusedRun; an
inversion has none) on. tests/test_launch_sequence_gpu.py compares against tests/golden/launch_sequence.json, which

    python -m tests.launch_sequence tests/golden/launch_sequence.json

writes on a GPU. The fixture was recorded with this script on the commit before samplers/options.py existed; it uses nothing
newer (the settings are enabled on the UNet by hand), so it runs there unchanged."""
import json
import sys

import torch

DEV = "cuda:0"
FREEU = dict(s1=0.9, s2=0.2, b1=1.4, b2=1.6, version=2)
TODO = dict(factor=2, levels=(0, 1, 2), mode="mean")
APG = dict(eta=0.0, norm_threshold=20.0, momentum=-0.5)
S = 2


def inputs(seed=21, b=1, t=4, h=16, w=16):
    g = torch.Generator().manual_seed(seed)
    ctx = [torch.randn(b, 77 + 16 * t, 128, generator=g) for _ in range(2)]
    cc = (torch.randn(b, 4, t, h, w, generator=g) * 0.2).to(DEV)
    return dict(x=torch.randn(b, 4, t, h, w, generator=g).to(DEV), noises=torch.randn(S, b, 4, t, h, w, generator=g).to(DEV),
                fs=torch.tensor([24] * b).to(DEV), branches=[{"c_crossattn": [c.to(DEV)], "c_concat": [cc]} for c in ctx])


def traced_step(run, x):
    """[[kernel name, tag], ...] of the run's second eager step from a rewind (the first one allocates and packs)."""
    from dynamicrafter_amd import ops
    run.step()
    run.rewind(x)
    with ops.Tracer() as tr:
        run.step()
        launches = [[r[0], "" if r[5] is None else str(r[5])] for r in tr.records]
        run.sync()
        tr.summary()                                    # releases the events
    return launches


def record(model, inp):
    """{"fused_off", "invert_off", "fused_on", "invert_on"}: the four launch lists. Leaves the UNet's settings off."""
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler, FusedRun, InvertRun
    net = model.model.diffusion_model
    s = DDIMSampler(model)
    s.make_schedule(S, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
    common = dict(fs=inp["fs"], cfg_scale=7.5)
    fused = lambda **kw: FusedRun(s, inp["x"].clone(), inp["branches"], noises=inp["noises"], **common, **kw)
    invert = lambda: InvertRun(s, inp["x"].clone(), inp["branches"], S, **common)
    out = dict(fused_off=traced_step(fused(guidance_rescale=0.7), inp["x"]), invert_off=traced_step(invert(), inp["x"]))
    net.enable_freeu(**FREEU)
    net.enable_token_downsampling(**TODO)
    try:
        out.update(fused_on=traced_step(fused(apg=dict(APG)), inp["x"]), invert_on=traced_step(invert(), inp["x"]))
    finally:
        net.disable_freeu()
        net.disable_token_downsampling()
    return out


if __name__ == "__main__":
    from tests.test_windows_gpu import _tiny_model
    with open(sys.argv[1], "w") as f:
        json.dump(record(_tiny_model()[0], inputs()), f, indent=0)
        f.write("\n")

"""Generate tests/golden/sds_tiny.npz by running the REFERENCE's own SDS optimisation (guidance_pipeline.py:
_optimization_loop :759-808, _sds_loss :350-424) on CPU on the tiny model with recipe weights.

Run in the build container only:  python tests/golden/make_golden_sds.py
The pipeline instance is made with object.__new__ (no checkpoint download, no debug directory); its model is
make_golden.build_lvd's LatentVisualDiffusion. The draws of every step (t, noise) are recorded by wrapping
_sample_timestep and torch.randn_like during the run, the initial latent by wrapping torch.randn, and the latent and
loss.item() after every step by replacing _save_debug_step on the instance. The conditioning tensors are not stored:
they are regenerated from the seeds below (CPU torch.Generator), and their sums are stored as a check.

Cases:
  a  256 config (eps), "uniform" spacing, no rescale, Adam, CFG 7.5, B = 1, 8 steps
  b  512 config (v, zero terminal SNR), "uniform_trailing", rescale 0.7, AdamW, B = 2, 8 steps
  c  one _sds_loss call + backward per weight type "t", "ada", "uniform" (512 config, B = 2): latents.grad, loss
  tseq/<tag>  _sample_timestep called 8 times after torch.manual_seed(TSEQ_SEED) (only randint draws on the CPU)
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

T, H, W = 4, 8, 8
STEPS = 8
TSEQ_SEED = 1234
CASES = {   # tag: config, UNet extras, pipeline resolution, optimizer, batch, conditioning seed, run seed
    "a": ("inference_256_v1.0.yaml", dict(image_cross_attention_scale_learnable=True), (256, 256), "Adam", 1, 300, 7),
    "b": ("inference_512_v1.0.yaml", dict(), (320, 512), "AdamW", 2, 310, 8),
    "c": ("inference_512_v1.0.yaml", dict(), (320, 512), "Adam", 2, 320, 9),
}


def conditioning(B, seed, default_fs):
    """cond / uc of _prepare_conditioning's form: context [B, 77 + 16 T, 128], c_concat [B, 4, T, H, W]."""
    cond = {"c_crossattn": [mg.rnd(B, 77 + 16 * T, 128, seed=seed)],
            "c_concat": [mg.rnd(B, 4, T, H, W, seed=seed + 1) * 0.18215]}
    uc = {"c_crossattn": [mg.rnd(B, 77 + 16 * T, 128, seed=seed + 2)], "c_concat": cond["c_concat"]}
    return {"cond": cond, "uc": uc, "fs": torch.tensor([default_fs] * B, dtype=torch.long)}


def pipeline(tag):
    cname, extra, res, _, B, cseed, _ = CASES[tag]
    model, p = mg.build_lvd(cname, dict(mg.TINY_UNET, **extra), mg.TINY_AE)
    mg.load_recipe_weights(model.model.diffusion_model, seed=11)
    import guidance_pipeline as gp
    pipe = object.__new__(gp.DynamiCrafterGuidancePipeline)
    pipe.model, pipe.device, pipe.resolution, pipe.debug_enabled = model, "cpu", res, False
    return pipe, conditioning(B, cseed, p["unet_config"]["params"]["default_fs"])


class Recorder:
    """Records the step draws: _sample_timestep's t and torch.randn_like's noise (and torch.randn's first draw)."""

    def __init__(self, pipe):
        self.t, self.noise, self.randn = [], [], []
        self.pipe = pipe
        orig_t = pipe._sample_timestep

        def sample_t(*a, **k):
            t = orig_t(*a, **k)
            self.t.append(t.clone())
            return t
        pipe._sample_timestep = sample_t

    def __enter__(self):
        self._randn_like, self._randn = torch.randn_like, torch.randn

        def randn_like(x, *a, **k):
            n = self._randn_like(x, *a, **k)
            self.noise.append(n.clone())
            return n

        def randn(*a, **k):
            n = self._randn(*a, **k)
            self.randn.append(n.clone())
            return n
        torch.randn_like, torch.randn = randn_like, randn
        return self

    def __exit__(self, *exc):
        torch.randn_like, torch.randn = self._randn_like, self._randn


def gen_trajectory(tag, out):
    cname, _, _, opt, B, _, seed = CASES[tag]
    pipe, cond = pipeline(tag)
    steps = []
    pipe._save_debug_step = lambda step, loss, latents, conditioning=None, save_interval=100: \
        steps.append((latents.detach().clone(), loss))
    torch.manual_seed(seed)
    with Recorder(pipe) as rec:
        final = pipe._optimization_loop((B, 4, T, H, W), cond, "cpu", num_optimization_steps=STEPS, learning_rate=0.05,
                                        cfg_scale=7.5, optimizer_type=opt)
    assert len(rec.randn) == 1 and len(rec.t) == STEPS and len(rec.noise) == STEPS and len(steps) == STEPS
    out[f"{tag}/latent0"] = rec.randn[0]
    out[f"{tag}/t"] = torch.stack(rec.t)
    out[f"{tag}/noises"] = torch.stack(rec.noise)
    out[f"{tag}/latents"] = torch.stack([s[0] for s in steps])
    out[f"{tag}/losses"] = np.array([s[1] for s in steps], dtype=np.float64)
    out[f"{tag}/ctx_sums"] = np.array([cond["cond"]["c_crossattn"][0].double().sum().item(),
                                       cond["uc"]["c_crossattn"][0].double().sum().item(),
                                       cond["cond"]["c_concat"][0].double().sum().item()])
    assert torch.equal(final, steps[-1][0])


def gen_single_losses(out):
    _, _, _, _, B, _, seed = CASES["c"]
    pipe, cond = pipeline("c")
    torch.manual_seed(seed)
    latent0 = torch.randn(B, 4, T, H, W)
    out["c/latent0"] = latent0
    for wt in ("t", "ada", "uniform"):
        lat = latent0.clone().requires_grad_(True)
        with Recorder(pipe) as rec:
            loss = pipe._sds_loss(lat, cond, cfg_scale=7.5, weight_type=wt)
        loss.backward()
        out[f"c/{wt}/t"] = rec.t[0]
        out[f"c/{wt}/noise"] = rec.noise[0]
        out[f"c/{wt}/grad"] = lat.grad
        out[f"c/{wt}/loss"] = np.float64(loss.item())


def gen_t_sequences(out):
    for tag in ("a", "b"):
        pipe, _ = pipeline(tag)
        B = CASES[tag][4]
        torch.manual_seed(TSEQ_SEED)
        out[f"tseq/{tag}"] = torch.stack([pipe._sample_timestep(B) for _ in range(STEPS)])


if __name__ == "__main__":
    mg.install_stubs()
    # guidance_pipeline.py imports these at module level; nothing of them runs on the optimisation path
    funcs = types.ModuleType("scripts.evaluation.funcs")
    funcs.load_model_checkpoint = funcs.get_latent_z = None
    sys.modules["scripts.evaluation.funcs"] = funcs
    for name in ("matplotlib", "matplotlib.pyplot"):
        sys.modules.setdefault(name, types.ModuleType(name))
    torch.set_num_threads(8)
    out = {}
    for tag in ("a", "b"):
        gen_trajectory(tag, out)
    gen_single_losses(out)
    gen_t_sequences(out)
    mg.save("sds_tiny", **out)

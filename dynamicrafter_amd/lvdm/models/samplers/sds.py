"""SDSGuidance — score-distillation (SDS) optimisation of a video latent on the fused HIP UNet path.

This restates the reference's DynamiCrafterGuidancePipeline optimisation (guidance_pipeline.py: _sample_timestep
:273-302, _add_noise :304-324, _apply_guidance_rescale :326-348, _sds_loss :350-424, _optimization_loop :759-808).
Instead of sampling, the latent L is optimised directly. Per step k (n = k + 1 is Adam's step number):

    t      ~ DDIM grid of 50 steps, index uniform in [int(50 min_ratio), max(int(50 max_ratio), lo + 1))  (per clip)
    x_t    = c1 L + c2 eps_k,                       c1 = sqrt(abar_t), c2 = sqrt(1 - abar_t)
    e      = e_u + s (e_c - e_u)  [+ guidance rescale phi]      (only with an unconditional branch and s > 1)
    x0     = (x_t - c2 e) / c1    ("reference": the raw output read as eps, also for the v-models)
           | c1 x_t - c2 e        ("parameterization": the v -> x0 conversion)
    grad   = nan_to_num(w d | d / max(mean|d|, 1e-4) | d),  d = L - x0,  w = 1 - abar_t   ("t" | "ada" | "uniform")
    L      <- Adam / AdamW step (torch.optim's formulas) on g = grad / (B N), N = numel(L)
    loss_k = 0.5 mean(grad^2) / B                   (the value the reference prints)

Each step is four launch groups, with no torch math and no allocation: the noising pass (dc_sds_noise), one
batched cond + uncond UNet forward (`apply_model_rows`), the update (dc_sds_step: the guidance-rescale partials,
the "ada" reduction, the gradient + Adam pass and the loss) and the step counter. Per-step values live in device
tables indexed by the counter, so one captured hipGraph of a step is replayed S times.

Random draws follow the reference's order for a given seed: the initial latent from torch.randn on the device,
then per step the timestep indices from torch.randint on the CPU and the noise from randn on the device. They are
all drawn up front, step by step, as DDIMSampler does: the noise costs S x the latent's size of device memory
(1000 steps at 1024: 2.4 GB).
"""
import math

import numpy as np
import torch

from .... import ops
from ..utils_diffusion import make_ddim_timesteps
from .ddim import StepRun

GRID_STEPS = 50                                  # _sample_timestep draws on the 50-step DDIM grid
WEIGHT_TYPES = ops.SDS_WEIGHT_TYPES
X0_FORMULAS = ops.SDS_X0_FORMULAS
# torch.optim settings of _optimization_loop :766-771 (AdamW keeps torch's default weight decay, 1e-2)
OPTIMIZERS = {"Adam": dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
              "AdamW": dict(betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)}


def default_timestep_spacing(width):
    """The reference's rule (_sample_timestep :277-281): trailing spacing for the 512 and 1024 models."""
    return "uniform_trailing" if width in (512, 1024) else "uniform"


def default_guidance_rescale(width):
    """The reference's rule (_apply_guidance_rescale :331-333): 0.7 for the 512 and 1024 models."""
    return 0.7 if width in (512, 1024) else 0.0


def timestep_grid(num_timesteps, spacing):
    return make_ddim_timesteps(ddim_discr_method=spacing, num_ddim_timesteps=GRID_STEPS,
                               num_ddpm_timesteps=num_timesteps, verbose=False)


def step_bounds(n, min_step_ratio, max_step_ratio):
    """[lo, hi) of the grid indices _sample_timestep draws from; ValueError for an empty or out-of-grid range."""
    if not (0.0 <= min_step_ratio <= max_step_ratio <= 1.0):
        raise ValueError(f"step ratios must satisfy 0 <= min <= max <= 1, got {min_step_ratio}, {max_step_ratio}")
    lo = int(n * min_step_ratio)
    hi = max(int(n * max_step_ratio), lo + 1)
    if hi > n:
        raise ValueError(f"step ratios {min_step_ratio}, {max_step_ratio} select no index of the {n}-step grid")
    return lo, hi


def draw_timesteps(grid, lo, hi, batch_size):
    """One step's draw, as _sample_timestep: torch.randint on the CPU generator, then the grid's timesteps."""
    idx = torch.randint(lo, hi, (batch_size,), device="cpu")
    return torch.from_numpy(np.asarray(grid)[idx.numpy()]).long()


def noise_tables(alphas_cumprod, t):
    """c1, c2, w [S, B] fp32 for timesteps t [S, B], as torch computes them from the fp32 alphas_cumprod."""
    acp = alphas_cumprod.detach().float().cpu()
    a = acp[t.long().clamp(0, acp.shape[0] - 1)]
    return torch.sqrt(a), torch.sqrt(1.0 - a), 1.0 - a


def adam_tables(steps, lr, betas):
    """step_size[k] = lr / (1 - beta1^n), bc2_sqrt[k] = sqrt(1 - beta2^n), n = k + 1: torch.optim.Adam's Python-float
    values, rounded to fp32 as the update kernels see them."""
    b1, b2 = betas
    step_size = [lr / (1 - b1 ** float(n)) for n in range(1, steps + 1)]
    bc2_sqrt = [math.sqrt(1 - b2 ** float(n)) for n in range(1, steps + 1)]
    return torch.tensor(step_size, dtype=torch.float64).float(), torch.tensor(bc2_sqrt, dtype=torch.float64).float()


class SdsRun(StepRun):
    """State of one SDS run: the latent (optimised in place), the noised latent x_t the UNet reads, Adam's moments,
    the per-step loss, the device tables / counter and optionally the captured hipGraph of a step."""

    def __init__(self, model, latent, branches, tables, t_table, noises, *, fs=None, cfg_scale=7.5,
                 guidance_rescale=0.0, weight_type="t", x0_formula="reference", betas=(0.9, 0.999), eps=1e-8,
                 decay=1.0):
        super().__init__(model, latent, branches, t_table, fs=fs)
        if noises.numel() < self.S * latent.numel():
            raise ValueError(f"noises: {self.S} steps x {latent.numel()} elements needed, got {noises.numel()}")
        self.noises = noises
        self.tables = tables
        self.x_t = torch.empty_like(latent)
        self.m = torch.zeros_like(latent)
        self.v = torch.zeros_like(latent)
        self.loss = torch.zeros(self.S, dtype=torch.float32, device=latent.device)
        self.kw = dict(B=latent.shape[0], Cc=latent.shape[1], THW=int(np.prod(latent.shape[2:])),
                       weight_type=weight_type, x0_formula=x0_formula, cfg_scale=cfg_scale,
                       guidance_rescale=guidance_rescale, betas=betas, eps=eps, decay=decay)

    def _enqueue(self):
        """Kernel launches of one step (no allocation, no host sync): noising, batched UNet, SDS + Adam update."""
        kw = self.kw
        ops.sds_noise(self.tables, self.img, self.noises, self.x_t, B=kw["B"], step_index=self.counter,
                      noise_step_stride=self.img.numel())
        e = self.model.apply_model_rows(self.x_t, self.prep, self.t_table, t_index=self.counter)
        M = kw["B"] * kw["THW"]
        e_u = e[M:2 * M] if self.nb > 1 else None
        ops.sds_step(self.tables, e[:M], e_u, self.x_t, self.img, self.m, self.v, self.ws, self.loss,
                     step_index=self.counter, **kw)
        ops.advance_counter(self.counter)

    def _reset_state(self):
        self.m.zero_()
        self.v.zero_()
        self.loss.zero_()


class SDSGuidance:
    """`SDSGuidance(model).optimize(cond, uc, fs, shape, ...) -> (latents, losses)` on a LatentVisualDiffusion whose
    UNet runs on the fused HIP path."""

    def __init__(self, model):
        self.model = model
        self._last_run = None

    @torch.no_grad()
    def optimize(self, cond, uc, fs, shape, num_optimization_steps=100, learning_rate=0.05, cfg_scale=7.5,
                 guidance_rescale=None, timestep_spacing=None, min_step_ratio=0.02, max_step_ratio=0.98,
                 weight_type="t", optimizer_type="Adam", x0_formula="reference", latents=None, t_draws=None,
                 noises=None, use_graph=True, callback=None):
        """Optimise a latent of `shape` [B, C, T, h, w] for `num_optimization_steps` steps. cond / uc are the
        conditioning dicts of the reference's _prepare_conditioning (uc may be None); the unconditional branch is
        evaluated only when uc is given and cfg_scale > 1. guidance_rescale and timestep_spacing default to the
        reference's rules for the width 8 w. `latents` ([B, C, T, h, w]), `t_draws` ([S, B] timesteps) and
        `noises` ([S, B, C, T, h, w]) inject the draws. callback(i, latents, loss_i) runs after step i (a host
        sync per step). Returns the latent and the per-step losses (fp32 CPU tensor [S])."""
        if weight_type not in WEIGHT_TYPES:
            raise ValueError(f"weight_type must be one of {WEIGHT_TYPES}, got {weight_type!r}")
        if optimizer_type not in OPTIMIZERS:
            raise ValueError(f"optimizer_type must be one of {tuple(OPTIMIZERS)}, got {optimizer_type!r}")
        if x0_formula not in X0_FORMULAS:
            raise ValueError(f"x0_formula must be one of {X0_FORMULAS}, got {x0_formula!r}")
        S = int(num_optimization_steps)
        if S < 1:
            raise ValueError(f"num_optimization_steps must be >= 1, got {num_optimization_steps}")
        m = self.model
        shape = tuple(int(s) for s in shape)
        width = shape[-1] * 8
        spacing = default_timestep_spacing(width) if timestep_spacing is None else timestep_spacing
        grid = timestep_grid(m.num_timesteps, spacing)
        lo, hi = step_bounds(len(grid), min_step_ratio, max_step_ratio)
        if guidance_rescale is None:
            guidance_rescale = default_guidance_rescale(width)
        branches = [cond] + ([uc] if uc is not None and cfg_scale > 1.0 else [])
        if not hasattr(m, "apply_model_rows") or not all(isinstance(c, dict) for c in branches):
            raise NotImplementedError("SDSGuidance runs the batched HIP UNet path only: a LatentVisualDiffusion "
                                      "and conditioning dicts")
        dev = m.device
        if dev.type != "cuda":
            raise RuntimeError("SDSGuidance runs on the HIP path only: put the model on the GPU")
        B = shape[0]
        # draws in the reference's order: the initial latent, then per step t (CPU generator) and the noise (device)
        if latents is None:
            latents = torch.randn(shape, device=dev, dtype=torch.float32)
        L = latents.to(device=dev, dtype=torch.float32).contiguous().clone()
        if tuple(L.shape) != shape:
            raise ValueError(f"latents: shape {tuple(L.shape)}, expected {shape}")
        if t_draws is None or noises is None:
            ts, ns = [], []
            for _ in range(S):
                if t_draws is None:
                    ts.append(draw_timesteps(grid, lo, hi, B))
                if noises is None:
                    ns.append(torch.randn(shape, device=dev, dtype=torch.float32))
            if ts:
                t_draws = torch.stack(ts)
            if ns:
                noises = torch.stack(ns)
        t_draws = torch.as_tensor(t_draws).long().cpu().reshape(S, B)
        noises = noises.to(device=dev, dtype=torch.float32).contiguous()
        c1, c2, w = noise_tables(m.alphas_cumprod, t_draws)
        opt = OPTIMIZERS[optimizer_type]
        step_size, bc2_sqrt = adam_tables(S, learning_rate, opt["betas"])
        tables = {k: v.reshape(-1).contiguous().to(dev) for k, v in
                  (("c1", c1), ("c2", c2), ("w", w), ("step_size", step_size), ("bc2_sqrt", bc2_sqrt))}
        run = SdsRun(m, L, branches, tables, t_draws, noises, fs=fs, cfg_scale=cfg_scale,
                     guidance_rescale=guidance_rescale, weight_type=weight_type, x0_formula=x0_formula,
                     betas=opt["betas"], eps=opt["eps"], decay=1.0 - learning_rate * opt["weight_decay"])
        if use_graph:
            run.capture()
        for i in range(S):
            run.step()
            if callback:
                run.sync()                       # the graph runs on its own stream
                callback(i, run.img, run.loss[i].item())
        run.sync()
        self._last_run = run
        return run.img, run.loss.cpu()

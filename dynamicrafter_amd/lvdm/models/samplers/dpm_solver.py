"""DPMSolverSampler — multistep DPM-Solver++ (2M and 2M SDE) on the DDIM sampler's schedule and fused HIP path.

`DPMSolverSampler(model, solver="dpmpp_2m" | "dpmpp_2m_sde").sample(...)` takes the arguments of `DDIMSampler.sample`
and returns the same `(samples, intermediates)`. It runs on the DDIM timesteps of `timestep_spacing` ("uniform",
"uniform_trailing", "quad") and evaluates the model exactly as DDIM does (batched cond / uncond / image-only branches,
CFG or adaptive projected guidance (`apg=`), guidance rescale, v or eps parameterisation, dynamic rescale, mask / x0
blending, hipGraph capture).

Per executed step i, with alpha = sqrt(ddim_alphas), sigma = sqrt(1 - ddim_alphas) at t (suffix t) and at the DDIM
"prev" timestep (suffix p), lambda = log(alpha / sigma), h_i = lambda_p - lambda_t, r_i = scale_arr_prev / scale_arr
(dynamic rescale, else 1) and x0_i the raw data prediction (after CFG and guidance rescale, before dynamic rescale):

    D_i    = (1 + k_i) x0_i - k_i x0_{i-1},    k_i = h_i / (2 h_{i-1})
    x_prev = A_i (x_t - alpha_t D_i) + alpha_p r_i D_i + N_i temperature z_i

    dpmpp_2m      A = sigma_p / sigma_t             N = 0
    dpmpp_2m_sde  A = sigma_p / sigma_t e^-h        N = sigma_p sqrt(1 - e^-2h)

With k = 0, dpmpp_2m is the DDIM eta = 0 step, dynamic rescale included. k = 0 on the first step, on the last step
when S < 15 (lower order final), and wherever h_{i-1} or h_i is not a finite positive number: the zero-terminal-SNR
first step (alpha_t = 0, lambda = -inf) and the repeated timesteps "quad" produces at large S (h = 0). The
coefficients are computed on the host in float64 and kept as fp32 device tables in execution order next to DDIM's.
The update is one kernel, dc_dpmpp_step, which keeps x0 of the last step in a two-slot device ring indexed by the
step counter, so one captured step graph is replayed S times.
"""
import numpy as np
import torch

from .... import ops
from .ddim import DDIMSampler, FusedRun, _update_kw, apg_generic
from .ddim_multiplecond import DDIMSampler as DDIMSampler_multicond

SOLVERS = ("dpmpp_2m", "dpmpp_2m_sde")
LOWER_ORDER_FINAL_BELOW = 15


def dpm_coefficients(a_t, a_prev, ratio=None, solver="dpmpp_2m", lower_order_final=True):
    """Per-step float64 coefficients {A, alpha_t, alpha_p_r, k, N (None for 2M), h} from the DDIM alphas in execution
    order (a_t = alphas_cumprod at the step's timestep, a_prev at the one it steps to) and the dynamic-rescale ratio."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    a_t = np.asarray(a_t, dtype=np.float64)
    a_p = np.asarray(a_prev, dtype=np.float64)
    S = a_t.shape[0]
    r = np.ones(S) if ratio is None else np.asarray(ratio, dtype=np.float64)
    al_t, sg_t = np.sqrt(a_t), np.sqrt(1.0 - a_t)
    al_p, sg_p = np.sqrt(a_p), np.sqrt(1.0 - a_p)
    with np.errstate(divide="ignore"):
        lam_t = np.log(al_t) - np.log(sg_t)            # -inf at a zero-terminal-SNR t = 999
        lam_p = np.log(al_p) - np.log(sg_p)
    h = lam_p - lam_t
    if solver == "dpmpp_2m":
        A, N = sg_p / sg_t, None
    else:
        A = sg_p / sg_t * np.exp(-h)                   # e^-inf = 0: the first ZTSNR step keeps no x_t
        N = sg_p * np.sqrt(-np.expm1(-2.0 * h))
    ok = np.isfinite(h) & (h > 0)
    k = np.zeros(S)
    for i in range(1, S):
        if ok[i] and ok[i - 1]:                         # rho = h_{i-1}/h_i; infinite or zero h: first order (the limit)
            k[i] = h[i] / (2.0 * h[i - 1])
    if lower_order_final and S < LOWER_ORDER_FINAL_BELOW:
        k[-1] = 0.0
    return dict(A=A, alpha_t=al_t, alpha_p_r=al_p * r, k=k, N=N, h=h)


class DpmRun(FusedRun):
    """FusedRun whose step ends in dc_dpmpp_step instead of dc_ddim_step; owns the x0 history ring."""

    def __init__(self, sampler, img, branches, **kw):
        super().__init__(sampler, img, branches, **kw)
        self.x0_hist = torch.zeros((2,) + tuple(img.shape), dtype=torch.float32, device=img.device)

    def _update(self, e_c, e_u, e_i):
        ops.dpmpp_step(self.sampler._tables, e_c, e_u, e_i, self.img, self.noises, self.img, self.pred_x0, self.ws,
                       self.x0_hist, step_index=self.counter, **self.kw)

    def _reset_state(self):
        super()._reset_state()
        self.x0_hist.zero_()                            # capture()'s eager warm-up step wrote slot 0


class DPMSolverSampler(DDIMSampler):
    """DDIMSampler with the DPM-Solver++ update: `sample` and `ddim_sampling` are DDIMSampler's. `eta` is accepted for
    signature compatibility and not used: the stochastic variant is chosen by name (solver="dpmpp_2m_sde"), whose noise
    is scaled by `temperature`. `noises=` ([S, *x.shape]) injects the per-step draws of the SDE variant; the ODE variant
    draws none and ignores them."""
    _run_class = DpmRun

    def __init__(self, model, solver="dpmpp_2m", schedule="linear", **kwargs):
        if solver not in SOLVERS:
            raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
        super().__init__(model, schedule=schedule, **kwargs)
        self.solver = solver

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        """DDIM's schedule and tables (eta is not used), plus the solver's tables dpm_A, dpm_alpha_t, dpm_alpha_p_r,
        dpm_k [, dpm_N] in execution order."""
        super().make_schedule(ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=0., verbose=verbose)
        order = np.arange(self.ddim_timesteps.shape[0])[::-1].copy()
        a_t = self.ddim_alphas.double().numpy()[order]
        a_p = np.asarray(self.ddim_alphas_prev, dtype=np.float64)[order]
        ratio = None
        if getattr(self.model, "use_dynamic_rescale", False):
            ratio = (self.ddim_scale_arr_prev.double() / self.ddim_scale_arr.double()).numpy()[order]
        co = dpm_coefficients(a_t, a_p, ratio, self.solver)
        for k in ("A", "alpha_t", "alpha_p_r", "k", "N"):
            if co[k] is not None:
                if not np.isfinite(co[k]).all():
                    raise RuntimeError(f"DPM-Solver++ table {k} is not finite: {co[k]}")
                self._tables["dpm_" + k] = torch.as_tensor(co[k]).float().contiguous().to(self.model.device)
        self.dpm_coefficients = co

    def _step_noise_plan(self, noises):
        sde = "dpm_N" in self._tables                   # only the SDE variant draws (and keeps) a step noise
        return (noises if sde else None), sde and noises is None, True

    def _generic_update(self, img, branches, g, kwargs, model=None):
        """The same kernel on the NCTHW outputs of separate apply_model calls, with a ring of its own."""
        m, dev = self.model if model is None else model, img.device
        hist = torch.zeros((2,) + tuple(img.shape), dtype=torch.float32, device=dev)
        ws = ops.step_workspace(img.shape[0], dev)
        apg, state = g.get("apg"), g.get("apg_state")   # checked by the caller: two branches, no guidance rescale
        w = g["unconditional_guidance_scale"]
        kw = _update_kw(m, img, w if apg is None else 1.0, kwargs.get("cfg_img"), g["guidance_rescale"],
                        g["temperature"], e_nchw=True)
        v_param = m.parameterization == "v"

        def update(img, i, noise):
            ts = torch.full((img.shape[0],), int(self._exec_timesteps[i]), device=dev, dtype=torch.long)
            e = [m.apply_model(img, ts, c, fs=g["fs"]).to(torch.float32).contiguous() for c in branches]
            e += [None] * (3 - len(e))
            if apg is not None:                         # adaptive projected guidance, then a single branch
                e[0], e[1] = apg_generic(self._tables, apg, state, e[0], e[1], img, w, v_param=v_param, index=i), None
            return ops.dpmpp_step(self._tables, e[0], e[1], e[2], img, noise, torch.empty_like(img),
                                  torch.empty_like(img), ws, hist, index=i, **kw)
        return update

    def p_sample_ddim(self, *args, **kwargs):
        raise NotImplementedError("p_sample_ddim is DDIMSampler's single-step update; DPMSolverSampler is multistep")

    def decode(self, *args, **kwargs):
        raise NotImplementedError("decode runs DDIM steps from a latent; use DDIMSampler for it")

    def encode(self, *args, **kwargs):
        raise NotImplementedError("encode is DDIM inversion; a multistep solver needs its own: use DDIMSampler for it")

    def ddim_sampling(self, cond, shape, *args, **kwargs):
        # a multistep solver started inside the schedule needs a restart rule of its own (its x0 history is empty there)
        if kwargs.get("timesteps") is not None or (len(args) > 3 and args[3] is not None):
            raise NotImplementedError("timesteps= (a partial run) is implemented for DDIMSampler only")
        return super().ddim_sampling(cond, shape, *args, **kwargs)


def make_sampler(model, name="ddim", multiple_cond_cfg=False):
    """The sampler a harness function's `sampler=` names: "ddim" (the reference's; its ddim_multiplecond class with
    `multiple_cond_cfg`) or one of SOLVERS."""
    if name == "ddim":
        return DDIMSampler_multicond(model) if multiple_cond_cfg else DDIMSampler(model)
    if name in SOLVERS:
        return DPMSolverSampler(model, solver=name)
    raise ValueError(f"sampler must be 'ddim' or one of {SOLVERS}, got {name!r}")

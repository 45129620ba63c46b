"""DPMSolverSampler — multistep DPM-Solver++ (2M and 2M SDE) on the DDIM sampler's schedule and fused HIP path.

`DPMSolverSampler(model, solver="dpmpp_2m" | "dpmpp_2m_sde").sample(...)` takes the arguments of `DDIMSampler.sample`
and returns the same `(samples, intermediates)`. It runs on the DDIM timesteps of `timestep_spacing` ("uniform",
"uniform_trailing", "quad") and evaluates the model exactly as DDIM does (batched cond / uncond / image-only branches,
CFG, guidance rescale, v or eps parameterisation, dynamic rescale, mask / x0 blending, hipGraph capture).

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
from .ddim import DDIMSampler, FusedRun

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

    def capture(self):
        super().capture()
        self.x0_hist.zero_()                            # the eager warm-up step wrote slot 0
        torch.cuda.synchronize()
        return self

    def rewind(self, x_T=None):
        super().rewind(x_T)
        self.x0_hist.zero_()
        torch.cuda.synchronize()


class DPMSolverSampler(DDIMSampler):
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

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, schedule_verbose=False, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, precision=None, fs=None,
               timestep_spacing="uniform", guidance_rescale=0.0, **kwargs):
        """DDIMSampler.sample with the DPM-Solver++ update. `eta` is accepted for signature compatibility and not
        used: the stochastic variant is chosen by name (solver="dpmpp_2m_sde"), whose noise is scaled by
        `temperature`. `noises=` ([S, *x.shape]) injects the per-step draws of the SDE variant; the ODE variant draws
        none."""
        return super().sample(S, batch_size, shape, conditioning=conditioning, callback=callback,
                              normals_sequence=normals_sequence, img_callback=img_callback, quantize_x0=quantize_x0,
                              eta=eta, mask=mask, x0=x0, temperature=temperature, noise_dropout=noise_dropout,
                              score_corrector=score_corrector, corrector_kwargs=corrector_kwargs, verbose=verbose,
                              schedule_verbose=schedule_verbose, x_T=x_T, log_every_t=log_every_t,
                              unconditional_guidance_scale=unconditional_guidance_scale,
                              unconditional_conditioning=unconditional_conditioning, precision=precision, fs=fs,
                              timestep_spacing=timestep_spacing, guidance_rescale=guidance_rescale, **kwargs)

    def ddim_sampling(self, *args, **kwargs):
        # DDIMSampler.sample dispatches here
        return self.dpm_sampling(*args, **kwargs)

    @torch.no_grad()
    def dpm_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                     quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100, temperature=1.,
                     noise_dropout=0., score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.,
                     unconditional_conditioning=None, verbose=True, precision=None, fs=None, guidance_rescale=0.0,
                     noises=None, use_graph=False, **kwargs):
        if ddim_use_original_steps or timesteps is not None or quantize_denoised or score_corrector is not None \
                or noise_dropout > 0.:
            raise NotImplementedError("only the options DynamiCrafter inference uses are implemented "
                                      "(no original-steps / partial / quantised / corrected sampling)")
        m = self.model
        dev = m.device
        if dev.type != "cuda":
            raise RuntimeError("DPMSolverSampler runs on the HIP path only: put the model on the GPU")
        b = shape[0]
        img = (torch.randn(shape, device=dev) if x_T is None else x_T.to(dev)).to(torch.float32).contiguous().clone()
        S = self._exec_timesteps.shape[0]
        clean_cond = kwargs.pop("clean_cond", False)
        cfg_img = kwargs.get("cfg_img")
        branches = self._branches(cond, unconditional_conditioning, unconditional_guidance_scale, kwargs)
        if cfg_img is None:
            cfg_img = unconditional_guidance_scale
        sde = "dpm_N" in self._tables
        q_noises = kwargs.pop("q_noises", None)
        draw_q = mask is not None and not clean_cond and q_noises is None
        if (sde and noises is None) or draw_q:
            # drawn up front (a captured graph indexes them by the device step counter); per step the q_sample draw
            # comes first, as in DDIMSampler. Only the SDE variant draws step noise.
            qs, ns = [], []
            for _ in range(S):
                if draw_q:
                    qs.append(torch.randn(shape, device=dev))
                if sde and noises is None:
                    ns.append(torch.randn(shape, device=dev))
            if qs:
                q_noises = torch.stack(qs)
            if ns:
                noises = torch.stack(ns)
        if not sde:
            noises = None
        if noises is not None:
            noises = noises.to(device=dev, dtype=torch.float32).contiguous()
            if noises.numel() < S * img.numel():
                raise ValueError(f"noises: {S} steps x {img.numel()} elements needed, got {noises.numel()}")
        if mask is not None and not clean_cond and q_noises.numel() < S * img.numel():
            raise ValueError(f"q_noises: {S} steps x {img.numel()} elements needed, got {q_noises.numel()}")
        fast = hasattr(m, "apply_model_rows") and all(isinstance(c, dict) for c in branches)
        intermediates = {"x_inter": [img.clone()], "pred_x0": [img.clone()]}

        if fast:
            run = DpmRun(self, img, branches, fs=fs, noises=noises, cfg_scale=unconditional_guidance_scale,
                         cfg_img=cfg_img, guidance_rescale=guidance_rescale, temperature=temperature, mask=mask, x0=x0,
                         q_noises=q_noises, clean_cond=clean_cond)
            if use_graph:
                run.capture()
            for i in range(S):
                run.step()
                index = S - i - 1
                log_now = index % log_every_t == 0 or index == S - 1
                if use_graph and (callback or img_callback or log_now):
                    run.sync()
                if callback: callback(i)
                if img_callback: img_callback(run.pred_x0, i)
                if log_now:
                    intermediates["x_inter"].append(img.clone())
                    intermediates["pred_x0"].append(run.pred_x0.clone())
            run.sync()
            self._last_run = run
            return img, intermediates

        # generic path: any model exposing apply_model(x, t, c, **kw) -> [B, C, ...]; the same kernel on NCTHW outputs
        uc2 = kwargs.get("unconditional_conditioning_img_nonetext")
        hist = torch.zeros((2,) + tuple(img.shape), dtype=torch.float32, device=dev)
        ws = torch.empty(16 * b * 256, dtype=torch.float32, device=dev)
        full = lambda t: t.to(device=dev, dtype=torch.float32).expand_as(img).contiguous()
        kw = dict(B=b, Cc=img.shape[1], THW=int(np.prod(img.shape[2:])), v_param=m.parameterization == "v",
                  cfg_scale=unconditional_guidance_scale, cfg_img=cfg_img, guidance_rescale=guidance_rescale,
                  temperature=temperature, e_nchw=True)
        for i, step in enumerate(self._exec_timesteps):
            index = S - i - 1
            ts = torch.full((b,), int(step), device=dev, dtype=torch.long)
            if mask is not None:
                assert x0 is not None
                qn = None if clean_cond else q_noises[i].to(dev, torch.float32).contiguous()
                img = ops.mask_blend(img.contiguous().clone(), full(x0), full(mask), qn, self._tables, index=i,
                                     clean=clean_cond)
            e = [m.apply_model(img, ts, c, fs=fs).to(torch.float32).contiguous() for c in branches]
            e += [None] * (3 - len(e))
            x_prev, pred_x0 = torch.empty_like(img), torch.empty_like(img)
            ops.dpmpp_step(self._tables, e[0], e[1], e[2], img, None if noises is None else noises[i], x_prev, pred_x0,
                           ws, hist, index=i, **kw)
            img = x_prev
            if callback: callback(i)
            if img_callback: img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == S - 1:
                intermediates["x_inter"].append(img)
                intermediates["pred_x0"].append(pred_x0)
        return img, intermediates

    def p_sample_ddim(self, *args, **kwargs):
        raise NotImplementedError("p_sample_ddim is DDIMSampler's single-step update; DPMSolverSampler is multistep")

    def decode(self, *args, **kwargs):
        raise NotImplementedError("decode runs DDIM steps from a latent; use DDIMSampler for it")

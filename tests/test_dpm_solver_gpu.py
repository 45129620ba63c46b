"""DPM-Solver++ (2M / 2M SDE) on the GPU: dc_dpmpp_step against a float64 restatement, the convergence order on a
Gaussian toy problem with its exact denoiser, a tiny-UNet trajectory against the CPU oracle UNet, graph == eager,
rewind, and the inference harness's `sampler=` keyword.

Stated tolerances:
  dc_dpmpp_step (fp32)         max-rel <= 1e-5 (x_prev, pred_x0, the stored x0)
  convergence, S = 8..64       2M error slope < -1.7 and 2M < DDIM eta = 0 at every S (the restatement's bounds,
                               tests/test_dpm_solver_cpu.py)
  8-step 2M SDE trajectory     rel-L2 <= 8.5e-2, the DDIM 10-step trajectory bound (measured 6.4e-2 2-branch /
                               5.8e-2 3-branch; 1.5x measured would exceed it)
"""
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = (8, 16, 32, 64)
GAUSS_S = 6.0
SLOPE_BOUND = -1.7


def rel_l2(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def maxrel(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# ---- float64 restatement (DPM-Solver++, Lu et al. 2022, arXiv:2211.01095; the SDE variant in its midpoint form)
def restated_coefficients(a_t, a_p, ratio, sde):
    a_t, a_p = np.asarray(a_t, np.float64), np.asarray(a_p, np.float64)
    r = np.ones_like(a_t) if ratio is None else np.asarray(ratio, np.float64)
    al, sg, alp, sgp = np.sqrt(a_t), np.sqrt(1 - a_t), np.sqrt(a_p), np.sqrt(1 - a_p)
    e_h = (al * sgp) / (sg * alp)                                   # e^-h, h = lambda_p - lambda_t
    A = sgp / sg * (e_h if sde else 1.0)
    cD = alp * (r - e_h ** (2 if sde else 1))
    N = sgp * np.sqrt(1 - e_h ** 2) if sde else np.zeros_like(a_t)
    S = a_t.shape[0]
    k = np.zeros(S)
    for i in range(1, S):
        if 0 < e_h[i - 1] < 1 and 0 < e_h[i] < 1:
            k[i] = np.log(e_h[i]) / (2.0 * np.log(e_h[i - 1]))      # 1 / (2 rho), rho = h_{i-1} / h_i
    if S < 15:
        k[-1] = 0.0
    return dict(A=A, cD=cD, N=N, k=k, r=r)


def restated_update(co, i, x, x0, x0_prev, z=None, temperature=1.0):
    D = x0 if co["k"][i] == 0 else (1 + co["k"][i]) * x0 - co["k"][i] * x0_prev
    out = co["A"][i] * x + co["cD"][i] * D
    return out if z is None else out + co["N"][i] * temperature * z


def restated_model_output(e_c, e_u=None, e_i=None, cfg=1.0, cfg_img=1.0, gr=0.0):
    if e_u is None:
        return e_c
    mo = e_u + cfg_img * (e_i - e_u) + cfg * (e_c - e_i) if e_i is not None else e_u + cfg * (e_c - e_u)
    if gr > 0:
        dims = tuple(range(1, e_c.ndim))
        st = e_c.std(axis=dims, ddof=1, keepdims=True)
        sc = mo.std(axis=dims, ddof=1, keepdims=True)
        mo = gr * mo * (st / sc) + (1 - gr) * mo
    return mo


def exec_alphas(sampler):
    order = np.arange(sampler.ddim_timesteps.shape[0])[::-1]
    a_t = sampler.ddim_alphas.double().numpy()[order]
    a_p = np.asarray(sampler.ddim_alphas_prev, np.float64)[order]
    ratio = None
    if sampler.model.use_dynamic_rescale:
        ratio = (sampler.ddim_scale_arr_prev.double() / sampler.ddim_scale_arr.double()).numpy()[order]
    return a_t, a_p, ratio


class ScheduleModel:
    """The model's schedule buffers on the GPU (oracle.ddim.ModelSchedule); `apply_model` is the exact denoiser of
    data N(0, s^2), returned as v or eps (generic sampler path)."""

    def __init__(self, ztsnr, param, dynres=False, s=GAUSS_S):
        from oracle import ddim as oddim
        ms = oddim.ModelSchedule(rescale_betas_zero_snr=ztsnr, parameterization=param, use_dynamic_rescale=dynres)
        for k in ("num_timesteps", "parameterization", "use_dynamic_rescale"):
            setattr(self, k, getattr(ms, k))
        for k in ("alphas_cumprod", "betas", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
                  "sqrt_one_minus_alphas_cumprod"):
            setattr(self, k, getattr(ms, k).to(DEV))
        if dynres:
            self.scale_arr = ms.scale_arr.to(DEV)
        self.device = torch.device(DEV)
        self.s = s
        self._acp = ms.alphas_cumprod.double()

    def apply_model(self, x, t, c, **kw):
        a = self._acp[int(t[0])].item()
        al, sg = np.sqrt(a), np.sqrt(1 - a)
        xd = x.double()
        x0 = al * self.s ** 2 / (a * self.s ** 2 + 1 - a) * xd
        out = (al * xd - x0) / sg if self.parameterization == "v" else (xd - al * x0) / sg
        return out.float()


@pytest.mark.parametrize("sde", [False, True])
@pytest.mark.parametrize("param", ["v", "eps"])
def test_dpmpp_step_kernel_vs_restatement(sde, param):
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    S, B, Cc, T, HW, ld = 8, 2, 4, 3, 40, 8
    THW = T * HW
    g = torch.Generator().manual_seed(21)
    for dynres in (False, True):
        m = ScheduleModel(param == "v", param, dynres)
        s = DPMSolverSampler(m, solver="dpmpp_2m_sde" if sde else "dpmpp_2m")
        s.make_schedule(S, ddim_discretize="uniform_trailing", verbose=False)
        co = restated_coefficients(*exec_alphas(s), sde)
        tab = {k: v.double().cpu().numpy() for k, v in s._tables.items()}
        for nb in (1, 2, 3):
            for gr in ((0.0, 0.7) if nb > 1 else (0.0,)):
                for nchw in (False, True):
                    for i in (2, 5):             # k > 0 (step 1 of ZTSNR follows h = inf)
                        x = torch.randn(B, Cc, THW, generator=g)
                        es = [torch.randn(B, Cc, THW, generator=g) * (1 + 0.3 * j) for j in range(nb)]
                        hist = torch.randn(2, B, Cc, THW, generator=g)
                        z = torch.randn(B, Cc, THW, generator=g) if sde else None
                        if nchw:
                            e_dev = [e.to(DEV) for e in es]
                        else:                                       # channels-last rows [B*THW, ld], first Cc valid
                            e_dev = []
                            for e in es:
                                rows = torch.randn(B * THW, ld, generator=g)
                                rows[:, :Cc] = e.permute(0, 2, 1).reshape(B * THW, Cc)
                                e_dev.append(rows.to(DEV))
                        e_dev += [None] * (3 - nb)
                        xd, hd = x.to(DEV), hist.to(DEV).contiguous()
                        xp, px0 = torch.empty_like(xd), torch.empty_like(xd)
                        ws = torch.empty(16 * B * 256, device=DEV)
                        ops.dpmpp_step(s._tables, e_dev[0], e_dev[1], e_dev[2], xd, None if z is None else z.to(DEV),
                                       xp, px0, ws, hd, B=B, Cc=Cc, THW=THW, index=i, v_param=param == "v",
                                       cfg_scale=7.5, cfg_img=2.0, guidance_rescale=gr, temperature=0.8, e_nchw=nchw)
                        # restatement
                        en = [e.double().numpy() for e in es] + [None] * (3 - nb)
                        mo = restated_model_output(en[0], en[1], en[2], 7.5, 2.0, gr)
                        xn = x.double().numpy()
                        if param == "v":
                            x0 = tab["sqrt_acp_t"][i] * xn - tab["sqrt_1macp_t"][i] * mo
                        else:
                            x0 = (xn - tab["sqrt_one_minus_at"][i] * mo) / np.sqrt(tab["a_t"][i])
                        prev = hist[(i - 1) & 1].double().numpy()
                        ref = restated_update(co, i, xn, x0, prev, None if z is None else z.double().numpy(), 0.8)
                        tag = (sde, param, dynres, nb, gr, nchw, i)
                        assert co["k"][i] > 0, tag
                        assert maxrel(xp, ref) <= 1e-5, (tag, maxrel(xp, ref))
                        assert maxrel(px0, co["r"][i] * x0) <= 1e-5, tag
                        assert maxrel(hd[i & 1], x0) <= 1e-5, tag
                        assert torch.equal(hd[(i - 1) & 1].cpu(), hist[(i - 1) & 1]), tag     # the read slot is kept


def _gauss_errors(m, solver, S):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    x_T = torch.randn(1, 4, 2, 4, 4, generator=torch.Generator().manual_seed(3)).to(DEV)
    s = DDIMSampler(m) if solver == "ddim" else DPMSolverSampler(m, solver=solver)
    out, _ = s.sample(S, 1, (4, 2, 4, 4), conditioning=None, verbose=False, eta=0.0, x_T=x_T,
                      timestep_spacing="uniform_trailing")
    a_t = s.ddim_alphas[-1].item()
    a_e = float(s.ddim_alphas_prev[0])
    s2 = m.s ** 2
    exact = np.sqrt(a_e * s2 + 1 - a_e) / np.sqrt(a_t * s2 + 1 - a_t) * x_T.double()
    assert torch.isfinite(out).all()
    return rel_l2(out, exact)


@pytest.mark.parametrize("ztsnr,param", [(True, "v"), (False, "eps")])
def test_convergence_order_on_gaussian_data(ztsnr, param):
    """Data N(0, s^2) with the exact denoiser; the probability-flow solution is a scaling of x_T. DPM-Solver++ 2M's
    final error falls faster than -1.7 in log-log over S = 8..64 and is below DDIM eta = 0's at every S."""
    m = ScheduleModel(ztsnr, param)
    e2 = [_gauss_errors(m, "dpmpp_2m", S) for S in STEPS]
    e1 = [_gauss_errors(m, "ddim", S) for S in STEPS]
    slope = np.polyfit(np.log(STEPS), np.log(e2), 1)[0]
    slope1 = np.polyfit(np.log(STEPS), np.log(e1), 1)[0]
    print(f"\n[dpm convergence {param}] 2M {' '.join('%.2e' % v for v in e2)} slope {slope:.2f}; "
          f"DDIM {' '.join('%.2e' % v for v in e1)} slope {slope1:.2f}")
    assert slope < SLOPE_BOUND
    assert all(a < b for a, b in zip(e2, e1))


def _tiny_model():
    from dynamicrafter_amd.utils.utils import instantiate_from_config
    from oracle import unet as ounet
    from oracle.weights import fill_state_dict
    from tests.golden_cfg import TINY_AE, TINY_UNET
    root = os.path.join(os.path.dirname(__file__), "..", "dynamicrafter_amd", "configs")
    cfg = yaml.safe_load(open(os.path.join(root, "inference_512_v1.0.yaml")))
    p = cfg["model"]["params"]
    params = dict(TINY_UNET, default_fs=24)
    p["unet_config"]["params"] = params
    p["first_stage_config"]["params"]["ddconfig"] = dict(TINY_AE)
    for k in ("cond_stage_config", "img_cond_stage_config", "image_proj_stage_config"):
        p[k] = {"target": "torch.nn.Identity"}
    model = instantiate_from_config(cfg["model"])
    ocfg = ounet.UNetCfg.from_params(params)
    sd = fill_state_dict(ounet.unet_param_shapes(ocfg), seed=11)
    model.model.diffusion_model.load_state_dict(sd, strict=True)
    return model.to(DEV).eval(), sd, ocfg


@pytest.fixture(scope="module")
def tiny():
    return _tiny_model()


def _inputs(S, seed=9, b=1, t=4, h=16, w=16):
    g = torch.Generator().manual_seed(seed)
    return dict(x_T=torch.randn(b, 4, t, h, w, generator=g),
                ctx=[torch.randn(b, 77 + 16 * t, 128, generator=g) for _ in range(3)],
                cc=torch.randn(b, 4, t, h, w, generator=g) * 0.2,
                noises=torch.randn(S, b, 4, t, h, w, generator=g),
                q_noises=torch.randn(S, b, 4, t, h, w, generator=g),
                x0=torch.randn(b, 4, t, h, w, generator=g),
                fs=torch.tensor([24] * b))


def _sample(model, inp, S, solver="dpmpp_2m_sde", nb=2, use_graph=False, mask=None):
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    mk = lambda c: {"c_crossattn": [c.to(DEV)], "c_concat": [inp["cc"].to(DEV)]}
    kw = {}
    if nb == 3:
        kw = dict(cfg_img=2.0, unconditional_conditioning_img_nonetext=mk(inp["ctx"][2]))
    if mask is not None:
        kw.update(mask=mask.to(DEV), x0=inp["x0"].to(DEV), q_noises=inp["q_noises"].to(DEV))
    s = DPMSolverSampler(model, solver=solver)
    x_T = inp["x_T"]
    out, _ = s.sample(S, x_T.shape[0], tuple(x_T.shape[1:]), conditioning=mk(inp["ctx"][0]), verbose=False,
                      unconditional_guidance_scale=7.5, unconditional_conditioning=mk(inp["ctx"][1]),
                      x_T=x_T.to(DEV), fs=inp["fs"].to(DEV), timestep_spacing="uniform_trailing", guidance_rescale=0.7,
                      noises=inp["noises"].to(DEV), use_graph=use_graph, **kw)
    return out, s


@pytest.mark.parametrize("nb", [2, 3])
def test_tiny_unet_sde_trajectory_vs_oracle(tiny, nb):
    """8 dpmpp_2m_sde steps of the tiny UNet (v-param, ZTSNR, dynamic rescale, CFG 7.5, guidance rescale 0.7 [, cfg_img
    2.0]) through the fused path against the restatement driving the CPU oracle UNet."""
    from oracle import unet as ounet
    model, sd, ocfg = tiny
    S = 8
    inp = _inputs(S)
    out, s = _sample(model, inp, S, nb=nb)
    assert s._last_run.nb == nb
    co = restated_coefficients(*exec_alphas(s), sde=True)
    tab = {k: v.double().cpu().numpy() for k, v in s._tables.items()}
    x = inp["x_T"].double().numpy()
    prev = None
    for i, t in enumerate(s._exec_timesteps):
        ts = torch.full((1,), int(t), dtype=torch.long)
        xin = torch.cat([torch.from_numpy(x).float(), inp["cc"]], 1)
        e = [ounet.unet_forward(sd, ocfg, xin, ts, inp["ctx"][j], inp["fs"]).double().numpy() for j in range(nb)]
        e += [None] * (3 - nb)
        mo = restated_model_output(e[0], e[1], e[2], 7.5, 2.0, 0.7)
        x0 = tab["sqrt_acp_t"][i] * x - tab["sqrt_1macp_t"][i] * mo
        x = restated_update(co, i, x, x0, prev, inp["noises"][i].double().numpy())
        prev = x0
    r = rel_l2(out, torch.from_numpy(x))
    print(f"\n[dpm trajectory {nb}-branch] 8 dpmpp_2m_sde steps vs oracle rel-L2 {r:.3e}")
    assert torch.isfinite(out).all()
    assert r < 8.5e-2                                # measured 6.4e-2 / 5.8e-2 (2 / 3 branches)


def test_graph_equals_eager_bitwise_with_mask(tiny):
    model = tiny[0]
    S = 6
    inp = _inputs(S, seed=12)
    mask = torch.zeros(1, 1, 4, 16, 16)
    mask[:, :, 0] = 1.0
    eager, _ = _sample(model, inp, S, use_graph=False, mask=mask)
    graph, s = _sample(model, inp, S, use_graph=True, mask=mask)
    assert s._last_run.graph is not None
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, graph)


def test_rewind_equals_fresh_runs(tiny):
    """Two clips through one captured run with rewind() in between equal two fresh runs: the history ring and the
    step counter start over."""
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler, DpmRun
    model = tiny[0]
    S = 4
    a, b = _inputs(S, seed=31), _inputs(S, seed=32)
    b["ctx"], b["cc"], b["noises"] = a["ctx"], a["cc"], a["noises"]            # same conditioning, different x_T
    s = DPMSolverSampler(model, solver="dpmpp_2m_sde")
    s.make_schedule(S, ddim_discretize="uniform_trailing", verbose=False)
    mk = lambda c: {"c_crossattn": [c.to(DEV)], "c_concat": [a["cc"].to(DEV)]}
    br = [mk(a["ctx"][0]), mk(a["ctx"][1])]

    def fresh(x_T):
        run = DpmRun(s, x_T.to(DEV).clone(), br, fs=a["fs"].to(DEV), noises=a["noises"].to(DEV), cfg_scale=7.5,
                     guidance_rescale=0.7).capture()
        for _ in range(S):
            run.step()
        run.sync()
        return run, run.img.clone()

    run, first = fresh(a["x_T"])
    run.rewind(b["x_T"].to(DEV))
    for _ in range(S):
        run.step()
    run.sync()
    second = run.img.clone()
    _, ref_b = fresh(b["x_T"])
    _, ref_a = fresh(a["x_T"])
    with pytest.raises(RuntimeError, match="rewind"):            # step S + 1 would index past the per-step tables
        run.step()
    assert torch.equal(first, ref_a)
    assert torch.equal(second, ref_b)
    assert not torch.equal(first, second)


def test_default_draws_follow_the_solver(tiny):
    """Without injected noises: dpmpp_2m (no mask) draws nothing, so the device generator is where it was; dpmpp_2m_sde
    with a mask draws, per step, q_sample's noise and then the step's noise - the same seed gives the same sample as
    drawing them in that order by hand and injecting them."""
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    model = tiny[0]
    S = 6
    inp = _inputs(S, seed=21)
    mk = lambda c: {"c_crossattn": [c.to(DEV)], "c_concat": [inp["cc"].to(DEV)]}
    x_T = inp["x_T"].to(DEV)
    kw = dict(S=S, batch_size=1, shape=tuple(x_T.shape[1:]), conditioning=mk(inp["ctx"][0]), verbose=False,
              unconditional_guidance_scale=7.5, unconditional_conditioning=mk(inp["ctx"][1]), x_T=x_T,
              fs=inp["fs"].to(DEV), timestep_spacing="uniform_trailing", guidance_rescale=0.7)
    torch.manual_seed(777)
    out, _ = DPMSolverSampler(model, solver="dpmpp_2m").sample(**kw)
    after = torch.randn(4, device=DEV)
    torch.manual_seed(777)
    assert torch.equal(after, torch.randn(4, device=DEV))
    assert torch.isfinite(out).all()
    mask = torch.zeros(1, 1, 4, 16, 16)
    mask[:, :, 0] = 1.0
    kwm = dict(kw, mask=mask.to(DEV), x0=inp["x0"].to(DEV))
    torch.manual_seed(4321)
    a, _ = DPMSolverSampler(model, solver="dpmpp_2m_sde").sample(**kwm)
    torch.manual_seed(4321)
    qs, ns = [], []
    for _ in range(S):
        qs.append(torch.randn(x_T.shape, device=DEV)); ns.append(torch.randn(x_T.shape, device=DEV))
    b, _ = DPMSolverSampler(model, solver="dpmpp_2m_sde").sample(noises=torch.stack(ns), q_noises=torch.stack(qs), **kwm)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


def test_image_guided_synthesis_sampler_keyword():
    from dynamicrafter_amd.scripts.evaluation.inference import image_guided_synthesis
    from dynamicrafter_amd.utils.utils import instantiate_from_config
    from tests.golden_cfg import TINY_AE, TINY_RESAMPLER, TINY_UNET
    from oracle.weights import fill_state_dict
    root = os.path.join(os.path.dirname(__file__), "..", "dynamicrafter_amd", "configs")
    cfg = yaml.safe_load(open(os.path.join(root, "inference_512_v1.0.yaml")))
    p = cfg["model"]["params"]
    p["unet_config"]["params"] = dict(TINY_UNET, default_fs=24)
    p["first_stage_config"]["params"]["ddconfig"] = dict(TINY_AE)
    p["cond_stage_config"] = {"target": "tests.golden_cfg.ToyTextEmbedder"}
    p["img_cond_stage_config"] = {"target": "tests.golden_cfg.ToyImageEmbedder"}
    p["image_proj_stage_config"] = {"target": "lvdm.modules.encoders.resampler.Resampler", "params": dict(TINY_RESAMPLER)}
    model = instantiate_from_config(cfg["model"])
    for mod, seed in ((model.model.diffusion_model, 11), (model.first_stage_model, 13), (model.image_proj_model, 14)):
        sdict = mod.state_dict()
        mod.load_state_dict(fill_state_dict({k: tuple(v.shape) for k, v in sdict.items()}, seed), strict=True)
    model = model.to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    b, t, H, W, S = 1, 4, 128, 128, 5
    videos = (torch.rand(b, 3, t, H, W, generator=g) * 2 - 1).to(DEV)
    x_T = torch.randn(b, 4, t, H // 8, W // 8, generator=g).to(DEV)
    noises = torch.randn(S, b, 4, t, H // 8, W // 8, generator=g).to(DEV)
    kw = dict(n_samples=1, ddim_steps=S, ddim_eta=1.0, unconditional_guidance_scale=7.5, cfg_img=None, fs=24,
              timestep_spacing="uniform_trailing", guidance_rescale=0.7, x_T=x_T, noises=noises)
    outs = {}
    for name, extra in (("default", {}), ("ddim", dict(sampler="ddim")), ("dpmpp_2m", dict(sampler="dpmpp_2m")),
                        ("dpmpp_2m_sde", dict(sampler="dpmpp_2m_sde"))):
        torch.manual_seed(0)                              # the posterior draw of the first-stage encode
        outs[name] = image_guided_synthesis(model, ["a corgi"], videos, [b, 4, t, H // 8, W // 8], **kw, **extra)
    assert torch.equal(outs["ddim"], outs["default"])
    for name in ("dpmpp_2m", "dpmpp_2m_sde"):
        assert outs[name].shape == outs["ddim"].shape and torch.isfinite(outs[name]).all(), name
        assert not torch.equal(outs[name], outs["ddim"]), name
    with pytest.raises(ValueError):
        image_guided_synthesis(model, ["a corgi"], videos, [b, 4, t, H // 8, W // 8], **kw, sampler="euler")

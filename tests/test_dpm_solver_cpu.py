"""DPM-Solver++ (2M / 2M SDE) without a GPU: the sampler's coefficient tables against a float64 restatement of the
published formulas, the first-order reduction to DDIM eta = 0, the convergence order of the restatement on a Gaussian
toy problem (the bounds tests/test_dpm_solver_gpu.py asserts on the device), and the C ABI's argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ddim as oddim

STEPS = (8, 16, 32, 64)


# ---- float64 restatement, from DPM-Solver++ (Lu et al. 2022, arXiv:2211.01095) in its diffusers / k-diffusion form
def restated_coefficients(a_t, a_p, ratio, sde, lower_order_final=True):
    """Per step: A, alpha_t, the D coefficient of x_prev = A x + c_D D (+ N z), k and N. The ODE step is
    x_p = (sigma_p/sigma_t) x + alpha_p (1 - e^-h) D, the SDE midpoint step x_p = (sigma_p/sigma_t) e^-h x
    + alpha_p (1 - e^-2h) D + sigma_p sqrt(1 - e^-2h) z, with e^-h = (alpha_t sigma_p) / (sigma_t alpha_p); the
    dynamic-rescale ratio r multiplies the alpha_p term of the DDIM step this reduces to: c_D = alpha_p (r - e^-mh)."""
    a_t, a_p = np.asarray(a_t, np.float64), np.asarray(a_p, np.float64)
    r = np.ones_like(a_t) if ratio is None else np.asarray(ratio, np.float64)
    al, sg, alp, sgp = np.sqrt(a_t), np.sqrt(1 - a_t), np.sqrt(a_p), np.sqrt(1 - a_p)
    e_h = (al * sgp) / (sg * alp)
    m = 2 if sde else 1
    A = sgp / sg * (e_h if sde else 1.0)
    cD = alp * (r - e_h ** m)
    N = sgp * np.sqrt(1 - e_h ** 2) if sde else np.zeros_like(a_t)
    S = a_t.shape[0]
    k = np.zeros(S)
    for i in range(1, S):
        if e_h[i - 1] > 0 and e_h[i - 1] < 1 and e_h[i] > 0 and e_h[i] < 1:
            r0 = np.log(e_h[i - 1]) / np.log(e_h[i])         # h_{i-1} / h_i
            k[i] = 1.0 / (2.0 * r0)
    if lower_order_final and S < 15:
        k[-1] = 0.0
    return dict(A=A, alpha_t=al, cD=cD, k=k, N=N, alpha_p_r=alp * r)


def restated_step(co, i, x, x0, x0_prev, z=None, temperature=1.0):
    D = x0 if co["k"][i] == 0 else (1 + co["k"][i]) * x0 - co["k"][i] * x0_prev
    out = co["A"][i] * x + co["cD"][i] * D
    if z is not None:
        out = out + co["N"][i] * temperature * z
    return out


class CpuModel:
    """The schedule buffers of the model (oracle.ddim.ModelSchedule), on the CPU: enough for make_schedule."""

    def __init__(self, ztsnr, param, dynres):
        ms = oddim.ModelSchedule(rescale_betas_zero_snr=ztsnr, parameterization=param, use_dynamic_rescale=dynres)
        for k in ("num_timesteps", "alphas_cumprod", "betas", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
                  "sqrt_one_minus_alphas_cumprod", "parameterization", "use_dynamic_rescale"):
            setattr(self, k, getattr(ms, k))
        if dynres:
            self.scale_arr = ms.scale_arr
        self.device = torch.device("cpu")


def _exec_alphas(sampler):
    order = np.arange(sampler.ddim_timesteps.shape[0])[::-1]
    a_t = sampler.ddim_alphas.double().numpy()[order]
    a_p = np.asarray(sampler.ddim_alphas_prev, np.float64)[order]
    ratio = None
    if sampler.model.use_dynamic_rescale:
        ratio = (sampler.ddim_scale_arr_prev.double() / sampler.ddim_scale_arr.double()).numpy()[order]
    return a_t, a_p, ratio


CONFIGS = [(z, p, d) for z in (True, False) for p in ("v", "eps") for d in (True, False)]


@pytest.mark.parametrize("solver", ["dpmpp_2m", "dpmpp_2m_sde"])
@pytest.mark.parametrize("disc", ["uniform", "uniform_trailing", "quad"])
@pytest.mark.parametrize("S", [8, 25, 50])
def test_coefficient_tables_vs_restatement(solver, disc, S):
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    sde = solver.endswith("sde")
    for ztsnr, param, dynres in CONFIGS:
        s = DPMSolverSampler(CpuModel(ztsnr, param, dynres), solver=solver)
        s.make_schedule(S, ddim_discretize=disc, verbose=False)
        tab = {k: s._tables["dpm_" + k].double().numpy() for k in ("A", "alpha_t", "alpha_p_r", "k")}
        tab["N"] = s._tables["dpm_N"].double().numpy() if sde else np.zeros(S)
        assert ("dpm_N" in s._tables) == sde
        for k, v in tab.items():
            assert v.shape == (S,) and np.isfinite(v).all(), (k, v)
        ref = restated_coefficients(*_exec_alphas(s), sde)
        cD = tab["alpha_p_r"] - tab["A"] * tab["alpha_t"]
        for k in ("A", "alpha_t", "alpha_p_r", "k", "N"):
            np.testing.assert_allclose(tab[k], ref[k], rtol=2e-6, atol=1e-7, err_msg=f"{k} {ztsnr} {param} {dynres}")
        np.testing.assert_allclose(cD, ref["cD"], rtol=1e-5, atol=1e-6)
        assert tab["k"][0] == 0.0
        if S < 15:
            assert tab["k"][-1] == 0.0
        t0 = s._exec_timesteps[0]
        if ztsnr and t0 == 999:                          # alpha_t = 0: lambda = -inf at the first step
            assert tab["alpha_t"][0] == 0.0 and tab["k"][1] == 0.0
            if sde:                                      # A = (sigma_p/sigma_t) e^-inf = 0, N = sigma_p
                assert tab["A"][0] == 0.0
                np.testing.assert_allclose(tab["N"][0], np.sqrt(1 - _exec_alphas(s)[1][0]), rtol=1e-6)
        ts = s._exec_timesteps
        for i in range(S - 1):                            # a repeated timestep ("quad") is a step with h = 0:
            if ts[i] == ts[i + 1]:                        # first order on it and on the step after it
                assert tab["k"][i] == 0.0 and tab["k"][i + 1] == 0.0


def test_quad_repeated_timesteps_stay_finite():
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    s = DPMSolverSampler(CpuModel(False, "eps", False), solver="dpmpp_2m_sde")
    s.make_schedule(50, ddim_discretize="quad", verbose=False)
    ts = s._exec_timesteps
    rep = [i for i in range(49) if ts[i] == ts[i + 1]]       # the step from t to the same t
    assert rep, "quad at S = 50 repeats a timestep"          # t = 1, 1, 2, 4, ...
    co = s.dpm_coefficients
    for i in rep:
        assert co["h"][i] == 0.0 and co["k"][i] == 0.0 and co["A"][i] == 1.0 and co["N"][i] == 0.0
        assert co["k"][i + 1] == 0.0


@pytest.mark.parametrize("disc", ["uniform", "uniform_trailing", "quad"])
@pytest.mark.parametrize("ztsnr,param,dynres", CONFIGS)
def test_first_order_reduces_to_ddim_eta0(disc, ztsnr, param, dynres):
    """k = 0: x_prev = A (x - alpha_t x0) + alpha_p r x0 with the 2M tables is DDIM's eta = 0 step: A = sigma_p/sigma_t
    and alpha_p r - A alpha_t = alpha_p r - sigma_p alpha_t / sigma_t, from DDIMSampler.make_schedule's tables."""
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    S = 25
    m = CpuModel(ztsnr, param, dynres)
    d = DDIMSampler(m)
    d.make_schedule(S, ddim_discretize=disc, ddim_eta=0.0, verbose=False)
    p = DPMSolverSampler(m, solver="dpmpp_2m")
    p.make_schedule(S, ddim_discretize=disc, verbose=False)
    dt = {k: v.double().numpy() for k, v in d._tables.items()}
    assert (dt["sigma_t"] == 0).all()
    r = dt.get("scale_ratio", np.ones(S))
    dir_coef = np.sqrt(1 - dt["a_prev"])
    A_ddim = dir_coef / dt["sqrt_one_minus_at"]
    cD_ddim = np.sqrt(dt["a_prev"]) * r - dir_coef * np.sqrt(dt["a_t"]) / dt["sqrt_one_minus_at"]
    A = p._tables["dpm_A"].double().numpy()
    cD = p._tables["dpm_alpha_p_r"].double().numpy() - A * p._tables["dpm_alpha_t"].double().numpy()
    np.testing.assert_allclose(A, A_ddim, rtol=1e-6)
    np.testing.assert_allclose(cD, cD_ddim, rtol=1e-6, atol=1e-7)
    # one whole step on random data: the k = 0 update vs the oracle's DDIM eta = 0 step (fp32 arithmetic)
    sc = oddim.DDIMSchedule(oddim.ModelSchedule(rescale_betas_zero_snr=ztsnr, parameterization=param,
                                                use_dynamic_rescale=dynres), S, disc, 0.0)
    g = torch.Generator().manual_seed(4)
    x, e = torch.randn(2, 4, 3, 5, generator=g).double()
    for i in range(1, S):                                  # skip t = 999 of ZTSNR + eps (x0 divides by alpha_t = 0)
        j = S - 1 - i
        xp_ref, px0_ref = oddim.p_sample_ddim(sc, x.float(), j, e.float())
        tt = sc.tables
        if param == "v":
            x0 = tt["sqrt_acp_t"][j].double() * x - tt["sqrt_1macp_t"][j].double() * e
        else:
            x0 = (x - tt["sqrt_one_minus_at"][j].double() * e) / np.sqrt(dt["a_t"][i])
        xp = A[i] * x + cD[i] * x0
        scale = xp_ref.abs().max().item()
        assert (xp - xp_ref.double()).abs().max().item() <= 2e-5 * scale, (i, disc)


def _gauss_run(ms, S, s, first_order):
    """Restated 2M on data N(0, s^2) with the exact denoiser; returns |x_end - exact| / exact for x_T = 1."""
    ts = oddim.make_ddim_timesteps("uniform_trailing", S, ms.num_timesteps)
    acp = ms.alphas_cumprod.double().numpy()
    a_t = acp[ts][::-1]
    a_p = np.asarray([acp[0]] + list(acp[ts[:-1]]))[::-1]
    co = restated_coefficients(a_t, a_p, None, sde=False)
    if first_order:
        co["k"][:] = 0.0
    x, x0_prev = 1.0, None
    for i in range(S):
        al, sg = np.sqrt(a_t[i]), np.sqrt(1 - a_t[i])
        x0 = al * s * s / (al * al * s * s + sg * sg) * x
        x = restated_step(co, i, x, x0, x0_prev)
        x0_prev = x0
    exact = np.sqrt(a_p[-1] * s * s + 1 - a_p[-1]) / np.sqrt(a_t[0] * s * s + 1 - a_t[0])
    return abs(x - exact) / exact


GAUSS_S = 6.0       # data std of the toy problem; tests/test_dpm_solver_gpu.py uses the same value and bounds
SLOPE_BOUND = -1.7


@pytest.mark.parametrize("ztsnr,param", [(True, "v"), (False, "eps")])
def test_restated_convergence_order_on_gaussian_data(ztsnr, param):
    """The bounds of the GPU convergence test, confirmed on the restatement: 2M's error slope over S = 8..64 is
    steeper than -1.7 (measured -1.80 ZTSNR / -2.87 eps schedule) and 2M beats DDIM eta = 0 at every S."""
    ms = oddim.ModelSchedule(rescale_betas_zero_snr=ztsnr, parameterization=param)
    e2 = [_gauss_run(ms, S, GAUSS_S, False) for S in STEPS]
    e1 = [_gauss_run(ms, S, GAUSS_S, True) for S in STEPS]
    slope = np.polyfit(np.log(STEPS), np.log(e2), 1)[0]
    print(f"\n[dpm restatement {param}] 2M {['%.2e' % v for v in e2]} slope {slope:.2f}; DDIM {['%.2e' % v for v in e1]}")
    assert slope < SLOPE_BOUND
    assert all(a < b for a, b in zip(e2, e1))


def test_dpmpp_step_argument_errors_without_gpu():
    """Bad arguments are rejected before any launch, with DC_ERR_ARG (-2) / DC_ERR_SHAPE (-1)."""
    from dynamicrafter_amd import _hip
    lib = _hip.lib()
    f = C.c_void_p(8)                                   # never dereferenced: every call below returns before a launch

    def params(**over):
        p = _hip.DcDpmParams()
        for k in ("A", "alpha_t", "alpha_p_r", "k", "sqrt_one_minus_at", "sqrt_acp_t", "sqrt_1macp_t", "x0_hist"):
            setattr(p, k, 8)
        p.v_param = 1
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def call(p, B=1, Cc=4, THW=16, ld_e=4, e=f, x=f, noise=None, ws=f):
        return lib.dc_dpmpp_step(None if p is None else C.byref(p), e, None, None, ld_e, x, noise, f, f, B, Cc, THW, ws,
                                 None)

    assert call(None) == -2
    for k in ("A", "alpha_t", "alpha_p_r", "k", "x0_hist"):
        assert call(params(**{k: 0})) == -2, k
    assert call(params(sqrt_acp_t=0)) == -2                    # v-param needs the v tables
    assert call(params(v_param=0, sqrt_one_minus_at=0)) == -2  # eps needs sigma_t
    assert call(params(N=8)) == -2                             # SDE coefficients without a noise buffer
    assert call(params(), e=None) == -2
    assert call(params(), x=None) == -2
    assert call(params(), ws=None) == -2
    assert call(params(), B=0) == -1
    assert call(params(), Cc=0) == -1
    assert call(params(), THW=0) == -1
    assert call(params(), ld_e=3) == -1                        # channels-last rows narrower than C


def test_dpmpp_wrapper_and_sampler_reject_bad_use_without_gpu():
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    m = CpuModel(True, "v", True)
    with pytest.raises(ValueError):
        DPMSolverSampler(m, solver="dpmpp_3m")
    s = DPMSolverSampler(m, solver="dpmpp_2m_sde")
    s.make_schedule(4, ddim_discretize="uniform_trailing", verbose=False)
    x = torch.zeros(1, 4, 2, 3)
    with pytest.raises(ValueError, match="x0_hist"):                # the ring must hold two latents
        ops.dpmpp_step(s._tables, x, None, None, x, x, x, x, torch.zeros(16 * 256), torch.zeros(x.numel()),
                       B=1, Cc=4, THW=6, e_nchw=True)
    for bad in (dict(ddim_use_original_steps=True), dict(quantize_x0=True), dict(noise_dropout=0.1),
                dict(score_corrector=object())):
        with pytest.raises(NotImplementedError):
            s.sample(4, 1, (4, 2, 3), conditioning=None, verbose=False, **bad)
    with pytest.raises(NotImplementedError):
        s.decode(x, {}, 2)
    with pytest.raises(RuntimeError, match="HIP path"):            # no CPU fallback
        s.sample(4, 1, (4, 2, 3), conditioning=None, verbose=False, x_T=torch.zeros(1, 4, 2, 3))

"""SDS guidance without a GPU: the host tables (timestep grid, step ratios, spacing / rescale rules, c1 / c2 / w, Adam's
step sizes) against torch, the timestep draws against the reference's for the same seed, a float64 restatement of
SDS + Adam driving the oracle UNet against the reference's recorded trajectories (tests/golden/sds_tiny.npz), and the
C ABI's argument checks.

Stated tolerances (restatement, float64 on the oracle's fp32 UNet, vs the reference's fp32 CPU run):
  per-step latents   rel-L2 and max-rel <= 1.5x measured;  losses rel <= 1.5x measured
  case (c)           gradients max-rel <= 1e-5 (measured 2.7e-6), loss rel <= 1e-5
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sds_restatement as R


def test_timestep_grid_ratios_and_resolution_rules():
    from dynamicrafter_amd.lvdm.models.samplers import sds
    g = sds.timestep_grid(1000, "uniform")
    assert len(g) == 50 and g[0] == 1 and g[-1] == 981
    gt = sds.timestep_grid(1000, "uniform_trailing")
    assert len(gt) == 50 and gt[0] == 19 and gt[-1] == 999
    assert sds.step_bounds(50, 0.02, 0.98) == (1, 49)
    assert sds.step_bounds(50, 0.5, 0.5) == (25, 26)                 # max(hi, lo + 1), as the reference
    for bad in ((0.6, 0.4), (-0.1, 0.5), (0.2, 1.5), (1.0, 1.0)):
        with pytest.raises(ValueError):
            sds.step_bounds(50, *bad)
    for w, spacing, phi in ((256, "uniform", 0.0), (320, "uniform", 0.0), (512, "uniform_trailing", 0.7),
                            (1024, "uniform_trailing", 0.7)):
        assert sds.default_timestep_spacing(w) == spacing
        assert sds.default_guidance_rescale(w) == phi


def test_noise_tables_match_torch():
    from dynamicrafter_amd.lvdm.models.samplers import sds
    from oracle import ddim as oddim
    for ztsnr in (False, True):
        acp = oddim.ModelSchedule(rescale_betas_zero_snr=ztsnr).alphas_cumprod.float()
        t = torch.tensor([[1, 981], [501, 999], [0, 21]])
        c1, c2, w = sds.noise_tables(acp, t)
        for k in range(t.shape[0]):                                   # _add_noise / _sds_loss, per step
            a = acp[t[k]]
            assert torch.equal(c1[k], torch.sqrt(a)) and torch.equal(c2[k], torch.sqrt(1.0 - a))
            assert torch.equal(w[k], 1.0 - a)
        assert c1.dtype == c2.dtype == w.dtype == torch.float32


@pytest.mark.parametrize("opt", ["Adam", "AdamW"])
def test_adam_tables_against_torch_optim(opt):
    """A few steps of torch.optim on a synthetic gradient against the update the kernel computes from the fp32
    step_size / bc2_sqrt tables (fp32 arithmetic in torch's order)."""
    from dynamicrafter_amd.lvdm.models.samplers import sds
    cfg = sds.OPTIMIZERS[opt]
    lr, S = 0.05, 6
    step_size, bc2_sqrt = sds.adam_tables(S, lr, cfg["betas"])
    b1, b2 = cfg["betas"]
    np.testing.assert_allclose(step_size.double().numpy(), [lr / (1 - b1 ** n) for n in range(1, S + 1)], rtol=1e-7)
    np.testing.assert_allclose(bc2_sqrt.double().numpy(), [np.sqrt(1 - b2 ** n) for n in range(1, S + 1)], rtol=1e-7)
    g = torch.Generator().manual_seed(3)
    p = torch.randn(64, generator=g).requires_grad_(True)
    ref = (torch.optim.Adam if opt == "Adam" else torch.optim.AdamW)([p], lr=lr, betas=cfg["betas"], eps=cfg["eps"])
    L = p.detach().clone()
    m, v = torch.zeros_like(L), torch.zeros_like(L)
    decay = torch.tensor(1.0 - lr * cfg["weight_decay"], dtype=torch.float32)
    for k in range(S):
        grad = torch.randn(64, generator=g) * 1e-4
        ref.zero_grad()
        p.grad = grad.clone()
        ref.step()
        m = m.lerp(grad, 1 - b1)
        v = v * b2 + (1 - b2) * grad * grad
        if cfg["weight_decay"]:
            L = L * decay
        L = L - step_size[k] * (m / (v.sqrt() / bc2_sqrt[k] + cfg["eps"]))
        assert (L - p.detach()).abs().max().item() <= 2e-7 * L.abs().max().item(), (opt, k)


def test_host_timestep_draws_equal_the_reference():
    """draw_timesteps after torch.manual_seed equals the reference's _sample_timestep for the same seed."""
    from dynamicrafter_amd.lvdm.models.samplers import sds
    gd = R.golden()
    for tag in ("a", "b"):
        spacing, B = R.CASES[tag][6], R.CASES[tag][3]
        grid = sds.timestep_grid(1000, spacing)
        lo, hi = sds.step_bounds(len(grid), 0.02, 0.98)
        torch.manual_seed(1234)
        t = torch.stack([sds.draw_timesteps(grid, lo, hi, B) for _ in range(8)])
        assert torch.equal(t, torch.from_numpy(gd[f"tseq/{tag}"])), tag
        assert np.isin(gd[f"{tag}/t"], grid[lo:hi]).all(), tag        # the trajectories' draws lie on the grid


def _oracle_unet(tag):
    from oracle import unet as ounet
    from oracle.weights import fill_state_dict
    from tests.golden_cfg import TINY_UNET
    cname, extra = R.CASES[tag][:2]
    params = dict(TINY_UNET, default_fs=R.DEFAULT_FS[cname], **extra)
    ocfg = ounet.UNetCfg.from_params(params)
    sd = fill_state_dict(ounet.unet_param_shapes(ocfg), seed=11)
    fs = R.conditioning(tag)[3]
    return lambda x, t, ctx: ounet.unet_forward(sd, ocfg, x, t, ctx, fs)


def _acp(tag):
    from oracle import ddim as oddim
    return oddim.ModelSchedule(rescale_betas_zero_snr=tag != "a").alphas_cumprod.float().numpy()


def test_fixture_conditioning_regenerates():
    gd = R.golden()
    for tag in ("a", "b"):
        ctx, uctx, cc, _ = R.conditioning(tag)
        np.testing.assert_allclose([ctx.double().sum().item(), uctx.double().sum().item(), cc.double().sum().item()],
                                   gd[f"{tag}/ctx_sums"], rtol=1e-12)


# 1.5x measured. Adam divides by sqrt(v) + eps: where a gradient element is near eps in size, a 1e-7 difference of the
# fp32 UNet outputs moves that element's step by up to ~1e-3, so the max-rel bound is looser than the rel-L2 one
# (measured a: rel-L2 2.3e-5, max-rel 2.1e-4, loss 3.1e-6; b: 6.9e-7, 2.5e-6, 2.4e-7)
TRAJ_TOL = {"a": dict(rel_l2=3.5e-5, maxrel=3.1e-4, loss=4.7e-6), "b": dict(rel_l2=1.1e-6, maxrel=3.8e-6, loss=3.6e-7)}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_reproduces_reference_trajectory(tag):
    gd = R.golden()
    ctx, uctx, cc, _ = R.conditioning(tag)
    opt, phi = R.CASES[tag][2], R.CASES[tag][5]
    lats, losses = R.restated_trajectory(_oracle_unet(tag), _acp(tag), gd[f"{tag}/latent0"], gd[f"{tag}/t"],
                                         gd[f"{tag}/noises"], ctx, uctx, cc, None, opt, phi)
    l2 = max(R.rel_l2(lats[k], gd[f"{tag}/latents"][k]) for k in range(len(lats)))
    mr = max(R.maxrel(lats[k], gd[f"{tag}/latents"][k]) for k in range(len(lats)))
    lerr = (np.abs(losses - gd[f"{tag}/losses"]) / np.abs(gd[f"{tag}/losses"])).max()
    print(f"\n[sds restatement {tag}] per-step latents: rel-L2 {l2:.2e} max-rel {mr:.2e}; loss rel {lerr:.2e}")
    tol = TRAJ_TOL[tag]
    assert l2 <= tol["rel_l2"] and mr <= tol["maxrel"] and lerr <= tol["loss"]


def test_restatement_reproduces_reference_gradients():
    """Case (c): one _sds_loss + backward per weight type; latents.grad = grad / (B N) and the loss."""
    gd = R.golden()
    ctx, uctx, cc, _ = R.conditioning("c")
    unet = _oracle_unet("c")
    acp = _acp("c")
    L = gd["c/latent0"].astype(np.float64)
    for wt in ("t", "ada", "uniform"):
        t = gd[f"c/{wt}/t"].astype(np.int64)
        a = R.bcast(acp[t].astype(np.float64), L.ndim)
        x_t = np.sqrt(a) * L + np.sqrt(1.0 - a) * gd[f"c/{wt}/noise"]
        xin = torch.cat([torch.from_numpy(x_t).float(), cc], 1)
        e_c = unet(xin, torch.from_numpy(t), ctx).double().numpy()
        e_u = unet(xin, torch.from_numpy(t), uctx).double().numpy()
        grad = R.sds_grad(L, x_t, R.guidance(e_c, e_u, 7.5, 0.7), a, wt)
        B, N = L.shape[0], L.size
        err = R.maxrel(grad / (B * N), gd[f"c/{wt}/grad"])
        loss = 0.5 * np.mean(grad * grad) / B
        print(f"\n[sds gradient {wt}] max-rel {err:.2e} loss rel {abs(loss / gd[f'c/{wt}/loss'] - 1):.2e}")
        assert err <= 1e-5, wt
        assert abs(loss / gd[f"c/{wt}/loss"] - 1) <= 1e-5, wt


def test_sds_abi_argument_errors_without_gpu():
    """Bad arguments are rejected before any launch, with DC_ERR_ARG (-2) / DC_ERR_SHAPE (-1)."""
    from dynamicrafter_amd import _hip
    lib = _hip.lib()
    f = C.c_void_p(8)                                   # never dereferenced: every call below returns before a launch

    def params(**over):
        p = _hip.DcSdsParams()
        for k in ("c1", "c2", "w", "step_size", "bc2_sqrt"):
            setattr(p, k, 8)
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def step(p, B=1, Cc=4, THW=16, ld_e=4, e=f, x_t=f, lat=f, m=f, v=f, ws=f):
        return lib.dc_sds_step(None if p is None else C.byref(p), e, None, ld_e, x_t, lat, m, v, B, Cc, THW, ws, None)

    assert step(None) == -2
    for k in ("c1", "c2", "w", "step_size", "bc2_sqrt"):
        assert step(params(**{k: 0})) == -2, k
    assert step(params(weight_type=3)) == -2
    assert step(params(weight_type=-1)) == -2
    for k in ("e", "x_t", "lat", "m", "v", "ws"):
        assert step(params(), **{k: None}) == -2, k
    assert step(params(), B=0) == -1
    assert step(params(), Cc=0) == -1
    assert step(params(), THW=0) == -1
    assert step(params(), ld_e=3) == -1                       # channels-last rows narrower than C

    def noise(p, B=1, n=16, lat=f, nz=f, x_t=f):
        return lib.dc_sds_noise(None if p is None else C.byref(p), lat, nz, x_t, B, n, None)

    assert noise(None) == -2
    assert noise(params(c1=0)) == -2
    assert noise(params(c2=0)) == -2
    for k in ("lat", "nz", "x_t"):
        assert noise(params(), **{k: None}) == -2, k
    assert noise(params(), B=0) == -1
    assert noise(params(), n=0) == -1


def test_wrappers_and_optimize_reject_bad_use_without_gpu():
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.lvdm.models.samplers.sds import SDSGuidance
    x = torch.zeros(1, 4, 2, 3)
    tabs = {k: torch.zeros(2) for k in ("c1", "c2", "w", "step_size", "bc2_sqrt")}
    ws = torch.zeros(16 * 256)
    with pytest.raises(ValueError, match="weight_type"):
        ops.sds_step(tabs, x, None, x, x, x, x, ws, B=1, Cc=4, THW=6, weight_type="huber", e_nchw=True)
    with pytest.raises(ValueError, match="x0_formula"):
        ops.sds_step(tabs, x, None, x, x, x, x, ws, B=1, Cc=4, THW=6, x0_formula="eps", e_nchw=True)
    with pytest.raises(ValueError, match="c1"):                     # the per-clip tables must cover B clips
        ops.sds_step(tabs, x, None, x, x, x, x, ws, B=1, Cc=4, THW=6, index=2, e_nchw=True)
    with pytest.raises(ValueError, match="noise"):                  # S steps of noise behind a step counter
        ops.sds_noise(tabs, x, x, x.clone(), B=1, step_index=torch.zeros(1, dtype=torch.int32),
                      noise_step_stride=x.numel())

    class Model:                                                    # never reached: the checks come first
        num_timesteps = 1000
    g = SDSGuidance(Model())
    for bad in (dict(weight_type="huber"), dict(optimizer_type="SGD"), dict(x0_formula="v"),
                dict(min_step_ratio=0.7, max_step_ratio=0.3), dict(num_optimization_steps=0)):
        with pytest.raises(ValueError):
            g.optimize({}, None, None, (1, 4, 2, 8, 8), **bad)

"""SDS guidance on the GPU: dc_sds_step / dc_sds_noise against the float64 restatement (tests/sds_restatement.py), the
tiny-UNet trajectories of the reference's own run (tests/golden/sds_tiny.npz) and of the restatement driving the CPU
oracle UNet, graph == eager, rewind, and DynamiCrafterGuidancePipeline end to end.

Stated tolerances:
  dc_sds_step (fp32)            max-rel <= 1e-5 (latent, m, v, loss)
  dc_sds_noise (fp32)           max-rel <= 1e-6
  8-step trajectories (bf16 UNet) per-step latent rel-L2 and loss rel <= 1.5x measured (printed): vs the reference
                                a 1.84e-2, b 1.61e-2; vs the oracle restatement a 1.84e-2, b 1.61e-2; losses a 7.2e-3,
                                b 3.8e-3
"""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import sds_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tables(t, acp, S, lr, opt):
    from dynamicrafter_amd.lvdm.models.samplers import sds
    c1, c2, w = sds.noise_tables(acp, t)
    step_size, bc2_sqrt = sds.adam_tables(S, lr, sds.OPTIMIZERS[opt]["betas"])
    return {k: v.reshape(-1).contiguous().to(DEV) for k, v in
            (("c1", c1), ("c2", c2), ("w", w), ("step_size", step_size), ("bc2_sqrt", bc2_sqrt))}


def _rows(e, ld, g):
    """[B, C, THW] -> channels-last rows [B*THW, ld] (first C valid), the UNet's output layout."""
    B, Cc, THW = e.shape
    rows = torch.randn(B * THW, ld, generator=g)
    rows[:, :Cc] = e.permute(0, 2, 1).reshape(B * THW, Cc)
    return rows


def test_sds_step_kernel_vs_restatement():
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.lvdm.models.samplers import sds
    from oracle import ddim as oddim
    acp = oddim.ModelSchedule(rescale_betas_zero_snr=True).alphas_cumprod.float()
    S, k, Cc, THW, ld, lr = 6, 3, 4, 96, 8, 0.05
    g = torch.Generator().manual_seed(41)
    n = 0
    cases = [(wt, opt, x0f, phi, B, None) for wt in ("t", "ada", "uniform") for opt in ("Adam", "AdamW")
             for x0f in ("reference", "parameterization") for phi in (0.0, 0.7) for B in (1, 2)]
    cases += [("t", "Adam", "reference", 0.0, 2, "nan"), ("ada", "AdamW", "reference", 0.0, 2, "nan"),
              ("uniform", "Adam", "reference", 0.7, 1, "nan")]
    for wt, opt, x0f, phi, B, special in cases:
        t = torch.randint(100, 900, (S, B), generator=g)
        tabs = _tables(t, acp, S, lr, opt)
        L = torch.randn(B, Cc, THW, generator=g)
        x_t = torch.randn(B, Cc, THW, generator=g)
        m = torch.randn(B, Cc, THW, generator=g) * 1e-4
        v = torch.rand(B, Cc, THW, generator=g) * 1e-8
        e_c = torch.randn(B, Cc, THW, generator=g)
        e_u = torch.randn(B, Cc, THW, generator=g) * 0.8 + 0.2 * e_c
        if special == "nan":
            e_c[-1, 1, 5] = float("nan")
        g_rows = torch.Generator().manual_seed(n)
        Ld, md, vd = L.to(DEV), m.to(DEV), v.to(DEV)
        loss = torch.full((S,), -1.0, device=DEV)
        ws = torch.empty(16 * B * 256, device=DEV)
        cfg = sds.OPTIMIZERS[opt]
        ops.sds_step(tabs, _rows(e_c, ld, g_rows).to(DEV), _rows(e_u, ld, g_rows).to(DEV), x_t.to(DEV), Ld, md, vd,
                     ws, loss, B=B, Cc=Cc, THW=THW, index=k, weight_type=wt, x0_formula=x0f, cfg_scale=7.5,
                     guidance_rescale=phi, betas=cfg["betas"], eps=cfg["eps"], decay=1.0 - lr * cfg["weight_decay"])
        torch.cuda.synchronize()
        # restatement, step n = k + 1 > 1 from the given moments
        a = R.bcast(acp[t[k]].double().numpy(), 3)
        e = R.guidance(e_c.double().numpy(), e_u.double().numpy(), 7.5, phi)
        grad = R.sds_grad(L.double().numpy(), x_t.double().numpy(), e, a, wt, x0f)
        (b1, b2), eps, wd = R.OPT[opt]
        Bn = B * L.numel()
        gg = grad / Bn
        Lr = L.double().numpy() * (1 - lr * wd)
        mr = b1 * m.double().numpy() + (1 - b1) * gg
        vr = b2 * v.double().numpy() + (1 - b2) * gg * gg
        Lr = Lr - lr / (1 - b1 ** (k + 1)) * mr / (np.sqrt(vr) / np.sqrt(1 - b2 ** (k + 1)) + eps)
        lr_ = 0.5 * np.mean(grad * grad) / B
        tag = (wt, opt, x0f, phi, B, special)
        assert R.maxrel(Ld.cpu(), Lr) <= 1e-5, (tag, R.maxrel(Ld.cpu(), Lr))
        assert R.maxrel(md.cpu(), mr) <= 1e-5, tag
        assert R.maxrel(vd.cpu(), vr) <= 1e-5, tag
        got = loss.cpu().double().numpy()
        assert abs(got[k] - lr_) <= 1e-5 * abs(lr_) + 1e-30, (tag, got[k], lr_)
        assert (np.delete(got, k) == -1.0).all(), tag                     # only loss[k] is written
        if special == "nan":
            assert torch.isfinite(Ld).all(), tag
        n += 1
    assert n == 51


def test_sds_noise_kernel_with_step_counter():
    from dynamicrafter_amd import ops
    from oracle import ddim as oddim
    acp = oddim.ModelSchedule().alphas_cumprod.float()
    S, B = 5, 2
    g = torch.Generator().manual_seed(42)
    t = torch.randint(1, 999, (S, B), generator=g)
    tabs = _tables(t, acp, S, 0.05, "Adam")
    L = torch.randn(B, 4, 3, 40, generator=g)
    noises = torch.randn(S, B, 4, 3, 40, generator=g)
    x_t = torch.empty(L.shape, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    for k in range(S):
        ops.sds_noise(tabs, L.to(DEV), noises.to(DEV), x_t, B=B, step_index=counter, noise_step_stride=L.numel())
        ops.advance_counter(counter)
        a = acp[t[k]].view(B, 1, 1, 1)
        ref = torch.sqrt(a) * L + torch.sqrt(1.0 - a) * noises[k]          # _add_noise in fp32
        assert R.maxrel(x_t.cpu(), ref) <= 1e-6, k
    assert int(counter.item()) == S


# ---- the tiny UNet
def _tiny_model(tag, toy_conditioners=False):
    from dynamicrafter_amd.utils.utils import instantiate_from_config
    from oracle.weights import fill_state_dict
    from tests.golden_cfg import TINY_AE, TINY_RESAMPLER, TINY_UNET
    cname, extra = R.CASES[tag][:2]
    root = os.path.join(os.path.dirname(__file__), "..", "dynamicrafter_amd", "configs")
    cfg = yaml.safe_load(open(os.path.join(root, cname)))
    p = cfg["model"]["params"]
    p["unet_config"]["params"] = dict(TINY_UNET, default_fs=p["unet_config"]["params"]["default_fs"], **extra)
    p["first_stage_config"]["params"]["ddconfig"] = dict(TINY_AE)
    if toy_conditioners:
        p["cond_stage_config"] = {"target": "tests.golden_cfg.ToyTextEmbedder"}
        p["img_cond_stage_config"] = {"target": "tests.golden_cfg.ToyImageEmbedder"}
        p["image_proj_stage_config"] = {"target": "lvdm.modules.encoders.resampler.Resampler",
                                        "params": dict(TINY_RESAMPLER)}
    else:
        for k in ("cond_stage_config", "img_cond_stage_config", "image_proj_stage_config"):
            p[k] = {"target": "torch.nn.Identity"}
    model = instantiate_from_config(cfg["model"])
    mods = [(model.model.diffusion_model, 11), (model.first_stage_model, 13)]
    if toy_conditioners:
        mods.append((model.image_proj_model, 14))
    for mod, seed in mods:
        sdict = mod.state_dict()
        mod.load_state_dict(fill_state_dict({k: tuple(v.shape) for k, v in sdict.items()}, seed), strict=True)
    return model.to(DEV).eval()


def _optimize(model, tag, use_graph=False, snapshots=None, **over):
    from dynamicrafter_amd.lvdm.models.samplers.sds import SDSGuidance
    gd = R.golden()
    ctx, uctx, cc, fs = R.conditioning(tag)
    _, _, opt, B, _, phi, spacing = R.CASES[tag]
    cond = {"c_crossattn": [ctx.to(DEV)], "c_concat": [cc.to(DEV)]}
    uc = {"c_crossattn": [uctx.to(DEV)], "c_concat": [cc.to(DEV)]}
    cb = None
    if snapshots is not None:
        cb = lambda i, lat, loss: snapshots.append(lat.detach().cpu().clone())
    kw = dict(num_optimization_steps=8, learning_rate=0.05, cfg_scale=7.5, guidance_rescale=phi,
              timestep_spacing=spacing, optimizer_type=opt, latents=torch.from_numpy(gd[f"{tag}/latent0"]).to(DEV),
              t_draws=torch.from_numpy(gd[f"{tag}/t"]), noises=torch.from_numpy(gd[f"{tag}/noises"]).to(DEV),
              use_graph=use_graph, callback=cb)
    kw.update(over)
    g = SDSGuidance(model)
    lat, losses = g.optimize(cond, uc, fs.to(DEV), (B, 4, R.T, R.H, R.W), **kw)
    return lat.clone(), losses, g


# measured on MI355X (1.5x rule): per-step latent rel-L2 vs the reference's run / vs the restatement on the oracle UNet,
# and the loss rel error over the steps
# (measured a: 1.84e-2 / 1.84e-2 / 7.2e-3; b: 1.61e-2 / 1.61e-2 / 3.8e-3)
TRAJ_TOL = {"a": dict(ref=2.8e-2, oracle=2.8e-2, loss=1.1e-2), "b": dict(ref=2.4e-2, oracle=2.4e-2, loss=5.7e-3)}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_tiny_unet_trajectory_vs_reference_and_oracle(tag):
    """8 SDS + Adam(W) steps with the fixture's draws: (a) 256 config, Adam, no rescale, B = 1; (b) 512 config (v,
    ZTSNR), AdamW, rescale 0.7, B = 2; against the reference's recorded latents / losses and the float64 restatement
    driving the CPU oracle UNet."""
    from oracle import ddim as oddim
    from oracle import unet as ounet
    from oracle.weights import fill_state_dict
    from tests.golden_cfg import TINY_UNET
    gd = R.golden()
    model = _tiny_model(tag)
    snaps = []
    lat, losses, _ = _optimize(model, tag, snapshots=snaps)
    assert torch.isfinite(lat).all() and len(snaps) == 8
    cname, extra, opt, _, _, phi, _ = R.CASES[tag]
    params = dict(TINY_UNET, default_fs=R.DEFAULT_FS[cname], **extra)
    ocfg = ounet.UNetCfg.from_params(params)
    sd = fill_state_dict(ounet.unet_param_shapes(ocfg), seed=11)
    ctx, uctx, cc, fs = R.conditioning(tag)
    acp = oddim.ModelSchedule(rescale_betas_zero_snr=tag != "a").alphas_cumprod.float().numpy()
    o_lats, o_losses = R.restated_trajectory(lambda x, t, c: ounet.unet_forward(sd, ocfg, x, t, c, fs), acp,
                                             gd[f"{tag}/latent0"], gd[f"{tag}/t"], gd[f"{tag}/noises"], ctx, uctx, cc,
                                             None, opt, phi)
    e_ref = max(R.rel_l2(snaps[k], gd[f"{tag}/latents"][k]) for k in range(8))
    e_orc = max(R.rel_l2(snaps[k], o_lats[k]) for k in range(8))
    e_loss = (np.abs(losses.double().numpy() - gd[f"{tag}/losses"]) / np.abs(gd[f"{tag}/losses"])).max()
    print(f"\n[sds trajectory {tag}] per-step latent rel-L2 vs reference {e_ref:.3e}, vs oracle restatement "
          f"{e_orc:.3e}; loss rel {e_loss:.3e}")
    assert torch.equal(lat.cpu(), snaps[-1])
    tol = TRAJ_TOL[tag]
    assert e_ref <= tol["ref"] and e_orc <= tol["oracle"] and e_loss <= tol["loss"]


def test_graph_equals_eager_bitwise():
    model = _tiny_model("b")
    eager, le, _ = _optimize(model, "b", use_graph=False, weight_type="ada")
    graph, lg, g = _optimize(model, "b", use_graph=True, weight_type="ada")
    assert g._last_run.graph is not None
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, graph) and torch.equal(le, lg)


def test_rewind_equals_fresh_run():
    """Two runs through one captured SdsRun with rewind() in between equal two fresh runs: counter, moments and
    losses start over."""
    model = _tiny_model("a")
    gd = R.golden()
    first, l1, g = _optimize(model, "a", use_graph=True)
    run = g._last_run
    other = torch.from_numpy(gd["a/latent0"]).to(DEV) * 0.5 + 0.1
    run.rewind(other)
    for _ in range(run.S):
        run.step()
    run.sync()
    second, l2 = run.img.clone(), run.loss.cpu()
    with pytest.raises(RuntimeError, match="rewind"):
        run.step()
    ref2, lr2, _ = _optimize(model, "a", use_graph=True, latents=other)
    ref1, lr1, _ = _optimize(model, "a", use_graph=True)
    assert torch.equal(first, ref1) and torch.equal(l1, lr1)
    assert torch.equal(second, ref2) and torch.equal(l2, lr2)
    assert not torch.equal(first, second)


def test_pipeline_end_to_end_equals_manual_sequence():
    from dynamicrafter_amd.guidance_pipeline import DynamiCrafterGuidancePipeline
    from dynamicrafter_amd.lvdm.models.samplers.sds import SDSGuidance
    model = _tiny_model("b", toy_conditioners=True)
    image = np.random.default_rng(3).integers(0, 256, (80, 64, 3), dtype=np.uint8)   # resize + centre crop
    pipe = DynamiCrafterGuidancePipeline(model, resolution="64_64")
    kw = dict(prompt="a corgi", negative_prompt="blurry", frame_stride=24)
    torch.manual_seed(21)
    videos = pipe(image, num_optimization_steps=3, **kw)["videos"]
    assert videos.shape == (1, 3, 4, 64, 64) and torch.isfinite(videos).all()
    torch.manual_seed(21)
    cond, shape = pipe.prepare(image, kw["prompt"], kw["negative_prompt"], 7.5, kw["frame_stride"])
    assert cond["uc"] is not None and shape == (1, 4, 4, 8, 8)
    lat, losses = SDSGuidance(model).optimize(cond["cond"], cond["uc"], cond["fs"], shape, num_optimization_steps=3)
    manual = model.decode_first_stage(lat)
    assert torch.equal(videos, manual)
    assert losses.shape == (3,) and torch.isfinite(losses).all()
    torch.manual_seed(21)
    again = pipe(image, num_optimization_steps=3, return_dict=False, loss_type="csd", weight_type="ada", **kw)
    assert torch.equal(again, videos)                 # loss_type / weight_type change nothing, as in the reference

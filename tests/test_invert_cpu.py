"""DDIM inversion and partial denoising without a GPU: the float64 restatement's round trip on the Gaussian toy problem,
the run lengths of `timesteps=k`, the strength -> steps mapping, argument checking, the C ABI and the command line.

Stated bounds:
  round trip (invert n steps, then n DDIM eta = 0 steps) on the exact denoiser of N(0, s^2): the relative L2 error falls
  monotonically over S = 8, 16, 32, 64 with a log-log slope < -0.7 (first order: the inverse step takes eps at the source
  level, the forward step at the destination). Measured: slopes -0.98 .. -0.80, worst error at S = 64 5.9e-2."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import ddim as oddim
from tests import invert_restatement as R

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

SCHEDULES = {
    "eps-uniform": (dict(parameterization="eps"), "uniform"),
    "v-ztsnr-rescale-trailing": (dict(rescale_betas_zero_snr=True, parameterization="v", use_dynamic_rescale=True,
                                      base_scale=0.7), "uniform_trailing"),
}


def _round_trip(ms, spacing, S, n, s, x0):
    sc = oddim.DDIMSchedule(ms, S, spacing, 0.0)
    am = R.gaussian_denoiser(ms, s)
    x = R.invert_loop(am, sc, x0, None, n=n)
    back = oddim.ddim_sample(am, sc, x, None, t_start=n)
    return R.rel_l2(back, x0)


@pytest.mark.parametrize("half", [True, False], ids=["n=S/2", "n=S"])
@pytest.mark.parametrize("s", [1.0, 6.0])
@pytest.mark.parametrize("name", list(SCHEDULES))
def test_round_trip_converges_first_order(name, s, half):
    kw, spacing = SCHEDULES[name]
    ms = oddim.ModelSchedule(**kw)
    x0 = torch.randn(2, 4, 2, 8, 8, generator=torch.Generator().manual_seed(31), dtype=torch.float64) * s
    Ss = [8, 16, 32, 64]
    errs = [_round_trip(ms, spacing, S, S // 2 if half else S, s, x0) for S in Ss]
    slope = float(np.polyfit(np.log(Ss), np.log(errs), 1)[0])
    print(f"\n[round trip {name} s={s} {'n=S/2' if half else 'n=S'}] rel-L2 " + " ".join(f"{e:.3e}" for e in errs)
          + f" slope {slope:.3f}")
    assert all(np.isfinite(errs))
    assert all(b < a for a, b in zip(errs, errs[1:])), errs
    assert slope < -0.7, slope


def test_inverse_step_is_the_algebraic_inverse_of_the_ddim_step_in_float64():
    """For equal eps (eps-parameterisation: the model output itself) the forward eta = 0 step undoes the inverse step, the
    dynamic rescale included; the forward tables are fp32 values, so the residue is their rounding (a few 1e-8)."""
    ms = oddim.ModelSchedule(parameterization="eps", use_dynamic_rescale=True, base_scale=0.7)
    S = 6
    sc = oddim.DDIMSchedule(ms, S, "uniform", 0.0)
    g = torch.Generator().manual_seed(2)
    for k in range(S):
        x = torch.randn(1, 4, 2, 4, 4, generator=g, dtype=torch.float64)
        e = torch.randn(1, 4, 2, 4, 4, generator=g, dtype=torch.float64)
        up, _ = R.invert_step(sc, x, k, e)
        down, _ = oddim.p_sample_ddim(sc, up, k, e)
        assert R.max_rel(down, x) < 1e-6, (k, R.max_rel(down, x))


class _CpuModel:
    """The schedule buffers of a model on the CPU: enough for make_schedule and the argument checks."""

    def __init__(self, **kw):
        ms = oddim.ModelSchedule(**kw)
        for k in ("num_timesteps", "parameterization", "use_dynamic_rescale", "alphas_cumprod", "betas",
                  "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"):
            setattr(self, k, getattr(ms, k))
        if ms.use_dynamic_rescale:
            self.scale_arr = ms.scale_arr
        self.device = torch.device("cpu")


def _sampler(S, cls=None, spacing="uniform", **kw):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    s = (cls or DDIMSampler)(_CpuModel(**kw))
    s.make_schedule(S, ddim_discretize=spacing, ddim_eta=0.0, verbose=False)
    return s


@pytest.mark.parametrize("S", [6, 49, 50])
def test_timesteps_run_lengths_follow_the_literal_expression(S):
    s = _sampler(S, spacing="uniform_trailing")      # "uniform" gives 1000 // S-spaced steps: 7 for S = 6, 50 for S = 49
    assert s.ddim_timesteps.shape[0] == S
    for k in (0, 1, 2, S - 1, S, S + 3):
        subset_end = int(min(k / S, 1) * S) - 1                  # reference ddim.py:155
        want = np.arange(S)[:subset_end].shape[0]                # :156
        assert s.subset_steps(k) == want, (S, k)
    assert s.subset_steps(0) == S - 1                            # subset_end = -1: all but the last index
    assert s.subset_steps(S) == S - 1 and s.subset_steps(S + 3) == S - 1     # the off-by-one
    if S == 49:
        assert int(1 / 49 * 49) == 0 and s.subset_steps(1) == 48             # float rounding: subset_end = -1
        assert int(2 / 49 * 49) == 1 and s.subset_steps(2) == 0              # and here one short: an empty selection
    else:
        assert s.subset_steps(1) == 0 and s.subset_steps(2) == 1             # k = 1: an empty selection


def test_inversion_tables_and_existing_tables():
    """New keys in ascending k next to the forward tables, which stay what they were (execution order, same values)."""
    S = 10
    s = _sampler(S, spacing="uniform_trailing", rescale_betas_zero_snr=True, parameterization="v", use_dynamic_rescale=True)
    sc = oddim.DDIMSchedule(oddim.ModelSchedule(rescale_betas_zero_snr=True, parameterization="v", use_dynamic_rescale=True),
                            S, "uniform_trailing", 0.0)
    for nm in ("a_t", "a_prev", "sigma_t", "sqrt_one_minus_at", "sqrt_acp_t", "sqrt_1macp_t"):
        assert np.array_equal(s._tables[nm].numpy()[::-1], sc.tables[nm].numpy()), nm
    t = R.inverse_tables(sc)
    assert np.array_equal(s._inv_timesteps, R.source_timesteps(sc))
    for ours, theirs in (("inv_sqrt_a_src", "sa_src"), ("inv_sqrt_1ma_src", "s1_src"), ("inv_sqrt_a_dst", "sa_dst"),
                         ("inv_sqrt_1ma_dst", "s1_dst"), ("inv_scale_ratio", "r")):
        assert s._tables[ours].dtype == torch.float32 and s._tables[ours].shape == (S,)
        assert np.array_equal(s._tables[ours].numpy(), t[theirs].float().numpy()), ours
    # a_prev[k] = alphas_cumprod[t_src[k]] exactly, and > 0; the last destination level is 0 with zero-terminal SNR
    assert np.array_equal(s.model.alphas_cumprod.numpy()[s._inv_timesteps], s._tables["a_prev"].numpy()[::-1])
    assert float(s._tables["inv_sqrt_a_src"].min()) > 0 and float(s._tables["inv_sqrt_a_dst"][-1]) == 0.0


def test_strength_to_steps():
    from dynamicrafter_amd.scripts.evaluation.edit import strength_steps
    assert strength_steps(0.6, 50) == 30
    assert strength_steps(0.5, 50) == 25
    assert strength_steps(0.0, 50) == 1 and strength_steps(0.001, 50) == 1       # lower clamp
    assert strength_steps(1.0, 50) == 50 and strength_steps(1.7, 50) == 50       # upper clamp
    assert strength_steps(1.0, 6) == 6 and strength_steps(0.6, 6) == 4
    assert strength_steps(0.25, 6) == round(1.5) == 2                            # Python's round: halves go to even
    with pytest.raises(ValueError):
        strength_steps(0.5, 0)


def test_ops_ddim_invert_step_checks_its_arguments():
    from dynamicrafter_amd import ops
    B, C, THW, S = 1, 4, 10, 3
    tables = {k: torch.ones(S) for k in ("inv_sqrt_a_src", "inv_sqrt_1ma_src", "inv_sqrt_a_dst", "inv_sqrt_1ma_dst")}
    x = torch.zeros(B, C, THW)
    e = torch.zeros(B * THW, 16)
    ws = torch.zeros(ops.STEP_WS_FLOATS * B)
    ok = dict(B=B, Cc=C, THW=THW)
    call = lambda tb=tables, e_c=e, e_u=None, e_i=None, xx=x, xn=x, p=x, w=ws, **kw: \
        ops.ddim_invert_step(tb, e_c, e_u, e_i, xx, xn, p, w, **dict(ok, **kw))
    with pytest.raises(ValueError, match="x_next"):
        call(xn=torch.zeros(B * C * THW - 1))
    with pytest.raises(ValueError, match="workspace"):
        call(w=ws[:-1])
    with pytest.raises(ValueError, match="e_cond"):
        call(e_c=e[:-1])
    with pytest.raises(ValueError, match="e_uncond"):
        call(e_u=torch.zeros(B * C * THW - 1), e_nchw=True, e_c=torch.zeros(B * C * THW))
    with pytest.raises(ValueError, match="e_img needs e_uncond"):
        call(e_i=e)
    with pytest.raises(ValueError, match="ld_e"):
        call(ld_e=3)
    with pytest.raises(ValueError, match="outside"):
        call(index=S)
    with pytest.raises(ValueError, match="outside"):
        call(index=-1)
    with pytest.raises(ValueError, match="missing"):
        call(tb={k: v for k, v in tables.items() if k != "inv_sqrt_a_dst"})
    with pytest.raises(ValueError, match="entries"):
        call(tb=dict(tables, inv_scale_ratio=torch.ones(S + 1)))
    with pytest.raises(ValueError, match="fp32"):
        call(tb=dict(tables, inv_sqrt_a_src=torch.ones(S, dtype=torch.float64)))


def test_cabi_declares_exports_and_refuses_bad_arguments():
    import ctypes as C
    from dynamicrafter_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "dcrafter_hip.h")).read()
    assert re.search(r"\bint dc_ddim_invert_step\s*\(const DcInvertParams\*", hdr)
    assert "typedef struct DcInvertParams" in hdr and "ddim.py:179" in hdr
    assert "dc_ddim_invert_step" in _hip.SIGNATURES
    nm = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T dc_ddim_invert_step\b", nm)
    lib = _hip.lib()
    p = _hip.DcInvertParams()
    q = C.c_void_p(8)
    assert lib.dc_ddim_invert_step(None, q, None, None, 4, q, q, q, 1, 4, 16, q, None) == -2
    assert lib.dc_ddim_invert_step(C.byref(p), q, None, None, 4, q, q, q, 1, 4, 16, q, None) == -2     # no tables
    p.sqrt_a_src = p.sqrt_1ma_src = p.sqrt_a_dst = p.sqrt_1ma_dst = 8
    assert lib.dc_ddim_invert_step(C.byref(p), q, None, None, 4, q, None, q, 1, 4, 16, q, None) == -2   # no x_next
    assert lib.dc_ddim_invert_step(C.byref(p), q, None, q, 4, q, q, q, 1, 4, 16, q, None) == -2         # e_img without e_uncond
    assert lib.dc_ddim_invert_step(C.byref(p), q, None, None, 4, q, q, q, 0, 4, 16, q, None) == -1      # B < 1
    assert lib.dc_ddim_invert_step(C.byref(p), q, None, None, 3, q, q, q, 1, 4, 16, q, None) == -1      # ld_e < C
    p.index = -1
    assert lib.dc_ddim_invert_step(C.byref(p), q, None, None, 4, q, q, q, 1, 4, 16, q, None) == -2


def test_encode_and_partial_runs_refuse_what_the_issue_says():
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    S = 6
    s = _sampler(S, spacing="uniform_trailing")
    x = torch.zeros(1, 4, 2, 4, 4)
    with pytest.raises(NotImplementedError):
        s.encode(x, None, 3, use_original_steps=True)
    with pytest.raises(ValueError, match="window"):
        s.encode(x, None, 3, window_stride=2)
    for bad in (0, S + 1, -1, 2.5):
        with pytest.raises(ValueError, match="t_enc"):
            s.encode(x, None, bad)
    with pytest.raises(RuntimeError, match="HIP path"):       # the arguments are fine: only the device is missing
        s.encode(x, None, S)
    for kw in (dict(ddim_use_original_steps=True), dict(quantize_denoised=True), dict(score_corrector=object()),
               dict(noise_dropout=0.1)):
        with pytest.raises(NotImplementedError):
            s.ddim_sampling(None, tuple(x.shape), timesteps=3, **kw)
    with pytest.raises(RuntimeError, match="HIP path"):       # timesteps= itself is accepted now
        s.ddim_sampling(None, tuple(x.shape), timesteps=3)
    d = _sampler(S, cls=DPMSolverSampler, spacing="uniform_trailing")
    with pytest.raises(NotImplementedError):
        d.encode(x, None, 3)
    with pytest.raises(NotImplementedError):
        d.decode(x, None, 3)
    with pytest.raises(NotImplementedError):
        d.ddim_sampling(None, tuple(x.shape), timesteps=3)
    with pytest.raises(NotImplementedError):
        d.sample(S, 1, tuple(x.shape[1:]), verbose=False, timesteps=3)


@pytest.mark.parametrize("kw", [dict(loop=True), dict(interp=True), dict(num_frames=8), dict(window_stride=2),
                                dict(sampler="dpmpp_2m")])
def test_video_guided_synthesis_refusals(kw):
    from dynamicrafter_amd.scripts.evaluation import funcs
    from dynamicrafter_amd.scripts.evaluation.edit import video_guided_synthesis
    assert funcs.video_guided_synthesis is video_guided_synthesis
    v = torch.zeros(1, 3, 4, 16, 16)
    with pytest.raises(ValueError, match=next(iter(kw))):
        video_guided_synthesis(None, [""], v, v, [1, 4, 4, 2, 2], **kw)


def test_edit_parser_extends_the_generate_line_and_leaves_it_alone():
    from dynamicrafter_amd.scripts.evaluation import edit, inference
    before = vars(inference.get_parser().parse_args([]))
    line = ["--config", "c.yaml", "--ckpt_path", "m.ckpt", "--prompt_dir", "p", "--savedir", "o", "--height", "320", "--width",
            "512", "--ddim_steps", "7", "--video_length", "16", "--frame_stride", "24", "--text_input",
            "--unconditional_guidance_scale", "7.5", "--seed", "5", "--timestep_spacing", "uniform_trailing",
            "--guidance_rescale", "0.7", "--perframe_ae", "--multiple_cond_cfg", "--cfg_img", "2.0", "--container", "avi",
            "--quality", "80", "--n_samples", "2", "--ddim_eta", "0.5"]
    gen = vars(inference.get_parser().parse_args(line))
    ed = vars(edit.get_parser().parse_args(line + ["--source_dir", "s", "--strength", "0.4", "--no_invert",
                                                   "--source_prompt_file", "sp.txt"]))
    own = dict(source_dir="s", strength=0.4, no_invert=True, source_prompt_file="sp.txt")
    assert {k: ed[k] for k in own} == own
    assert {k: v for k, v in ed.items() if k not in own} == gen
    d = vars(edit.get_parser().parse_args([]))
    assert (d["source_dir"], d["strength"], d["no_invert"], d["source_prompt_file"]) == (None, 0.6, False, None)
    assert d["ddim_eta"] == 0.0                              # the edit line's one changed default
    assert {k: v for k, v in d.items() if k not in own and k != "ddim_eta"} == \
        {k: v for k, v in before.items() if k != "ddim_eta"}
    assert vars(inference.get_parser().parse_args([])) == before and before["ddim_eta"] == 1.0
    with pytest.raises(SystemExit):
        inference.get_parser().parse_args(["--strength", "0.5"])

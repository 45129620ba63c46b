"""Adaptive projected guidance without a GPU: the restatement's own invariants, validation of the `apg=` dict, the combinations
the samplers refuse (before any GPU work: the stub model lives on the CPU, and a call that got past the checks would stop at
"runs on the HIP path only"), the command-line flags and the C ABI."""
import ctypes as C
import math
import os
import re
import subprocess
import types

import pytest
import torch

from oracle import ddim as oddim
from tests import apg_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APG = dict(eta=0.0, norm_threshold=2.5, momentum=-0.5)
SHAPE = [1, 4, 4, 8, 8]


def _data(seed, B=3, shape=(4, 3, 5, 7)):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((B,) + shape, generator=g, dtype=torch.float64) for _ in range(3)]


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("space,v_param", [("model", True), ("x0", True), ("x0", False)])
def test_eta_one_without_threshold_and_momentum_is_plain_cfg(space, v_param):
    e_c, e_u, x = _data(1)
    got, m = R.apg(e_c, e_u, x, None, w=7.5, eta=1.0, space=space, v_param=v_param, sqrt_a=0.6, sqrt_1ma=0.8)
    ref = R.cfg(e_c, e_u, 7.5)                          # both spaces are affine in the output: CFG commutes with the map
    assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    m_prev = torch.randn(m.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    again, _ = R.apg(e_c, e_u, x, m_prev, w=7.5, eta=1.0, momentum=0.0, norm_threshold=0.0, space=space, v_param=v_param,
                     sqrt_a=0.6, sqrt_1ma=0.8)
    assert torch.equal(again, got)                      # momentum 0 ignores m_prev; a threshold <= 0 is no threshold


@pytest.mark.parametrize("space,v_param", [("model", True), ("x0", True), ("x0", False)])
def test_equal_predictions_give_the_conditional_one(space, v_param):
    e_c, _, x = _data(3)
    got, m = R.apg(e_c, e_c.clone(), x, None, w=7.5, space=space, v_param=v_param, sqrt_a=0.6, sqrt_1ma=0.8, **APG)
    assert (got - e_c).abs().max().item() <= 1e-13 and not m.any()
    zero, _ = R.apg(torch.zeros_like(e_c), e_c, x * 0, None, w=7.5, space="model", eta=0.3)
    assert torch.isfinite(zero).all()                   # p_c = 0: par = 0, no division


def test_projection_clip_and_momentum():
    p_c, p_u, _ = _data(4)
    g0, m0 = R.guide(p_c, p_u, None, w=5.0, eta=0.0)
    upd = (g0 - p_c).flatten(1)
    assert ((upd * p_c.flatten(1)).sum(1).abs() <= 1e-10 * upd.norm(dim=1) * p_c.flatten(1).norm(dim=1)).all()   # eta = 0: orthogonal
    norm = (p_c - p_u).flatten(1).norm(dim=1)
    thr = 0.5 * norm.min().item()
    g1, _ = R.guide(p_c, p_u, None, w=5.0, eta=1.0, norm_threshold=thr)
    assert torch.allclose((g1 - p_c).flatten(1).norm(dim=1), torch.full((3,), 4.0 * thr, dtype=torch.float64), rtol=1e-12)
    _, m1 = R.guide(p_c, p_u, m0, w=5.0, momentum=-0.5, norm_threshold=thr)
    assert torch.equal(m1, (p_c - p_u) - 0.5 * m0)      # the running update is kept unscaled


# ------------------------------------------------------------------ the apg= dict
def test_apg_config_validates():
    from dynamicrafter_amd.lvdm.models.samplers.ddim import APG_DEFAULTS, apg_config
    assert apg_config(None) is None
    assert apg_config({}) == APG_DEFAULTS == dict(eta=0.0, norm_threshold=None, momentum=0.0, space="x0")
    assert apg_config(dict(eta=1, norm_threshold=15, momentum=-0.5, space="model")) == \
        dict(eta=1.0, norm_threshold=15.0, momentum=-0.5, space="model")
    with pytest.raises(ValueError, match="unknown keys"):
        apg_config(dict(eta=0.0, threshold=1.0))
    with pytest.raises(ValueError, match="dict"):
        apg_config((0.0, 15.0, -0.5))
    for k in ("eta", "momentum", "norm_threshold"):
        for bad in (float("nan"), float("inf"), "0.5", True, 1j) + ((None,) if k != "norm_threshold" else ()):
            with pytest.raises(ValueError, match="finite"):
                apg_config({k: bad})
    for bad in ("eps", "X0", None, 0):
        with pytest.raises(ValueError, match="space"):
            apg_config(dict(space=bad))


class _CpuModel:
    """The schedule buffers of a model, on the CPU: the samplers take it up to the point where they need the GPU."""

    def __init__(self, parameterization="v", zero_snr=True):
        ms = oddim.ModelSchedule(parameterization=parameterization, rescale_betas_zero_snr=zero_snr)
        for k in ("num_timesteps", "parameterization", "use_dynamic_rescale", "alphas_cumprod", "betas",
                  "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"):
            setattr(self, k, getattr(ms, k))
        self.device = torch.device("cpu")
        self.model = types.SimpleNamespace(diffusion_model=types.SimpleNamespace())
        self.temporal_length = 4


def _cond():
    return {"c_crossattn": [torch.zeros(1, 141, 128)], "c_concat": [torch.zeros(SHAPE)]}


def _sample(sampler, **kw):
    args = dict(S=4, batch_size=1, shape=SHAPE[1:], conditioning=_cond(), verbose=False, unconditional_guidance_scale=7.5,
                unconditional_conditioning=_cond(), timestep_spacing="uniform_trailing", apg=APG)
    args.update(kw)
    return sampler.sample(**args)


def test_samplers_refuse_before_any_gpu_work():
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    for cls in (DDIMSampler, DPMSolverSampler):
        s = cls(_CpuModel())
        with pytest.raises(RuntimeError, match="HIP path"):           # a good call gets as far as the device check
            _sample(s)
        with pytest.raises(ValueError, match="two guidance branches"):
            _sample(s, unconditional_conditioning_img_nonetext=_cond(), cfg_img=2.0)
        with pytest.raises(ValueError, match="two guidance branches"):
            _sample(s, cfg_img=2.0)
        with pytest.raises(ValueError, match="guidance_rescale"):
            _sample(s, guidance_rescale=0.7)
        with pytest.raises(ValueError, match="needs classifier-free guidance"):
            _sample(s, unconditional_conditioning=None)
        with pytest.raises(ValueError, match="needs classifier-free guidance"):
            _sample(s, unconditional_guidance_scale=1.0)
        with pytest.raises(ValueError, match="unknown keys"):
            _sample(s, apg=dict(APG, beta=1.0))
        with pytest.raises(ValueError, match="finite"):
            _sample(s, apg=dict(APG, eta=float("nan")))
        with pytest.raises(RuntimeError, match="HIP path"):           # without apg none of this is looked at
            _sample(s, apg=None, guidance_rescale=0.7, cfg_img=2.0)


def test_eps_model_in_x0_space_needs_a_positive_alpha():
    """x0 = (x - sqrt(1-a) eps) / sqrt(a) does not exist at a = 0: refused when the run is built, nothing divides."""
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    s = DDIMSampler(_CpuModel("eps", zero_snr=True))
    with pytest.raises(ValueError, match="a_t > 0"):
        _sample(s)                                                    # uniform_trailing reaches t = 999, a_t = 0
    with pytest.raises(RuntimeError, match="HIP path"):
        _sample(s, apg=dict(APG, space="model"))
    with pytest.raises(RuntimeError, match="HIP path"):
        _sample(s, timestep_spacing="uniform")                        # the last timestep is 751: a_t > 0
    with pytest.raises(RuntimeError, match="HIP path"):
        _sample(DDIMSampler(_CpuModel("eps", zero_snr=False)))
    with pytest.raises(RuntimeError, match="HIP path"):
        _sample(DDIMSampler(_CpuModel("v", zero_snr=True)))           # v: x0 = sqrt(a) x - sqrt(1-a) v exists everywhere
    # a partial run that stops short of the a_t = 0 step is fine
    s.make_schedule(4, ddim_discretize="uniform_trailing", verbose=False)
    x = torch.zeros(SHAPE)
    kw = dict(unconditional_guidance_scale=7.5, unconditional_conditioning=_cond(), apg=APG)
    with pytest.raises(RuntimeError, match="HIP path"):
        s.decode(x, _cond(), 3, **kw)
    with pytest.raises(ValueError, match="a_t > 0"):
        s.decode(x, _cond(), 4, **kw)


def test_decode_refuses_and_encode_has_no_apg():
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    s = DDIMSampler(_CpuModel())
    s.make_schedule(4, ddim_discretize="uniform_trailing", verbose=False)
    x = torch.zeros(SHAPE)
    kw = dict(unconditional_guidance_scale=7.5, unconditional_conditioning=_cond(), apg=APG)
    with pytest.raises(RuntimeError, match="HIP path"):
        s.decode(x, _cond(), 2, **kw)
    with pytest.raises(ValueError, match="guidance_rescale"):
        s.decode(x, _cond(), 2, guidance_rescale=0.7, **kw)
    with pytest.raises(ValueError, match="two guidance branches"):
        s.decode(x, _cond(), 2, unconditional_conditioning_img_nonetext=_cond(), cfg_img=2.0, **kw)
    with pytest.raises(ValueError, match="needs classifier-free guidance"):
        s.decode(x, _cond(), 2, apg=APG)
    with pytest.raises(ValueError, match="encode: apg="):
        s.encode(x, _cond(), 2, **kw)
    with pytest.raises(ValueError, match="encode: apg="):
        s.encode(x, _cond(), 2, apg=None)
    with pytest.raises(RuntimeError, match="HIP path"):
        s.encode(x, _cond(), 2)


def test_harness_functions_take_apg(monkeypatch):
    from dynamicrafter_amd.scripts.evaluation import edit, funcs, inference
    from dynamicrafter_amd.scripts.gradio.dynamicrafter_pipeline import DynamiCrafterImg2VideoPipeline
    import inspect
    model = _CpuModel()
    model.uncond_type = "zero_embed"
    cond = _cond()
    # batch_ddim_sampling: APG takes the place of the 0.7 guidance rescale it would otherwise pass at this width
    with pytest.raises(RuntimeError, match="HIP path"):
        funcs.batch_ddim_sampling(model, dict(cond, fs=torch.tensor([3])), SHAPE, ddim_steps=2, cfg_scale=7.5, apg=APG)
    with pytest.raises(ValueError, match="needs classifier-free guidance"):
        funcs.batch_ddim_sampling(model, dict(cond, fs=torch.tensor([3])), SHAPE, ddim_steps=2, apg=APG)
    for mod in (inference, edit):
        monkeypatch.setattr(mod, "build_conditioning", lambda *a, **k: (cond, cond, None))
    video = torch.zeros(1, 3, 4, 64, 64)
    with pytest.raises(RuntimeError, match="HIP path"):
        inference.image_guided_synthesis(model, [""], video, SHAPE, ddim_steps=2, fs=3, unconditional_guidance_scale=7.5, apg=APG)
    with pytest.raises(ValueError, match="guidance_rescale"):
        inference.image_guided_synthesis(model, [""], video, SHAPE, ddim_steps=2, fs=3, unconditional_guidance_scale=7.5,
                                         guidance_rescale=0.7, apg=APG)
    with pytest.raises(ValueError, match="unknown keys"):
        inference.image_guided_synthesis(model, [""], video, SHAPE, ddim_steps=2, fs=3, unconditional_guidance_scale=7.5,
                                         sampler="dpmpp_2m", apg=dict(APG, scale=2))
    monkeypatch.setattr(edit, "get_latent_z", lambda m, v: torch.zeros(SHAPE))
    with pytest.raises(ValueError, match="unknown keys"):             # invert=False: straight to decode, which checks first
        edit.video_guided_synthesis(model, [""], video, video, SHAPE, ddim_steps=2, fs=3, unconditional_guidance_scale=7.5,
                                    invert=False, apg=dict(APG, scale=2))
    with pytest.raises(RuntimeError, match="HIP path"):
        edit.video_guided_synthesis(model, [""], video, video, SHAPE, ddim_steps=2, fs=3, unconditional_guidance_scale=7.5,
                                    invert=False, apg=APG)
    assert inspect.signature(DynamiCrafterImg2VideoPipeline.__call__).parameters["apg"].default is None


def test_command_line_flags():
    from dynamicrafter_amd.scripts.evaluation import edit, inference
    for mod in (inference, edit):
        a = mod.get_parser().parse_args([])
        assert not hasattr(a, "apg") and not hasattr(a, "apg_space") and inference.apg_from_args(a) is None      # default: off
        a = mod.get_parser().parse_args(["--apg", "0", "15", "-0.5"])
        assert inference.apg_from_args(a) == dict(eta=0.0, norm_threshold=15.0, momentum=-0.5, space="x0")
        a = mod.get_parser().parse_args(["--apg", "0.25", "0", "0", "--apg_space", "model"])
        assert inference.apg_from_args(a) == dict(eta=0.25, norm_threshold=None, momentum=0.0, space="model")
        assert inference.apg_from_args(mod.get_parser().parse_args(["--apg_space", "model"])) is None
        with pytest.raises(SystemExit):
            mod.get_parser().parse_args(["--apg", "0", "15"])
        with pytest.raises(SystemExit):
            mod.get_parser().parse_args(["--apg_space", "eps"])
    from dynamicrafter_amd.lvdm.models.samplers.ddim import apg_config
    assert apg_config(inference.apg_from_args(inference.get_parser().parse_args(["--apg", "0", "15", "-0.5"])))


# ------------------------------------------------------------------ the C ABI
NEW = ("dc_apg_workspace_floats", "dc_apg_reduce", "dc_apg_apply")


def test_apg_entries_are_exported_and_declared():
    from dynamicrafter_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "dcrafter_hip.h")).read()
    declared = set(re.findall(r"\b(dc_[a-z0-9_]+)\s*\(", hdr))
    lib = _hip.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (dc_[a-z0-9_]+)", nm))
    for name in NEW:
        assert name in declared and name in exported and name in _hip.SIGNATURES and hasattr(lib, name)
    for name in NEW[1:]:
        assert _hip.SIGNATURES[name][0] is C.c_int and _hip.SIGNATURES[name][1][-1] is C.c_void_p           # int, stream last
    # the ctypes struct has the header's fields, in its order
    body = re.search(r"typedef struct DcApgParams \{(.*?)\} DcApgParams;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?\w+\*?\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S), re.M)
    assert fields == [f for f, _ in _hip.DcApgParams._fields_]
    src = open(os.path.join(ROOT, "dynamicrafter_amd", "csrc", "guidance.hip")).read()
    assert "atomic" not in re.sub(r"//.*", "", src).lower()           # partial sums in a workspace, added in a fixed order
    assert " guidance " in open(os.path.join(ROOT, "dynamicrafter_amd", "csrc", "build.sh")).read()


def test_workspace_size():
    """Three partial sums per workgroup, min(256, ceil(THW / 256)) workgroups per clip."""
    from dynamicrafter_amd import _hip, ops
    for (B, Cc, THW), G in (((1, 4, 1), 1), ((2, 4, 105), 1), ((3, 4, 256), 1), ((1, 4, 257), 2), ((1, 4, 16384), 64),
                            ((2, 4, 40960), 160), ((1, 4, 65536), 256), ((1, 4, 147456), 256), ((5, 3, 2 ** 31 - 1), 256)):
        assert ops.apg_workspace_floats(B=B, Cc=Cc, THW=THW) == 3 * B * G
    assert _hip.lib().dc_apg_workspace_floats(0, 4, 16) == -2
    with pytest.raises(ValueError):
        ops.apg_workspace_floats(B=1, Cc=4, THW=0)


def test_cabi_refuses_bad_arguments_without_gpu():
    from dynamicrafter_amd import _hip
    lib = _hip.lib()
    q = C.c_void_p(256)

    def params(**kw):
        p = _hip.DcApgParams()
        for k in ("a_t", "sqrt_one_minus_at", "sqrt_acp_t", "sqrt_1macp_t"):
            setattr(p, k, 256)
        p.v_param, p.x0_space, p.cfg_scale, p.eta, p.norm_threshold, p.momentum = 1, 1, 7.5, 0.0, 2.0, -0.5
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    red = lambda p, ec=q, eu=q, ld=4, x=q, m=q, B=2, Cc=4, THW=35, ws=q: lib.dc_apg_reduce(p, ec, eu, ld, x, m, B, Cc, THW, ws, None)
    app = lambda p, ec=q, ld=4, x=q, m=q, out=q, ldo=4, B=2, Cc=4, THW=35, ws=q: lib.dc_apg_apply(p, ec, ld, x, m, out, ldo, B, Cc,
                                                                                                   THW, ws, None)
    for fn in (red, app):
        assert fn(None) == -2
        for missing in ("ec", "m", "ws", "x"):
            assert fn(params(), **{missing: None}) == -2, missing
        assert fn(params(sqrt_acp_t=0)) == -2 and fn(params(sqrt_1macp_t=0)) == -2
        assert fn(params(v_param=0, a_t=0)) == -2 and fn(params(v_param=0, sqrt_one_minus_at=0)) == -2
        assert fn(params(index=-1)) == -2
        for k in ("cfg_scale", "eta", "momentum"):
            assert fn(params(**{k: math.inf})) == -2 and fn(params(**{k: math.nan})) == -2, k
        assert fn(params(norm_threshold=math.nan)) == -2
        for bad in (dict(B=0), dict(B=65536), dict(Cc=0), dict(THW=0), dict(ld=3)):
            assert fn(params(), **bad) == -1, bad
    assert red(params(), eu=None) == -2
    assert app(params(), out=None) == -2
    assert app(params(), ldo=3) == -1

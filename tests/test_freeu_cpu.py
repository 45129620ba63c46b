"""FreeU without a GPU: the real-form skip filter against the published FFT form, the stage selection on the released configs,
argument validation, the command-line flags, and that every caller puts the model's previous setting back when the call raises."""
import ctypes as C
import os
import types

import pytest
import torch
import yaml

from oracle import ddim as oddim
from tests import freeu_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREEU = dict(s1=0.9, s2=0.2, b1=1.5, b2=1.6, version=2)


@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (9, 16), (18, 32), (5, 8)])
@pytest.mark.parametrize("s", [0.2, 0.9, 1.0, 1.7])
def test_real_form_equals_the_published_fft_form(H, W, s):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
    a, b = R.skip_filter_real(x, s), R.skip_filter_fft(x, s)
    assert (a - b).abs().max().item() <= 1e-10
    if s == 1.0:
        assert torch.equal(a, x)
    c = torch.full((1, 1, H, W), 0.75, dtype=torch.float64)           # a constant plane is its own mean: scaled by s
    assert (R.skip_filter_real(c, s) - s * c).abs().max().item() <= 1e-10


def test_backbone_restatement():
    g = torch.Generator().manual_seed(1)
    h = torch.randn(2, 8, 3, 4, generator=g, dtype=torch.float64)
    h[1] = 0.25                                                       # a flat frame: version 2 leaves it alone
    v1 = R.backbone_scale(h, 1.5, 1)
    assert torch.equal(v1[:, :4], h[:, :4] * 1.5) and torch.equal(v1[:, 4:], h[:, 4:])
    v2 = R.backbone_scale(h, 1.5, 2)
    assert torch.equal(v2[1], h[1]) and torch.equal(v2[:, 4:], h[:, 4:])
    f = R.backbone_factor(h, 1.5, 2)[0]
    assert f.min().item() == 1.0 and f.max().item() == 1.5             # mhat spans [0, 1] over a frame
    m = h[0].mean(0)
    assert torch.allclose(f[0], 0.5 * (m - m.min()) / (m.max() - m.min()) + 1.0, rtol=0, atol=1e-14)


@pytest.mark.parametrize("name", ["inference_256_v1.0.yaml", "inference_512_v1.0.yaml", "inference_1024_v1.0.yaml"])
def test_stage_selection_on_the_released_configs(name):
    """Stage 1 on up blocks 0-6 (h has 1280 channels), stage 2 on 7-9 (640), nothing on 10-11 - from the layout alone, no weights."""
    from dynamicrafter_amd.lvdm.modules.networks import openaimodel3d as M
    p = yaml.safe_load(open(os.path.join(ROOT, "dynamicrafter_amd", "configs", name)))["model"]["params"]["unet_config"]["params"]
    plan = M.cat_plan(M._block_layout(p))
    mc = p["model_channels"]
    assert mc == 320 and len(plan) == 12
    stages = M.freeu_stages(plan, mc)
    assert stages == [1] * 7 + [2] * 3 + [None] * 2
    assert [ch for ch, _ in plan] == [1280] * 7 + [640] * 3 + [320] * 2
    assert stages == [R.freeu_stage(ch, mc) for ch, _ in plan]
    for (ch, cs), st in zip(plan, stages):
        if st is not None:
            assert ch % 128 == 0 and cs % 64 == 0                     # what ops.freeu needs


@pytest.fixture(scope="module")
def net():
    from dynamicrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    from tests.golden_cfg import TINY_UNET
    return UNetModel(**TINY_UNET)


def test_tiny_config_follows_the_same_rule(net):
    from dynamicrafter_amd.lvdm.modules.networks.openaimodel3d import freeu_stages
    assert [ch for ch, _ in net._cat_plan] == [256] * 7 + [128] * 3 + [64] * 2
    assert freeu_stages(net._cat_plan, net.model_channels) == [1] * 7 + [2] * 3 + [None] * 2


def test_enable_freeu_validates_and_round_trips(net):
    assert net.freeu is None
    net.enable_freeu(0.9, 0.2, 1.5, 1.6)
    assert net.freeu == dict(s1=0.9, s2=0.2, b1=1.5, b2=1.6, version=1)
    net.enable_freeu(1, 1, 1, 1, version=2)
    assert net.freeu == dict(s1=1.0, s2=1.0, b1=1.0, b2=1.0, version=2)
    before = net.freeu
    for bad in (float("nan"), float("inf"), -float("inf"), None, "0.9", True, 1j):
        for pos in range(4):
            args = [0.9, 0.2, 1.5, 1.6]
            args[pos] = bad
            with pytest.raises(ValueError, match="finite"):
                net.enable_freeu(*args)
    for bad in (0, 3, 1.5, "1", None, True):
        with pytest.raises(ValueError, match="version"):
            net.enable_freeu(0.9, 0.2, 1.5, 1.6, version=bad)
    assert net.freeu == before                                        # a refused call changes nothing
    assert net.set_freeu(None) == before and net.freeu is None
    assert net.set_freeu(before) is None and net.freeu == before
    net.disable_freeu()
    assert net.freeu is None


def test_cabi_refuses_bad_arguments_without_gpu():
    from dynamicrafter_amd import _hip
    lib = _hip.lib()
    q = C.c_void_p(256)
    ok = (q, 192, 128, 64, 2, 3, 5)
    assert lib.dc_freeu_skip_stats(None, *ok[1:], q, None, None, None) == -2
    assert lib.dc_freeu_skip_stats(*ok, None, None, None, None) == -2
    assert lib.dc_freeu_skip_stats(*ok, q, q, None, None) == -2                      # hmean without mm
    assert lib.dc_freeu_hmean(*ok, None, None) == -2
    assert lib.dc_freeu_apply(*ok, None, 1.0, 1.0, None, None, None) == -2
    for bad in ((q, 192, 64, 64, 2, 3, 5),            # ch % 128
                (q, 192, 128, 32, 2, 3, 5),           # cs % 64
                (q, 184, 128, 64, 2, 3, 5),           # ld < ch + cs
                (q, 196, 128, 64, 2, 3, 5),           # ld % 8
                (C.c_void_p(264), 192, 128, 64, 2, 3, 5),          # not 16-byte aligned
                (q, 192, 128, 64, 0, 3, 5), (q, 192, 128, 64, 2, 0, 5), (q, 192, 128, 64, 2, 3, 0),
                (q, 192, 128, 64, 2, 2000, 49),       # H + W beyond the trig table
                (q, 192, 128, 64, 70000, 3, 5),       # F beyond gridDim.y
                (q, 192, 128, 64, 2048, 100, 100)):   # 2^31 elements or more
        assert lib.dc_freeu_skip_stats(*bad, q, None, None, None) == -1, bad
        assert lib.dc_freeu_hmean(*bad, q, None) == -1, bad
        assert lib.dc_freeu_apply(*bad, q, 1.0, 1.0, None, None, None) == -1, bad


def test_scratch_size():
    """Seven sums per (frame, skip channel), times the slices a large plane is summed in (min(8, HW // 256), at least 1);
    version 2 adds the row means and a (min, max) pair per frame."""
    from dynamicrafter_amd import _hip, ops
    for (cs, F, H, W), nz in (((64, 2, 3, 5), 1), ((1280, 32, 5, 8), 1), ((640, 32, 20, 32), 2), ((192, 1, 18, 32), 2),
                              ((320, 32, 40, 64), 8), ((320, 32, 72, 128), 8), ((64, 1, 16, 31), 1), ((64, 1, 16, 32), 2)):
        assert ops.freeu_scratch_floats(cs=cs, F=F, H=H, W=W) == nz * F * cs * 7
        assert ops.freeu_scratch_floats(cs=cs, F=F, H=H, W=W, version=2) == nz * F * cs * 7 + F * H * W + 2 * F
    assert _hip.lib().dc_freeu_scratch_floats(64, 1, 4, 4, 3) == -2
    with pytest.raises(ValueError):
        ops.freeu_scratch_floats(cs=64, F=0, H=4, W=4)


def test_command_line_flags():
    from dynamicrafter_amd.scripts.evaluation import edit, inference
    for mod in (inference, edit):
        a = mod.get_parser().parse_args([])
        assert not hasattr(a, "freeu") and not hasattr(a, "freeu_version") and inference.freeu_from_args(a) is None     # default: off
        a = mod.get_parser().parse_args(["--freeu", "0.9", "0.2", "1.4", "1.6"])
        assert inference.freeu_from_args(a) == dict(s1=0.9, s2=0.2, b1=1.4, b2=1.6, version=1)
        assert inference.freeu_from_args(mod.get_parser().parse_args(["--freeu_version", "2"])) is None
        a = mod.get_parser().parse_args(["--freeu", "0.9", "0.2", "1.4", "1.6", "--freeu_version", "2"])
        assert inference.freeu_from_args(a) == dict(s1=0.9, s2=0.2, b1=1.4, b2=1.6, version=2)
        with pytest.raises(SystemExit):
            mod.get_parser().parse_args(["--freeu", "0.9", "0.2", "1.4"])
        with pytest.raises(SystemExit):
            mod.get_parser().parse_args(["--freeu_version", "3"])


# ------------------------------------------------------------------ the callers restore the previous setting
class _CpuModel:
    """Schedule buffers of a model on the CPU around a real UNetModel: the samplers accept it up to the point where they need
    the GPU, which is inside the FreeU scope."""

    def __init__(self, net):
        ms = oddim.ModelSchedule()
        for k in ("num_timesteps", "parameterization", "use_dynamic_rescale", "alphas_cumprod", "betas",
                  "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"):
            setattr(self, k, getattr(ms, k))
        self.device = torch.device("cpu")
        self.model = types.SimpleNamespace(diffusion_model=net)
        self.temporal_length = 4


@pytest.fixture()
def spied(net, monkeypatch):
    """(model, the settings set_freeu was called with) with a setting already in force."""
    net.enable_freeu(0.5, 0.6, 1.1, 1.2)
    seen = []
    real = net.set_freeu
    monkeypatch.setattr(net, "set_freeu", lambda cfg: (seen.append(cfg), real(cfg))[1])
    yield _CpuModel(net), seen
    net.disable_freeu()


PREV = dict(s1=0.5, s2=0.6, b1=1.1, b2=1.2, version=1)
SHAPE = [1, 4, 4, 8, 8]


def _check(net, seen):
    assert seen == [FREEU, PREV]                  # enabled for the call, then the previous setting put back
    assert net.freeu == PREV


def test_samplers_restore_after_a_raise(spied):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    from dynamicrafter_amd.lvdm.models.samplers.options import model_settings_scope
    freeu_scope = lambda model, cfg: model_settings_scope(model, dict(freeu=cfg))
    model, seen = spied
    net = model.model.diffusion_model
    x = torch.zeros(SHAPE)
    for cls in (DDIMSampler, DPMSolverSampler):
        del seen[:]
        with pytest.raises(RuntimeError, match="HIP path"):
            cls(model).sample(S=2, batch_size=1, shape=SHAPE[1:], conditioning=None, verbose=False, freeu=FREEU)
        _check(net, seen)
    s = DDIMSampler(model)
    s.make_schedule(4, verbose=False)
    for call in (lambda: s.encode(x, None, 2, freeu=FREEU), lambda: s.decode(x, None, 2, freeu=FREEU)):
        del seen[:]
        with pytest.raises(RuntimeError, match="HIP path"):
            call()
        _check(net, seen)
    del seen[:]
    with pytest.raises(ValueError, match="finite"):               # a bad setting is refused before anything runs
        s.encode(x, None, 2, freeu=dict(FREEU, b1=float("nan")))
    assert net.freeu == PREV
    with pytest.raises(ValueError, match="no FreeU"):
        with freeu_scope(types.SimpleNamespace(), FREEU):
            pass
    del seen[:]
    with pytest.raises(RuntimeError, match="HIP path"):           # None leaves the model alone
        s.encode(x, None, 2)
    assert seen == [] and net.freeu == PREV


def test_harness_functions_restore_after_a_raise(spied, monkeypatch):
    from dynamicrafter_amd.scripts.evaluation import edit, funcs, inference
    model, seen = spied
    net = model.model.diffusion_model
    cond = {"c_crossattn": [torch.zeros(1, 141, 128)], "c_concat": [torch.zeros(SHAPE)]}
    with pytest.raises(RuntimeError, match="HIP path"):
        funcs.batch_ddim_sampling(model, dict(cond, fs=torch.tensor([3])), SHAPE, ddim_steps=2, freeu=FREEU)
    _check(net, seen)
    for mod in (inference, edit):
        monkeypatch.setattr(mod, "build_conditioning", lambda *a, **k: (cond, None, None))
    del seen[:]
    with pytest.raises(RuntimeError, match="HIP path"):
        inference.image_guided_synthesis(model, [""], torch.zeros(1, 3, 4, 64, 64), SHAPE, ddim_steps=2, fs=3, freeu=FREEU)
    _check(net, seen)
    monkeypatch.setattr(edit, "get_latent_z", lambda m, v: torch.zeros(SHAPE))
    del seen[:]
    with pytest.raises(RuntimeError, match="HIP path"):
        edit.video_guided_synthesis(model, [""], torch.zeros(1, 3, 4, 64, 64), torch.zeros(1, 3, 4, 64, 64), SHAPE,
                                    ddim_steps=2, fs=3, freeu=FREEU)
    _check(net, seen)


def test_pipeline_has_the_diffusers_methods(net):
    from dynamicrafter_amd.scripts.gradio.dynamicrafter_pipeline import DynamiCrafterImg2VideoPipeline
    pipe = DynamiCrafterImg2VideoPipeline("256_256", model=_CpuModel(net))
    pipe.enable_freeu(0.9, 0.2, 1.4, 1.6)
    assert net.freeu == dict(s1=0.9, s2=0.2, b1=1.4, b2=1.6, version=1)
    pipe.enable_freeu(s1=0.9, s2=0.2, b1=1.4, b2=1.6, version=2)
    assert net.freeu["version"] == 2
    pipe.disable_freeu()
    assert net.freeu is None

"""The table of sampling options (lvdm/models/samplers/options.py) without a GPU: every entry point takes every option, a
further option costs one entry, the combined model-settings scope restores what it found, and the parser helpers."""
import inspect
import types

import pytest
import torch

from oracle import ddim as oddim

FREEU = dict(s1=0.9, s2=0.2, b1=1.4, b2=1.6, version=2)
APG = dict(eta=0.25, norm_threshold=None, momentum=0.0, space="model")
TODO = dict(factor=4, levels=(0, 1), mode="mean")
ALL_FLAGS = ["--freeu", "0.9", "0.2", "1.4", "1.6", "--freeu_version", "2", "--apg", "0.25", "0", "0", "--apg_space", "model",
             "--token_downsampling", "4", "--token_downsampling_levels", "0", "1", "--token_downsampling_mode", "mean"]
SHAPE = [1, 4, 4, 8, 8]


class _CpuModel:
    """Schedule buffers of a model on the CPU around `net`: the samplers accept it up to the point where they need the GPU,
    which is inside the model-settings scope (tests/test_todo_cpu.py)."""

    def __init__(self, net):
        ms = oddim.ModelSchedule()
        for k in ("num_timesteps", "parameterization", "use_dynamic_rescale", "alphas_cumprod", "betas",
                  "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"):
            setattr(self, k, getattr(ms, k))
        self.device = torch.device("cpu")
        self.model = types.SimpleNamespace(diffusion_model=net)
        self.temporal_length = 4


class _Net:
    """A stand-in UNet: set_<name> for the given names, each recording its calls and returning the previous setting."""

    def __init__(self, **settings):
        self.settings, self.calls = dict(settings), {k: [] for k in settings}
        for name in settings:
            setattr(self, "set_" + name, lambda cfg, name=name: self._set(name, cfg))

    def _set(self, name, cfg):
        self.calls[name].append(cfg)
        if isinstance(cfg, dict) and cfg.get("factor") == 9:      # what a model's own validation does
            raise ValueError(f"{name}: refused")
        prev, self.settings[name] = self.settings[name], cfg
        return prev


def _entry_points():
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    from dynamicrafter_amd.scripts.evaluation import edit, funcs, inference
    from dynamicrafter_amd.scripts.gradio.dynamicrafter_pipeline import DynamiCrafterImg2VideoPipeline
    samplers = [DDIMSampler.sample, DDIMSampler.ddim_sampling, DDIMSampler.decode, DDIMSampler.encode, DPMSolverSampler.sample]
    harness = [inference.image_guided_synthesis, funcs.batch_ddim_sampling, edit.video_guided_synthesis,
               DynamiCrafterImg2VideoPipeline.__call__]
    return samplers, harness


# ------------------------------------------------------------------ 1. the table against the entry points
def test_every_entry_point_takes_every_option():
    from dynamicrafter_amd.lvdm.models.samplers import options
    assert list(options.OPTIONS) == ["freeu", "apg", "token_downsampling"]
    assert [o.name for o in options.of_kind(options.MODEL_SETTING)] == ["freeu", "token_downsampling"]
    assert [o.name for o in options.of_kind(options.RUN_SETTING)] == ["apg"]
    samplers, harness = _entry_points()
    for fn in samplers + harness:
        params = inspect.signature(fn).parameters
        forwards = any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values())
        for name in options.OPTIONS:
            assert (name in params and params[name].default is None) or forwards, (fn.__qualname__, name)
    for fn in harness:                                  # the harness functions name them, and document them from the table
        params = inspect.signature(fn).parameters
        for opt in options.OPTIONS.values():
            assert params[opt.name].default is None, (fn.__qualname__, opt.name)
            assert opt.doc in fn.__doc__, (fn.__qualname__, opt.name)


def test_decode_takes_the_tables_names_only_and_encode_refuses_run_settings():
    from dynamicrafter_amd.lvdm.models.samplers import options
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    s = DDIMSampler(_CpuModel(_Net(freeu=None, token_downsampling=None)))
    s.make_schedule(4, verbose=False)
    x = torch.zeros(SHAPE)
    with pytest.raises(TypeError, match="unexpected keyword argument 'guidance'"):
        s.decode(x, None, 2, guidance=1.0)
    with pytest.raises(RuntimeError, match="HIP path"):
        s.decode(x, None, 2, freeu=None, apg=None, token_downsampling=None)
    for opt in options.of_kind(options.RUN_SETTING):
        for value in (dict(opt.keys), None):
            with pytest.raises(ValueError, match=f"encode: {opt.name}= is a sampling-time guidance with a running state; an "
                                                 f"inversion under it is not defined"):
                s.encode(x, None, 2, **{opt.name: value})
    with pytest.raises(RuntimeError, match="HIP path"):
        s.encode(x, None, 2)


# ------------------------------------------------------------------ 2. a fourth option costs one entry
def test_a_fourth_option_costs_one_entry(monkeypatch):
    from dynamicrafter_amd.lvdm.models.samplers import options
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    from dynamicrafter_amd.scripts.evaluation import edit, inference
    probe = options.Option("probe", "probe", options.MODEL_SETTING, dict(gain=1.0), "`probe`: a throw-away setting.",
                           (("--probe", dict(type=float, help="gain")),), lambda probe: dict(gain=probe))
    monkeypatch.setitem(options.OPTIONS, "probe", probe)
    new, prev = dict(gain=2.5), dict(gain=0.5)
    # both command lines, the namespace helper, the harness helper
    for mod in (inference, edit):
        assert not hasattr(mod.get_parser().parse_args([]), "probe")
        args = mod.get_parser().parse_args(["--probe", "2.5"])
        assert options.options_from_args(args) == dict(probe=new)
        assert options.from_args("probe", args) == new
    assert options.fold(dict(x_T=None), probe=new, apg=None) == dict(x_T=None, probe=new)
    # scoped and restored around the sampler calls, which raise inside the scope
    net = _Net(probe=prev)
    model = _CpuModel(net)
    x = torch.zeros(SHAPE)
    for cls in (DDIMSampler, DPMSolverSampler):
        del net.calls["probe"][:]
        with pytest.raises(RuntimeError, match="HIP path"):
            cls(model).sample(S=2, batch_size=1, shape=SHAPE[1:], conditioning=None, verbose=False, probe=new)
        assert net.calls["probe"] == [new, prev] and net.settings["probe"] == prev
    s = DDIMSampler(model)
    s.make_schedule(4, verbose=False)
    for call in (lambda: s.encode(x, None, 2, probe=new), lambda: s.decode(x, None, 2, probe=new)):
        del net.calls["probe"][:]
        with pytest.raises(RuntimeError, match="HIP path"):
            call()
        assert net.calls["probe"] == [new, prev] and net.settings["probe"] == prev
    with pytest.raises(ValueError, match="unknown keys"):
        s.encode(x, None, 2, probe=dict(gian=2.5))
    with pytest.raises(ValueError, match="has no probe"):
        DDIMSampler(_CpuModel(_Net())).sample(S=2, batch_size=1, shape=SHAPE[1:], conditioning=None, verbose=False, probe=new)
    # and through a harness function, which has never heard of it
    monkeypatch.setattr(inference, "build_conditioning", lambda *a, **k: ({"c_crossattn": [torch.zeros(1, 141, 128)]}, None, None))
    del net.calls["probe"][:]
    with pytest.raises(RuntimeError, match="HIP path"):
        inference.image_guided_synthesis(model, [""], torch.zeros(1, 3, 4, 64, 64), SHAPE, ddim_steps=2, fs=3, probe=new)
    assert net.calls["probe"] == [new, prev] and net.settings["probe"] == prev


# ------------------------------------------------------------------ 3. the combined scope
def test_combined_scope_restores_both():
    from dynamicrafter_amd.lvdm.models.samplers.options import model_settings_scope
    prev = dict(freeu=dict(s1=0.5, s2=0.6, b1=1.1, b2=1.2, version=1), token_downsampling=dict(factor=3, levels=(2,), mode="nearest"))
    net = _Net(**prev)
    model = _CpuModel(net)
    with pytest.raises(KeyError, match="inside"):
        with model_settings_scope(model, dict(freeu=FREEU, token_downsampling=TODO)):
            assert net.settings == dict(freeu=FREEU, token_downsampling=TODO)
            raise KeyError("inside")
    assert net.calls == dict(freeu=[FREEU, prev["freeu"]], token_downsampling=[TODO, prev["token_downsampling"]])
    assert net.settings == prev
    net.calls = dict(freeu=[], token_downsampling=[])
    with model_settings_scope(model, dict(freeu=None, token_downsampling=None)):
        pass
    with model_settings_scope(net, {}):                 # a UNet itself; nothing given
        pass
    assert net.calls == dict(freeu=[], token_downsampling=[]) and net.settings == prev
    # the second setting is refused by the model: the block is not entered and the first is put back
    with pytest.raises(ValueError, match="token_downsampling: refused"):
        with model_settings_scope(model, dict(freeu=FREEU, token_downsampling=dict(TODO, factor=9))):
            pytest.fail("entered the block with a refused setting")
    assert net.calls == dict(freeu=[FREEU, prev["freeu"]], token_downsampling=[dict(TODO, factor=9)]) and net.settings == prev
    for bad, match in ((dict(TODO, scale=2), "unknown keys"), ((4, (0, 1), "mean"), "dict"), (4, "dict")):
        with pytest.raises(ValueError, match=match):
            with model_settings_scope(model, dict(freeu=FREEU, token_downsampling=bad)):
                pytest.fail("entered the block with a refused setting")
        assert net.settings == prev


# ------------------------------------------------------------------ 4. the parser helpers
def test_parser_helpers():
    from dynamicrafter_amd.lvdm.models.samplers import options
    from dynamicrafter_amd.scripts.evaluation import edit, inference
    for mod in (inference, edit):
        assert options.options_from_args(mod.get_parser().parse_args([])) == {}
        args = mod.get_parser().parse_args(ALL_FLAGS)
        assert options.options_from_args(args) == dict(freeu=FREEU, apg=APG, token_downsampling=TODO)
        assert (inference.freeu_from_args(args), inference.apg_from_args(args), inference.token_downsampling_from_args(args)) == \
            (FREEU, APG, TODO)
        assert options.options_from_args(mod.get_parser().parse_args(["--token_downsampling", "2"])) == \
            dict(token_downsampling=dict(factor=2, levels=(0,), mode="nearest"))
    assert options.fold(dict(apg=APG), freeu=None, apg=None, token_downsampling=TODO) == dict(apg=APG, token_downsampling=TODO)

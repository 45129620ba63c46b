"""K/V token downsampling without a GPU: the restated UNet loop against the oracle's, the pooling definition against torch's
slicing / avg_pool2d, argument validation of the model, the scope helper and the C entry, the command-line flags, and that
every caller puts the model's previous setting back when the call raises."""
import ctypes as C
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import ddim as oddim
from oracle import unet as ounet
from tests import todo_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TODO = dict(factor=2, levels=(0, 1), mode="mean")
POOL_CASES = [(9, 16, 2), (5, 7, 3), (1, 1, 2), (4, 6, 2), (18, 32, 4), (3, 3, 8)]


# ------------------------------------------------------------------ the restatement
def test_restated_loop_is_the_oracles_loop():
    from oracle.weights import fill_state_dict
    from tests.golden_cfg import TINY_UNET
    ocfg = ounet.UNetCfg.from_params(dict(TINY_UNET, default_fs=24))
    sd = fill_state_dict(ounet.unet_param_shapes(ocfg), seed=11)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 8, 2, 8, 8, generator=g)
    ctx = torch.randn(1, 77 + 16 * 2, 128, generator=g)
    ts, fs = torch.tensor([321]), torch.tensor([12])
    plain = ounet.unet_forward(sd, ocfg, x, ts, ctx, fs)
    assert torch.equal(R.unet_forward_todo(sd, ocfg, x, ts, ctx, fs, todo=None), plain)
    on = R.unet_forward_todo(sd, ocfg, x, ts, ctx, fs, todo=dict(factor=2, levels=(0,)))
    assert on.shape == plain.shape and torch.isfinite(on).all() and not torch.equal(on, plain)
    # the level is tracked through down / up (and ends at 0: asserted inside): level 3 of an 8 x 8 latent is one token, which
    # pooling keeps, so selecting it changes not a bit; level 2 is 2 x 2 tokens pooled to one
    assert torch.equal(R.unet_forward_todo(sd, ocfg, x, ts, ctx, fs, todo=dict(factor=2, levels=(3,))), plain)
    lv2 = R.unet_forward_todo(sd, ocfg, x, ts, ctx, fs, todo=dict(factor=2, levels=(2,), mode="mean"))
    assert not torch.equal(lv2, plain) and not torch.equal(lv2, on)


@pytest.mark.parametrize("H,W,f", POOL_CASES)
def test_pool_tokens_is_slicing_and_avg_pool(H, W, f):
    Fr, Cc = 3, 8
    g = torch.Generator().manual_seed(100 * H + 10 * W + f)
    n = torch.randn(Fr, H * W, Cc, generator=g, dtype=torch.float64)
    Hp, Wp = R.pooled_grid(H, W, f)
    assert (Hp, Wp) == ((H + f - 1) // f, (W + f - 1) // f)
    near = R.pool_tokens(n, H, W, f, "nearest")
    assert near.dtype == torch.float64 and near.shape == (Fr, Hp * Wp, Cc)
    assert torch.equal(near, n.reshape(Fr, H, W, Cc)[:, ::f, ::f].reshape(Fr, Hp * Wp, Cc))
    mean = R.pool_tokens(n, H, W, f, "mean")
    ref = F.avg_pool2d(n.reshape(Fr, H, W, Cc).permute(0, 3, 1, 2), f, ceil_mode=True, count_include_pad=False)
    assert ref.shape[-2:] == (Hp, Wp)
    assert (mean - ref.permute(0, 2, 3, 1).reshape(Fr, Hp * Wp, Cc)).abs().max().item() <= 1e-14
    assert torch.equal(R.pool_tokens(n.float(), H, W, f, "mean"), R.pool_tokens(n.float().double(), H, W, f, "mean"))
    with pytest.raises(ValueError):
        R.pool_tokens(n, H, W, f, "max")


def test_ops_pooled_grid_is_the_restatements():
    from dynamicrafter_amd import ops
    for H, W, f in POOL_CASES:
        assert ops.pooled_grid(H, W, f) == R.pooled_grid(H, W, f)


def test_self_attention_todo_at_factor_covering_nothing_is_plain_attention():
    """Pooling a 1 x 1 grid keeps its one token: the restated attn1 then is the oracle's cross_attention with context None."""
    g = torch.Generator().manual_seed(3)
    sd = {f"a.to_{k}.weight": torch.randn(64, 64, generator=g) * 0.1 for k in "qkv"}
    sd["a.to_out.0.weight"] = torch.randn(64, 64, generator=g) * 0.1
    sd["a.to_out.0.bias"] = torch.randn(64, generator=g) * 0.1
    n = torch.randn(2, 1, 64, generator=g)
    ref = ounet.cross_attention(sd, "a", n, None, 1, 64, None, False)
    for mode in R.MODES:
        assert torch.equal(R.self_attention_todo(sd, "a", n, 1, 64, 1, 1, 2, mode), ref)


# ------------------------------------------------------------------ the model's setting
@pytest.fixture(scope="module")
def net():
    from dynamicrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    from tests.golden_cfg import TINY_UNET
    return UNetModel(**TINY_UNET)


def test_spatial_levels_of_the_layouts(net):
    import yaml
    from dynamicrafter_amd.lvdm.modules.networks import openaimodel3d as M
    assert M.spatial_levels(net._layout) == [0, 1, 2, 3]
    for name in ("inference_256_v1.0.yaml", "inference_512_v1.0.yaml", "inference_1024_v1.0.yaml"):
        p = yaml.safe_load(open(os.path.join(ROOT, "dynamicrafter_amd", "configs", name)))["model"]["params"]["unet_config"]["params"]
        assert M.spatial_levels(M._block_layout(p)) == [0, 1, 2, 3]
    only_deep = dict(net._cfg, attention_resolutions=[4])             # transformers at level 2, and the middle block's at 3
    assert M.spatial_levels(M._block_layout(only_deep)) == [2, 3]


def test_enable_validates_and_round_trips(net):
    assert net.token_downsampling is None
    net.enable_token_downsampling()
    assert net.token_downsampling == dict(factor=2, levels=(0,), mode="nearest")
    net.enable_token_downsampling(4, levels=[2, 0, 0], mode="mean")
    assert net.token_downsampling == dict(factor=4, levels=(0, 2), mode="mean")
    net.enable_token_downsampling(8, levels={1})
    before = net.token_downsampling
    assert before == dict(factor=8, levels=(1,), mode="nearest")
    got = net.token_downsampling
    got["factor"] = 3                                                 # a copy: editing it does not reach the model
    assert net.token_downsampling == before
    for bad in (1, 9, 0, -2, 2.0, "2", None, True, False):
        with pytest.raises(ValueError, match="factor"):
            net.enable_token_downsampling(bad)
    for bad in ((), [], (4,), (-1,), (0, 4), (0.0,), ("0",), (True,), (None,)):
        with pytest.raises(ValueError, match="level"):
            net.enable_token_downsampling(2, levels=bad)
    for bad in (0, None, "0", "01", 1.5):
        with pytest.raises(ValueError, match="levels"):
            net.enable_token_downsampling(2, levels=bad)
    for bad in ("max", "Nearest", "", None, 0, 1):
        with pytest.raises(ValueError, match="mode"):
            net.enable_token_downsampling(2, mode=bad)
    assert net.token_downsampling == before                           # a refused call changes nothing
    assert net.set_token_downsampling(None) == before and net.token_downsampling is None
    assert net.set_token_downsampling(before) is None and net.token_downsampling == before
    net.disable_token_downsampling()
    assert net.token_downsampling is None


def test_a_level_without_a_spatial_transformer_is_refused():
    from dynamicrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    from tests.golden_cfg import TINY_UNET
    deep = UNetModel(**dict(TINY_UNET, attention_resolutions=[4]))
    deep.enable_token_downsampling(2, levels=(2,))
    deep.enable_token_downsampling(2, levels=(3, 2))                  # the middle block's transformer sits at the last level
    deep.enable_token_downsampling(2, levels=(2,))
    for lv in ((0,), (1,), (0, 2)):
        with pytest.raises(ValueError, match="holds no spatial transformer"):
            deep.enable_token_downsampling(2, levels=lv)
    assert deep.token_downsampling == dict(factor=2, levels=(2,), mode="nearest")


def test_the_setting_survives_a_weight_load_and_the_split_weights_do_not(net):
    """load_state_dict drops the packed table (the split q / kv weights live in it); the setting is the user's and stays."""
    net.enable_token_downsampling(2)
    try:
        net._packed = {"device": "x", "attn1_split": True}
        net.load_state_dict(net.state_dict())
        assert net._packed is None and net.token_downsampling == dict(factor=2, levels=(0,), mode="nearest")
    finally:
        net.disable_token_downsampling()


# ------------------------------------------------------------------ the C entry
def test_export_is_declared_in_the_header_and_bound():
    from dynamicrafter_amd import _hip
    text = open(os.path.join(ROOT, "include", "dcrafter_hip.h")).read()
    m = re.search(r"int\s+dc_ln_pool_tokens\s*\(([^;]*)\)\s*;", text)
    assert m, "dc_ln_pool_tokens is not declared in include/dcrafter_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = _hip.SIGNATURES["dc_ln_pool_tokens"]
    assert res is C.c_int and len(args) == len(params) == 14
    for p, a in zip(params, args):                                    # pointer / int / float, one by one
        want = C.c_void_p if "*" in p else C.c_float if p.startswith("float") else C.c_int
        assert a is want, (p, a)
    assert "replaces" in text[text.rfind("/*", 0, m.start()):m.start()]
    assert "token_pool" in open(os.path.join(ROOT, "dynamicrafter_amd", "csrc", "build.sh")).read()
    assert hasattr(_hip.lib(), "dc_ln_pool_tokens")


def test_cabi_refuses_bad_arguments_without_gpu():
    from dynamicrafter_amd import _hip
    fn = _hip.lib().dc_ln_pool_tokens
    q = C.c_void_p(256)
    ok = dict(x=q, ldx=64, y=q, ldy=64, gamma=q, beta=q, F=2, H=4, W=6, C=64, factor=2, mode=0)
    call = lambda **kw: fn(*dict(ok, **kw).values(), 1e-5, None)
    for k in ("x", "y", "gamma", "beta"):
        assert call(**{k: None}) == -2, k
    for bad in (dict(C=60), dict(C=0), dict(C=2056, ldx=2056, ldy=2056), dict(ldx=68), dict(ldy=68), dict(ldx=56), dict(ldy=56),
                dict(x=C.c_void_p(264)), dict(y=C.c_void_p(264)), dict(F=0), dict(H=0), dict(W=0), dict(H=-1),
                dict(factor=1), dict(factor=9), dict(factor=0), dict(mode=2), dict(mode=-1),
                dict(F=2048, H=1024, W=1024)):                         # 2^31 input rows
        assert call(**bad) == -1, bad


def test_ops_refuses_before_a_launch():
    """ops.ln_pool_tokens checks its operands on the host: these raise on CPU tensors' metadata, ahead of any launch."""
    from dynamicrafter_amd import ops
    x = torch.zeros(48, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="CUDA"):
        ops.ln_pool_tokens(x, x, torch.zeros(64), torch.zeros(64), F=2, H=4, W=6, factor=2, mode="nearest")


# ------------------------------------------------------------------ the command line
def test_command_line_flags():
    from dynamicrafter_amd.scripts.evaluation import edit, inference
    names = ("token_downsampling", "token_downsampling_levels", "token_downsampling_mode")
    for mod in (inference, edit):
        a = mod.get_parser().parse_args([])
        assert not any(hasattr(a, n) for n in names) and inference.token_downsampling_from_args(a) is None
        a = mod.get_parser().parse_args(["--token_downsampling", "2"])
        assert inference.token_downsampling_from_args(a) == dict(factor=2, levels=(0,), mode="nearest")
        assert not hasattr(a, "token_downsampling_levels") and not hasattr(a, "token_downsampling_mode")
        a = mod.get_parser().parse_args(["--token_downsampling", "4", "--token_downsampling_levels", "0", "1",
                                         "--token_downsampling_mode", "mean"])
        assert inference.token_downsampling_from_args(a) == dict(factor=4, levels=(0, 1), mode="mean")
        for argv in (["--token_downsampling_levels", "1"], ["--token_downsampling_mode", "mean"]):
            with pytest.raises(ValueError, match="needs --token_downsampling"):
                inference.token_downsampling_from_args(mod.get_parser().parse_args(argv))
        for argv in (["--token_downsampling", "1"], ["--token_downsampling", "9"], ["--token_downsampling", "2.5"],
                     ["--token_downsampling"], ["--token_downsampling_mode", "max"], ["--token_downsampling_levels"],
                     ["--token_downsampling_levels", "x"]):
            with pytest.raises(SystemExit):
                mod.get_parser().parse_args(argv)


def test_namespace_without_the_flags_is_what_it_was():
    """The three flags have argparse.SUPPRESS defaults: a run without them sees the attribute names it saw before."""
    from dynamicrafter_amd.scripts.evaluation import edit, inference
    for mod in (inference, edit):
        plain = vars(mod.get_parser().parse_args([]))
        assert not [k for k in plain if "token" in k]
        with_flag = vars(mod.get_parser().parse_args(["--token_downsampling", "2"]))
        assert {k: v for k, v in with_flag.items() if k != "token_downsampling"} == plain


# ------------------------------------------------------------------ the callers restore the previous setting
class _CpuModel:
    """Schedule buffers of a model on the CPU around a real UNetModel: the samplers accept it up to the point where they need
    the GPU, which is inside the scope."""

    def __init__(self, net):
        ms = oddim.ModelSchedule()
        for k in ("num_timesteps", "parameterization", "use_dynamic_rescale", "alphas_cumprod", "betas",
                  "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"):
            setattr(self, k, getattr(ms, k))
        self.device = torch.device("cpu")
        self.model = types.SimpleNamespace(diffusion_model=net)
        self.temporal_length = 4


PREV = dict(factor=3, levels=(2,), mode="nearest")
SHAPE = [1, 4, 4, 8, 8]


@pytest.fixture()
def spied(net, monkeypatch):
    """(model, the settings set_token_downsampling was called with) with a setting already in force."""
    net.enable_token_downsampling(**PREV)
    seen = []
    real = net.set_token_downsampling
    monkeypatch.setattr(net, "set_token_downsampling", lambda cfg: (seen.append(cfg), real(cfg))[1])
    yield _CpuModel(net), seen
    net.disable_token_downsampling()


def _check(net, seen):
    assert seen == [TODO, PREV]                   # enabled for the call, then the previous setting put back
    assert net.token_downsampling == PREV


def test_scope_helper(spied):
    from dynamicrafter_amd.lvdm.models.samplers.options import model_settings_scope
    token_downsampling_scope = lambda model, cfg: model_settings_scope(model, dict(token_downsampling=cfg))
    model, seen = spied
    net = model.model.diffusion_model
    with token_downsampling_scope(model, TODO):
        assert net.token_downsampling == TODO
    _check(net, seen)
    del seen[:]
    with token_downsampling_scope(net, dict(factor=4)):               # a UNetModel itself; missing keys take the defaults
        assert net.token_downsampling == dict(factor=4, levels=(0,), mode="nearest")
    assert net.token_downsampling == PREV
    del seen[:]
    with token_downsampling_scope(model, None):                       # None leaves the model alone
        assert net.token_downsampling == PREV
    assert seen == []
    with pytest.raises(KeyError):
        with token_downsampling_scope(model, TODO):
            raise KeyError("inside")
    assert net.token_downsampling == PREV
    for bad, match in ((dict(TODO, factor=9), "factor"), (dict(TODO, levels=()), "levels"), (dict(TODO, levels=(7,)), "level"),
                       (dict(TODO, mode="max"), "mode"), (dict(TODO, scale=2), "unknown keys"), ((2, (0,), "mean"), "dict"),
                       (2, "dict")):
        with pytest.raises(ValueError, match=match):
            with token_downsampling_scope(model, bad):
                pytest.fail("entered the block with a refused setting")
        assert net.token_downsampling == PREV
    with pytest.raises(ValueError, match="no token downsampling"):
        with token_downsampling_scope(types.SimpleNamespace(), TODO):
            pass


def test_samplers_restore_after_a_raise(spied):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    model, seen = spied
    net = model.model.diffusion_model
    x = torch.zeros(SHAPE)
    for cls in (DDIMSampler, DPMSolverSampler):
        del seen[:]
        with pytest.raises(RuntimeError, match="HIP path"):
            cls(model).sample(S=2, batch_size=1, shape=SHAPE[1:], conditioning=None, verbose=False, token_downsampling=TODO)
        _check(net, seen)
    s = DDIMSampler(model)
    s.make_schedule(4, verbose=False)
    for call in (lambda: s.encode(x, None, 2, token_downsampling=TODO), lambda: s.decode(x, None, 2, token_downsampling=TODO)):
        del seen[:]
        with pytest.raises(RuntimeError, match="HIP path"):
            call()
        _check(net, seen)
    del seen[:]
    with pytest.raises(ValueError, match="mode"):                 # a bad setting is refused before anything runs
        s.encode(x, None, 2, token_downsampling=dict(TODO, mode="max"))
    assert net.token_downsampling == PREV
    del seen[:]
    with pytest.raises(RuntimeError, match="HIP path"):           # None leaves the model alone
        s.encode(x, None, 2)
    assert seen == [] and net.token_downsampling == PREV
    # together with freeu=: both settings are put back
    net.enable_freeu(0.5, 0.6, 1.1, 1.2)
    try:
        with pytest.raises(RuntimeError, match="HIP path"):
            s.decode(x, None, 2, token_downsampling=TODO, freeu=dict(s1=0.9, s2=0.2, b1=1.5, b2=1.6))
        assert net.token_downsampling == PREV and net.freeu == dict(s1=0.5, s2=0.6, b1=1.1, b2=1.2, version=1)
    finally:
        net.disable_freeu()


def test_harness_functions_restore_after_a_raise(spied, monkeypatch):
    from dynamicrafter_amd.scripts.evaluation import edit, funcs, inference
    model, seen = spied
    net = model.model.diffusion_model
    cond = {"c_crossattn": [torch.zeros(1, 141, 128)], "c_concat": [torch.zeros(SHAPE)]}
    with pytest.raises(RuntimeError, match="HIP path"):
        funcs.batch_ddim_sampling(model, dict(cond, fs=torch.tensor([3])), SHAPE, ddim_steps=2, token_downsampling=TODO)
    _check(net, seen)
    for mod in (inference, edit):
        monkeypatch.setattr(mod, "build_conditioning", lambda *a, **k: (cond, None, None))
    del seen[:]
    with pytest.raises(RuntimeError, match="HIP path"):
        inference.image_guided_synthesis(model, [""], torch.zeros(1, 3, 4, 64, 64), SHAPE, ddim_steps=2, fs=3,
                                         token_downsampling=TODO)
    _check(net, seen)
    monkeypatch.setattr(edit, "get_latent_z", lambda m, v: torch.zeros(SHAPE))
    del seen[:]
    with pytest.raises(RuntimeError, match="HIP path"):
        edit.video_guided_synthesis(model, [""], torch.zeros(1, 3, 4, 64, 64), torch.zeros(1, 3, 4, 64, 64), SHAPE,
                                    ddim_steps=2, fs=3, token_downsampling=TODO)
    assert seen[0] == TODO and seen[-1] == PREV and net.token_downsampling == PREV


def test_pipeline_has_the_methods_and_the_keyword(net):
    import inspect
    from dynamicrafter_amd.scripts.gradio.dynamicrafter_pipeline import DynamiCrafterImg2VideoPipeline
    pipe = DynamiCrafterImg2VideoPipeline("256_256", model=_CpuModel(net))
    pipe.enable_token_downsampling()
    assert net.token_downsampling == dict(factor=2, levels=(0,), mode="nearest")
    pipe.enable_token_downsampling(factor=4, levels=(0, 1), mode="mean")
    assert net.token_downsampling == dict(factor=4, levels=(0, 1), mode="mean")
    with pytest.raises(ValueError, match="factor"):
        pipe.enable_token_downsampling(factor=1)
    pipe.disable_token_downsampling()
    assert net.token_downsampling is None
    assert inspect.signature(DynamiCrafterImg2VideoPipeline.__call__).parameters["token_downsampling"].default is None

"""The optional dict keywords of a sampling call (`freeu=`, `apg=`, `token_downsampling=`), declared once: OPTIONS below. What
carries an option from a command line or a harness function to the sampler reads this table, so a further option is one
entry here plus whatever implements it.

An option is one of two kinds:
  MODEL_SETTING  a setting of the UNet, in force for the duration of a call and put back afterwards (`model_settings_scope`,
                 `takes_model_settings`). The UNet validates it: `set_<name>(cfg)` enables cfg (None: disables) and returns
                 the setting that was in force.
  RUN_SETTING    handed to the run, which owns whatever state it needs (`apg=`: validated by ddim.apg_config / check_apg).

OPTIONS holds the options that act on a latent of the model's own extent. EXTENT_OPTIONS holds the run settings that
change what extent a call denoises (`tiles=`: frames larger than the trained size, samplers/tiles.py); they
are a table of their own because they are no guidance - an inversion or a partial run refuses them for its own reason,
as it refuses `window_stride` - and the same helpers (`fold`, `documented`, the parser helpers) serve both tables.
"""
import argparse
import contextlib
import functools
from collections import namedtuple

MODEL_SETTING, RUN_SETTING = "model setting", "run setting"
REQUIRED = "<required>"                                   # the default of a key that has none

# name: the keyword; title: what the messages call it; keys: the allowed keys with their defaults; doc: the paragraph that
# `documented` appends; flags: (flag, add_argument's arguments) pairs, all with default SUPPRESS, so a namespace holds the
# given flags only; from_flags: the parsed values of the given flags (at least one) -> the dict, or None
Option = namedtuple("Option", "name title kind keys doc flags from_flags")


def _token_downsampling_from_flags(token_downsampling=None, **secondary):
    """The two secondary flags without FACTOR are an error, not a silent no-op."""
    if token_downsampling is None:
        raise ValueError(f"--{next(iter(secondary))} needs --token_downsampling FACTOR")
    return dict(factor=token_downsampling, levels=tuple(secondary.get("token_downsampling_levels", (0,))),
                mode=secondary.get("token_downsampling_mode", "nearest"))


OPTIONS = {o.name: o for o in (
    Option("freeu", "FreeU", MODEL_SETTING, dict(s1=REQUIRED, s2=REQUIRED, b1=REQUIRED, b2=REQUIRED, version=1),
           "`freeu` (not in the reference): None, or dict(s1=, s2=, b1=, b2=, version=1) - FreeU on the UNet's decoder for this "
           "call (UNetModel.enable_freeu, DESIGN 4.12); the model's previous setting is back when the call returns or raises.",
           (("--freeu", dict(type=float, nargs=4, metavar=("S1", "S2", "B1", "B2"), help="FreeU on the UNet's decoder, diffusers' "
                             "argument order (its SD-2.1 suggestion: 0.9 0.2 1.4 1.6); default off")),
            ("--freeu_version", dict(type=int, choices=(1, 2), help="FreeU backbone scaling: 1 = constant b (default), 2 = b "
                                     "weighted by the normalised channel mean"))),
           lambda freeu=None, freeu_version=1: freeu and dict(zip(("s1", "s2", "b1", "b2"), freeu), version=freeu_version)),
    Option("apg", "adaptive projected guidance", RUN_SETTING, dict(eta=0.0, norm_threshold=None, momentum=0.0, space="x0"),
           "`apg` (not in the reference): None, or dict(eta=0.0, norm_threshold=None, momentum=0.0, space=\"x0\") - adaptive "
           "projected guidance in place of the plain CFG combine (lvdm/models/samplers/ddim.py, DESIGN 4.13). Two guidance "
           "branches at a guidance scale other than 1 only, and not with guidance_rescale > 0.",
           (("--apg", dict(type=float, nargs=3, metavar=("ETA", "NORM_THRESHOLD", "MOMENTUM"), help="adaptive projected guidance "
                           "in place of plain CFG (the paper's suggestion for SDXL-class models: 0 15 -0.5); NORM_THRESHOLD <= 0 "
                           "switches the clipping off; needs --guidance_rescale 0; default off")),
            ("--apg_space", dict(type=str, choices=("x0", "model"), help="where APG projects: x0 = the denoised prediction "
                                 "(default, the paper), model = the raw output (diffusers)"))),
           lambda apg=None, apg_space="x0": apg and dict(eta=apg[0], norm_threshold=apg[1] if apg[1] > 0 else None,
                                                         momentum=apg[2], space=apg_space)),
    Option("token_downsampling", "token downsampling", MODEL_SETTING, dict(factor=2, levels=(0,), mode="nearest"),
           "`token_downsampling` (not in the reference): None, or dict(factor=2, levels=(0,), mode=\"nearest\") - K/V token "
           "downsampling in the spatial self-attentions of those resolution levels for this call "
           "(UNetModel.enable_token_downsampling, DESIGN 4.14); the model's previous setting is back when the call returns or "
           "raises.",
           (("--token_downsampling", dict(type=int, choices=tuple(range(2, 9)), metavar="FACTOR", help="K/V token downsampling "
                                          "(ToDo) in the spatial self-attentions: keys and values from the tokens subsampled by "
                                          "FACTOR (2..8) per axis; default off")),
            ("--token_downsampling_levels", dict(type=int, nargs="+", metavar="L", help="resolution levels it acts on (0 = the "
                                                 "latent's own resolution; default 0)")),
            ("--token_downsampling_mode", dict(type=str, choices=("nearest", "mean"), help="nearest = every FACTOR-th token "
                                               "(default, the paper), mean = the average of each FACTOR x FACTOR cell"))),
           _token_downsampling_from_flags),
)}


def _tiles_from_flags(tile=None, **secondary):
    """The command line gives pixels; `tiles.tiles_from_pixels` converts with the autoencoder's factor."""
    if tile is None:
        raise ValueError(f"--{next(iter(secondary))} needs --tile HEIGHT WIDTH")
    stride = secondary.get("tile_stride")
    return dict(size=tuple(tile), stride=None if stride is None else tuple(stride),
                shift=tuple(secondary.get("tile_shift", (0, 0))))


EXTENT_OPTIONS = {o.name: o for o in (
    Option("tiles", "spatial tiles", RUN_SETTING, dict(size=REQUIRED, stride=None, weights="triangle", shift=(0, 0), per_call=None),
           "`tiles` (not in the reference): None, or dict(size=(h, w), stride=None, weights=\"triangle\", shift=(0, 0), "
           "per_call=None) in latent units - spatially tiled sampling of a latent larger than `size`, the size the model was "
           "trained at: the UNet denoises overlapping boxes of `size` (stride: default size // 2 per axis) and their outputs "
           "are blended ahead of the unchanged update (lvdm/models/samplers/tiles.py, DESIGN 4.16). Full runs only; beside "
           "`window_stride` the time axis is tiled as well.",
           (("--tile", dict(type=int, nargs=2, metavar=("HEIGHT", "WIDTH"), help="spatially tiled sampling: the tile size in "
                            "pixels (the size the model was trained at) for --height / --width larger than it; default off")),
            ("--tile_stride", dict(type=int, nargs=2, metavar=("SY", "SX"), help="tile stride in pixels (default half a tile)")),
            ("--tile_shift", dict(type=int, nargs=2, metavar=("DY", "DX"), help="pixels the interior tile seams move per step "
                                  "(default 0 0)"))),
           _tiles_from_flags),
)}


def all_options():
    """Every option of both tables, OPTIONS first."""
    return {**OPTIONS, **EXTENT_OPTIONS}


def of_kind(kind):
    return [o for o in OPTIONS.values() if o.kind == kind]


def check_keys(opt, cfg):
    """`cfg` is a dict with keys of the option's: the check every option shares, ahead of its own validation."""
    if not isinstance(cfg, dict):
        raise ValueError(f"{opt.name}= takes a dict with keys {list(opt.keys)} or None, got {type(cfg).__name__}")
    unknown = sorted(set(cfg) - set(opt.keys))
    if unknown:
        raise ValueError(f"{opt.name}=: unknown keys {unknown}; known: {list(opt.keys)}")


# ---------------------------------------------------------------------------------------------- model settings
@contextlib.contextmanager
def model_settings_scope(model, settings):
    """Run a block with the model settings of `settings` ({name: dict or None}, e.g. a call's kwargs: they are taken out of
    it, other names stay) on the UNet of `model` (a LatentDiffusion: its model.diffusion_model, or a UNetModel itself) and
    restore what was in force before, whatever happens inside. None changes nothing and calls no setter. A refused setting
    raises ValueError before the block is entered, with the settings made ahead of it put back. A run captured inside the
    block keeps the settings in its graph after the block ends."""
    net = getattr(getattr(model, "model", None), "diffusion_model", model)
    with contextlib.ExitStack() as restore:
        for opt in of_kind(MODEL_SETTING):
            cfg = settings.pop(opt.name, None)
            if cfg is None:
                continue
            check_keys(opt, cfg)
            setter = "set_" + opt.name                  # looked up on the instance at each call
            if not hasattr(net, setter):
                raise ValueError(f"{opt.name}=: {type(net).__name__} has no {opt.title} (expected the HIP UNetModel)")
            prev = getattr(net, setter)(dict(cfg))      # validates before anything runs
            restore.callback(lambda setter=setter, prev=prev: getattr(net, setter)(prev))
        yield


def takes_model_settings(fn):
    """Gives a sampler method every model-setting keyword (model_settings_scope on self.model around the whole call)."""
    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        with model_settings_scope(self.model, kwargs):
            return fn(self, *args, **kwargs)
    return wrapped


# ---------------------------------------------------------------------------------------------- harness functions
def fold(kwargs, **given):
    """Adds the option arguments that are not None to the `kwargs` a harness function passes on, and returns them. None is
    dropped, not forwarded: a callee that has no such option (`encode` and `apg=`) refuses the name itself."""
    kwargs.update({k: v for k, v in given.items() if v is not None})
    return kwargs


def documented(fn):
    """Appends every option's paragraph to the docstring of a function that takes them."""
    last = fn.__doc__.rstrip().split("\n")[-1]
    indent = last[:len(last) - len(last.lstrip())]          # a one-line docstring: none
    fn.__doc__ = "\n".join([fn.__doc__.rstrip()] + [indent + o.doc for o in all_options().values()])
    return fn


# ---------------------------------------------------------------------------------------------- command line
def add_option_arguments(parser):
    """Every option's flags. They appear in the namespace only when given (`from_args` reads them): without them a run's
    arguments are what they were."""
    for opt in all_options().values():
        for flag, kw in opt.flags:
            parser.add_argument(flag, default=argparse.SUPPRESS, **kw)


def from_args(name, args):
    """The flags of option `name` in a parsed namespace as its dict, or None."""
    opt = all_options()[name]
    given = {d: getattr(args, d) for d in (flag.lstrip("-") for flag, _ in opt.flags) if getattr(args, d, None) is not None}
    return opt.from_flags(**given) if given else None


def options_from_args(args):
    """{name: dict} of the options a parsed namespace gives."""
    out = {name: from_args(name, args) for name in all_options()}
    return {k: v for k, v in out.items() if v is not None}

"""First-frame-guided video editing on the fused path (not in the reference): start from the latent of a source clip
instead of pure noise, and denoise it under the conditioning of an edited first frame.

    video_guided_synthesis   source clip + edited first frame -> edited clip (DDIM inversion or SDEdit start, partial denoise)
    strength_steps           strength -> how many of the S steps run
    run_edit, get_parser, main   the command line (python -m dynamicrafter_amd.scripts.evaluation.edit)

With `invert=True` the source latent is taken up the schedule deterministically by `DDIMSampler.encode` (DDIM inversion,
the reference's TODO at lvdm/models/samplers/ddim.py:179) under the SOURCE clip's own first frame and prompt at guidance
scale 1, then `DDIMSampler.decode` brings it down again under the EDITED frame with the caller's guidance settings: the
motion is kept, the appearance follows the edit. With `invert=False` the start is `stochastic_encode` (SDEdit): the
source latent plus noise at the level where `decode` starts.
"""
import datetime
import os
import random
import time

import torch

from ...lvdm.models.samplers import options
from ...lvdm.models.samplers.dpm_solver import make_sampler
from . import inference as I
from .inference import build_conditioning, get_latent_z


def strength_steps(strength, ddim_steps):
    """n = max(1, min(S, round(strength * S))): how many of the S DDIM steps the edit inverts and denoises."""
    S = int(ddim_steps)
    if S < 1:
        raise ValueError(f"ddim_steps must be at least 1, got {ddim_steps}")
    return max(1, min(S, round(strength * S)))


_REFUSED = ("loop", "interp", "num_frames", "window_stride")


@torch.no_grad()
@options.documented
def video_guided_synthesis(model, prompts, videos, source, noise_shape, n_samples=1, ddim_steps=50, ddim_eta=0.0,
                           unconditional_guidance_scale=1.0, cfg_img=None, fs=None, text_input=False,
                           multiple_cond_cfg=False, timestep_spacing="uniform", guidance_rescale=0.0, strength=0.6,
                           invert=True, source_prompts=None, freeu=None, apg=None, token_downsampling=None,
                           tiles=None, **kwargs):
    """Returns [batch, n_samples, c, t, h, w] decoded frames. `videos` [b, 3, t, h, w] is what `load_data_prompts` gives for
    the EDITED first frame (that frame over all frames), `source` [b, 3, t, h, w] what `load_video_batch` gives for the
    clip to edit; the other arguments are `image_guided_synthesis`'s. n = strength_steps(strength, ddim_steps) steps run.

    In this order (each first-stage encode draws from the posterior, so the order fixes the result for a seed):
    the edited conditioning (`build_conditioning`), z = get_latent_z(model, source), then
      invert=True:  the source conditioning from source[:, :, :1] and `source_prompts` (default "") at guidance scale 1,
                    x = encode(z, cond_src, n, fs=fs) once for all samples;
      invert=False: per sample x = stochastic_encode(z, full(n - 1), noise) - index n - 1 is the level where
                    decode(t_start=n) starts; `noise=` injects the draw;
    then per sample decode(x, cond, n, ...) under the edited conditioning and decode_first_stage.
    `use_graph=` goes to encode and decode; every other keyword argument goes to `DDIMSampler.decode` (`noises`,
    `temperature`, `mask`, ...). `loop`, `interp`, `num_frames`, `window_stride` and a `sampler` other than "ddim" raise
    ValueError: their conditioning or solver has no defined inverse here.
    The model settings among the options below are in force for the inversion and the denoise alike, so that the denoise
    runs the model the inversion inverted; `apg` goes to the denoise (`DDIMSampler.decode`): the inversion runs at guidance
    scale 1 and has none. `tiles` goes to the denoise too, which takes it for a full run only (strength 1 without an
    inversion): a tiled inversion is not defined, and a partial run refuses tiles."""
    if tiles is not None and invert:
        raise ValueError("video_guided_synthesis: tiles with invert=True is not supported (a tiled inversion is not defined)")
    options.fold(kwargs, freeu=freeu, apg=apg, token_downsampling=token_downsampling, tiles=tiles)
    with options.model_settings_scope(model, kwargs):
        return _video_guided_synthesis(model, prompts, videos, source, noise_shape, n_samples, ddim_steps, ddim_eta,
                                       unconditional_guidance_scale, cfg_img, fs, text_input, multiple_cond_cfg,
                                       timestep_spacing, guidance_rescale, strength, invert, source_prompts, **kwargs)


def _video_guided_synthesis(model, prompts, videos, source, noise_shape, n_samples, ddim_steps, ddim_eta,
                            unconditional_guidance_scale, cfg_img, fs, text_input, multiple_cond_cfg, timestep_spacing,
                            guidance_rescale, strength, invert, source_prompts, **kwargs):
    for k in _REFUSED:
        if kwargs.get(k):
            raise ValueError(f"video_guided_synthesis: {k} = {kwargs[k]!r} is not supported (no inversion is defined "
                             f"for its conditioning)")
        kwargs.pop(k, None)
    name = kwargs.pop("sampler", None)
    if name not in (None, "ddim"):
        raise ValueError(f"video_guided_synthesis: sampler must be 'ddim', got {name!r} (a multistep solver has no "
                         f"inversion here)")
    n = strength_steps(strength, ddim_steps)
    if tuple(source.shape[:1]) + tuple(source.shape[2:3]) != (noise_shape[0], noise_shape[2]):
        raise ValueError(f"video_guided_synthesis: source {tuple(source.shape)} does not hold {noise_shape[0]} clips of "
                         f"{noise_shape[2]} frames")
    sampler = make_sampler(model, "ddim", multiple_cond_cfg)
    sampler.make_schedule(ddim_num_steps=ddim_steps, ddim_discretize=timestep_spacing, ddim_eta=ddim_eta, verbose=False)

    batch_size = noise_shape[0]
    fs = torch.tensor([fs] * batch_size, dtype=torch.long, device=model.device)
    if not text_input:
        prompts = [""] * batch_size
    use_graph = kwargs.pop("use_graph", False)
    noise = kwargs.pop("noise", None)

    cond, uc, uc_2 = build_conditioning(model, prompts, videos, unconditional_guidance_scale, cfg_img, multiple_cond_cfg)
    z = get_latent_z(model, source)
    if invert:
        src_prompts = [""] * batch_size if source_prompts is None else list(source_prompts)
        cond_src, _, _ = build_conditioning(model, src_prompts, source[:, :, :1], 1.0, num_frames=source.shape[2])
        x_inv, _ = sampler.encode(z, cond_src, n, fs=fs, use_graph=use_graph)

    batch_variants = []
    for _ in range(n_samples):
        if invert:
            x = x_inv
        else:
            t = torch.full((batch_size,), n - 1, dtype=torch.long, device=z.device)
            x = sampler.stochastic_encode(z, t, noise=noise)
        samples = sampler.decode(x, cond, n, unconditional_guidance_scale=unconditional_guidance_scale,
                                 unconditional_conditioning=uc, fs=fs, guidance_rescale=guidance_rescale, cfg_img=cfg_img,
                                 unconditional_conditioning_img_nonetext=uc_2, use_graph=use_graph, **kwargs)
        batch_variants.append(model.decode_first_stage(samples))
    return torch.stack(batch_variants).permute(1, 0, 2, 3, 4, 5)


# ---------------------------------------------------------------------------------------------- driver
def run_edit(args, gpu_num, gpu_no, device=None):
    """`inference.run_inference` for editing: the images of --prompt_dir are the EDITED first frames, and the source of
    <prompt_dir>/<stem>.<ext> is <source_dir>/<stem>.avi (Motion-JPEG, its first --video_length frames). Clips go to
    <savedir>/samples_separate through save_results_seperate as on the generate line; returns the paths written."""
    import yaml
    from ... import parallel
    from ...utils.save_video import save_results_seperate
    from ...utils.utils import instantiate_from_config
    from .funcs import load_video_batch
    if not args.source_dir:
        raise ValueError("--source_dir is required: the folder of the source clips (<stem>.avi)")
    device = torch.device("cuda", gpu_no if device is None else device)
    torch.cuda.set_device(device)
    # the inputs first: a missing source clip is reported before the checkpoint is read
    assert (args.height % 16 == 0) and (args.width % 16 == 0), "Error: image size [h,w] should be multiples of 16!"
    assert args.bs == 1, "Current implementation only support [batch size = 1]!"
    n_frames = args.video_length

    fakedir = os.path.join(args.savedir, "samples")
    os.makedirs(os.path.join(args.savedir, "samples_separate"), exist_ok=True)
    assert os.path.exists(args.prompt_dir), "Error: prompt file Not Found!"
    filename_list, data_list, prompt_list = I.load_data_prompts(args.prompt_dir, video_size=(args.height, args.width),
                                                                video_frames=n_frames, device=device)
    source_prompts = [""] * len(prompt_list)
    if args.source_prompt_file:
        source_prompts = I.load_prompts(args.source_prompt_file)
        if len(source_prompts) != len(prompt_list):
            raise ValueError(f"--source_prompt_file has {len(source_prompts)} prompts, the prompt folder {len(prompt_list)}")
    sources = [os.path.join(args.source_dir, os.path.splitext(name)[0] + ".avi") for name in filename_list]
    for path in sources:
        if not os.path.exists(path):
            raise FileNotFoundError(f"no source clip {path} for the edited frame of the same stem")
    with open(args.config) as f:
        config = yaml.safe_load(f)
    model_config = config.pop("model", {})
    model_config["params"]["unet_config"]["params"]["use_checkpoint"] = False
    model = instantiate_from_config(model_config)
    model = model.to(device)
    model.perframe_ae = args.perframe_ae
    assert os.path.exists(args.ckpt_path), "Error: checkpoint Not Found!"
    model = I.load_model_checkpoint(model, args.ckpt_path)
    model.eval()

    h, w = args.height // 8, args.width // 8
    noise_shape = [args.bs, model.model.diffusion_model.out_channels, n_frames, h, w]
    indices = parallel.shard_indices(len(prompt_list), gpu_num, gpu_no)
    print("Edits [rank:%d] %d/%d samples loaded." % (gpu_no, len(indices), len(prompt_list)))

    extra = {k: getattr(args, k) for k in ("sampler", "num_frames", "window_stride", "loop", "interp")}
    extra.update(options.options_from_args(args))
    save_kw = dict(container=args.container, quality=args.quality)
    written = []
    start = time.time()
    with torch.no_grad():
        for i in indices:
            videos = data_list[i][None].to(device)
            source = load_video_batch([sources[i]], 1, video_size=(args.height, args.width), video_frames=n_frames,
                                      device=device)
            batch = video_guided_synthesis(model, [prompt_list[i]], videos, source, noise_shape, args.n_samples,
                                           args.ddim_steps, args.ddim_eta, args.unconditional_guidance_scale, args.cfg_img,
                                           args.frame_stride, args.text_input, args.multiple_cond_cfg,
                                           args.timestep_spacing, args.guidance_rescale, strength=args.strength,
                                           invert=not args.no_invert, source_prompts=[source_prompts[i]], **extra)
            written += save_results_seperate(prompt_list[i], batch[0], filename_list[i], fakedir, fps=8, **save_kw)
    print(f"Saved in {args.savedir}. Time used: {(time.time() - start):.2f} seconds")
    return written


def get_parser():
    """The generate line's flags (`inference.get_parser()`, a fresh parser each call) plus the edit's own. --ddim_eta
    defaults to 0 here: a deterministic denoise is what an inversion inverts."""
    parser = I.get_parser()
    parser.add_argument("--source_dir", type=str, default=None, help="folder of the source clips: <stem>.avi (Motion-JPEG) "
                        "for every <stem>.png / .jpg of --prompt_dir")
    parser.add_argument("--strength", type=float, default=0.6, help="share of the DDIM steps that is inverted and denoised")
    parser.add_argument("--no_invert", action="store_true", default=False, help="start from the source latent plus noise "
                        "(SDEdit) instead of its DDIM inversion")
    parser.add_argument("--source_prompt_file", type=str, default=None, help="one prompt per source clip for the inversion "
                        "(default: the empty prompt)")
    parser.set_defaults(ddim_eta=0.0)
    return parser


def main(argv=None):
    """Rank and device from WORLD_SIZE / RANK / LOCAL_RANK as `inference.main`."""
    print("@DynamiCrafter edit: %s" % datetime.datetime.now().strftime("%Y-%m-%d-%H-%M-%S"))
    args = get_parser().parse_args(argv)
    seed = args.seed
    if seed < 0:
        seed = random.randint(0, 2 ** 31)
    I.seed_everything(seed)
    gpu_num, rank = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0))
    return run_edit(args, gpu_num, rank, device=int(os.environ.get("LOCAL_RANK", rank)))


if __name__ == "__main__":
    main()

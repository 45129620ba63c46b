"""The programmatic entry points on the GPU: scripts.evaluation.funcs (batch_ddim_sampling, load_image_batch, save_videos), the
two Image2Video classes and DynamiCrafterImg2VideoPipeline, on the tiny model of the existing tests (tests/golden_cfg.py
stand-ins for the CLIP towers, the seeded weight recipe), 4 DDIM steps (the "uniform" spacing of the reference takes steps
that divide 1000: 3 would index timestep 1000), 64 x 64 frames (the smallest the tiny nets admit) and
4 latent frames. What is compared is this package against itself assembled by hand (torch.equal) and the float resize against
torch on the CPU (tests/resize_f32_restatement.TOL); the sampler and the networks have their own parity tests."""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import jpeg_restatement as J
from tests import resize_f32_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS, T_MODEL, SIZE = 4, 4, 64


def _tiny_model(cname):
    """As test_image_guided_synthesis_vs_reference builds it."""
    from dynamicrafter_amd.utils.utils import instantiate_from_config
    from oracle.weights import fill_state_dict
    from tests.golden_cfg import TINY_AE, TINY_RESAMPLER, TINY_UNET
    root = os.path.join(os.path.dirname(__file__), "..", "dynamicrafter_amd", "configs")
    cfg = yaml.safe_load(open(os.path.join(root, cname)))
    p = cfg["model"]["params"]
    extra = dict(image_cross_attention_scale_learnable=True) if "256" in cname else {}
    p["unet_config"]["params"] = dict(TINY_UNET, default_fs=p["unet_config"]["params"]["default_fs"], **extra)
    p["first_stage_config"]["params"]["ddconfig"] = dict(TINY_AE)
    p["cond_stage_config"] = {"target": "tests.golden_cfg.ToyTextEmbedder"}
    p["img_cond_stage_config"] = {"target": "tests.golden_cfg.ToyImageEmbedder"}
    p["image_proj_stage_config"] = {"target": "lvdm.modules.encoders.resampler.Resampler", "params": dict(TINY_RESAMPLER)}
    model = instantiate_from_config(cfg["model"])
    for mod, seed in ((model.model.diffusion_model, 11), (model.first_stage_model, 13), (model.image_proj_model, 14)):
        sd = mod.state_dict()
        mod.load_state_dict(fill_state_dict({k: tuple(v.shape) for k, v in sd.items()}, seed), strict=True)
    return model.to(DEV).eval()


@pytest.fixture(scope="module")
def models():
    return {c: _tiny_model(f"inference_{c}_v1.0.yaml") for c in ("512", "256")}


@pytest.fixture(scope="module")
def photo():
    """A non-square uint8 image, 90 x 70."""
    a = np.random.default_rng(2).integers(0, 256, size=(90, 70, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


def _normalised(image):
    return (torch.from_numpy(np.array(image)).permute(2, 0, 1).float() / 255. - 0.5) * 2


def _resize_center_crop_cpu(image, video_size):
    """torch on the CPU: Resize(min(video_size)) -> CenterCrop(video_size) of the normalised image."""
    from dynamicrafter_amd.scripts.evaluation.inference import resize_geometry
    g = resize_geometry(image.shape[0], image.shape[1], video_size)
    return R.torch_reference(_normalised(image).numpy(), (g.rh, g.rw), tuple(video_size), (g.top - g.pad_top, g.left - g.pad_left))


def _avi_frames(path):
    return J.walk_avi(open(path, "rb").read())["frames"]


# ------------------------------------------------------------------------------------------------ funcs.batch_ddim_sampling
@pytest.mark.parametrize("cname,width,spacing,rescale", [("512", 8, "uniform_trailing", 0.7), ("256", 32, "uniform", 0.0)])
def test_batch_ddim_sampling_equals_the_sampler_called_by_hand(models, monkeypatch, cname, width, spacing, rescale):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.scripts.evaluation import funcs
    model = models[cname]
    b, t, h = 1, T_MODEL, 8
    g = torch.Generator().manual_seed(3)
    x_T = torch.randn(b, 4, t, h, width, generator=g).to(DEV)
    noises = torch.randn(STEPS, b, 4, t, h, width, generator=g).to(DEV)
    cc = (torch.randn(b, 4, t, h, width, generator=g) * 0.2).to(DEV)
    img = (torch.rand(b, 3, 40, 40, generator=g) * 2 - 1).to(DEV)
    cond_emb = torch.cat([model.get_learned_conditioning(["a corgi"]), model.image_proj_model(model.embedder(img))], dim=1)
    fs = torch.tensor([24], dtype=torch.long, device=DEV)
    cond = {"c_crossattn": [cond_emb], "c_concat": [cc], "fs": fs}

    seen = []
    real = DDIMSampler.sample

    def spy(self, *a, **k):
        seen.append(k)
        return real(self, *a, **k)
    monkeypatch.setattr(DDIMSampler, "sample", spy)
    out = funcs.batch_ddim_sampling(model, cond, [b, 4, t, h, width], n_samples=2, ddim_steps=STEPS, ddim_eta=1.0, cfg_scale=7.5,
                                    temporal_cfg_scale=3.0, x_T=x_T, noises=noises)
    monkeypatch.setattr(DDIMSampler, "sample", real)
    assert "fs" not in cond and sorted(cond) == ["c_concat", "c_crossattn"]
    assert tuple(out.shape) == (b, 2, 3, t, 8 * h, 8 * width) and torch.isfinite(out).all()
    assert torch.equal(out[:, 0], out[:, 1])                                  # the same x_T and noises for every sample
    assert len(seen) == 2
    for k in seen:
        assert k["timestep_spacing"] == spacing and k["guidance_rescale"] == rescale and k["clean_cond"] is True
        assert "temporal_length" not in k and "conditional_guidance_scale_temporal" not in k
        assert k["x_T"] is x_T and k["noises"] is noises and k["fs"] is fs
        assert k["unconditional_conditioning"]["c_concat"][0] is cc           # shared, not copied

    uc_img = model.image_proj_model(model.embedder(torch.zeros(b, 3, 224, 224, device=DEV)))
    uc = {"c_crossattn": [torch.cat([model.get_learned_conditioning([""]), uc_img], dim=1)], "c_concat": [cc]}
    samples, _ = DDIMSampler(model).sample(S=STEPS, conditioning={"c_crossattn": [cond_emb], "c_concat": [cc]}, batch_size=b,
                                           shape=(4, t, h, width), verbose=False, unconditional_guidance_scale=7.5,
                                           unconditional_conditioning=uc, eta=1.0, x_T=x_T, fs=fs, timestep_spacing=spacing,
                                           guidance_rescale=rescale, noises=noises, clean_cond=True)
    assert torch.equal(out[:, 0], model.decode_first_stage(samples))
    # without guidance there is no unconditional branch
    cond["fs"] = fs
    seen.clear()
    monkeypatch.setattr(DDIMSampler, "sample", spy)
    funcs.batch_ddim_sampling(model, cond, [b, 4, t, h, width], ddim_steps=STEPS, cfg_scale=1.0, x_T=x_T, noises=noises)
    assert seen[0]["unconditional_conditioning"] is None


# ------------------------------------------------------------------------------------------------ Image2Video
class _Capture:
    """Wraps get_latent_z and batch_ddim_sampling of scripts.gradio.i2v_test and the model's embedder."""

    def __init__(self, monkeypatch, model):
        from dynamicrafter_amd.scripts.gradio import i2v_test
        self.videos, self.z, self.cond, self.embedded = [], [], [], []
        real_z, real_s = i2v_test.get_latent_z, i2v_test.batch_ddim_sampling

        def get_latent_z(m, videos):
            self.videos.append(videos.clone())
            self.z.append(real_z(m, videos))
            return self.z[-1]

        def batch_ddim_sampling(m, cond, noise_shape, **kw):
            self.cond.append({k: (v[0].clone() if isinstance(v, list) else v.clone()) for k, v in cond.items()})
            self.noise_shape = list(noise_shape)
            self.kw = dict(kw)
            return real_s(m, cond, noise_shape, **kw)
        monkeypatch.setattr(i2v_test, "get_latent_z", get_latent_z)
        monkeypatch.setattr(i2v_test, "batch_ddim_sampling", batch_ddim_sampling)
        self.hook = model.embedder.register_forward_hook(lambda mod, inp, out: self.embedded.append(inp[0].clone()))


def test_i2v_test_get_image(models, photo, monkeypatch, tmp_path):
    from dynamicrafter_amd.scripts.gradio.i2v_test import Image2Video
    model = models["512"]
    cap = _Capture(monkeypatch, model)
    try:
        i2v = Image2Video(str(tmp_path / "a"), resolution=f"{SIZE}_{SIZE}", model=model)
        path = i2v.get_image(np.array(photo), "a corgi/running fast", steps=STEPS, cfg_scale=7.5, eta=1.0, fs=24, seed=7)
        again = Image2Video(str(tmp_path / "b"), resolution=f"{SIZE}_{SIZE}", model=model).get_image(
            np.array(photo), "a corgi/running fast", steps=STEPS, cfg_scale=7.5, eta=1.0, fs=24, seed=7)
    finally:
        cap.hook.remove()
    assert path == str(tmp_path / "a" / "a_corgi_slash_running_fast.avi") and os.path.exists(path)
    frames = _avi_frames(path)
    assert len(frames) == T_MODEL
    assert open(path, "rb").read() == open(again, "rb").read()               # the same seed, the same bytes
    # the resized image: torch's Resize + CenterCrop on the CPU (90 x 70 -> 82 x 64 -> rows 9 .. 72)
    videos = cap.videos[0]
    assert tuple(videos.shape) == (1, 3, 1, SIZE, SIZE)
    err = float(np.abs(videos[0, :, 0].cpu().numpy() - _resize_center_crop_cpu(photo, (SIZE, SIZE))).max())
    print(f"get_image: resized image vs torch CPU max abs error {err:.3g}")
    assert err <= R.TOL
    # c_concat: its latent on every frame
    cc = cap.cond[0]["c_concat"]
    assert tuple(cc.shape) == (1, 4, T_MODEL, SIZE // 8, SIZE // 8) and cap.noise_shape == list(cc.shape)
    for t in range(T_MODEL):
        assert torch.equal(cc[:, :, t], cap.z[0][:, :, 0])
    assert cap.cond[0]["fs"].tolist() == [24] and cap.kw["ddim_steps"] == STEPS and cap.kw["cfg_scale"] == 7.5
    # the embedder saw the unresized image
    assert tuple(cap.embedded[0].shape) == (1, 3, 90, 70)
    assert float((cap.embedded[0][0].cpu() - _normalised(photo)).abs().max()) <= 1.2e-7
    # steps are capped at 60 (a stub in place of the sampling: 60 steps are not run here)
    from dynamicrafter_amd.scripts.gradio import i2v_test
    asked = []

    def stub(m, cond, noise_shape, **kw):
        asked.append(kw["ddim_steps"])
        return torch.zeros(1, 1, 3, T_MODEL, SIZE, SIZE, device=DEV)
    monkeypatch.setattr(i2v_test, "batch_ddim_sampling", stub)
    assert i2v.get_image(np.array(photo), "", steps=100) == str(tmp_path / "a" / "empty_prompt.avi") and asked == [60]


def test_i2v_test_application_loop_and_interpolation(models, photo, monkeypatch, tmp_path):
    from dynamicrafter_amd.scripts.gradio.i2v_test_application import Image2Video
    model = models["512"]
    photo2 = np.ascontiguousarray(photo[::-1, :, ::-1][:80])                 # another image, another size: 80 x 70
    cap = _Capture(monkeypatch, model)
    try:
        i2v = Image2Video(str(tmp_path), resolution=f"{SIZE}_{SIZE}", model=model)
        x_T = torch.randn(1, 4, T_MODEL, SIZE // 8, SIZE // 8, generator=torch.Generator().manual_seed(1)).to(DEV)
        loop = i2v.get_image(np.array(photo), "loop", steps=STEPS, fs=24, seed=7, x_T=x_T)
        interp = i2v.get_image(np.array(photo), "interp", steps=STEPS, fs=24, seed=7, image2=photo2)
    finally:
        cap.hook.remove()
    assert cap.kw == dict(n_samples=1, ddim_steps=STEPS, ddim_eta=1.0, cfg_scale=7.5) and len(cap.cond) == 2
    # a loop: zeros except the first and the last frame, both the image's latent; the repeated last frame is dropped
    cc, z = cap.cond[0]["c_concat"], cap.z[0]
    assert len(cap.z) == 3 and tuple(cc.shape) == (1, 4, T_MODEL, SIZE // 8, SIZE // 8)
    assert torch.equal(cc[:, :, 0], z[:, :, 0]) and torch.equal(cc[:, :, -1], z[:, :, 0]) and (cc[:, :, 1:-1] == 0).all()
    assert z.abs().max() > 0
    assert loop == str(tmp_path / "loop.avi") and len(_avi_frames(loop)) == T_MODEL - 1
    # interpolation: the last frame is the second image's latent, all frames are kept
    cc, z, z2 = cap.cond[1]["c_concat"], cap.z[1], cap.z[2]
    assert torch.equal(cc[:, :, 0], z[:, :, 0]) and torch.equal(cc[:, :, -1], z2[:, :, 0]) and (cc[:, :, 1:-1] == 0).all()
    assert not torch.equal(z, z2)
    err = float(np.abs(cap.videos[2][0, :, 0].cpu().numpy() - _resize_center_crop_cpu(photo2, (SIZE, SIZE))).max())
    assert err <= R.TOL
    assert interp == str(tmp_path / "interp.avi") and len(_avi_frames(interp)) == T_MODEL


# ------------------------------------------------------------------------------------------------ the pipeline
class _Seeded:
    """The pipeline behind a fixed global seed: the AE's posterior sample of the image latent draws from torch's global CPU
    generator (as in the reference), whatever `generator=` / `latents=` say, so every call here starts from the same state."""

    def __init__(self, pipe):
        self._pipe = pipe

    def __call__(self, *a, **k):
        torch.manual_seed(0)
        return self._pipe(*a, **k)

    def __getattr__(self, name):
        return getattr(self._pipe, name)


@pytest.fixture(scope="module")
def pipe(models):
    from dynamicrafter_amd.scripts.gradio.dynamicrafter_pipeline import DynamiCrafterImg2VideoPipeline
    return _Seeded(DynamiCrafterImg2VideoPipeline(f"{SIZE}_{SIZE}", model=models["512"]))


def _latents(seed, w=SIZE // 8):
    return torch.randn(1, 4, T_MODEL, SIZE // 8, w, generator=torch.Generator().manual_seed(seed))


def test_pipeline_latents_and_generator_are_honoured(pipe, photo):
    kw = dict(num_inference_steps=STEPS, guidance_scale=7.5, eta=0.0, frame_stride=24, return_dict=False)
    a = pipe(photo, "a corgi", latents=_latents(1), **kw)
    assert isinstance(a, torch.Tensor) and a.device == torch.device(DEV) and tuple(a.shape) == (1, 3, T_MODEL, SIZE, SIZE)
    assert torch.equal(a, pipe(photo, "a corgi", latents=_latents(1), **kw))
    assert not torch.equal(a, pipe(photo, "a corgi", latents=_latents(2), **kw))
    g = pipe(photo, "a corgi", generator=torch.Generator().manual_seed(5), **kw)
    assert torch.equal(g, pipe(photo, "a corgi", generator=torch.Generator().manual_seed(5), **kw))
    assert not torch.equal(g, pipe(photo, "a corgi", generator=torch.Generator().manual_seed(6), **kw))
    # a generator draws what torch.randn draws from it: the same clip as passing those latents
    x = torch.randn(1, 4, T_MODEL, SIZE // 8, SIZE // 8, generator=torch.Generator().manual_seed(5))
    assert torch.equal(g, pipe(photo, "a corgi", latents=x, **kw))
    with pytest.raises(ValueError):
        pipe(photo, "a corgi", latents=_latents(1, w=4), **kw)


def test_pipeline_negative_prompt(pipe, photo):
    kw = dict(num_inference_steps=STEPS, eta=0.0, frame_stride=24, return_dict=False, latents=_latents(1))
    assert not torch.equal(pipe(photo, "a corgi", negative_prompt="x", guidance_scale=7.5, **kw),
                           pipe(photo, "a corgi", negative_prompt=None, guidance_scale=7.5, **kw))
    assert torch.equal(pipe(photo, "a corgi", negative_prompt="x", guidance_scale=1.0, **kw),
                       pipe(photo, "a corgi", negative_prompt=None, guidance_scale=1.0, **kw))
    with pytest.raises(ValueError):
        pipe(photo, ["a", "b"], negative_prompt=["x"], guidance_scale=7.5, **dict(kw, latents=None))


def test_pipeline_output_types_batch_and_callback(pipe, photo, tmp_path):
    from PIL import Image
    kw = dict(num_inference_steps=STEPS, guidance_scale=7.5, eta=0.0, frame_stride=24, latents=_latents(1))
    t = pipe(photo, "a corgi", **kw)
    assert isinstance(t, dict) and list(t) == ["videos"] and isinstance(t["videos"], torch.Tensor)
    n = pipe(Image.fromarray(np.array(photo)), "a corgi", output_type="numpy", **kw)["videos"]
    assert isinstance(n, np.ndarray) and n.dtype == np.float32 and n.shape == (1, 3, T_MODEL, SIZE, SIZE)
    assert np.array_equal(n, t["videos"].cpu().numpy())                       # a PIL image is the same input as its array
    p = pipe(photo, "a corgi", output_type="pil", return_dict=False, **kw)
    assert len(p) == 1 and len(p[0]) == T_MODEL and all(isinstance(f, Image.Image) and f.size == (SIZE, SIZE) for f in p[0])
    u8 = ((t["videos"][0, :, 0].clamp(-1, 1) + 1) / 2 * 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    assert np.abs(np.asarray(p[0][0]).astype(int) - u8.astype(int)).max() <= 1
    with pytest.raises(ValueError):
        pipe(photo, "a corgi", output_type="mp4", **kw)
    # two prompts, one image: its conditioning is repeated over the batch
    calls = []
    two = pipe(photo, ["a corgi", "a cat"], generator=torch.Generator().manual_seed(5), output_type="tensor", return_dict=False,
               callback=lambda i, ts, lat: calls.append((i, ts)), callback_steps=2, **dict(kw, latents=None))
    assert tuple(two.shape) == (2, 3, T_MODEL, SIZE, SIZE) and not torch.equal(two[0], two[1])
    assert [i for i, _ in calls] == [0, 2] and calls[0][1] > calls[1][1]
    # the no-op switches, and save_video
    assert pipe.enable_attention_slicing() is None and pipe.disable_attention_slicing() is None
    assert pipe.enable_xformers_memory_efficient_attention() is None and pipe.to(DEV) is pipe._pipe
    path = pipe.save_video(t["videos"], str(tmp_path / "clips" / "out.mp4"))
    assert path == str(tmp_path / "clips" / "out.avi") and len(_avi_frames(path)) == T_MODEL


def test_pipeline_height_and_width_resize_exactly(pipe, photo):
    """height / width of another aspect than the image's: an exact Resize((h, w)), no crop, no padding."""
    got = pipe._preprocess_image(photo, 64, 128)
    assert tuple(got.shape) == (3, 64, 128) and got.device == torch.device(DEV)
    ref = R.torch_reference(_normalised(photo).numpy(), (64, 128))
    assert float(np.abs(got.cpu().numpy() - ref).max()) <= R.TOL
    crop = pipe._preprocess_image(torch.from_numpy(np.array(photo)).permute(2, 0, 1))          # a uint8-valued tensor
    assert float(np.abs(crop.cpu().numpy() - _resize_center_crop_cpu(photo, (SIZE, SIZE))).max()) <= R.TOL
    out = pipe(photo, "a corgi", height=64, width=128, num_inference_steps=STEPS, guidance_scale=7.5, frame_stride=24,
               latents=_latents(1, w=16), return_dict=False)
    assert tuple(out.shape) == (1, 3, T_MODEL, 64, 128) and torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------ funcs.load_image_batch / save_videos
def test_load_image_batch_and_save_videos(tmp_path):
    from PIL import Image
    from dynamicrafter_amd.scripts.evaluation import funcs
    rng = np.random.default_rng(4)
    paths, pixels = [], []
    for name, hw in (("one.png", (40, 72)), ("two.png", (90, 61))):
        pixels.append(rng.integers(0, 256, size=hw + (3,), dtype=np.uint8))
        Image.fromarray(pixels[-1]).save(str(tmp_path / name))
        paths.append(str(tmp_path / name))
    batch = funcs.load_image_batch(paths, (32, 48))
    assert tuple(batch.shape) == (2, 3, 32, 48) and batch.dtype == torch.float32 and batch.device == torch.device(DEV)
    for got, px in zip(batch.cpu(), pixels):
        x = torch.from_numpy(px).permute(2, 0, 1).float()[None]
        ref = torch.nn.functional.interpolate(x, size=(32, 48), mode="bilinear", align_corners=False, antialias=False)[0]
        ref = (ref / 255. - 0.5) * 2
        err = float((got - ref).abs().max())
        print(f"load_image_batch: max abs error vs torch CPU {err:.3g}")
        assert err <= R.TOL
    with pytest.raises(NotImplementedError):
        funcs.load_image_batch([str(tmp_path / "clip.mp4")], (32, 48))
    with pytest.raises(NotImplementedError):
        funcs.load_image_batch([str(tmp_path / "x.bmp")], (32, 48))
    # save_videos: n_samples side by side, one file per batch entry, the extension of the container
    clips = torch.rand(2, 2, 3, 3, 16, 32, generator=torch.Generator().manual_seed(0)).to(DEV) * 2 - 1
    out = funcs.save_videos(clips, str(tmp_path / "v"), ["first", "second"], fps=8)
    assert out == [str(tmp_path / "v" / "first.avi"), str(tmp_path / "v" / "second.avi")]
    for p in out:
        fr = _avi_frames(p)
        im = Image.open(__import__("io").BytesIO(fr[0]))
        assert len(fr) == 3 and im.size == (64, 16)
    assert funcs.save_videos(clips[:1], str(tmp_path / "v"), ["g"], container="gif") == [str(tmp_path / "v" / "g.gif")]

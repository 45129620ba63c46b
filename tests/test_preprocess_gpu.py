"""The input side of the harness on the GPU: the dc_prep_* launches against Pillow's own resize (equality in every pixel; the
plain-numpy restatement that explains the arithmetic is tests/preprocess_restatement.py, held to Pillow by
tests/test_preprocess_cpu.py), the launches inside a captured graph, load_data_prompts on a folder of files, and run_inference
end to end on the tiny model of the existing tests.

Images (np.random.default_rng(1) per case): uniform noise, a smooth ramp plus a checkerboard, all 0, all 255."""
import functools
import io
import os

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

from tests import jpeg_restatement as J
from tests import preprocess_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ["noise", "ramp", "zeros", "ones"]
FLOAT_TOL = 1.2e-7          # one fp32 ulp at 1.0: the room an equivalent formula such as u8 * (2 / 255) - 1 needs
SENT_F, SENT_B = -7777.0, 0xA5
# ((h, w), video_size). The first five give the resizes 37x53 -> 16x22, none, 9x7 -> 30x24 (padded to 32), 301x200 -> 48x32 and
# 64x100 -> 32x50; then a crop of both passes' output, padding and crop together, the two directions of round-half-even, and a
# crop without any resize.
CASES = [((37, 53), (16, 22)), ((16, 16), (16, 16)), ((9, 7), (32, 24)), ((301, 200), (48, 32)), ((64, 100), (32, 50)),
         ((37, 53), (16, 16)), ((301, 200), (32, 48)), ((16, 21), (16, 16)), ((16, 23), (16, 16)), ((16, 40), (16, 16))]
_ids = lambda c: f"{c[0][0]}x{c[0][1]}to{c[1][0]}x{c[1][1]}"


def _pillow_resize(a, oh, ow):
    return np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR))


@functools.lru_cache(maxsize=None)
def _image(kind, hw):
    a = R.make_image(kind, hw[0], hw[1], np.random.default_rng(1))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _expected_u8(kind, hw, vs):
    """Pillow's resize + torchvision's crop / pad: uint8 [ch, cw, 3]."""
    e = R.transform_u8(np.array(_image(kind, hw)), vs, resize_fn=_pillow_resize)
    e.setflags(write=False)
    return e


def _expected_float(u8):
    """torch's CPU ToTensor + Normalize on uint8 [h, w, 3] -> fp32 [3, h, w]."""
    v = torch.from_numpy(np.array(u8)).permute(2, 0, 1).to(torch.float32).div(255)
    return v.sub(0.5).div(0.5)


def _check_frame(frame, u8, what):
    """frame fp32 [3, h, w] (CPU) against the expected uint8 picture: every pixel equal, floats within FLOAT_TOL."""
    got = torch.round((frame.double() + 1.0) * 127.5).to(torch.int64).permute(1, 2, 0).numpy()
    bad = int((got != u8.astype(np.int64)).sum())
    err = float((frame - _expected_float(u8)).abs().max())
    print(f"{what}: {bad} of {u8.size} bytes differ from Pillow, max float error {err:.3g}")
    assert bad == 0, what
    assert err <= FLOAT_TOL, what


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_preprocess_image_equals_pillow_in_every_pixel(case):
    from dynamicrafter_amd.scripts.evaluation.inference import preprocess_image, resize_geometry
    hw, vs = case
    g, r = resize_geometry(hw[0], hw[1], vs), R.geometry(hw[0], hw[1], vs)
    assert (g.rh, g.rw) == (r["rh"], r["rw"])
    for kind in KINDS:
        a = np.array(_image(kind, hw))
        exp = _expected_u8(kind, hw, vs)
        for T in (1, 3):
            src = torch.from_numpy(a).to(DEV) if T == 1 else a          # a device tensor and an ndarray
            out = preprocess_image(src, vs, T)
            assert out.shape == (3, T) + tuple(vs) and out.dtype == torch.float32 and out.device == torch.device(DEV)
            o = out.cpu()
            for t in range(T):
                _check_frame(o[:, t], exp, f"{kind} {_ids(case)} T{T} frame {t}")


@pytest.mark.parametrize("axis", [1, 2], ids=["horizontal_40x40to40x17", "vertical_40x40to17x40"])
def test_single_pass_at_abi_level(axis):
    """One launch of dc_prep_finish with the pass of one axis, the crop being the whole resized image."""
    from dynamicrafter_amd import ops
    oh, ow = (40, 17) if axis == 1 else (17, 40)
    tab = ops.ResizeTables(40, 17, DEV)
    for kind in KINDS:
        a = np.array(_image(kind, (40, 40)))
        buf = torch.full((3 * 2 * oh * ow + 64,), SENT_F, dtype=torch.float32, device=DEV)
        clip = buf[:3 * 2 * oh * ow].view(3, 2, oh, ow)
        ops.prep_finish(torch.from_numpy(a).to(DEV), clip, tab, axis=axis, src_hw=(40, 40), origin=(0, 0), resized=(oh, ow),
                        offset=(0, 0), t0=0, nt=2)
        torch.cuda.synchronize()
        b = buf.cpu()
        assert (b[3 * 2 * oh * ow:] == SENT_F).all(), "dc_prep_finish wrote past the clip"
        exp = _pillow_resize(a, oh, ow)
        for t in range(2):
            _check_frame(b[:3 * 2 * oh * ow].view(3, 2, oh, ow)[:, t], exp, f"{kind} axis {axis} frame {t}")
    with pytest.raises(ValueError):          # tables of the other size
        ops.prep_finish(torch.zeros(40, 40, 3, dtype=torch.uint8, device=DEV), clip, ops.ResizeTables(40, 16, DEV), axis=axis,
                        src_hw=(40, 40), origin=(0, 0), resized=(oh, ow), offset=(0, 0), t0=0, nt=2)


def test_interp_halves_and_sentinels():
    """Two different images into the two halves of a 4-frame clip through preprocess_launch with a caller's workspace: bytes
    behind the workspace, floats behind the clip and the frames outside t0 .. t0 + nt - 1 stay as they were."""
    from dynamicrafter_amd.scripts.evaluation import inference as I
    vs, T = (16, 16), 4
    n = 3 * T * 16 * 16
    buf = torch.full((n + 64,), SENT_F, dtype=torch.float32, device=DEV)
    clip = buf[:n].view(3, T, 16, 16)
    imgs = [("noise", (37, 53)), ("ramp", (301, 200))]
    for i, (kind, hw) in enumerate(imgs):
        plan = I.preprocess_plan(hw[0], hw[1], vs, DEV)
        assert plan.two_pass and plan.workspace_bytes > 0
        ws = torch.full((plan.workspace_bytes + 64,), SENT_B, dtype=torch.uint8, device=DEV)
        I.preprocess_launch(plan, torch.from_numpy(np.array(_image(kind, hw))).to(DEV), clip, ws, 2 * i, 2)
        torch.cuda.synchronize()
        assert (ws[plan.workspace_bytes:] == SENT_B).all(), "dc_prep_resize_h wrote past the workspace"
        with pytest.raises(ValueError):
            I.preprocess_launch(plan, torch.from_numpy(np.array(_image(kind, hw))).to(DEV), clip, ws[:plan.workspace_bytes - 1], 0, 2)
        b = buf.cpu()
        assert (b[n:] == SENT_F).all(), "dc_prep_finish wrote past the clip"
        if i == 0:
            assert (b[:n].view(3, T, 16, 16)[:, 2:] == SENT_F).all(), "frames outside t0 .. t0 + nt - 1 were written"
    o = buf[:n].view(3, T, 16, 16).cpu()
    for t in range(T):
        kind, hw = imgs[t // 2]
        _check_frame(o[:, t], _expected_u8(kind, hw, vs), f"interp frame {t}")
    # the same through preprocess_image's out / t0 / nt
    out = torch.full((3, T, 16, 16), SENT_F, dtype=torch.float32, device=DEV)
    I.preprocess_image(np.array(_image(*imgs[1])), vs, T, out=out, t0=2, nt=2)
    assert (out[:, :2] == SENT_F).all() and torch.equal(out[:, 2:].cpu(), o[:, 2:])
    with pytest.raises(RuntimeError):
        I.preprocess_image(torch.zeros(8, 8, 3, dtype=torch.uint8), vs, T)


def test_launches_replay_from_a_captured_graph():
    """Neither entry allocates or synchronises: captured once, the replay on a new source gives what eager launches give."""
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.scripts.evaluation import inference as I
    hw, vs, T = (37, 53), (16, 16), 2
    plan = I.preprocess_plan(hw[0], hw[1], vs, DEV)
    src = torch.from_numpy(np.array(_image("ramp", hw))).to(DEV)
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=DEV)
    out = torch.zeros((3, T) + vs, dtype=torch.float32, device=DEV)
    enqueue = lambda: I.preprocess_launch(plan, src, out, ws, 0, T)
    enqueue()
    torch.cuda.synchronize()
    eager_ramp = out.clone()
    graph = ops.DeviceGraph().capture(enqueue)
    src.copy_(torch.from_numpy(np.array(_image("noise", hw))).to(DEV))
    out.zero_()
    torch.cuda.synchronize()
    graph.launch()
    graph.sync()
    replay_noise = out.clone()
    out.zero_()
    enqueue()
    torch.cuda.synchronize()
    assert torch.equal(replay_noise, out) and not torch.equal(replay_noise, eager_ramp)
    _check_frame(replay_noise[:, 1].cpu(), _expected_u8("noise", hw, vs), "graph replay")


def _write_folder(d, sizes, prompts, fmts=("png", "jpg", "png")):
    """Images named so that they sort in the order given; -> [(name, decoded uint8 pixels)]"""
    rng = np.random.default_rng(1)
    os.makedirs(d, exist_ok=True)
    files = []
    for i, (hw, fmt) in enumerate(zip(sizes, fmts)):
        name = f"img_{i:02d}_{'abc'[i]}.{fmt}"
        Image.fromarray(R.make_image("ramp" if i % 2 else "noise", hw[0], hw[1], rng)).save(os.path.join(d, name), quality=95)
        files.append((name, np.asarray(Image.open(os.path.join(d, name)).convert("RGB"))))
    with open(os.path.join(d, "prompts.txt"), "w") as f:
        f.write("\n".join(prompts) + "\n")
    return files


def test_load_data_prompts(tmp_path):
    from dynamicrafter_amd.scripts.evaluation import inference as I
    prompts = ["a boat at sea", "a cat, sleeping", "fireworks"]
    files = _write_folder(str(tmp_path), [(40, 72), (90, 61), (33, 33)], prompts)
    names, data, got_prompts = I.load_data_prompts(str(tmp_path), video_size=(32, 48), video_frames=3, device=DEV)
    assert names == [n for n, _ in files] and got_prompts == prompts and len(data) == 3
    for clip, (name, pixels) in zip(data, files):
        assert clip.shape == (3, 3, 32, 48) and clip.dtype == torch.float32 and clip.device == torch.device(DEV)
        ref = I.preprocess_image(pixels, (32, 48), 1)
        for t in range(3):
            assert torch.equal(clip[:, t], ref[:, 0]), name
        _check_frame(clip[:, 0].cpu(), R.transform_u8(pixels, (32, 48), resize_fn=_pillow_resize), name)
    # interp: images 0 and 1 for the first prompt (a prompt file of one line)
    with open(str(tmp_path / "prompts.txt"), "w") as f:
        f.write("morph\n")
    names, data, got_prompts = I.load_data_prompts(str(tmp_path), video_size=(32, 48), video_frames=4, interp=True, device=DEV)
    assert names == [files[0][0]] and got_prompts == ["morph"] and data[0].shape == (3, 4, 32, 48)
    for t in range(4):
        assert torch.equal(data[0][:, t], I.preprocess_image(files[t // 2][1], (32, 48), 1)[:, 0])
    with pytest.raises(RuntimeError):
        I.load_data_prompts(str(tmp_path), video_size=(32, 48), video_frames=3, device="cpu")


# ------------------------------------------------------------------------------------------------ run_inference
SIZE, T_MODEL = 64, 4       # TINY_UNET halves the latent three times and the AE has a factor of 8: 64 is the smallest frame


@pytest.fixture(scope="module")
def tiny_files(tmp_path_factory):
    """The tiny model of the existing GPU tests with toy conditioners, as a YAML and a {"state_dict": ...} checkpoint, and a
    prompt folder of two prompts and two images larger than the frame."""
    from dynamicrafter_amd.utils.utils import instantiate_from_config
    from oracle.weights import fill_state_dict
    from tests.golden_cfg import TINY_AE, TINY_RESAMPLER, TINY_UNET
    d = tmp_path_factory.mktemp("inference")
    root = os.path.join(os.path.dirname(__file__), "..", "dynamicrafter_amd", "configs")
    cfg = yaml.safe_load(open(os.path.join(root, "inference_512_v1.0.yaml")))
    p = cfg["model"]["params"]
    p["unet_config"]["params"] = dict(TINY_UNET, default_fs=24)
    p["first_stage_config"]["params"]["ddconfig"] = dict(TINY_AE)
    p["cond_stage_config"] = {"target": "tests.golden_cfg.ToyTextEmbedder"}
    p["img_cond_stage_config"] = {"target": "tests.golden_cfg.ToyImageEmbedder"}
    p["image_proj_stage_config"] = {"target": "lvdm.modules.encoders.resampler.Resampler", "params": dict(TINY_RESAMPLER)}
    with open(str(d / "tiny.yaml"), "w") as f:
        yaml.safe_dump(cfg, f)
    model = instantiate_from_config(cfg["model"])
    for mod, seed in ((model.model.diffusion_model, 11), (model.first_stage_model, 13), (model.image_proj_model, 14)):
        sdict = mod.state_dict()
        mod.load_state_dict(fill_state_dict({k: tuple(v.shape) for k, v in sdict.items()}, seed), strict=True)
    torch.save({"state_dict": model.state_dict()}, str(d / "tiny.ckpt"))
    files = _write_folder(str(d / "prompts"), [(100, 150), (131, 97)], ["a corgi runs", "waves on a beach"], fmts=("png", "jpg"))
    return dict(dir=d, config=str(d / "tiny.yaml"), ckpt=str(d / "tiny.ckpt"), prompts=str(d / "prompts"),
                stems=[n.split(".")[0] for n, _ in files])


def _args(tf, savedir, *extra):
    from dynamicrafter_amd.scripts.evaluation.inference import get_parser
    return get_parser().parse_args(["--config", tf["config"], "--ckpt_path", tf["ckpt"], "--prompt_dir", tf["prompts"],
                                    "--savedir", str(savedir), "--height", str(SIZE), "--width", str(SIZE), "--ddim_steps", "2",
                                    "--video_length", str(T_MODEL), "--frame_stride", "24", "--text_input",
                                    "--unconditional_guidance_scale", "7.5", "--seed", "123", *extra])


def _run(tf, savedir, *extra, gpu_num=1, gpu_no=0, device=None):
    from dynamicrafter_amd.scripts.evaluation import inference as I
    args = _args(tf, savedir, *extra)
    I.seed_everything(args.seed)
    return I.run_inference(args, gpu_num, gpu_no, device=device)


def _apng_frames(path):
    im = Image.open(path)
    frames = []
    for i in range(getattr(im, "n_frames", 1)):
        im.seek(i)
        frames.append(np.asarray(im.convert("RGB")))
    return frames


def test_run_inference_end_to_end(tiny_files, tmp_path):
    tf = tiny_files
    written = _run(tf, tmp_path / "a")
    sep = tmp_path / "a" / "samples_separate"
    assert sorted(os.listdir(str(sep))) == [f"{s}_sample0.png" for s in tf["stems"]]
    assert sorted(written) == sorted(str(sep / f"{s}_sample0.png") for s in tf["stems"])
    clips = []
    for s in tf["stems"]:
        frames = _apng_frames(str(sep / f"{s}_sample0.png"))
        assert len(frames) == T_MODEL and all(f.shape == (SIZE, SIZE, 3) for f in frames)
        clips.append(open(str(sep / f"{s}_sample0.png"), "rb").read())
    assert clips[0] != clips[1]
    # the same seed gives the same bytes
    _run(tf, tmp_path / "b")
    for s, ref in zip(tf["stems"], clips):
        assert open(str(tmp_path / "b" / "samples_separate" / f"{s}_sample0.png"), "rb").read() == ref
    # rank 1 of 2 takes the second prompt only (on the one device there is here)
    _run(tf, tmp_path / "c", gpu_num=2, gpu_no=1, device=0)
    assert os.listdir(str(tmp_path / "c" / "samples_separate")) == [f"{tf['stems'][1]}_sample0.png"]


def test_run_inference_avi(tiny_files, tmp_path):
    tf = tiny_files
    _run(tf, tmp_path, "--container", "avi", "--quality", "90")
    sep = tmp_path / "samples_separate"
    assert sorted(os.listdir(str(sep))) == [f"{s}_sample0.avi" for s in tf["stems"]]
    for s in tf["stems"]:
        r = J.walk_avi(open(str(sep / f"{s}_sample0.avi"), "rb").read())
        assert len(r["frames"]) == T_MODEL
        for fr in r["frames"]:
            im = Image.open(io.BytesIO(fr))
            im.load()
            assert im.size == (SIZE, SIZE) and im.mode == "RGB"

"""Host side of the float image resize and of the application classes, without a GPU: ops.resize_coeffs_f32 against the plain
restatement (equality), the restatement against torch.nn.functional.interpolate on the CPU (tests/resize_f32_restatement.TOL),
the centre-crop geometry with its 0.0 padding, the argument checks of the two C entries, and the import / naming contract of
scripts.evaluation.funcs and scripts.gradio.*."""
import ctypes as C
import importlib
import sys

import numpy as np
import pytest
import torch

from tests import resize_f32_restatement as R

SIZES = sorted({(a, b) for _, hw, r, _, _ in R.CASES for a, b in ((hw[0], r[0]), (hw[1], r[1]))} | {(3000, 576), (4000, 1024)})


@pytest.mark.parametrize("antialias", [True, False])
def test_resize_coeffs_f32_equals_the_restatement(antialias):
    from dynamicrafter_amd import ops
    for n_in, n_out in SIZES:
        k, xmin, n = ops.resize_coeffs_f32(n_in, n_out, antialias)
        rk, rxmin, rn = R.coeffs(n_in, n_out, antialias)
        assert k.dtype == np.float32 and xmin.dtype == np.int32 and n.dtype == np.int32
        assert k.shape == rk.shape and np.array_equal(k, rk), (n_in, n_out)
        assert np.array_equal(xmin, rxmin) and np.array_equal(n, rn), (n_in, n_out)
        assert (n >= 1).all() and (xmin >= 0).all() and (xmin + n <= n_in).all() and (n <= k.shape[1]).all()
        assert np.abs(k.sum(1) - 1.0).max() < 1e-6 and (k >= 0).all()
        assert (k[np.arange(k.shape[1])[None, :] >= n[:, None]] == 0).all()
    with pytest.raises(ValueError):
        ops.resize_coeffs_f32(0, 4, antialias)


def test_two_tap_rule_without_antialias():
    """antialias=False: two taps at half-pixel centres, the clamped border pixel alone at the ends."""
    k, xmin, n = R.coeffs(128, 16, False)
    assert k.shape[1] == 2 and (n == 2).all() and np.array_equal(xmin, 8 * np.arange(16) + 3)
    assert np.array_equal(k, np.full((16, 2), 0.5, np.float32))
    k, xmin, n = R.coeffs(7, 33, False)
    assert xmin[0] == 0 and k[0, 0] == 1.0 and k[0, 1] == 0.0                    # src < 0 is clamped to pixel 0
    assert n[-1] == 1 and xmin[-1] == 6 and k[-1, 0] == 1.0                        # both taps are the last pixel


@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_restatement_matches_torch_interpolate(case, antialias):
    _, hw, resized, crop, offset = case
    for c in R.CHANNELS:
        img = R.make_image(c, hw[0], hw[1])
        got = R.resize_crop(img, resized, crop, offset, antialias)
        ref = R.torch_reference(img, resized, crop, offset, antialias)
        err = float(np.abs(got - ref).max())
        print(f"{case[0]} C={c} antialias={antialias}: max abs error {err:.3g}")
        assert got.shape == ref.shape and err <= R.TOL


def test_square_image_to_320x512_pads_96_columns_of_zero_each_side():
    from dynamicrafter_amd.scripts.evaluation.inference import resize_geometry
    g = resize_geometry(100, 100, (320, 512))
    assert (g.rh, g.rw) == (320, 320) and (g.pad_left, g.pad_right) == (96, 96) and (g.top, g.left) == (0, 0)
    yoff, xoff = g.top - g.pad_top, g.left - g.pad_left
    assert (yoff, xoff) == (0, -96)
    img = R.make_image(3, 100, 100) * 0.5 + 0.25                      # no exact 0.0 inside the image
    out = R.resize_crop(img, (g.rh, g.rw), (320, 512), (yoff, xoff), True)
    assert out.shape == (3, 320, 512)
    assert (out[:, :, :96] == 0.0).all() and (out[:, :, 416:] == 0.0).all() and (out[:, :, 96:416] != 0.0).all()
    # an odd difference: the extra column goes to the right (CenterCrop pads (c - i) // 2 before, the rest after)
    g = resize_geometry(50, 50, (20, 33))
    assert (g.rh, g.rw, g.pad_left, g.pad_right, g.left) == (20, 20, 6, 7, 0)
    assert R.CASES[5][0].startswith("odd_pad") and R.CASES[5][4] == (g.top - g.pad_top, g.left - g.pad_left)


def test_entries_check_arguments_without_gpu():
    from dynamicrafter_amd import _hip
    lib = _hip.lib()
    p = C.c_void_p(16)
    assert lib.dc_resize_f32_h(None, p, p, p, p, 3, 3, 8, 8, 4, 0, 8, 0, 4, 0, None) == -2
    assert lib.dc_resize_f32_h(p, p, p, p, p, 3, 0, 8, 8, 4, 0, 8, 0, 4, 0, None) == -1         # C = 0
    assert lib.dc_resize_f32_h(p, p, p, p, p, 3, 3, 8, 8, 4, 1, 8, 0, 4, 0, None) == -1         # rows past H
    assert lib.dc_resize_f32_h(p, p, p, p, p, 3, 3, 8, 8, 4, 0, 8, 1, 4, 0, None) == -1         # columns past out_w
    assert lib.dc_resize_f32_h(p, p, p, p, p, 3, 3, 8, 8, 4, 0, 8, 0, 4, -1, None) == -1        # seg < 0
    assert lib.dc_resize_f32_h(p, p, p, p, p, 17, 3, 8, 8, 4, 0, 8, 0, 4, 16384, None) == -1    # a tile beyond the LDS form
    assert lib.dc_resize_f32_finish(p, None, p, p, p, 3, 1, 3, 8, 8, 0, 0, 8, 4, 0, 0, 8, 4, None) == -2
    assert lib.dc_resize_f32_finish(p, p, None, p, p, 3, 1, 3, 8, 8, 0, 0, 8, 4, 0, 0, 8, 4, None) == -2   # a pass without tables
    assert lib.dc_resize_f32_finish(p, p, p, p, p, 3, 3, 3, 8, 8, 0, 0, 8, 4, 0, 0, 8, 4, None) == -1      # axis 3
    # axis 0 addresses src directly: it must hold every resized pixel the crop keeps (8 x 8 of a 16 x 16 image does not)
    assert lib.dc_resize_f32_finish(p, p, None, None, None, 0, 0, 3, 8, 8, 0, 0, 16, 16, 0, 0, 16, 16, None) == -1


def test_cpu_tensors_are_refused():
    from dynamicrafter_amd import ops
    with pytest.raises(RuntimeError):
        ops.resize_f32(torch.zeros(3, 8, 8), (4, 4))


APP_MODULES = ["dynamicrafter_amd.scripts.evaluation.funcs", "dynamicrafter_amd.scripts.gradio.i2v_test",
               "dynamicrafter_amd.scripts.gradio.i2v_test_application", "dynamicrafter_amd.scripts.gradio.dynamicrafter_pipeline"]


def test_app_modules_import_without_gpu_and_without_gradio():
    for name in APP_MODULES:
        importlib.import_module(name)
    assert "gradio" not in sys.modules and "torchvision" not in sys.modules and "cv2" not in sys.modules
    from dynamicrafter_amd.scripts.evaluation import funcs, inference
    from dynamicrafter_amd.scripts.gradio import dynamicrafter_pipeline, i2v_test, i2v_test_application
    for fn in ("get_latent_z", "load_model_checkpoint", "load_prompts"):
        assert getattr(funcs, fn) is getattr(inference, fn)                  # re-exported, not second copies
    assert funcs.get_filelist is not inference.get_filelist
    for fn in ("batch_ddim_sampling", "get_dirlist", "load_image_batch", "load_video_batch", "save_videos"):
        assert callable(getattr(funcs, fn))
    assert issubclass(i2v_test_application.Image2Video, i2v_test.Image2Video)
    for m in ("_preprocess_image", "_encode_prompt", "_encode_image", "_prepare_conditioning", "_prepare_latents",
              "_decode_latents", "_postprocess_video", "__call__", "save_video", "to", "enable_attention_slicing",
              "disable_attention_slicing", "enable_xformers_memory_efficient_attention"):
        assert callable(getattr(dynamicrafter_pipeline.DynamiCrafterImg2VideoPipeline, m))


def test_funcs_filelists_and_unsupported_loaders(tmp_path):
    from dynamicrafter_amd.scripts.evaluation import funcs
    for name in ("b.png", "a.png", "c.txt"):
        (tmp_path / name).write_bytes(b"")
    (tmp_path / "sub2").mkdir()
    (tmp_path / "sub1").mkdir()
    assert funcs.get_filelist(str(tmp_path), "png") == [str(tmp_path / "a.png"), str(tmp_path / "b.png")]
    assert len(funcs.get_filelist(str(tmp_path))) == 3
    assert funcs.get_dirlist(str(tmp_path)) == [str(tmp_path / "sub1"), str(tmp_path / "sub2")]
    assert funcs.get_dirlist(str(tmp_path / "missing")) == []
    with pytest.raises(NotImplementedError):
        funcs.load_video_batch(["x.mp4"], 1)


@pytest.mark.parametrize("module", ["i2v_test", "i2v_test_application"])
def test_image2video_does_not_download(module, tmp_path):
    mod = importlib.import_module(f"dynamicrafter_amd.scripts.gradio.{module}")
    with pytest.raises(RuntimeError, match="ckpt_path"):
        mod.Image2Video(str(tmp_path / "out"), resolution="320_512")
    i2v = mod.Image2Video(str(tmp_path / "out"), resolution="320_512", model=object())
    assert i2v.resolution == (320, 512) and i2v.save_fps == 8 and (tmp_path / "out").is_dir()
    with pytest.raises(RuntimeError, match="ckpt_path"):
        i2v.download_model()
    from dynamicrafter_amd.scripts.gradio.dynamicrafter_pipeline import DynamiCrafterImg2VideoPipeline
    with pytest.raises(RuntimeError, match="ckpt_path"):
        DynamiCrafterImg2VideoPipeline("256_256")


def test_prompt_to_filename_rule():
    from dynamicrafter_amd.scripts.gradio.i2v_test import prompt_to_filename
    assert prompt_to_filename("a/b c") == "a_slash_b_c"
    assert prompt_to_filename("") == "empty_prompt"
    long = "a man fishing in a boat at sunset, golden hour, 4k"
    assert prompt_to_filename(long) == long.replace(" ", "_")[:40] and len(prompt_to_filename(long)) == 40
    assert prompt_to_filename("x" * 39 + "/y") == "x" * 39 + "_"                 # the cut comes after the replacement

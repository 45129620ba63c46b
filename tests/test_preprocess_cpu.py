"""Prompt-folder loading and the inference CLI, the parts that need no GPU: the restatement (tests/preprocess_restatement.py -
the reference of the GPU tests) against Pillow's own resize, the package's host coefficient tables against the restatement's,
torchvision's size / crop arithmetic on known answers, the file handling and the parser, and the argument checks of the two
dc_prep_* entries."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from PIL import Image

from tests import preprocess_restatement as R

# (h, w) -> (oh, ow): down- and up-scaling, identity (both axes, one axis), a reduction factor of 2.5 on both axes; the last one
# (not among the eight of the issue) has a reduction factor of 80 along x: 160 taps per output pixel, ksize 161
RESIZES = [((37, 53), (16, 22)), ((16, 16), (16, 16)), ((9, 7), (32, 24)), ((301, 200), (48, 32)), ((64, 100), (32, 50)),
           ((33, 17), (32, 16)), ((5, 400), (2, 160)), ((40, 40), (40, 17)), ((6, 400), (6, 5))]
_ids = lambda c: f"{c[0][0]}x{c[0][1]}to{c[1][0]}x{c[1][1]}"


@pytest.mark.parametrize("case", RESIZES, ids=_ids)
def test_restatement_equals_pillow_in_every_pixel(case):
    (h, w), (oh, ow) = case
    rng = np.random.default_rng(1)
    for kind in ("noise", "ramp", "zeros", "ones"):
        a = R.make_image(kind, h, w, rng)
        ref = np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR))
        got = R.resize(a, oh, ow)
        assert got.shape == ref.shape == (oh, ow, 3)
        assert int((got != ref).sum()) == 0, f"{kind}: {int((got != ref).sum())} of {ref.size} bytes differ from Pillow"


def test_the_longest_case_has_160_taps():
    k, xmin, n = R.coeffs(400, 5)
    assert k.shape == (5, 2 * 80 + 1) and int(n.max()) == 160


@pytest.mark.parametrize("case", RESIZES + [((3024, 4032), (576, 768))], ids=_ids)
def test_host_coefficient_tables_equal_the_restatements(case):
    from dynamicrafter_amd import ops
    (h, w), (oh, ow) = case
    for n_in, n_out in ((w, ow), (h, oh)):
        k, xmin, n = ops.resize_coeffs(n_in, n_out)
        rk, rxmin, rn = R.coeffs(n_in, n_out)
        assert k.dtype == np.int32 and xmin.dtype == np.int32 and n.dtype == np.int32
        assert k.shape == rk.shape and (k == rk).all() and (xmin == rxmin).all() and (n == rn).all()
        assert (xmin + n <= n_in).all() and (n <= k.shape[1]).all() and (n >= 1).all()
        assert (k.sum(axis=1) > (1 << 22) - k.shape[1]).all()               # weights sum to 1 up to the rounding of each tap


def test_resize_geometry_known_answers():
    from dynamicrafter_amd.scripts.evaluation.inference import resize_geometry
    g = resize_geometry(37, 53, (16, 16))
    assert (g.rh, g.rw, g.left, g.top) == (16, 22, 3, 0) and (g.pad_top, g.pad_bottom, g.pad_left, g.pad_right) == (0, 0, 0, 0)
    g = resize_geometry(9, 7, (32, 24))
    assert (g.rh, g.rw) == (30, 24) and (g.pad_top, g.pad_bottom, g.pad_left, g.pad_right) == (1, 1, 0, 0)
    assert (g.top, g.left) == (0, 0)
    g = resize_geometry(301, 200, (32, 48))
    assert (g.rh, g.rw, g.top) == (48, 32, 8) and (g.pad_left, g.pad_right, g.left) == (8, 8, 0)
    # round-half-even both ways: resized widths 21 and 23 cropped to 16 give 2.5 -> 2 and 3.5 -> 4
    g = resize_geometry(16, 21, (16, 16))
    assert (g.rh, g.rw, g.left) == (16, 21, 2)
    g = resize_geometry(16, 23, (16, 16))
    assert (g.rh, g.rw, g.left) == (16, 23, 4)
    g = resize_geometry(16, 40, (16, 16))
    assert (g.rh, g.rw, g.left, g.top) == (16, 40, 12, 0)
    # odd padding: the extra pixel goes after
    g = resize_geometry(8, 40, (16, 13))        # s = 13: rh = 13, rw = 65
    assert (g.rh, g.rw) == (13, 65) and (g.pad_top, g.pad_bottom) == (1, 2) and g.left == 26
    for hw, vs in (((37, 53), (16, 16)), ((9, 7), (32, 24)), ((301, 200), (32, 48)), ((16, 21), (16, 16)), ((8, 40), (16, 13))):
        r = R.geometry(hw[0], hw[1], vs)
        g = resize_geometry(hw[0], hw[1], vs)
        assert (g.rh, g.rw, (g.pad_top, g.pad_bottom, g.pad_left, g.pad_right), g.top, g.left) == \
            (r["rh"], r["rw"], r["pad"], r["top"], r["left"])
    with pytest.raises(ValueError):
        resize_geometry(0, 5, (16, 16))


def _folder(tmp_path, n_images=4):
    rng = np.random.default_rng(1)
    names = ["b_02.png", "a_01.jpg", "c_03.JPEG", "d_04.PNG", "e_05.jpeg"][:n_images]
    for i, nm in enumerate(names):
        Image.fromarray(R.make_image("noise", 20 + i, 30 - i, rng)).save(str(tmp_path / nm))
    (tmp_path / "skip.gif").write_bytes(b"GIF89a")
    (tmp_path / "z_prompts.txt").write_text("unused\n")
    (tmp_path / "prompts.txt").write_text("  first prompt \n\nsecond prompt\n   \nthird\n")
    return names


def test_get_filelist_and_load_prompts(tmp_path):
    from dynamicrafter_amd.scripts.evaluation import inference as I
    _folder(tmp_path, 5)
    files = I.get_filelist(str(tmp_path), ["jpg", "png", "jpeg", "JPEG", "PNG"])
    assert [os.path.basename(f) for f in files] == ["a_01.jpg", "b_02.png", "c_03.JPEG", "d_04.PNG", "e_05.jpeg"]
    assert [os.path.basename(f) for f in I.get_filelist(str(tmp_path), ["txt"])] == ["prompts.txt", "z_prompts.txt"]
    assert I.get_filelist(str(tmp_path), ["mp4"]) == []
    assert I.load_prompts(str(tmp_path / "prompts.txt")) == ["first prompt", "second prompt", "third"]


def test_load_data_prompts_pairing_and_cpu_refusal(tmp_path, monkeypatch):
    """The pairing logic without a GPU: preprocess_image is replaced by a recorder. Non-interp takes image idx, interp images
    2 idx and 2 idx + 1 into the two halves, named after the first of the pair; a CPU device raises before anything is read."""
    import torch
    from dynamicrafter_amd.scripts.evaluation import inference as I
    _folder(tmp_path, 5)
    (tmp_path / "prompts.txt").write_text("one\ntwo\n")
    with pytest.raises(RuntimeError):
        I.load_data_prompts(str(tmp_path), video_size=(16, 16), video_frames=4, device="cpu")
    with pytest.raises(RuntimeError):
        I.preprocess_image(torch.zeros(8, 8, 3, dtype=torch.uint8), (16, 16), 4)
    calls = []

    def fake(img, video_size, video_frames, out=None, t0=0, nt=None):
        calls.append((img.shape, tuple(video_size), video_frames, t0, nt))
        return out

    monkeypatch.setattr(I, "preprocess_image", fake)
    monkeypatch.setattr(torch, "empty", lambda *a, **k: None)                 # no device here to allocate on
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    names, data, prompts = I.load_data_prompts(str(tmp_path), video_size=(16, 24), video_frames=4)
    assert names == ["a_01.jpg", "b_02.png"] and prompts == ["one", "two"] and len(data) == 2
    assert calls == [((21, 29, 3), (16, 24), 4, 0, None), ((20, 30, 3), (16, 24), 4, 0, None)]
    del calls[:]
    names, data, prompts = I.load_data_prompts(str(tmp_path), video_size=(16, 24), video_frames=4, interp=True)
    assert names == ["a_01.jpg", "c_03.JPEG"]
    assert [(c[0], c[3], c[4]) for c in calls] == [((21, 29, 3), 0, 2), ((20, 30, 3), 2, 2), ((22, 28, 3), 0, 2), ((23, 27, 3), 2, 2)]


# inference.py:383-413 of the reference: flag -> default ("store_true" flags default to False)
REFERENCE_FLAGS = dict(savedir=None, ckpt_path=None, config=None, prompt_dir=None, n_samples=1, ddim_steps=50, ddim_eta=1.0, bs=1,
                       height=512, width=512, frame_stride=3, unconditional_guidance_scale=1.0, seed=123, video_length=16,
                       negative_prompt=False, text_input=False, multiple_cond_cfg=False, cfg_img=None,
                       timestep_spacing="uniform", guidance_rescale=0.0, perframe_ae=False, use_fixed_scheduler=False,
                       loop=False, interp=False)
OUR_FLAGS = dict(sampler="ddim", container="apng", quality=90, num_frames=None, window_stride=None)


def test_parser_flags_and_defaults():
    from dynamicrafter_amd.scripts.evaluation.inference import get_parser
    args = vars(get_parser().parse_args([]))
    assert args == {**REFERENCE_FLAGS, **OUR_FLAGS}
    for k, v in args.items():
        assert type(v) is type({**REFERENCE_FLAGS, **OUR_FLAGS}[k]), k
    a = get_parser().parse_args("--config c.yaml --ckpt_path m.ckpt --prompt_dir p --savedir s --height 320 --width 512 "
                                "--unconditional_guidance_scale 7.5 --ddim_steps 50 --ddim_eta 1.0 --text_input "
                                "--video_length 16 --frame_stride 24 --timestep_spacing uniform_trailing --guidance_rescale 0.7 "
                                "--perframe_ae --seed -1 --interp --loop --multiple_cond_cfg --cfg_img 2.0 --negative_prompt "
                                "--use_fixed_scheduler --bs 1 --n_samples 2 --container avi --quality 80 --sampler dpmpp_2m "
                                "--num_frames 32 --window_stride 8".split())
    assert (a.height, a.width, a.frame_stride, a.seed, a.cfg_img, a.container, a.sampler) == (320, 512, 24, -1, 2.0, "avi", "dpmpp_2m")
    assert a.text_input and a.perframe_ae and a.interp and a.loop and a.multiple_cond_cfg and a.negative_prompt
    assert (a.num_frames, a.window_stride, a.quality, a.n_samples) == (32, 8, 80, 2)
    with pytest.raises(SystemExit):
        get_parser().parse_args(["--container", "mp4"])


def test_prep_entries_reject_bad_arguments_without_gpu():
    """NULL operands -> DC_ERR_ARG (-2), bad shapes -> DC_ERR_SHAPE (-1), all before any launch."""
    from dynamicrafter_amd import _hip
    lib = _hip.lib()
    p = C.c_void_p(8)
    # dc_prep_resize_h(src, dst, k, xmin, n, ksize, H, W, out_w, y0, rows, x0, cols, stream)
    ok = [p, p, p, p, p, 5, 40, 40, 17, 0, 40, 0, 17]
    for i in range(5):
        a = list(ok); a[i] = None
        assert lib.dc_prep_resize_h(*a, None) == -2
    for i, bad in ((5, 0), (6, 0), (7, 0), (8, 0), (9, -1), (10, 0), (10, 41), (11, -1), (12, 0), (12, 18), (9, 1), (11, 1)):
        a = list(ok); a[i] = bad
        assert lib.dc_prep_resize_h(*a, None) == -1, (i, bad)
    # dc_prep_finish(src, clip, k, kmin, kn, ksize, axis, sh, sw, sy0, sx0, rh, rw, yoff, xoff, ch, cw, T, t0, nt, stream)
    ok = [p, p, p, p, p, 5, 2, 40, 17, 0, 0, 17, 17, 0, 0, 17, 17, 3, 0, 3]
    for i in range(5):
        a = list(ok); a[i] = None
        assert lib.dc_prep_finish(*a, None) == -2
    a = list(ok); a[6] = 0; a[7] = 17; a[2] = a[3] = a[4] = None            # axis 0 takes no tables
    a[0] = None
    assert lib.dc_prep_finish(*a, None) == -2
    for i, bad in ((5, 0), (6, 3), (6, -1), (7, 0), (8, 0), (9, -1), (10, -1), (11, 0), (12, 0), (15, 0), (16, 0), (17, 0),
                   (18, -1), (18, 1), (19, 0), (19, 4),
                   (8, 16),          # vertical pass: src narrower than the columns the crop keeps
                   (10, 1)):         # ... or starting right of the first of them
        a = list(ok); a[i] = bad
        assert lib.dc_prep_finish(*a, None) == -1, (i, bad)
    # horizontal pass: src must hold the rows the crop keeps
    h = [p, p, p, p, p, 5, 1, 40, 40, 0, 0, 40, 17, 12, 0, 16, 17, 1, 0, 1]
    for i, bad in ((7, 27), (9, 13)):
        a = list(h); a[i] = bad
        assert lib.dc_prep_finish(*a, None) == -1, (i, bad)


def test_prep_entries_are_exported_and_declared():
    from dynamicrafter_amd import _hip
    nm = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (dc_[a-z0-9_]+)", nm))
    hdr = open(os.path.join(os.path.dirname(_hip._HERE), "include", "dcrafter_hip.h")).read()
    for name in ("dc_prep_resize_h", "dc_prep_finish"):
        assert name in exported and name in _hip.SIGNATURES
        decl = hdr[:hdr.index(f"int {name}(")]
        comment = decl[decl.rindex("/*"):]
        assert "replaces scripts/evaluation/inference.py:7" in comment          # the call site it stands for
        assert _hip.SIGNATURES[name][0] is C.c_int and _hip.SIGNATURES[name][1][-1] is C.c_void_p      # int, stream last


def test_main_takes_rank_and_device_from_the_environment(monkeypatch):
    """Under torch.distributed.run a process is rank RANK of WORLD_SIZE on device LOCAL_RANK; alone it is rank 0 of 1. A negative
    seed draws one; random, numpy and torch are seeded from it."""
    import random
    import torch
    from dynamicrafter_amd.scripts.evaluation import inference as I
    seen = []
    monkeypatch.setattr(I, "run_inference", lambda args, gpu_num, gpu_no, device=None: seen.append((gpu_num, gpu_no, device, args.seed)))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    I.main(["--seed", "7"])
    first = (random.random(), float(np.random.rand()), float(torch.rand(1)))
    I.main(["--seed", "7"])
    assert first == (random.random(), float(np.random.rand()), float(torch.rand(1)))
    monkeypatch.setenv("WORLD_SIZE", "8"); monkeypatch.setenv("RANK", "11"); monkeypatch.setenv("LOCAL_RANK", "3")
    I.main(["--seed", "-1"])
    assert seen == [(1, 0, 0, 7), (1, 0, 0, 7), (8, 11, 3, -1)]

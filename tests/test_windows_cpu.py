"""Windowed sampling, host side: the window plan's invariants, its refusals, the argument checks of the two C entries
(no GPU needed: they return before any launch) and the harness's refusal of num_frames with loop / interp.

Stated tolerance: the per-frame sum of the normalised weights is 1 within W * 2^-24 (float64 normalisation, each of
the <= W terms rounded to fp32)."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

from dynamicrafter_amd.lvdm.models.samplers.windows import window_plan

# (T_long, T, stride): T_long == T, T_long = T + 1, stride 1, stride == T, the flagship 32 / 16 / 8, odd sizes
GEOMETRIES = [(4, 4, 2), (16, 16, 8), (5, 4, 2), (17, 16, 8), (9, 4, 1), (12, 4, 4), (40, 16, 16), (32, 16, 8),
              (8, 4, 2), (24, 16, 8), (23, 7, 3), (64, 16, 5)]
SHIFTS = (0, 1, 3)                    # 3 divides neither 2, 4, 5, 8 nor 16
STEPS = (1, 7)


@pytest.mark.parametrize("weights", ["uniform", "triangle"])
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_plan_invariants(geom, weights):
    T_long, T, stride = geom
    for shift, S in itertools.product(SHIFTS, STEPS):
        starts, wn = window_plan(T_long, T, stride, weights, shift, S)
        assert starts.dtype == np.int32 and wn.dtype == np.float32
        assert starts.ndim == 2 and starts.shape[0] == S                       # one row per step: W constant over steps
        W = starts.shape[1]
        assert wn.shape == (S, W, T)
        assert starts.min() >= 0 and starts.max() + T <= T_long, (geom, shift)  # every window inside the clip
        assert wn.min() >= 0.0
        for i in range(S):
            covered = np.zeros(T_long, dtype=bool)
            total = np.zeros(T_long, dtype=np.float64)
            for w in range(W):
                s = int(starts[i, w])
                if wn[i, w].any():
                    covered[s:s + T] = True
                total[s:s + T] += wn[i, w].astype(np.float64)
            assert covered.all(), (geom, weights, shift, i)                     # by windows that carry weight
            assert np.abs(total - 1.0).max() <= W * 2.0 ** -24, (geom, weights, shift, i, np.abs(total - 1.0).max())
        if shift % stride and S > 1 and T_long - T > stride:
            assert (starts[0] != starts[1]).any(), "a shifting plan moves the interior windows"
        if T_long > T:                                                          # the ends stay clamped at every step
            assert (starts[:, 0] == 0).all() and (starts.max(axis=1) == T_long - T).all()


def test_triangle_is_positive_at_the_ends_and_peaks_at_the_centre():
    from dynamicrafter_amd.lvdm.models.samplers.windows import window_profile
    for T in (1, 4, 7, 16):
        p = window_profile(T, "triangle")
        assert p[0] > 0 and p[-1] > 0 and p.argmax() in ((T - 1) // 2, T // 2) and (p == p[::-1]).all()
    # a uniform average puts a hard seam at a window's edge, the triangle does not: weight of window 0 around frame 8
    _, wu = window_plan(32, 16, 8, "uniform")
    _, wt = window_plan(32, 16, 8, "triangle")
    assert wu[0, 0, 7] == 1.0 and wu[0, 0, 8] == 0.5
    assert abs(float(wt[0, 0, 8]) - float(wt[0, 0, 7])) < 0.2


def test_padding_windows_carry_no_weight():
    starts, wn = window_plan(8, 4, 2, "triangle", shift=1, S=4)      # the displaced steps need 4 windows, the others 3
    assert starts.shape == (4, 4)
    assert starts[0].tolist() == [0, 2, 4, 4] and not wn[0, 3].any()
    assert starts[1].tolist() == [0, 1, 3, 4] and wn[1].all(axis=1).all()
    starts, wn = window_plan(32, 16, 8, multiple_of=2)                # 3 windows padded to two calls of 2
    assert starts.shape == (1, 4) and not wn[0, 3].any() and wn[0, :3].all()


def test_single_window_when_the_clip_is_one_window_long():
    for weights, shift in itertools.product(("uniform", "triangle"), (0, 1, 5)):
        starts, wn = window_plan(16, 16, 8, weights, shift, S=5)
        assert starts.shape == (5, 1) and not starts.any()
        assert (wn == np.float32(1.0)).all()


@pytest.mark.parametrize("kw, names", [
    (dict(T_long=15, T=16, stride=8), ("15", "16")),
    (dict(T_long=32, T=16, stride=0), ("stride", "0")),
    (dict(T_long=32, T=16, stride=-2), ("stride", "-2")),
    (dict(T_long=32, T=16, stride=17), ("17", "16")),
    (dict(T_long=32, T=16, stride=8, weights="hann"), ("hann",)),
    (dict(T_long=32, T=16, stride=8, shift=-1), ("shift", "-1")),
])
def test_plan_refusals_name_the_offending_values(kw, names):
    with pytest.raises(ValueError) as ei:
        window_plan(**kw)
    for n in names:
        assert n in str(ei.value), (n, str(ei.value))


def test_check_plan_refuses_tables_a_kernel_must_not_index_with():
    from dynamicrafter_amd.lvdm.models.samplers.windows import check_plan
    starts, wn = window_plan(8, 4, 2)
    assert check_plan(starts, wn, 8, 4) == (1, 3)
    bad = starts.copy(); bad[0, 2] = 5
    with pytest.raises(ValueError, match="start"):
        check_plan(bad, wn, 8, 4)
    bad = starts.copy(); bad[0, 0] = -1
    with pytest.raises(ValueError, match="start"):
        check_plan(bad, wn, 8, 4)
    with pytest.raises(ValueError, match="sum to 1"):
        check_plan(starts, wn * 0.5, 8, 4)
    with pytest.raises(ValueError, match="finite"):
        check_plan(starts, wn * np.float32("nan"), 8, 4)
    with pytest.raises(ValueError, match=r"\[S, W\]"):
        check_plan(starts, wn[:, :, :3], 8, 4)


def test_window_abi_argument_errors_without_gpu():
    """NULL operands give DC_ERR_ARG (-2), bad shapes DC_ERR_SHAPE (-1), before any launch."""
    from dynamicrafter_amd import _hip
    lib = _hip.lib()
    f, z = C.c_void_p(16), C.c_void_p(0)                  # never dereferenced: every call returns before a launch
    #            index S  W  w0 n_w B  Cx Cc TL T  HW c_pad nrep
    good_pack = [0, 4, 3, 0, 3, 1, 4, 4, 8, 4, 16, 64, 1]
    pack = lambda x, cc, out, st, ints: lib.dc_pack_latent_windows(x, cc, out, st, z, *ints, z)
    assert pack(z, f, f, f, good_pack) == -2
    assert pack(f, z, f, f, good_pack) == -2              # Cc > 0 needs c_concat
    assert pack(f, f, z, f, good_pack) == -2
    assert pack(f, f, f, z, good_pack) == -2
    for pos, val in ((11, 60), (11, 4), (4, 4), (3, -1), (8, 3), (0, 4), (0, -1), (12, 0), (1, 0)):
        ints = list(good_pack); ints[pos] = val
        assert pack(f, f, f, f, ints) == -1, (pos, val)
    #             index S  W  w0 n_w nb B  C  TL T  HW acc
    good_merge = [0, 4, 3, 0, 3, 2, 1, 4, 8, 4, 16, 0]
    merge = lambda e, out, st, wn, ints, ld_e=4, ld_out=4: lib.dc_window_merge(e, ld_e, out, ld_out, st, wn, z, *ints, z)
    assert merge(z, f, f, f, good_merge) == -2
    assert merge(f, z, f, f, good_merge) == -2
    assert merge(f, f, z, f, good_merge) == -2
    assert merge(f, f, f, z, good_merge) == -2
    for pos, val in ((4, 4), (3, 1), (8, 3), (0, 4), (5, 0), (7, 0), (2, 0)):
        ints = list(good_merge); ints[pos] = val
        assert merge(f, f, f, f, ints) == -1, (pos, val)
    assert merge(f, f, f, f, good_merge, ld_e=3) == -1
    assert merge(f, f, f, f, good_merge, ld_out=2) == -1


def test_library_exports_the_window_entries():
    from dynamicrafter_amd import _hip
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("dc_pack_latent_windows", "dc_window_merge"):
        assert f" T {name}\n" in out, name
        assert name in _hip.SIGNATURES


def test_harness_refuses_num_frames_with_loop_or_interp():
    """Raised from the arguments alone: the model is never touched (an object() has no attribute to touch)."""
    from dynamicrafter_amd.scripts.evaluation.inference import image_guided_synthesis
    for kw in (dict(loop=True), dict(interp=True)):
        with pytest.raises(ValueError, match="num_frames"):
            image_guided_synthesis(object(), ["x"], None, [1, 4, 32, 8, 8], num_frames=32, **kw)


def test_windows_per_call_rule():
    """Equal chunks: the fewest calls under the caps, then the fewest windows per call; refusals."""
    from dynamicrafter_amd.lvdm.models.samplers.windows import windows_per_call
    assert windows_per_call(3, 5) == 3                     # all in one call
    assert windows_per_call(3, 5, per_call=8) == 3         # a cap above W changes nothing
    assert windows_per_call(3, 2) == 2                     # the scratch limit binds: 2 calls of 2 (one padding window)
    assert windows_per_call(7, 5) == 4                     # 2 calls either way: 4 + 4 rather than 5 + 5
    assert windows_per_call(7, 5, per_call=3) == 3         # the caller's cap binds: 3 calls of 3
    assert windows_per_call(7, 2, per_call=3) == 2         # a per_call above the scratch limit is clamped to it
    assert windows_per_call(4, 9, per_call=1) == 1
    for W, cap, pc in ((5, 3, None), (9, 4, 2), (16, 5, None), (1, 1, 1)):
        n = windows_per_call(W, cap, pc)
        calls = -(-W // n)
        assert 1 <= n <= cap and (pc is None or n <= pc) and calls * n >= W > (calls - 1) * n
    with pytest.raises(ValueError, match="windows_per_call"):
        windows_per_call(3, 5, per_call=0)
    with pytest.raises(ValueError, match="scratch"):
        windows_per_call(3, 0)


@pytest.mark.parametrize("res,hw,caps", [("256", (32, 32), (102, 51, 34)), ("512", (40, 64), (40, 20, 13)),
                                         ("1024", (72, 128), (11, 5, 3))])
def test_scratch_limit_of_the_released_configs(res, hw, caps):
    """max_row_width from the block layout (no device: the model is built on the meta device) and the windows per call
    it admits with 1 / 2 / 3 branches: floor((2^31 - 1) / (16 h w 1280)) / branches."""
    import os
    import torch
    import yaml
    from dynamicrafter_amd.utils.utils import instantiate_from_config
    root = os.path.join(os.path.dirname(__file__), "..", "dynamicrafter_amd", "configs")
    cfg = yaml.safe_load(open(os.path.join(root, f"inference_{res}_v1.0.yaml")))
    p = cfg["model"]["params"]
    for k in ("cond_stage_config", "img_cond_stage_config", "image_proj_stage_config"):
        p[k] = {"target": "torch.nn.Identity"}
    with torch.device("meta"):
        model = instantiate_from_config(cfg["model"])
    net = model.model.diffusion_model
    # level 0: 320 channels, GEGLU hidden 4 x 320; level 1: 4 x 640 / 4; level 2: the 2560-wide concat / 16 ...
    assert net.max_row_width() == 1280.0
    assert net.max_context_row_width() == 4 * 1280        # k / v / k_ip / v_ip of the 1280-wide transformers
    h, w = hw
    for nb, cap in zip((1, 2, 3), caps):
        assert model.max_windows_per_call((1, 4, 32, h, w), nb, 16) == cap
        assert cap == (2 ** 31 - 1) // (16 * h * w * 1280) // nb
    assert model.max_windows_per_call((2, 4, 32, h, w), 2, 16) == caps[1] // 2
    with pytest.raises(ValueError, match="2\\^31"):
        model.max_windows_per_call((1, 4, 32, 512, 512), 2, 16)
    # a latent of a few positions: the context rows are the larger buffers
    assert model.max_windows_per_call((1, 4, 32, 2, 2), 1, 16) == (2 ** 31 - 1) // (16 * 93 * 5120)


def test_arena_refuses_a_buffer_of_2_to_the_31_elements():
    import torch
    from dynamicrafter_amd.ops import Arena
    a = Arena()
    assert a.get("ok", 2 ** 20, 2 ** 10, device="meta").shape == (2 ** 20, 2 ** 10)
    with pytest.raises(ValueError, match="2\\^31"):
        a.get("big", 2 ** 21, 2 ** 10, device="meta")

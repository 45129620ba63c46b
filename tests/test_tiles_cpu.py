"""Spatially tiled sampling without a GPU: the host plan (lvdm/models/samplers/tiles.py) against the float64 restatement
(tests/tiles_restatement.py), its refusals, the option entry with its flags, the generalised chunk cap and the C entries'
argument checks."""
import numpy as np
import pytest

from tests import tiles_restatement as R

CASES = [((4, 16, 24), (4, 16, 16), (1, 8, 8)), ((4, 24, 32), (4, 16, 16), (1, 8, 8)), ((8, 24, 32), (4, 16, 16), (2, 8, 8))]


# ------------------------------------------------------------------ 1. the plan
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("weights", ["uniform", "triangle"])
@pytest.mark.parametrize("long_shape,box_shape,stride", CASES)
def test_plan_coverage_sums_to_one_and_equals_the_restatement(long_shape, box_shape, stride, weights, shift):
    from dynamicrafter_amd.lvdm.models.samplers.tiles import check_tiles, coverage_bound, tile_plan
    S = 5
    shifts = tuple(shift if L > n else 0 for L, n in zip(long_shape, box_shape))
    box, g = tile_plan(long_shape, box_shape, stride, weights, shifts, S)
    assert box.dtype == np.int32 and g.dtype == np.float32
    assert check_tiles(box, g, long_shape, box_shape) == (S, box.shape[1])
    ref = R.plan(long_shape, box_shape, stride, weights, shifts, S)
    assert box.shape[1] == max(len(st) for st in ref)
    worst = 0.0
    for i, boxes in enumerate(ref):
        n_axis = [len({b[0][a] for b in boxes}) for a in range(3)]
        assert len(boxes) == int(np.prod(n_axis))
        for k, (start, gt, gy, gx) in enumerate(boxes):           # flat index (wt Wy + wy) Wx + wx
            assert tuple(box[i, k]) == start
            assert np.array_equal(g[i, k], np.concatenate([gt, gy, gx]))
        for k in range(len(boxes), box.shape[1]):                 # padding: the last box again, weight 0
            assert tuple(box[i, k]) == boxes[-1][0] and not g[i, k].any()
        cover = R.coverage(box[i], g[i], long_shape, box_shape)
        bound = coverage_bound(n_axis)
        assert bound < (sum(n_axis) + 2.5) * 2.0 ** -24
        worst = max(worst, float(np.abs(cover - 1).max()) / bound)
        assert np.abs(cover - 1).max() <= bound
    print(f"\n[tile plan {long_shape} {weights} shift {shift}] W {box.shape[1]}, worst |sum - 1| / bound {worst:.3f}")
    if shift:
        assert (box[0] != box[1]).any()                            # the seams move


def test_degenerate_plan_is_one_box_of_weight_one():
    from dynamicrafter_amd.lvdm.models.samplers.tiles import tile_plan
    box, g = tile_plan((4, 16, 16), (4, 16, 16), (2, 8, 8), "triangle", (1, 1, 1), 3)
    assert box.shape == (3, 1, 3) and not box.any()
    assert g.shape == (3, 1, 36) and (g == 1.0).all()
    # an untiled axis takes any stride: it has no seams to place
    box, g = tile_plan((4, 16, 16), (4, 16, 16), (99, 0, -3), "uniform", (0, 0, 0), 1)
    assert box.shape == (1, 1, 3) and (g == 1.0).all()


def test_per_axis_tables_equal_window_plan():
    from dynamicrafter_amd.lvdm.models.samplers.tiles import tile_plan
    from dynamicrafter_amd.lvdm.models.samplers.windows import window_plan
    S = 4
    box, g = tile_plan((8, 16, 40), (4, 16, 16), (2, 8, 8), "triangle", (1, 0, 3), S)
    st, wt = window_plan(8, 4, 2, "triangle", 1, S)
    sx, wx = window_plan(40, 16, 8, "triangle", 3, S)
    for i in range(S):
        live_t = [w for w in range(st.shape[1]) if wt[i, w].any()]
        live_x = [w for w in range(sx.shape[1]) if wx[i, w].any()]
        k = 0
        for a in live_t:
            for c in live_x:
                assert tuple(box[i, k]) == (st[i, a], 0, sx[i, c])
                assert np.array_equal(g[i, k, :4], wt[i, a]) and (g[i, k, 4:20] == 1.0).all()
                assert np.array_equal(g[i, k, 20:], wx[i, c])
                k += 1
        assert not g[i, k:].any()


def test_padding_boxes_have_weight_zero():
    from dynamicrafter_amd.lvdm.models.samplers.tiles import check_tiles, pad_tiles, tile_plan
    # shift 3 at stride 8 on a width of 40: steps need 4 or 5 boxes along x
    box, g = tile_plan((4, 16, 40), (4, 16, 16), (1, 8, 8), "triangle", (0, 0, 3), 4)
    counts = [int(g[i].any(axis=1).sum()) for i in range(4)]
    assert min(counts) < max(counts) == box.shape[1]
    for i, n in enumerate(counts):
        assert g[i, :n].any(axis=1).all() and not g[i, n:].any()
        assert (box[i, n:] == box[i, n - 1]).all()
    b3, g3 = tile_plan((4, 16, 40), (4, 16, 16), (1, 8, 8), "triangle", (0, 0, 3), 4, multiple_of=3)
    assert b3.shape[1] == 6 and np.array_equal(b3[:, :5], box) and not g3[:, 5:].any()
    assert (b3[:, 5] == b3[:, 4]).all()
    b2, g2 = pad_tiles(box, g, 2)
    assert np.array_equal(b2, b3) and np.array_equal(g2, g3)
    assert check_tiles(b3, g3, (4, 16, 40), (4, 16, 16)) == (4, 6)


def test_refusals_name_their_values():
    from dynamicrafter_amd.lvdm.models.samplers.tiles import check_box, check_tiles, tile_plan, tiles_from_pixels
    ok = dict(long_shape=(4, 24, 32), box_shape=(4, 16, 16), stride=(1, 8, 8), weights="triangle", shift=(0, 0, 0), S=2)
    for change, match in ((dict(box_shape=(4, 32, 16)), "box extent 32 along height exceeds the latent's 24"),
                          (dict(box_shape=(8, 16, 16)), "box extent 8 along time exceeds the latent's 4"),
                          (dict(stride=(1, 0, 8)), "stride 0 along height"),
                          (dict(stride=(1, 8, 17)), "stride 17 along width must be in 1 .. 16"),
                          (dict(shift=(0, -1, 0)), "shift along height must be >= 0, got -1"),
                          (dict(weights="gauss"), "'gauss'"),
                          (dict(S=0), "S = 0")):
        with pytest.raises(ValueError, match=match):
            tile_plan(**dict(ok, **change))
    with pytest.raises(ValueError, match="20 x 16 latent positions .* multiples of 8"):
        check_box((20, 16), 8)
    assert check_box((16, 24), 8) == (16, 24)
    with pytest.raises(ValueError, match=r"--tile \(576, 1020\) must be multiples of 8"):
        tiles_from_pixels(dict(size=(576, 1020), stride=None, shift=(0, 0)), 8)
    with pytest.raises(ValueError, match=r"--tile_shift \(0, 4\)"):
        tiles_from_pixels(dict(size=(576, 1024), stride=None, shift=(0, 4)), 8)
    assert tiles_from_pixels(dict(size=(576, 1024), stride=(288, 512), shift=(0, 8)), 8) == \
        dict(size=(72, 128), stride=(36, 64), shift=(0, 1))
    # check_tiles on tables a kernel must not see
    box, g = tile_plan(**ok)
    bad = box.copy(); bad[0, 0, 2] = 17
    with pytest.raises(ValueError, match=r"starts along width span \[0, 17\], a box of 16 must start in \[0, 16\]"):
        check_tiles(bad, g, (4, 24, 32), (4, 16, 16))
    bad = box.copy(); bad[1, 1, 1] = -1
    with pytest.raises(ValueError, match="starts along height"):
        check_tiles(bad, g, (4, 24, 32), (4, 16, 16))
    for v, match in ((np.nan, "finite"), (-0.5, "finite and >= 0"), (0.25, "do not sum to 1")):
        bg = g.copy(); bg[0, 0, 5] = v
        with pytest.raises(ValueError, match=match):
            check_tiles(box, bg, (4, 24, 32), (4, 16, 16))
    with pytest.raises(ValueError, match="are not"):
        check_tiles(box, g[:, :, :-1], (4, 24, 32), (4, 16, 16))


def test_sampler_refuses_before_the_gpu():
    """Partial runs and an inversion refuse tiles, as they refuse windows."""
    import torch
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from tests.test_options_cpu import _CpuModel, _Net
    s = DDIMSampler(_CpuModel(_Net()))
    s.make_schedule(4, verbose=False)
    x = torch.zeros(1, 4, 4, 24, 32)
    with pytest.raises(ValueError, match="tiled .* inversion is not defined"):
        s.encode(x, None, 2, tiles=dict(size=(16, 16)))


def test_harness_refusals_before_the_gpu():
    """image_guided_synthesis: loop / interp stay refused when time is tiled too; the autoencoder's buffer limit is named."""
    import types
    from dynamicrafter_amd.scripts.evaluation.inference import check_ae_extent, image_guided_synthesis
    for kw in (dict(loop=True), dict(interp=True)):
        with pytest.raises(ValueError, match="tiles with window_stride = 8 cannot be combined"):
            image_guided_synthesis(object(), ["x"], None, [1, 4, 16, 72, 256], window_stride=8, tiles=dict(size=(72, 128)), **kw)
    ae = types.SimpleNamespace(ddconfig=dict(ch=128, ch_mult=[1, 2, 4, 4]))
    frame_by_frame = types.SimpleNamespace(first_stage_model=ae, perframe_ae=True, ae_frames_per_call=1)
    all_at_once = types.SimpleNamespace(first_stage_model=ae, perframe_ae=False)
    check_ae_extent(frame_by_frame, [1, 4, 16, 72, 256])                 # 576 x 2048, one frame per call: 3.0e8 elements
    check_ae_extent(frame_by_frame, [1, 4, 16, 128, 128])
    with pytest.raises(ValueError, match="2\\^31-element buffer limit at 256 channels"):
        check_ae_extent(all_at_once, [1, 4, 16, 72, 256])
    with pytest.raises(ValueError, match="216 x 256 = 55296 positions .* h w <= 46340"):
        check_ae_extent(frame_by_frame, [1, 4, 16, 216, 256])
    check_ae_extent(types.SimpleNamespace(), [1, 4, 16, 216, 256])      # a model without this autoencoder: nothing to check


# ------------------------------------------------------------------ 2. the option entry
def test_tiles_option_flags_round_trip():
    from dynamicrafter_amd.lvdm.models.samplers import options
    from dynamicrafter_amd.lvdm.models.samplers.tiles import tiles_config, tiles_from_pixels
    from dynamicrafter_amd.scripts.evaluation import inference
    opt = options.EXTENT_OPTIONS["tiles"]
    assert opt.kind == options.RUN_SETTING and list(options.all_options())[-1] == "tiles"
    assert list(opt.keys) == ["size", "stride", "weights", "shift", "per_call"]
    p = inference.get_parser()
    assert options.from_args("tiles", p.parse_args([])) is None
    args = p.parse_args(["--tile", "576", "1024", "--tile_stride", "288", "256", "--tile_shift", "8", "16"])
    px = options.from_args("tiles", args)
    assert px == dict(size=(576, 1024), stride=(288, 256), shift=(8, 16)) == options.options_from_args(args)["tiles"]
    cfg = tiles_config(tiles_from_pixels(px, 8), opt.keys)
    assert cfg == dict(size=(72, 128), stride=(36, 32), weights="triangle", shift=(1, 2), per_call=None)
    assert tiles_config(dict(size=(16, 24)), opt.keys)["stride"] == (8, 12)       # the default: half a tile per axis
    with pytest.raises(ValueError, match="--tile_stride needs --tile"):
        options.from_args("tiles", p.parse_args(["--tile_stride", "8", "8"]))
    with pytest.raises(ValueError, match=r"unknown keys \['sizes'\]"):
        options.check_keys(opt, dict(sizes=(16, 16)))
    with pytest.raises(ValueError, match="size must be"):
        tiles_config(dict(stride=(8, 8)), opt.keys)
    # every harness function names it and documents it from the table
    import inspect
    from dynamicrafter_amd.scripts.evaluation import edit, funcs
    from dynamicrafter_amd.scripts.gradio.dynamicrafter_pipeline import DynamiCrafterImg2VideoPipeline
    for fn in (inference.image_guided_synthesis, funcs.batch_ddim_sampling, edit.video_guided_synthesis,
               DynamiCrafterImg2VideoPipeline.__call__):
        assert inspect.signature(fn).parameters["tiles"].default is None and opt.doc in fn.__doc__, fn.__qualname__
    assert options.fold(dict(x_T=None), tiles=dict(size=(16, 16)), apg=None) == dict(x_T=None, tiles=dict(size=(16, 16)))


# ------------------------------------------------------------------ 3. the chunk cap
@pytest.mark.parametrize("res,hw,caps", [("256", (32, 32), (102, 51, 34)), ("512", (40, 64), (40, 20, 13)),
                                         ("1024", (72, 128), (11, 5, 3))])
def test_chunk_cap_generalisation_returns_todays_numbers(res, hw, caps):
    """max_windows_per_call with hw=: the numbers tests/test_windows_cpu.py pins, recomputed for a latent larger than the
    box through the new argument; without it, the old call."""
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
    assert model.model.diffusion_model.spatial_multiple() == 8
    h, w = hw
    for nb, cap in zip((1, 2, 3), caps):
        assert model.max_windows_per_call((1, 4, 32, h, w), nb, 16) == cap
        assert model.max_windows_per_call((1, 4, 32, h, w), nb, 16, hw=hw) == cap
        assert model.max_windows_per_call((1, 4, 16, 2 * h, 3 * w), nb, 16, hw=hw) == cap      # the box counts, not the latent
        assert cap == (2 ** 31 - 1) // (16 * h * w * 1280) // nb
    assert model.max_windows_per_call((2, 4, 32, 4 * h, w), 2, 16, hw=hw) == caps[1] // 2
    with pytest.raises(ValueError, match="2\\^31"):
        model.max_windows_per_call((1, 4, 32, 1024, 1024), 2, 16, hw=(512, 512))
    assert model.max_windows_per_call((1, 4, 32, 64, 64), 1, 16, hw=(2, 2)) == (2 ** 31 - 1) // (16 * 93 * 5120)


# ------------------------------------------------------------------ 4. the C entries refuse bad arguments on the host
def test_tile_cabi_argument_errors_without_gpu():
    """Return codes, no launch: null pointers are DC_ERR_ARG (-2), geometry is DC_ERR_SHAPE (-1). The pointers are never
    dereferenced on the host."""
    import ctypes as C
    from dynamicrafter_amd import _hip
    lib = _hip.lib()
    p = C.c_void_p(256)
    #            index S  W  w0 n_w B  Cx Cc TL  HL  WL  T  H   Wd  c_pad nrep
    good_pack = [0,    2, 6, 0, 6,  1, 4, 4, 4,  24, 32, 4, 16, 16, 64,   1]
    assert lib.dc_pack_latent_tiles(None, p, p, p, None, *good_pack, None) == -2
    assert lib.dc_pack_latent_tiles(p, p, p, None, None, *good_pack, None) == -2
    assert lib.dc_pack_latent_tiles(p, None, p, p, None, *good_pack, None) == -2          # Cc > 0 without cc
    for pos, v in ((0, 2), (0, -1), (3, 1), (4, 0), (4, 7), (9, 15), (10, 8), (11, 5), (14, 60), (14, 4), (15, 0), (6, 0),
                   (5, 0), (1, 0)):
        args = list(good_pack); args[pos] = v
        assert lib.dc_pack_latent_tiles(p, p, p, p, None, *args, None) == -1, (pos, v)
    #             index S  W  w0 n_w nb B  C  TL  HL  WL  T  H   Wd  accumulate
    good_merge = [1,    2, 6, 2, 4,  2, 1, 4, 4,  24, 32, 4, 16, 16, 0]
    assert lib.dc_tile_merge(None, 4, p, 4, p, p, None, *good_merge, None) == -2
    assert lib.dc_tile_merge(p, 4, p, 4, p, None, None, *good_merge, None) == -2
    assert lib.dc_tile_merge(p, 3, p, 4, p, p, None, *good_merge, None) == -1              # ld_e < C
    assert lib.dc_tile_merge(p, 4, p, 2, p, p, None, *good_merge, None) == -1              # ld_out < C
    for pos, v in ((0, 2), (3, 3), (4, 0), (5, 0), (6, 0), (7, 0), (8, 3), (12, 25), (13, 33), (2, 0)):
        args = list(good_merge); args[pos] = v
        assert lib.dc_tile_merge(p, 4, p, 4, p, p, None, *args, None) == -1, (pos, v)
    # extents whose row count leaves int32: refused, not wrapped
    big = list(good_merge); big[8:14] = [64, 8192, 8192, 4, 16, 16]
    assert lib.dc_tile_merge(p, 4, p, 4, p, p, None, *big, None) == -1

"""The float image resize on the GPU (dc_resize_f32_h / dc_resize_f32_finish through ops.resize_f32) against
torch.nn.functional.interpolate run on the CPU, on the shape pairs of tests/resize_f32_restatement.CASES, with antialias both
ways and 1, 3 and 4 channels. Inputs are uniform in [-1, 1] (np.random.default_rng(0)).

Tolerance (resize_f32_restatement.TOL = 2e-5 max abs): |x| <= 1, the weights of an output sum to 1 and a pass has at most
2 * ceil(8) + 1 = 17 taps at the largest scale used here (8), so a pass rounds by about 20 * 2^-23; two passes, and torch's own
rounding doubles it. It does not hold beyond scale 8."""
import functools

import numpy as np
import pytest
import torch

from tests import resize_f32_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7777.0
GUARD = 64
_ids = [c[0] for c in R.CASES]


@functools.lru_cache(maxsize=None)
def _reference(name, c, antialias):
    """(image, torch-CPU result) of a case, computed once."""
    _, hw, resized, crop, offset = next(k for k in R.CASES if k[0] == name)
    img = R.make_image(c, hw[0], hw[1])
    ref = R.torch_reference(img, resized, crop, offset, antialias)
    img.setflags(write=False); ref.setflags(write=False)
    return img, ref


def _guarded(shape):
    """A sentinel-filled buffer and the view of `shape` in its middle."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


@pytest.mark.parametrize("antialias", [True, False], ids=["aa", "noaa"])
@pytest.mark.parametrize("case", R.CASES, ids=_ids)
def test_resize_f32_matches_torch_cpu(case, antialias):
    from dynamicrafter_amd import ops
    name, hw, resized, crop, offset = case
    for c in R.CHANNELS:
        img, ref = _reference(name, c, antialias)
        src = torch.from_numpy(np.array(img)).to(DEV)
        out = ops.resize_f32(src, resized, crop_hw=crop, offset=offset, antialias=antialias)
        assert out.shape == ref.shape and out.dtype == torch.float32 and out.device == torch.device(DEV)
        got = out.cpu().numpy()
        err = float(np.abs(got - ref).max())
        print(f"{name} C={c} antialias={antialias}: max abs error vs torch CPU {err:.3g}")
        assert err <= R.TOL
        if crop is not None:                                                  # the padding is exactly 0.0
            pad = np.ones(ref.shape[1:], dtype=bool)
            pad[max(-offset[0], 0):resized[0] - offset[0], max(-offset[1], 0):resized[1] - offset[1]] = False
            assert pad.any() and (got[:, pad] == 0.0).all() and not np.signbit(got[:, pad]).any()
        # into a caller's tensor: the same values, nothing written outside it
        buf, view = _guarded(ref.shape)
        assert ops.resize_f32(src, resized, crop_hw=crop, offset=offset, antialias=antialias, out=view) is view
        torch.cuda.synchronize()
        b = buf.cpu()
        assert (b[:GUARD] == SENT).all() and (b[-GUARD:] == SENT).all(), "resize_f32 wrote outside out"
        assert torch.equal(view, out)
        assert torch.equal(src.cpu(), torch.from_numpy(np.array(img)))        # the input is not touched


def test_crop_inside_and_window_off_the_image():
    """A crop smaller than the resized image (the intermediate holds only what it keeps), and a window that misses it."""
    from dynamicrafter_amd import ops
    img = R.make_image(3, 37, 53)
    src = torch.from_numpy(img).to(DEV)
    for antialias in (True, False):
        ref = R.torch_reference(img, (16, 24), (7, 9), (5, 11), antialias)
        out = ops.resize_f32(src, (16, 24), crop_hw=(7, 9), offset=(5, 11), antialias=antialias)
        assert float(np.abs(out.cpu().numpy() - ref).max()) <= R.TOL
    out = ops.resize_f32(src, (16, 24), crop_hw=(4, 4), offset=(16, 0))
    assert (out == 0.0).all()


def test_staged_and_direct_horizontal_pass_give_the_same_bits():
    """The two forms of dc_resize_f32_h on two tiles (300 columns, the second one partial) and on a window of columns that
    starts inside the first tile."""
    from dynamicrafter_amd import ops
    src = torch.from_numpy(R.make_image(2, 12, 700)).to(DEV)
    tab = ops.ResizeTablesF32(700, 300, True, DEV)
    assert ops.resize_f32_h_seg(tab, 0, 300) > 0
    for y0, rows, x0, cols in ((0, 12, 0, 300), (3, 7, 41, 259)):
        outs = []
        for staged in (True, False):
            buf, view = _guarded((2, rows, cols))
            ops.resize_f32_h(src, view, tab, y0=y0, rows=rows, x0=x0, cols=cols, staged=staged)
            torch.cuda.synchronize()
            assert (buf[:GUARD] == SENT).all() and (buf[-GUARD:] == SENT).all()
            outs.append(view.clone())
        assert torch.equal(outs[0], outs[1])
        k, xmin, n = R.coeffs(700, 300, True)
        ref = R.one_pass(src.cpu().numpy()[:, y0:y0 + rows], k, xmin, n, axis=2)[:, :, x0:x0 + cols]
        assert float(np.abs(outs[0].cpu().numpy() - ref).max()) <= R.TOL


def test_horizontal_pass_at_the_lds_threshold():
    """Scale 30 (61 taps) is the last whose tile fits the LDS form, scale 31 (63 taps) the first that takes the direct one. Beyond
    scale 8 the tolerance follows the tap count as in the module docstring: 4 * (ksize + 3) * 2^-23."""
    from dynamicrafter_amd import ops
    for scale, staged in ((30, True), (31, False)):
        tab = ops.ResizeTablesF32(16 * scale, 16, True, DEV)
        assert (ops.resize_f32_h_seg(tab, 0, 16) > 0) == staged
        img = R.make_image(1, 2 * scale, 16 * scale)
        out = ops.resize_f32(torch.from_numpy(img).to(DEV), (2, 16)).cpu().numpy()
        tol = 4 * (tab.ksize + 3) * 2.0 ** -23
        assert float(np.abs(out - R.torch_reference(img, (2, 16))).max()) <= tol
    with pytest.raises(ValueError):
        ops.resize_f32_h(torch.zeros(1, 62, 496, device=DEV), torch.empty(62 * 16, device=DEV), tab, y0=0, rows=62, x0=0, cols=16,
                         staged=True)


def test_bad_arguments_raise():
    from dynamicrafter_amd import ops
    src = torch.zeros(3, 37, 53, device=DEV)
    buf, view = _guarded((3, 16, 24))
    with pytest.raises(ValueError):                   # a crop window larger than the output tensor
        ops.resize_f32(src, (16, 24), crop_hw=(16, 30), out=view)
    with pytest.raises(ValueError):                   # another channel count
        ops.resize_f32(src[:1], (16, 24), out=view)
    with pytest.raises(ValueError):                   # tables built for another size
        ops.resize_f32_finish(src, view, ops.ResizeTablesF32(53, 20, True, DEV), axis=1, src_hw=(37, 53), origin=(0, 0),
                              resized=(37, 24), offset=(0, 0))
    with pytest.raises(ValueError):                   # tables for another source width
        ops.resize_f32_h(src, torch.empty(3 * 37 * 24, device=DEV), ops.ResizeTablesF32(50, 24, True, DEV), y0=0, rows=37, x0=0,
                         cols=24)
    with pytest.raises(ValueError):                   # an intermediate that does not hold the rows the vertical pass reads
        ops.resize_f32_finish(torch.empty(3, 10, 24, device=DEV), view, ops.ResizeTablesF32(37, 16, True, DEV), axis=2,
                              src_hw=(10, 24), origin=(0, 0), resized=(16, 24), offset=(0, 0))
    with pytest.raises(ValueError):                   # a workspace too small
        ops.resize_f32_h(src, torch.empty(10, device=DEV), ops.ResizeTablesF32(53, 24, True, DEV), y0=0, rows=37, x0=0, cols=24)
    with pytest.raises(RuntimeError):                 # a CPU tensor
        ops.resize_f32(torch.zeros(3, 37, 53), (16, 24))
    with pytest.raises(RuntimeError):
        ops.resize_f32(src, (16, 24), out=torch.empty(3, 16, 24))
    torch.cuda.synchronize()
    assert (buf == SENT).all(), "a refused call launched"

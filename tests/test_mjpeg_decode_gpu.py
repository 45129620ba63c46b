"""Motion-JPEG input on the GPU: the three dc_jpeg_decode_* launches against the numpy restatement of the decoder
(tests/jpeg_decode_restatement.py; its own standing against libjpeg is tests/test_mjpeg_decode_cpu.py) - coefficients word for
word, pixels within one level of the float64 arithmetic - then the round trip through the package's own encoder, streams that
must be refused, funcs.load_video_batch / load_image_batch end to end, and the launches inside a captured graph.

Inputs: tests/mjpeg_decode_cases.py (16x16 = one MCU, 24x40, 37x53 = odd both ways; "noise" and "smooth" frames)."""
import functools

import numpy as np
import pytest
import torch

from tests import jpeg_decode_restatement as D
from tests import jpeg_restatement as J
from tests.mjpeg_decode_cases import KINDS, LIBJPEG_BOUND, SIZES, frames, libjpeg_distance, pillow_file, pillow_rgb, pixel_batches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PSNR_MARGIN_DB = 0.25       # tests/test_mjpeg_cpu.py: five times the float64 restatement's largest shortfall against libjpeg
_ids = lambda s: f"{s[0]}x{s[1]}" if isinstance(s, tuple) else str(s)


def run_batch(files, planar=False):
    """The three launches on `files` (one geometry) with sentinels behind every output; nothing raises on a bad segment.
    Returns (coef int16 [T, my, mx, bpm, 64], status int32 [n_seg], frame_seg, out as numpy)."""
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.utils import load_video as L
    infos = [L.parse_jpeg(f) for f in files]
    W, H, ncomp, hs, vs = infos[0].geometry()
    assert all(i.geometry() == infos[0].geometry() for i in infos)
    my, mx, bpm, per_frame = ops.jpeg_decode_geometry(H, W, ncomp, hs, vs)
    T = len(files)
    buf, layout = L.pack_jpeg_batch(files, infos)
    n_seg = layout["seg"][1]
    dev_buf = torch.from_numpy(buf).to(DEV)
    coef = torch.full((T * per_frame + 64,), -7777, dtype=torch.int16, device=DEV)
    planes = torch.full((T * per_frame + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    status = torch.full((n_seg + 4,), -7, dtype=torch.int32, device=DEV)
    n_out = T * H * W * 3
    out = torch.full((n_out + 64,), 77, dtype=torch.float32 if planar else torch.uint8, device=DEV)
    L.launch_jpeg_decode(dev_buf, layout, coef, planes, status, out, T=T, H=H, W=W, ncomp=ncomp, hs=hs, vs=vs)
    torch.cuda.synchronize()
    c, p, s, o = coef.cpu().numpy(), planes.cpu().numpy(), status.cpu().numpy(), out.cpu().numpy()
    assert (c[T * per_frame:] == -7777).all(), "dc_jpeg_decode_entropy wrote past the coefficients"
    assert (p[T * per_frame:] == 0xA5).all(), "dc_jpeg_decode_idct wrote past the planes"
    assert (s[n_seg:] == -7).all() and (s[:n_seg] >= 0).all(), "status words"
    assert (o[n_out:] == 77).all(), "dc_jpeg_decode_output wrote past its output"
    o = o[:n_out].reshape((T, 3, H, W) if planar else (T, H, W, 3))
    fs = buf[layout["frame_seg"]:layout["frame_seg"] + 4 * (T + 1)].view(np.int32)
    return c[:T * per_frame].reshape(T, my, mx, bpm, 64), s[:n_seg], fs, o


@functools.lru_cache(maxsize=None)
def ref_coef(data):
    c = D.coefficients(data)
    c.setflags(write=False)
    return c


def check_coefficients(files):
    coef, status, _, _ = run_batch(files)
    assert not status.any(), status
    for t, data in enumerate(files):
        ref = ref_coef(data)
        assert coef[t].shape == ref.shape
        bad = np.argwhere(coef[t] != ref)
        assert bad.size == 0, f"frame {t}: {len(bad)} coefficients differ, the first at (my, mx, block, k) = {bad[0].tolist()}"
    return coef


# ------------------------------------------------------------------------------------------------ 1. entropy stage, exact
@pytest.mark.parametrize("ri", [1, 3, "frame"])
@pytest.mark.parametrize("hw", SIZES, ids=_ids)
def test_coefficients_of_the_encoder_restatements_files(hw, ri):
    """Two frames per batch (noise, smooth) at qualities 50 and 100. 37x53 at ri = 1 has 12 intervals: RST7 wraps to RST0."""
    my, mx = J.mcu_grid(*hw)
    r = my * mx if ri == "frame" else ri
    for q in (50, 100):
        files = [J.encode(frames(kind, hw), q, ri=r)[0] for kind in KINDS]
        coef = check_coefficients(files)
        for t, kind in enumerate(KINDS):                          # and they are what the encoder put in
            assert np.array_equal(coef[t], J.coefficients(frames(kind, hw), J.quant_tables(q))[0])
    if hw == (37, 53) and ri == 1:
        assert b"\xff\xd7" in files[0] and files[0].count(b"\xff\xd0") >= 2


@pytest.mark.parametrize("mode", [0, 1, 2, "L"], ids=["444", "422", "420", "grey"])
def test_coefficients_of_pillows_files(mode):
    """No DRI (one lane decodes the frame), optimised Huffman tables, restart intervals in libjpeg's MCU-row units, in every
    sampling; a batch mixes them, so the tables differ from frame to frame."""
    for hw in SIZES:
        f = frames("noise", hw)[0]
        files = [pillow_file(f, mode, 90, optimize=False), pillow_file(f, mode, 90, optimize=True),
                 pillow_file(f, mode, 50, optimize=True, rst=1), pillow_file(frames("smooth", hw)[0], mode, 100, optimize=True, rst=3)]
        assert D.parse(files[0])["huff"] != D.parse(files[1])["huff"] and D.parse(files[0])["ri"] == 0
        check_coefficients(files)


def hand_made(name):
    """Coefficient blocks [2, 3, 5, 6, 64] for a 48x80 4:2:0 frame (3 x 5 MCUs), T = 2."""
    shape = (2, 3, 5, 6, 64)
    c = np.zeros(shape, dtype=np.int16)
    if name == "zeros":                          # DC category 0 and EOB only
        pass
    elif name == "zrl":                          # runs of 16 .. 62 zeros in front of a value, and EOB behind it
        for b in range(6):
            c[:, :, :, b, 17 + 9 * b] = 5 - b
        c[1, ..., 33] = -2
    elif name == "last":                         # a non-zero coefficient 63: three ZRLs, run 14, no EOB
        c[..., 63] = 1
        c[1, ..., 63] = -3
    elif name == "longest":                      # AC +-1023 (category 10); the DC of each component alternates -1024 / +1016
        c[..., 1::2] = 1023                      # from one of its blocks to the next: differences of category 11
        c[..., 2::2] = -1023
        m = np.arange(15).reshape(3, 5)
        for b in range(4):
            c[:, :, :, b, 0] = np.where((4 * m + b) % 2 == 0, -1024, 1016)
        c[:, :, :, 4:, 0] = np.where(m % 2 == 0, -1024, 1016)[None, :, :, None]
    elif name == "random":                       # dense blocks: code bytes of FF, so stuffing
        c = np.random.default_rng(1).integers(-1023, 1024, size=shape).astype(np.int16)
    return c


@pytest.mark.parametrize("ri", [1, 4, 15])
@pytest.mark.parametrize("name", ["zeros", "zrl", "last", "longest", "random"])
def test_coefficients_of_hand_made_blocks(name, ri):
    coef = hand_made(name)
    q = J.quant_tables(90)
    files = [J.jfif(J.entropy_scan(coef[t], ri), 48, 80, q, ri) for t in range(2)]
    if name == "random":
        assert all(b"\xff\x00" in f[f.index(b"\xff\xda"):] for f in files)
    if name == "longest":
        assert int(np.abs(np.diff(coef[0, 0, :, 4, 0].astype(np.int32))).max()) == 2040          # category 11
    got, status, _, _ = run_batch(files)
    assert not status.any(), status
    assert np.array_equal(got, coef)
    assert np.array_equal(ref_coef(files[0]), coef[0])            # the restatement reads them the same way


# ------------------------------------------------------------------------------------------------ 2. pixels
@pytest.mark.parametrize("mode", [0, 1, 2, "L"], ids=["444", "422", "420", "grey"])
def test_pixels_against_the_float64_restatement(mode):
    """The coefficients are exact (above), so this is the pixel stage alone: no sample may differ from the float64 restatement
    by more than 1 level, and at most 1 in 1000 of the mode's samples may differ at all (the float32 restatement differs in at
    most 1 of 114 372 on these files: test_mjpeg_decode_cpu.py). The fp32 planar output holds exactly the uint8 output."""
    differ = total = 0
    for hw, files in pixel_batches(mode):
        coef, status, _, got = run_batch(files)
        assert not status.any()
        planar = run_batch(files, planar=True)[3]
        assert planar.dtype == np.float32 and np.array_equal(planar, got.transpose(0, 3, 1, 2).astype(np.float32))
        for t, data in enumerate(files):
            ref = D.pixels(data, np.float64, ref_coef(data))
            d = np.abs(got[t].astype(np.int32) - ref.astype(np.int32))
            assert d.max() <= 1, f"{hw} file {t}: a sample differs by {int(d.max())}"
            differ += int((d != 0).sum())
            total += d.size
    print(f"mode {mode}: {differ} of {total} samples differ from the float64 restatement")
    assert differ <= total // 1000


# ------------------------------------------------------------------------------------------------ 3. round trip
@pytest.mark.parametrize("hw", [(40, 72), (33, 17)], ids=_ids)
@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_through_the_packages_encoder(kind, hw):
    """encode_jpeg_frames -> decode_jpeg_frames at quality 90: within the libjpeg bound of test_mjpeg_decode_cpu.py of Pillow
    decoding the same bytes, and a PSNR against the source within PSNR_MARGIN_DB of Pillow's."""
    from dynamicrafter_amd.utils import load_video as L
    from dynamicrafter_amd.utils import save_video as S
    src = frames(kind, hw, 2)
    files = S.encode_jpeg_frames(torch.from_numpy(np.array(src)).to(DEV), quality=90)
    got = L.decode_jpeg_frames(files, device=DEV)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2,) + hw + (3,) and got.device == torch.device(DEV)
    got = got.cpu().numpy()
    cap_max, cap_share = LIBJPEG_BOUND[2]
    for t in range(2):
        ref = pillow_rgb(files[t])
        mx, share = libjpeg_distance(got[t], ref)
        ours, theirs = J.psnr(got[t], src[t]), J.psnr(ref, src[t])
        print(f"{kind} {hw} frame {t}: max {mx}, share above 1 level {share:.5f}; {ours:.3f} dB, Pillow's decoder {theirs:.3f} dB")
        assert mx <= cap_max and share <= cap_share
        assert abs(ours - theirs) <= PSNR_MARGIN_DB


# ------------------------------------------------------------------------------------------------ 4. bad streams
def _replace_segment(data, k, fn):
    from dynamicrafter_amd.utils import load_video as L
    a, n = L.scan_segments(data, L.parse_jpeg(data))[k].tolist()
    return data[:a] + fn(data[a:a + n]) + data[a + n:]


@pytest.mark.parametrize("damage", ["halved", "no_code"])
def test_bad_segments_raise_and_the_rest_decodes(damage):
    """Frame 1 of 3, segment 5 of 12 (37x53 at ri = 1): its length halved, or its bytes replaced by sixteen 1-bits, which is a
    code of no Annex K table. decode_jpeg_frames raises ValueError naming frame and segment; the launches themselves set that
    segment's status and nothing else, and every other frame decodes as it does in a clean batch. The scan bytes of a batch are
    one allocation (with the tables in front), so an over-read in a faulty build would stay inside it."""
    from dynamicrafter_amd.utils import load_video as L
    clean = [J.encode(frames(kind, (37, 53)), 90, ri=1)[0] for kind in ("noise", "smooth", "noise")]
    fn = (lambda s: s[:len(s) // 2]) if damage == "halved" else (lambda s: b"\xff\x00\xff\x00\xff\x00")
    files = [clean[0], _replace_segment(clean[1], 5, fn), clean[2]]
    with pytest.raises(ValueError, match="frame 1 segment 5"):
        L.decode_jpeg_frames(files, device=DEV)
    _, status, fs, got = run_batch(files)
    assert fs.tolist() == [0, 12, 24, 36]
    assert np.flatnonzero(status).tolist() == [12 + 5], status
    if damage == "no_code":
        assert status[17] == 1
    ref = run_batch(clean)[3]
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2])
    assert np.array_equal(got[1, :15], ref[1, :15])               # rows whose luma and chroma lie in the MCU row in front of it
    # a frame of another geometry in the batch is refused on the host
    with pytest.raises(ValueError, match="one geometry"):
        L.decode_jpeg_frames([clean[0], J.encode(frames("noise", (24, 40)), 90)[0]], device=DEV)


# ------------------------------------------------------------------------------------------------ 5. end to end
def _clip(tmp_path, t=6, hw=(24, 40)):
    from dynamicrafter_amd.scripts.evaluation import funcs
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(1, 1, 3, t, hw[0], hw[1], generator=g) * 0.5).to(DEV)
    return funcs.save_videos(x, str(tmp_path / "v"), ["clip"], fps=8, container="avi")[0]


def test_load_video_batch_end_to_end(tmp_path):
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.scripts.evaluation import funcs
    from dynamicrafter_amd.utils import load_video as L
    p = _clip(tmp_path)
    frames_u8, fps = L.read_video(p, device=DEV)
    assert tuple(frames_u8.shape) == (6, 24, 40, 3) and frames_u8.dtype == torch.uint8 and fps == 8.0
    _, _, _, files = L.read_avi_mjpeg(p)
    for t in range(6):                                            # what any other reader sees, within the libjpeg bound
        mx, share = libjpeg_distance(frames_u8[t].cpu().numpy(), pillow_rgb(files[t]))
        assert mx <= LIBJPEG_BOUND[2][0] and share <= LIBJPEG_BOUND[2][1]
    want = ((frames_u8.float() / 255. - 0.5) * 2).permute(3, 0, 1, 2)                           # [3, t, h, w]
    #        stride, video_frames -> frames of the clip
    cases = {(1, 6): [0, 1, 2, 3, 4, 5], (2, 3): [0, 2, 4], (1, 4): [0, 1, 2, 3], (1, 8): [0, 1, 2, 3, 4, 5, 5, 5],
             (2, 5): [0, 2, 4, 4, 4], (1, -1): [0, 1, 2, 3, 4, 5], (2, -1): [0, 1, 2, 2, 2, 2]}
    for (stride, n), idx in cases.items():
        # two clips per call, except where the reference's own rule (video_frames < 0 resets the stride for the files that
        # follow) would give the second clip another length
        paths = [p] if (n < 0 and stride > 1) else [p, p]
        got = funcs.load_video_batch(paths, stride, video_size=(24, 40), video_frames=n)
        assert tuple(got.shape) == (len(paths), 3, len(idx), 24, 40) and got.dtype == torch.float32
        assert got.device == torch.device(DEV) and got.is_contiguous() and float(got.min()) >= -1.0 and float(got.max()) <= 1.0
        assert torch.equal(got[0], want[:, idx]) and torch.equal(got[-1], got[0]), (stride, n)
    # another size: exactly ops.resize_f32(antialias=False) of the decoded planes
    planes = L.decode_jpeg_frames([files[0], files[2]], device=DEV, planar=True)
    assert tuple(planes.shape) == (2, 3, 24, 40) and planes.dtype == torch.float32
    assert torch.equal(planes, frames_u8[[0, 2]].permute(0, 3, 1, 2).float())
    ref = (ops.resize_f32(planes.view(6, 24, 40), (32, 48), antialias=False).view(2, 3, 32, 48) / 255. - 0.5) * 2
    got = funcs.load_video_batch([p], 2, video_size=(32, 48), video_frames=2)
    assert tuple(got.shape) == (1, 3, 2, 32, 48) and torch.equal(got[0], ref.permute(1, 0, 2, 3))
    # load_image_batch: the first frame
    img = funcs.load_image_batch([p, p], (24, 40))
    assert tuple(img.shape) == (2, 3, 24, 40) and torch.equal(img[0], want[:, 0]) and torch.equal(img[1], want[:, 0])
    assert torch.equal(funcs.load_image_batch([p], (32, 48))[0], ref[0])
    with pytest.raises(NotImplementedError):
        funcs.load_video_batch([p, str(tmp_path / "clip.mp4")], 1)


def test_read_video_takes_a_single_jpeg_and_a_grey_clip(tmp_path):
    from dynamicrafter_amd.utils import load_video as L
    from dynamicrafter_amd.utils import save_video as S
    f = frames("smooth", (37, 53), 2)
    grey = [pillow_file(f[t], "L", 90) for t in range(2)]
    p = S.write_avi_mjpeg(str(tmp_path / "grey.avi"), grey, 53, 37, 25)
    got, fps = L.read_video(p, device=DEV)
    assert fps == 25.0 and tuple(got.shape) == (2, 37, 53, 3)
    got = got.cpu().numpy()
    assert (got[..., 0] == got[..., 1]).all() and (got[..., 0] == got[..., 2]).all()
    for t in range(2):
        assert libjpeg_distance(got[t], pillow_rgb(grey[t]))[0] <= LIBJPEG_BOUND["L"][0]
    (tmp_path / "one.jpg").write_bytes(pillow_file(f[0], 1, 90))
    one, fps = L.read_video(str(tmp_path / "one.jpg"), device=DEV)
    assert fps == 0.0 and tuple(one.shape) == (1, 37, 53, 3)
    mx, share = libjpeg_distance(one[0].cpu().numpy(), pillow_rgb(pillow_file(f[0], 1, 90)))
    assert mx <= LIBJPEG_BOUND[1][0] and share <= LIBJPEG_BOUND[1][1]


# ------------------------------------------------------------------------------------------------ 6. capture
def test_decode_launches_replay_from_a_captured_graph():
    """The three entries (and the memset in front of the first) neither allocate nor synchronise: captured once into a graph,
    the replay on another batch copied into the captured buffers gives the bits the eager launches give."""
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.utils import load_video as L
    hw, T = (37, 53), 2
    batches = [[J.encode(frames(kind, hw), q, ri=3)[0] for q in (50, 90)] for kind in ("smooth", "noise")]
    packed = [L.pack_jpeg_batch(b) for b in batches]
    size = max(buf.size for buf, _ in packed)
    layout = dict(packed[0][1])
    assert all(lay["seg"] == layout["seg"] and lay["scan"][0] == layout["scan"][0] for _, lay in packed)
    layout["scan"] = (layout["scan"][0], size - layout["scan"][0])            # the longer of the two scans
    host = [torch.from_numpy(np.concatenate([buf, np.zeros(size - buf.size, np.uint8)])) for buf, _ in packed]
    my, mx, bpm, per_frame = ops.jpeg_decode_geometry(hw[0], hw[1], 3, 2, 2)
    dev_buf = host[0].to(DEV)
    coef = torch.empty(T * per_frame, dtype=torch.int16, device=DEV)
    planes = torch.empty(T * per_frame, dtype=torch.uint8, device=DEV)
    status = torch.empty(layout["seg"][1], dtype=torch.int32, device=DEV)
    out = torch.zeros((T,) + hw + (3,), dtype=torch.uint8, device=DEV)

    def enqueue():
        L.launch_jpeg_decode(dev_buf, layout, coef, planes, status, out, T=T, H=hw[0], W=hw[1], ncomp=3, hs=2, vs=2)

    def result():
        assert not status.cpu().numpy().any()
        return coef.cpu().numpy().copy(), out.cpu().numpy().copy()

    enqueue()
    torch.cuda.synchronize()
    eager_smooth = result()
    assert np.array_equal(eager_smooth[1], L.decode_jpeg_frames(batches[0], device=DEV).cpu().numpy())
    graph = ops.DeviceGraph().capture(enqueue)
    dev_buf.copy_(host[1])                                        # another batch in the captured buffers
    out.zero_(); coef.fill_(-1); status.fill_(-1)
    torch.cuda.synchronize()
    graph.launch()
    graph.sync()
    replay_noise = result()
    enqueue()
    torch.cuda.synchronize()
    eager_noise = result()
    for a, b, c in zip(replay_noise, eager_noise, eager_smooth):
        assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(replay_noise[1], L.decode_jpeg_frames(batches[1], device=DEV).cpu().numpy())

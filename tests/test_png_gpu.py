"""PNG / APNG output with deflate="hip" on the GPU: the three dc_png_* launches against the plain-Python restatement
(tests/png_restatement.py; its own standing against Pillow, zlib and the strict decoder is tests/test_png_cpu.py), the writers end
to end through Pillow and the strict decoder, the save_results harness, and the launches inside a captured graph. Everything here
is integer arithmetic, so every comparison is for equality.

Frames: noise, flat, ramp, photo at 96x160x3, 33x17x3, 1x1x3, 96x160x1, 96x160x4 (T = 3); chunks of 1, 7 and 64 bytes, the whole
frame, the default; 160x160x3 at 65535 (two chunks). Chunks of 1 and 7 bytes on the larger frames run with T = 1 (the reference
is a Python loop over tens of thousands of chunks). Byte planes: P.aimed_planes(). Every output buffer has sentinel elements
behind it and behind each row's reported length."""
import functools
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from tests import png_restatement as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(96, 160, 3), (33, 17, 3), (1, 1, 3), (96, 160, 1), (96, 160, 4)]
KINDS = ["noise", "flat", "ramp", "photo"]
CHUNKS = [1, 7, 64, "frame", None]
SENT = 0xA5
_ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


@functools.lru_cache(maxsize=None)
def _frames(kind, shape):
    f = P.make_frames(kind, 3, *shape)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _planes(kind, shape):
    f = _frames(kind, shape)
    p = np.stack([P.filter_plane(f[t])[0].reshape(-1) for t in range(f.shape[0])])
    p.setflags(write=False)
    return p


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. filters
def _gpu_filter(frames):
    from dynamicrafter_amd import ops
    T, H, W, C = frames.shape
    n = T * H * (1 + W * C)
    planes = torch.full((n + 64,), SENT, dtype=torch.uint8, device=DEV)
    ops.png_filter(_dev(frames), planes)
    torch.cuda.synchronize()
    got = planes.cpu().numpy()
    assert (got[n:] == SENT).all(), "dc_png_filter wrote past its output"
    return got[:n].reshape(T, H, 1 + W * C)


@pytest.mark.parametrize("shape", SHAPES + [(160, 160, 3)], ids=_ids)
@pytest.mark.parametrize("kind", KINDS)
def test_filter_equals_the_restatement(kind, shape):
    f = _frames(kind, shape)
    got = _gpu_filter(f)
    for t in range(f.shape[0]):
        ref, _ = P.filter_plane(f[t])
        assert (got[t, :, 0] == ref[:, 0]).all(), f"frame {t}: filter types differ"
        assert (got[t] == ref).all(), f"frame {t}: residuals differ"
    if kind == "photo" and shape == (96, 160, 3):
        assert len(set(got[:, :, 0].reshape(-1).tolist())) >= 3                  # the choice really varies from row to row


def test_filter_ties_go_to_the_lowest_type():
    """Zeros: all five filters cost 0 -> type 0. A constant row over a zero row: Sub (1) and Paeth (4) both cost the first pixel
    only, None and Up the whole row -> 1. The same row again below it: Up (2) and Paeth (4) both cost 0 -> 2. One non-zero
    pixel at the start of a top row: None and Up (over the zero row) cost that pixel, Sub and Paeth also the one behind it -> 0."""
    f = np.zeros((2, 4, 70, 3), dtype=np.uint8)
    f[0, 1:] = 200
    f[1, 0, 0] = 9
    got = _gpu_filter(f)
    for t in range(2):
        ref, cost = P.filter_plane(f[t])
        assert (got[t] == ref).all()
    _, cost = P.filter_plane(f[0])
    assert cost[0].tolist() == [0] * 5 and got[0, 0, 0] == 0
    assert cost[1, 1] == cost[1, 4] == cost[1].min() and got[0, 1, 0] == 1
    assert cost[2, 2] == cost[2, 4] == 0 < cost[2, 1] and got[0, 2, 0] == 2
    _, cost = P.filter_plane(f[1])
    assert cost[0, 0] == cost[0, 2] == cost[0].min() > 0 and got[1, 0, 0] == 0


# ------------------------------------------------------------------------------------------------ 2. deflate + pack
def _deflate_and_pack(planes, chunk, frame_stride=None):
    """Runs dc_png_deflate and dc_png_pack on planes uint8 [T, N] with sentinels behind every buffer and checks them against the
    restatement: chunk strings, lengths, Adler values, offsets, packed streams, frame_len. Returns (streams, lens)."""
    from dynamicrafter_amd import ops
    T, N = planes.shape
    chunk = ops.PNG_CHUNK if chunk is None else chunk
    cpf = (N + chunk - 1) // chunk
    n_ch = T * cpf
    stride = ops.png_chunk_max_bytes(min(chunk, N))
    scratch = torch.full((n_ch * stride + 64,), SENT, dtype=torch.uint8, device=DEV)
    chunk_len, chunk_adler, chunk_off = (torch.full((n_ch + 4,), -7, dtype=torch.int32, device=DEV) for _ in range(3))
    frame_len = torch.full((T + 4,), -7, dtype=torch.int32, device=DEV)
    assert ops.png_deflate(_dev(planes).reshape(-1), scratch, chunk_len, chunk_adler, T=T, N=N, chunk=chunk, stride=stride) == n_ch
    torch.cuda.synchronize()
    ref = [P.plane_chunks(planes[t].tobytes(), chunk) for t in range(T)]
    flat = [r for fr in ref for r in fr]
    cl = chunk_len.cpu().numpy()
    assert (cl[n_ch:] == -7).all() and cl[:n_ch].tolist() == [len(s) for s, _, _ in flat], "chunk lengths differ"
    ca = chunk_adler.cpu().numpy()
    assert (ca[n_ch:] == -7).all() and ca[:n_ch].view(np.uint32).tolist() == [a for _, _, a in flat], "chunk Adler values differ"
    sc = scratch.cpu().numpy()
    assert (sc[n_ch * stride:] == SENT).all(), "dc_png_deflate wrote past the scratch buffer"
    want = np.full((n_ch, stride), SENT, dtype=np.uint8)
    for i, (s, _, _) in enumerate(flat):
        want[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    bad = np.flatnonzero((sc[:n_ch * stride].reshape(n_ch, stride) != want).any(1))
    assert bad.size == 0, f"chunk strings differ (or bytes were written past their length) in chunks {bad[:8].tolist()}"
    streams = [P.zlib_stream(planes[t].tobytes(), chunk) for t in range(T)]
    lens = [len(s) for s in streams]
    fs = frame_stride or ops.png_frame_max_bytes(N, chunk)
    out = torch.full((T * fs + 64,), SENT, dtype=torch.uint8, device=DEV)
    ops.png_pack(scratch, chunk_len, chunk_adler, chunk_off, out, frame_len, T=T, N=N, chunk=chunk, stride=stride, frame_stride=fs)
    torch.cuda.synchronize()
    fl = frame_len.cpu().numpy()
    assert (fl[T:] == -7).all() and fl[:T].tolist() == lens, "frame_len differs"
    co = chunk_off.cpu().numpy()
    assert (co[n_ch:] == -7).all() and (co[:n_ch:cpf] == 2).all()
    o = out.cpu().numpy()
    assert (o[T * fs:] == SENT).all(), "dc_png_pack wrote past its output"
    o = o[:T * fs].reshape(T, fs)
    for t in range(T):
        assert (o[t, lens[t]:] == SENT).all(), f"frame {t}: bytes written past frame_len"
        assert o[t, :min(lens[t], fs)].tobytes() == streams[t][:fs], f"frame {t}: the packed stream differs"
    return streams, lens


@pytest.mark.parametrize("name", sorted(P.aimed_planes()))
def test_deflate_and_pack_on_the_aimed_planes(name):
    planes, chunk = P.aimed_planes()[name]
    streams, _ = _deflate_and_pack(planes, chunk)
    for t in range(planes.shape[0]):
        assert P.inflate_strict(streams[t], planes.shape[1]) == planes[t].tobytes()
    stored = [s for _, s, _ in P.plane_chunks(planes[0].tobytes(), chunk)]
    if name == "noise":
        assert all(stored)
    if name in ("runs", "one-byte-1000", "no-match", "fibonacci", "powers-of-two", "cl-overflow"):
        assert not any(stored)


@pytest.mark.parametrize("chunk", CHUNKS, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("kind", KINDS)
def test_deflate_and_pack_on_the_image_planes(kind, shape, chunk):
    planes = _planes(kind, shape)
    chunk = planes.shape[1] if chunk == "frame" else chunk
    if chunk in (1, 7) and planes.shape[1] > 10000:
        planes = planes[:1]
    _, lens = _deflate_and_pack(planes, chunk)
    assert max(lens) <= P.frame_max_bytes(planes.shape[1], chunk or P.CHUNK_DEFAULT)


def test_deflate_and_pack_at_the_largest_chunk():
    """160x160x3: 76960 bytes at 65535 are two chunks; the first fills the largest LDS layout the kernel takes."""
    for kind in ("photo", "noise"):
        _deflate_and_pack(_planes(kind, (160, 160, 3))[:1], 65535)


def test_pack_drops_what_does_not_fit_and_reports_the_full_length():
    planes = _planes("photo", (33, 17, 3))
    full = [len(P.zlib_stream(planes[t].tobytes(), 64)) for t in range(3)]
    _, lens = _deflate_and_pack(planes, 64, frame_stride=min(full) - 101)       # asserts frame_len and what lies behind the rows
    assert lens == full


def test_wrappers_refuse_short_buffers_and_bad_strides():
    from dynamicrafter_amd import ops
    planes = torch.zeros(3 * 100, dtype=torch.uint8, device=DEV)
    stride = ops.png_chunk_max_bytes(7)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)
    scratch = torch.zeros(3 * 15 * stride, dtype=torch.uint8, device=DEV)
    kw = dict(T=3, N=100, chunk=7)
    with pytest.raises(ValueError):
        ops.png_deflate(planes, scratch, i32(45), i32(45), stride=stride - 4, **kw)
    with pytest.raises(ValueError):
        ops.png_deflate(planes, scratch[:-1], i32(45), i32(45), stride=stride, **kw)
    with pytest.raises(ValueError):
        ops.png_deflate(planes, scratch, i32(44), i32(45), stride=stride, **kw)
    with pytest.raises(ValueError):
        ops.png_deflate(planes, scratch, i32(45), i32(44), stride=stride, **kw)
    with pytest.raises(ValueError):
        ops.png_deflate(planes, scratch[1:], i32(15), i32(15), T=1, N=100, chunk=7, stride=stride)     # not 4-byte aligned
    with pytest.raises(ValueError):
        ops.png_deflate(planes, scratch, i32(45), i32(45), T=3, N=100, chunk=65536, stride=65544)
    with pytest.raises(ValueError):
        ops.png_filter(torch.zeros(1, 4, 4, 2, dtype=torch.uint8, device=DEV), torch.zeros(100, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.png_filter(torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=DEV), torch.zeros(51, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.png_pack(scratch, i32(45), i32(45), i32(45), torch.zeros(10, dtype=torch.uint8, device=DEV), i32(3), stride=stride,
                     frame_stride=100, **kw)


# ------------------------------------------------------------------------------------------------ 3. end to end
def _samples(n=2, t=3, h=24, w=40):
    g = torch.Generator().manual_seed(1)
    return (torch.randn(n, 3, t, h, w, generator=g) * 0.5).to(DEV)


def _check_file(path, grid, fps=8, chunk=None, loops=0, still=False):
    """The file is, byte for byte, what the restatement writes for the uint8 frames `grid`; Pillow and the strict decoder read it
    back as the frames."""
    data = open(path, "rb").read()
    T, H, W, C = grid.shape
    assert data == P.png_bytes(grid, chunk, fps, loops, still)
    d = P.decode(data)
    assert (d["frames"] == grid).all() and (d["width"], d["height"], d["channels"]) == (W, H, C)
    im = Image.open(io.BytesIO(data))
    assert im.size == (W, H) and getattr(im, "n_frames", 1) == T
    for t in range(T):
        im.seek(t)
        assert (np.asarray(im.convert({1: "L", 3: "RGB", 4: "RGBA"}[C])).reshape(H, W, C) == grid[t]).all(), f"frame {t}"
    return data


def _same_pixels(path_a, path_b):
    a, b = P.decode(open(path_a, "rb").read()), P.decode(open(path_b, "rb").read())
    return (a["frames"] == b["frames"]).all() and a["fps"] == b["fps"] and a["loops"] == b["loops"]


def test_write_png_and_apng_end_to_end(tmp_path):
    from dynamicrafter_amd.utils import save_video as S
    grid = S.frames_to_uint8(_samples(n=2, t=3, h=96, w=80))
    g = grid.cpu().numpy()
    a = S.write_apng(str(tmp_path / "sub" / "a.png"), grid, fps=8, deflate="hip")
    data = _check_file(a, g)
    assert open(S.write_apng(str(tmp_path / "a2.png"), grid, fps=8, deflate="hip"), "rb").read() == data    # two runs, the same bytes
    z = S.write_apng(str(tmp_path / "z.png"), grid, fps=8, deflate="zlib")
    assert _same_pixels(a, z) and open(z, "rb").read() != data
    p = S.write_png(str(tmp_path / "p.png"), grid[1], deflate="hip")
    _check_file(p, g[1:2], still=True)
    assert _same_pixels(p, S.write_png(str(tmp_path / "pz.png"), grid[1], deflate="zlib"))
    for c in (1, 4):                                             # grey and RGBA, an odd size, loops and fps in the container
        f = _frames("photo", (33, 17, 3))[:, :, :, :1].repeat(c, 3) if c == 1 else _frames("photo", (96, 160, 4))[:2]
        _check_file(S.write_apng(str(tmp_path / f"c{c}.png"), _dev(f), fps=10, loops=2, deflate="hip"), f, fps=10, loops=2)
    one = np.full((1, 1, 1, 3), 200, dtype=np.uint8)
    _check_file(S.write_apng(str(tmp_path / "one.png"), _dev(one), deflate="hip"), one)
    streams = S.encode_png_frames(_dev(_frames("ramp", (33, 17, 3))), chunk=50)
    assert streams == [P.zlib_stream(p.tobytes(), 50) for p in _planes("ramp", (33, 17, 3))]


def test_writers_refuse_what_they_cannot_code(tmp_path):
    from dynamicrafter_amd.utils import save_video as S
    z = lambda c: torch.zeros(1, 16, 16, c, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        S.encode_png_frames(z(2))
    with pytest.raises(ValueError):
        S.encode_png_frames(z(3), chunk=0)
    with pytest.raises(ValueError):
        S.encode_png_frames(z(3), chunk=65536)
    with pytest.raises(ValueError):
        S.encode_png_frames(z(3).float())
    with pytest.raises(RuntimeError):
        S.encode_png_frames(z(3).cpu())
    with pytest.raises(ValueError):
        S.write_apng(str(tmp_path / "x.png"), z(3)[0], deflate="hip")
    with pytest.raises(ValueError):
        S.write_apng(str(tmp_path / "x.png"), z(3), deflate="gpu")
    assert not list(tmp_path.iterdir())


def test_save_results_with_hip_deflate(tmp_path, monkeypatch):
    from dynamicrafter_amd.scripts.evaluation import funcs
    from dynamicrafter_amd.utils import save_video as S
    monkeypatch.delenv("DC_PNG_DEFLATE", raising=False)
    x = _samples()
    d = str(tmp_path / "samples")
    grid = S.frames_to_uint8(x).cpu().numpy()
    p = S.save_results("a prompt", x, "clip0001.mp4", d, fps=8, deflate="hip")
    assert p.endswith("clip0001.png")
    hip = _check_file(p, grid)
    z = S.save_results("a prompt", x, "zlib.mp4", d, fps=8)      # the default still writes what it wrote before
    ref = S.write_apng(str(tmp_path / "ref.png"), S.frames_to_uint8(x), fps=8, deflate="zlib")
    assert open(z, "rb").read() == open(ref, "rb").read() != hip and _same_pixels(p, z)
    p = S.save_results("a prompt", x, "loop.mp4", d, fps=8, loop=True, deflate="hip")
    _check_file(p, grid[:-1])                                    # loop mode drops the duplicated last frame
    monkeypatch.setenv("DC_PNG_DEFLATE", "hip")                  # how the generate command line reaches the path
    assert open(S.save_results("a prompt", x, "env.mp4", d, fps=8), "rb").read() == hip
    assert open(S.save_results("a prompt", x, "envz.mp4", d, fps=8, deflate="zlib"), "rb").read() == open(ref, "rb").read()
    monkeypatch.delenv("DC_PNG_DEFLATE")
    ps = funcs.save_videos(x[None], str(tmp_path / "v"), ["b0"], fps=8, container="apng", deflate="hip")
    assert open(ps[0], "rb").read() == hip
    ps = S.tensor_to_frames(x, str(tmp_path / "stills"), deflate="hip")
    assert len(ps) == 3
    for t, q in enumerate(ps):
        _check_file(q, grid[t:t + 1], still=True)
    pz = S.tensor_to_frames(x, str(tmp_path / "stillz"))
    assert all(_same_pixels(a, b) for a, b in zip(ps, pz))


def test_save_results_seperate_with_hip_deflate(tmp_path, monkeypatch):
    from dynamicrafter_amd.utils import save_video as S
    monkeypatch.delenv("DC_PNG_DEFLATE", raising=False)
    x = _samples()
    d = str(tmp_path / "samples")
    ps = S.save_results_seperate("a prompt", x, "clip0001.mp4", d, fps=10, deflate="hip")
    assert len(ps) == 2 and all("samples_separate" in p and p.endswith(f"_sample{i}.png") for i, p in enumerate(ps))
    zs = S.save_results_seperate("a prompt", x, "z.mp4", d, fps=10)
    for i, p in enumerate(ps):
        _check_file(p, S.frames_to_uint8(x[i:i + 1]).cpu().numpy(), fps=10)
        assert _same_pixels(p, zs[i])
        ref = S.write_apng(str(tmp_path / f"ref{i}.png"), S.frames_to_uint8(x[i:i + 1]), fps=10, deflate="zlib")
        assert open(zs[i], "rb").read() == open(ref, "rb").read()


# ------------------------------------------------------------------------------------------------ 4. capture
def test_launches_replay_from_a_captured_graph():
    """png_filter, png_deflate and png_pack neither allocate nor synchronise: captured once into a graph on one stream, the
    replay on new frames gives the bytes the eager launches give."""
    from dynamicrafter_amd import ops
    shape, chunk, T = (33, 17, 3), 500, 3
    H, W, C = shape
    N = H * (1 + W * C)
    cpf = (N + chunk - 1) // chunk
    stride = ops.png_chunk_max_bytes(chunk)
    fs = ops.png_frame_max_bytes(N, chunk)
    frames = _dev(_frames("photo", shape))
    planes = torch.empty(T * N, dtype=torch.uint8, device=DEV)
    scratch = torch.empty(T * cpf * stride, dtype=torch.uint8, device=DEV)
    chunk_len, chunk_adler, chunk_off = (torch.empty(T * cpf, dtype=torch.int32, device=DEV) for _ in range(3))
    frame_len = torch.empty(T, dtype=torch.int32, device=DEV)
    out = torch.zeros(T * fs, dtype=torch.uint8, device=DEV)

    def enqueue():
        ops.png_filter(frames, planes)
        ops.png_deflate(planes, scratch, chunk_len, chunk_adler, T=T, N=N, chunk=chunk, stride=stride)
        ops.png_pack(scratch, chunk_len, chunk_adler, chunk_off, out, frame_len, T=T, N=N, chunk=chunk, stride=stride, frame_stride=fs)

    def result():
        ln = frame_len.cpu().tolist()
        o = out.cpu().numpy().reshape(T, fs)
        return [o[t, :ln[t]].tobytes() for t in range(T)]

    enqueue()
    torch.cuda.synchronize()
    eager_photo = result()
    graph = ops.DeviceGraph().capture(enqueue)
    frames.copy_(_dev(_frames("ramp", shape)))                   # new input in the captured buffers
    out.zero_()
    torch.cuda.synchronize()
    graph.launch()
    graph.sync()
    replay_ramp = result()
    enqueue()
    torch.cuda.synchronize()
    assert replay_ramp == result() and replay_ramp != eager_photo
    assert replay_ramp == [P.zlib_stream(p.tobytes(), chunk) for p in _planes("ramp", shape)]
    assert [zlib.decompress(s) for s in replay_ramp] == [p.tobytes() for p in _planes("ramp", shape)]

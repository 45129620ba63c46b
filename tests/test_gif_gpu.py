"""Animated GIF output on the GPU: the four dc_gif_* launches against the plain-Python restatement (tests/gif_restatement.py; its
own standing against Pillow's decoder and the strict decoder is tests/test_gif_cpu.py), the encoder end to end through Pillow and
the strict decoder, the save_results harness with container="gif", and the launches inside a captured graph. Everything here is
integer arithmetic, so every comparison is for equality.

RGB inputs are the Motion-JPEG tests' (noise / smooth, T = 2; 40x72, 33x17, 1x1); index planes are the CPU test's (noise, flat,
runs, smooth, T = 3; 80x96, 33x17, 1x1; chunks of 1 and 7 pixels, the whole frame, the default). Every output buffer has
sentinel elements behind it and behind each row's reported length."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

from tests import gif_restatement as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RGB_SIZES = [(40, 72), (33, 17), (1, 1)]
IDX_SIZES = [(80, 96), (33, 17), (1, 1)]
CHUNKS = [1, 7, "frame", None]
SENT = 0xA5
_ids = lambda s: f"{s[0]}x{s[1]}" if isinstance(s, tuple) else str(s)


@functools.lru_cache(maxsize=None)
def _frames(kind, hw):
    f = G.make_frames(kind, 2, hw[0], hw[1], np.random.default_rng(1))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _indices(kind, hw):
    v = G.make_indices(kind, 3, hw[0], hw[1], np.random.default_rng(1))
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _ref_chunks(kind, hw, chunk):
    """per frame: [(bytes, bits)] per chunk, and the packed image data"""
    idx = _indices(kind, hw)
    return [(G.frame_chunks(idx[t], chunk), G.image_data(idx[t], chunk)) for t in range(idx.shape[0])]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. histogram
def _gpu_hist(frames_dev):
    from dynamicrafter_amd import ops
    hist = torch.full((ops.GIF_HIST_BINS + 4,), -7, dtype=torch.int32, device=DEV)          # the entry clears what it counts in
    ops.gif_histogram(frames_dev, hist)
    torch.cuda.synchronize()
    h = hist.cpu().numpy()
    assert (h[ops.GIF_HIST_BINS:] == -7).all(), "dc_gif_histogram wrote past its table"
    return h[:ops.GIF_HIST_BINS].view(np.uint32)


@pytest.mark.parametrize("hw", RGB_SIZES, ids=_ids)
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_histogram_equals_the_restatement(kind, hw):
    f = _frames(kind, hw)
    got = _gpu_hist(_dev(f))
    assert int(got.sum()) == 2 * hw[0] * hw[1]
    assert (got == G.histogram(f)).all()


def test_histogram_of_flat_frames_and_of_a_two_sample_grid():
    """Flat frames send every pixel to one counter (the runs a thread merges); the grid of two samples side by side is what
    save_results hands to the encoder."""
    from dynamicrafter_amd.utils import save_video as S
    flat = np.zeros((2, 33, 17, 3), dtype=np.uint8)
    flat[1] = (255, 128, 7)
    assert (_gpu_hist(_dev(flat)) == G.histogram(flat)).all()
    grid = S.frames_to_uint8(_samples())
    assert tuple(grid.shape) == (3, 24, 80, 3)
    assert (_gpu_hist(grid) == G.histogram(grid.cpu().numpy())).all()


# ------------------------------------------------------------------------------------------------ 2. palette mapping
def _gpu_map(frames, palette, n, dither):
    from dynamicrafter_amd import ops
    T, H, W, _ = frames.shape
    idx = torch.full((T * H * W + 64,), SENT, dtype=torch.uint8, device=DEV)
    ops.gif_map(_dev(frames), _dev(palette), idx, n=n, dither=dither)
    torch.cuda.synchronize()
    got = idx.cpu().numpy()
    assert (got[T * H * W:] == SENT).all(), "dc_gif_map wrote past its output"
    return got[:T * H * W].reshape(T, H, W)


@pytest.mark.parametrize("n", [256, 2, 1])
@pytest.mark.parametrize("hw", RGB_SIZES, ids=_ids)
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_map_is_bit_exact(kind, hw, n):
    """256 entries: the palette the package builds for these frames (padded with a ramp if the clip has fewer colours). 2 and 1:
    the first entries of a 256-entry table, so an entry beyond n that is nearer must not be taken."""
    from dynamicrafter_amd.utils import save_video as S
    f = _frames(kind, hw)
    pal = G.ramp_palette()
    if n == 256:
        own = S.gif_palette(G.histogram(f))
        pal = np.concatenate([own, pal[:256 - own.shape[0]]])
    for dither in (0, 16, 64):
        ref = G.map_indices(f, pal[:n], dither)
        got = _gpu_map(f, pal, n, dither)
        assert int(got.max()) < n
        assert (got == ref).all(), f"dither {dither}: {int((got != ref).sum())} of {ref.size} indices differ"
    if n == 256 and hw == (40, 72):
        assert (G.map_indices(f, pal, 16) != G.map_indices(f, pal, 0)).any()    # the dither really moves pixels
        assert len(np.unique(G.map_indices(f, pal, 0))) > 100


def test_map_ties_go_to_the_lowest_index_and_the_offset_ignores_the_frame():
    f = np.empty((2, 9, 11, 3), dtype=np.uint8)
    f[...] = (102, 100, 100)
    pal = np.array([[250, 0, 0], [104, 100, 100], [100, 100, 100], [102, 98, 100], [102, 100, 102]], dtype=np.uint8)
    got = _gpu_map(f, pal, 5, 0)
    assert (got == 1).all() and (G.map_indices(f, pal, 0) == 1).all()           # four entries at distance 4: the first of them
    got = _gpu_map(f, pal[::-1].copy(), 5, 0)
    assert (got == 0).all()
    ramp = np.stack([np.arange(256)] * 3, 1).astype(np.uint8)
    g = _gpu_map(f, ramp, 256, 64)
    assert (g[0] == g[1]).all() and len(np.unique(g)) > 8 and (g == G.map_indices(f, ramp, 64)).all()


# ------------------------------------------------------------------------------------------------ 3. LZW + pack
def _lzw_and_pack(idx, chunk, frame_stride=None):
    """Runs dc_gif_lzw and dc_gif_pack on idx uint8 [T, H, W] with sentinels behind every buffer; returns (per frame the chunk
    strings as (bytes, bits), per frame the packed image data, frame_len)."""
    from dynamicrafter_amd import ops
    T, H, W = idx.shape
    hw = H * W
    chunk = ops.GIF_CHUNK if chunk is None else chunk
    cpf = (hw + chunk - 1) // chunk
    n_ch = T * cpf
    stride = ops.gif_chunk_max_bytes(min(chunk, hw))
    scratch = torch.full((n_ch * stride + 64,), SENT, dtype=torch.uint8, device=DEV)
    chunk_bits = torch.full((n_ch + 4,), -7, dtype=torch.int32, device=DEV)
    chunk_off = torch.full((n_ch + 4,), -7, dtype=torch.int32, device=DEV)
    frame_len = torch.full((T + 4,), -7, dtype=torch.int32, device=DEV)
    assert ops.gif_lzw(_dev(idx).reshape(-1), scratch, chunk_bits, T=T, hw=hw, chunk=chunk, stride=stride) == n_ch
    torch.cuda.synchronize()
    cb = chunk_bits.cpu().numpy()
    assert (cb[n_ch:] == -7).all() and (cb[:n_ch] >= 18).all() and (cb[:n_ch] <= 8 * stride).all()
    sc = scratch.cpu().numpy()
    assert (sc[n_ch * stride:] == SENT).all(), "dc_gif_lzw wrote past the scratch buffer"
    rows = sc[:n_ch * stride].reshape(n_ch, stride)
    nb = (cb[:n_ch] + 7) // 8
    for i in range(n_ch):
        assert (rows[i, nb[i]:] == SENT).all(), f"chunk {i}: bytes written past its length"
    chunks = [[(rows[t * cpf + s, :nb[t * cpf + s]].tobytes(), int(cb[t * cpf + s])) for s in range(cpf)] for t in range(T)]
    lens = [len(G.sub_blocks(G.merge(fr))) for fr in chunks]
    fs = frame_stride or ops.gif_frame_max_bytes(hw, chunk)
    out = torch.full((T * fs + 64,), SENT, dtype=torch.uint8, device=DEV)
    ops.gif_pack(scratch, chunk_bits, chunk_off, out, frame_len, T=T, chunks_per_frame=cpf, stride=stride, frame_stride=fs)
    torch.cuda.synchronize()
    fl = frame_len.cpu().numpy()
    assert (fl[T:] == -7).all() and fl[:T].tolist() == lens
    co = chunk_off.cpu().numpy()
    assert (co[n_ch:] == -7).all() and (co[:n_ch:cpf] == 9).all()
    o = out.cpu().numpy()
    assert (o[T * fs:] == SENT).all(), "dc_gif_pack wrote past its output"
    o = o[:T * fs].reshape(T, fs)
    for t in range(T):
        assert (o[t, lens[t]:] == SENT).all(), f"frame {t}: bytes written past frame_len"
    return chunks, [o[t, :min(lens[t], fs)].tobytes() for t in range(T)], lens


@pytest.mark.parametrize("chunk", CHUNKS, ids=_ids)
@pytest.mark.parametrize("hw", IDX_SIZES, ids=_ids)
@pytest.mark.parametrize("kind", ["noise", "flat", "runs", "smooth"])
def test_lzw_and_pack_are_bit_exact(kind, hw, chunk):
    """Chunk strings, their lengths in bits and the packed sub-blocked frames against the restatement. Noise at 80x96 in one
    chunk fills the table inside the chunk; chunks of 1 and 7 pixels end off byte boundaries (18 bits and up), so the pack
    really shifts; flat and runs give long matches (few codes per stage round)."""
    chunk = hw[0] * hw[1] if chunk == "frame" else chunk
    idx = _indices(kind, hw)
    ref = _ref_chunks(kind, hw, chunk)
    chunks, packed, lens = _lzw_and_pack(idx, chunk)
    for t in range(idx.shape[0]):
        rc, rp = ref[t]
        assert len(chunks[t]) == len(rc)
        assert [b for _, b in chunks[t]] == [b for _, b in rc], f"frame {t}: chunk bit lengths differ"
        for s, (a, b) in enumerate(zip(chunks[t], rc)):
            assert a[0] == b[0], f"frame {t} chunk {s}: the code string differs"
        assert packed[t] == rp, f"frame {t}: packed image data differs"
        assert lens[t] <= G.frame_max_bytes(hw[0] * hw[1], chunk or G.CHUNK_DEFAULT)
    if kind == "noise" and hw == (80, 96) and chunk == 80 * 96:
        assert chunks[0][0][1] > 12 * (G.CLEAR_INTERVAL + 1)    # more codes than one table holds: it was reset inside


def _no_match_pixels(n, rng):
    """n pixels in which no pair of neighbours occurs twice: the coder never finds a match, every pixel is one code."""
    px, seen = [0], set()
    while len(px) < n:
        k = int(rng.integers(256))
        if (px[-1], k) not in seen:
            seen.add((px[-1], k))
            px.append(k)
    return np.array(px, dtype=np.uint8)


def test_lzw_terminator_width_at_the_table_edges():
    """Chunks of n codes for n around 255, 767 and 1791: the terminator behind the n-th code is read at the smallest width w with
    258 + n - 1 < 2^w, one bit more than the n-th code itself at n = 255, 767, 1791. Two chunks per frame, so both a Clear and
    an EOI stand there."""
    width = lambda j: 9 if j == 0 else min(12, max(9, (258 + j - 1).bit_length()))
    for n in (254, 255, 256, 766, 767, 768, 1791):
        px = _no_match_pixels(n, np.random.default_rng(n))
        idx = np.concatenate([px, px[::-1]]).reshape(1, 2, n)
        ref = G.frame_chunks(idx[0], n)
        assert ref[0][1] == ref[1][1] == sum(width(j) for j in range(n + 1))
        chunks, packed, _ = _lzw_and_pack(idx, n)
        assert chunks[0] == ref and packed[0] == G.image_data(idx[0], n)


def test_pack_drops_what_does_not_fit_and_reports_the_full_length():
    idx = _indices("noise", (33, 17))
    full = [G.image_data(idx[t], 7) for t in range(3)]
    fs = min(len(x) for x in full) - 101
    _, packed, lens = _lzw_and_pack(idx, 7, frame_stride=fs)                    # asserts frame_len == the full lengths
    assert lens == [len(x) for x in full] and packed == [x[:fs] for x in full]


def test_wrappers_refuse_short_buffers_and_bad_strides():
    from dynamicrafter_amd import ops
    idx = torch.zeros(3 * 100, dtype=torch.uint8, device=DEV)
    stride = ops.gif_chunk_max_bytes(7)
    cb = torch.zeros(3 * 15, dtype=torch.int32, device=DEV)
    scratch = torch.zeros(3 * 15 * stride, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ops.gif_lzw(idx, scratch, cb, T=3, hw=100, chunk=7, stride=stride - 4)
    with pytest.raises(ValueError):
        ops.gif_lzw(idx, scratch[:-1], cb, T=3, hw=100, chunk=7, stride=stride)
    with pytest.raises(ValueError):
        ops.gif_lzw(idx, scratch, cb[:-1], T=3, hw=100, chunk=7, stride=stride)
    with pytest.raises(ValueError):
        ops.gif_lzw(idx, scratch[1:], cb, T=1, hw=100, chunk=7, stride=stride)            # not 4-byte aligned
    with pytest.raises(ValueError):
        ops.gif_map(torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=DEV), torch.zeros(6, dtype=torch.uint8, device=DEV),
                    torch.zeros(16, dtype=torch.uint8, device=DEV), n=3)
    with pytest.raises(ValueError):
        ops.gif_histogram(torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=DEV), torch.zeros(100, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.gif_pack(scratch, cb, cb.clone(), torch.zeros(10, dtype=torch.uint8, device=DEV),
                     torch.zeros(3, dtype=torch.int32, device=DEV), T=3, chunks_per_frame=15, stride=stride, frame_stride=100)


# ------------------------------------------------------------------------------------------------ 4. end to end
def _samples(n=2, t=3, h=24, w=40):
    g = torch.Generator().manual_seed(1)
    return (torch.randn(n, 3, t, h, w, generator=g) * 0.5).to(DEV)


def _check_file(path, grid, fps, dither=0, chunk=None, loops=0):
    """The file at `path` is, byte for byte, what the restatement writes for the uint8 frames `grid` with the package's palette;
    Pillow and the strict decoder read it back as palette[indices]."""
    from dynamicrafter_amd.utils import save_video as S
    data = open(path, "rb").read()
    T, H, W, _ = grid.shape
    pal = S.gif_palette(G.histogram(grid))
    idx = G.map_indices(grid, pal, dither)
    im = Image.open(io.BytesIO(data))
    assert im.n_frames == T and im.size == (W, H)
    assert im.info["duration"] == 10 * G.delay_cs(fps) and im.info["loop"] == loops
    for t in range(T):
        im.seek(t)
        assert (np.asarray(im.convert("RGB")) == pal[idx[t]]).all(), f"frame {t}"
    d = G.decode(data)
    assert (d["frames"] == idx).all() and d["delays"] == [G.delay_cs(fps)] * T and d["loops"] == loops
    assert (d["palette"][:len(pal)] == pal).all() and (d["palette"][len(pal):] == 0).all()
    assert data == G.gif_bytes(W, H, pal, [G.image_data(idx[t], chunk) for t in range(T)], fps, loops)
    return data


@pytest.mark.parametrize("dither", [0, 16])
def test_write_gif_end_to_end(tmp_path, dither):
    """96x160 pixels are two chunks at the default size; 33x17 goes in chunks of 50 pixels; 1x1 has a palette of one entry."""
    from dynamicrafter_amd.utils import save_video as S
    grid = S.frames_to_uint8(_samples(n=2, t=3, h=96, w=80))
    p = S.write_gif(str(tmp_path / "sub" / "a.gif"), grid, fps=8, dither=dither)
    a = _check_file(p, grid.cpu().numpy(), 8, dither)
    p2 = S.write_gif(str(tmp_path / "b.gif"), grid, fps=8, dither=dither)
    assert open(p2, "rb").read() == a                            # two runs, the same bytes
    f = _frames("smooth", (33, 17))
    p = S.write_gif(str(tmp_path / "c.gif"), _dev(f), fps=10, loops=2, dither=dither, chunk=50)
    _check_file(p, f, 10, dither, chunk=50, loops=2)
    pal, images = S.encode_gif_frames(_dev(f), dither=dither, chunk=50)
    assert pal.shape[0] <= 256 and len(images) == 2
    one = np.zeros((1, 1, 1, 3), dtype=np.uint8)
    _check_file(S.write_gif(str(tmp_path / "d.gif"), _dev(one), fps=100), one, 100)


def test_more_than_65535_frames_in_one_call():
    """A pack launch takes at most 65535 frames (gridDim.y): 65537 frames of 1x1 pixels, two flat colours alternating with the
    parity of the frame, come back as 65537 images, the same on both sides of the batch boundary. Two occupied histogram cells
    get their centres 8 (v >> 3) + 4 as palette entries: a decoded channel is at most 4 from the frame's."""
    from dynamicrafter_amd.utils import save_video as S
    colours = np.array([[200, 30, 90], [20, 180, 240]], dtype=np.uint8)
    f = colours[np.arange(65537) % 2].reshape(65537, 1, 1, 3)
    pal, images = S.encode_gif_frames(_dev(f))
    assert len(images) == 65537
    assert images[65534:] == [images[0], images[1], images[0]] and images[0] != images[1]
    d = G.decode(S.gif_file(1, 1, pal, images[:2]))
    got = d["palette"][d["frames"]].astype(np.int32)                       # [2, 1, 1, 3]
    assert got.shape == (2, 1, 1, 3) and np.abs(got - f[:2].astype(np.int32)).max() <= 4


def test_encoder_refuses_what_it_cannot_code():
    from dynamicrafter_amd.utils import save_video as S
    z = lambda c: torch.zeros(1, 16, 16, c, dtype=torch.uint8, device=DEV)
    for c in (4, 1):
        with pytest.raises(ValueError):
            S.encode_gif_frames(z(c))
    with pytest.raises(ValueError):
        S.encode_gif_frames(z(3), dither=65)
    with pytest.raises(ValueError):
        S.encode_gif_frames(z(3), chunk=0)
    with pytest.raises(ValueError):
        S.encode_gif_frames(z(3).float())
    with pytest.raises(RuntimeError):
        S.encode_gif_frames(z(3).cpu())


def test_save_results_gif(tmp_path):
    from dynamicrafter_amd.utils import save_video as S
    x = _samples()
    d = str(tmp_path / "samples")
    grid = S.frames_to_uint8(x).cpu().numpy()
    p = S.save_results("a prompt", x, "clip0001.mp4", d, fps=8, container="gif")
    assert p.endswith("clip0001.gif")
    _check_file(p, grid, 8)
    p = S.save_results("a prompt", x, "dith.mp4", d, fps=8, container="gif", dither=16)
    _check_file(p, grid, 8, dither=16)
    p = S.save_results("a prompt", x, "loop.mp4", d, fps=8, loop=True, container="gif")
    _check_file(p, grid[:-1], 8)                                 # loop mode drops the duplicated last frame
    # the default still writes the APNG it wrote before
    p = S.save_results("a prompt", x, "clip0001.mp4", d, fps=8)
    assert p.endswith("clip0001.png")
    ref = S.write_apng(str(tmp_path / "ref.png"), S.frames_to_uint8(x), fps=8)
    assert open(p, "rb").read() == open(ref, "rb").read()
    with pytest.raises(ValueError):
        S.save_results("a prompt", x, "clip0001.mp4", d, container="mp4")


def test_save_results_seperate_gif(tmp_path):
    from dynamicrafter_amd.utils import save_video as S
    x = _samples()
    d = str(tmp_path / "samples")
    ps = S.save_results_seperate("a prompt", x, "clip0001.mp4", d, fps=10, container="gif")
    assert len(ps) == 2 and all("samples_separate" in p and p.endswith(f"_sample{i}.gif") for i, p in enumerate(ps))
    for i, p in enumerate(ps):
        _check_file(p, S.frames_to_uint8(x[i:i + 1]).cpu().numpy(), 10)
    ps = S.save_results_seperate("a prompt", x, "clip0001.mp4", d, fps=10, loop=True, container="gif", dither=64)
    for i, p in enumerate(ps):
        _check_file(p, S.frames_to_uint8(x[i:i + 1, :, :-1]).cpu().numpy(), 10, dither=64)
    ps = S.save_results_seperate("a prompt", x, "clip0001.mp4", d, fps=10)
    for i, p in enumerate(ps):
        ref = S.write_apng(str(tmp_path / f"ref{i}.png"), S.frames_to_uint8(x[i:i + 1]), fps=10)
        assert p.endswith(".png") and open(p, "rb").read() == open(ref, "rb").read()
    with pytest.raises(ValueError):
        S.save_results_seperate("a prompt", x, "clip0001.mp4", d, container="mp4")


# ------------------------------------------------------------------------------------------------ 5. capture
def test_launches_replay_from_a_captured_graph():
    """gif_map, gif_lzw and gif_pack on a given palette neither allocate nor synchronise: captured once into a graph on one
    stream, the replay on new frames gives the bytes the eager launches give."""
    from dynamicrafter_amd import ops
    hw, chunk = (40, 72), 500
    T, n = 2, hw[0] * hw[1]
    cpf = (n + chunk - 1) // chunk
    stride = ops.gif_chunk_max_bytes(chunk)
    fs = ops.gif_frame_max_bytes(n, chunk)
    frames = _dev(_frames("smooth", hw))
    pal = G.ramp_palette()
    pal_dev = _dev(pal)
    idx = torch.empty(T * n, dtype=torch.uint8, device=DEV)
    scratch = torch.empty(T * cpf * stride, dtype=torch.uint8, device=DEV)
    chunk_bits, chunk_off = (torch.empty(T * cpf, dtype=torch.int32, device=DEV) for _ in range(2))
    frame_len = torch.empty(T, dtype=torch.int32, device=DEV)
    out = torch.zeros(T * fs, dtype=torch.uint8, device=DEV)

    def enqueue():
        ops.gif_map(frames, pal_dev, idx, n=256, dither=16)
        ops.gif_lzw(idx, scratch, chunk_bits, T=T, hw=n, chunk=chunk, stride=stride)
        ops.gif_pack(scratch, chunk_bits, chunk_off, out, frame_len, T=T, chunks_per_frame=cpf, stride=stride, frame_stride=fs)

    def result():
        ln = frame_len.cpu().tolist()
        o = out.cpu().numpy().reshape(T, fs)
        return [o[t, :ln[t]].tobytes() for t in range(T)]

    enqueue()
    torch.cuda.synchronize()
    eager_smooth = result()
    graph = ops.DeviceGraph().capture(enqueue)
    frames.copy_(_dev(_frames("noise", hw)))                     # new input in the captured buffers
    out.zero_()
    torch.cuda.synchronize()
    graph.launch()
    graph.sync()
    replay_noise = result()
    enqueue()
    torch.cuda.synchronize()
    assert replay_noise == result() and replay_noise != eager_smooth
    ref = G.map_indices(_frames("noise", hw), pal, 16)
    assert replay_noise == [G.image_data(ref[t], chunk) for t in range(T)]

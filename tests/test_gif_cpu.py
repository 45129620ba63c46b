"""Animated GIF output, the parts that need no GPU: the restatement (tests/gif_restatement.py - the reference of the GPU tests)
against Pillow's decoder and its own strict decoder, the host palette builder, the palette's quality against Pillow's median
cut, the container writer, and the argument checks of the four dc_gif_* entries.

Index planes (np.random.default_rng(1) per case, T = 3): "noise" = uniform 0..255, "flat", "runs" = arange // 37 % 256,
"smooth". Sizes: 80x96 (7680 pixels: noise coded as one chunk per frame fills the 4096-entry table inside the chunk), 33x17,
1x1. Chunks: 1 and 7 pixels, the whole frame, and the default."""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest
from PIL import Image

from tests import gif_restatement as G

SIZES = [(80, 96), (33, 17), (1, 1)]
KINDS = ["noise", "flat", "runs", "smooth"]
CHUNKS = [1, 7, "frame", None]
# dB by which the clip-global palette may fall short of Pillow's per-frame median cut. 0: no input of this file falls short (the
# smallest lead is 1.3 dB, on the larger smooth clip)
PALETTE_MARGIN_DB = 0.0
_ids = lambda s: f"{s[0]}x{s[1]}" if isinstance(s, tuple) else str(s)


@functools.lru_cache(maxsize=None)
def _indices(kind, hw):
    v = G.make_indices(kind, 3, hw[0], hw[1], np.random.default_rng(1))
    v.setflags(write=False)
    return v


def _open(data):
    im = Image.open(io.BytesIO(data))
    return im


# ------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("chunk", CHUNKS, ids=_ids)
@pytest.mark.parametrize("hw", SIZES, ids=_ids)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_decodes_exactly_in_pillow_and_in_the_strict_decoder(kind, hw, chunk):
    H, W = hw
    idx = _indices(kind, hw)
    chunk = H * W if chunk == "frame" else chunk
    pal = G.ramp_palette()
    data = G.encode(idx, pal, chunk, fps=8, loops=0)
    im = _open(data)
    assert im.n_frames == 3 and im.size == (W, H)
    assert im.info["duration"] == 130 and im.info["loop"] == 0
    for t in range(3):
        im.seek(t)
        assert (np.asarray(im.convert("RGB")) == pal[idx[t]]).all(), f"frame {t}"
    d = G.decode(data)
    assert (d["width"], d["height"], d["loops"], d["delays"]) == (W, H, 0, [13] * 3)
    assert (d["frames"] == idx).all() and (d["palette"] == pal).all()
    for t in range(3):                                           # the stated bounds hold for what the restatement writes
        n = min(chunk or G.CHUNK_DEFAULT, H * W)
        assert all(len(b) <= G.chunk_max_bytes(n) for b, _ in G.frame_chunks(idx[t], chunk))
        assert len(G.image_data(idx[t], chunk)) <= G.frame_max_bytes(H * W, chunk or G.CHUNK_DEFAULT)


def test_the_cases_reach_the_paths_they_are_there_for():
    """Noise at one chunk per frame resets the table inside the chunk (a 12-bit Clear that no chunk boundary explains); a chunk
    whose 255th code is its last ends on a terminator one bit wider than its last data code."""
    idx = _indices("noise", (80, 96))
    (data, bits), = G.frame_chunks(idx[0], 80 * 96)
    assert bits > 12 * (G.CLEAR_INTERVAL + 1)
    seen, pos, width, j = 0, 0, 9, 0
    acc = int.from_bytes(data, "little")
    while pos < bits:                                            # a walk by the encoder's rule: count the Clears
        code = (acc >> pos) & ((1 << width) - 1)
        pos += width
        j += 1
        if code == G.CLEAR:
            seen, j = seen + 1, 0
        width = 9
        while j >= 1 and 258 + j - 1 >= (1 << width) and width < 12:
            width += 1
    assert seen == 1
    px = np.arange(255) % 256                                    # 255 distinct pixels: 255 data codes, no match
    data, bits = G.lzw_chunk(px, True)
    assert bits == 255 * 9 + 10 and (int.from_bytes(data, "little") >> (255 * 9)) == G.EOI


def test_strict_decoder_refuses_the_classic_mistakes():
    """17 x 30 pixels in two chunks of 255 distinct pixels: each chunk is 255 data codes at 9 bits and a terminator that a decoder
    reads at 10. A Clear written at 9 bits there (the width of the encoder, which has not added "its" entry) is the classic bug;
    the second chunk begins with an odd pixel, so the misread code is 256 + 512 and no decoder state can take it."""
    pal = G.ramp_palette()
    px = np.concatenate([np.arange(1, 256), 255 - np.arange(255)]).astype(np.uint8)

    def stream(first_terminator_width, eoi=True):
        b = G._Bits()
        b.put(G.CLEAR, 9)
        for v in px[:255]:
            b.put(int(v), 9)
        b.put(G.CLEAR, first_terminator_width)
        for v in px[255:]:
            b.put(int(v), 9)
        if eoi:
            b.put(G.EOI, 10)
        return b.result()[0]

    file = lambda s, h=30: G.gif_bytes(17, h, pal, [G.sub_blocks(s)])
    right = stream(10)
    assert right == G.merge(G.frame_chunks(px, 255))
    good = file(right)
    assert (G.decode(good)["frames"].reshape(-1) == px).all()
    for bad in (file(stream(9)),                                 # the narrow terminator
                file(stream(10, eoi=False)),                     # no EOI
                file(right + b"\x00"),                           # a byte behind the one that holds EOI
                file(G.lzw_chunk(px, True)[0]),                  # no leading Clear
                file(right, h=31),                               # EOI before the frame is full
                file(right, h=29),                               # indices beyond the frame
                good[:-1],                                       # no trailer
                good + b"\x00",                                  # bytes behind the trailer
                good[:-40]):                                     # a sub-block that runs beyond the file
        with pytest.raises(G.GifError):
            G.decode(bad)
    bits = 9 + 2 * (255 * 9 + 10)
    assert bits % 8 == 3
    padded = bytearray(right)
    padded[-1] |= 0x80                                           # a set pad bit
    with pytest.raises(G.GifError):
        G.decode(file(bytes(padded)))


def test_bayer_matrix_and_dither_offsets():
    b = G.bayer(8)
    assert b[0].tolist() == [0, 32, 8, 40, 2, 34, 10, 42] and b[1].tolist() == [48, 16, 56, 24, 50, 18, 58, 26]
    assert sorted(b.reshape(-1).tolist()) == list(range(64))
    f = np.full((1, 8, 8, 3), 128, dtype=np.uint8)
    grey = np.stack([np.arange(256)] * 3, 1).astype(np.uint8)
    assert (G.map_indices(f, grey, 0) == 128).all()
    d64 = G.map_indices(f, grey, 64)[0].astype(int) - 128
    assert d64.min() == -32 and d64.max() == 31 and (d64 == (2 * b - 63) * 64 // 128).all()


# ------------------------------------------------------------------------------------------------ 2. the palette
def test_gif_palette_is_deterministic_distinct_and_at_most_256():
    from dynamicrafter_amd.utils import save_video as S
    for kind in ("noise", "smooth"):
        f = G.make_frames(kind, 2, 40, 72, np.random.default_rng(1))
        h = G.histogram(f)
        p = S.gif_palette(h)
        assert p.dtype == np.uint8 and p.ndim == 2 and p.shape[1] == 3 and 1 <= p.shape[0] <= 256
        assert len({tuple(e) for e in p.tolist()}) == p.shape[0]
        assert (S.gif_palette(h.copy()) == p).all()
        assert (S.gif_palette(h.view(np.int32)) == p).all()     # the device histogram arrives as int32 bit patterns
    with pytest.raises(ValueError):
        S.gif_palette(np.zeros(32768, dtype=np.uint32))
    with pytest.raises(ValueError):
        S.gif_palette(np.ones(100, dtype=np.uint32))


def test_gif_palette_of_few_colours_is_those_colours():
    from dynamicrafter_amd.utils import save_video as S
    cols = np.array([[0, 0, 0], [255, 255, 255], [200, 16, 99], [200, 17, 99 + 8], [7, 130, 250]], dtype=np.uint8)
    f = cols[np.random.default_rng(1).integers(0, 5, size=(2, 9, 11))]
    assert len(set(f.reshape(-1, 3).dot([65536, 256, 1]).tolist())) == 5
    p = S.gif_palette(G.histogram(f))
    centres = (cols >> 3) * 8 + 4
    assert sorted(map(tuple, p.tolist())) == sorted(map(tuple, centres.tolist()))
    black = S.gif_palette(G.histogram(np.zeros((2, 5, 7, 3), dtype=np.uint8)))
    assert black.tolist() == [[4, 4, 4]]
    # 256 occupied cells: exactly their centres; 257: one pair has to share an entry
    cells = np.random.default_rng(2).choice(32768, size=257, replace=False)
    h = np.zeros(32768, dtype=np.uint32)
    h[cells[:256]] = np.arange(1, 257)
    p = S.gif_palette(h)
    want = np.stack([cells[:256] >> 10, (cells[:256] >> 5) & 31, cells[:256] & 31], 1) * 8 + 4
    assert sorted(map(tuple, p.tolist())) == sorted(map(tuple, want.tolist()))
    h[cells[256]] = 5
    p = S.gif_palette(h)
    assert p.shape == (256, 3) and len({tuple(e) for e in p.tolist()}) == 256


def _pillow_psnr(frame):
    q = Image.fromarray(frame).quantize(256, method=Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE)
    return G.psnr(np.asarray(q.convert("RGB")), frame)


@pytest.mark.parametrize("case", [("smooth", 2, 40, 72), ("noise", 2, 40, 72), ("smooth", 4, 96, 160)], ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}")
def test_palette_quality_against_pillows_median_cut(case):
    """One palette for the whole clip against Pillow's own 256-colour median cut of every single frame, both without dither:
    per frame our PSNR must not fall below Pillow's."""
    from dynamicrafter_amd.utils import save_video as S
    kind, T, H, W = case
    f = G.make_frames(kind, T, H, W, np.random.default_rng(1))
    pal = S.gif_palette(G.histogram(f))
    rec = pal[G.map_indices(f, pal, 0)]
    for t in range(T):
        ours, ref = G.psnr(rec[t], f[t]), _pillow_psnr(f[t])
        print(f"{kind} {T}x{H}x{W} frame {t}: {pal.shape[0]} colours for the clip {ours:.3f} dB, Pillow per frame {ref:.3f} dB")
        assert ours >= ref - PALETTE_MARGIN_DB


# ------------------------------------------------------------------------------------------------ 3. container and host code
@pytest.mark.parametrize("fps,delay", [(8, 13), (10, 10), (100, 2)])
def test_container_fields(fps, delay):
    from dynamicrafter_amd.utils import save_video as S
    idx = _indices("smooth", (33, 17)) % 200
    pal = G.ramp_palette(200)                                    # fewer than 256 entries: the table is padded with zeros
    images = [G.image_data(idx[t], None) for t in range(3)]
    for loops in (0, 3):
        data = S.gif_file(17, 33, pal, images, fps=fps, loops=loops)
        assert data == G.gif_bytes(17, 33, pal, images, fps=fps, loops=loops)   # the restatement assembles the same bytes
        d = G.decode(data)
        assert (d["width"], d["height"], d["loops"], d["delays"]) == (17, 33, loops, [delay] * 3)
        assert (d["palette"][:200] == pal).all() and (d["palette"][200:] == 0).all()
        im = _open(data)
        assert im.n_frames == 3 and im.size == (17, 33) and im.info["duration"] == 10 * delay and im.info["loop"] == loops
        im.seek(2)
        assert (np.asarray(im.convert("RGB")) == pal[idx[2]]).all()
    assert S.gif_delay(fps) == delay == G.delay_cs(fps)


def test_container_refuses_what_a_gif_cannot_hold():
    from dynamicrafter_amd.utils import save_video as S
    pal, img = G.ramp_palette(), [G.image_data(np.zeros((1, 1), dtype=np.uint8))]
    S.gif_file(65535, 1, pal, img)
    for w, h in ((65536, 1), (1, 65536), (0, 1)):
        with pytest.raises(ValueError):
            S.gif_file(w, h, pal, img)
    with pytest.raises(ValueError):
        S.gif_file(1, 1, pal, [])
    with pytest.raises(ValueError):
        S.gif_file(1, 1, np.zeros((257, 3), dtype=np.uint8), img)
    with pytest.raises(ValueError):
        S.gif_file(1, 1, pal, img, loops=65536)
    with pytest.raises(ValueError):
        S.gif_file(1, 1, pal, img, fps=0)


def test_host_entry_points_without_a_gpu(tmp_path):
    import torch
    from dynamicrafter_amd.scripts.evaluation.inference import get_parser
    from dynamicrafter_amd.utils import save_video as S
    cpu = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        S.encode_gif_frames(cpu)
    with pytest.raises(RuntimeError):
        S.write_gif(str(tmp_path / "x.gif"), cpu)
    with pytest.raises(RuntimeError):
        S._write_clip(str(tmp_path / "x"), cpu, 8, "gif", 90)
    with pytest.raises(ValueError, match="'apng', 'avi' or 'gif'"):
        S._write_clip(str(tmp_path / "x"), cpu, 8, "mp4", 90)
    assert not os.listdir(tmp_path)
    p = get_parser()
    assert p.parse_args(["--container", "gif"]).container == "gif"
    assert p.parse_args([]).container == "apng"
    with pytest.raises(SystemExit):
        p.parse_args(["--container", "mp4"])


def test_bounds_are_the_same_in_the_header_the_wrappers_and_the_restatement():
    from dynamicrafter_amd import _hip, ops
    hdr = open(os.path.join(os.path.dirname(_hip._HERE), "include", "dcrafter_hip.h")).read()
    assert "#define DC_GIF_CLEAR_INTERVAL 3838" in hdr and "#define DC_GIF_HIST_BINS 32768" in hdr
    assert "#define DC_GIF_CHUNK_MAX_BITS(n) (12LL * ((n) + (n) / DC_GIF_CLEAR_INTERVAL + 1))" in hdr
    assert ops.GIF_CLEAR_INTERVAL == G.CLEAR_INTERVAL == 4095 - 258 + 1 and ops.GIF_CHUNK == G.CHUNK_DEFAULT
    for n in (1, 7, 3837, 3838, 8192, 7680, 589824):
        assert ops.gif_chunk_max_bytes(n) == G.chunk_max_bytes(n) and G.chunk_max_bytes(n) % 4 == 0
        for chunk in (1, 7, 4096, 8192):
            assert ops.gif_frame_max_bytes(n, chunk) == G.frame_max_bytes(n, chunk)
    assert 4096 <= ops.GIF_CHUNK <= 16384


def test_gif_entries_reject_bad_arguments_without_gpu():
    """Null pointers and a misaligned scratch -> DC_ERR_ARG (-2); sizes below 1, n outside 1..256, dither outside 0..64, a stride
    below the worst case or no multiple of 4, bit offsets beyond 32 bits -> DC_ERR_SHAPE (-1); all before any launch."""
    from dynamicrafter_amd import _hip
    lib = _hip.lib()
    p = C.c_void_p(8)
    assert lib.dc_gif_histogram(None, p, 1, 16, 16, None) == -2
    assert lib.dc_gif_histogram(p, None, 1, 16, 16, None) == -2
    assert lib.dc_gif_histogram(p, p, 0, 16, 16, None) == -1
    assert lib.dc_gif_histogram(p, p, 1, 0, 16, None) == -1
    assert lib.dc_gif_histogram(p, p, 1, 16, 0, None) == -1
    assert lib.dc_gif_histogram(p, p, 65536, 65536, 1, None) == -1            # 2^32 pixels: a counter could wrap
    assert lib.dc_gif_map(None, p, p, 1, 16, 16, 256, 0, None) == -2
    assert lib.dc_gif_map(p, None, p, 1, 16, 16, 256, 0, None) == -2
    assert lib.dc_gif_map(p, p, None, 1, 16, 16, 256, 0, None) == -2
    assert lib.dc_gif_map(p, p, p, 1, 16, 16, 0, 0, None) == -1
    assert lib.dc_gif_map(p, p, p, 1, 16, 16, 257, 0, None) == -1
    assert lib.dc_gif_map(p, p, p, 1, 16, 16, 256, 65, None) == -1
    assert lib.dc_gif_map(p, p, p, 1, 16, 16, 256, -1, None) == -1
    assert lib.dc_gif_map(p, p, p, 1, 0, 16, 256, 0, None) == -1
    assert lib.dc_gif_map(p, p, p, 0, 16, 16, 256, 0, None) == -1
    stride = G.chunk_max_bytes(100)
    assert lib.dc_gif_lzw(None, p, p, 1, 256, 100, stride, None) == -2
    assert lib.dc_gif_lzw(p, None, p, 1, 256, 100, stride, None) == -2
    assert lib.dc_gif_lzw(p, p, None, 1, 256, 100, stride, None) == -2
    assert lib.dc_gif_lzw(p, C.c_void_p(10), p, 1, 256, 100, stride, None) == -2
    assert lib.dc_gif_lzw(p, p, p, 0, 256, 100, stride, None) == -1
    assert lib.dc_gif_lzw(p, p, p, 1, 0, 100, stride, None) == -1
    assert lib.dc_gif_lzw(p, p, p, 1, 256, 0, stride, None) == -1
    assert lib.dc_gif_lzw(p, p, p, 1, 256, 100, stride - 4, None) == -1
    assert lib.dc_gif_lzw(p, p, p, 1, 256, 100, stride + 2, None) == -1
    assert lib.dc_gif_lzw(p, p, p, 1, 50, 100, G.chunk_max_bytes(50) - 4, None) == -1   # the frame is the longest chunk
    assert lib.dc_gif_pack(None, p, p, p, p, 1, 3, stride, 1000, None) == -2
    assert lib.dc_gif_pack(p, None, p, p, p, 1, 3, stride, 1000, None) == -2
    assert lib.dc_gif_pack(p, p, None, p, p, 1, 3, stride, 1000, None) == -2
    assert lib.dc_gif_pack(p, p, p, None, p, 1, 3, stride, 1000, None) == -2
    assert lib.dc_gif_pack(p, p, p, p, None, 1, 3, stride, 1000, None) == -2
    assert lib.dc_gif_pack(p, p, p, p, p, 0, 3, stride, 1000, None) == -1
    assert lib.dc_gif_pack(p, p, p, p, p, 65536, 3, stride, 1000, None) == -1
    assert lib.dc_gif_pack(p, p, p, p, p, 1, 0, stride, 1000, None) == -1
    assert lib.dc_gif_pack(p, p, p, p, p, 1, 3, 0, 1000, None) == -1
    assert lib.dc_gif_pack(p, p, p, p, p, 1, 3, stride, 0, None) == -1
    assert lib.dc_gif_pack(p, p, p, p, p, 1, 1 << 20, 1 << 10, 1000, None) == -1          # 2^33 bits in a frame

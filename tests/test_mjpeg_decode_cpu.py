"""Motion-JPEG input without a GPU: the numpy restatement of the decoder (tests/jpeg_decode_restatement.py) against libjpeg
through Pillow, the package's JPEG header parser and AVI reader (dynamicrafter_amd/utils/load_video.py), the frame selection of
funcs.load_video_batch, and the argument checks of the dc_jpeg_decode_* entries.

Inputs are jpeg_restatement.make_frames "noise" and "smooth" (np.random.default_rng(1)) at 16x16 (one 4:2:0 MCU), 24x40 and
37x53 (odd both ways: a chroma plane of 19 x 27 real samples inside 24 x 32 padded ones)."""
import ctypes as C
import io
import itertools
import struct

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_decode_restatement as D
from tests import jpeg_restatement as J

from tests.mjpeg_decode_cases import (KINDS, LIBJPEG_BOUND, QUALITIES, SIZES, frames, libjpeg_distance, pillow_file, pillow_rgb,
                                      pixel_batches)


# ------------------------------------------------------------------------------------------------ 1. restatement vs libjpeg
@pytest.mark.parametrize("mode", [0, 1, 2, "L"], ids=["444", "422", "420", "grey"])
def test_restatement_against_libjpeg(mode):
    cap_max, cap_share = LIBJPEG_BOUND[mode]
    worst = (0, 0.0)
    for opt, rst, kind, hw, q in itertools.product((True, False), (None, 1, 3), KINDS, SIZES, QUALITIES):
        data = pillow_file(frames(kind, hw)[0], mode, q, opt, rst)
        p = D.parse(data)
        assert (p["height"], p["width"]) == hw and (p["ri"] > 0) == bool(rst)
        mx, share = libjpeg_distance(D.pixels(data), pillow_rgb(data))
        worst = (max(worst[0], mx), max(worst[1], share))
        assert mx <= cap_max and share <= cap_share, (opt, rst, kind, hw, q, mx, share)
    print(f"mode {mode}: largest difference {worst[0]}, largest share above 1 level {worst[1]:.6f}")


def test_restatement_float32_against_float64():
    """What fp32 itself costs in the pixel stage (4:2:0 at 16x16, 37x53 and 64x96, two frames, three qualities): no sample
    differs by more than 1 and at most 3 in 36 864 (8e-5) differ at all; measured: 1 of 150 498."""
    differ = total = 0
    for hw in ((16, 16), (37, 53), (64, 96)):
        for q in QUALITIES:
            for data in J.encode(frames("noise", hw, 2), q):
                co = D.coefficients(data)
                d = np.abs(D.pixels(data, np.float64, co).astype(np.int32) - D.pixels(data, np.float32, co).astype(np.int32))
                assert d.max() <= 1
                differ += int((d != 0).sum())
                total += d.size
    print(f"float32 vs float64: {differ} of {total} samples differ")
    assert differ <= 3 * total // 36864


@pytest.mark.parametrize("mode", [0, 1, 2, "L"], ids=["444", "422", "420", "grey"])
def test_gpu_pixel_inputs_stay_within_their_cap_in_float32(mode):
    """tests/test_mjpeg_decode_gpu.py holds the kernels' fp32 pixels to the float64 restatement on pixel_batches(mode): no
    sample off by more than 1, at most 1 in 1000 of a mode's samples off at all. The fp32 restatement must meet that with
    room, or the cap would measure the inputs and not the kernels."""
    differ = total = 0
    for _, files in pixel_batches(mode):
        for data in files:
            co = D.coefficients(data)
            d = np.abs(D.pixels(data, np.float64, co).astype(np.int32) - D.pixels(data, np.float32, co).astype(np.int32))
            assert d.max() <= 1
            differ += int((d != 0).sum())
            total += d.size
    print(f"mode {mode}: float32 vs float64 restatement: {differ} of {total} samples differ")
    assert differ * 4 <= total // 1000


# ------------------------------------------------------------------------------------------------ 2. coefficients
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", KINDS)
def test_coefficients_come_back_exactly(kind, hw):
    f = frames(kind, hw, 2)
    my, mx = J.mcu_grid(*hw)
    for q in QUALITIES:
        ref = J.coefficients(f, J.quant_tables(q))
        for ri in (1, 3, my * mx):
            files = J.encode(f, q, ri=ri)
            for t in range(2):
                assert np.array_equal(D.coefficients(files[t]), ref[t]), (q, ri, t)


# ------------------------------------------------------------------------------------------------ 3. the package's parser
def same_parse(data):
    """The package's parse_jpeg and scan_segments against the restatement's parse."""
    from dynamicrafter_amd.utils import load_video as L
    info, p = L.parse_jpeg(data), D.parse(data)
    assert (info.width, info.height, info.ncomp, info.hs, info.vs, info.ri) == (p["width"], p["height"], len(p["comps"]), p["hs"],
                                                                                 p["vs"], p["ri"])
    assert {k: list(v) for k, v in info.qtabs.items()} == {k: v.tolist() for k, v in p["q"].items()}
    assert {k: (bytes(b), bytes(v)) for k, (b, v) in info.huff.items()} == {k: (bytes(b), bytes(v)) for k, (b, v) in p["huff"].items()}
    assert info.comps == [(tq, td, ta) for _, _, _, tq, td, ta in p["comps"]]
    segs = L.scan_segments(data, info)
    assert [data[a:a + n] for a, n in segs.tolist()] == p["segments"]
    return info


def test_parse_jpeg_agrees_with_the_restatement():
    for mode, opt, rst in itertools.product((0, 1, 2, "L"), (True, False), (None, 1, 3)):
        info = same_parse(pillow_file(frames("noise", (37, 53))[0], mode, 90, opt, rst))
        assert info.mcus == {0: 35, 1: 20, 2: 12, "L": 35}[mode]
    info = same_parse(J.encode(frames("smooth", (37, 53)), 90, ri=1)[0])
    assert info.ri == 1 and info.geometry() == (53, 37, 3, 2, 2)


def cmyk_file():
    b = io.BytesIO()
    Image.fromarray(np.asarray(frames("noise", (16, 16))[0])).convert("CMYK").save(b, "JPEG")
    return b.getvalue()


def test_parse_errors_name_the_cause():
    from dynamicrafter_amd.utils import load_video as L
    f = frames("smooth", (37, 53))[0]
    good = J.encode(frames("smooth", (37, 53)), 90, ri=1)[0]

    def refuses(data, match):
        with pytest.raises(ValueError, match=match):
            L.scan_segments(data, L.parse_jpeg(data))

    refuses(pillow_file(f, 2, progressive=True), "progressive")
    refuses(cmyk_file(), "4 components")
    sos = good.index(b"\xff\xda")
    refuses(good[:sos + 6], "truncated header")
    refuses(good[:good.index(b"\xff\xc0") + 7], "truncated header")
    refuses(good[:2], "truncated header")
    assert good.count(b"\xff\xd3") == 1 and good.count(b"\xff\xd4") == 1
    refuses(good.replace(b"\xff\xd3", b"\xff\xd5"), "count up modulo 8")                       # RST3 -> RST5
    cut = good.index(b"\xff\xd3")
    refuses(good[:cut] + good[good.index(b"\xff\xd4"):], "restart segments")                    # a segment dropped
    sof = good.index(b"\xff\xc0")
    refuses(good[:sof + 4] + b"\x0c" + good[sof + 5:], "12-bit")
    refuses(good[:sof + 1] + b"\xc1" + good[sof + 2:], "SOF1")
    dqt = good.index(b"\xff\xdb")
    refuses(good[:dqt + 4] + b"\x10" + good[dqt + 5:], "16-bit quantisation")
    refuses(good[:sof + 11] + b"\x12" + good[sof + 12:], "sampling")                            # luma 1x2
    refuses(good[:-2] + b"\xff\xda" + good[sos + 2:], "more than one scan")                    # a second SOS behind the scan
    refuses(b"\x89PNG", "no SOI")


def strip_dht(data):
    out, i = bytearray(data[:2]), 2
    while data[i + 1] != 0xDA:
        n = int.from_bytes(data[i + 2:i + 4], "big")
        if data[i + 1] != 0xC4:
            out += data[i:i + 2 + n]
        i += 2 + n
    return bytes(out + data[i:])


def test_missing_dht_means_annex_k():
    from dynamicrafter_amd.utils import load_video as L
    for mode in (0, 1, 2, "L"):
        data = pillow_file(frames("smooth", (24, 40))[0], mode, 90, optimize=False, rst=3)
        bare = strip_dht(data)
        assert b"\xff\xc4" not in bare[:bare.index(b"\xff\xda")] and len(bare) < len(data)
        a, b = L.parse_jpeg(data), L.parse_jpeg(bare)
        for key, (bits, vals) in a.huff.items():              # a grey file carries two of the four tables
            assert (bytes(bits), bytes(vals)) == tuple(bytes(x) for x in b.huff[key])
        same_parse(bare)
        assert np.array_equal(D.coefficients(bare), D.coefficients(data))
        assert np.array_equal(D.pixels(bare), D.pixels(data))


def test_frame_table_block_layout():
    """The per-frame block the kernels read (DC_JPEG_FRAME_TAB_BYTES): Huffman tables by class and id, quantisation tables in
    zigzag order, selectors per component."""
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.utils import load_video as L
    data = pillow_file(frames("noise", (24, 40))[0], 1, 90, optimize=True)
    info = L.parse_jpeg(data)
    tab = L._frame_table(info)
    assert tab.size == ops.JPEG_FRAME_TAB_BYTES == 1352
    p = D.parse(data)
    for (tc, th), (bits, vals) in p["huff"].items():
        at = (2 * tc + th) * 272
        assert bytes(tab[at:at + 16]) == bytes(bits) and bytes(tab[at + 16:at + 16 + len(vals)]) == bytes(vals)
        assert not tab[at + 16 + len(vals):at + 272].any()
    for tq, q in p["q"].items():
        assert tab[1088 + 64 * tq:1152 + 64 * tq].tolist() == q.tolist()
    assert tab[1344:1350].tolist() == [0x00, 0x11, 0x11, 0, 1, 1]
    buf, layout = L.pack_jpeg_batch([data, data])
    n_seg = layout["seg"][1]
    seg = buf[:20 * n_seg].view(np.int32).reshape(n_seg, 5)
    assert n_seg == 2 and layout["max_spf"] == 1 and seg[:, 4].tolist() == [0, 1] and seg[:, 2].tolist() == [0, 0]
    assert seg[:, 3].tolist() == [info.mcus] * 2 and seg[1, 0] == seg[0, 1]
    lo, hi = info.scan
    o = layout["scan"][0]
    assert bytes(buf[o:o + seg[0, 1]]) == data[lo:hi] and buf[layout["frame_seg"]:][:12].view(np.int32).tolist() == [0, 1, 2]


# ------------------------------------------------------------------------------------------------ 4. the AVI reader
def _riff(tag, body):
    return tag + struct.pack("<I", len(body)) + body + (b"\x00" if len(body) & 1 else b"")


def _avi(movi, handler=b"MJPG", compression=b"MJPG", rate=25, scale=2, size=(40, 24), extra_stream=b""):
    strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", handler, 0, 0, 0, 0, scale, rate, 0, 4, 0, 0xFFFFFFFF, 0, 0, 0, *size)
    strf = struct.pack("<IiiHH4sIiiII", 40, size[0], size[1], 1, 24, compression, 0, 0, 0, 0, 0)
    strl = _riff(b"LIST", b"strl" + _riff(b"strh", strh) + _riff(b"strf", strf))
    hdrl = _riff(b"LIST", b"hdrl" + _riff(b"avih", bytes(56)) + extra_stream + strl)
    body = b"AVI " + hdrl + _riff(b"JUNK", bytes(13)) + _riff(b"LIST", b"movi" + movi) + _riff(b"idx1", bytes(16))
    return b"RIFF" + struct.pack("<I", len(body)) + body


def test_avi_reader_on_the_writers_file(tmp_path):
    from dynamicrafter_amd.utils import load_video as L
    from dynamicrafter_amd.utils import save_video as S
    files = J.encode(frames("smooth", (24, 40), 3), 90)
    p = S.write_avi_mjpeg(str(tmp_path / "clip.avi"), files, 40, 24, 8)
    w, h, fps, got = L.read_avi_mjpeg(p)
    assert (w, h, fps) == (40, 24, 8.0) and got == files


def test_avi_reader_on_a_hand_built_file(tmp_path):
    """A `rec ` list, a JUNK chunk inside movi, an odd-sized chunk (padded), an empty chunk (repeats the previous frame), the
    chunks of another stream, `00db`, a lower-case handler; rate / scale = 12.5."""
    from dynamicrafter_amd.utils import load_video as L
    a, b, c = (J.encode(frames("noise", (24, 40), 3), q)[t] for t, q in enumerate((50, 90, 100)))
    if len(a) % 2 == 0:
        a += b"\x00"                                             # an odd-sized chunk; bytes behind EOI are ignored by decoders
    assert len(a) % 2 == 1
    movi = (_riff(b"00dc", a) + _riff(b"JUNK", bytes(7)) + _riff(b"01wb", bytes(10))
            + _riff(b"LIST", b"rec " + _riff(b"00dc", b) + _riff(b"00dc", b"") + _riff(b"01wb", bytes(3))) + _riff(b"00db", c)
            + _riff(b"00dc", b""))
    path = tmp_path / "hand.avi"
    path.write_bytes(_avi(movi, handler=b"mjpg", compression=b"\x00\x00\x00\x00"))
    w, h, fps, got = L.read_avi_mjpeg(str(path))
    assert (w, h, fps) == (40, 24, 12.5) and got == [a, b, b, c, c]
    path.write_bytes(_avi(movi, handler=b"\x00\x00\x00\x00", compression=b"mjpg"))             # named by biCompression alone
    assert L.read_avi_mjpeg(str(path))[3] == [a, b, b, c, c]
    # the video stream is the second one: its chunks are 01dc
    audio = _riff(b"LIST", b"strl" + _riff(b"strh", b"auds" + bytes(52)) + _riff(b"strf", bytes(16)))
    path.write_bytes(_avi(_riff(b"00wb", bytes(9)) + _riff(b"01dc", b) + _riff(b"00dc", a), extra_stream=audio))
    assert L.read_avi_mjpeg(str(path))[3] == [b]
    # trailing data behind the first RIFF (an OpenDML AVIX part) is not read
    path.write_bytes(_avi(_riff(b"00dc", b)) + b"RIFF" + struct.pack("<I", 4 + 8 + len(c)) + b"AVIX" + _riff(b"00dc", c))
    assert L.read_avi_mjpeg(str(path))[3] == [b]


def test_avi_reader_refuses_other_codecs(tmp_path):
    from dynamicrafter_amd.utils import load_video as L
    path = tmp_path / "h264.avi"
    path.write_bytes(_avi(_riff(b"00dc", bytes(20)), handler=b"H264", compression=b"H264"))
    with pytest.raises(ValueError, match="H264"):
        L.read_avi_mjpeg(str(path))
    path.write_bytes(b"RIFF" + struct.pack("<I", 4) + b"WAVE")
    with pytest.raises(ValueError, match="not an AVI"):
        L.read_avi_mjpeg(str(path))
    with pytest.raises(ValueError, match="only .avi"):
        L.read_video(str(tmp_path / "clip.mp4"))


# ------------------------------------------------------------------------------------------------ 5. funcs
def reference_selection(total_frames, frame_stride, video_frames):
    """The formulas of the reference's load_video_batch: max_valid = (total - 1) // stride + 1; video_frames < 0 -> required =
    total and stride 1; query = min(required, max_valid); indices stride * i; padding = required - max_valid if positive."""
    max_valid = (total_frames - 1) // frame_stride + 1
    required = total_frames if video_frames < 0 else video_frames
    stride = 1 if video_frames < 0 else frame_stride
    return [stride * i for i in range(min(required, max_valid))], max(required - max_valid, 0), stride


@pytest.mark.parametrize("case", [(16, 1, 16), (16, 2, 16), (5, 3, 16), (7, 1, -1), (1, 4, 2)], ids=str)
def test_frame_selection_follows_the_reference(case):
    from dynamicrafter_amd.scripts.evaluation import funcs
    got = funcs.video_frame_indices(*case)
    assert got == reference_selection(*case)
    total, stride, frames_ = case
    idx, pad, _ = got
    assert all(0 <= i < total for i in idx) and len(idx) + pad == (total if frames_ < 0 else frames_)
    expect = {(16, 1, 16): (list(range(16)), 0), (16, 2, 16): (list(range(0, 16, 2)), 8), (5, 3, 16): ([0, 3], 14),
              (7, 1, -1): (list(range(7)), 0), (1, 4, 2): ([0], 1)}[case]
    assert (idx, pad) == expect
    with pytest.raises(ValueError):
        funcs.video_frame_indices(16, 0, 16)


def test_unchanged_refusals(tmp_path):
    from dynamicrafter_amd.scripts.evaluation import funcs
    with pytest.raises(NotImplementedError):
        funcs.load_video_batch(["x.mp4"], 1)
    with pytest.raises(NotImplementedError):
        funcs.load_video_batch([str(tmp_path / "clip.avi"), "x.mkv"], 1)                        # before any file is opened
    with pytest.raises(NotImplementedError):
        funcs.load_image_batch(["x.mp4"], (32, 48), device="cuda:0")
    with pytest.raises(NotImplementedError):
        funcs.load_image_batch(["x.bmp"], (32, 48), device="cuda:0")
    with pytest.raises(RuntimeError):
        funcs.load_video_batch([str(tmp_path / "clip.avi")], 1, device="cpu")
    from dynamicrafter_amd.utils import load_video as L
    with pytest.raises(RuntimeError):
        L.decode_jpeg_frames(J.encode(frames("noise", (16, 16)), 90), device="cpu")


def test_load_video_imports_without_torch_at_module_level():
    import subprocess
    import sys
    code = ("import sys, importlib.util as u; s = u.spec_from_file_location('lv', sys.argv[1]); m = u.module_from_spec(s); "
            "s.loader.exec_module(m); assert 'torch' not in sys.modules; print('ok')")
    from dynamicrafter_amd.utils import load_video as L
    r = subprocess.run([sys.executable, "-c", code, L.__file__], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


# ------------------------------------------------------------------------------------------------ 6. C entries
def test_decode_entries_reject_bad_arguments_without_gpu():
    """Null pointers -> DC_ERR_ARG (-2); a bad shape or a sampling the decoder does not take -> DC_ERR_SHAPE (-1); all before
    any HIP call."""
    from dynamicrafter_amd import _hip
    lib = _hip.lib()
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    ent = lambda *a: lib.dc_jpeg_decode_entropy(*a)
    ok = [p, 16, p, p, p, p, p, 1, 1, 1, 1, 3, 2, 2, 1, None]
    for k in (0, 2, 3, 4, 5, 6):
        assert ent(*[None if i == k else v for i, v in enumerate(ok)]) == -2
    for k, v in ((1, 0), (7, 0), (8, 0), (8, 65536), (9, 0), (10, 0), (11, 2), (11, 4), (12, 3), (13, 0), (14, 0)):
        assert ent(*[v if i == k else x for i, x in enumerate(ok)]) == -1, (k, v)
    assert ent(p, 16, p, p, p, p, p, 1, 1, 1, 1, 3, 1, 2, 1, None) == -1                       # luma 1x2
    assert ent(p, 16, p, p, p, p, p, 1, 1, 1, 1, 1, 2, 2, 1, None) == -1                       # grey is 1x1
    assert ent(p, 16, p, p, p, p, p, 1, 1, 1 << 15, 1 << 15, 3, 2, 2, 1, None) == -1           # MCU count overflows
    assert lib.dc_jpeg_decode_idct(None, p, p, 1, 1, 1, 3, 2, 2, None) == -2
    assert lib.dc_jpeg_decode_idct(p, None, p, 1, 1, 1, 3, 2, 2, None) == -2
    assert lib.dc_jpeg_decode_idct(p, p, None, 1, 1, 1, 3, 2, 2, None) == -2
    assert lib.dc_jpeg_decode_idct(p, p, p, 0, 1, 1, 3, 2, 2, None) == -1
    assert lib.dc_jpeg_decode_idct(p, p, p, 1, 1, 0, 3, 2, 2, None) == -1
    assert lib.dc_jpeg_decode_idct(p, p, p, 1, 1, 1, 3, 2, 3, None) == -1
    assert lib.dc_jpeg_decode_output(None, p, 1, 16, 16, 3, 2, 2, 0, None) == -2
    assert lib.dc_jpeg_decode_output(p, None, 1, 16, 16, 3, 2, 2, 0, None) == -2
    assert lib.dc_jpeg_decode_output(p, p, 1, 0, 16, 3, 2, 2, 0, None) == -1
    assert lib.dc_jpeg_decode_output(p, p, 1, 16, 65536, 3, 2, 2, 0, None) == -1
    assert lib.dc_jpeg_decode_output(p, p, 1, 16, 16, 2, 1, 1, 0, None) == -1
    assert lib.dc_jpeg_decode_output(p, p, 1, 16, 16, 3, 2, 2, 2, None) == -1


def test_host_wrappers_refuse_cpu_tensors():
    import torch
    from dynamicrafter_amd import ops
    u8, i16, i32 = (torch.zeros(4096, dtype=d) for d in (torch.uint8, torch.int16, torch.int32))
    with pytest.raises(ValueError):
        ops.jpeg_decode_entropy(u8, i32[:5], i32[:2], u8, i16, i32[:1], T=1, my=1, mx=1, ncomp=3, hs=2, vs=2, max_segs_per_frame=1)
    with pytest.raises(ValueError):
        ops.jpeg_decode_idct(i16, u8, u8, T=1, my=1, mx=1, ncomp=3, hs=2, vs=2)
    with pytest.raises(ValueError):
        ops.jpeg_decode_output(u8, u8, T=1, H=16, W=16, ncomp=3, hs=2, vs=2)
    with pytest.raises(ValueError):
        ops.jpeg_decode_geometry(16, 16, 3, 1, 2)
    assert ops.jpeg_decode_geometry(37, 53, 3, 2, 2) == (3, 4, 6, 3 * 4 * 384)
    assert ops.jpeg_decode_geometry(37, 53, 3, 2, 1) == (5, 4, 4, 5 * 4 * 256)
    assert ops.jpeg_decode_geometry(37, 53, 1, 1, 1) == (5, 7, 1, 35 * 64)

"""Motion-JPEG output, the parts that need no GPU: the quantisation and Huffman tables against the ones Pillow (libjpeg)
writes, the restatement (tests/jpeg_restatement.py - the reference of the GPU tests) against Pillow's decoder and encoder, the
AVI writer through a RIFF walker, and the argument checks of the three dc_jpeg_* entries."""
import ctypes as C
import io
import os
import struct

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_restatement as J

SIZES = [(40, 72), (16, 16), (33, 17), (1, 1)]
PSNR_MARGIN_DB = 0.25       # five times the largest shortfall of the float64 restatement against libjpeg's integer DCT (0.05 dB)


def _pillow_jpeg(frame, q):
    b = io.BytesIO()
    Image.fromarray(frame).save(b, "JPEG", quality=q, subsampling=2, optimize=False)
    return b.getvalue()


def _decode(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


@pytest.mark.parametrize("q", [10, 50, 90, 100])
def test_tables_equal_the_ones_pillow_writes(q):
    from dynamicrafter_amd.utils import save_video as S
    ref = J.markers(_pillow_jpeg(J.make_frames("smooth", 1, 16, 16, np.random.default_rng(1))[0], q))
    dqt = b"".join(p for m, p in ref if m == 0xDB)
    dqt = {dqt[i]: dqt[i + 1:i + 65] for i in range(0, len(dqt), 65)}
    nat, zz = S.jpeg_quant_tables(q)
    assert nat.shape == zz.shape == (2, 64)
    for i in range(2):
        assert bytes(bytearray(zz[i].tolist())) == dqt[i]
        assert (nat[i][list(S.JPEG_ZIGZAG)] == zz[i]).all()
        assert (nat[i] == J.quant_tables(q)[i]).all()
    ours = J.markers(S.jpeg_header(16, 16, zz, 1))
    dht = lambda ms: sorted(p for m, p in ms if m == 0xC4)
    mine, theirs = dht(ours), dht(ref)
    if len(theirs) == 1:                                         # one DHT segment may hold all four tables
        mine = [b"".join(p for m, p in ours if m == 0xC4)]
        theirs = [b"".join(p for m, p in ref if m == 0xC4)]
    assert len(b"".join(mine)) == 2 * (17 + 12) + 2 * (17 + 162)
    assert mine == theirs
    for bad in (0, 101):
        with pytest.raises(ValueError):
            S.jpeg_quant_tables(bad)


def test_header_layout():
    from dynamicrafter_amd.utils import save_video as S
    _, zz = S.jpeg_quant_tables(90)
    h = S.jpeg_header(72, 40, zz, 5)
    assert h == J.jfif(b"", 40, 72, J.quant_tables(90), 5)[:-2]                 # the restatement assembles the same bytes
    ms = J.markers(h)
    assert [m for m, _ in ms] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert ms[0][1][:7] == b"JFIF\x00\x01\x01"
    assert ms[3][1] == struct.pack(">BHHB", 8, 40, 72, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert ms[8][1] == struct.pack(">H", 5)


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_decodes_and_matches_pillows_encoder(kind, hw):
    """The restatement's files open in Pillow with the right size; per frame their PSNR against the source is at least that of
    Pillow's own encoder at the same tables minus 0.25 dB. (At 1x1 a PSNR has three samples and moves in steps of 3 dB; the two
    encoders land on the same step for these inputs.) float32 arithmetic gives the same coefficients as float64 here, which is
    what lets the GPU test cap the kernel's deviations at ties between summation orders."""
    H, W = hw
    f = J.make_frames(kind, 2, H, W, np.random.default_rng(1))
    for q in (50, 90, 100):
        qt = J.quant_tables(q)
        c64 = J.coefficients(f, qt)
        assert c64.shape == (2,) + J.mcu_grid(H, W) + (6, 64)
        assert int((c64 != J.coefficients(f, qt, np.float32)).sum()) == 0
        for ri in (1, J.mcu_grid(H, W)[1]):
            files = [J.jfif(J.entropy_scan(c64[t], ri), H, W, qt, ri) for t in range(2)]
            for t in range(2):
                im = _decode(files[t])
                assert im.size == (W, H) and im.mode == "RGB"
                ours = J.psnr(np.asarray(im), f[t])
                ref = J.psnr(np.asarray(_decode(_pillow_jpeg(f[t], q)).convert("RGB")), f[t])
                print(f"{kind} {H}x{W} q{q} ri{ri} frame {t}: restatement {ours:.3f} dB, Pillow {ref:.3f} dB")
                assert ours >= ref - PSNR_MARGIN_DB


def test_restatement_entropy_corner_cases_decode():
    """Runs above 15 (ZRL), a block that ends on coefficient 63 (no EOB), the longest codes, a stuffed 0xFF: the decoder must
    take every one of them, and read the very coefficients back (checked through the DC term of a flat block)."""
    z = np.zeros((1, 1, 6, 64), dtype=np.int16)
    z[..., 63] = 1
    assert len(J.entropy_segments(z[0], 1)[0]) > 6
    qt = J.quant_tables(100)
    _decode(J.jfif(J.entropy_scan(z[0], 1), 16, 16, qt, 1))
    rnd = np.random.default_rng(1).integers(-1023, 1024, size=(3, 5, 6, 64)).astype(np.int16)
    scan = J.entropy_scan(rnd, 1)
    assert b"\xff\x00" in scan and scan.count(b"\xff\xd7") >= 1
    _decode(J.jfif(scan, 40, 72, qt, 1))
    flat = np.zeros((1, 1, 6, 64), dtype=np.int16)
    flat[0, 0, :4, 0] = 40                                       # Y = 128 + 40 / 8 * q(=1) -> 133
    im = np.asarray(_decode(J.jfif(J.entropy_scan(flat[0], 1), 16, 16, qt, 1)).convert("YCbCr"))
    assert np.abs(im[..., 0].astype(int) - 133).max() <= 1 and np.abs(im[..., 1:].astype(int) - 128).max() <= 1


def test_avi_writer_through_a_riff_walker(tmp_path):
    from dynamicrafter_amd.utils import save_video as S
    H, W, fps = 33, 17, 8
    f = J.make_frames("smooth", 3, H, W, np.random.default_rng(1))
    frames = J.encode(f, 90, ri=1)
    path = S.write_avi_mjpeg(str(tmp_path / "sub" / "clip.avi"), frames, W, H, fps)
    data = open(path, "rb").read()
    r = J.walk_avi(data)                                         # asserts that sizes nest and sum to the file size
    assert set(r["chunks"]) == {"hdrl/avih", "hdrl/strl/strh", "hdrl/strl/strf", "idx1"}
    avih = struct.unpack("<14I", r["chunks"]["hdrl/avih"])
    assert avih[0] == 1000000 // fps and avih[3] & 0x10 and avih[4] == 3 and avih[6] == 1 and avih[8:10] == (W, H)
    strh = struct.unpack("<4s4sIHHIIIIIIIIhhhh", r["chunks"]["hdrl/strl/strh"])
    assert strh[0] == b"vids" and strh[1] == b"MJPG"
    scale, rate, length = strh[6], strh[7], strh[9]
    assert (scale, rate, length) == (1, fps, 3) and strh[-2:] == (W, H)
    strf = struct.unpack("<IiiHH4sIiiII", r["chunks"]["hdrl/strl/strf"])
    assert strf[:6] == (40, W, H, 1, 24, b"MJPG")
    assert r["frames"] == frames and len(r["idx"]) == 3
    for (ckid, flags, off, size), fr in zip(r["idx"], frames):
        at = r["movi"] + off
        assert ckid == b"00dc" and flags & 0x10 and data[at:at + 4] == b"00dc"
        assert struct.unpack("<I", data[at + 4:at + 8])[0] == size == len(fr)
        im = _decode(data[at + 8:at + 8 + size])
        assert im.size == (W, H)
    assert any(len(fr) % 2 for fr in frames), "no odd-length frame: the padding path is not exercised"
    with pytest.raises(ValueError):
        S.write_avi_mjpeg(str(tmp_path / "x.avi"), [], W, H, fps)
    with pytest.raises(ValueError):
        S.write_avi_mjpeg(str(tmp_path / "x.avi"), [b"not a jpeg"], W, H, fps)


def test_jpeg_entries_reject_bad_arguments_without_gpu():
    """Null pointers -> DC_ERR_ARG (-2); H < 1, ri < 1, a stride below the worst case, no segments -> DC_ERR_SHAPE (-1); all
    before any launch."""
    from dynamicrafter_amd import _hip
    lib = _hip.lib()
    p = C.c_void_p(8)
    assert lib.dc_jpeg_dct_quant(None, p, p, 1, 16, 16, None) == -2
    assert lib.dc_jpeg_dct_quant(p, None, p, 1, 16, 16, None) == -2
    assert lib.dc_jpeg_dct_quant(p, p, None, 1, 16, 16, None) == -2
    assert lib.dc_jpeg_dct_quant(p, p, p, 1, 0, 16, None) == -1
    assert lib.dc_jpeg_dct_quant(p, p, p, 1, 16, 0, None) == -1
    assert lib.dc_jpeg_dct_quant(p, p, p, 0, 16, 16, None) == -1
    stride = 3 * 2496 + 1
    assert lib.dc_jpeg_entropy(None, p, p, 1, 3, 5, 3, stride, None) == -2
    assert lib.dc_jpeg_entropy(p, None, p, 1, 3, 5, 3, stride, None) == -2
    assert lib.dc_jpeg_entropy(p, p, None, 1, 3, 5, 3, stride, None) == -2
    assert lib.dc_jpeg_entropy(p, p, p, 1, 3, 5, 0, stride, None) == -1
    assert lib.dc_jpeg_entropy(p, p, p, 1, 0, 5, 3, stride, None) == -1
    assert lib.dc_jpeg_entropy(p, p, p, 1, 3, 5, 3, stride - 1, None) == -1
    assert lib.dc_jpeg_pack(None, p, p, p, p, 1, 5, stride, 100, None) == -2
    assert lib.dc_jpeg_pack(p, p, p, None, p, 1, 5, stride, 100, None) == -2
    assert lib.dc_jpeg_pack(p, p, p, p, None, 1, 5, stride, 100, None) == -2
    assert lib.dc_jpeg_pack(p, p, p, p, p, 1, 0, stride, 100, None) == -1
    assert lib.dc_jpeg_pack(p, p, p, p, p, 0, 5, stride, 100, None) == -1
    assert lib.dc_jpeg_pack(p, p, p, p, p, 1, 5, stride, 0, None) == -1
    hdr = open(os.path.join(os.path.dirname(_hip._HERE), "include", "dcrafter_hip.h")).read()
    assert "#define DC_JPEG_MCU_MAX_BYTES 2496" in hdr and J.MCU_MAX_BYTES == 2496


def test_host_entry_points_refuse_cpu_tensors_and_other_channel_counts():
    import torch
    from dynamicrafter_amd.utils import save_video as S
    with pytest.raises(RuntimeError):
        S.encode_jpeg_frames(torch.zeros(1, 16, 16, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        S._write_clip("x", torch.zeros(1, 16, 16, 3, dtype=torch.uint8), 8, "mp4", 90)

"""Output side of the harness: decoded clips -> files (second half).

Counterpart of the reference's `save_results` / `save_results_seperate` (scripts/evaluation/inference.py:115-162) and
`tensor_to_mp4` (utils/save_video.py:27-43). Their arithmetic - clamp to [-1,1], (v+1)/2, x255, uint8 truncation, the
n clips of a batch side by side (`make_grid(nrow=n, padding=0)`), frames as [t, h, w, c] - is one HIP kernel
(`dc_frames_to_u8`) on the decoded tensor where it lies. The container differs: the reference hands the frames to
torchvision.io.write_video (h264, crf 10); no h264 encoder exists in this image, so by default clips are written as APNG
(animated PNG: lossless, zlib only, one file per clip, plays in browsers) and single frames as PNG. File names keep the
reference's stems; only the extension changes (.png instead of .mp4).

The PNG writers take `deflate=`: "zlib" is the host path (the frames travel to the CPU, zlib level 6 on filter-0 scanlines, frame
after frame) and what they do when nothing is said; "hip" keeps the frames on the GPU: per row the PNG filter with the least
sum of absolute residuals, then every 16 KiB of scanlines deflated on their own into whole bytes - run-length matches, one
dynamic-Huffman block, or a stored block where that is not shorter - and packed behind 78 01 with the Adler-32 combined from the
chunks (csrc/png.hip: filter, deflate of one chunk per wave, pack). Only the zlib streams travel to the host, which adds the chunk
framing and the CRCs. `deflate=None` reads the environment variable DC_PNG_DEFLATE (so the generate command line reaches the HIP
path without a new flag) and falls back to "zlib". DESIGN.md 4.10.

`container="avi"` writes a video file instead: Motion-JPEG in an AVI container. The frames are encoded as baseline JPEG
(T.81 SOF0, YCbCr 4:2:0, Annex K tables scaled by `quality` as libjpeg does, restart intervals) by three HIP launches on
the uint8 frames where they lie (csrc/jpeg.hip: coefficients, entropy coding of one restart segment per wave, pack); only the
packed scans travel to the host, which adds the JFIF headers and the RIFF structure.

`container="gif"` writes an animated GIF89a, the format the reference's gallery is shared in: one global colour table of up to
256 entries for the whole clip (built on the host from a 15-bit histogram the GPU counts), every pixel mapped to its nearest
entry, optionally behind an ordered dither, and LZW-coded in independent chunks (csrc/gif.hip: histogram, map, LZW of one chunk
per wave, pack); only the packed image data travels to the host. A GIF frame lasts a whole number of centiseconds, at least 2:
the file plays at 100 / delay frames per second, delay = max(2, floor(100 / fps + 0.5)), not at `fps` (8 -> 13 cs = 7.69 fps).
"""
import ctypes as C
import math
import os
import struct
import zlib

import numpy as np
import torch

from .. import _hip, ops
from ..ops import stream_ptr


def frames_to_uint8(video):
    """video [n, c, t, h, w] fp32 on the GPU, values nominally in [-1, 1] -> uint8 [t, h, n*w, c] (same device)."""
    if not video.is_cuda:
        raise RuntimeError("frames_to_uint8 runs on the HIP path only (there is no CPU fallback)")
    if video.dim() != 5:
        raise ValueError(f"expected [n, c, t, h, w], got {tuple(video.shape)}")
    v = video.detach().to(torch.float32).contiguous()
    n, c, t, h, w = v.shape
    out = torch.empty((t, h, n * w, c), dtype=torch.uint8, device=v.device)
    _hip.check(_hip.lib().dc_frames_to_u8(C.c_void_p(v.data_ptr()), C.c_void_p(out.data_ptr()), n, c, t, h, w, stream_ptr()),
               "dc_frames_to_u8")
    return out


# ---------------------------------------------------------------------------------------------- what the GPU encoders share
_ENCODE_SCRATCH_BYTES = 256 << 20        # coder scratch per batch of frames (worst-case sized rows)


def _gpu_u8_frames(name, frames, channels, hint, ndim=4):
    """The input check of the GPU encoders: a CUDA uint8 [(t,) h, w, c] tensor with c in `channels`, returned contiguous.
    RuntimeError for what is not on the GPU (`hint` says what there is instead), ValueError for any other dtype or shape."""
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise RuntimeError(f"{name} runs on the HIP path only ({hint})")
    if frames.dtype != torch.uint8 or frames.dim() != ndim or frames.shape[-1] not in channels:
        want = ("t, " if ndim == 4 else "") + "h, w, " + "|".join(map(str, channels))
        raise ValueError(f"{name}: uint8 [{want}] expected, got {frames.dtype} {tuple(frames.shape)}"
                         + ("" if len(channels) > 1 else " (APNG takes 1 and 4 channels)"))
    return frames.contiguous()


def _encode_batches(name, f, stage, n_words, rows_per_frame, stride, frame_stride, bound, code, pack):
    """The batch loop of the GPU encoders (stream_pack.h): f uint8 [t, ...] on the GPU -> t byte strings, one packed
    stream per frame. A coder writes rows_per_frame strings per frame into scratch rows of `stride` bytes, the pack gathers them into one
    row of frame_stride bytes per frame. Frames per batch: what _ENCODE_SCRATCH_BYTES of scratch hold, at most 65535 (a pack
    launches one workgroup row per frame: gridDim.y). Per batch `code(frames, stage, scratch, words, n)` launches the stages in
    front of the pack for the n frames given and `pack(scratch, words, out, frame_len, n, frame_stride)` the pack; `stage` =
    (elements per frame, dtype) of the coder's intermediate buffer, `words` = n_words int32 buffers with one element per
    scratch row (lengths, offsets). Then frame_len comes back, the used part of the rows in one device-to-host copy, and the
    rows are sliced. `bound` says whether frame_stride is a proven worst case (a longer frame is an error) or a guess (the
    pack dropped the excess and reported the full length: it runs once more into rows that wide)."""
    t, dev = f.shape[0], f.device
    tb = max(1, min(t, 65535, _ENCODE_SCRATCH_BYTES // (rows_per_frame * stride)))
    stage = torch.empty(tb * stage[0], dtype=stage[1], device=dev)
    scratch = torch.empty(tb * rows_per_frame * stride, dtype=torch.uint8, device=dev)
    words = [torch.empty(tb * rows_per_frame, dtype=torch.int32, device=dev) for _ in range(n_words)]
    frame_len = torch.empty(tb, dtype=torch.int32, device=dev)
    out = torch.empty(tb * frame_stride, dtype=torch.uint8, device=dev)
    streams = []
    for t0 in range(0, t, tb):
        n = min(tb, t - t0)
        code(f[t0:t0 + n], stage, scratch, words, n)
        pack(scratch, words, out, frame_len, n, frame_stride)
        lens = frame_len[:n].cpu().tolist()
        if max(lens) > frame_stride:
            if bound:
                raise RuntimeError(f"{name}: a frame of {max(lens)} bytes outgrew the worst case {frame_stride}")
            frame_stride = max(lens)             # a frame outgrew the guess (the kernel dropped the excess): pack into wider rows
            out = torch.empty(tb * frame_stride, dtype=torch.uint8, device=dev)
            pack(scratch, words, out, frame_len, n, frame_stride)
        host = out[:n * frame_stride].view(n, frame_stride)[:, :max(lens)].cpu().numpy()
        streams += [host[i, :lens[i]].tobytes() for i in range(n)]
    return streams


# ---------------------------------------------------------------------------------------------- PNG / APNG (zlib, or csrc/png.hip)
def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def _ihdr(w, h, c):
    color = {1: 0, 3: 2, 4: 6}[c]
    return _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color, 0, 0, 0))


def _scanlines(frame, level):
    """uint8 [h, w, c] -> zlib stream of filter-0 scanlines"""
    h = frame.shape[0]
    raw = np.empty((h, 1 + frame.shape[1] * frame.shape[2]), dtype=np.uint8)
    raw[:, 0] = 0
    raw[:, 1:] = frame.reshape(h, -1)
    return zlib.compress(raw.tobytes(), level)


def png_deflate_mode(deflate=None):
    """"zlib" (the host compressor on filter-0 scanlines) or "hip" (csrc/png.hip); None reads the environment variable
    DC_PNG_DEFLATE and falls back to "zlib"."""
    if deflate is None:
        deflate = os.environ.get("DC_PNG_DEFLATE") or "zlib"
    if deflate not in ("zlib", "hip"):
        raise ValueError(f"deflate must be 'zlib' or 'hip', got {deflate!r}")
    return deflate


def encode_png_frames(frames_u8, chunk=None):
    """frames_u8: uint8 [t, h, w, c] on the GPU (what frames_to_uint8 returns; c in 1, 3, 4) -> list of t zlib streams (bytes), the
    payload of an IDAT / fdAT chunk each. Lossless: adaptive row filters, then every `chunk` bytes of scanlines (default
    ops.PNG_CHUNK, at most 65535) deflated on their own with run-length matches and dynamic Huffman tables, or stored where that is
    not shorter. Three launches per batch of frames and one device-to-host copy of the packed streams."""
    f = _gpu_u8_frames("encode_png_frames", frames_u8, (1, 3, 4), "deflate='zlib' is the host path")
    t, h, w, c = f.shape
    N = h * (1 + w * c)
    if t < 1 or h < 1 or w < 1 or N > 0x7FFFFFFF:
        raise ValueError(f"encode_png_frames: frames of {h} x {w} x {c} x {t}")
    chunk = ops.PNG_CHUNK if chunk is None else int(chunk)
    if not 1 <= chunk <= ops.PNG_CHUNK_LIMIT:
        raise ValueError(f"chunk must be in 1..{ops.PNG_CHUNK_LIMIT} bytes, got {chunk}")
    stride = ops.png_chunk_max_bytes(min(chunk, N))

    def code(frames, planes, scratch, words, n):
        ops.png_filter(frames, planes)
        ops.png_deflate(planes, scratch, words[0], words[1], T=n, N=N, chunk=chunk, stride=stride)

    def pack(scratch, words, out, frame_len, n, frame_stride):
        ops.png_pack(scratch, *words, out, frame_len, T=n, N=N, chunk=chunk, stride=stride, frame_stride=frame_stride)

    return _encode_batches("encode_png_frames", f, (N, torch.uint8), 3, (N + chunk - 1) // chunk, stride,
                           ops.png_frame_max_bytes(N, chunk), True, code, pack)


def _hip_streams(name, frames, ndim):
    """The zlib streams of deflate="hip" for uint8 [(t,) h, w, c] on the GPU; refuses everything else before a file exists."""
    f = _gpu_u8_frames(f"{name}: deflate='hip'", frames, (1, 3, 4), "deflate='zlib' takes numpy and CPU tensors", ndim)
    return encode_png_frames(f if ndim == 4 else f[None])


def _png_file(w, h, c, stream):
    return b"\x89PNG\r\n\x1a\n" + _ihdr(w, h, c) + _chunk(b"IDAT", stream) + _chunk(b"IEND", b"")


def write_png(path, frame, level=6, deflate=None):
    """frame: uint8 [h, w, c] (c in 1, 3, 4), numpy or tensor. `deflate`: "zlib" (zlib at `level` on filter-0 scanlines, on the
    host), "hip" (encode_png_frames; a CUDA tensor only) or None = png_deflate_mode()."""
    if png_deflate_mode(deflate) == "hip":
        stream, = _hip_streams("write_png", frame, 3)
        shape = frame.shape
    else:
        f = np.ascontiguousarray(frame.cpu().numpy() if isinstance(frame, torch.Tensor) else frame)
        if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] not in (1, 3, 4):
            raise ValueError(f"write_png: uint8 [h, w, 1|3|4] expected, got {f.dtype} {f.shape}")
        stream, shape = _scanlines(f, level), f.shape
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(_png_file(shape[1], shape[0], shape[2], stream))
    return path


def write_apng(path, frames, fps=8, level=6, loops=0, deflate=None):
    """frames: uint8 [t, h, w, c]. Animated PNG (acTL / fcTL / fdAT): frame 0 doubles as the still image every PNG
    reader shows; `loops` = 0 repeats forever. `deflate` as in write_png; the chunk framing is the same for both."""
    if png_deflate_mode(deflate) == "hip":
        streams = _hip_streams("write_apng", frames, 4)
        t, h, w, c = frames.shape
    else:
        f = np.ascontiguousarray(frames.cpu().numpy() if isinstance(frames, torch.Tensor) else frames)
        if f.dtype != np.uint8 or f.ndim != 4 or f.shape[3] not in (1, 3, 4):
            raise ValueError(f"write_apng: uint8 [t, h, w, 1|3|4] expected, got {f.dtype} {f.shape}")
        t, h, w, c = f.shape
        streams = None
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    seq = 0
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + _ihdr(w, h, c) + _chunk(b"acTL", struct.pack(">II", t, loops)))
        for i in range(t):
            fh.write(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, 0, 0, 1, int(fps), 0, 0)))
            seq += 1
            data = streams[i] if streams is not None else _scanlines(f[i], level)
            if i == 0:
                fh.write(_chunk(b"IDAT", data))
            else:
                fh.write(_chunk(b"fdAT", struct.pack(">I", seq) + data))
                seq += 1
        fh.write(_chunk(b"IEND", b""))
    return path


# ---------------------------------------------------------------------------------------------- baseline JPEG / MJPEG AVI
# ITU-T T.81 Annex K.1 / K.2 quantisation tables (natural, row-major order)
_K1_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
            14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
            49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_K2_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
              47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# zigzag scan (T.81 figure 5): JPEG_ZIGZAG[k] = 8 * row + col of the k-th coefficient
JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
               28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
               47, 55, 62, 63)
# Annex K.3 - K.6 Huffman tables as DHT payloads (class/id byte, BITS, HUFFVAL), in the order libjpeg writes them; the kernels
# carry the same tables (csrc/jpeg.hip)
_AC_COMMON = ("535455565758595a636465666768696a737475767778797a", "92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6"
              "c7c8c9cad2d3d4d5d6d7d8d9da")
JPEG_DHT = (
    bytes.fromhex("00" "00010501010101010100000000000000" "000102030405060708090a0b"),
    bytes.fromhex("10" "0002010303020403050504040000017d" "01020300041105122131410613516107227114328191a1082342b1c11552d1f024"
                  "33627282090a161718191a25262728292a3435363738393a434445464748494a" + _AC_COMMON[0] + "838485868788898a"
                  + _AC_COMMON[1] + "e1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"),
    bytes.fromhex("01" "00030101010101010101010000000000" "000102030405060708090a0b"),
    bytes.fromhex("11" "00020102040403040705040400010277" "000102031104052131061241510761711322328108144291a1b1c109233352f015"
                  "6272d10a162434e125f11718191a262728292a35363738393a434445464748494a" + _AC_COMMON[0] + "82838485868788898a"
                  + _AC_COMMON[1] + "e2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"),
)


def jpeg_quant_tables(quality):
    """(natural, zigzag): the luminance and chrominance tables uint8 [2, 64] for `quality` in 1..100, row-major and in zigzag
    order (as a DQT segment and the kernels hold them). Annex K scaled by libjpeg's rule: s = 5000 / q below 50, else
    200 - 2 q; entry = clamp((base * s + 50) / 100, 1, 255), integer arithmetic."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"JPEG quality must be in 1..100, got {quality}")
    s = 5000 // q if q < 50 else 200 - 2 * q
    nat = np.array([[min(max((b * s + 50) // 100, 1), 255) for b in base] for base in (_K1_LUMA, _K2_CHROMA)], dtype=np.uint8)
    return nat, np.ascontiguousarray(nat[:, list(JPEG_ZIGZAG)])


def _marker(m, payload):
    return bytes((0xFF, m)) + struct.pack(">H", len(payload) + 2) + payload


def jpeg_header(width, height, qtab_zigzag, restart_mcus):
    """SOI, APP0 (JFIF 1.01), 2 x DQT, SOF0 (Y 2x2 / table 0, Cb and Cr 1x1 / table 1), 4 x DHT, DRI, SOS: everything in
    front of the entropy-coded scan."""
    out = b"\xff\xd8" + _marker(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i in range(2):
        out += _marker(0xDB, bytes((i,)) + bytes(bytearray(int(v) for v in qtab_zigzag[i])))
    out += _marker(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes((1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for t in JPEG_DHT:
        out += _marker(0xC4, t)
    out += _marker(0xDD, struct.pack(">H", restart_mcus))
    return out + _marker(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


def encode_jpeg_frames(frames_u8, quality=90, restart_mcus=None):
    """frames_u8: uint8 [t, h, w, 3] on the GPU (what frames_to_uint8 returns) -> list of t complete JFIF files (bytes).
    Baseline JPEG, YCbCr 4:2:0; `restart_mcus` = MCUs (16x16 pixels) per restart interval, i.e. per independently coded
    segment (default 8, or the whole frame if it is smaller). Three launches per batch of frames, one device-to-host copy of
    the packed scans."""
    f = _gpu_u8_frames("encode_jpeg_frames", frames_u8, (3,), "there is no CPU fallback")
    t, h, w, _ = f.shape
    if t < 1 or not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f"encode_jpeg_frames: frames of {h} x {w} x {t}")
    my, mx = ops.jpeg_mcu_grid(h, w)
    nmcu = my * mx
    ri = min(8, nmcu) if restart_mcus is None else int(restart_mcus)
    if not 1 <= ri <= 65535:
        raise ValueError(f"restart_mcus must be in 1..65535, got {restart_mcus}")
    _, qz = jpeg_quant_tables(quality)
    header = jpeg_header(w, h, qz, ri)
    qtab = torch.from_numpy(qz).to(f.device)
    spf = (nmcu + ri - 1) // ri
    stride = min(ri, nmcu) * ops.JPEG_MCU_MAX_BYTES + 1

    def code(frames, coef, scratch, words, n):
        ops.jpeg_dct_quant(frames, qtab, coef)
        ops.jpeg_entropy(coef, scratch, words[0], T=n, my=my, mx=mx, ri=ri, stride=stride)

    def pack(scratch, words, out, frame_len, n, frame_stride):
        ops.jpeg_pack(scratch, *words, out, frame_len, T=n, segs_per_frame=spf, stride=stride, frame_stride=frame_stride)

    # rows of 1.5 bytes per pixel: a first guess far above typical frames, not a bound
    scans = _encode_batches("encode_jpeg_frames", f, (nmcu * 384, torch.int16), 2, spf, stride, nmcu * 384 + 2 * spf, False,
                            code, pack)
    return [header + scan + b"\xff\xd9" for scan in scans]


def write_jpeg(path, frame_u8, quality=90):
    """frame_u8: uint8 [h, w, 3] on the GPU -> one JFIF file."""
    if not isinstance(frame_u8, torch.Tensor) or frame_u8.dim() != 3:
        raise ValueError("write_jpeg: a uint8 [h, w, 3] GPU tensor expected")
    data = encode_jpeg_frames(frame_u8[None], quality=quality)[0]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(data)
    return path


def _riff(tag, data):
    return tag + struct.pack("<I", len(data)) + data + (b"\x00" if len(data) & 1 else b"")


def _riff_list(kind, data):
    return _riff(b"LIST", kind + data)


def write_avi_mjpeg(path, jpeg_frames, width, height, fps):
    """jpeg_frames: JFIF files (bytes) of width x height -> AVI 1.0 with one Motion-JPEG video stream at `fps` frames per
    second (an integer: scale 1, rate fps). Layout: RIFF 'AVI ' { LIST hdrl { avih, LIST strl { strh, strf } }, LIST movi
    { 00dc ... }, idx1 }; every frame is a key frame; idx1 offsets count from the 'movi' fourcc. Pure host code."""
    frames = [bytes(f) for f in jpeg_frames]
    rate = int(fps)
    if not frames or rate < 1 or rate != fps or width < 1 or height < 1:
        raise ValueError(f"write_avi_mjpeg: {len(frames)} frames of {width} x {height} at {fps} fps")
    if any(f[:2] != b"\xff\xd8" for f in frames):
        raise ValueError("write_avi_mjpeg: every frame must be a JPEG file (SOI first)")
    n, biggest = len(frames), max(len(f) for f in frames)
    avih = struct.pack("<14I", 1000000 // rate, biggest * rate, 0, 0x10, n, 0, 1, biggest, width, height, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", b"MJPG", 0, 0, 0, 0, 1, rate, 0, n, biggest, 0xFFFFFFFF, 0,
                       0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    hdrl = _riff_list(b"hdrl", _riff(b"avih", avih) + _riff_list(b"strl", _riff(b"strh", strh) + _riff(b"strf", strf)))
    movi, idx, pos = [], [], 4                                   # pos: offset of the next chunk from the 'movi' fourcc
    for f in frames:
        ck = _riff(b"00dc", f)
        idx.append(struct.pack("<4sIII", b"00dc", 0x10, pos, len(f)))      # AVIIF_KEYFRAME
        movi.append(ck)
        pos += len(ck)
    body = b"AVI " + hdrl + _riff_list(b"movi", b"".join(movi)) + _riff(b"idx1", b"".join(idx))
    if len(body) + 8 >= 1 << 32:
        raise ValueError("write_avi_mjpeg: AVI 1.0 holds less than 4 GiB")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return path


# ---------------------------------------------------------------------------------------------- animated GIF
def gif_palette(hist):
    """hist: 32768 pixel counts over the bins (r>>3)<<10 | (g>>3)<<5 | (b>>3) (numpy or tensor, int32 bit patterns are read as
    uint32) -> palette uint8 [n <= 256, 3]. A deterministic box-splitting quantiser on the occupied cells of the 32^3 grid with
    count-weighted statistics (cell centres 8 v + 4): the box with the largest weighted sum of squared distances to its mean is
    split by the axis-aligned cut that leaves the least such sum in the two halves (Wu's criterion, evaluated from 32-bin
    marginal sums of the box; ties go to the lowest axis, then the lowest cut), until there are 256 boxes or every box is one
    cell. An entry is the rounded weighted mean of its box; two boxes lie on different sides of a cut, so their entries differ
    by at least 8 in that channel. A clip with at most 256 occupied cells gets exactly their centres. Pure numpy."""
    h = hist.detach().cpu().numpy() if isinstance(hist, torch.Tensor) else np.asarray(hist)
    if h.dtype == np.int32:
        h = h.view(np.uint32)
    h = h.reshape(-1).astype(np.int64)
    if h.size != ops.GIF_HIST_BINS or (h < 0).any() or not h.any():
        raise ValueError("gif_palette: 32768 non-negative counts expected, at least one of them above 0")
    occ = np.flatnonzero(h)
    w = h[occ].astype(np.float64)
    g = np.stack([occ >> 10, (occ >> 5) & 31, occ & 31], 1)                     # grid coordinates 0..31, int64 [m, 3]
    wg = w[:, None] * g                                                         # exact: counts < 2^32, coordinates < 2^5
    wq = (wg * g).sum(1)

    def stats(ix):
        W, S = w[ix].sum(), wg[ix].sum(0)
        return W, S, (0.0 if ix.size == 1 else max(wq[ix].sum() - float(S @ S) / W, 0.0))

    boxes = [np.arange(occ.size)]
    st = [stats(boxes[0])]
    while len(boxes) < 256:
        b = max(range(len(boxes)), key=lambda i: (st[i][2], -i))                # the largest sum; the earliest box on a tie
        W, S, sse = st[b]
        ix = boxes[b]
        if ix.size < 2 or sse <= 0.0:
            break
        score = np.full((3, 31), -1.0)
        gb, wb, wgb = g[ix], w[ix], wg[ix]
        for a in range(3):
            wl = np.cumsum(np.bincount(gb[:, a], wb, 32))[:31]                  # weight at coordinate <= c, c = 0..30
            sl = np.stack([np.cumsum(np.bincount(gb[:, a], wgb[:, k], 32))[:31] for k in range(3)], 1)
            ok = (wl > 0) & (wl < W)
            wr, sr = W - wl, S[None] - sl
            with np.errstate(divide="ignore", invalid="ignore"):
                sc = (sl * sl).sum(1) / wl + (sr * sr).sum(1) / wr
            score[a, ok] = sc[ok]
        a, c = divmod(int(np.argmax(score)), 31)
        left = gb[:, a] <= c
        boxes[b], st[b] = ix[left], stats(ix[left])
        boxes.append(ix[~left])
        st.append(stats(ix[~left]))
    pal = np.array([np.floor(8.0 * S / W + 4.0 + 0.5) for W, S, _ in st])
    return np.clip(pal, 0, 255).astype(np.uint8)


def gif_delay(fps):
    """Centiseconds per frame: max(2, floor(100 / fps + 0.5)). Players treat delays below 2 as 10, so 2 is the shortest."""
    if not fps > 0:
        raise ValueError(f"fps must be positive, got {fps}")
    return min(max(2, int(math.floor(100.0 / fps + 0.5))), 65535)


def gif_file(width, height, palette, images, fps=8, loops=0):
    """The GIF89a container around `images` (per frame: the sub-blocked LZW data behind the minimum code size byte, closed by
    its 00 block): header, logical screen descriptor, the global colour table padded to 256 entries with zeros, a NETSCAPE2.0
    loop extension (`loops` = 0 repeats forever), per frame a graphic control extension (disposal 1, gif_delay(fps)) and a
    full-frame image descriptor without a local table, the trailer. Pure host code; returns bytes."""
    pal = np.ascontiguousarray(palette, dtype=np.uint8)
    images = [bytes(d) for d in images]
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise ValueError(f"gif_file: a GIF holds at most 65535 x 65535 pixels, got {width} x {height}")
    if pal.ndim != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= 256:
        raise ValueError(f"gif_file: a palette uint8 [1..256, 3] expected, got {pal.shape}")
    if not images or not 0 <= int(loops) <= 65535:
        raise ValueError(f"gif_file: {len(images)} frames, loops {loops}")
    delay = gif_delay(fps)
    out = [b"GIF89a", struct.pack("<HHBBB", width, height, 0xF7, 0, 0), pal.tobytes() + bytes(3 * (256 - pal.shape[0])),
           b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", int(loops)) + b"\x00"]
    for d in images:
        out += [b"\x21\xf9\x04" + struct.pack("<BHB", 0x04, delay, 0) + b"\x00",
                b"\x2c" + struct.pack("<HHHHB", 0, 0, width, height, 0), b"\x08", d]
    out.append(b"\x3b")
    return b"".join(out)


def encode_gif_frames(frames_u8, dither=0, chunk=None):
    """frames_u8: uint8 [t, h, w, 3] on the GPU (what frames_to_uint8 returns) -> (palette uint8 [n <= 256, 3] (numpy), list of
    t image data byte strings for gif_file). `dither` in 0..64 is the amplitude of the ordered (Bayer 8x8) dither in front of the
    nearest-colour search; 0 = none: the smallest file, smooth gradients band. `chunk` = pixels per independently LZW-coded chunk
    (default ops.GIF_CHUNK). One histogram launch and one device-to-host copy of 128 KiB for the palette, then three launches per
    batch of frames and one copy of the packed data."""
    f = _gpu_u8_frames("encode_gif_frames", frames_u8, (3,), "there is no CPU fallback")
    t, h, w, _ = f.shape
    if t < 1 or not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f"encode_gif_frames: frames of {h} x {w} x {t}")
    if not 0 <= int(dither) <= 64:
        raise ValueError(f"dither must be in 0..64, got {dither}")
    hw = h * w
    chunk = ops.GIF_CHUNK if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be at least 1 pixel, got {chunk}")
    hist = torch.empty(ops.GIF_HIST_BINS, dtype=torch.int32, device=f.device)
    ops.gif_histogram(f, hist)
    palette = gif_palette(hist)
    pal_dev = torch.from_numpy(palette).to(f.device)
    cpf = (hw + chunk - 1) // chunk
    stride = ops.gif_chunk_max_bytes(min(chunk, hw))

    def code(frames, idx, scratch, words, n):
        ops.gif_map(frames, pal_dev, idx, n=palette.shape[0], dither=int(dither))
        ops.gif_lzw(idx, scratch, words[0], T=n, hw=hw, chunk=chunk, stride=stride)

    def pack(scratch, words, out, frame_len, n, frame_stride):
        ops.gif_pack(scratch, *words, out, frame_len, T=n, chunks_per_frame=cpf, stride=stride, frame_stride=frame_stride)

    return palette, _encode_batches("encode_gif_frames", f, (hw, torch.uint8), 2, cpf, stride,
                                    ops.gif_frame_max_bytes(hw, chunk), True, code, pack)


def write_gif(path, frames_u8, fps=8, loops=0, dither=0, chunk=None):
    """frames_u8: uint8 [t, h, w, 3] on the GPU -> an animated GIF89a that plays at 100 / gif_delay(fps) frames per second."""
    palette, images = encode_gif_frames(frames_u8, dither=dither, chunk=chunk)
    data = gif_file(frames_u8.shape[2], frames_u8.shape[1], palette, images, fps=fps, loops=loops)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(data)
    return path


def _write_clip(stem, grid, fps, container, quality, dither=0, deflate=None):
    """grid uint8 [t, h, w, c] on the GPU -> <stem>.png (APNG, compressed as `deflate` says), <stem>.avi (Motion-JPEG) or
    <stem>.gif."""
    if container == "apng":
        return write_apng(stem + ".png", grid, fps=fps, deflate=deflate)
    if container == "avi":
        return write_avi_mjpeg(stem + ".avi", encode_jpeg_frames(grid, quality=quality), grid.shape[2], grid.shape[1], fps)
    if container == "gif":
        return write_gif(stem + ".gif", grid, fps=fps, dither=dither)
    raise ValueError(f"container must be 'apng', 'avi' or 'gif', got {container!r}")


# ---------------------------------------------------------------------------------------------- reference-named entry points
def save_results(prompt, samples, filename, fakedir, fps=8, loop=False, container="apng", quality=90, dither=0, deflate=None):
    """inference.py:115-137: the batch as ONE clip, its n samples side by side. samples [n, c, t, h, w]. `container`: "apng"
    (default, lossless; `deflate` = "zlib", "hip" or None for png_deflate_mode()), "avi" (Motion-JPEG at JPEG `quality`) or "gif"
    (256 colours, ordered dither of amplitude `dither`)."""
    video = samples[:, :, :-1] if loop else samples            # loop mode drops the duplicated last frame
    grid = frames_to_uint8(video)
    return _write_clip(os.path.join(fakedir, filename.split(".")[0]), grid, fps, container, quality, dither, deflate)


def save_results_seperate(prompt, samples, filename, fakedir, fps=10, loop=False, container="apng", quality=90, dither=0,
                          deflate=None):
    """inference.py:140-162: one clip file per sample, under `samples_separate` (name kept as the reference spells it)."""
    video = samples[:, :, :-1] if loop else samples
    out = []
    d = fakedir.replace("samples", "samples_separate")
    for i in range(video.shape[0]):
        grid = frames_to_uint8(video[i:i + 1])
        out.append(_write_clip(os.path.join(d, f"{filename.split('.')[0]}_sample{i}"), grid, fps, container, quality, dither,
                               deflate))
    return out


def tensor_to_frames(video, savedir, stem="frame", fmt="png", quality=90, deflate=None):
    """One still per frame of a [n, c, t, h, w] batch laid out side by side (the still-image twin of tensor_to_mp4,
    utils/save_video.py:27-43): PNG (default; `deflate` as in write_png, "hip" keeps the frames on the device and encodes them
    in one batch) or, with fmt="jpg", baseline JPEG at `quality`."""
    grid = frames_to_uint8(video)
    if fmt == "png" and png_deflate_mode(deflate) == "hip":
        os.makedirs(os.path.abspath(savedir), exist_ok=True)
        out = []
        for i, stream in enumerate(encode_png_frames(grid)):
            out.append(os.path.join(savedir, f"{stem}_{i:04d}.png"))
            with open(out[-1], "wb") as fh:
                fh.write(_png_file(grid.shape[2], grid.shape[1], grid.shape[3], stream))
        return out
    if fmt == "png":
        grid = grid.cpu().numpy()
        return [write_png(os.path.join(savedir, f"{stem}_{i:04d}.png"), grid[i], deflate="zlib") for i in range(grid.shape[0])]
    if fmt != "jpg":
        raise ValueError(f"fmt must be 'png' or 'jpg', got {fmt!r}")
    os.makedirs(os.path.abspath(savedir), exist_ok=True)
    out = []
    for i, data in enumerate(encode_jpeg_frames(grid, quality=quality)):
        out.append(os.path.join(savedir, f"{stem}_{i:04d}.jpg"))
        with open(out[-1], "wb") as fh:
            fh.write(data)
    return out

"""Input side of the harness: clip files -> frames on the device. The reading counterpart of save_video.py.

The reference reads clips through decord (`VideoReader.get_batch`, scripts/evaluation/funcs.py:154-169 and :188-190); no video
decoder can be installed beside this package, so it reads the one video format it also writes: Motion-JPEG in an AVI container
(what `container="avi"` produces, and what ffmpeg's `-c:v mjpeg` and most cameras write). The host walks the RIFF structure and
the JFIF headers and cuts every scan into its restart segments; the frames are decoded by three HIP launches per batch
(csrc/jpeg_decode.hip: Huffman decoding with one lane per segment, dequantisation + inverse DCT, chroma upsampling + colour
conversion) from one host-to-device copy of the scans and tables. There is no CPU fallback.

Decoded: baseline sequential DCT (SOF0), 8-bit, one interleaved scan, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0, tables from the
file (Annex K's when a frame carries no DHT), with or without restart intervals. A scan without restart markers is one
segment, decoded by one lane: correct, but serial. Everything else raises ValueError naming the cause.

torch and the kernels are imported when a frame is decoded, not with this module: `parse_jpeg` and `read_avi_mjpeg` are plain
host code.
"""
import math
import os
import struct

import numpy as np

_SCRATCH_BYTES = 256 << 20               # coefficients + sample planes per batch of frames
_SOF_NAMES = {0xC1: "extended sequential DCT (SOF1)", 0xC2: "progressive DCT (SOF2)", 0xC3: "lossless (SOF3)",
              0xC5: "differential sequential (SOF5)", 0xC6: "differential progressive (SOF6)", 0xC7: "differential lossless (SOF7)",
              0xC9: "arithmetic-coded sequential (SOF9)", 0xCA: "arithmetic-coded progressive (SOF10)",
              0xCB: "arithmetic-coded lossless (SOF11)", 0xCD: "arithmetic-coded differential (SOF13)",
              0xCE: "arithmetic-coded differential progressive (SOF14)", 0xCF: "arithmetic-coded differential lossless (SOF15)"}


class JpegInfo:
    """What `parse_jpeg` finds in front of the scan. qtabs: {id: bytes[64] in zigzag order}; huff: {(class, id): (BITS bytes[16],
    HUFFVAL bytes)}, class 0 = DC, 1 = AC; comps: per component (Tq, Td, Ta); hs x vs: the luma sampling (chroma is 1x1);
    ri: MCUs per restart interval, 0 = none; scan: (start, end) byte positions of the entropy-coded data in the file."""
    __slots__ = ("width", "height", "ncomp", "hs", "vs", "qtabs", "huff", "comps", "ri", "scan")

    def geometry(self):
        return self.width, self.height, self.ncomp, self.hs, self.vs

    @property
    def mcus(self):
        return math.ceil(self.height / (8 * self.vs)) * math.ceil(self.width / (8 * self.hs))


def _check_huff(key, bits, vals):
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code > 1 << length:
            raise ValueError(f"parse_jpeg: Huffman table {key[0]}/{key[1]} has more codes of length {length} than fit")
        code <<= 1
    if len(vals) != sum(bits) or len(vals) > 256:
        raise ValueError(f"parse_jpeg: Huffman table {key[0]}/{key[1]} is cut short")


def parse_jpeg(data):
    """The marker walk of one JFIF / JPEG file up to its scan -> JpegInfo. A DQT or DHT segment may hold several tables; a file
    without DHT (the usual AVI MJPEG frame) gets the Annex K tables of save_video.JPEG_DHT. Raises ValueError naming the cause
    for what the decoder does not take: frame types other than SOF0, 12-bit samples, 16-bit quantisation tables, four
    components, sampling other than luma 1x1 / 2x1 / 2x2 over chroma 1x1, a scan that is not the only one or not interleaved,
    a truncated header."""
    d = bytes(data)
    if d[:2] != b"\xff\xd8":
        raise ValueError("parse_jpeg: not a JPEG file (no SOI)")
    info = JpegInfo()
    info.qtabs, info.huff, info.ri = {}, {}, 0
    frame = None
    i = 2
    while True:
        if i + 4 > len(d):
            raise ValueError("parse_jpeg: truncated header (the file ends in front of SOS)")
        if d[i] != 0xFF:
            raise ValueError(f"parse_jpeg: no marker at byte {i}")
        m = d[i + 1]
        if m == 0xFF:                                            # fill byte
            i += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:                       # stand-alone markers
            i += 2
            continue
        if m == 0xD9:
            raise ValueError("parse_jpeg: truncated header (EOI in front of SOS)")
        n = struct.unpack(">H", d[i + 2:i + 4])[0]
        body = d[i + 4:i + 2 + n]
        if n < 2 or len(body) != n - 2:
            raise ValueError(f"parse_jpeg: truncated header (marker FF{m:02X} at byte {i} runs past the end)")
        i += 2 + n
        if m == 0xDB:
            j = 0
            while j < len(body):
                pq, tq = body[j] >> 4, body[j] & 15
                if pq:
                    raise ValueError("parse_jpeg: 16-bit quantisation tables are not baseline")
                if tq > 3 or j + 65 > len(body):
                    raise ValueError("parse_jpeg: bad DQT segment")
                info.qtabs[tq] = body[j + 1:j + 65]
                j += 65
        elif m == 0xC4:
            j = 0
            while j < len(body):
                tc, th = body[j] >> 4, body[j] & 15
                if tc > 1 or th > 1 or j + 17 > len(body):
                    raise ValueError("parse_jpeg: bad DHT segment (baseline has tables 0 and 1 of class DC and AC)")
                bits = body[j + 1:j + 17]
                vals = body[j + 17:j + 17 + sum(bits)]
                _check_huff((tc, th), bits, vals)
                info.huff[(tc, th)] = (bits, vals)
                j += 17 + len(vals)
        elif m == 0xDD:
            if len(body) != 2:
                raise ValueError("parse_jpeg: bad DRI segment")
            info.ri = struct.unpack(">H", body)[0]
        elif m == 0xC0:
            if frame is not None:
                raise ValueError("parse_jpeg: two frame headers")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise ValueError("parse_jpeg: truncated header (bad SOF0 segment)")
            prec, info.height, info.width, nc = struct.unpack(">BHHB", body[:6])
            if prec != 8:
                raise ValueError(f"parse_jpeg: {prec}-bit samples (only 8-bit precision is decoded)")
            if nc not in (1, 3):
                raise ValueError(f"parse_jpeg: {nc} components (1 = grey and 3 = YCbCr are decoded; CMYK is not)")
            if info.height < 1 or info.width < 1:
                raise ValueError(f"parse_jpeg: a frame of {info.width} x {info.height}")
            frame = [(body[6 + 3 * k], body[7 + 3 * k] >> 4, body[7 + 3 * k] & 15, body[8 + 3 * k]) for k in range(nc)]
            samp = [(h, v) for _, h, v, _ in frame]
            if nc == 1:
                samp = [(1, 1)]                                  # a one-component scan is not interleaved: its MCU is one block
            if samp[0] not in ((1, 1), (2, 1), (2, 2)) or any(s != (1, 1) for s in samp[1:]):
                raise ValueError(f"parse_jpeg: sampling {samp} (luma 1x1, 2x1 or 2x2 over chroma 1x1 is decoded)")
            if any(tq > 3 for *_, tq in frame):
                raise ValueError("parse_jpeg: bad SOF0 segment (quantisation table above 3)")
            info.ncomp, (info.hs, info.vs) = nc, samp[0]
        elif m in _SOF_NAMES:
            raise ValueError(f"parse_jpeg: {_SOF_NAMES[m]} is not decoded (only baseline, SOF0)")
        elif m == 0xDA:
            if frame is None:
                raise ValueError("parse_jpeg: SOS in front of the frame header")
            ns = body[0] if body else 0
            if len(body) != 4 + 2 * ns:
                raise ValueError("parse_jpeg: truncated header (bad SOS segment)")
            if ns != len(frame):
                raise ValueError(f"parse_jpeg: a scan of {ns} of the {len(frame)} components (more than one scan)")
            info.comps = []
            for k, (cid, _, _, tq) in enumerate(frame):
                cs, t = body[1 + 2 * k], body[2 + 2 * k]
                if cs != cid or (t >> 4) > 1 or (t & 15) > 1:
                    raise ValueError("parse_jpeg: bad SOS segment (component order or table selector)")
                info.comps.append((tq, t >> 4, t & 15))
            if tuple(body[1 + 2 * ns:]) != (0, 63, 0):
                raise ValueError("parse_jpeg: the scan is not a baseline scan (Ss, Se, Ah/Al must be 0, 63, 0)")
            break
    if not info.huff:
        from .save_video import JPEG_DHT
        for t in JPEG_DHT:
            info.huff[(t[0] >> 4, t[0] & 15)] = (t[1:17], t[17:])
    for tq, td, ta in info.comps:
        if tq not in info.qtabs:
            raise ValueError(f"parse_jpeg: quantisation table {tq} is not in the file")
        if (0, td) not in info.huff or (1, ta) not in info.huff:
            raise ValueError(f"parse_jpeg: Huffman table DC {td} / AC {ta} is not in the file")
    # the end of the scan: the first FF that is followed by neither 00 (stuffing), RSTn nor another FF (fill)
    a = np.frombuffer(d, np.uint8, offset=i)
    ff = np.flatnonzero(a[:-1] == 0xFF) if a.size > 1 else np.zeros(0, np.int64)
    nxt = a[ff + 1]
    ends = ff[(nxt != 0) & (nxt != 0xFF) & ((nxt < 0xD0) | (nxt > 0xD7))]
    end = i + int(ends[0]) if ends.size else len(d)             # AVI frames without EOI exist: the scan then runs to the end
    if ends.size and a[ends[0] + 1] != 0xD9:
        raise ValueError(f"parse_jpeg: marker FF{a[ends[0] + 1]:02X} behind the scan (more than one scan, or tables between scans)")
    info.scan = (i, end)
    return info


def scan_segments(data, info):
    """The independently coded segments of the scan: int64 [n, 2] (start, length) in file positions - one per restart interval,
    or the whole scan without DRI. RSTn are found with numpy: in entropy-coded data FF is followed only by 00 or a marker, so
    there are no false hits. Raises ValueError unless the markers count up modulo 8 and there are ceil(MCUs / ri) segments."""
    lo, hi = info.scan
    a = np.frombuffer(data, np.uint8, count=hi - lo, offset=lo)
    ff = np.flatnonzero(a[:-1] == 0xFF) if a.size > 1 else np.zeros(0, np.int64)
    rst = ff[(a[ff + 1] >= 0xD0) & (a[ff + 1] <= 0xD7)]
    want = math.ceil(info.mcus / info.ri) if info.ri else 1
    if rst.size + 1 != want:
        raise ValueError(f"scan_segments: {rst.size + 1} restart segments, {want} expected ({info.mcus} MCUs, interval {info.ri})")
    if not np.array_equal(a[rst + 1] - 0xD0, np.arange(rst.size) % 8):
        raise ValueError("scan_segments: the restart markers do not count up modulo 8")
    starts = np.concatenate([[0], rst + 2])
    ends = np.concatenate([rst, [a.size]])
    return np.stack([starts + lo, ends - starts], 1).astype(np.int64)


# ---------------------------------------------------------------------------------------------- AVI
def _chunks(d, lo, hi):
    """(fourcc, body start, body size) of the chunks in d[lo:hi]; a chunk that runs past `hi` ends the walk (truncated file)."""
    i = lo
    while i + 8 <= hi:
        cc, n = d[i:i + 4], struct.unpack("<I", d[i + 4:i + 8])[0]
        if i + 8 + n > hi:
            n = hi - i - 8
        yield cc, i + 8, n
        i += 8 + n + (n & 1)                                     # odd sizes are padded


def read_avi_mjpeg(path):
    """An AVI file with a Motion-JPEG video stream -> (width, height, fps, [JPEG file of every frame as bytes]). The first
    `vids` stream whose handler (strh) or biCompression (strf) is MJPG, in either letter case, is taken; its `NNdc` / `NNdb`
    chunks of `movi` are the frames, in file order, those inside `rec ` lists included; a zero-length chunk repeats the previous
    frame; JUNK and idx1 are ignored. fps = rate / scale of the stream header. Another codec raises ValueError naming its fourcc.
    Only the first RIFF 'AVI ' of the file is read: the OpenDML extensions (AVIX chunks of files above 1 GiB, the super index)
    are not. Pure host code."""
    with open(path, "rb") as fh:
        d = fh.read()
    if len(d) < 12 or d[:4] != b"RIFF" or d[8:12] != b"AVI ":
        raise ValueError(f"read_avi_mjpeg: {path} is not an AVI file")
    top = min(len(d), 8 + struct.unpack("<I", d[4:8])[0])
    streams, movi = [], None
    for cc, at, n in _chunks(d, 12, top):
        if cc != b"LIST":
            continue
        kind = d[at:at + 4]
        if kind == b"hdrl":
            for c2, a2, n2 in _chunks(d, at + 4, at + n):
                if c2 == b"LIST" and d[a2:a2 + 4] == b"strl":
                    strh = strf = b""
                    for c3, a3, n3 in _chunks(d, a2 + 4, a2 + n2):
                        if c3 == b"strh":
                            strh = d[a3:a3 + n3]
                        elif c3 == b"strf":
                            strf = d[a3:a3 + n3]
                    streams.append((strh, strf))
        elif kind == b"movi" and movi is None:
            movi = (at + 4, at + n)
    video = [(k, h, f) for k, (h, f) in enumerate(streams) if h[:4] == b"vids"]
    pick = None
    for k, h, f in video:
        if h[4:8].upper() == b"MJPG" or f[16:20].upper() == b"MJPG":
            pick = (k, h, f)
            break
    if pick is None:
        if not video:
            raise ValueError(f"read_avi_mjpeg: {path} has no video stream")
        cc = video[0][2][16:20] or video[0][1][4:8]
        raise ValueError(f"read_avi_mjpeg: {path}: codec {cc.decode('latin-1')!r} is not Motion-JPEG (only MJPG is read)")
    k, strh, strf = pick
    if len(strh) < 28 or len(strf) < 12 or movi is None:
        raise ValueError(f"read_avi_mjpeg: {path}: truncated stream header or no movi list")
    scale, rate = struct.unpack("<II", strh[20:28])
    width, height = struct.unpack("<ii", strf[4:12])
    tags = (b"%02ddc" % k, b"%02ddb" % k)
    frames = []

    def walk(lo, hi):
        for cc, at, n in _chunks(d, lo, hi):
            if cc == b"LIST":
                if d[at:at + 4] == b"rec ":
                    walk(at + 4, at + n)
            elif cc in tags:
                if n:
                    frames.append(d[at:at + n])
                elif frames:
                    frames.append(frames[-1])                    # a dropped frame: the previous one is shown again

    walk(*movi)
    if not frames:
        raise ValueError(f"read_avi_mjpeg: {path} holds no frame of stream {k}")
    return width, abs(height), (rate / scale if scale else 0.0), frames


# ---------------------------------------------------------------------------------------------- decoding
def _frame_table(info):
    """The DC_JPEG_FRAME_TAB_BYTES block of one frame (include/dcrafter_hip.h)."""
    from ..ops import JPEG_FRAME_TAB_BYTES
    tab = np.zeros(JPEG_FRAME_TAB_BYTES, np.uint8)
    for (tc, th), (bits, vals) in info.huff.items():
        at = (tc * 2 + th) * 272
        tab[at:at + 16] = np.frombuffer(bits, np.uint8)
        tab[at + 16:at + 16 + len(vals)] = np.frombuffer(vals, np.uint8)
    for tq, q in info.qtabs.items():
        tab[1088 + 64 * tq:1088 + 64 * tq + 64] = np.frombuffer(q, np.uint8)
    for c, (tq, td, ta) in enumerate(info.comps):
        tab[1344 + c] = td | (ta << 4)
        tab[1347 + c] = tq
    return tab


def pack_jpeg_batch(files, infos=None):
    """Everything the device needs of a batch of JPEG files of one geometry, in ONE host buffer (so it is one copy):
    (buffer uint8, layout) with layout = {"seg": (byte offset, n_seg), "frame_seg": offset, "ftab": offset, "scan": (offset,
    bytes), "max_spf": most segments in a frame}. Descriptor rows: scan offset, length, first MCU, MCUs, frame. The scan of
    every frame is copied whole, so the RSTn markers stay between its segments, outside every descriptor's range."""
    from ..ops import JPEG_FRAME_TAB_BYTES
    infos = infos or [parse_jpeg(f) for f in files]
    segs, frame_seg, scans, pos = [], [0], [], 0
    for t, (f, info) in enumerate(zip(files, infos)):
        sg = scan_segments(f, info)
        lo, hi = info.scan
        ri = info.ri or info.mcus
        d = np.empty((len(sg), 5), np.int64)
        d[:, 0] = pos + sg[:, 0] - lo                            # the frame's scan is copied whole: its RSTn lie between segments
        d[:, 1] = sg[:, 1]
        d[:, 2] = np.arange(len(sg)) * ri
        d[:, 3] = np.minimum(ri, info.mcus - d[:, 2])
        d[:, 4] = t
        segs.append(d)
        scans.append(f[lo:hi])
        pos += hi - lo
        frame_seg.append(frame_seg[-1] + len(sg))
    if pos >= 1 << 31:
        raise ValueError("pack_jpeg_batch: the scans of a batch must stay below 2 GiB")
    segs = np.concatenate(segs)
    T, n_seg = len(files), len(segs)
    o_fs = 20 * n_seg
    o_tab = o_fs + 4 * (T + 1)
    o_scan = o_tab + T * JPEG_FRAME_TAB_BYTES
    buf = np.zeros(o_scan + max(pos, 1), np.uint8)
    buf[:o_fs].view(np.int32)[:] = segs.astype(np.int32).reshape(-1)
    buf[o_fs:o_tab].view(np.int32)[:] = np.asarray(frame_seg, np.int32)
    for t, info in enumerate(infos):
        buf[o_tab + t * JPEG_FRAME_TAB_BYTES:o_tab + (t + 1) * JPEG_FRAME_TAB_BYTES] = _frame_table(info)
    buf[o_scan:o_scan + pos] = np.frombuffer(b"".join(scans), np.uint8)
    return buf, {"seg": (0, n_seg), "frame_seg": o_fs, "ftab": o_tab, "scan": (o_scan, max(pos, 1)),
                 "max_spf": int(np.diff(frame_seg).max())}


def launch_jpeg_decode(dev_buf, layout, coef, planes, status, out, *, T, H, W, ncomp, hs, vs):
    """The three launches of a packed batch that lies on the device (no allocation, no synchronisation: capturable)."""
    from .. import ops
    import torch
    my, mx, _, _ = ops.jpeg_decode_geometry(H, W, ncomp, hs, vs)
    (o_seg, n_seg), o_fs, o_tab, (o_scan, n_scan) = layout["seg"], layout["frame_seg"], layout["ftab"], layout["scan"]
    seg = dev_buf[o_seg:o_seg + 20 * n_seg].view(torch.int32)
    frame_seg = dev_buf[o_fs:o_fs + 4 * (T + 1)].view(torch.int32)
    ftab = dev_buf[o_tab:o_tab + T * ops.JPEG_FRAME_TAB_BYTES]
    ops.jpeg_decode_entropy(dev_buf[o_scan:o_scan + n_scan], seg, frame_seg, ftab, coef, status, T=T, my=my, mx=mx, ncomp=ncomp,
                            hs=hs, vs=vs, max_segs_per_frame=layout["max_spf"])
    ops.jpeg_decode_idct(coef, ftab, planes, T=T, my=my, mx=mx, ncomp=ncomp, hs=hs, vs=vs)
    ops.jpeg_decode_output(planes, out, T=T, H=H, W=W, ncomp=ncomp, hs=hs, vs=vs)


def decode_jpeg_frames(files, device=None, planar=False):
    """files: JPEG files (bytes) of one geometry -> uint8 [t, h, w, 3] on the device (what frames_to_uint8 produces and
    encode_jpeg_frames takes), or with planar=True fp32 [t, 3, h, w] holding the same values 0..255 (3 t planes for
    ops.resize_f32). Per batch of frames - sized against a scratch budget, as encode_jpeg_frames sizes its batches - one
    host-to-device copy of the scans and tables, three launches, and one read of the segments' status words; a segment that did
    not decode raises ValueError naming the frame and the segment."""
    import torch
    from .. import ops
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("decode_jpeg_frames runs on the HIP path only (there is no CPU fallback)")
    files = [bytes(f) for f in files]
    if not files:
        raise ValueError("decode_jpeg_frames: no frames")
    infos = [parse_jpeg(f) for f in files]
    geo = infos[0].geometry()
    for i, info in enumerate(infos):
        if info.geometry() != geo:
            raise ValueError(f"decode_jpeg_frames: frame {i} is {info.geometry()}, frame 0 is {geo} (width, height, components, "
                             "luma sampling): one geometry per call")
    W, H, ncomp, hs, vs = geo
    my, mx, bpm, per_frame = ops.jpeg_decode_geometry(H, W, ncomp, hs, vs)
    t = len(files)
    tb = max(1, min(t, 65535, _SCRATCH_BYTES // (3 * per_frame)))          # int16 coefficients + uint8 planes
    with torch.cuda.device(device):
        out = torch.empty((t, 3, H, W) if planar else (t, H, W, 3), dtype=torch.float32 if planar else torch.uint8, device=device)
        coef = torch.empty(tb * per_frame, dtype=torch.int16, device=device)
        planes = torch.empty(tb * per_frame, dtype=torch.uint8, device=device)
        for t0 in range(0, t, tb):
            n = min(tb, t - t0)
            buf, layout = pack_jpeg_batch(files[t0:t0 + n], infos[t0:t0 + n])
            dev_buf = torch.from_numpy(buf).to(device)
            n_seg = layout["seg"][1]
            status = torch.full((n_seg,), -1, dtype=torch.int32, device=device)
            launch_jpeg_decode(dev_buf, layout, coef, planes, status, out[t0:t0 + n], T=n, H=H, W=W, ncomp=ncomp, hs=hs, vs=vs)
            st = status.cpu().numpy()
            bad = np.flatnonzero(st)
            if bad.size:
                fs = buf[layout["frame_seg"]:layout["frame_seg"] + 4 * (n + 1)].view(np.int32)
                f = int(np.searchsorted(fs, bad[0], side="right") - 1)
                why = ops.JPEG_SEG_STATUS.get(int(st[bad[0]]), f"status {int(st[bad[0]])}")
                raise ValueError(f"decode_jpeg_frames: frame {t0 + f} segment {int(bad[0] - fs[f])}: {why} "
                                 f"({bad.size} of the batch's {n_seg} segments did not decode)")
    return out


def read_video(path, device=None):
    """`.avi` (Motion-JPEG) -> (uint8 [t, h, w, 3] on the device, fps); `.jpg` / `.jpeg` -> one frame and fps 0."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".avi":
        _, _, fps, frames = read_avi_mjpeg(path)
        return decode_jpeg_frames(frames, device=device), fps
    if ext in (".jpg", ".jpeg"):
        with open(path, "rb") as fh:
            return decode_jpeg_frames([fh.read()], device=device), 0.0
    raise ValueError(f"read_video: {path}: only .avi (Motion-JPEG), .jpg and .jpeg are read")

"""Plain-numpy restatement of a baseline JPEG decoder (ITU-T T.81 sequential DCT, SOF0, 8-bit, one interleaved scan; grey or
YCbCr with luma sampling 1x1, 2x1 or 2x2 over chroma 1x1), shared by tests/test_mjpeg_decode_cpu.py and
tests/test_mjpeg_decode_gpu.py. Written from the standard, independent of the package's parser and kernels; it borrows only
the Annex K tables and the zigzag order of tests/jpeg_restatement.py. Three parts:

  parse()          the marker walk: size, sampling, tables, restart interval, the entropy-coded bytes
  coefficients()   Huffman decoding (T.81 F.2.2) -> quantised coefficients int16 [my, mx, blocks per MCU, 64] in zigzag
                   order: for 4:2:0 the layout of jpeg_restatement.coefficients (Y00 Y01 Y10 Y11 Cb Cr)
  pixels()         dequantisation, orthonormal inverse DCT, + 128, floor(v + 0.5), clamp to 0..255 (before upsampling);
                   chroma upsampled by the triangle filter (per doubled axis 3/4 of the nearer, 1/4 of the farther sample, edges
                   replicate, only the ceil(h / vs) x ceil(w / hs) real samples are used); R = Y + 1.402 (Cr - 128),
                   G = Y - 0.344136286 (Cb - 128) - 0.714136286 (Cr - 128), B = Y + 1.772 (Cb - 128); floor(v + 0.5), clamp.
                   The arithmetic runs in `dtype` (float64 is the reference; float32 shows what the number format costs)
"""
import numpy as np

from tests import jpeg_restatement as J


class Bad(ValueError):
    pass


def parse(data):
    """-> dict(width, height, comps=[(id, h, v, tq, td, ta)], hs, vs, q={id: int64[64] zigzag}, huff={(class, id): (bits, vals)},
    ri, segments=[bytes of each restart segment])"""
    d = bytes(data)
    if d[:2] != b"\xff\xd8":
        raise Bad("no SOI")
    out = {"q": {}, "huff": {}, "ri": 0}
    frame, i = None, 2
    while True:
        if i + 4 > len(d):
            raise Bad("header cut short")
        if d[i] != 0xFF:
            raise Bad(f"no marker at {i}")
        m, n = d[i + 1], int.from_bytes(d[i + 2:i + 4], "big")
        if i + 2 + n > len(d):
            raise Bad("header cut short")
        body = d[i + 4:i + 2 + n]
        i += 2 + n
        if m == 0xDB:
            while body:
                if body[0] >> 4:
                    raise Bad("16-bit quantisation table")
                out["q"][body[0] & 15] = np.array(list(body[1:65]), dtype=np.int64)
                body = body[65:]
        elif m == 0xC4:
            while body:
                bits = body[1:17]
                out["huff"][(body[0] >> 4, body[0] & 15)] = (bits, body[17:17 + sum(bits)])
                body = body[17 + sum(bits):]
        elif m == 0xDD:
            out["ri"] = int.from_bytes(body, "big")
        elif m == 0xC0:
            if body[0] != 8:
                raise Bad("precision")
            out["height"], out["width"] = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            if body[5] not in (1, 3):
                raise Bad(f"{body[5]} components")
            frame = [(body[6 + 3 * k], body[7 + 3 * k] >> 4, body[7 + 3 * k] & 15, body[8 + 3 * k]) for k in range(body[5])]
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise Bad(f"frame type FF{m:02X} is not baseline")
        elif m == 0xDA:
            if frame is None or body[0] != len(frame):
                raise Bad("scan does not hold every component")
            out["comps"] = [(cid, h, v, tq, body[2 + 2 * k] >> 4, body[2 + 2 * k] & 15) for k, (cid, h, v, tq) in enumerate(frame)]
            break
    if not out["huff"]:                                          # the usual AVI MJPEG frame: Annex K tables are implied
        out["huff"] = {(key >> 4, key & 15): bv for key, bv in J.HUFF.items()}
    samp = [(h, v) for _, h, v, *_ in out["comps"]]
    if len(samp) == 1:
        samp = [(1, 1)]                                          # a one-component scan is not interleaved
    if samp[0] not in ((1, 1), (2, 1), (2, 2)) or any(s != (1, 1) for s in samp[1:]):
        raise Bad(f"sampling {samp}")
    out["hs"], out["vs"] = samp[0]
    # the scan: up to the first marker that is neither stuffing nor RSTn; cut at the RSTn, which must count up modulo 8
    segs, cur, expect = [], bytearray(), 0
    while i < len(d):
        if d[i] == 0xFF and i + 1 < len(d) and d[i + 1] != 0:
            m = d[i + 1]
            if 0xD0 <= m <= 0xD7:
                if m - 0xD0 != expect:
                    raise Bad("restart markers out of order")
                expect = (expect + 1) % 8
                segs.append(bytes(cur))
                cur = bytearray()
                i += 2
                continue
            if m != 0xD9:
                raise Bad(f"marker FF{m:02X} behind the scan")
            break
        cur.append(d[i])
        i += 1
    segs.append(bytes(cur))
    out["segments"] = segs
    return out


def grid(p):
    return -(-p["height"] // (8 * p["vs"])), -(-p["width"] // (8 * p["hs"]))


def _decode_table(bits, vals):
    """{(length, code): symbol}, the canonical codes of T.81 Annex C"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


class _Reader:
    """The bits of one segment: FF 00 -> FF; beyond the end the bits read as 1s (`over` counts how many were taken there)."""

    def __init__(self, seg):
        raw = np.frombuffer(seg.replace(b"\xff\x00", b"\xff"), np.uint8)
        self.bits = np.unpackbits(raw).tolist()
        self.pos = 0

    def bit(self):
        b = self.bits[self.pos] if self.pos < len(self.bits) else 1
        self.pos += 1
        return b

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (length, code) in table:
                return table[(length, code)]
        raise Bad("a code that is in no table")

    def value(self, s):
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bit()
        return v if s == 0 or v >= 1 << (s - 1) else v - (1 << s) + 1          # F.2.2.1 EXTEND


def coefficients(data):
    """One file -> int16 [my, mx, blocks per MCU, 64], zigzag order."""
    p = parse(data)
    my, mx = grid(p)
    ny = p["hs"] * p["vs"]
    bpm = ny + len(p["comps"]) - 1
    nmcu = my * mx
    ri = p["ri"] or nmcu
    if len(p["segments"]) != -(-nmcu // ri):
        raise Bad(f"{len(p['segments'])} segments for {nmcu} MCUs at interval {ri}")
    tabs = {key: _decode_table(*bv) for key, bv in p["huff"].items()}
    out = np.zeros((nmcu, bpm, 64), dtype=np.int16)
    for s, seg in enumerate(p["segments"]):
        r = _Reader(seg)
        pred = [0, 0, 0]
        for m in range(s * ri, min(nmcu, (s + 1) * ri)):
            for b in range(bpm):
                c = 0 if b < ny else b - ny + 1
                _, _, _, _, td, ta = p["comps"][c]
                size = r.symbol(tabs[(0, td)])
                if size > 11:
                    raise Bad("DC category above 11")
                pred[c] += r.value(size)
                out[m, b, 0] = pred[c]
                k = 1
                while k < 64:
                    sym = r.symbol(tabs[(1, ta)])
                    run, size = sym >> 4, sym & 15
                    if size == 0:
                        if run == 15:
                            k += 16
                            continue
                        if run == 0:
                            break
                        raise Bad("EOBn in a baseline scan")
                    if size > 10:
                        raise Bad("AC category above 10")
                    k += run
                    if k > 63:
                        raise Bad("a run past coefficient 63")
                    out[m, b, k] = r.value(size)
                    k += 1
        if r.pos > len(r.bits):
            raise Bad(f"segment {s}: bytes missing")
        if len(r.bits) - r.pos >= 8:
            raise Bad(f"segment {s}: bytes left over")
    return out.reshape(my, mx, bpm, 64)


def _round_clamp(v):
    return np.clip(np.floor(v + v.dtype.type(0.5)), 0, 255)


def _upsample(c, axis, n_out):
    """Triangle filter along `axis` from c.shape[axis] real samples to n_out = 2 n or 2 n - 1 outputs."""
    n = c.shape[axis]
    o = np.arange(n_out)
    near = o // 2
    far = np.clip(near + np.where(o % 2 == 1, 1, -1), 0, n - 1)
    k = c.dtype.type
    return k(0.75) * np.take(c, near, axis) + k(0.25) * np.take(c, far, axis)


def pixels(data, dtype=np.float64, coef=None):
    """One file -> uint8 [h, w, 3]. `coef` replaces the file's own coefficients (same layout) when given."""
    p = parse(data)
    coef = coefficients(data) if coef is None else np.asarray(coef)
    my, mx = grid(p)
    hs, vs, h, w = p["hs"], p["vs"], p["height"], p["width"]
    ny = hs * vs
    D = J.dct_matrix(dtype)

    def plane(blocks, tq):                 # [a, b, 64] zigzag -> samples [8 a, 8 b], rounded and clamped
        a, b = blocks.shape[:2]
        F = np.zeros((a, b, 64), dtype=dtype)
        F[..., J.ZZ] = blocks.astype(dtype) * p["q"][tq].astype(dtype)
        s = np.einsum("vy,abvu,ux->abyx", D, F.reshape(a, b, 8, 8), D).astype(dtype) + dtype(128)
        return _round_clamp(s).transpose(0, 2, 1, 3).reshape(8 * a, 8 * b)

    yb = coef[:, :, :ny].reshape(my, mx, vs, hs, 64).transpose(0, 2, 1, 3, 4).reshape(my * vs, mx * hs, 64)
    Y = plane(yb, p["comps"][0][3])[:h, :w]
    if len(p["comps"]) == 1:
        return np.repeat(Y[..., None], 3, 2).astype(np.uint8)
    ch, cw = -(-h // vs), -(-w // hs)
    cc = []
    for c in (1, 2):
        x = plane(coef[:, :, ny + c - 1], p["comps"][c][3])[:ch, :cw]
        if vs == 2:
            x = _upsample(x, 0, h)
        if hs == 2:
            x = _upsample(x, 1, w)
        cc.append(x - dtype(128))
    k = dtype
    rgb = np.stack([Y + k(1.402) * cc[1], Y - k(0.344136286) * cc[0] - k(0.714136286) * cc[1], Y + k(1.772) * cc[0]], -1)
    return _round_clamp(rgb.astype(dtype)).astype(np.uint8)

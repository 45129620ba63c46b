"""Plain-Python restatement of the baseline JPEG / Motion-JPEG path (ITU-T T.81 sequential DCT, 8-bit, YCbCr 4:2:0,
Annex K tables, restart intervals), shared by tests/test_mjpeg_cpu.py and tests/test_mjpeg_gpu.py. Written from the
standard, independent of the package's kernels and of its header writer. Three parts:

  coefficients()   frames uint8 [T, H, W, 3] -> quantised coefficients int16 [T, my, mx, 6, 64] in zigzag order, the
                   arithmetic in `dtype` (float64 is the reference; float32 shows what the number format itself costs)
  entropy_*()      coefficients -> the Huffman-coded byte string of every restart segment, and the scan with RSTm markers
  jfif()           scan -> a complete JFIF file

An MCU is 16x16 pixels and holds the blocks Y00 Y01 Y10 Y11 Cb Cr; pixels beyond the frame replicate its last row / column.
"""
import numpy as np

MCU_MAX_BYTES = 2496          # 6 blocks x (22 + 63 x 26) bits, every byte stuffed, plus the padded last byte

# Annex K.1 / K.2 quantisation tables, natural (row-major) order
K1_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
           14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
           49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
K2_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
             47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

# Annex K.3 - K.6 Huffman tables as (BITS, HUFFVAL); keys are the DHT class/id bytes
_AC_TAIL = ("535455565758595a636465666768696a737475767778797a")
HUFF = {
    0x00: (bytes.fromhex("00010501010101010100000000000000"), bytes(range(12))),
    0x10: (bytes.fromhex("0002010303020403050504040000017d"), bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738"
        "393a434445464748494a" + _AC_TAIL + "838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4"
        "c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")),
    0x01: (bytes.fromhex("00030101010101010101010000000000"), bytes(range(12))),
    0x11: (bytes.fromhex("00020102040403040705040400010277"), bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637"
        "38393a434445464748494a" + _AC_TAIL + "82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2"
        "c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")),
}


def zigzag():
    """ZZ[k] = natural index (8 * row + col) of the k-th coefficient of the zigzag scan (T.81 figure 5)."""
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return np.array(order, dtype=np.int64)


ZZ = zigzag()


def quant_tables(quality):
    """The two tables [2, 64] in natural order: Annex K scaled the way libjpeg's jpeg_set_quality does."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality must be in 1..100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.array([[min(max((b * s + 50) // 100, 1), 255) for b in base] for base in (K1_LUMA, K2_CHROMA)], dtype=np.int64)


def mcu_grid(H, W):
    return (H + 15) // 16, (W + 15) // 16


# ------------------------------------------------------------------------------------------------ coefficient stage
def dct_matrix(dtype=np.float64):
    """Orthonormal DCT-II: D[u, x] = c(u) / 2 * cos((2 x + 1) u pi / 16), c(0) = 1 / sqrt 2."""
    u = np.arange(8, dtype=np.float64)[:, None]
    x = np.arange(8, dtype=np.float64)[None, :]
    d = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    d[0] /= np.sqrt(2.0)
    return d.astype(dtype)


def coefficients(frames, qtab_natural, dtype=np.float64):
    """frames uint8 [T, H, W, 3]; qtab_natural [2, 64] -> int16 [T, my, mx, 6, 64], zigzag order."""
    f = np.asarray(frames)
    T, H, W, c = f.shape
    assert c == 3 and f.dtype == np.uint8
    my, mx = mcu_grid(H, W)
    yy = np.minimum(np.arange(my * 16), H - 1)
    xx = np.minimum(np.arange(mx * 16), W - 1)
    p = f[:, yy][:, :, xx].astype(dtype)
    k = lambda v: dtype(v)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = k(0.299) * R + k(0.587) * G + k(0.114) * B
    Cb = k(-0.168735892) * R - k(0.331264108) * G + k(0.5) * B + k(128)
    Cr = k(0.5) * R - k(0.418687589) * G - k(0.081312411) * B + k(128)
    sub = lambda a: (a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2]) * k(0.25)
    D = dct_matrix(dtype)
    q = np.asarray(qtab_natural).astype(dtype)

    def blocks(plane, tq):            # plane [T, 8 a, 8 b] -> quantised [T, a, b, 64] zigzag
        a, b = plane.shape[1] // 8, plane.shape[2] // 8
        s = (plane - k(128)).reshape(T, a, 8, b, 8).transpose(0, 1, 3, 2, 4)          # [T, a, b, y, x]
        F = np.einsum("vy,tabyx,ux->tabvu", D, s, D).astype(dtype).reshape(T, a, b, 64)
        x = F[..., ZZ] / q[tq][ZZ]
        r = np.sign(x) * np.floor(np.abs(x) + k(0.5))
        r[..., 1:] = np.clip(r[..., 1:], -1023, 1023)
        return r.astype(np.int16)

    yb = blocks(Y, 0).reshape(T, my, 2, mx, 2, 64).transpose(0, 1, 3, 2, 4, 5).reshape(T, my, mx, 4, 64)
    out = np.empty((T, my, mx, 6, 64), dtype=np.int16)
    out[:, :, :, :4] = yb
    out[:, :, :, 4] = blocks(sub(Cb), 1)
    out[:, :, :, 5] = blocks(sub(Cr), 1)
    return out


# ------------------------------------------------------------------------------------------------ entropy coder
def huff_codes(bits, vals):
    """Canonical codes of T.81 Annex C: {symbol: (code, length)}."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


_CODES = {key: huff_codes(*bv) for key, bv in HUFF.items()}


class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, n):
        self.acc = (self.acc << n) | (value & ((1 << n) - 1))
        self.n += n
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def _amplitude(w, v):
    size = abs(v).bit_length()
    return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)


def _block(w, blk, pred, dc, ac):
    size, amp = _amplitude(w, int(blk[0]) - pred)
    w.put(*dc[size])
    w.put(amp, size)
    run = 0
    for k in range(1, 64):
        v = int(blk[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            w.put(*ac[0xF0])
            run -= 16
        size, amp = _amplitude(w, v)
        w.put(*ac[(run << 4) | size])
        w.put(amp, size)
        run = 0
    if run:
        w.put(*ac[0x00])
    return int(blk[0])


def entropy_segments(coef_frame, ri):
    """coef_frame int16 [my, mx, 6, 64] -> the byte strings of its ceil(my mx / ri) restart segments."""
    m = np.asarray(coef_frame).reshape(-1, 6, 64)
    segs = []
    for s in range(0, m.shape[0], ri):
        w = _Bits()
        pred = [0, 0, 0]
        for mcu in m[s:s + ri]:
            for b in range(6):
                comp = 0 if b < 4 else b - 3
                pred[comp] = _block(w, mcu[b], pred[comp], _CODES[0x00 if comp == 0 else 0x01],
                                    _CODES[0x10 if comp == 0 else 0x11])
        segs.append(w.flush())
    return segs


def join_segments(segs):
    """RSTm between the segments of a frame (m = index mod 8), none after the last."""
    out = bytearray()
    for i, s in enumerate(segs):
        out += s
        if i + 1 < len(segs):
            out += bytes([0xFF, 0xD0 + (i & 7)])
    return bytes(out)


def entropy_scan(coef_frame, ri):
    return join_segments(entropy_segments(coef_frame, ri))


# ------------------------------------------------------------------------------------------------ file assembly
def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def jfif(scan, H, W, qtab_natural, ri):
    q = np.asarray(qtab_natural)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i in range(2):
        out += _seg(0xDB, bytes([i]) + bytes(int(v) for v in q[i][ZZ]))
    out += _seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for key in (0x00, 0x10, 0x01, 0x11):
        out += _seg(0xC4, bytes([key]) + HUFF[key][0] + HUFF[key][1])
    out += _seg(0xDD, ri.to_bytes(2, "big"))
    out += _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out + scan + b"\xff\xd9"


def encode(frames, quality, ri=None, dtype=np.float64):
    """frames uint8 [T, H, W, 3] -> list of JFIF files."""
    f = np.asarray(frames)
    T, H, W, _ = f.shape
    q = quant_tables(quality)
    ri = ri or mcu_grid(H, W)[1]
    coef = coefficients(f, q, dtype)
    return [jfif(entropy_scan(coef[t], ri), H, W, q, ri) for t in range(T)]


# ------------------------------------------------------------------------------------------------ test inputs / measures
def make_frames(kind, T, H, W, rng):
    """The two inputs of the tests: "noise" = 0.6 N(0,1); "smooth" = sines and a checkerboard plus 0.05 N(0,1); both through
    clamp, (v + 1) / 2 * 255 and truncation. Returns uint8 [T, H, W, 3]."""
    if kind == "noise":
        v = 0.6 * rng.standard_normal((T, H, W, 3))
    else:
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        base = np.stack([np.sin(x / 9 + y / 13), np.cos(x / 5) * np.sin(y / 7), ((x // 8 + y // 8) % 2) * 1.6 - 0.8], -1)
        v = base[None] + 0.05 * rng.standard_normal((T, H, W, 3))
    return ((np.clip(v, -1, 1) + 1) / 2 * 255).astype(np.uint8)


def psnr(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    mse = float(np.mean(d * d))
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def markers(data):
    """[(marker, payload)] of a JFIF file up to and including SOS."""
    out, i = [], 2
    assert data[:2] == b"\xff\xd8"
    while True:
        assert data[i] == 0xFF, hex(data[i])
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        out.append((m, bytes(data[i + 4:i + 2 + n])))
        i += 2 + n
        if m == 0xDA:
            return out


def walk_avi(data):
    """Minimal RIFF walker for an AVI file: checks that chunk sizes nest and sum to the file size; returns
    {"chunks": {fourcc path: payload, ...}, "frames": [payload of each 00dc], "movi": offset of the 'movi' fourcc,
    "idx": [(ckid, flags, offset, size)]}."""
    import struct
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    assert struct.unpack("<I", data[4:8])[0] + 8 == len(data)
    res = {"chunks": {}, "frames": [], "movi": None, "idx": []}

    def walk(lo, hi, path):
        i = lo
        while i < hi:
            cc, n = data[i:i + 4], struct.unpack("<I", data[i + 4:i + 8])[0]
            assert i + 8 + n <= hi, (path, cc, n)
            if cc == b"LIST":
                kind = data[i + 8:i + 12]
                if kind == b"movi":
                    res["movi"] = i + 8
                walk(i + 12, i + 8 + n, path + kind.decode() + "/")
            else:
                body = data[i + 8:i + 8 + n]
                if cc == b"00dc":
                    res["frames"].append(body)
                else:
                    res["chunks"][path + cc.decode()] = body
            i += 8 + n + (n & 1)
        assert i == hi, (path, i, hi)

    walk(12, len(data), "")
    idx = res["chunks"].get("idx1", b"")
    assert len(idx) % 16 == 0
    res["idx"] = [struct.unpack("<4sIII", idx[j:j + 16]) for j in range(0, len(idx), 16)]
    return res

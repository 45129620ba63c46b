"""Plain-Python restatement of the animated GIF path (GIF89a, one global colour table, LZW minimum code size 8, the raster of
a frame coded in independent chunks), shared by tests/test_gif_cpu.py and tests/test_gif_gpu.py. Written from the GIF89a
specification (W3C, 1990: sections 18-26 and appendix F), independent of the package's kernels and of its container writer.

  histogram()      frames uint8 [T, H, W, 3] -> 32768 counts over (r>>3)<<10 | (g>>3)<<5 | (b>>3)
  map_indices()    frames + palette + dither -> indices uint8 [T, H, W] (ordered dither, exact nearest entry, lowest index on ties)
  lzw_chunk()      indices of one chunk -> its code string (bytes, length in bits)
  image_data()     indices of one frame -> the sub-blocked image data behind the minimum code size byte
  gif_bytes()      palette + image data per frame -> a complete file
  decode()         the STRICT decoder: walks the file, decodes the LZW data with a decoder's own table and refuses whatever a
                   lenient player would forgive (see its docstring)

The chunk rule: a frame's raster is cut into chunks of `chunk` pixels (the last may be shorter; chunks may cross rows). A chunk's
string starts in the reset state (code width 9, next code 258), holds the chunk's data codes - with a Clear at 12 bits and a reset
whenever code 4095 has been assigned - and ends with a Clear if another chunk of the frame follows, with EOI if not. A frame's
code stream is a 9-bit Clear followed by its chunks' strings, bit after bit, codes LSB first, the last byte padded with zeros.
"""
import numpy as np

from tests.jpeg_restatement import make_frames, psnr  # noqa: F401  (the RGB inputs are the Motion-JPEG tests' inputs)

HIST_BINS = 32768
CHUNK_DEFAULT = 8192
CLEAR, EOI, FIRST = 256, 257, 258
CLEAR_INTERVAL = 3838         # data codes from a reset to the one that assigns code 4095 (258 + 3838 - 1 = 4095)


def chunk_max_bytes(n):
    """Worst case of one chunk of n pixels: n data codes, n // 3838 Clears inside it, one terminator, 12 bits each; in whole
    32-bit words."""
    return (12 * (n + n // CLEAR_INTERVAL + 1) + 31) // 32 * 4


def frame_max_bytes(hw, chunk):
    full, rest = divmod(hw, chunk)
    bits = 9 + full * 12 * (chunk + chunk // CLEAR_INTERVAL + 1)
    if rest:
        bits += 12 * (rest + rest // CLEAR_INTERVAL + 1)
    n = (bits + 7) // 8
    return n + (n + 254) // 255 + 1


# ------------------------------------------------------------------------------------------------ inputs
def make_indices(kind, T, H, W, rng):
    """Index planes uint8 [T, H, W]: "noise" = uniform 0..255; "flat" = one value per frame; "runs" = arange // 37 % 256,
    shifted from frame to frame; "smooth" = a slow sine surface."""
    n = H * W
    if kind == "noise":
        v = rng.integers(0, 256, size=(T, n))
    elif kind == "flat":
        v = np.repeat(7 + np.arange(T)[:, None], n, 1)
    elif kind == "runs":
        v = (np.arange(n)[None] + 11 * np.arange(T)[:, None]) // 37 % 256
    elif kind == "smooth":
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        v = np.stack([128 + 100 * np.sin(x / 9 + y / 13 + t / 5) for t in range(T)]).reshape(T, n)
    else:
        raise ValueError(kind)
    return v.astype(np.uint8).reshape(T, H, W)


def ramp_palette(n=256):
    """n distinct colours that are no grey ramp (so that a swapped channel or an off-by-one index shows)."""
    i = np.arange(n)
    return np.stack([i, 255 - i, (i * 7 + 3) % 256], 1).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ histogram, mapping
def histogram(frames):
    f = np.asarray(frames).reshape(-1, 3).astype(np.int64)
    bins = ((f[:, 0] >> 3) << 10) | ((f[:, 1] >> 3) << 5) | (f[:, 2] >> 3)
    return np.bincount(bins, minlength=HIST_BINS).astype(np.uint32)


def bayer(n=8):
    """The n x n ordered-dither index matrix by the usual recursion M(2n) = [[4M, 4M + 2], [4M + 3, 4M + 1]], M(1) = [[0]]."""
    m = np.zeros((1, 1), dtype=np.int64)
    while m.shape[0] < n:
        m = np.block([[4 * m, 4 * m + 2], [4 * m + 3, 4 * m + 1]])
    return m


def map_indices(frames, palette, dither=0):
    """d = floor((2 B[y & 7][x & 7] - 63) * dither / 128); c' = clamp(c + d, 0, 255) per channel; index = the first palette entry
    at the least squared distance to c'."""
    f = np.asarray(frames).astype(np.int64)
    T, H, W, _ = f.shape
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = (2 * bayer(8)[y & 7, x & 7] - 63) * int(dither) // 128                  # Python's // floors
    c = np.clip(f + d[None, :, :, None], 0, 255).reshape(-1, 1, 3)
    pal = np.asarray(palette).astype(np.int64)[None]
    out = np.empty(c.shape[0], dtype=np.uint8)
    for i in range(0, c.shape[0], 4096):
        dist = ((c[i:i + 4096] - pal) ** 2).sum(-1)
        out[i:i + 4096] = np.argmin(dist, 1)                                    # argmin returns the first minimum
    return out.reshape(T, H, W)


# ------------------------------------------------------------------------------------------------ LZW encoder
class _Bits:
    """Codes appended LSB first; whole bytes leave the accumulator as they fill."""

    def __init__(self):
        self.out, self.acc, self.n, self.bits = bytearray(), 0, 0, 0

    def put(self, code, width):
        assert 0 <= code < (1 << width)
        self.acc |= code << self.n
        self.n += width
        self.bits += width
        k = self.n // 8
        self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
        self.acc >>= 8 * k
        self.n -= 8 * k

    def result(self):
        """(bytes, bits): the last byte padded with zero bits"""
        return bytes(self.out) + (bytes([self.acc]) if self.n else b""), self.bits


def lzw_chunk(pixels, last):
    """One chunk -> (bytes, bits). The width of a code is the one a decoder has when it reads it: a decoder that has read j >= 1
    codes since the last reset has added j - 1 entries, its next free code is 258 + j - 1, and it reads at the smallest width
    w in 9..12 with 258 + j - 1 < 2^w. That holds for the terminator too, although the encoder adds no entry in front of it."""
    px = [int(v) for v in np.asarray(pixels).reshape(-1)]
    out = _Bits()
    table, j = {}, 0                             # j = codes written since the last reset

    def width():
        w = 9
        while j >= 1 and 258 + j - 1 >= (1 << w) and w < 12:
            w += 1
        return w

    prefix = px[0]
    for k in px[1:]:
        code = table.get((prefix, k))
        if code is not None:
            prefix = code
            continue
        out.put(prefix, width())
        j += 1
        table[(prefix, k)] = FIRST + j - 1
        prefix = k
        if FIRST + j - 1 == 4095:                # the table is full: Clear at 12 bits, start over
            out.put(CLEAR, 12)
            table, j = {}, 0
    out.put(prefix, width())
    j += 1
    out.put(EOI if last else CLEAR, width())
    return out.result()


def frame_chunks(indices, chunk=None):
    """indices of one frame (any shape) -> [(bytes, bits)] per chunk."""
    px = np.asarray(indices).reshape(-1)
    chunk = CHUNK_DEFAULT if chunk is None else chunk
    starts = range(0, px.size, chunk)
    return [lzw_chunk(px[s:s + chunk], s + chunk >= px.size) for s in starts]


def merge(chunks):
    """A 9-bit Clear, then the chunk strings bit after bit -> the frame's code stream as bytes."""
    out = _Bits()
    out.put(CLEAR, 9)
    for data, bits in chunks:
        v = int.from_bytes(data, "little")
        assert v >> bits == 0 and len(data) == (bits + 7) // 8
        out.put(v, bits)
    return out.result()[0]


def sub_blocks(data):
    out = bytearray()
    for i in range(0, len(data), 255):
        out.append(min(255, len(data) - i))
        out += data[i:i + 255]
    out.append(0)
    return bytes(out)


def image_data(indices, chunk=None):
    return sub_blocks(merge(frame_chunks(indices, chunk)))


# ------------------------------------------------------------------------------------------------ container
def delay_cs(fps):
    return max(2, int(np.floor(100.0 / fps + 0.5)))


def gif_bytes(width, height, palette, images, fps=8, loops=0):
    pal = np.asarray(palette, dtype=np.uint8)
    le16 = lambda v: int(v).to_bytes(2, "little")
    out = bytearray(b"GIF89a" + le16(width) + le16(height) + bytes([0x80 | 0x70 | 0x07, 0, 0]))
    out += pal.tobytes() + bytes(3 * (256 - len(pal)))
    out += bytes([0x21, 0xFF, 11]) + b"NETSCAPE2.0" + bytes([3, 1]) + le16(loops) + b"\x00"
    for d in images:
        out += bytes([0x21, 0xF9, 4, 1 << 2]) + le16(delay_cs(fps)) + bytes([0, 0])
        out += bytes([0x2C]) + le16(0) + le16(0) + le16(width) + le16(height) + bytes([0])
        out += bytes([8]) + d
    out.append(0x3B)
    return bytes(out)


def encode(frames_idx, palette, chunk=None, fps=8, loops=0):
    T, H, W = frames_idx.shape
    return gif_bytes(W, H, palette, [image_data(frames_idx[t], chunk) for t in range(T)], fps, loops)


# ------------------------------------------------------------------------------------------------ strict decoder
class GifError(AssertionError):
    pass


def _need(cond, msg):
    if not cond:
        raise GifError(msg)


def _read_blocks(data, pos):
    """Sub-blocks from pos on -> (payload, position behind the 00 block)."""
    out = bytearray()
    while True:
        _need(pos < len(data), "a sub-block length byte lies beyond the file")
        n = data[pos]
        pos += 1
        if n == 0:
            return bytes(out), pos
        _need(pos + n <= len(data), "a sub-block runs beyond the file")
        out += data[pos:pos + n]
        pos += n


_ROOTS = {i: bytes([i]) for i in range(256)}


def lzw_decode(payload, npix):
    """Appendix F decoder, minimum code size 8, with its own table (entries are added one code later than an encoder adds them).
    Refuses: a stream that does not begin with Clear, a code above the next free one, a data code in front of which nothing can
    be added, more or fewer than npix indices, anything but EOI behind the npix-th index, EOI at another width than the
    decoder's, more than 7 pad bits or a set pad bit, bytes behind the byte that holds EOI."""
    total = 8 * len(payload)
    pos, width, nxt, prev = 0, 9, FIRST, None
    table = dict(_ROOTS)
    out = bytearray()
    first = True
    while True:
        _need(pos + width <= total, f"the data ends inside a code ({len(out)} of {npix} indices decoded)")
        code = (int.from_bytes(payload[pos >> 3:(pos >> 3) + 3], "little") >> (pos & 7)) & ((1 << width) - 1)
        pos += width
        if first:
            _need(code == CLEAR, "the stream does not begin with a Clear code")
            first = False
        if len(out) == npix:
            _need(code == EOI, f"code {code} at width {width} where EOI must follow the last index")
        if code == EOI:
            break
        if code == CLEAR:
            width, nxt, prev = 9, FIRST, None
            table = dict(_ROOTS)
            continue
        if prev is None:
            _need(code < 256, f"code {code} right behind a Clear")
            entry = table[code]
        else:
            _need(code <= nxt and nxt < 4096 or code < nxt, f"code {code} with {nxt} as the next free code")
            entry = table[code] if code < nxt else table[prev] + table[prev][:1]
            if nxt < 4096:
                table[nxt] = table[prev] + entry[:1]
                nxt += 1
                if nxt == (1 << width) and width < 12:
                    width += 1
        out += entry
        _need(len(out) <= npix, "more indices than the frame has pixels")
        prev = code
    _need(len(out) == npix, f"EOI after {len(out)} of {npix} indices")
    _need(total - pos <= 7, f"{total - pos} bits behind EOI")
    _need(total == pos or payload[-1] >> (8 - (total - pos)) == 0, "a pad bit is set")
    return np.frombuffer(bytes(out), dtype=np.uint8)


def decode(data):
    """Walks a file of the layout this project writes and returns dict(width, height, palette [256, 3], loops, delays [cs],
    frames [T, H, W] indices). Refuses anything else: another version, no global table, a local table, interlacing, a frame that
    is not the full screen, an unknown block, a missing trailer, bytes behind the trailer, and what lzw_decode refuses."""
    _need(data[:6] == b"GIF89a", "no GIF89a signature")
    w, h = int.from_bytes(data[6:8], "little"), int.from_bytes(data[8:10], "little")
    packed = data[10]
    _need(packed & 0x80 and (packed & 7) == 7, "no global colour table of 256 entries")
    pos = 13
    palette = np.frombuffer(data[pos:pos + 768], dtype=np.uint8).reshape(256, 3)
    pos += 768
    loops, delays, frames, gce = None, [], [], None
    while True:
        _need(pos < len(data), "no trailer")
        b = data[pos]
        pos += 1
        if b == 0x3B:
            break
        if b == 0x21:
            label = data[pos]
            pos += 1
            payload_at = pos
            payload, pos = _read_blocks(data, pos)
            if label == 0xFF:
                _need(data[payload_at] == 11 and payload[:11] == b"NETSCAPE2.0", "an unknown application extension")
                _need(len(payload) == 14 and payload[11] == 1, "a malformed NETSCAPE2.0 extension")
                loops = int.from_bytes(payload[12:14], "little")
            elif label == 0xF9:
                _need(len(payload) == 4 and data[payload_at] == 4, "a malformed graphic control extension")
                _need(gce is None, "two graphic control extensions in front of one image")
                gce = payload
            else:
                _need(False, f"an unknown extension {label:#x}")
        elif b == 0x2C:
            x, y, fw, fh = (int.from_bytes(data[pos + 2 * i:pos + 2 * i + 2], "little") for i in range(4))
            _need((x, y, fw, fh) == (0, 0, w, h), "a frame that is not the full screen")
            _need(data[pos + 8] == 0, "a local colour table or an interlaced frame")
            pos += 9
            _need(data[pos] == 8, "LZW minimum code size is not 8")
            payload, pos = _read_blocks(data, pos + 1)
            _need(gce is not None, "an image without a graphic control extension")
            _need((gce[0] >> 2) & 7 == 1 and not gce[0] & 1, "disposal is not 1, or a transparent index is set")
            delays.append(int.from_bytes(gce[1:3], "little"))
            gce = None
            frames.append(lzw_decode(payload, w * h).reshape(h, w))
        else:
            _need(False, f"an unknown block {b:#x}")
    _need(pos == len(data), "bytes behind the trailer")
    _need(frames, "no frames")
    return dict(width=w, height=h, palette=palette, loops=loops, delays=delays, frames=np.stack(frames))

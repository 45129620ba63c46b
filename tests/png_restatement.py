"""Plain-Python restatement of the GPU PNG / APNG path (csrc/png.hip, utils/save_video.py deflate="hip"), shared by
tests/test_png_cpu.py and tests/test_png_gpu.py. Written from the PNG specification (W3C, 2nd edition: sections 5, 9, 10), the APNG
specification, RFC 1950 and RFC 1951, independent of the package's kernels and of its container writer.

  filter_plane()   frame uint8 [H, W, C] -> scanlines uint8 [H, 1 + W C]: per row the filter type 0..4 with the least sum of
                   min(r, 256 - r) over its residual bytes, the lowest type on a tie; filters read raw bytes (row 0: a zero row)
  run_tokens()     bytes of one chunk -> literals and distance-1 matches by the greedy run rule
  huff_lengths()   counts -> code lengths under a limit: the builder as the kernel builds it (see its docstring)
  chunk_string()   bytes of one chunk -> its byte-aligned string: one dynamic block + an empty stored block, or one stored block
  zlib_stream()    plane bytes -> 78 01, the chunk strings, Adler-32 (combined from the chunks' own values)
  png_bytes()      frames -> a complete PNG (T = 1, still=True) or APNG file
  decode()         the STRICT decoder (see its docstring)
"""
import functools
import struct
import zlib

import numpy as np

CHUNK_DEFAULT = 16384
CHUNK_LIMIT = 65535           # LEN of a stored block is 16 bits
ADLER_BASE = 65521
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
MAX_ROUNDS = 17               # halvings of a count below 2^16 until it is 1, plus the first build


def chunk_max_bytes(n):
    """Worst case of one chunk of n bytes: the stored form, n + 5; in whole 32-bit words."""
    return (n + 5 + 3) // 4 * 4


def frame_max_bytes(N, chunk):
    return 6 + N + 5 * ((N + chunk - 1) // chunk)


# ------------------------------------------------------------------------------------------------ inputs
def make_frames(kind, T, H, W, C, seed=1):
    """uint8 [T, H, W, C]. "noise" = uniform; "flat" = one value per frame and channel; "ramp" = a smooth diagonal ramp;
    "photo" = four low-frequency sinusoids per channel plus integer noise in -3..3."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if kind == "noise":
        f = rng.integers(0, 256, size=(T, H, W, C))
    elif kind == "flat":
        f = np.broadcast_to((40 + 7 * np.arange(T)[:, None, None, None] + 50 * np.arange(C)) % 256, (T, H, W, C))
    elif kind == "ramp":
        f = np.stack([np.stack([(x * (2 + c) + y * 3) // 4 + 5 * t + 30 * c for c in range(C)], -1) for t in range(T)]) % 256
    elif kind == "photo":
        f = np.empty((T, H, W, C))
        for t in range(T):
            for c in range(C):
                v = np.full((H, W), 128.0)
                for _ in range(4):
                    fx, fy, ph = rng.uniform(0.01, 0.09), rng.uniform(0.01, 0.09), rng.uniform(0, 6.28)
                    v += 28.0 * np.sin(fx * x + fy * y + ph + 0.2 * t)
                f[t, :, :, c] = np.floor(v) + rng.integers(-3, 4, size=(H, W))
        f = np.clip(f, 0, 255)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(f).astype(np.uint8)


RUN_LENGTHS = (1, 2, 3, 4, 259, 260, 261, 262, 517)


def _spread(counts, first):
    """bytes in which byte first + k occurs counts[k] times and no two neighbours are equal, so every byte is a literal: always the
    byte with the most occurrences left that differs from the last one"""
    left, out, total = list(counts), [], sum(counts)
    while len(out) < total:
        k = max((k for k in range(len(left)) if left[k] and (not out or out[-1] != first + k)), key=lambda k: (left[k], -k))
        out.append(first + k)
        left[k] -= 1
    return bytes(out)


def fibonacci_bytes():
    """4180 bytes in which byte k of 17 occurs F(k) = 1, 1, 2, 3, ... 1597 times. With end-of-block that is 18 counts; a Huffman
    build that takes the merged node on a tie makes them one chain, 17 deep. huff_lengths takes the leaf on a tie, which splits
    the chain in two: 9 deep, no halving (tests/test_png_cpu.py pins both numbers)."""
    f = [1, 1]
    while len(f) < 17:
        f.append(f[-1] + f[-2])
    return _spread(f, 100)


@functools.lru_cache(maxsize=None)
def powers_of_two_bytes():
    """65535 bytes (the longest chunk there is) in which byte k of 16 occurs 2^k times: every count equals the sum of all smaller
    ones and end-of-block, so at every step the two lightest are the chain so far and the next leaf, whatever the tie rule: one
    chain, 16 deep, and the 15-bit limit has to act."""
    return _spread([1 << k for k in range(16)], 60)


def cl_overflow_bytes():
    """tests/golden/png_cl_overflow.bin: 4703 bytes, Zipf-distributed over 245 symbols (seed 10 of the seed search DESIGN 4.10 describes), whose
    code-length tokens have the counts 19, 1, 1, 1, 2, 3, 5, 8, 22, 37, 71, 65, 26 for the symbols 0..12: plain Huffman puts them 8
    deep, above the 7 bits the code-length alphabet may use."""
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_cl_overflow.bin"), "rb") as fh:
        return np.frombuffer(fh.read(), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def aimed_planes():
    """name -> (planes uint8 [T, N], chunk): byte planes aimed at single rules of the chunk coder.
    runs: runs of the lengths that sit at the edges of the match rule (3 = the shortest match behind the literal is length 3 at
    run 4; 259 = one full match; 260..262 = a full match and 1, 2 literals or a second match; 517 = two full matches), in one
    chunk; runs-cut: the same bytes in chunks of 300, so runs cross chunk boundaries and are cut there; one-byte: chunks of a
    single distinct byte, 1000, 2 and 1 long; no-match: seven symbols, no run above 3 (the distance code is a single zero
    length); fibonacci: counts with many ties; powers-of-two: the 15-bit limit, in the longest chunk; cl-overflow: the 7-bit limit of the code-length alphabet; noise: the stored form; mixed: noise, runs and zeros in one plane of several chunks."""
    rng = np.random.default_rng(5)
    runs = np.concatenate([np.full(L, (17 + 31 * i) % 256, dtype=np.uint8) for i, L in enumerate(RUN_LENGTHS)])
    runs3 = np.stack([runs, runs[::-1], np.roll(runs, 100)])
    nomatch = (np.arange(3 * 2000).reshape(3, 2000) * 3 % 7 + (np.arange(3 * 2000).reshape(3, 2000) // 3) % 5).astype(np.uint8)
    fib = np.frombuffer(fibonacci_bytes(), dtype=np.uint8)
    mixed = np.concatenate([rng.integers(0, 256, 700), np.zeros(900), rng.integers(0, 4, 800), np.full(300, 9),
                            rng.integers(0, 256, 301)]).astype(np.uint8)
    return {
        "runs": (runs3, runs.size),
        "runs-cut": (runs3, 300),
        "one-byte-1000": (np.full((1, 1000), 0x55, dtype=np.uint8), 1000),
        "one-byte-2": (np.full((3, 4), 7, dtype=np.uint8), 2),
        "one-byte-1": (np.full((1, 3), 0, dtype=np.uint8), 1),
        "no-match": (nomatch, 2000),
        "fibonacci": (fib[None], fib.size),
        "powers-of-two": (np.frombuffer(powers_of_two_bytes(), dtype=np.uint8)[None], 65535),
        "cl-overflow": (cl_overflow_bytes()[None], 4703),
        "noise": (rng.integers(0, 256, size=(3, 5000)).astype(np.uint8), 2048),
        "mixed": (np.stack([mixed, mixed[::-1], np.roll(mixed, 333)]), 1024),
    }


# ------------------------------------------------------------------------------------------------ scanline filters
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_plane(frame):
    """uint8 [H, W, C] -> (scanlines uint8 [H, 1 + W C], the five costs int64 [H, 5])."""
    H, W, C = frame.shape
    x = frame.reshape(H, W * C).astype(np.int64)
    b = np.concatenate([np.zeros((1, W * C), dtype=np.int64), x[:-1]])           # the row above
    a = np.concatenate([np.zeros((H, C), dtype=np.int64), x[:, :-C]], 1) if W > 1 else np.zeros_like(x)
    c = np.concatenate([np.zeros((H, C), dtype=np.int64), b[:, :-C]], 1) if W > 1 else np.zeros_like(x)
    res = np.stack([x, x - a, x - b, x - (a + b) // 2, x - _paeth(a, b, c)]) % 256         # [5, H, W C]
    cost = np.minimum(res, 256 - res).sum(2).T                                             # [H, 5]
    ftype = np.argmin(cost, 1)                                                             # the first of equal minima
    out = np.empty((H, 1 + W * C), dtype=np.uint8)
    out[:, 0] = ftype
    out[:, 1:] = res[ftype, np.arange(H)]
    return out, cost


def unfilter_plane(plane, H, W, C):
    """scanlines [H, 1 + W C] -> uint8 [H, W, C] by the five PNG filters, byte by byte."""
    n = W * C
    prev = [0] * n
    rows = []
    for y in range(H):
        ft, r = int(plane[y, 0]), plane[y, 1:].tolist()
        cur = [0] * n
        for i in range(n):
            a = cur[i - C] if i >= C else 0
            b = prev[i]
            c = prev[i - C] if i >= C else 0
            if ft == 0:
                p = 0
            elif ft == 1:
                p = a
            elif ft == 2:
                p = b
            elif ft == 3:
                p = (a + b) // 2
            elif ft == 4:
                q = a + b - c
                pa, pb, pc = abs(q - a), abs(q - b), abs(q - c)
                p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            else:
                raise PngError(f"row {y}: filter type {ft}")
            cur[i] = (r[i] + p) & 255
        rows.append(cur)
        prev = cur
    return np.array(rows, dtype=np.uint8).reshape(H, W, C)


# ------------------------------------------------------------------------------------------------ tokens
def run_tokens(data):
    """bytes -> tokens: a literal is its byte value 0..255, a match of length m at distance 1 is -m. A maximal run of L equal
    bytes: one literal, then matches of min(rem, 258) while rem >= 3, then the 0..2 bytes left as literals."""
    out, i, n = [], 0, len(data)
    while i < n:
        j = i + 1
        while j < n and data[j] == data[i]:
            j += 1
        out.append(data[i])
        rem = j - i - 1
        while rem >= 3:
            m = min(rem, 258)
            out.append(-m)
            rem -= m
        out += [data[i]] * rem
        i = j
    return out


def length_symbol(m):
    """match length 3..258 -> (symbol 257..285, extra bits, extra value), RFC 1951 section 3.2.5"""
    for k in range(28, -1, -1):
        if m >= LEN_BASE[k]:
            return 257 + k, LEN_EXTRA[k], m - LEN_BASE[k]
    raise ValueError(m)


# ------------------------------------------------------------------------------------------------ code tables
def huff_lengths(counts, limit):
    """Code lengths of a deterministic Huffman build. If a single symbol has a count, the lowest other symbol gets count 1 (a
    code of one symbol would be incomplete). Leaves = the symbols with a count, sorted by (count, symbol). Two queues: the leaves,
    and the merged nodes in the order they are made; each step takes twice the lighter front, the leaf on a tie, and appends
    their sum. While the deepest leaf is deeper than `limit`, every count becomes (count + 1) // 2 and the build runs again."""
    f = list(counts)
    used = [s for s, c in enumerate(f) if c]
    if len(used) == 1:
        f[1 if used[0] == 0 else 0] = 1
    for _ in range(MAX_ROUNDS):
        leaves = sorted((c, s) for s, c in enumerate(f) if c)
        m = len(leaves)
        lw = [c for c, _ in leaves]
        iw, lpar, ipar = [], [0] * m, [0] * (m - 1)
        li = ii = 0
        for k in range(m - 1):
            w = 0
            for _ in range(2):
                if li < m and (ii >= k or lw[li] <= iw[ii]):
                    w += lw[li]
                    lpar[li] = k
                    li += 1
                else:
                    w += iw[ii]
                    ipar[ii] = k
                    ii += 1
            iw.append(w)
        depth = [0] * (m - 1)
        for k in range(m - 3, -1, -1):
            depth[k] = depth[ipar[k]] + 1
        lens = [0] * len(f)
        for i, (_, s) in enumerate(leaves):
            lens[s] = depth[lpar[i]] + 1
        if max(lens) <= limit:
            return lens
        f = [(c + 1) // 2 for c in f]
    raise AssertionError("the halving loop did not end")


def canonical_codes(lens):
    """RFC 1951 section 3.2.2: codes by length, then by symbol; returned bit-reversed (Huffman codes go out MSB first)."""
    maxl = max(lens)
    bl = [0] * (maxl + 2)
    for l in lens:
        if l:
            bl[l] += 1
    nxt, code = [0] * (maxl + 2), 0
    for b in range(1, maxl + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            out[s] = int(format(nxt[l], f"0{l}b")[::-1], 2)
            nxt[l] += 1
    return out


def cl_tokens(seq):
    """code lengths -> (symbol 0..18, extra bits, extra value) by runs. A run of zeros: 18 for min(L, 138) while L >= 11, then 17
    if 3 <= L, else the zeros themselves. A run of v > 0: v once, then 16 for min(L, 6) while L >= 3, then the 0..2 left."""
    out, i, n = [], 0, len(seq)
    while i < n:
        j = i + 1
        while j < n and seq[j] == seq[i]:
            j += 1
        v, L = seq[i], j - i
        if v == 0:
            while L >= 11:
                m = min(L, 138)
                out.append((18, 7, m - 11))
                L -= m
            if L >= 3:
                out.append((17, 3, L - 3))
                L = 0
        else:
            out.append((v, 0, 0))
            L -= 1
            while L >= 3:
                m = min(L, 6)
                out.append((16, 2, m - 3))
                L -= m
        out += [(v, 0, 0)] * L
        i = j
    return out


# ------------------------------------------------------------------------------------------------ one chunk
def _pack(fields):
    """[(value, bits)] LSB first -> (bytes padded with zero bits, bit length)"""
    val = np.array([v for v, _ in fields], dtype=np.uint64)
    nb = np.array([b for _, b in fields], dtype=np.int64)
    end = np.cumsum(nb)
    total = int(end[-1])
    idx = np.arange(total) - np.repeat(end - nb, nb)
    bits = ((np.repeat(val, nb) >> idx.astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits, bitorder="little").tobytes(), total


def dynamic_block(data):
    """One BTYPE 10 block with BFINAL 0 for the bytes -> [(value, bits)]"""
    toks = run_tokens(data)
    cnt = [0] * 286
    cnt[256] = 1
    has_match = False
    for t in toks:
        if t >= 0:
            cnt[t] += 1
        else:
            cnt[length_symbol(-t)[0]] += 1
            has_match = True
    ll = huff_lengths(cnt, 15)
    lc = canonical_codes(ll)
    hlit = max(257, max(s for s in range(286) if ll[s]) + 1)
    ct = cl_tokens(ll[:hlit] + [1 if has_match else 0])
    ccnt = [0] * 19
    for s, _, _ in ct:
        ccnt[s] += 1
    cll = huff_lengths(ccnt, 7)
    clc = canonical_codes(cll)
    hclen = max(4, max(i for i in range(19) if cll[CL_ORDER[i]]) + 1)
    f = [(0, 1), (2, 2), (hlit - 257, 5), (0, 5), (hclen - 4, 4)] + [(cll[CL_ORDER[i]], 3) for i in range(hclen)]
    for s, eb, ev in ct:
        f.append((clc[s], cll[s]))
        if eb:
            f.append((ev, eb))
    for t in toks:
        if t >= 0:
            f.append((lc[t], ll[t]))
        else:
            s, eb, ev = length_symbol(-t)
            f.append((lc[s], ll[s]))
            if eb:
                f.append((ev, eb))
            f.append((0, 1))                                     # distance code 0 (distance 1), one bit
    f.append((lc[256], ll[256]))
    return f


@functools.lru_cache(maxsize=1 << 16)
def chunk_string(data, final):
    """(the chunk's string, True if it is the stored form). (a) the dynamic block, an empty stored block that carries BFINAL,
    padded to the byte, 00 00 FF FF; (b) one stored block; (b) exactly when (a) is not shorter."""
    n = len(data)
    assert 1 <= n <= CHUNK_LIMIT
    body, bits = _pack(dynamic_block(data) + [(1 if final else 0, 1), (0, 2)])
    a = body + b"\x00\x00\xff\xff"
    assert len(body) == (bits + 7) // 8
    if len(a) < n + 5:
        return a, False
    return bytes((1 if final else 0,)) + struct.pack("<HH", n, n ^ 0xFFFF) + data, True


def adler_pair(data):
    """(A, B) of the bytes alone: A = 1 + sum, B = n + sum of (n - i) d[i], both modulo 65521"""
    d = np.frombuffer(data, dtype=np.uint8).astype(np.int64)
    n = d.size
    return int((1 + d.sum()) % ADLER_BASE), int((n + ((n - np.arange(n)) * d).sum()) % ADLER_BASE)


def adler_combine(p1, p2, len2):
    """zlib's adler32_combine on (A, B) pairs"""
    rem = len2 % ADLER_BASE
    s1 = p1[0]
    s2 = (rem * s1) % ADLER_BASE
    s1 += p2[0] + ADLER_BASE - 1
    s2 += p1[1] + p2[1] + ADLER_BASE - rem
    return s1 % ADLER_BASE, s2 % ADLER_BASE


def plane_chunks(plane, chunk=None):
    """plane bytes -> per chunk (string, stored?, A | B << 16)"""
    chunk = CHUNK_DEFAULT if chunk is None else chunk
    data = bytes(plane)
    out = []
    for p in range(0, len(data), chunk):
        d = data[p:p + chunk]
        s, stored = chunk_string(d, p + chunk >= len(data))
        a, b = adler_pair(d)
        out.append((s, stored, a | (b << 16)))
    return out


def zlib_stream(plane, chunk=None):
    chunk = CHUNK_DEFAULT if chunk is None else chunk
    data = bytes(plane)
    parts, pair = [], None
    for i, (s, _, ad) in enumerate(plane_chunks(data, chunk)):
        parts.append(s)
        p = (ad & 0xFFFF, ad >> 16)
        pair = p if pair is None else adler_combine(pair, p, min(chunk, len(data) - i * chunk))
    return b"\x78\x01" + b"".join(parts) + struct.pack(">I", pair[0] | (pair[1] << 16))


# ------------------------------------------------------------------------------------------------ container
def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def container(W, H, C, streams, fps=8, loops=0, still=False):
    """zlib streams per frame -> PNG (still: one stream, no animation chunks) or APNG"""
    out = [b"\x89PNG\r\n\x1a\n", _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, {1: 0, 3: 2, 4: 6}[C], 0, 0, 0))]
    if still:
        assert len(streams) == 1
        return b"".join(out + [_chunk(b"IDAT", streams[0]), _chunk(b"IEND", b"")])
    out.append(_chunk(b"acTL", struct.pack(">II", len(streams), loops)))
    seq = 0
    for i, s in enumerate(streams):
        out.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, W, H, 0, 0, 1, int(fps), 0, 0)))
        seq += 1
        if i == 0:
            out.append(_chunk(b"IDAT", s))
        else:
            out.append(_chunk(b"fdAT", struct.pack(">I", seq) + s))
            seq += 1
    return b"".join(out + [_chunk(b"IEND", b"")])


def png_bytes(frames, chunk=None, fps=8, loops=0, still=False):
    """frames uint8 [T, H, W, C] -> the file deflate="hip" writes"""
    T, H, W, C = frames.shape
    return container(W, H, C, [zlib_stream(filter_plane(frames[t])[0].tobytes(), chunk) for t in range(T)], fps, loops, still)


# ------------------------------------------------------------------------------------------------ the strict decoder
class PngError(ValueError):
    pass


def inflate_strict(stream, N):
    """The zlib stream must inflate to exactly N bytes, end there (eof, which includes a matching Adler-32) and leave nothing."""
    d = zlib.decompressobj()
    try:
        raw = d.decompress(stream)
    except zlib.error as e:
        raise PngError(f"inflate: {e}")
    if not d.eof or d.unused_data or d.unconsumed_tail:
        raise PngError("the stream does not end where its data ends")
    if len(raw) != N:
        raise PngError(f"{len(raw)} bytes inflated, {N} expected")
    return raw


def decode(data):
    """Walks a PNG / APNG file and refuses: a bad signature or CRC, chunks out of order, an APNG sequence number out of order, a
    frame count that differs from acTL, a frame that is not the full canvas, a stream that does not pass inflate_strict, a filter
    byte above 4, bytes behind IEND. Returns {width, height, channels, frames uint8 [T, H, W, C], fps, loops, filters [T][H]}."""
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise PngError("signature")
    pos, chunks = 8, []
    while pos < len(data):
        if pos + 12 > len(data):
            raise PngError("truncated chunk")
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if len(body) != n or pos + 12 + n > len(data):
            raise PngError("chunk runs beyond the file")
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != zlib.crc32(tag + body) & 0xFFFFFFFF:
            raise PngError(f"CRC of {tag}")
        chunks.append((tag, body))
        pos += 12 + n
        if tag == b"IEND":
            break
    if pos != len(data) or not chunks or chunks[-1][0] != b"IEND" or chunks[0][0] != b"IHDR":
        raise PngError("IHDR first, IEND last, nothing behind")
    W, H, depth, color, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    if depth != 8 or color not in (0, 2, 6) or comp or flt or lace:
        raise PngError("IHDR")
    C = {0: 1, 2: 3, 6: 4}[color]
    streams, seq, nframes, loops, fps, pending = [], 0, None, 0, None, False
    for tag, body in chunks[1:-1]:
        if tag == b"acTL":
            nframes, loops = struct.unpack(">II", body)
        elif tag == b"fcTL":
            s, w, h, x, y, num, den, dis, blend = struct.unpack(">IIIIIHHBB", body)
            if s != seq or (w, h, x, y) != (W, H, 0, 0) or pending:
                raise PngError("fcTL")
            fps = den / num
            seq += 1
            pending = True
        elif tag == b"IDAT":
            if streams or (nframes is not None and not pending):
                raise PngError("IDAT")
            streams.append(body)
            pending = False
        elif tag == b"fdAT":
            if not pending or struct.unpack(">I", body[:4])[0] != seq or not streams:
                raise PngError("fdAT")
            seq += 1
            streams.append(body[4:])
            pending = False
        else:
            raise PngError(f"unexpected chunk {tag}")
    if pending or not streams or (nframes is not None and nframes != len(streams)):
        raise PngError("frame count")
    frames, filters = [], []
    for s in streams:
        plane = np.frombuffer(inflate_strict(s, H * (1 + W * C)), dtype=np.uint8).reshape(H, 1 + W * C)
        if plane[:, 0].max() > 4:
            raise PngError("filter type above 4")
        filters.append(plane[:, 0].tolist())
        frames.append(unfilter_plane(plane, H, W, C))
    return {"width": W, "height": H, "channels": C, "frames": np.stack(frames), "fps": fps, "loops": loops, "filters": filters}

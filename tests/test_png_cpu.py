"""PNG / APNG output with deflate="hip", the parts that need no GPU: the restatement (tests/png_restatement.py - the reference of
the GPU tests) against Pillow's decoder, zlib's inflate and its own strict decoder, its size against zlib's Z_RLE strategy and
against the deflate="zlib" path, the bound macros, the argument checks of the three dc_png_* entries, and the deflate= keyword of
the writers on the host.

Frames (seeded): "noise", "flat", "ramp", "photo" at 96x160x3, 33x17x3, 1x1x3, 96x160x1, 96x160x4; chunks of 1, 7 and 64 bytes, the
whole frame, the default 16384; 160x160x3 at 65535. T = 2, or 1 where the Python loop walks tens of thousands of chunks."""
import ctypes as C
import functools
import io
import os
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import png_restatement as P

SHAPES = [(96, 160, 3), (33, 17, 3), (1, 1, 3), (96, 160, 1), (96, 160, 4)]
KINDS = ["noise", "flat", "ramp", "photo"]
CHUNKS = [1, 7, 64, "frame", 16384]
_ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


@functools.lru_cache(maxsize=None)
def _frames(kind, shape):
    f = P.make_frames(kind, 2, *shape)
    f.setflags(write=False)
    return f


def _decodes_everywhere(data, f, fps=8, loops=0):
    T, H, W, Cc = f.shape
    d = P.decode(data)
    assert (d["width"], d["height"], d["channels"], d["loops"]) == (W, H, Cc, loops) and d["fps"] in (fps, None)
    assert (d["frames"] == f).all()
    im = Image.open(io.BytesIO(data))
    assert im.size == (W, H) and getattr(im, "n_frames", 1) == T
    for t in range(T):
        im.seek(t)
        assert (np.asarray(im.convert({1: "L", 3: "RGB", 4: "RGBA"}[Cc])).reshape(H, W, Cc) == f[t]).all(), f"frame {t}"
    return d


# ------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("chunk", CHUNKS, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_decodes_exactly_in_pillow_and_in_the_strict_decoder(kind, shape, chunk):
    f = _frames(kind, shape)
    N = shape[0] * (1 + shape[1] * shape[2])
    chunk = N if chunk == "frame" else chunk
    if chunk in (1, 7) and N > 10000:
        f = f[:1]
    _decodes_everywhere(P.png_bytes(f, chunk, fps=8, loops=0), f)
    for t in range(f.shape[0]):
        s = P.zlib_stream(P.filter_plane(f[t])[0].tobytes(), chunk)
        assert len(s) <= P.frame_max_bytes(N, chunk)
    if shape == (33, 17, 3):
        _decodes_everywhere(P.png_bytes(f[:1], chunk, still=True), f[:1])


def test_restatement_at_the_largest_chunk():
    f = _frames("photo", (160, 160, 3))
    N = 160 * 481
    assert (N + 65534) // 65535 == 2
    _decodes_everywhere(P.png_bytes(f, 65535, fps=10, loops=3), f, fps=10, loops=3)
    with pytest.raises(AssertionError):
        P.chunk_string(bytes(65536), True)


def test_filter_choice_follows_the_rule():
    """argmin with the first of equal minima; the costs are sums of min(r, 256 - r); un-filtering gives the frame back."""
    f = _frames("photo", (96, 160, 3))[0]
    plane, cost = P.filter_plane(f)
    for y in range(96):
        ft = int(plane[y, 0])
        assert cost[y, ft] == cost[y].min() and (cost[y, :ft] > cost[y, ft]).all()
        r = plane[y, 1:].astype(np.int64)
        assert int(np.minimum(r, 256 - r).sum()) == cost[y, ft]
    assert (P.unfilter_plane(plane, 96, 160, 3) == f).all()
    assert len(set(plane[:, 0].tolist())) >= 2
    z = np.zeros((3, 5, 3), dtype=np.uint8)
    assert (P.filter_plane(z)[0] == 0).all()                     # all five cost 0: None wins the tie


def test_strict_decoder_refuses_the_classic_mistakes():
    f = _frames("ramp", (33, 17, 3))
    good = P.png_bytes(f, 64)
    P.decode(good)
    plane = P.filter_plane(f[0])[0].tobytes()
    s = P.zlib_stream(plane, 64)
    N = len(plane)
    wrong_adler = s[:-4] + struct.pack(">I", (struct.unpack(">I", s[-4:])[0] + 1) & 0xFFFFFFFF)
    not_final = b"\x78\x01" + b"".join(c for c, _, _ in P.plane_chunks(plane + b"\x00", 64)[:-1]) + s[-4:]
    bad5 = bytearray(plane)
    bad5[0] = 5
    for bad in (wrong_adler, s + b"\x00", s[:-1], not_final):
        with pytest.raises(P.PngError):
            P.inflate_strict(bad, N)
    with pytest.raises(P.PngError):
        P.inflate_strict(s, N + 1)
    for bad in (good[:-1], good + b"\x00", good[:40] + bytes((good[40] ^ 1,)) + good[41:],
                P.container(17, 33, 3, [P.zlib_stream(bytes(bad5), 64)], still=True),
                P.container(17, 33, 3, [s], still=False)[:-12],
                P.container(17, 32, 3, [s], still=True)):
        with pytest.raises(P.PngError):
            P.decode(bad)


# ------------------------------------------------------------------------------------------------ 2. aimed byte planes
def test_token_rule_at_the_edges_of_the_match_lengths():
    t = lambda L: P.run_tokens(bytes([9]) * L)
    assert t(1) == [9] and t(2) == [9, 9] and t(3) == [9, 9, 9] and t(4) == [9, -3]
    assert t(259) == [9, -258] and t(260) == [9, -258, 9] and t(261) == [9, -258, 9, 9] and t(262) == [9, -258, -3]
    assert t(517) == [9, -258, -258] and t(518) == [9, -258, -258, 9]
    assert P.run_tokens(bytes([1, 1, 2, 2, 2, 2, 2, 3])) == [1, 1, 2, -4, 3]
    for m, want in ((3, (257, 0, 0)), (10, (264, 0, 0)), (11, (265, 1, 0)), (12, (265, 1, 1)), (18, (268, 1, 1)), (19, (269, 2, 0)),
                    (130, (280, 4, 15)), (226, (283, 5, 31)), (131, (281, 5, 0)), (227, (284, 5, 0)), (257, (284, 5, 30)), (258, (285, 0, 0))):
        assert P.length_symbol(m) == want


@pytest.mark.parametrize("name", sorted(P.aimed_planes()))
def test_aimed_planes_inflate_exactly(name):
    planes, chunk = P.aimed_planes()[name]
    T, N = planes.shape
    for t in range(T):
        data = planes[t].tobytes()
        s = P.zlib_stream(data, chunk)
        assert P.inflate_strict(s, N) == data and len(s) <= P.frame_max_bytes(N, chunk)
        parts = P.plane_chunks(data, chunk)
        assert len(parts) == (N + chunk - 1) // chunk
        for i, (string, stored, adler) in enumerate(parts):
            d = data[i * chunk:(i + 1) * chunk]
            assert adler == zlib.adler32(d) and len(string) <= len(d) + 5
            assert stored == (string[0] & 6 == 0 and len(string) == len(d) + 5)
            assert zlib.decompressobj(-15).decompress(string) == d          # every chunk string inflates on its own
    stored = [st for _, st, _ in P.plane_chunks(planes[0].tobytes(), chunk)]
    if name in ("noise", "one-byte-1", "one-byte-2"):
        assert all(stored)                                       # noise must take the stored form; so do chunks of one or two bytes
    if name in ("runs", "runs-cut", "one-byte-1000", "no-match", "fibonacci", "powers-of-two", "cl-overflow", "mixed"):
        assert not any(stored)


def test_the_cases_reach_the_paths_they_are_there_for():
    planes, chunk = P.aimed_planes()["runs-cut"]
    cuts = set(range(chunk, planes.shape[1], chunk))
    edges = set(np.cumsum(P.RUN_LENGTHS).tolist())
    assert cuts - edges, "no run crosses a chunk boundary"
    toks = P.run_tokens(P.aimed_planes()["no-match"][0][0].tobytes())
    assert min(toks) >= 0
    assert min(P.run_tokens(P.aimed_planes()["one-byte-1000"][0][0].tobytes())) == -258
    # Fibonacci counts: 17 symbols, 4180 bytes, all literals. A build that takes the merged node on ties chains the 18 counts 17
    # deep; this builder takes the leaf, which splits the chain in two: 9 deep, complete, and the 15-bit limit does not act
    fib = P.fibonacci_bytes()
    cnt = np.bincount(np.frombuffer(fib, dtype=np.uint8), minlength=286).tolist()
    assert len(fib) == 4180 and sorted(c for c in cnt if c) == [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597]
    assert min(P.run_tokens(fib)) >= 0
    cnt[256] = 1
    lens = P.huff_lengths(cnt, 15)
    assert lens == P.huff_lengths(cnt, 99) and max(lens) == 9 and sum(2.0 ** -l for l in lens if l) == 1.0
    # powers of two: one chain whatever the tie rule, 16 deep in 65535 bytes; the builder ends within 15 with a complete code
    pw = P.powers_of_two_bytes()
    cnt = np.bincount(np.frombuffer(pw, dtype=np.uint8), minlength=286).tolist()
    assert len(pw) == 65535 and sorted(c for c in cnt if c) == [1 << k for k in range(16)] and min(P.run_tokens(pw)) >= 0
    cnt[256] = 1
    assert max(P.huff_lengths(cnt, 99)) == 16
    lens = P.huff_lengths(cnt, 15)
    assert max(lens) <= 15 and lens != P.huff_lengths(cnt, 99) and sum(2.0 ** -l for l in lens if l) == 1.0
    # the code-length alphabet of the seed-search plane: 8 deep without the limit, 7 with it, still complete
    ov = P.cl_overflow_bytes().tobytes()
    c2 = [0] * 286
    c2[256] = 1
    for tk in P.run_tokens(ov):
        c2[tk if tk >= 0 else P.length_symbol(-tk)[0]] += 1
    ll = P.huff_lengths(c2, 15)
    cc = [0] * 19
    for s, _, _ in P.cl_tokens(ll[:max(257, max(s for s in range(286) if ll[s]) + 1)] + [1 if min(P.run_tokens(ov)) < 0 else 0]):
        cc[s] += 1
    assert max(P.huff_lengths(cc, 99)) == 8
    cl = P.huff_lengths(cc, 7)
    assert max(cl) == 7 and sum(2.0 ** -l for l in cl if l) == 1.0


def test_length_builder_on_hand_made_counts():
    assert P.huff_lengths([5, 0, 0, 0], 15) == [1, 1, 0, 0]      # a single symbol: the lowest other one joins it
    assert P.huff_lengths([0, 0, 7], 15) == [1, 0, 1]
    assert P.huff_lengths([1, 1, 1, 1], 15) == [2, 2, 2, 2]
    assert P.huff_lengths([1, 1, 2], 15) == [2, 2, 1]
    assert P.huff_lengths([2, 1, 1], 15) == [1, 2, 2]
    assert max(P.huff_lengths([1] * 286, 15)) == 9 and max(P.huff_lengths([1] * 19, 7)) == 5
    pw = [1, 1, 2, 4, 8, 16, 32, 64, 128]                        # one chain, 8 deep: the 7-bit limit halves until it fits
    assert P.huff_lengths(pw + [0] * 10, 99) == [8, 8, 7, 6, 5, 4, 3, 2, 1] + [0] * 10
    lens = P.huff_lengths(pw + [0] * 10, 7)
    assert max(lens) <= 7 and sum(2.0 ** -l for l in lens if l) == 1.0 and lens[9:] == [0] * 10
    assert P.canonical_codes([2, 1, 3, 3]) == [0b01, 0b0, 0b011, 0b111]          # 10, 0, 110, 111 read from the top bit
    assert P.cl_tokens([0] * 150 + [5] * 9 + [0, 0] + [3] * 3) == [(18, 7, 127), (18, 7, 1), (5, 0, 0), (16, 2, 3), (5, 0, 0),
                                                                 (5, 0, 0), (0, 0, 0), (0, 0, 0), (3, 0, 0), (3, 0, 0), (3, 0, 0)]
    assert P.cl_tokens([0] * 10 + [7] * 4) == [(17, 3, 7), (7, 0, 0), (16, 2, 0)]


def test_adler_combine_matches_zlib():
    rng = np.random.default_rng(3)
    data = rng.integers(0, 256, 70000).astype(np.uint8).tobytes()
    pair = lambda d: (zlib.adler32(d) & 0xFFFF, zlib.adler32(d) >> 16)
    assert P.adler_pair(data[:65535]) == pair(data[:65535])
    acc = P.adler_pair(data[:1000])
    for p in range(1000, 70000, 23000):
        acc = P.adler_combine(acc, P.adler_pair(data[p:p + 23000]), len(data[p:p + 23000]))
    assert acc == pair(data)


# ------------------------------------------------------------------------------------------------ 3. sizes
def _rle_yardstick(plane, chunk):
    total = 0
    for p in range(0, len(plane), chunk):
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        total += len(co.compress(plane[p:p + chunk]) + co.flush())
    return total


@pytest.mark.parametrize("case", [("photo", (96, 160, 3)), ("ramp", (96, 160, 3)), ("flat", (96, 160, 3)), ("noise", (96, 160, 3)),
                                  ("photo", (160, 160, 3))], ids=lambda c: f"{c[0]}-{_ids(c[1])}")
def test_stream_size_against_zlib_rle_per_chunk(case):
    """At chunk 16384 the stream is at most the summed length of zlib's Z_RLE deflate of every chunk of the same filtered bytes,
    plus 6 (header, Adler), plus 5 per chunk (the alignment block), plus 0.5 %."""
    kind, shape = case
    plane = P.filter_plane(_frames(kind, shape)[0])[0].tobytes()
    N, nch = len(plane), (len(plane) + 16383) // 16384
    ours, rle = len(P.zlib_stream(plane, 16384)), _rle_yardstick(plane, 16384)
    print(f"{kind} {shape}: stream {ours} bytes = {ours / N:.4f} of the scanlines; zlib Z_RLE per chunk {rle}; "
          f"ours without header, trailer and alignment blocks {ours - 6 - 5 * nch} ({(ours - 6 - 5 * nch) / rle:.5f} of it)")
    assert ours <= (rle + 6 + 5 * nch) * 1.005
    assert ours <= P.frame_max_bytes(N, 16384)
    if kind == "noise":
        assert ours == P.frame_max_bytes(N, 16384)


@pytest.mark.parametrize("kind", ["photo", "ramp"])
def test_file_is_smaller_than_the_zlib_path_writes(kind, tmp_path):
    from dynamicrafter_amd.utils import save_video as S
    f = _frames(kind, (96, 160, 3))
    hip = P.png_bytes(f, None, fps=8)
    z = os.path.getsize(S.write_apng(str(tmp_path / "z.png"), np.array(f), fps=8, deflate="zlib"))
    print(f"{kind}: restatement of deflate='hip' {len(hip)} bytes, deflate='zlib' {z} bytes")
    assert len(hip) < z


# ------------------------------------------------------------------------------------------------ 4. bounds, entries, host code
def test_bounds_are_the_same_in_the_header_the_wrappers_and_the_restatement():
    from dynamicrafter_amd import _hip, ops
    hdr = open(os.path.join(os.path.dirname(_hip._HERE), "include", "dcrafter_hip.h")).read()
    assert "#define DC_PNG_CHUNK 16384 " in hdr and "#define DC_PNG_CHUNK_LIMIT 65535 " in hdr
    assert "#define DC_PNG_CHUNK_MAX_BYTES(n) (((n) + 5LL + 3) / 4 * 4)" in hdr
    assert "#define DC_PNG_FRAME_MAX_BYTES(N, chunk) (6LL + (N) + 5LL * (((N) + (chunk) - 1LL) / (chunk)))" in hdr
    assert ops.PNG_CHUNK == P.CHUNK_DEFAULT == 16384 and ops.PNG_CHUNK_LIMIT == P.CHUNK_LIMIT == 65535
    for n in (1, 2, 3, 4, 7, 1716, 16384, 46176, 65535, 1771776):
        assert ops.png_chunk_max_bytes(n) == P.chunk_max_bytes(n) >= n + 5 and P.chunk_max_bytes(n) % 4 == 0
        for chunk in (1, 7, 16384, 65535):
            assert ops.png_frame_max_bytes(n, chunk) == P.frame_max_bytes(n, chunk) == 6 + n + 5 * -(-n // chunk)


def test_png_entries_reject_bad_arguments_without_gpu():
    """Null pointers and a misaligned scratch -> DC_ERR_ARG (-2); sizes below 1, channels other than 1, 3, 4, a chunk above 65535,
    a stride below the worst case or no multiple of 4, offsets beyond 31 bits -> DC_ERR_SHAPE (-1); all before any launch."""
    from dynamicrafter_amd import _hip
    lib = _hip.lib()
    p = C.c_void_p(8)
    assert lib.dc_png_filter(None, p, 1, 16, 16, 3, None) == -2
    assert lib.dc_png_filter(p, None, 1, 16, 16, 3, None) == -2
    for bad in ((0, 16, 16, 3), (1, 0, 16, 3), (1, 16, 0, 3), (1, 16, 16, 2), (1, 16, 16, 0), (1, 16, 16, 5)):
        assert lib.dc_png_filter(p, p, *bad, None) == -1
    assert lib.dc_png_filter(p, p, 1, 65536, 16384, 3, None) == -1            # a plane of 2^31 bytes and more
    stride = P.chunk_max_bytes(100)
    ok = (1, 256, 100, stride)
    for i in range(4):
        args = [p, p, p, p]
        args[i] = None
        assert lib.dc_png_deflate(*args, *ok, None) == -2
    assert lib.dc_png_deflate(p, C.c_void_p(10), p, p, *ok, None) == -2
    for bad in ((0, 256, 100, stride), (1, 0, 100, stride), (1, 256, 0, stride), (1, 256, 100, stride - 4), (1, 256, 100, stride + 2),
                (1, 50, 100, P.chunk_max_bytes(50) - 4),                        # the frame is the longest chunk
                (1, 1 << 20, 65536, P.chunk_max_bytes(65536)),                  # LEN of a stored block is 16 bits
                (1 << 16, 1 << 30, 1 << 14, P.chunk_max_bytes(1 << 14))):       # 2^32 chunks
        assert lib.dc_png_deflate(p, p, p, p, *bad, None) == -1
    ok = (1, 256, 100, stride, 1000)
    for i in range(6):
        args = [p] * 6
        args[i] = None
        assert lib.dc_png_pack(*args, *ok, None) == -2
    for bad in ((0, 256, 100, stride, 1000), (65536, 256, 100, stride, 1000), (1, 0, 100, stride, 1000), (1, 256, 0, stride, 1000),
                (1, 256, 65536, stride, 1000), (1, 256, 100, 0, 1000), (1, 256, 100, stride, 0),
                (1, 1 << 30, 1, 8, 1000)):                                      # 2^30 chunks of 8 bytes: offsets pass 2^31
        assert lib.dc_png_pack(p, p, p, p, p, p, *bad, None) == -1


def _today(frames, fps=8, loops=0):
    """What write_apng wrote before deflate= existed: zlib level 6 on filter-0 scanlines in the APNG framing."""
    T, H, W, Cc = frames.shape
    raw = lambda f: b"".join(b"\x00" + f[y].tobytes() for y in range(H))
    return P.container(W, H, Cc, [zlib.compress(raw(frames[t]), 6) for t in range(T)], fps, loops)


def test_default_writes_what_it_wrote_before(tmp_path, monkeypatch):
    import torch
    from dynamicrafter_amd.utils import save_video as S
    monkeypatch.delenv("DC_PNG_DEFLATE", raising=False)
    f = np.array(_frames("photo", (33, 17, 3)))
    for i, src in enumerate((f, torch.from_numpy(f))):
        a = S.write_apng(str(tmp_path / f"a{i}.png"), src, fps=8)
        assert open(a, "rb").read() == _today(f)
        b = S.write_apng(str(tmp_path / f"b{i}.png"), src, fps=8, deflate="zlib")
        assert open(b, "rb").read() == _today(f)
        p = S.write_png(str(tmp_path / f"p{i}.png"), src[1])
        raw = b"".join(b"\x00" + f[1, y].tobytes() for y in range(33))
        assert open(p, "rb").read() == P.container(17, 33, 3, [zlib.compress(raw, 6)], still=True)
    g = np.array(_frames("ramp", (96, 160, 4)))
    assert open(S.write_apng(str(tmp_path / "g.png"), g, fps=10, loops=2), "rb").read() == _today(g, 10, 2)


def test_deflate_keyword_and_environment_on_the_host(tmp_path, monkeypatch):
    import torch
    from dynamicrafter_amd.utils import save_video as S
    monkeypatch.delenv("DC_PNG_DEFLATE", raising=False)
    cpu = torch.zeros(2, 16, 16, 3, dtype=torch.uint8)
    out = tmp_path / "out"
    out.mkdir()
    x = str(out / "x.png")
    for src in (cpu, cpu.numpy()):
        with pytest.raises(RuntimeError):
            S.write_apng(x, src, deflate="hip")
        with pytest.raises(RuntimeError):
            S.write_png(x, src[0], deflate="hip")
        with pytest.raises(RuntimeError):
            S._write_clip(str(out / "x"), src, 8, "apng", 90, deflate="hip")
    with pytest.raises(RuntimeError):
        S.encode_png_frames(cpu)
    for bad in ("gpu", "", "HIP", 6):
        with pytest.raises(ValueError):
            S.write_apng(x, cpu, deflate=bad)
        with pytest.raises(ValueError):
            S.write_png(x, cpu[0], deflate=bad)
    assert S.png_deflate_mode() == "zlib" and S.png_deflate_mode("hip") == "hip"
    monkeypatch.setenv("DC_PNG_DEFLATE", "hip")                  # the variable is honoured ...
    assert S.png_deflate_mode() == "hip"
    with pytest.raises(RuntimeError):
        S.write_apng(x, cpu)
    with pytest.raises(RuntimeError):
        S.write_png(x, cpu[0])
    assert not os.listdir(out)                                   # nothing above left a file
    z = S.write_apng(str(tmp_path / "z.png"), cpu, deflate="zlib")              # ... and an explicit keyword overrides it
    assert open(z, "rb").read() == _today(cpu.numpy())
    monkeypatch.setenv("DC_PNG_DEFLATE", "fast")
    with pytest.raises(ValueError):
        S.write_apng(x, cpu)
    monkeypatch.setenv("DC_PNG_DEFLATE", "")                     # an empty variable is no variable
    assert open(S.write_apng(str(tmp_path / "e.png"), cpu), "rb").read() == _today(cpu.numpy())
    monkeypatch.setenv("DC_PNG_DEFLATE", "zlib")
    assert open(S.write_apng(str(tmp_path / "e2.png"), cpu), "rb").read() == _today(cpu.numpy())

"""Same-box timing of the two ways a decoded clip becomes an APNG (utils/save_video.py write_apng): deflate="zlib" (frames_to_uint8,
the whole uint8 clip to the host, zlib level 6 on filter-0 scanlines, frame after frame) against deflate="hip" (frames_to_uint8,
dc_png_filter / dc_png_deflate / dc_png_pack, the packed zlib streams to the host, chunk framing and CRCs). Wall time from the
decoded fp32 tensor on the GPU to a closed file, the two paths alternating in one process, median of --runs; the file sizes; the
three stages' times from HIP events (ops.Tracer) in a run of their own; the host's share of the "hip" path (CRC + file write of
streams it already holds); and the stream size and the deflate launch's time at the chunk sizes of --chunks. The "hip" file is
decoded once by Pillow and compared with the frames.

usage: python tools/png_ab.py [--res 1024] [--frames 16] [--runs 5] [--chunks 8192,16384,32768] [--out FILE]
The clip is tools/mjpeg_ab.py's (drifting sines, a checkerboard and 0.05 N(0,1) of noise per pixel): a synthetic clip, not a decoded
model clip; sizes depend on content, times hardly. Prints one JSON object (and writes it to --out)."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mjpeg_ab import SIZES, make_clip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="1024", choices=sorted(SIZES))
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chunks", default="8192,16384,32768")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("png_ab.py measures on the GPU; none found")
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.utils import save_video as S
    dev = torch.device("cuda:0")
    h, w = SIZES[args.res]
    clip = make_clip(args.frames, h, w, dev)
    tmp = tempfile.mkdtemp(prefix="png_ab_")
    paths = {k: os.path.join(tmp, f"{k}.png") for k in ("zlib", "hip")}
    fns = {k: (lambda k=k: S.write_apng(paths[k], S.frames_to_uint8(clip), fps=8, deflate=k)) for k in paths}
    for fn in fns.values():                                      # warm-up: code objects, allocator, page cache
        fn()
    torch.cuda.synchronize()
    wall = {k: [] for k in fns}
    for _ in range(args.runs):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                                 # ends with the file closed (both paths synchronise on their copy)
            wall[k].append(time.perf_counter() - t0)
    sizes = {k: os.path.getsize(p) for k, p in paths.items()}
    grid = S.frames_to_uint8(clip)
    from PIL import Image
    im = Image.open(paths["hip"])
    host_grid = grid.cpu().numpy()
    same = im.n_frames == args.frames
    for t in range(args.frames):
        im.seek(t)
        same = same and bool((np.asarray(im.convert("RGB")) == host_grid[t]).all())
    with ops.Tracer() as tr:
        streams = S.encode_png_frames(grid)
    torch.cuda.synchronize()
    kern = {k: round(v["ms"], 4) for k, v in tr.summary().items()}
    enc_s, host_s = [], []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        streams = S.encode_png_frames(grid)                      # launches, the sync on frame_len, the copy of the streams
        t1 = time.perf_counter()
        buf = io.BytesIO()
        for i, s in enumerate(streams):
            buf.write(S._chunk(b"IDAT" if i == 0 else b"fdAT", s))
        with open(paths["hip"], "wb") as fh:
            fh.write(buf.getvalue())
        host_s.append(time.perf_counter() - t1)
        enc_s.append(t1 - t0)
    by_chunk, ms_by_chunk = {}, {}
    for c in (int(v) for v in args.chunks.split(",") if v):
        with ops.Tracer() as trc:
            by_chunk[str(c)] = sum(len(d) for d in S.encode_png_frames(grid, chunk=c))
        torch.cuda.synchronize()
        ms_by_chunk[str(c)] = round(trc.summary()["png_deflate"]["ms"], 4)
    res = {
        "tool": "png_ab", "device": torch.cuda.get_device_name(0), "clip": [args.frames, h, w], "chunk": ops.PNG_CHUNK,
        "runs": args.runs, "hip_file_decodes_to_the_frames": same,
        "zlib_wall_s_median": round(statistics.median(wall["zlib"]), 4), "zlib_wall_s": [round(v, 4) for v in wall["zlib"]],
        "hip_wall_s_median": round(statistics.median(wall["hip"]), 4), "hip_wall_s": [round(v, 4) for v in wall["hip"]],
        "zlib_bytes": sizes["zlib"], "hip_bytes": sizes["hip"], "uint8_clip_bytes": int(grid.numel()),
        "hip_stream_bytes": sum(len(s) for s in streams), "png_kernels_ms": kern,
        "hip_encode_to_host_ms_median": round(1e3 * statistics.median(enc_s), 3),
        "hip_crc_and_write_ms_median": round(1e3 * statistics.median(host_s), 3),
        "hip_stream_bytes_by_chunk": by_chunk, "png_deflate_ms_by_chunk": ms_by_chunk,
    }
    for p in paths.values():
        os.remove(p)
    os.rmdir(tmp)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

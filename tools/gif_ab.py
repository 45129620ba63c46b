"""Same-box timing of the two ways a decoded clip becomes a file anyone can look at (utils/save_video.py): APNG (frames_to_uint8,
the whole uint8 clip to the host, zlib level 6 per frame) against animated GIF (frames_to_uint8, histogram, the palette on the
host, dc_gif_map / dc_gif_lzw / dc_gif_pack, the packed image data to the host, container assembly). Wall time from the decoded
fp32 tensor on the GPU to a closed file, the two paths alternating, median of --runs; the file sizes; the GIF stages' times from
HIP events (ops.Tracer) and the host palette step from the host clock, in a run of their own; and the image data size and the
LZW launch's time at the chunk sizes of --chunks. There is no earlier GIF path to compare against: the APNG column is there for
scale only.

usage: python tools/gif_ab.py [--res 1024] [--frames 16] [--runs 5] [--dither 0] [--chunks 4096,8192,16384] [--out FILE]
The clip is tools/mjpeg_ab.py's (drifting sines, a checkerboard and 0.05 N(0,1) of noise per pixel): sizes depend on content,
times hardly. Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mjpeg_ab import SIZES, make_clip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="1024", choices=sorted(SIZES))
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dither", type=int, default=0)
    ap.add_argument("--chunks", default="4096,8192,16384")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gif_ab.py measures on the GPU; none found")
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.utils import save_video as S
    dev = torch.device("cuda:0")
    h, w = SIZES[args.res]
    clip = make_clip(args.frames, h, w, dev)
    tmp = tempfile.mkdtemp(prefix="gif_ab_")
    paths = {"apng": os.path.join(tmp, "clip.png"), "gif": os.path.join(tmp, "clip.gif")}

    def apng():
        S.write_apng(paths["apng"], S.frames_to_uint8(clip), fps=8)

    def gif():
        S.write_gif(paths["gif"], S.frames_to_uint8(clip), fps=8, dither=args.dither)

    fns = {"apng": apng, "gif": gif}
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
    with ops.Tracer() as tr:
        palette, images = S.encode_gif_frames(grid, dither=args.dither)
    torch.cuda.synchronize()
    kern = {k: round(v["ms"], 4) for k, v in tr.summary().items()}
    hist = torch.empty(ops.GIF_HIST_BINS, dtype=torch.int32, device=dev)
    ops.gif_histogram(grid, hist)
    host_hist = hist.cpu()
    pal_s = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        S.gif_palette(host_hist)
        pal_s.append(time.perf_counter() - t0)
    by_chunk, lzw_by_chunk = {}, {}
    for c in (int(v) for v in args.chunks.split(",") if v):
        with ops.Tracer() as trc:
            by_chunk[str(c)] = sum(len(d) for d in S.encode_gif_frames(grid, dither=args.dither, chunk=c)[1])
        torch.cuda.synchronize()
        lzw_by_chunk[str(c)] = round(trc.summary()["gif_lzw"]["ms"], 4)
    res = {
        "tool": "gif_ab", "device": torch.cuda.get_device_name(0), "clip": [args.frames, h, w], "dither": args.dither,
        "chunk": ops.GIF_CHUNK, "runs": args.runs, "palette_entries": int(palette.shape[0]),
        "apng_wall_s_median": round(statistics.median(wall["apng"]), 4), "apng_wall_s": [round(v, 4) for v in wall["apng"]],
        "gif_wall_s_median": round(statistics.median(wall["gif"]), 4), "gif_wall_s": [round(v, 4) for v in wall["gif"]],
        "apng_bytes": sizes["apng"], "gif_bytes": sizes["gif"],
        "uint8_clip_bytes": int(grid.numel()), "gif_image_data_bytes": sum(len(d) for d in images),
        "gif_kernels_ms": kern, "gif_palette_host_ms_median": round(1e3 * statistics.median(pal_s), 3),
        "gif_image_data_bytes_by_chunk": by_chunk, "gif_lzw_ms_by_chunk": lzw_by_chunk,
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

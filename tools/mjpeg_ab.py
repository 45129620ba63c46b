"""Same-box A/B of the two ways a decoded clip becomes a file (utils/save_video.py): APNG (frames_to_uint8, the whole uint8
clip to the host, zlib level 6 per frame) against Motion-JPEG AVI (frames_to_uint8, three dc_jpeg_* launches, the packed scans
to the host, RIFF assembly). Wall time from the decoded fp32 tensor on the GPU to a closed file, the two paths alternating,
median of --runs; the file sizes; and the three JPEG stages' times from HIP events (ops.Tracer) in a run of their own.

usage: python tools/mjpeg_ab.py [--res 1024] [--frames 16] [--runs 5] [--quality 90] [--out FILE]
The clip is synthetic (drifting sines, a checkerboard and 0.05 N(0,1) of noise per pixel): sizes depend on content, times
hardly. Prints one JSON object (and writes it to --out)."""
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

SIZES = {"1024": (576, 1024), "512": (320, 512), "256": (256, 256)}


def make_clip(t, h, w, dev):
    g = torch.Generator().manual_seed(1)
    y = torch.arange(h, dtype=torch.float32)[None, :, None]
    x = torch.arange(w, dtype=torch.float32)[None, None, :]
    f = torch.arange(t, dtype=torch.float32)[:, None, None]
    r = torch.sin(x / 37 + y / 53 + f / 5)
    gch = torch.cos(x / 21 - f / 7) * torch.sin(y / 29)
    b = (((x + 2 * f) // 32 + y // 32) % 2) * 1.2 - 0.6
    v = torch.stack([r, gch, b.expand_as(r)], 0) + 0.05 * torch.randn(3, t, h, w, generator=g)
    return v[None].contiguous().to(dev)                          # [1, 3, t, h, w]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="1024", choices=sorted(SIZES))
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mjpeg_ab.py measures on the GPU; none found")
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.utils import save_video as S
    dev = torch.device("cuda:0")
    h, w = SIZES[args.res]
    clip = make_clip(args.frames, h, w, dev)
    tmp = tempfile.mkdtemp(prefix="mjpeg_ab_")
    paths = {"apng": os.path.join(tmp, "clip.png"), "avi": os.path.join(tmp, "clip.avi")}

    def apng():
        S.write_apng(paths["apng"], S.frames_to_uint8(clip), fps=8)

    def avi():
        grid = S.frames_to_uint8(clip)
        S.write_avi_mjpeg(paths["avi"], S.encode_jpeg_frames(grid, quality=args.quality), w, h, 8)

    fns = {"apng": apng, "avi": avi}
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
    grid = S.frames_to_uint8(clip)
    with ops.Tracer() as tr:
        files = S.encode_jpeg_frames(grid, quality=args.quality)
    torch.cuda.synchronize()
    kern = {k: round(v["ms"], 4) for k, v in tr.summary().items()}
    my, mx = ops.jpeg_mcu_grid(h, w)
    res = {
        "tool": "mjpeg_ab", "device": torch.cuda.get_device_name(0), "clip": [args.frames, h, w], "quality": args.quality,
        "restart_mcus": min(8, my * mx), "runs": args.runs,
        "apng_wall_s_median": round(statistics.median(wall["apng"]), 4), "apng_wall_s": [round(v, 4) for v in wall["apng"]],
        "avi_wall_s_median": round(statistics.median(wall["avi"]), 4), "avi_wall_s": [round(v, 4) for v in wall["avi"]],
        "apng_bytes": os.path.getsize(paths["apng"]), "avi_bytes": os.path.getsize(paths["avi"]),
        "uint8_clip_bytes": int(grid.numel()), "packed_scan_bytes": sum(len(f) for f in files),
        "jpeg_kernels_ms": kern,
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

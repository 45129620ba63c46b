"""Same-box A/B of two ways the frames of a Motion-JPEG clip become a uint8 tensor on the GPU: utils/load_video.decode_jpeg_frames
(header parse and segment table on the host, one host-to-device copy of the scans and tables, three dc_jpeg_decode_* launches)
against Pillow (libjpeg) decoding the same files on the host plus one copy of the decoded clip to the device. Wall time from the
files' bytes in host memory to the tensor on the device (the window ends in a device synchronise), the paths alternating, --reps
calls per sample, median of --runs samples.

The clip is written by the package's own encoder at --quality with its default restart interval (8 MCUs), so a 576x1024 frame
is 288 independently decodable segments. The same frames re-encoded by Pillow WITHOUT restart markers are timed too: there one
lane decodes a whole frame, the documented slow case. The three stages' times come from HIP events (ops.Tracer) in runs of their
own.

usage: python tools/mjpeg_decode_ab.py [--res 1024] [--frames 16] [--runs 7] [--reps 3] [--quality 90] [--out FILE]
Prints one JSON object (and writes it to --out)."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mjpeg_ab import SIZES, make_clip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="1024", choices=sorted(SIZES))
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mjpeg_decode_ab.py measures on the GPU; none found")
    from PIL import Image
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.utils import load_video as L
    from dynamicrafter_amd.utils import save_video as S
    dev = torch.device("cuda:0")
    h, w = SIZES[args.res]
    grid = S.frames_to_uint8(make_clip(args.frames, h, w, dev))
    ours = S.encode_jpeg_frames(grid, quality=args.quality)                 # default restart interval
    src = grid.cpu().numpy()
    plain = []
    for t in range(args.frames):                                             # the same frames, no restart markers
        b = io.BytesIO()
        Image.fromarray(src[t]).save(b, "JPEG", quality=args.quality, subsampling=2, optimize=False)
        plain.append(b.getvalue())
    assert L.parse_jpeg(ours[0]).ri > 0 and L.parse_jpeg(plain[0]).ri == 0

    def pillow(files):
        host = np.stack([np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files])
        return torch.from_numpy(host).to(dev)

    fns = {"hip_restart": lambda: L.decode_jpeg_frames(ours, device=dev), "pillow_restart": lambda: pillow(ours),
           "hip_no_restart": lambda: L.decode_jpeg_frames(plain, device=dev), "pillow_no_restart": lambda: pillow(plain)}
    outs = {k: fn() for k, fn in fns.items()}                                # warm-up: code objects, allocator
    torch.cuda.synchronize()
    diff = {}
    for a, b in (("hip_restart", "pillow_restart"), ("hip_no_restart", "pillow_no_restart")):
        d = (outs[a].to(torch.int16) - outs[b].to(torch.int16)).abs()
        diff[a] = {"max_abs_vs_pillow": int(d.max()), "share_above_1": round(float((d > 1).float().mean()), 6)}
    wall = {k: [] for k in fns}
    for _ in range(args.runs):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) / args.reps)
    kern = {}
    for k, files in (("hip_restart", ours), ("hip_no_restart", plain)):
        with ops.Tracer() as tr:
            L.decode_jpeg_frames(files, device=dev)
        torch.cuda.synchronize()
        kern[k] = {name: round(v["ms"], 4) for name, v in tr.summary().items()}
    t0 = time.perf_counter()
    for _ in range(args.reps):
        L.pack_jpeg_batch(ours)
    host_pack = (time.perf_counter() - t0) / args.reps
    res = {
        "tool": "mjpeg_decode_ab", "device": torch.cuda.get_device_name(0), "clip": [args.frames, h, w], "quality": args.quality,
        "restart_mcus": L.parse_jpeg(ours[0]).ri, "segments_per_frame": len(L.scan_segments(ours[0], L.parse_jpeg(ours[0]))),
        "runs": args.runs, "reps": args.reps,
        "file_bytes": {"restart": sum(len(f) for f in ours), "no_restart": sum(len(f) for f in plain)},
        "wall_s_median": {k: round(statistics.median(v), 5) for k, v in wall.items()},
        "wall_s": {k: [round(x, 5) for x in v] for k, v in wall.items()},
        "host_parse_and_pack_s": round(host_pack, 5),
        "kernels_ms": kern, "agreement": diff,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

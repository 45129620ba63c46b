"""The float image resize of the application classes (csrc/preprocess.hip through ops.resize_f32) against
torch.nn.functional.interpolate(mode="bilinear", antialias=True) on the same device tensor, same box, the two alternating.

Cases (a 3000x4000 image, 3 fp32 planes, uniform in [-1, 1] from seed 1):
  exact        resized to exactly 576x1024, what DynamiCrafterImg2VideoPipeline does with height= / width=
  center_crop  Resize(576) -> CenterCrop((576, 1024)): 576x768 and 128 columns of 0.0 each side, what Image2Video.get_image does;
               the baseline is interpolate followed by torch.nn.functional.pad
Per case:
  ours_us / torch_us   HIP events around --iters back-to-back calls (>= 20, after a warm-up of the same calls), per call; median of
                       --runs such windows, ours and torch alternating inside a run. ours writes into a caller's tensor and
                       allocates its intermediate from torch's caching allocator, as the applications call it
  per_kernel_us        ours split by launch (ops.Tracer, a run of its own)
  max_abs_diff         ours against torch's result on the device at the timed size
  floor_us             the source read once plus the result written once at --hbm-tbps

usage: python tools/resize_f32_ab.py [--runs 7] [--iters 20] [--hbm-tbps 4.1] [--out FILE]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HW, VIDEO_SIZE = (3000, 4000), (576, 1024)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters


def measure(name, src, resized, crop, offset, runs, iters, tbps):
    from dynamicrafter_amd import ops
    F = torch.nn.functional
    out = torch.empty((src.shape[0],) + tuple(crop), dtype=torch.float32, device=src.device)
    pad = (-offset[1], crop[1] - resized[1] + offset[1], -offset[0], crop[0] - resized[0] + offset[0])
    ours = lambda: ops.resize_f32(src, resized, crop_hw=crop, offset=offset, antialias=True, out=out)

    def theirs():
        r = F.interpolate(src[None], size=tuple(resized), mode="bilinear", align_corners=False, antialias=True)
        return F.pad(r, pad) if any(pad) else r
    for _ in range(3):
        ours(); theirs()
    torch.cuda.synchronize()
    diff = float((out - theirs()[0]).abs().max())
    t_ours, t_torch = [], []
    for _ in range(runs):
        t_ours.append(window(ours, iters))
        t_torch.append(window(theirs, iters))
    with ops.Tracer() as tr:
        for _ in range(iters):
            ours()
    torch.cuda.synchronize()
    kern = {k: round(v["ms"] * 1000.0 / v["launches"], 2) for k, v in tr.summary().items()}
    nbytes = 4 * (src.numel() + out.numel())
    return {"case": name, "image": list(src.shape), "resized": list(resized), "out": list(out.shape), "offset": list(offset),
            "ours_us": round(statistics.median(t_ours), 2), "ours_us_runs": [round(v, 2) for v in t_ours],
            "torch_us": round(statistics.median(t_torch), 2), "torch_us_runs": [round(v, 2) for v in t_torch],
            "per_kernel_us": kern, "max_abs_diff": diff, "floor_bytes": int(nbytes),
            "floor_us": round(nbytes / (tbps * 1e12) * 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--hbm-tbps", type=float, default=4.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resize_f32_ab.py measures on the GPU; none found")
    if args.iters < 20:
        raise SystemExit("--iters must be at least 20")
    from dynamicrafter_amd.scripts.evaluation.inference import resize_geometry
    dev = torch.device("cuda:0")
    src = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, size=(3,) + HW).astype(np.float32)).to(dev)
    g = resize_geometry(HW[0], HW[1], VIDEO_SIZE)
    cases = [("exact", VIDEO_SIZE, VIDEO_SIZE, (0, 0)),
             ("center_crop", (g.rh, g.rw), VIDEO_SIZE, (g.top - g.pad_top, g.left - g.pad_left))]
    res = {"tool": "resize_f32_ab", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hbm_tbps": args.hbm_tbps,
           "iters": args.iters, "runs": args.runs,
           "cases": [measure(n, src, r, c, o, args.runs, args.iters, args.hbm_tbps) for n, r, c, o in cases]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

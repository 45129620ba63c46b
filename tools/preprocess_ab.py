"""Image -> conditioning clip on the GPU (csrc/preprocess.hip through scripts/evaluation/inference.py preprocess_launch) against
Pillow's Image.resize on one host core of the same box, and against the byte floor.

Per case (3024x4032 -> 576x1024 and 1024x1024 -> 256x256, 16 frames; the image is uniform noise from seed 1):
  launches_us        the one or two launches, HIP events around --iters back-to-back repetitions, median of --runs, per repetition
  per_kernel_us      the same split by launch (ops.Tracer, a run of its own)
  upload_launch_us   host wall clock: the decoded uint8 image from pageable host memory to the device, the launches, a synchronise
  pillow_resize_us   Image.resize(BILINEAR) alone on the host (Pillow does not thread); crop / ToTensor / Normalize not included
  floor_us           the source read once plus the fp32 clip written once, at --hbm-tbps (default 4.1 TB/s, the rate the
                     HBM-bound norm passes of the UNet sustain: DESIGN 3.5)
  equal_to_pillow    the clip's frame 0, read back as uint8, equals Pillow's resize + crop / pad in every pixel (at the timed size)

usage: python tools/preprocess_ab.py [--runs 7] [--iters 20] [--frames 16] [--hbm-tbps 4.1] [--out FILE]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [((3024, 4032), (576, 1024)), ((1024, 1024), (256, 256))]


def measure(hw, vs, frames, runs, iters, tbps):
    from PIL import Image
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.scripts.evaluation import inference as I
    from tests import preprocess_restatement as R
    dev = torch.device("cuda:0")
    a = np.random.default_rng(1).integers(0, 256, size=hw + (3,), dtype=np.uint8)
    plan = I.preprocess_plan(hw[0], hw[1], vs, dev)
    g = plan.geometry
    src = torch.from_numpy(a).to(dev)
    ws = torch.empty(max(plan.workspace_bytes, 1), dtype=torch.uint8, device=dev)
    out = torch.empty((3, frames) + vs, dtype=torch.float32, device=dev)
    go = lambda: I.preprocess_launch(plan, src, out, ws, 0, frames)
    for _ in range(3):
        go()
    torch.cuda.synchronize()
    # correctness at the timed size
    got = torch.round((out[:, 0].double() + 1.0) * 127.5).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    pil = lambda x, oh, ow: np.asarray(Image.fromarray(x).resize((ow, oh), Image.BILINEAR))
    equal = bool((got == R.transform_u8(a, vs, resize_fn=pil)).all())
    per_iter = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            go()
        e1.record()
        torch.cuda.synchronize()
        per_iter.append(e0.elapsed_time(e1) * 1000.0 / iters)
    with ops.Tracer() as tr:
        for _ in range(iters):
            go()
    torch.cuda.synchronize()
    kern = {k: round(v["ms"] * 1000.0 / v["launches"], 2) for k, v in tr.summary().items()}
    wall = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = torch.from_numpy(a).to(dev)
        I.preprocess_launch(plan, s, out, ws, 0, frames)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
    img = Image.fromarray(a)
    pil_t = []
    for _ in range(max(3, runs // 2)):
        t0 = time.perf_counter()
        img.resize((g.rw, g.rh), Image.BILINEAR)
        pil_t.append((time.perf_counter() - t0) * 1e6)
    nbytes = a.size + out.numel() * 4
    return {
        "image": list(hw), "video_size": list(vs), "frames": frames, "resized": [g.rh, g.rw],
        "passes": (["horizontal"] if plan.tab_x is not None else []) + (["vertical"] if plan.tab_y is not None else []),
        "intermediate_bytes": plan.workspace_bytes, "taps": [plan.tab_x.ksize if plan.tab_x else 0, plan.tab_y.ksize if plan.tab_y else 0],
        "equal_to_pillow": equal,
        "launches_us": round(statistics.median(per_iter), 2), "launches_us_runs": [round(v, 2) for v in per_iter],
        "per_kernel_us": kern,
        "upload_launch_us": round(statistics.median(wall), 1), "upload_launch_us_runs": [round(v, 1) for v in wall],
        "pillow_resize_us": round(statistics.median(pil_t), 1), "pillow_resize_us_runs": [round(v, 1) for v in pil_t],
        "floor_bytes": int(nbytes), "floor_us": round(nbytes / (tbps * 1e12) * 1e6, 2),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--hbm-tbps", type=float, default=4.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_ab.py measures on the GPU; none found")
    res = {"tool": "preprocess_ab", "device": torch.cuda.get_device_name(0), "version": "direct (no LDS staging)",
           "hbm_tbps": args.hbm_tbps, "iters": args.iters,
           "cases": [measure(hw, vs, args.frames, args.runs, args.iters, args.hbm_tbps) for hw, vs in CASES]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

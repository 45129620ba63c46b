"""Inputs and bounds shared by tests/test_mjpeg_decode_cpu.py and tests/test_mjpeg_decode_gpu.py: the frames, the files Pillow
(libjpeg) and the encoder restatement write from them, and the measured distance of the float64 decoder restatement from libjpeg.

Frames are jpeg_restatement.make_frames "noise" and "smooth" (np.random.default_rng(1)) at 16x16 (one 4:2:0 MCU), 24x40 and
37x53 (odd both ways: a chroma plane of 19 x 27 real samples inside 24 x 32 padded ones; more than one MCU row and column in
every sampling)."""
import functools
import io
import itertools

import numpy as np
from PIL import Image

from tests import jpeg_restatement as J

SIZES = [(16, 16), (24, 40), (37, 53)]
KINDS = ["noise", "smooth"]
QUALITIES = (50, 90, 100)
# The float64 restatement against libjpeg (Pillow), measured on the CPU over every file of the mode below (qualities 50, 90,
# 100): (largest difference in levels, largest share of a file's samples that differ by more than 1). The differences are
# libjpeg's integer arithmetic: its 13-bit fixed-point IDCT, the (3 a + b + 8) >> 4 rounding inside its upsampler and its
# 16-bit fixed-point colour tables. Grey has neither upsampling nor colour conversion: what is left is the IDCT.
#   4:4:4  max 3, 1.04 %     4:2:2  max 3, 1.04 %     4:2:0  max 3, 1.17 %     grey  max 1, 0 %
MEASURED = {0: (3, 0.010417), 1: (3, 0.010417), 2: (3, 0.011719), "L": (1, 0.0)}
LIBJPEG_BOUND = {m: (mx + 1, 2 * share) for m, (mx, share) in MEASURED.items()}


@functools.lru_cache(maxsize=None)
def frames(kind, hw, T=1):
    f = J.make_frames(kind, T, hw[0], hw[1], np.random.default_rng(1))
    f.setflags(write=False)
    return f


def pillow_file(frame, mode, quality=90, optimize=False, rst=None, **kw):
    """mode: Pillow's `subsampling` 0 (4:4:4), 1 (4:2:2), 2 (4:2:0), or "L" (grey)."""
    im = Image.fromarray(np.asarray(frame))
    if mode == "L":
        im = im.convert("L")
    else:
        kw["subsampling"] = mode
    if rst:
        kw["restart_marker_blocks"] = rst
    b = io.BytesIO()
    im.save(b, "JPEG", quality=quality, optimize=optimize, **kw)
    return b.getvalue()


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def libjpeg_distance(got, ref):
    d = np.abs(np.asarray(got).astype(np.int32) - np.asarray(ref).astype(np.int32))
    return int(d.max()), float((d > 1).mean())


def pixel_batches(mode):
    """[((h, w), [files of that size])] for the pixel tests of `mode`: per size both kinds of frame at qualities 50, 90 and 100
    from Pillow - q 50 with a restart interval of one MCU row, q 90 with optimised Huffman tables, q 100 plain - so that one
    batch mixes tables and segment counts; 4:2:0 adds the encoder restatement's files at a restart interval of 3 MCUs."""
    out = []
    for hw in SIZES:
        files = []
        for kind, q in itertools.product(KINDS, QUALITIES):
            files.append(pillow_file(frames(kind, hw)[0], mode, q, optimize=q == 90, rst=1 if q == 50 else None))
            if mode == 2:
                files.append(J.encode(frames(kind, hw), q, ri=3)[0])
        out.append((hw, files))
    return out

"""Time of the segmentation behind the automatic bounding box: one device-resident float32
image (low background, one bright ellipsoid, beads) through spim_segment_bounds at radii 3, 12
and 50, at 512 x 512 x 256 and 768^3; the pieces alone (min / max, the filter with its image
written, the thresholded box); and in the same run
  * a device-to-device copy of the same buffer (the ceiling: one read, one write), and
  * the same chain in plain torch on the same GPU: amin / amax, per axis a zero F.pad and
    -max_pool3d(-x) (which is not Math.min: NaN and -0 are not the reference's), the box from a
    mask.  The torch box must equal the library's.

    python tools/autobbox_bench.py [--reps 10] [--warmup 2] [--shape Z Y X] [--out profiles/autobbox_bench.json]

The library calls return after their stream has drained, so each timed call is bracketed by
two HIP events on the caller's stream (the wall clock of the same calls is reported too).
Traffic the library's chain needs as built: min / max reads the image (4 N bytes), the x and y
passes read and write it (16 N), the z pass reads it (4 N, + 4 N when the filtered image is
asked for): 24 N against the copy's 8 N.  Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.dom_bench import timed  # noqa: E402

SHAPES = [(256, 512, 512), (768, 768, 768)]      # [z, y, x]
RADII = [3, 12, 50]
BACKGROUND = 5.0


def scene(shape, device):
    """background <= 1 %, an ellipsoid filling the middle half at >= 60 %, 2000 beads of 3^3"""
    import torch
    g = torch.Generator(device=device).manual_seed(7)
    img = torch.rand(shape, generator=g, device=device, dtype=torch.float32) * 0.01
    ax = [torch.arange(n, device=device, dtype=torch.float32) for n in shape]
    d = sum((((a - (n - 1) / 2) / (n / 4)) ** 2).reshape([-1 if i == j else 1 for j in range(3)])
            for i, (a, n) in enumerate(zip(ax, shape)))
    img = torch.where(d <= 1.0, 0.6 + 0.4 * torch.rand(shape, generator=g, device=device), img)
    rng = np.random.default_rng(3)
    for _ in range(2000):
        z, y, x = (int(rng.integers(1, n - 2)) for n in shape)
        img[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2] = 1.0
    return img.contiguous()


def torch_chain(img, radius, background):
    """(min, max, filtered, bounds_min, bounds_max, found) with torch operators"""
    import torch
    import torch.nn.functional as F
    mn, mx = img.amin(), img.amax()
    thr = (mx - mn).double() * (background / 100.0) + mn.double()
    x = img[None, None]
    k = 2 * radius + 1
    for pad, ks in (((radius, radius, 0, 0, 0, 0), (1, 1, k)), ((0, 0, radius, radius, 0, 0), (1, k, 1)),
                    ((0, 0, 0, 0, radius, radius), (k, 1, 1))):
        x = -F.max_pool3d(-F.pad(x, pad), ks, stride=1)
    filt = x[0, 0]
    mask = filt.double() > thr
    lo, hi = [], []
    for a, keep in ((2, (0, 1)), (1, (0, 2)), (0, (1, 2))):       # x, y, z
        idx = torch.nonzero(mask.any(dim=keep[1]).any(dim=keep[0]))
        found = idx.numel() > 0
        lo.append(int(idx.min()) if found else img.shape[a])
        hi.append(int(idx.max()) if found else 0)
    return float(mn), float(mx), filt, tuple(lo), tuple(hi), found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shape", type=int, nargs=3, metavar=("Z", "Y", "X"), default=None,
                    help="one image of this shape instead of the two standard ones (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "autobbox_bench.json"))
    a = ap.parse_args()
    import torch  # before the library loads: one shared HIP runtime (_lib.load)
    from spim_registration_amd import _lib, boundingbox as bb
    lib = _lib.load()
    if _lib.num_devices() < 1:
        raise SystemExit("autobbox_bench needs a GPU")
    dev = "cuda:0"
    stat = lambda v: {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3),
                      "max": round(float(np.max(v)), 3)}
    med = lambda v: float(np.median(v))
    cases = []
    for shape in ([tuple(a.shape)] if a.shape else SHAPES):
        img = scene(shape, dev)
        n = img.numel()
        dims = (C.c_int64 * 3)(shape[2], shape[1], shape[0])
        other = torch.empty_like(img)
        ptr = C.c_void_p(img.data_ptr())
        copy_ev, _ = timed(lambda: other.copy_(img), a.reps, a.warmup)
        mn, mx = C.c_float(), C.c_float()
        mm_ev, _ = timed(lambda: _lib.check(lib.spim_min_max(ptr, dims, 0, C.byref(mn), C.byref(mx))), a.reps,
                         a.warmup)
        lo, hi, found = (C.c_int64 * 3)(), (C.c_int64 * 3)(), C.c_int32()
        tb_ev, _ = timed(lambda: _lib.check(lib.spim_threshold_bounds(ptr, dims, 0.05, 0, lo, hi, C.byref(found))),
                         a.reps, a.warmup)
        case = {"shape_zyx": list(shape), "voxels": n, "copy_ms": stat(copy_ev),
                "copy_TBps": round(8.0 * n / (med(copy_ev) * 1e-3) / 1e12, 3),
                "min_max_ms": stat(mm_ev), "threshold_bounds_ms": stat(tb_ev), "radii": []}
        for r in RADII:
            res = _lib.SegmentResult()

            def run_seg():
                _lib.check(lib.spim_segment_bounds(ptr, dims, BACKGROUND, r, 0, None, C.byref(res)))

            def run_seg_img():
                _lib.check(lib.spim_segment_bounds(ptr, dims, BACKGROUND, r, 0, C.c_void_p(other.data_ptr()),
                                                   C.byref(res)))

            def run_filter():
                _lib.check(lib.spim_min_filter(ptr, dims, r, 0, C.c_void_p(other.data_ptr())))
            seg_ev, seg_wall = timed(run_seg, a.reps, a.warmup)
            box = (tuple(res.bounds_min), tuple(res.bounds_max), bool(res.found))
            segi_ev, _ = timed(run_seg_img, a.reps, a.warmup)
            flt_ev, _ = timed(run_filter, a.reps, a.warmup)
            filt_lib = other.clone()
            tor_ev, _ = timed(lambda: torch_chain(img, r, BACKGROUND), max(2, a.reps // 2), 1)
            tmn, tmx, tfilt, tlo, thi, tfound = torch_chain(img, r, BACKGROUND)
            assert (tlo, thi, tfound) == box, ("torch chain and library disagree", shape, r, (tlo, thi, tfound), box)
            assert (tmn, tmx) == (float(res.min), float(res.max))
            same = bool(torch.equal(tfilt, filt_lib))      # (values; this image has no NaN and no -0)
            del tfilt, filt_lib
            torch.cuda.empty_cache()
            case["radii"].append({
                "radius": r, "bounds_min": list(box[0]), "bounds_max": list(box[1]), "found": box[2],
                "segment_bounds_ms": stat(seg_ev), "segment_bounds_wall_ms": stat(seg_wall),
                "segment_bounds_with_image_ms": stat(segi_ev), "min_filter_ms": stat(flt_ev),
                "torch_chain_ms": stat(tor_ev),
                "speedup_over_torch_chain": round(med(tor_ev) / med(seg_ev), 2),
                "copy_over_segment_bounds": round(med(copy_ev) / med(seg_ev), 3),
                "traffic_as_built_TBps": round(24.0 * n / (med(seg_ev) * 1e-3) / 1e12, 3),
                "torch_filtered_image_equal": same,
            })
        cases.append(case)
        del img, other
        bb.release_workspace(0)
        torch.cuda.empty_cache()
    res = {"workload": "spim_segment_bounds on one device-resident float32 image: background <= 1 %, an ellipsoid "
                       ">= 60 %, 2000 beads; whole calls (min / max, threshold, x / y / z minimum filter, box)",
           "reps": a.reps, "warmup": a.warmup, "background_percent": BACKGROUND, "cases": cases}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

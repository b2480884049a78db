"""Downsampling time: one device-resident view of 768^3 synthetic beads (camera counts)
through spim_downsample at the factors (2,2,1), (4,4,1), (8,8,1) and (4,4,2), each beside the
same chain done level by level with plain torch slicing on the same GPU (a naive port: float32
arithmetic, one full pass over HBM per level; not bit-exact, not the bar), and the DoG pass
(spim_dog_interest_points at its defaults) on the view downsampled 2x in xy against the
full-resolution one.

    python tools/downsample_bench.py [--size 768] [--reps 20] [--warmup 3] [--out profiles/downsample_bench.json]

The library calls return after their stream has drained, so each timed call is bracketed by
two HIP events on the caller's stream (the wall clock of the same calls is reported too).
Compulsory traffic of a factor: the view read once and the result written once,
4 N (1 + 1 / (fx fy fz)) bytes; its rate is given as a share of the float4 copy kernel's
5.92 TB/s on this GPU (k_copy2).  Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.dom_bench import beads, timed  # noqa: E402

COPY_CEILING_TBPS = 5.92
FACTORS = [(2, 2, 1), (4, 4, 1), (8, 8, 1), (4, 4, 2)]


def torch_level(a, axis):
    """one simple2x level along ``axis`` with torch slicing (float32)"""
    a = a.movedim(axis, -1)
    m = a.shape[-1] // 2
    first = (a[..., 0] + a[..., 1] * 0.5) / 1.5
    mid = (a[..., 1:2 * m - 4:2] * 0.5 + a[..., 2:2 * m - 3:2] + a[..., 3:2 * m - 2:2] * 0.5) / 2.0
    last = (a[..., 2 * m - 2] + a[..., 2 * m - 3] * 0.5) / 1.5
    import torch
    return torch.cat([first[..., None], mid, last[..., None]], dim=-1).movedim(-1, axis).contiguous()


def torch_chain(a, factor):
    for axis, f in ((2, factor[0]), (1, factor[1]), (0, factor[2])):
        while f > 1:
            a = torch_level(a, axis)
            f //= 2
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--beads", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "downsample_bench.json"))
    a = ap.parse_args()
    import torch  # before the library loads: one shared HIP runtime (_lib.load)
    from spim_registration_amd import _lib, dog, downsample as ds
    lib = _lib.load()
    dimg = torch.from_numpy(beads(a.size, a.beads)).to("cuda:0")
    n = a.size ** 3
    dims = (C.c_int64 * 3)(a.size, a.size, a.size)
    stat = lambda v: {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3),
                      "max": round(float(np.max(v)), 3)}
    per_factor = []
    for factor in FACTORS:
        shape = ds.out_dims((a.size,) * 3, factor[0], factor[2])
        out = torch.empty(shape, dtype=torch.float32, device="cuda:0")
        f = (C.c_int32 * 3)(*factor)

        def run_lib():
            _lib.check(lib.spim_downsample(C.c_void_p(dimg.data_ptr()), dims, f, 0, C.c_void_p(out.data_ptr())))

        def run_torch():
            torch_chain(dimg, factor)
        ev, wall = timed(run_lib, a.reps, a.warmup)
        tev, _ = timed(run_torch, a.reps, a.warmup)
        ref = torch_chain(dimg, factor)
        nbytes = 4.0 * n * (1.0 + 1.0 / (factor[0] * factor[1] * factor[2]))
        tbps = nbytes / (np.median(ev) * 1e-3) / 1e12
        per_factor.append({
            "factor_xyz": list(factor), "out_shape_zyx": list(shape),
            "ms": stat(ev), "ms_wall": stat(wall), "compulsory_GB": round(nbytes / 1e9, 3),
            "TBps": round(float(tbps), 3), "share_of_copy_ceiling": round(float(tbps / COPY_CEILING_TBPS), 3),
            "torch_per_level_ms": stat(tev),
            "speedup_over_torch_per_level": round(float(np.median(tev) / np.median(ev)), 2),
            "max_abs_diff_to_torch_float32": float((out - ref).abs().max()),
        })
        del out, ref
    torch.cuda.empty_cache()
    counts = {}

    def run_full():
        counts["full"] = len(dog.interest_points_array(dimg)[0])

    def run_ds2():
        counts["ds2"] = len(dog.interest_points_array(dimg, downsample_xy=2)[0])
    full_ev, _ = timed(run_full, a.reps, a.warmup)
    ds2_ev, _ = timed(run_ds2, a.reps, a.warmup)
    res = {
        "workload": f"one device-resident {a.size}^3 float32 view, {a.beads} synthetic beads (camera counts); "
                    "spim_downsample whole calls (device in, device out)",
        "reps": a.reps, "warmup": a.warmup, "copy_ceiling_TBps": COPY_CEILING_TBPS,
        "downsample": per_factor,
        "dog_full_resolution_ms": stat(full_ev), "dog_full_resolution_points": counts["full"],
        "dog_downsample_xy2_ms": stat(ds2_ev), "dog_downsample_xy2_points": counts["ds2"],
        "dog_params": "sigma 1.8, threshold 0.008, localization 0; downsample_xy=2 includes the downsampling",
    }
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

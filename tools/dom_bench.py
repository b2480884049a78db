"""Difference-of-Mean bead detection time: one device-resident view of 768^3 synthetic
beads (camera counts) through spim_dom_interest_points at the reference's defaults (radii
2 / 3, threshold 0.02, no localisation), with the DoG pass of the same run on the same
view (spim_dog_interest_points at its defaults) beside it.

    python tools/dom_bench.py [--size 768] [--reps 20] [--warmup 3] [--out profiles/dom_bench.json]

Both calls return after their stream has drained, so each timed call is bracketed by two
HIP events on the caller's stream (the wall clock of the same calls is reported too).
Prints one JSON line and writes it to --out.
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


def beads(n: int, count: int, seed: int = 20140611) -> np.ndarray:
    """background 100 counts, 3x3x3 blobs of up to 4000 counts"""
    rng = np.random.default_rng(seed)
    img = np.full((n, n, n), 100.0, np.float32)
    pos = rng.integers(4, n - 4, size=(count, 3))
    amp = rng.uniform(2000.0, 4000.0, size=count).astype(np.float32)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                w = np.float32(np.exp(-0.9 * (dx * dx + dy * dy + dz * dz)))
                np.add.at(img, (pos[:, 0] + dz, pos[:, 1] + dy, pos[:, 2] + dx), amp * w)
    return img


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return ev, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--beads", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dom_bench.json"))
    a = ap.parse_args()
    import torch  # before the library loads: one shared HIP runtime (_lib.load)
    from spim_registration_amd import _lib
    lib = _lib.load()
    dimg = torch.from_numpy(beads(a.size, a.beads)).to("cuda:0")
    fp = C.POINTER(C.c_float)
    iptr = C.cast(C.c_void_p(dimg.data_ptr()), fp)
    dims = (C.c_int64 * 3)(a.size, a.size, a.size)
    cap = 1 << 20
    out = (_lib.InterestPointC * cap)()
    nout = C.c_int64(0)
    pm = _lib.DomParams()
    lib.spim_dom_params_default(C.byref(pm))
    pg = _lib.DogParams()
    lib.spim_dog_params_default(C.byref(pg))
    counts = {}

    def run_dom():
        _lib.check(lib.spim_dom_interest_points(iptr, dims, C.byref(pm), None, out, cap, C.byref(nout)))
        counts["dom"] = int(nout.value)

    def run_dog():
        _lib.check(lib.spim_dog_interest_points(iptr, dims, C.byref(pg), None, out, cap, C.byref(nout)))
        counts["dog"] = int(nout.value)
    dom_ev, dom_wall = timed(run_dom, a.reps, a.warmup)
    dog_ev, dog_wall = timed(run_dog, a.reps, a.warmup)
    n = a.size ** 3
    stat = lambda v: {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3),
                      "max": round(float(np.max(v)), 3)}
    res = {
        "workload": f"one device-resident {a.size}^3 view, {a.beads} synthetic beads (camera counts); whole "
                    "calls (min / max, image, peaks, sort, points out), localization 0",
        "reps": a.reps, "warmup": a.warmup,
        "dom_ms": stat(dom_ev), "dom_ms_wall": stat(dom_wall), "dom_interest_points": counts["dom"],
        "dom_params": "radius 2 / 3 (boxes 5 / 7), threshold 0.02",
        "dog_ms": stat(dog_ev), "dog_ms_wall": stat(dog_wall), "dog_interest_points": counts["dog"],
        "dog_params": "sigma 1.8, threshold 0.008",
        "dom_Gvoxels_per_s": round(n / np.median(dom_ev) / 1e6, 2),
        "compulsory_traffic_ms_at_8TBps": round(n * 8 / 8e12 * 1e3, 3),
    }
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

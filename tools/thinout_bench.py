"""Thin-out time: one ``spim_nn_distances`` call and a whole ``thinout.thin_out`` call on a
device-resident list of 2,000 / 16,000 / 160,000 detections, beside the same search in torch
float64 on the same GPU, the host time of ``scipy.spatial.cKDTree`` build plus query (k = 2: the
reference's algorithm, ThinOut_Detections.java:119-139) where scipy is importable, and the
fp64 VALU model of the pair kernel.

    python tools/thinout_bench.py [--sizes 2000 16000 160000] [--reps 15] [--warmup 3]
                                  [--out profiles/thinout_bench.json]

The list holds clustered and sparse detections at the bead density of a C4 view (20,000 per
768^3), a tenth of them in clumps of sigma 1.5 px, voxel size (0.73, 0.73, 2.0).  Each call
returns after its stream has drained and its results are on the host; a timed call is bracketed
by two HIP events on the caller's stream (wall clock beside it); the median and the spread (min,
max) over --reps are reported, 3 reps for the torch and host yardsticks above 20,000 points.  A
whole spim_nn_distances call holds the finite check, the scaling, the self-join, the merge and
the copies of dist / nearest to the host; thin_out adds the compaction, the copy of the kept
indices and the gather of the kept points on the device.  The torch yardstick: ``torch.cdist``
(no matrix-multiply shortcut) of row chunks of 1024 (64 above 16,000 points) against the whole
scaled list, the diagonal set to +inf, ``min`` per row (not bit-exact: no rule for the order of
the sum; the largest difference to it and to the kd-tree's distances is reported).  The model: the
pairs times the 8 non-fused fp64 VALU operations of a pair (3 subtractions, 3 products, 2 sums;
the comparison and the selects not counted) over the device's fp64 vector rate without FMA:
78.6 TFLOP/s counts an FMA as two, so 39.3e12 operations per second (MI355X data sheet).
Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_VECTOR_OPS_PER_S = 39.3e12      # 78.6 TFLOP/s peak fp64 vector, an FMA counted as two
OPS_PER_PAIR = 8
VOXEL = (0.73, 0.73, 2.0)


def detections(n: int, seed: int = 20140611, box: float = 768.0):
    rng = np.random.default_rng(seed + n)
    side = box * (n / 20000.0) ** (1.0 / 3.0)
    ncl = n // 10
    centres = rng.uniform(0.0, side, (max(ncl // 8, 1), 3))
    clumps = centres[rng.integers(0, len(centres), ncl)] + rng.normal(0.0, 1.5, (ncl, 3))
    pts = np.concatenate([clumps, rng.uniform(0.0, side, (n - ncl, 3))])
    return np.ascontiguousarray(pts[rng.permutation(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 16000, 160000])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thinout_bench.json"))
    a = ap.parse_args()
    import torch  # before the library loads: one shared HIP runtime (_lib.load)
    from spim_registration_amd import thinout
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out

    r3 = lambda x: round(float(x), 3)

    def stats(fn, reps):
        for _ in range(a.warmup):
            timed(fn)
        runs = [timed(fn) for _ in range(reps)]
        ev, wall = [r[0] for r in runs], [r[1] for r in runs]
        return ({"median": r3(np.median(ev)), "min": r3(min(ev)), "max": r3(max(ev)),
                 "wall_median": r3(np.median(wall))}, runs[-1][2])

    def host_stats(fn, reps):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return {"median": r3(np.median(t)), "min": r3(min(t)), "max": r3(max(t))}

    rows = []
    for n in a.sizes:
        hp = detections(n)
        dp = torch.from_numpy(hp).to("cuda:0")
        few = a.reps if n <= 20000 else 3
        nn_ms, (dist, _) = stats(lambda: thinout.nn_distances(dp, VOXEL), a.reps)
        to_ms, kept = stats(lambda: thinout.thin_out(dp, VOXEL, 0.0, 5.0), a.reps)
        vox = torch.tensor(VOXEL, dtype=torch.float64, device="cuda:0")

        # (the direct cdist kernel runs one block per output element: 64 rows at a time keep a
        # chunk against 160,000 columns below the 2^32 threads of one launch)
        def torch_nn(chunk=1024 if n <= 16000 else 64):
            c = dp * vox
            out = torch.empty(n, dtype=torch.float64, device="cuda:0")
            for i0 in range(0, n, chunk):
                d = torch.cdist(c[i0:i0 + chunk], c, compute_mode="donot_use_mm_for_euclid_dist")
                r = torch.arange(d.shape[0], device="cuda:0")
                d[r, i0 + r] = float("inf")
                out[i0:i0 + chunk] = d.min(dim=1).values
            return out.cpu().numpy()

        torch_ms, tdist = stats(torch_nn, few)
        pairs = n * n
        model_ms = pairs * OPS_PER_PAIR / FP64_VECTOR_OPS_PER_S * 1e3
        row = {
            "points": n, "pairs": pairs,
            "nn_distances_call_ms": nn_ms, "thin_out_call_ms": to_ms, "thin_out_kept": int(len(kept)),
            "median_nn_distance": r3(np.median(dist)),
            "nn_pairs_per_s_whole_call": r3(pairs / (nn_ms["median"] * 1e-3) / 1e9),
            "torch_fp64_cdist_min_ms": torch_ms,
            "torch_max_abs_difference": float(np.abs(tdist - dist).max()),
            "ratio_torch_over_nn_distances": r3(torch_ms["median"] / nn_ms["median"]),
            "fp64_valu_model_ms": r3(model_ms),
            "fraction_of_fp64_valu_model": r3(model_ms / nn_ms["median"]),
        }
        if cKDTree is not None:
            hc = hp * np.asarray(VOXEL)
            kd_ms = host_stats(lambda: cKDTree(hc).query(hc, k=2), few)
            row["ckdtree_max_abs_difference"] = float(np.abs(cKDTree(hc).query(hc, k=2)[0][:, 1] - dist).max())
            row["host_ckdtree_build_query_ms"] = kd_ms
            row["ratio_ckdtree_over_nn_distances"] = r3(kd_ms["median"] / nn_ms["median"])
        rows.append(row)
        print(f"[thinout_bench] {n} points done", file=sys.stderr, flush=True)
    res = {
        "workload": "one device-resident list per size: a tenth of the detections in clumps of sigma 1.5 px, the "
                    "rest uniform at 20,000 per 768^3, voxel size (0.73, 0.73, 2.0); whole C-ABI calls, results to "
                    "the host; thin_out removes the range [0, 5] and gathers the kept points on the device",
        "reps": a.reps, "warmup": a.warmup,
        "timing": "median (min, max) of HIP event pairs around each call, ms; wall median beside it; the host "
                  "kd-tree by perf_counter on this machine's CPU, one thread; 3 reps for the torch and host "
                  "yardsticks above 20,000 points",
        "yardstick_torch": "float64 on the same GPU: torch.cdist (donot_use_mm_for_euclid_dist) of row chunks of "
                           "1024 (64 above 16,000 points) against the whole scaled list, the diagonal set to +inf, min per row",
        "yardstick_host": "scipy.spatial.cKDTree(scaled).query(scaled, k=2)" if cKDTree is not None else
                          "scipy is not importable on this machine: no host kd-tree number",
        "yardstick_model": f"pairs x {OPS_PER_PAIR} non-fused fp64 VALU operations / {FP64_VECTOR_OPS_PER_S:.3g} "
                           "per second (78.6 TFLOP/s fp64 vector with an FMA counted as two)",
        "nn_pairs_per_s_unit": "1e9 ordered pairs per second",
        "tiles": list(thinout.tile_sizes()),
        "device": torch.cuda.get_device_name(0),
        "sizes": rows,
    }
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

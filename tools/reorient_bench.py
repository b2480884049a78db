"""Reorienting bounding box time: ``farthest_pair`` alone, one 27-matrix ``axis_boxes`` launch
and a whole ``reorient_bounding_box`` call on device-resident world points, at N = 2,000 /
16,000 / 160,000 (160,000: the 8 x 20,000 detections of a C4 timepoint), beside two yardsticks.

    python tools/reorient_bench.py [--sizes 2000 16000 160000] [--reps 15] [--warmup 3]
                                   [--out profiles/reorient_bench.json]

The points fill a 700 x 160 x 90 cuboid turned off the axes (tests/reorient_ref.py's scene at a
C4 volume's scale).  Each call returns after its stream has drained and its results are on the
host; a timed call is bracketed by two HIP events on the caller's stream (wall clock beside
it); the median and the spread (min, max) over --reps are reported.  Every size runs in a child
process of its own under a time limit; a child that fails ends the run.

Yardstick 1: the same farthest-pair search with torch on the GPU in float64 -- row chunks
against all later columns, per-coordinate differences, squares, sums, a max and an argmax per
chunk (not bit-exact: no scan-order rule); at N = 2,000 also a NumPy brute force over the full
matrix on the host.  Yardstick 2: the pairs times the 9 non-fused fp64 VALU operations of a pair
(3 subtractions, 3 products, 2 sums, 1 comparison) over the device's fp64 vector rate without
FMA: 78.6 TFLOP/s counts an FMA as two, so 39.3e12 operations per second (MI355X data sheet).
Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_VECTOR_OPS_PER_S = 39.3e12      # 78.6 TFLOP/s peak fp64 vector, an FMA counted as two
OPS_PER_PAIR = 9
CHILD_LIMIT_S = {2000: 120, 16000: 150, 160000: 420}


def scene(n: int, seed: int = 20140611):
    rng = np.random.default_rng(seed + n)
    local = rng.uniform(0.0, 1.0, (n, 3)) * np.array([700.0, 160.0, 90.0])
    u = np.array([0.6, 0.5, -0.62]) / np.linalg.norm([0.6, 0.5, -0.62])
    k = np.cross([1.0, 0.0, 0.0], u)
    s, c = np.linalg.norm(k), u[0]
    k = k / s
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    rot = np.eye(3) + s * K + (1.0 - c) * (K @ K)
    return np.ascontiguousarray(local @ rot.T + [400.0, 380.0, 350.0])


def one_size(n: int, reps: int, warmup: int) -> dict:
    import torch  # before the library loads: one shared HIP runtime (_lib.load)
    from spim_registration_amd import boundingbox as bb

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

    def stats(fn, reps_):
        for _ in range(warmup):
            timed(fn)
        runs = [timed(fn) for _ in range(reps_)]
        ev, wall = [r[0] for r in runs], [r[1] for r in runs]
        return ({"median": r3(np.median(ev)), "min": r3(min(ev)), "max": r3(max(ev)),
                 "wall_median": r3(np.median(wall))}, runs[-1][2])

    hp = scene(n)
    dp = torch.from_numpy(hp).to("cuda:0")
    ident = [np.eye(3, 4)]
    far_ms, far = stats(lambda: bb.farthest_pair(dp), reps)
    mats = np.stack([np.eye(3, 4)] * 27)
    for k in range(27):       # 27 different rotations about z (any finite matrices cost the same)
        a = 0.01 * k
        mats[k, :2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    box_ms, _ = stats(lambda: bb.axis_boxes(dp, mats), reps)
    whole_ms, whole = stats(lambda: bb.reorient_bounding_box([dp], ident, return_details=True), reps)

    def torch_far(chunk=1024):
        best, bi, bj = -1.0, -1, -1
        for i0 in range(0, n, chunk):
            a, b = dp[i0:i0 + chunk], dp[i0:]
            d = (a[:, None, 0] - b[None, :, 0]) ** 2
            d += (a[:, None, 1] - b[None, :, 1]) ** 2
            d += (a[:, None, 2] - b[None, :, 2]) ** 2
            m, flat = torch.max(d.reshape(-1), 0)
            m, flat = float(m), int(flat)
            if m > best:
                best, bi, bj = m, i0 + flat // d.shape[1], i0 + flat % d.shape[1]
        return bi, bj, best

    torch_ms, tfar = stats(torch_far, 3 if n > 20000 else max(reps // 3, 3))
    assert tfar[2] == far[2], (tfar, far)     # the same largest distance (the pair may differ among ties)
    pairs = n * (n - 1) // 2
    model_ms = pairs * OPS_PER_PAIR / FP64_VECTOR_OPS_PER_S * 1e3
    row = {
        "points": n, "pairs": pairs,
        "farthest_pair_call_ms": far_ms, "farthest_pair": [far[0], far[1]], "farthest_d2": far[2],
        "axis_boxes_27_call_ms": box_ms,
        "reorient_call_ms": whole_ms, "reorient_min_volume": whole[4]["min_volume"],
        "reorient_start_volume": whole[4]["start_volume"], "reorient_bb_dims": list(whole[3]),
        "torch_fp64_farthest_pair_ms": torch_ms,
        "ratio_torch_over_farthest_pair": r3(torch_ms["median"] / far_ms["median"]),
        "fp64_valu_model_ms": r3(model_ms),
        "fraction_of_fp64_valu_model": r3(model_ms / far_ms["median"]),
        "farthest_pair_pairs_per_s_whole_call": r3(pairs / (far_ms["median"] * 1e-3) / 1e9),
    }
    if n <= 2000:
        def numpy_far():
            d = hp[:, None, :] - hp[None, :, :]
            d = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            return np.unravel_index(np.argmax(np.triu(d, 1)), d.shape), float(d.max())
        numpy_far()
        t = []
        for _ in range(max(reps // 3, 3)):
            t0 = time.perf_counter()
            (i, j), dm = numpy_far()
            t.append((time.perf_counter() - t0) * 1e3)
        assert dm == far[2]
        row["host_numpy_brute_force_ms"] = {"median": r3(np.median(t)), "min": r3(min(t)), "max": r3(max(t))}
        row["ratio_numpy_over_farthest_pair"] = r3(np.median(t) / far_ms["median"])
    row["device"] = torch.cuda.get_device_name(0)
    row["tile"] = bb.reorient_tile()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 16000, 160000])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reorient_bench.json"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("ROW " + json.dumps(one_size(a.child, a.reps, a.warmup)), flush=True)
        return
    rows = []
    for n in a.sizes:          # a fresh process per size, each under its own time limit
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(a.reps),
                            "--warmup", str(a.warmup)], capture_output=True, text=True,
                           timeout=CHILD_LIMIT_S.get(n, 420))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"size {n}: exit status {r.returncode}; nothing more is started")
        rows.append(json.loads(line[-1][4:]))
    res = {
        "workload": "device-resident world points that fill a 700 x 160 x 90 cuboid turned off the axes; whole "
                    "C-ABI calls, results to the host; the whole call is reorient_bounding_box on one list under "
                    "the identity (finite check, world points, farthest pair, 1 + 8 axis_boxes launches, host "
                    "search)",
        "reps": a.reps, "warmup": a.warmup,
        "timing": "median (min, max) of HIP event pairs around each call, ms; wall median beside it; the NumPy "
                  "brute force by perf_counter on this machine's CPU",
        "yardstick_torch": "float64 on the same GPU: row chunks of 1024 against all later columns, per-coordinate "
                           "differences squared and summed, max / argmax per chunk; 3 reps above 20,000 points",
        "yardstick_model": f"pairs x {OPS_PER_PAIR} non-fused fp64 VALU operations / {FP64_VECTOR_OPS_PER_S:.3g} "
                           "per second (78.6 TFLOP/s fp64 vector with an FMA counted as two)",
        "device": rows[0].pop("device"), "tile": rows[0].pop("tile"),
        "sizes": rows,
    }
    for r in rows[1:]:
        r.pop("device", None)
        r.pop("tile", None)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

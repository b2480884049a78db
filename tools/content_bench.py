"""Time of spim_content_based_weights on one device-resident view at the reference's
default sigmas (20 / 40 voxels: 121 and 241 taps per axis).  HIP events around the call
(it synchronises its own stream before it returns, so the events bracket all of its
device work plus its allocations); the host clock is printed beside them.

    python tools/content_bench.py [--size 768] [--reps 5] [--warmup 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sigma1", type=float, default=20.0)
    ap.add_argument("--sigma2", type=float, default=40.0)
    a = ap.parse_args()
    import torch
    from spim_registration_amd.input_prep import content_based_weights
    if not torch.cuda.is_available():
        raise SystemExit("content_bench needs a GPU (there is no CPU path to time)")
    n = a.size
    g = torch.Generator(device="cuda").manual_seed(11)
    img = torch.rand((n, n, n), device="cuda", generator=g)
    s1, s2 = (a.sigma1,) * 3, (a.sigma2,) * 3
    for _ in range(a.warmup):
        w = content_based_weights(img, s1, s2)
    ev_ms, host_ms = [], []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        w = content_based_weights(img, s1, s2)
        e1.record()
        e1.synchronize()
        host_ms.append(round((time.perf_counter() - t0) * 1e3, 2))
        ev_ms.append(round(e0.elapsed_time(e1), 2))
    taps = [2 * int(3 * s + 0.5) + 1 for s in (a.sigma1, a.sigma2)]
    fma = 3 * sum(taps) * n ** 3
    best = min(ev_ms)
    print(json.dumps({"workload": f"content-based weights, {n}^3 float32 on the device, sigma {a.sigma1} / {a.sigma2}",
                      "taps": taps, "event_ms": ev_ms, "host_ms": host_ms,
                      "fma_per_call": fma, "tflops_fp32_at_best": round(2 * fma / best / 1e9, 2),
                      "weights_min_max": [float(w.min()), float(w.max())]}))


if __name__ == "__main__":
    main()

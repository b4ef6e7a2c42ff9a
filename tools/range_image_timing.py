#!/usr/bin/env python
"""Time the range image from a raw point cloud on the device: rd_range_image_from_points (csrc/k_rangeimg.h) on 120 000-point scans at
64 x 2048, B = 1 and B = 8, points resident -- HIP events on the launch stream around regions of 20 calls, 5 warm-up regions, the median
of 30 regions -- next to the NumPy restatement of the reference's get_range_image (tests/range_image_model.py) on this box's host (wall
clock, median of 5, NumPy's own threading; the core count is printed).  Made-up 64-beam tables, seeded clouds; the B = 1 result is
compared with the restatement first.

    python tools/range_image_timing.py [--out profiles/range_image_timing.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import range_image_model as M  # noqa: E402
from rangedet_amd import lib as rdlib  # noqa: E402
from rangedet_amd.runtime import TorchAllocator  # noqa: E402

H, W, N, CALLS, WARM, REGIONS = 64, 2048, 120000, 20, 5, 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    import torch
    L, A = rdlib.get_lib(), TorchAllocator()
    incl = np.linspace(-0.034, 0.436, H) + 0.002 * np.sin(np.arange(H))
    height = 0.21 - 0.095 * np.arange(H) / H
    clouds = [M.synth_cloud(40 + i, N, incl, height, W) for i in range(8)]
    res = dict(shape=dict(H=H, W=W, points_per_scan=[len(c) for c in clouds]), row_search="plain: H double atan2 per point",
               method="HIP events around regions of %d calls, %d warm-up regions, median of %d regions; host: wall clock, median of 5"
                      % (CALLS, WARM, REGIONS), device=torch.cuda.get_device_name(0))
    for B in (1, 8):
        cs = clouds[:B]
        off = (ctypes.c_longlong * (B + 1))(*np.concatenate([[0], np.cumsum([len(c) for c in cs])]).tolist())
        pts = A.upload(np.concatenate(cs))
        n = B * H * W
        nws = L.raw("rd_range_image_workspace_bytes")(B, H, W)
        img, mask, idx, ws = A.alloc(n * 20), A.alloc(n), A.alloc(n * 4), A.alloc(nws)
        args = [A.ptr(pts), ctypes.addressof(off), B, incl.ctypes.data, height.ctypes.data, H, W, A.ptr(img), A.ptr(mask), A.ptr(idx),
                A.ptr(ws), nws, A.stream]
        ts = []
        for r in range(WARM + REGIONS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                L.call("rd_range_image_from_points", *args)
            e1.record()
            e1.synchronize()
            if r >= WARM:
                ts.append(e0.elapsed_time(e1) * 1e3 / CALLS / B)
        res["B%d_us_per_scan" % B] = float(np.median(ts))
        res["B%d_us_per_scan_min_max" % B] = [float(min(ts)), float(max(ts))]
        if B == 1:
            want = M.get_range_image(cs[0], incl, height, W)
            got = A.to_numpy(A.view_f32(img, (H, W, 5)))
            res["equals_restatement"] = bool(got.tobytes() == want.tobytes())
    hs = []
    for _ in range(5):
        t0 = time.perf_counter()
        M.get_range_image(clouds[0], incl, height, W)
        hs.append((time.perf_counter() - t0) * 1e6)
    res["numpy_restatement_us_per_scan"] = float(np.median(hs))
    res["host_cores"] = dict(os_cpu_count=os.cpu_count(), usable=len(os.sched_getaffinity(0)), OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS"))
    print(json.dumps(res, indent=1))
    if opt.out:
        with open(opt.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

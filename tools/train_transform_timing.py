#!/usr/bin/env python
"""Time the training-time input chain on the device: rd_train_transform (csrc/k_target.h) at B = 8, 64 x 2650 padded to 2656, 60
boxes per frame -- HIP events, 20 warm-up launches, the median of 100 -- next to what the package offered for the same records
before it: rd_input_transform plus the per-record Bbox3dAssigner path (host miss-value fill, upload, one launch, download; wall
clock, it is host work).  Prints both times and the achieved bytes/s against the compulsory traffic counted from the tensor shapes.

    python tools/train_transform_timing.py [--out profiles/train_transform_timing.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rangedet_amd import lib as rdlib, synth  # noqa: E402
from rangedet_amd.core import input as CI  # noqa: E402
from rangedet_amd.input_transform import DeviceInputTransform, DeviceTrainTransform, train_shapes  # noqa: E402
from rangedet_amd.runtime import TorchAllocator  # noqa: E402

B, H, W, HP, WP, M = 8, 64, 2650, 64, 2656, 60


def boxes(rec, rng):
    """M boxes (1 - 6 m per side, any yaw) centred on points of the record."""
    P = rec["pc_vehicle_frame"][rec["range_image"][..., 0] > 0]
    c = P[rng.integers(0, len(P), M)].astype(np.float64)
    lwh, yaw = rng.uniform(1.0, 6.0, (M, 3)), rng.uniform(-np.pi, np.pi, M)
    cor = np.array([[.5, -.5], [-.5, -.5], [-.5, .5], [.5, .5]])[None] * lwh[:, None, :2]
    rot = np.stack([np.stack([np.cos(yaw), -np.sin(yaw)], 1), np.stack([np.sin(yaw), np.cos(yaw)], 1)], 1)
    xy = np.einsum('mij,mkj->mki', rot, cor) + c[:, None, :2]
    z = [np.repeat((c[:, 2] + sg * lwh[:, 2] / 2)[:, None, None], 4, 1) for sg in (-1, 1)]
    imu = np.concatenate([np.concatenate([xy, z[0]], 2), np.concatenate([xy, z[1]], 2)], 1).astype(np.float32)
    return imu, np.concatenate([c, lwh, yaw[:, None]], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    import torch
    L, A = rdlib.get_lib(), TorchAllocator()
    rng = np.random.default_rng(0)
    recs = []
    for i in range(B):
        r = synth.raw_record(i, H, W)
        r["gt_bbox_imu"], r["gt_bbox_csa"] = boxes(r, rng)
        recs.append(r)
    train = DeviceTrainTransform(pad_hw=(HP, WP), lib=L, alloc=A, iou_pred_names=())
    out = train(recs)
    A.sync()
    inbox = int((out["bbox3d_ind"] >= 0).sum())
    args, keep_out, keep_in = train.prepare(recs)                        # the launches alone, on resident inputs

    def median_ms(fn, n_warm=20, n=100):
        for _ in range(n_warm):
            fn()
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))
    t_train = median_ms(lambda: L.call("rd_train_transform", *args))
    # before: rd_input_transform (events) + per-record assigner (wall clock: numpy fill, upload, launch, download)
    inp = DeviceInputTransform(pad_hw=(HP, WP), lib=L, alloc=A)
    names = ['input_data', 'coord_s1'] + ['%s_s%d' % (n, s) for n in ('pc_vehicle_frame', 'range_image_mask') for s in (1, 2, 4)]
    ia = args[:3] + [ctypes.addressof(inp.norm), B, H, W, HP, WP] + [A.ptr(keep_out[k]) for k in names] + [args[-1]]
    t_input = median_ms(lambda: L.call("rd_input_transform", *ia))
    asg = CI.Bbox3dAssigner(type("P", (), dict(feat_size=(H, W))))
    chain = [dict(r, **{CI._CHAIN: [("LoadRecord", {}), ("ProcessMissValue", {})]}) for r in recs]
    ts = []
    for _ in range(3):
        A.sync()
        t0 = time.perf_counter()
        for r in chain:
            r[CI._CHAIN] = r[CI._CHAIN][:2]
            asg.apply(r)
        ts.append((time.perf_counter() - t0) * 1e3)
    t_assign = float(np.median(ts))
    shapes = train_shapes(B, H, W, HP, WP)
    bytes_out = sum(int(np.prod(v)) * 4 for v in shapes.values())
    bytes_in = B * H * W * (4 + 3) * 4 + B * H * 4 + B * M * (24 + 3 + 7) * 4
    res = dict(shape=dict(B=B, H=H, W=W, Hp=HP, Wp=WP, boxes_per_frame=M), pixels_in_a_box=inbox,
               rd_train_transform_ms=t_train, compulsory_bytes=dict(read=bytes_in, written=bytes_out),
               rd_train_transform_GBps=(bytes_in + bytes_out) / t_train / 1e6,
               before=dict(rd_input_transform_ms=t_input, per_record_assigner_ms_wall=t_assign, targets="not available"),
               method="HIP events, 20 warm-up launches, median of 100; assigner path: wall clock, median of 3 passes over the batch",
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res, indent=1))
    if opt.out:
        with open(opt.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

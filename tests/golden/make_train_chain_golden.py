#!/usr/bin/env python
"""Golden vectors of the TRAINING-time transform chain, made by the REFERENCE'S OWN PYTHON (build container only: reads
/root/reference; nothing of it travels, the outputs are data).

train_chain_{0,1,2}.npz: the reference's own sixteen transform objects, in the order and with the parameter objects its
config builds for is_train=True (config/rangedet/rangedet_veh_wo_aug_4_18e.py:346-366; the loss-graph builder is stubbed, the
graph is not part of this pin), applied to three 8 x 62 records padded to 64: the raw inputs, the ground truth and every
tensor of data_name + label_name plus rpn_cls_target_s* and bbox3d_ind_of_each_pt.  Only the fixture's own size replaces the
config's (64, 2650) / (64, 2656) in the three objects that carry it.

Stand-ins (installer of make_ref_python_golden.py, plus two): processing_cxx.assign3D_v2 = oracle.assign3d_v2 and
processing_cxx.get_point_num = oracle.get_point_num -- the documented restatements of assigner.h, PARITY UNPINNED (the header needs
Eigen).  So the target arithmetic, the FPN masking, the padding and the name lists are the reference's own; the assignment and the
counts are the restatement's.

Records: the synthetic raw record of make_ref_python_golden.fixture_record (runs of missing returns plus one solid missing block;
that function divides by H - 8, so at H = 8 the block is placed at row 0 here) with its ranges remapped to a near-to-far sweep over
the columns (4 m .. 45 m, +-10 % from the record's own ranges): at 8 x 62 the synthetic ranges have about four pixels below 15 m and
neighbouring points metres apart, which leaves the stride-4 level and a 10 % box coverage out of reach of any box placement.
Boxes are centred on chosen pixels' points, 1 - 6 m per side, yaws over the full circle: frame 0 five, frame 1 thirty-seven,
frame 2 a single class-2 box that FilterGTClass([1]) replaces by the zero box.

    python tests/golden/make_train_chain_golden.py
"""
import importlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

H, W, WP = 8, 62, 64
NBOX = (5, 37, 1)
TARGETS = ["rpn_reg_target", "rpn_reg_weight", "reg_normalize_weight", "rpn_cls_target"]
OUT_KEYS = ["input_data", "coord_s1", "gt_bbox_veh_for_iou_pred"] + \
    ["%s_s%d" % (n, s) for n in ["pc_vehicle_frame", "range_image_mask"] + TARGETS for s in (1, 2, 4)]


def fixture_record(i):
    from rangedet_amd import synth
    rec = synth.raw_record(i, H=H, W=W)
    ri, incl, az = rec["range_image"], rec["inclination"], rec["azimuth"]
    valid = ri[..., 0] > 0
    r = ((4.0 + 41.0 * np.arange(W) / (W - 1))[None, :] * (0.9 + 0.2 * ri[..., 0] / 75.0)).astype(np.float32)
    pc = np.stack([r * np.cos(incl)[:, None] * np.cos(az)[None, :], r * np.cos(incl)[:, None] * np.sin(az)[None, :],
                   r * np.sin(incl)[:, None] + 2.0], 2).astype(np.float32)
    ri[..., 0][valid] = r[valid]
    rec["pc_vehicle_frame"][valid] = pc[valid]
    h0, w0 = 0, (17 + 40 * i) % (W - 12)                    # the solid block of make_ref_python_golden.fixture_record
    ri[h0:h0 + 7, w0:w0 + 11] = -1
    rec["pc_vehicle_frame"][h0:h0 + 7, w0:w0 + 11] = 0
    return rec


def box_arrays(ctr, lwh, yaw):
    """(M,3) centres, (M,3) l w h, (M,) yaw -> gt_bbox_imu (M,8,3) (A B C D bottom, E F G H top) and gt_bbox_csa (M,7)."""
    l, w, h = lwh[:, 0], lwh[:, 1], lwh[:, 2]
    cor = np.stack([np.stack([l / 2, -w / 2], 1), np.stack([-l / 2, -w / 2], 1), np.stack([-l / 2, w / 2], 1),
                    np.stack([l / 2, w / 2], 1)], 1)
    rot = np.stack([np.stack([np.cos(yaw), -np.sin(yaw)], 1), np.stack([np.sin(yaw), np.cos(yaw)], 1)], 1)
    xy = np.einsum('mij,mkj->mki', rot, cor) + ctr[:, None, :2]
    bot = np.concatenate([xy, np.repeat((ctr[:, 2] - h / 2)[:, None, None], 4, 1)], 2)
    top = np.concatenate([xy, np.repeat((ctr[:, 2] + h / 2)[:, None, None], 4, 1)], 2)
    return (np.concatenate([bot, top], 1).astype(np.float32),
            np.concatenate([ctr, lwh, yaw[:, None]], 1).astype(np.float32))


def post_fill_state(rec):
    """Points / mask / "took the right neighbour's values" per pixel after LoadRecord + ProcessMissValue (numpy, for placing boxes)."""
    ri, pc = rec["range_image"], rec["pc_vehicle_frame"].copy()
    miss = ri[..., 0] == -1
    nb = list(range(1, W)) + [0]
    src_valid = np.where(miss, ri[:, nb, 0] > 0, ri[..., 0] > 0)
    pc[miss] = pc[:, nb][miss]
    pc[~src_valid] = 0
    return pc.reshape(-1, 3), src_valid.reshape(-1), (miss & src_valid).reshape(-1)


def inside(P, c, lwh, yaw):
    d = P - c
    u = np.cos(yaw) * d[:, 0] + np.sin(yaw) * d[:, 1]
    v = -np.sin(yaw) * d[:, 0] + np.cos(yaw) * d[:, 1]
    return (np.abs(u) < lwh[0] / 2) & (np.abs(v) < lwh[1] / 2) & (np.abs(d[:, 2]) < lwh[2] / 2) & ((d ** 2).sum(1) <= 20)


def place_boxes(rec, n, seed):
    """n boxes centred on pixels' points.  The first centres are chosen for the fixture conditions (a filled missing return, the
    pixels around flat index 256, one box per range level); the rest greedily by the number of uncovered points they hold."""
    rng = np.random.default_rng(seed)
    P, valid, filled = post_fill_state(rec)
    rng_of = np.where(rec["range_image"][..., 0] == -1, np.roll(rec["range_image"][..., 0], -1, 1), rec["range_image"][..., 0]).reshape(-1)
    idx = np.arange(H * W)
    pools = [valid & filled, valid & (np.abs(idx - 256) <= 3), valid & (rng_of >= 32), valid & (rng_of >= 17) & (rng_of < 28),
             valid & (rng_of >= 32)]
    ctr, lwh, yaw = [], [], []
    cov = np.zeros(H * W, bool)
    for k in range(n):
        size = rng.uniform(5.5, 6.0, 3) if k < 5 else rng.uniform(1.0, 6.0, 3)
        ang = -np.pi + 2 * np.pi * ((k * 0.381966) % 1.0) + rng.uniform(-0.05, 0.05)
        pool = np.where(pools[k] if k < len(pools) and pools[k].any() else valid)[0]
        gains = [(inside(P, P[j], size, ang) & valid & ~cov).sum() for j in pool]
        j = pool[int(np.argmax(gains))]
        cov |= inside(P, P[j], size, ang) & valid
        ctr.append(P[j]); lwh.append(size); yaw.append(ang)
    return box_arrays(np.array(ctr, np.float64), np.array(lwh), np.array(yaw))


def fixture_conditions(g):
    """What a frame with boxes must show (asserted here before writing and again by tests/test_train_targets.py)."""
    ind = g["bbox3d_ind"].reshape(-1)
    ri = g["raw_range_image"][..., 0]
    miss = (ri == -1)
    src_valid = np.where(miss, np.roll(ri, -1, 1) > 0, ri > 0).reshape(-1)
    assert (ind[src_valid] >= 0).sum() >= 0.10 * src_valid.sum(), ("coverage", (ind >= 0).sum(), src_valid.sum())
    for s in (1, 2, 4):
        n = int((g["rpn_reg_weight_s%d" % s][0] != 0).sum())
        assert n >= 8, ("level", s, n)
    lo, hi = set(ind[:256][ind[:256] >= 0].tolist()), set(ind[256:][ind[256:] >= 0].tolist())
    assert lo & hi, "no box with points on both sides of flat index 256"
    assert (ind[(miss.reshape(-1)) & src_valid] >= 0).any(), "no in-box pixel that was filled from its right neighbour"


def main():
    REF = "/root/reference"
    if not os.path.isdir(REF):
        raise SystemExit("needs %s (build container only)" % REF)
    import make_ref_python_golden as G
    G.install_stand_ins()
    from oracle import cpu_ops as O
    pcx = sys.modules["processing_cxx"]
    # the reference passes a (64*2650, 1) no-label-zone array whatever the frame's size (input.py:294): all zeros, cut to N
    pcx.assign3D_v2 = lambda pc, bbox, ctr, rad, mask, nlz, *lim: O.assign3d_v2(pc, bbox, ctr, rad, mask, nlz[:len(pc)], *lim)
    pcx.get_point_num = O.get_point_num
    cfgmod = importlib.import_module("config.rangedet.rangedet_veh_wo_aug_4_18e")

    class NoLossGraph:                       # get_config(True) builds the loss graph at import (config:156-158): not part of this pin
        def __init__(self, *a, **k):
            pass

        def get_train_symbol(self, *a, **k):
            return None
    cfgmod.Detector = NoLossGraph
    cfg = cfgmod.get_config(True)
    transform, data_name, label_name = cfg[9], cfg[10], cfg[11]
    assert [type(t).__module__ for t in transform] == ["rangedet.core.input"] * 16
    assert sys.modules["rangedet.core.input"].__file__.startswith(REF)
    for t in transform:                      # the config's objects say (64, 2650) / (64, 2656): the fixture's own size
        n = type(t).__name__
        if n == "PadData":
            t.pad_short, t.pad_long = H, WP
        elif n == "Bbox3dAssigner":
            t.height, t.width = H, W
        elif n == "GenerateTarget":
            t.input_height, t.input_width = H, W
    gen = [t for t in transform if type(t).__name__ == "GenerateTarget"][0]
    params = dict(stage_names=np.array([type(t).__name__ for t in transform]), data_name=np.array(data_name),
                  label_name=np.array(label_name), reg_weight=np.array(gen.reg_weight, np.float32),
                  label_set=np.array(gen.label_set), num_classes=np.array(gen.num_classes))
    with tempfile.TemporaryDirectory() as td:
        for i in range(3):
            rec = fixture_record(i)
            imu, csa = place_boxes(rec, NBOX[i], seed=500 + i)
            M = len(imu)
            gt = dict(gt_class=np.full(M, 2.0 if i == 2 else 1.0), gt_bbox_imu=imu, gt_bbox_csa=csa, gt_bbox_yaw=csa[:, 6].copy(),
                      points_in_box=np.zeros(M), meta_data=np.zeros((M, 4)))
            path = os.path.join(td, "rec.npz")
            np.savez(path, **rec)
            r = dict(pc_url=path, **{k: v.copy() for k, v in gt.items()})
            for t in transform:
                t.apply(r)
            out = {k: np.asarray(r[k]) for k in OUT_KEYS}
            assert all(v.dtype == np.float32 for v in out.values()), {k: v.dtype for k, v in out.items()}
            g = dict(raw_range_image=rec["range_image"], raw_pc_vehicle_frame=rec["pc_vehicle_frame"], raw_inclination=rec["inclination"],
                     raw_azimuth=rec["azimuth"], pad_hw=np.array([H, WP]), bbox3d_ind=r["bbox3d_ind_of_each_pt"].reshape(H, W).astype(np.int32),
                     **{"raw_" + k: np.asarray(v, np.float32) for k, v in gt.items()}, **out, **params)
            if i < 2:
                fixture_conditions(g)
            else:
                assert all(np.isfinite(out[k]).all() and not out[k].any() for k in OUT_KEYS if k.split("_s")[0] in TARGETS)
            np.savez_compressed(os.path.join(HERE, "train_chain_%d.npz" % i), **g)
            ind = g["bbox3d_ind"]
            print("train_chain_%d: %d boxes, %d of %d pixels in a box, per level %s" %
                  (i, M, (ind >= 0).sum(), H * W, [int((out["rpn_reg_weight_s%d" % s][0] != 0).sum()) for s in (1, 2, 4)]))


if __name__ == "__main__":
    main()

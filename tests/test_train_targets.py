"""The training-time input chain on the device (rd_train_transform, csrc/k_target.h; rangedet_amd.core.input TRAIN_CHAIN): Bbox3dAssigner,
GenerateTarget and the training FPN targets fused with the input transform, against

  * tests/golden/train_chain_{0,1,2}.npz -- the outputs of the reference's OWN sixteen transform objects with its own training parameters
    (tests/golden/make_train_chain_golden.py; the assignment and the point counts behind them are the oracle's restatement of assigner.h,
    parity unpinned), and
  * tests/target_model.py -- the numpy restatement pinned by those files, for the shapes without a golden file.

Exact by value: bbox3d_ind, both weight tensors, rpn_cls_target, the masks, pc_*, coord_s1, input_data channels 0-6, target channel 6
(z - h/2) and every zero outside boxes and in the padding.  input_data channel 7 (azimuth): 1e-6 (device atan2f).  The other target
channels follow an error model (device atan2f / sinf / cosf / logf differ from numpy's by ulps, float32 on both sides):
  channels 0, 1   compared after signed squaring t|t| (the square root amplifies without bound at zero, the sign may flip there):
                  4e-6 (|d.x| + |d.y|) + 1e-7 per pixel, d = box centre - point: an azimuth error of 1e-6 rad plus four float32 roundings
                  on each side
  channels 4, 5   4e-6
  channels 2,3,7  1e-6 max(1, |v|)
"""
import glob
import os

import numpy as np
import pytest

import target_model as TM
from conftest import BOTH
from rangedet_amd import lib as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(glob.glob(os.path.join(GOLD, "train_chain_[0-9].npz")))
STRIDES = (1, 2, 4)
EXACT = ["coord_s1", "bbox3d_ind"] + ["%s_s%d" % (n, s) for n in ("pc_vehicle_frame", "range_image_mask", "rpn_reg_weight",
                                                                    "reg_normalize_weight", "rpn_cls_target") for s in STRIDES]
SHAPES = {"input_data": (8, 8, 64), "coord_s1": (3, 8, 64), "gt_bbox_veh_for_iou_pred": (200, 8)}
for _s in STRIDES:
    SHAPES["pc_vehicle_frame_s%d" % _s] = (8 * 64 // _s, 3)
    for _n, _c in (("range_image_mask", 1), ("rpn_reg_target", 8), ("rpn_reg_weight", 8), ("reg_normalize_weight", 8), ("rpn_cls_target", 1)):
        SHAPES["%s_s%d" % (_n, _s)] = (_c, 8, 64 // _s)


def _gold():
    assert len(FILES) == 3
    return [np.load(f) for f in FILES]


def _raw(g):
    return dict(range_image=g["raw_range_image"], pc_vehicle_frame=g["raw_pc_vehicle_frame"], inclination=g["raw_inclination"],
                azimuth=g["raw_azimuth"])


def _filtered_gt(g):
    """What FilterGTClass([1]) leaves of a golden frame's ground truth (input.py:62-86)."""
    keep = g["raw_gt_class"] == 1
    if not keep.any():
        return np.zeros((1, 8, 3), np.float32), np.zeros((1, 7), np.float32)
    return g["raw_gt_bbox_imu"][keep], g["raw_gt_bbox_csa"][keep]


def _device(be, recs, gts, pad_hw):
    from rangedet_amd.input_transform import DeviceTrainTransform
    rr = [dict(r, gt_bbox_imu=imu, gt_bbox_csa=csa) for r, (imu, csa) in zip(recs, gts)]
    out = DeviceTrainTransform(pad_hw=pad_hw, lib=be.lib, alloc=be.alloc, iou_pred_names=())(rr)
    be.alloc.sync()
    return {k: np.array(be.alloc.to_numpy(v)) for k, v in out.items()}


def check(got, want, csas, H, W, what):
    """got / want: dicts of (B, ...) arrays; csas: per frame the (M,7) boxes the indices point into.  Prints each figure, then asserts."""
    B, _, Hp, Wp = want["input_data"].shape
    for k in EXACT:
        assert got[k].shape == tuple(want[k].shape) and np.array_equal(got[k], want[k]), (what, k)
    assert np.array_equal(got["input_data"][:, :7], want["input_data"][:, :7]), (what, "input_data 0-6")
    e_az = np.abs(got["input_data"][:, 7] - want["input_data"][:, 7]).max()
    fig = {"input_data[7]": e_az}
    ok = e_az < 1e-6
    for b in range(B):
        k = want["bbox3d_ind"][b]
        d = csas[b][np.maximum(k, 0)][..., :3] - want["pc_vehicle_frame_s1"][b].reshape(Hp, Wp, 3)[:H, :W]
        bound = np.zeros((Hp, Wp), np.float32)
        bound[:H, :W] = np.where(k >= 0, 4e-6 * (np.abs(d[..., 0]) + np.abs(d[..., 1])) + 1e-7, 0)
        for s in STRIDES:
            g, w = got["rpn_reg_target_s%d" % s][b], want["rpn_reg_target_s%d" % s][b]
            assert g.shape == w.shape, (what, s)
            zero = want["rpn_reg_weight_s%d" % s][b][0] == 0                 # outside boxes, outside the level's interval, padding
            assert not g[:, zero].any() and np.isfinite(g).all(), (what, b, s, "zeros")
            assert np.array_equal(g[6], w[6]), (what, b, s, "channel 6")
            sq = np.abs(g[:2] * np.abs(g[:2]) - w[:2] * np.abs(w[:2]))
            r01 = (sq / np.maximum(bound[:, s // 2::s][None], 1e-30))[:, ~zero].max(initial=0)
            e45 = np.abs(g[4:6] - w[4:6]).max()
            e237 = (np.abs(g[[2, 3, 7]] - w[[2, 3, 7]]) / np.maximum(1, np.abs(w[[2, 3, 7]]))).max()
            for name, v in (("ch0,1 / bound", r01), ("ch4,5", e45), ("ch2,3,7 rel", e237)):
                fig[name] = max(fig.get(name, 0), float(v))
            ok = ok and r01 <= 1 and e45 <= 4e-6 and e237 <= 1e-6
    print(what, {k: "%.3g" % v for k, v in fig.items()})
    assert ok, (what, fig)


def test_fixture_conditions_hold_on_the_committed_data():
    """The golden frames cannot go vacuous: frames 0 / 1 (5 / 37 boxes) have >= 10 % of the valid pixels in a box, >= 8 weighted pixels on
    every level, a box whose points straddle flat index 256 (two workgroups) and an in-box pixel that is a missing return filled from its
    right neighbour; frame 2 (only a class-2 box -> the zero box) has all-zero, finite targets."""
    gs = _gold()
    assert [int((g["raw_gt_class"] == 1).sum()) for g in gs] == [5, 37, 0] and gs[2]["raw_gt_class"].tolist() == [2.0]
    for g in gs[:2]:
        ind = g["bbox3d_ind"].reshape(-1)
        ri = g["raw_range_image"][..., 0]
        miss = ri == -1
        valid = np.where(miss, np.roll(ri, -1, 1) > 0, ri > 0).reshape(-1)
        assert (ind[valid] >= 0).sum() >= 0.10 * valid.sum() and (ind[~valid] == -1).all()
        assert all((g["rpn_reg_weight_s%d" % s][0] != 0).sum() >= 8 for s in STRIDES)
        assert set(ind[:256][ind[:256] >= 0].tolist()) & set(ind[256:][ind[256:] >= 0].tolist())
        assert (ind[miss.reshape(-1) & valid] >= 0).any()
        assert g["raw_gt_bbox_csa"][:, 3:6].min() >= 1 and g["raw_gt_bbox_csa"][:, 3:6].max() <= 6              # sizes of 1 - 6 m
    yaw = np.concatenate([g["raw_gt_bbox_csa"][:, 6] for g in gs[:2]])
    assert all(((yaw >= a) & (yaw < a + np.pi / 2)).sum() >= 5 for a in (-np.pi, -np.pi / 2, 0, np.pi / 2))    # yaws over the full circle
    for n in TM.TARGETS:
        for s in STRIDES:
            a = gs[2]["%s_s%d" % (n, s)]
            assert np.isfinite(a).all() and not a.any()
    for g in gs:
        for k, shp in SHAPES.items():
            assert g[k].shape == shp and g[k].dtype == np.float32, k


def test_restatement_equals_reference_python():
    """tests/target_model.py on the golden inputs against the reference's outputs (CPU only)."""
    for i, g in enumerate(_gold()):
        imu, csa = _filtered_gt(g)
        got = TM.train_transform(_raw(g), imu, csa, (8, 64))
        want = {k: g[k][None] for k in list(SHAPES) + ["bbox3d_ind"] if k != "gt_bbox_veh_for_iou_pred"}
        check(got, want, [csa], 8, 62, "restatement, frame %d" % i)
        assert np.array_equal(got["input_data"][0].view(np.uint32), g["input_data"].view(np.uint32))


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_golden_through_the_abi(be):
    """rd_train_transform on the three golden frames as one batch of 3 (Mmax 37, num_gt 5 / 37 / 1) against the reference's outputs."""
    gs = _gold()
    gts = [_filtered_gt(g) for g in gs]
    got = _device(be, [_raw(g) for g in gs], gts, (8, 64))
    want = {k: np.stack([g[k] for g in gs]) for k in list(SHAPES) + ["bbox3d_ind"] if k != "gt_bbox_veh_for_iou_pred"}
    check(got, want, [c for _, c in gts], 8, 62, "golden (%s)" % be.name)


_SECOND = {}


def _second_shape():
    """B = 3, 16 x 250 padded to 256 (W % 4 != 0, padded columns on every level, 16 workgroups per frame), 0 (the zero box) / 12 / 300 boxes
    (Mmax != num_gt, most boxes empty): records, boxes and the restatement's outputs, computed once."""
    if not _SECOND:
        cases = [TM.make_case(i, 16, 250, n) for i, n in enumerate((0, 12, 300))]
        refs = [TM.train_transform(rec, imu, csa, (16, 256)) for rec, imu, csa in cases]
        _SECOND.update(recs=[c[0] for c in cases], gts=[(c[1], c[2]) for c in cases],
                       want={k: np.concatenate([r[k] for r in refs]) for k in refs[0]})
        ind = _SECOND["want"]["bbox3d_ind"]
        assert (ind[0] == -1).all() and (ind[1] >= 0).sum() > 40 and (ind[2] >= 0).sum() > 40 and len(np.unique(ind[2])) < 30
        assert all((_SECOND["want"]["rpn_reg_weight_s%d" % s][1:] != 0).sum() >= 8 for s in STRIDES)
    return _SECOND


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_second_shape_against_the_restatement(be):
    c = _second_shape()
    got = _device(be, c["recs"], c["gts"], (16, 256))
    check(got, c["want"], [g[1] for g in c["gts"]], 16, 250, "16x250 (%s)" % be.name)


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_deterministic(be):
    """The point counts go through atomics (integer: order-independent): two runs of the second shape are byte-identical."""
    c = _second_shape()
    a, b = _device(be, c["recs"], c["gts"], (16, 256)), _device(be, c["recs"], c["gts"], (16, 256))
    assert sorted(a) == sorted(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_python_surface(be, monkeypatch):
    """get_train_transform -> run_chain on the golden records: the reference's stage list, names, parameter values, shapes and values;
    the fused bbox3d_ind equals what Bbox3dAssigner.apply writes; chains the fused entry does not implement are refused."""
    from rangedet_amd import processing_cxx
    from rangedet_amd.config import rangedet_ped_wo_aug_all_36e as pedmod
    from rangedet_amd.config import rangedet_veh_wo_aug_4_18e as cfgmod
    from rangedet_amd.core import input as CI
    gs = _gold()
    transform, data_name, label_name = cfgmod.get_train_transform(feat_size=(8, 62), pad_field=(8, 64))
    names = [type(t).__name__ for t in transform]
    assert names == gs[0]["stage_names"].tolist() == CI.TRAIN_CHAIN                                   # config:347-365
    assert data_name == gs[0]["data_name"].tolist() and label_name == gs[0]["label_name"].tolist()    # config:367-378
    gen = transform[names.index("GenerateTarget")].param                                               # config:217-221
    assert list(gen.reg_weight) == gs[0]["reg_weight"].tolist() and list(gen.label_set) == gs[0]["label_set"].tolist()
    assert gen.num_classes == int(gs[0]["num_classes"]) == 1
    assert pedmod.get_train_transform(feat_size=(8, 62), pad_field=(8, 64))[2][-2] == "gt_bbox_ped_for_iou_pred"

    def records():
        return [dict(_raw(g), **{k: g["raw_" + k] for k in ("gt_class", "gt_bbox_imu", "gt_bbox_csa", "gt_bbox_yaw", "points_in_box",
                                                            "meta_data")}) for g in gs]
    launches = []
    monkeypatch.setattr(processing_cxx, "_ctx", lambda: (be.lib, be.alloc))
    real = processing_cxx.assign3D_v2
    monkeypatch.setattr(processing_cxx, "assign3D_v2", lambda *a: launches.append(1) or real(*a))
    CI._TRANSFORMS.clear()
    recs, out = CI.run_chain(transform, records(), lib=be.lib, alloc=be.alloc)
    be.alloc.sync()
    assert not launches                                            # the per-record assigner did not run: the fused entry computes it
    got = {k: np.array(be.alloc.to_numpy(v)) for k, v in out.items()}
    assert set(data_name + label_name) <= set(got)
    for k in data_name + label_name:
        assert got[k].shape == (3,) + SHAPES[k], k
    assert np.array_equal(got["gt_bbox_veh_for_iou_pred"], np.stack([g["gt_bbox_veh_for_iou_pred"] for g in gs]))
    want = {k: np.stack([g[k] for g in gs]) for k in list(SHAPES) + ["bbox3d_ind"] if k != "gt_bbox_veh_for_iou_pred"}
    check(got, want, [_filtered_gt(g)[1] for g in gs], 8, 62, "run_chain (%s)" % be.name)
    # Bbox3dAssigner.apply, called directly, on the same records
    asg = transform[names.index("Bbox3dAssigner")]
    for b, rec in enumerate(records()):
        for t in transform[:names.index("Bbox3dAssigner")]:
            t.apply(rec)
        asg.apply(rec)
        assert rec["bbox3d_ind_of_each_pt"].shape == (8, 62, 1)
        assert np.array_equal(rec["bbox3d_ind_of_each_pt"][..., 0], got["bbox3d_ind"][b])
    assert len(launches) == 3
    # refused, not approximated
    with pytest.raises(NotImplementedError):
        CI.run_chain([t for t in transform if not isinstance(t, CI.Bbox3dAssigner)], records(), lib=be.lib, alloc=be.alloc)
    two = type("P", (), dict(feat_size=(8, 62), reg_weight=[3, 1, 1, 1, 1, 1, 1, 1], label_set=[1, 2], num_classes=2))
    rec = records()[0]
    CI.LoadRecord().apply(rec)
    with pytest.raises(NotImplementedError):
        CI.GenerateTarget(two).apply(rec)
    with pytest.raises(NotImplementedError):
        CI.GenerateTarget(gen).apply({})


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_status_codes(be):
    """RD_ESHAPE / RD_EWORKSPACE instead of a launch; the thread-local message is set.  (Every check precedes the first launch, so one
    zeroed buffer stands for all device pointers.)"""
    import ctypes
    from rangedet_amd.input_transform import TrainOutputs, make_norm
    L = be.lib
    buf = be.empty(1 << 16)
    p = be.ptr(buf)
    o = TrainOutputs()
    o.input_data = o.coord_s1 = o.bbox3d_ind = p
    for f in ("pc", "mask", "reg_target", "reg_weight", "reg_normalize_weight", "cls_target"):
        for l in range(3):
            getattr(o, f)[l] = p
    norm, rw = make_norm(), (ctypes.c_float * 8)(3, 1, 1, 1, 1, 1, 1, 1)

    def call(B=2, H=8, W=62, Hp=8, Wp=64, Mmax=5, num_gt=(5, 1), ws_bytes=None):
        ng = (ctypes.c_int * len(num_gt))(*num_gt)
        nb = L.raw("rd_train_transform_workspace_bytes")(B) if ws_bytes is None else ws_bytes
        return L.raw("rd_train_transform")(p, p, p, ctypes.addressof(norm), p, p, p, p, ctypes.addressof(ng), Mmax, 100.0, 20.0,
                                           ctypes.addressof(rw), B, H, W, Hp, Wp, ctypes.addressof(o), p, nb, be.stream)
    assert L.raw("rd_train_transform_workspace_bytes")(2) == 2 * 500 * 4
    for kw in (dict(Wp=62), dict(Wp=66), dict(Hp=7), dict(Wp=60), dict(Mmax=0), dict(num_gt=(5, 0)), dict(num_gt=(-1, 5)),
               dict(Mmax=501, num_gt=(501, 1)), dict(num_gt=(6, 1))):
        assert call(**kw) == R.RD_ESHAPE, kw
        assert L.rd_last_error_string().decode() != ""
    assert call(ws_bytes=2 * 500 * 4 - 1) == R.RD_EWORKSPACE and "workspace" in L.rd_last_error_string().decode()
    assert call(ws_bytes=0) == R.RD_EWORKSPACE

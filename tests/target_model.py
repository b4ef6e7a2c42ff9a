"""TEST INFRASTRUCTURE ONLY: numpy restatement of the reference's TRAINING-time transform chain for one record --
Bbox3dAssigner (rangedet/core/input.py:276-320), GenerateTarget (:323-519), the training PadData / TransposeData / GenerateFPNTarget /
TransAndReshape (:522-624 with the name lists of config/rangedet/rangedet_veh_wo_aug_4_18e.py:72-81,295-305,316-326,336) -- for any
H, W, pad and box set.  It sits on oracle/input_ref.py (the test-time chain, pinned bit for bit) and oracle.cpu_ops.assign3d_v2 /
get_point_num (restatements of assigner.h, parity unpinned).

PINNED by tests/test_train_targets.py::test_restatement_equals_reference_python against tests/golden/train_chain_*.npz (the reference's
own Python on the same inputs); used for the shapes that have no golden file.
"""
import numpy as np

from oracle import cpu_ops as O
from oracle import input_ref as IR

REG_WEIGHT = (3, 1, 1, 1, 1, 1, 1, 1)          # config:219
TARGETS = ("rpn_reg_target", "rpn_reg_weight", "reg_normalize_weight", "rpn_cls_target")


def post_fill(rec):
    """(pc (H,W,3), mask (H,W), clipped unnormalised range (H,W)) after LoadRecord + ProcessMissValue + SepAndClipData."""
    ri = np.asarray(rec['range_image'], np.float32)
    pc = np.asarray(rec['pc_vehicle_frame'], np.float32).copy()
    H, W, _ = ri.shape
    pc[~(ri[..., 0] > 0)] = 0
    miss = ri[..., 0] == -1
    nb = list(range(1, W)) + [0]
    r0 = np.where(miss, ri[:, nb, 0], ri[..., 0])
    mask = np.where(miss, ri[:, nb, 0] > 0, ri[..., 0] > 0)
    pc[miss] = pc[:, nb][miss]
    still = r0 == -1
    dn, up = r0[[H - 2, H - 1] + list(range(H - 2))], r0[list(range(2, H)) + [0, 1]]
    rt, lf = r0[:, [W - 2, W - 1] + list(range(W - 2))], r0[:, list(range(2, W)) + [0, 1]]
    car = still & ((dn != -1) | (up != -1) | (rt != -1) | (lf != -1))
    r = r0.copy()
    r[still] = 80
    r[car] = 0
    pc[still] = 0
    return pc, mask.astype(np.float32), np.clip(r, IR.CLIP['range_value'][0], IR.CLIP['range_value'][1]).astype(np.float32)


def reg_target(pc, csa, ind):
    """input.py:452-506 in float32: pc (N,3), csa (M,7) x y z l w h yaw, ind (N,) -> (N,8)."""
    out = np.zeros((len(pc), 8), np.float32)
    inb = ind >= 0
    if not inb.any():
        return out
    b = csa[ind]
    az = np.arctan2(pc[:, 1], pc[:, 0])
    c, s = np.cos(az), np.sin(az)
    d = b[:, :3] - pc
    r = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], 1)
    r = np.sqrt(np.abs(r)) * np.sign(r)
    with np.errstate(divide='ignore'):
        out = np.stack([r[:, 0], r[:, 1], np.log(b[:, 4]), np.log(b[:, 3]), np.cos(b[:, 6] - az), np.sin(b[:, 6] - az),
                        b[:, 2] - b[:, 5] / 2, np.log(b[:, 5])], 1).astype(np.float32)
    out[~inb] = 0
    return out


def train_transform(rec, gt_bbox_imu, gt_bbox_csa, pad_hw, reg_weight=REG_WEIGHT):
    """One record -> the named arrays of the training chain with batch dim 1 (float32; bbox3d_ind int32)."""
    gt = np.asarray(gt_bbox_imu, np.float32).reshape(-1, 8, 3)
    csa = np.asarray(gt_bbox_csa, np.float32).reshape(-1, 7)
    Hp, Wp = pad_hw
    base = IR.transform(rec, pad_hw)
    out = {k: base[k] for k in ('input_data', 'coord_s1', 'pc_vehicle_frame_s1', 'pc_vehicle_frame_s2', 'pc_vehicle_frame_s4')}
    pc, mask, unnorm = post_fill(rec)
    H, W = mask.shape
    lim = [float(f(gt[:, :, a])) for a in range(3) for f in (np.max, np.min)]
    ind = O.assign3d_v2(pc.reshape(-1, 3), gt.reshape(-1, 24), gt.mean(axis=1), np.full(len(gt), 100, np.float32), mask.reshape(-1),
                        np.zeros(H * W, np.float32), *lim, 20.0)
    with np.errstate(divide='ignore'):
        nw = 1 / O.get_point_num(ind.astype(np.float32))
    nw[nw == -1] = 0
    inb = (ind >= 0)
    full = {'rpn_reg_target': reg_target(pc.reshape(-1, 3), csa, ind),
            'rpn_reg_weight': inb[:, None] * np.asarray(reg_weight, np.float32)[None, :],
            'reg_normalize_weight': np.tile(nw[:, None], (1, 8)),
            'rpn_cls_target': inb[:, None].astype(np.float32),
            'range_image_mask': mask.reshape(-1, 1)}

    def pad(a):
        p = np.zeros((Hp, Wp, a.shape[-1]), np.float32)
        p[:H, :W] = a.reshape(H, W, -1)
        return p.transpose(2, 0, 1)
    un = pad(unnorm[..., None])
    for s in IR.FPN_STRIDES:
        lo, hi = IR.INTERVAL[s]
        m = ((lo <= un) & (un < hi)).astype(np.float32)
        for name, a in full.items():
            p = pad(a)
            if name != 'range_image_mask':
                p = p * m
            out['%s_s%d' % (name, s)] = np.ascontiguousarray(p[:, :, s // 2::s][None], dtype=np.float32)
    out['bbox3d_ind'] = ind.reshape(1, H, W).astype(np.int32)
    return out


def boxes(ctr, lwh, yaw):
    """(M,3) centres, (M,3) l w h, (M,) yaw -> gt_bbox_imu (M,8,3) (A B C D bottom face, E F G H top) and gt_bbox_csa (M,7)."""
    l, w, h = lwh[:, 0], lwh[:, 1], lwh[:, 2]
    cor = np.stack([np.stack([l / 2, -w / 2], 1), np.stack([-l / 2, -w / 2], 1), np.stack([-l / 2, w / 2], 1),
                    np.stack([l / 2, w / 2], 1)], 1)
    rot = np.stack([np.stack([np.cos(yaw), -np.sin(yaw)], 1), np.stack([np.sin(yaw), np.cos(yaw)], 1)], 1)
    xy = np.einsum('mij,mkj->mki', rot, cor) + ctr[:, None, :2]
    bot = np.concatenate([xy, np.repeat((ctr[:, 2] - h / 2)[:, None, None], 4, 1)], 2)
    top = np.concatenate([xy, np.repeat((ctr[:, 2] + h / 2)[:, None, None], 4, 1)], 2)
    return np.concatenate([bot, top], 1).astype(np.float32), np.concatenate([ctr, lwh, yaw[:, None]], 1).astype(np.float32)


def make_case(i, H, W, nbox, nfull=12):
    """Synthetic record i (ranges remapped to a 4 .. 45 m sweep over the columns, so that every FPN level holds points and
    neighbouring points share boxes) with `nbox` boxes: the first `nfull` centred on pixels' points, the rest 40 m above the scene
    (empty); nbox = 0 gives the single zero box FilterGTClass leaves."""
    from rangedet_amd import synth
    rng = np.random.default_rng(900 + i)
    rec = synth.raw_record(i, H=H, W=W)
    ri, incl, az = rec["range_image"], rec["inclination"], rec["azimuth"]
    valid = ri[..., 0] > 0
    r = ((4.0 + 41.0 * np.arange(W) / (W - 1))[None, :] * (0.9 + 0.2 * ri[..., 0] / 75.0)).astype(np.float32)
    pc = np.stack([r * np.cos(incl)[:, None] * np.cos(az)[None, :], r * np.cos(incl)[:, None] * np.sin(az)[None, :],
                   r * np.sin(incl)[:, None] + 2.0], 2).astype(np.float32)
    ri[..., 0][valid] = r[valid]
    rec["pc_vehicle_frame"][valid] = pc[valid]
    if nbox == 0:
        return rec, np.zeros((1, 8, 3), np.float32), np.zeros((1, 7), np.float32)
    P = rec["pc_vehicle_frame"][valid]
    ctr = P[rng.integers(0, len(P), nbox)].astype(np.float64)
    ctr[nfull:, 2] += 40.0
    imu, csa = boxes(ctr, rng.uniform(1.0, 6.0, (nbox, 3)), rng.uniform(-np.pi, np.pi, nbox))
    return rec, imu, csa

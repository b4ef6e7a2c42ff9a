"""Test-time input transform chain on the device: the build's counterpart of the reference's loader-side transforms
(rangedet/core/input.py: LoadRecord, ProcessMissValue, SepAndClipData, GetUnnormalizedRange, NormData, GetCoordinates,
CombineData, PadData, TransposeData, GenerateFPNTarget, TransAndReshape; constants config:245-282,71).

Only the raw record arrays (range_image (H,W,4), pc_vehicle_frame (H,W,3), inclination (H,)) go to the GPU; one fused
kernel (csrc/k_input.h, rd_input_transform) writes the named float32 tensors the graph consumes.
"""
import ctypes

import numpy as np

from . import lib as rdlib
from . import synth

ORDER = ['range_value', 'intensity', 'elongation', 'pc_vehicle_frame_x', 'pc_vehicle_frame_y', 'pc_vehicle_frame_z',
         'inclination', 'azimuth']


class InputNorm(ctypes.Structure):   # rd_input_norm_t
    _fields_ = [("clip_lo", ctypes.c_float * 7), ("clip_hi", ctypes.c_float * 7), ("mean", ctypes.c_float * 8),
                ("sd", ctypes.c_float * 8), ("interval_lo", ctypes.c_float * 3), ("interval_hi", ctypes.c_float * 3)]


def make_norm(clip=None, norm=None, interval=None, strides=(1, 2, 4)):
    clip, norm, interval = clip or synth.CLIP, norm or synth.NORM, interval or synth.INTERVAL
    n = InputNorm()
    for i, name in enumerate(ORDER):
        if i < 7:
            n.clip_lo[i], n.clip_hi[i] = clip[name]
        n.mean[i] = norm[name][0]
        n.sd[i] = np.float32(norm[name][1] ** 0.5)
    for l, s in enumerate(strides):
        n.interval_lo[l], n.interval_hi[l] = interval[s]
    return n


class DeviceInputTransform:
    def __init__(self, pad_hw=(64, 2656), lib=None, alloc=None, clip=None, norm=None, interval=None):
        from .runtime import TorchAllocator
        self.L = lib or rdlib.get_lib()
        self.A = alloc or TorchAllocator()
        self.pad_hw = tuple(pad_hw)
        self.norm = make_norm(clip, norm, interval)

    def __call__(self, records):
        """records: list of dicts with 'range_image', 'pc_vehicle_frame', 'inclination' (numpy) -> dict of device tensors."""
        A, L = self.A, self.L
        B = len(records)
        H, W, _ = records[0]['range_image'].shape
        Hp, Wp = self.pad_hw
        ri = A.upload(np.stack([np.asarray(r['range_image'], np.float32) for r in records]))
        pc = A.upload(np.stack([np.asarray(r['pc_vehicle_frame'], np.float32) for r in records]))
        inc = A.upload(np.stack([np.asarray(r['inclination'], np.float32) for r in records]))
        npx = Hp * Wp
        shapes = {'input_data': (B, 8, Hp, Wp), 'coord_s1': (B, 3, Hp, Wp)}
        for s in (1, 2, 4):
            shapes['pc_vehicle_frame_s%d' % s] = (B, npx // s, 3)
            shapes['range_image_mask_s%d' % s] = (B, npx // s)
        bufs = {k: A.alloc(int(np.prod(v)) * 4) for k, v in shapes.items()}
        st = A.stream_ptr(None) if hasattr(A, "stream_ptr") else A.stream
        L.call("rd_input_transform", A.ptr(ri), A.ptr(pc), A.ptr(inc), ctypes.addressof(self.norm), B, H, W, Hp, Wp,
               A.ptr(bufs['input_data']), A.ptr(bufs['coord_s1']), A.ptr(bufs['pc_vehicle_frame_s1']),
               A.ptr(bufs['pc_vehicle_frame_s2']), A.ptr(bufs['pc_vehicle_frame_s4']), A.ptr(bufs['range_image_mask_s1']),
               A.ptr(bufs['range_image_mask_s2']), A.ptr(bufs['range_image_mask_s4']), st)
        return {k: A.view_f32(bufs[k], shapes[k]) for k in shapes}


class TrainOutputs(ctypes.Structure):   # rd_train_outputs_t
    _fields_ = [("input_data", ctypes.c_void_p), ("coord_s1", ctypes.c_void_p), ("pc", ctypes.c_void_p * 3),
                ("mask", ctypes.c_void_p * 3), ("reg_target", ctypes.c_void_p * 3), ("reg_weight", ctypes.c_void_p * 3),
                ("reg_normalize_weight", ctypes.c_void_p * 3), ("cls_target", ctypes.c_void_p * 3), ("bbox3d_ind", ctypes.c_void_p)]


# field of rd_train_outputs_t -> name of the per-level tensor, channels
_TRAIN_LEVEL = [("mask", "range_image_mask", 1), ("reg_target", "rpn_reg_target", 8), ("reg_weight", "rpn_reg_weight", 8),
                ("reg_normalize_weight", "reg_normalize_weight", 8), ("cls_target", "rpn_cls_target", 1)]


def train_shapes(B, H, W, Hp, Wp):
    """Names and shapes of everything rd_train_transform writes (bbox3d_ind is int32, the rest float32)."""
    shapes = {'input_data': (B, 8, Hp, Wp), 'coord_s1': (B, 3, Hp, Wp), 'bbox3d_ind': (B, H, W)}
    for s in (1, 2, 4):
        shapes['pc_vehicle_frame_s%d' % s] = (B, Hp * Wp // s, 3)
        for _, name, c in _TRAIN_LEVEL:
            shapes['%s_s%d' % (name, s)] = (B, c, Hp, Wp // s)
    return shapes


class DeviceTrainTransform:
    """The training-time chain (config:346-378) for a batch of records in one rd_train_transform call (csrc/k_target.h): raw
    arrays and ground truth up, every tensor of data_name + label_name (and rpn_cls_target_s*, bbox3d_ind) stays on the device."""
    RADIUS, MAX_DIST = 100.0, 20.0      # rangedet/core/input.py:299,309 (both compared with squared distances, assigner.h:47-51)

    def __init__(self, pad_hw=(64, 2656), lib=None, alloc=None, clip=None, norm=None, interval=None,
                 reg_weight=(3, 1, 1, 1, 1, 1, 1, 1), iou_pred_names=('gt_bbox_veh_for_iou_pred',)):
        from .runtime import TorchAllocator
        self.L = lib or rdlib.get_lib()
        self.A = alloc or TorchAllocator()
        self.pad_hw = tuple(pad_hw)
        self.norm = make_norm(clip, norm, interval)
        if len(reg_weight) != 8:
            raise ValueError("reg_weight: 8 values (the 8 regression targets), got %r" % (reg_weight,))
        self.reg_weight = (ctypes.c_float * 8)(*[float(v) for v in reg_weight])
        self.iou_pred_names = tuple(iou_pred_names)

    def __call__(self, records):
        """records: dicts with 'range_image', 'pc_vehicle_frame', 'inclination', 'gt_bbox_imu' (M,8,3), 'gt_bbox_csa' (M,7) and the
        host stage's 'gt_bbox_<cls>_for_iou_pred' (numpy) -> dict of named (B, ...) device tensors."""
        args, out, _ = self.prepare(records)
        self.L.call("rd_train_transform", *args)
        return out

    def prepare(self, records):
        """Upload and allocate: (arguments of rd_train_transform, the named output tensors, the buffers the arguments point to)."""
        A, L = self.A, self.L
        B = len(records)
        H, W, _ = records[0]['range_image'].shape
        Hp, Wp = self.pad_hw
        gts = [np.asarray(r['gt_bbox_imu'], np.float32).reshape(-1, 8, 3) for r in records]
        csas = [np.asarray(r['gt_bbox_csa'], np.float32).reshape(-1, 7) for r in records]
        if any(len(g) != len(c) or len(g) < 1 for g, c in zip(gts, csas)):
            raise ValueError("gt_bbox_imu / gt_bbox_csa: the same number (>= 1) of boxes per record")
        Mmax = max(len(g) for g in gts)
        imu, ctr, csa = np.zeros((B, Mmax, 24), np.float32), np.zeros((B, Mmax, 3), np.float32), np.zeros((B, Mmax, 7), np.float32)
        lim = np.zeros((B, 6), np.float32)
        for b, (g, c) in enumerate(zip(gts, csas)):
            imu[b, :len(g)] = g.reshape(-1, 24)
            ctr[b, :len(g)] = g.mean(axis=1)                               # exactly Bbox3dAssigner's host arithmetic (input.py:301-308):
            lim[b] = [f(g[:, :, a]) for a in range(3) for f in (np.max, np.min)]   # the assignment depends on their last bit
            csa[b, :len(g)] = c
        num_gt = (ctypes.c_int * B)(*[len(g) for g in gts])
        dev = [A.upload(np.stack([np.asarray(r[k], np.float32) for r in records]))
               for k in ('range_image', 'pc_vehicle_frame', 'inclination')] + [A.upload(x) for x in (imu, ctr, lim, csa)]
        shapes = train_shapes(B, H, W, Hp, Wp)
        bufs = {k: A.alloc(int(np.prod(v)) * 4) for k, v in shapes.items()}
        o = TrainOutputs()
        o.input_data, o.coord_s1, o.bbox3d_ind = A.ptr(bufs['input_data']), A.ptr(bufs['coord_s1']), A.ptr(bufs['bbox3d_ind'])
        for l, s in enumerate((1, 2, 4)):
            o.pc[l] = A.ptr(bufs['pc_vehicle_frame_s%d' % s])
            for field, name, _ in _TRAIN_LEVEL:
                getattr(o, field)[l] = A.ptr(bufs['%s_s%d' % (name, s)])
        nb = L.raw("rd_train_transform_workspace_bytes")(B)
        ws = A.alloc(nb)
        st = A.stream_ptr(None) if hasattr(A, "stream_ptr") else A.stream
        args = [A.ptr(t) for t in dev[:3]] + [ctypes.addressof(self.norm)] + [A.ptr(t) for t in dev[3:]] + \
            [ctypes.addressof(num_gt), Mmax, self.RADIUS, self.MAX_DIST, ctypes.addressof(self.reg_weight), B, H, W, Hp, Wp,
             ctypes.addressof(o), A.ptr(ws), nb, st]
        out = {k: (A.view_i32 if k == 'bbox3d_ind' else A.view_f32)(bufs[k], shapes[k]) for k in shapes}
        for name in self.iou_pred_names:                                 # GetFixedLengthGTBbox (host stage), (B, fixed_length, 8)
            fixed = np.stack([np.asarray(r[name], np.float32) for r in records])
            out[name] = A.view_f32(A.upload(fixed), fixed.shape)
        return args, out, (dev, ws, num_gt, o)

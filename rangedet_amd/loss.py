"""The RPN loss head on the device: the build's counterpart of RangeRpnHead.get_fpn_loss with get_iou_target, get_vfl_loss and
get_normalize_reg_loss (rangedet/symbol/head/builder.py:156-196,268-422) and vari_focal_loss (rangedet/symbol/head/loss.py:4-30) in the
reference.  One rd_rpn_loss call (csrc/k_loss.h) per pyramid level turns the head outputs and the training inputs into the reference's
loss maps and into what MakeLoss sends back to the logits and the deltas; the decoded boxes never reach memory.

    train = DeviceTrainTransform(...)(records)                # or core.input.run_chain(get_train_transform(...)[0], records)[1]
    out = RpnLoss()(logits, deltas, train)                    # flat (B,N) / (B,N,8) head outputs, or one tensor per level
    RpnLoss.update_metrics(metric_list, out)                  # the config's six ScalarLoss objects

This is not a recorded training graph: get_config(True) and the builder's loss methods keep raising, and nothing here goes back through
the towers (rangedet_amd.backward.HeadTowerBackward takes d_logit / d_delta from here).  One class, iou_type 'bev'.
"""
import ctypes

import numpy as np

from . import lib as rdlib


class LossParam(ctypes.Structure):   # rd_loss_param_t
    _fields_ = [("alpha", ctypes.c_float), ("gamma", ctypes.c_float), ("cls_loss_weight", ctypes.c_float),
                ("reg_loss_weight", ctypes.c_float), ("smooth_l1_scalar", ctypes.c_float), ("scale_loss_shift", ctypes.c_float),
                ("l1", ctypes.c_int)]


def make_loss_param(loss_param=None, fp16=True):
    """rd_loss_param_t from a class with the attributes of the reference's RpnParam.loss (config:122-129).  smooth_l1_scalar defaults to
    1 and l1 to False like in builder.py:395-397; scale_loss_shift is 1 unless fp16 (builder.py:97)."""
    if loss_param is None:
        from .config.rangedet_veh_wo_aug_4_18e import get_loss_param
        loss_param = get_loss_param(fp16)
    iou_type = getattr(loss_param, "iou_type", "bev")
    if iou_type != "bev":
        raise NotImplementedError("RpnLoss: iou_type %r -- the fused loss computes the 'bev' IoU target only (the '3d' op exists as "
                                  "rd_batch_rotated_iou_3d, not inside the loss)" % (iou_type,))
    p = LossParam()
    p.alpha, p.gamma = float(loss_param.alpha), float(loss_param.gamma)
    p.cls_loss_weight, p.reg_loss_weight = float(loss_param.cls_loss_weight), float(loss_param.reg_loss_weight)
    p.smooth_l1_scalar = float(getattr(loss_param, "smooth_l1_scalar", 1.0))
    p.scale_loss_shift = float(getattr(loss_param, "scale_loss_shift", 128.0)) if fp16 else 1.0
    p.l1 = 1 if getattr(loss_param, "l1", False) else 0
    return p


class RpnLoss:
    """(logits, deltas, train) -> dict of device tensors on the current stream, without a host synchronisation:
      rpn_cls_loss_s{s} (B,1,H,W/s), rpn_reg_loss_s{s} (B,8,H,W/s)   the reference's outputs of these names
      iou_target_s{s} (B,1,H,W/s)                                      the IoU target (behind block_grad in the reference)
      stats_s{s} (4,)                                                  norm_cls, norm_reg, sum(cls_loss), sum(reg_loss)
      d_logit, d_delta                                                 the gradients, in the layout logits / deltas came in
    The buffers are reused between calls with the same shapes: a result is valid until the next such call."""

    def __init__(self, loss_param=None, fp16=True, strides=(1, 2, 4), class_name='veh', lib=None, alloc=None):
        if not isinstance(class_name, str):
            if len(class_name) != 1:
                raise NotImplementedError("RpnLoss: one class per head (GenerateTarget makes single-class targets, input.py:383-384), "
                                          "got %r" % (tuple(class_name),))
            class_name = class_name[0]
        self.param = make_loss_param(loss_param, fp16)
        self.strides = tuple(strides)
        self.gt_name = 'gt_bbox_%s_for_iou_pred' % class_name
        self.L = lib or rdlib.get_lib()
        if alloc is None:
            from .runtime import TorchAllocator
            alloc = TorchAllocator()
        self.A = alloc
        self._bufs = {}

    def _level_inputs(self, train):
        A, lv = self.A, []
        gt = A.as_device_f32(train[self.gt_name])
        if len(gt.shape) != 3 or gt.shape[2] != 8:
            raise ValueError("%s: (B, n_gt, 8), got %r" % (self.gt_name, tuple(gt.shape)))
        for s in self.strides:
            t = {k: A.as_device_f32(train['%s_s%d' % (name, s)]) for k, name in
                 (("mask", "range_image_mask"), ("reg_target", "rpn_reg_target"), ("reg_weight", "rpn_reg_weight"),
                  ("reg_norm_weight", "reg_normalize_weight"), ("pc", "pc_vehicle_frame"))}
            if len(t["mask"].shape) != 4 or t["mask"].shape[1] != 1:
                raise ValueError("range_image_mask_s%d: (B, 1, H, W/s) as the training-time chain writes it, got %r" % (s, tuple(t["mask"].shape)))
            B, H, Wl = int(t["mask"].shape[0]), int(t["mask"].shape[2]), int(t["mask"].shape[3])
            want = {"mask": B * H * Wl, "reg_target": B * 8 * H * Wl, "reg_weight": B * 8 * H * Wl, "reg_norm_weight": B * 8 * H * Wl,
                    "pc": B * H * Wl * 3}
            for k, v in t.items():
                if int(np.prod(v.shape)) != want[k] or B != gt.shape[0]:
                    raise ValueError("level s%d: %s has shape %r next to a (%d, 1, %d, %d) mask" % (s, k, tuple(v.shape), B, H, Wl))
            lv.append((t, B, H, Wl))
        return gt, lv

    def __call__(self, logits, deltas, train):
        A, L = self.A, self.L
        gt, lv = self._level_inputs(train)
        B = lv[0][1]
        ns = [H * Wl for _, _, H, Wl in lv]
        flat = not isinstance(logits, (list, tuple))
        if flat != (not isinstance(deltas, (list, tuple))):
            raise ValueError("logits and deltas: both flat tensors or both per-level lists")
        if flat:
            N = sum(ns)
            lg, dl = A.as_device_f32(logits), A.as_device_f32(deltas)
            if tuple(lg.shape) != (B, N) or tuple(dl.shape) != (B, N, 8):
                raise ValueError("flat logits / deltas: (%d, %d) and (%d, %d, 8) for these levels, got %r and %r" %
                                 (B, N, B, N, tuple(lg.shape), tuple(dl.shape)))
            offs = np.concatenate([[0], np.cumsum(ns)]).tolist()
            src = [(rdlib.ptr(lg) + 4 * offs[l], N, rdlib.ptr(dl) + 32 * offs[l], 8 * N) for l in range(len(ns))]
        else:
            if len(logits) != len(ns) or len(deltas) != len(ns):
                raise ValueError("one logit and one delta tensor per level (%d), got %d and %d" % (len(ns), len(logits), len(deltas)))
            src, keep = [], []                                    # keep: contiguous copies stay alive until the calls are enqueued
            for l, n in enumerate(ns):
                lg, dl = A.as_device_f32(logits[l]), A.as_device_f32(deltas[l])
                if int(np.prod(lg.shape)) != B * n or tuple(dl.shape) != (B, n, 8):
                    raise ValueError("level %d: logits of %d values and deltas (%d, %d, 8), got %r and %r" %
                                     (l, B * n, B, n, tuple(lg.shape), tuple(dl.shape)))
                keep += [lg, dl]
                src.append((rdlib.ptr(lg), n, rdlib.ptr(dl), 8 * n))
        key = (B, tuple((H, Wl) for _, _, H, Wl in lv), flat)
        if key not in self._bufs:
            per = []
            for n in ns:
                nws = L.raw("rd_rpn_loss_workspace_bytes")(B, n)
                per.append(dict(cls=A.alloc(B * n * 4), reg=A.alloc(B * 8 * n * 4), iou=A.alloc(B * n * 4), stats=A.alloc(16),
                                ws=A.alloc(nws), nws=nws))
            grads = [(A.alloc(B * sum(ns) * 4), A.alloc(B * sum(ns) * 32))] if flat else [(A.alloc(B * n * 4), A.alloc(B * n * 32)) for n in ns]
            self._bufs[key] = (per, grads)
        per, grads = self._bufs[key]
        st = A.stream_ptr(None) if hasattr(A, "stream_ptr") else A.stream
        out = {}
        for l, (s, (t, _, H, Wl)) in enumerate(zip(self.strides, lv)):
            n, pb = ns[l], per[l]
            lp, lbs, dp, dbs = src[l]
            if flat:
                glp, gdp = A.ptr(grads[0][0]) + (lp - src[0][0]), A.ptr(grads[0][1]) + (dp - src[0][2])
            else:
                glp, gdp = A.ptr(grads[l][0]), A.ptr(grads[l][1])
            L.call("rd_rpn_loss", lp, lbs, dp, dbs, rdlib.ptr(t["pc"]), rdlib.ptr(gt), int(gt.shape[1]), rdlib.ptr(t["mask"]),
                   rdlib.ptr(t["reg_target"]), rdlib.ptr(t["reg_weight"]), rdlib.ptr(t["reg_norm_weight"]), B, H, Wl,
                   ctypes.addressof(self.param), A.ptr(pb["cls"]), A.ptr(pb["reg"]), glp, gdp, A.ptr(pb["iou"]), None, A.ptr(pb["stats"]),
                   A.ptr(pb["ws"]), pb["nws"], st)
            out['rpn_cls_loss_s%d' % s] = A.view_f32(pb["cls"], (B, 1, H, Wl))
            out['rpn_reg_loss_s%d' % s] = A.view_f32(pb["reg"], (B, 8, H, Wl))
            out['iou_target_s%d' % s] = A.view_f32(pb["iou"], (B, 1, H, Wl))
            out['stats_s%d' % s] = A.view_f32(pb["stats"], (4,))
        if flat:
            out['d_logit'], out['d_delta'] = A.view_f32(grads[0][0], (B, sum(ns))), A.view_f32(grads[0][1], (B, sum(ns), 8))
        else:
            out['d_logit'] = [A.view_f32(g[0], (B, n)) for g, n in zip(grads, ns)]
            out['d_delta'] = [A.view_f32(g[1], (B, n, 8)) for g, n in zip(grads, ns)]
        return out

    @staticmethod
    def update_metrics(metric_list, out):
        """Feed the config's ScalarLoss objects (config:403-416) by their output_names ('rpn_reg_loss_s1_output', ...)."""
        for m in metric_list:
            names = [n[:-len("_output")] if n.endswith("_output") else n for n in m.output_names]
            missing = [n for n in names if n not in out]
            if missing:
                raise KeyError("metric %s: no output named %s" % (m.name, ", ".join(missing)))
            m.update([], [out[n] for n in names])

"""Loss head timing (dev tool): RpnLoss (one rd_rpn_loss call per level) against the route the library offered before it -- per level
rd_decode3d_bbox + rd_batch_rotated_iou, then the loss and gradient formulas as torch operations on the device.

    python tools/loss_timing.py [--batch 8] [--iters 50] [--repeats 7] [--out profiles/loss_timing.json]

B frames of 64 x 2656, three levels, 200 GT rows per frame (40 real boxes, the rest padding).  Each figure is the median over `repeats`
windows of `iters` calls between device events, after a warm-up of both routes; the windows alternate fused / torch and the whole series
is run in both orders.  The two routes' results are compared on the same inputs before anything is timed."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rangedet_amd import build, lib as rdlib  # noqa: E402
from rangedet_amd.loss import RpnLoss  # noqa: E402
from rangedet_amd.runtime import TorchAllocator  # noqa: E402
from tools.timing_util import series  # noqa: E402

H, WP, STRIDES, NGT, NREAL = 64, 2656, (1, 2, 4), 200, 40


def make_inputs(B, dev, L, st):
    g = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda *s: torch.rand(*s, generator=g)          # noqa: E731
    N = sum(H * WP // s for s in STRIDES)
    logits = (torch.randn(B, N, generator=g) * 3).to(dev)
    deltas = (torch.randn(B, N, 8, generator=g) * 0.7).to(dev)
    train, off = {}, 0
    gt = torch.tensor([0, 0, 0, 1e-3, 1e-3, 1e-3, 1e-3, 0]).repeat(B, NGT, 1)
    for l, s in enumerate(STRIDES):
        Wl = WP // s
        n = H * Wl
        r, az = 5 + 70 * rnd(B, n), (rnd(B, n) * 2 - 1) * np.pi
        pc = torch.stack([r * torch.cos(az), r * torch.sin(az), rnd(B, n) * 3 - 1], -1).to(dev)
        take = NREAL // len(STRIDES) + (1 if l < NREAL % len(STRIDES) else 0)
        pick = torch.stack([torch.randperm(n, generator=g)[:take] for _ in range(B)])
        bi = torch.arange(B)[:, None]
        bid, pickd = bi.to(dev), pick.to(dev)
        lv = deltas[:, off:off + n]
        lv[bid, pickd, 2:6] = torch.tensor([np.log(2.0), np.log(4.0), 1.0, 0.0], device=dev, dtype=torch.float32)
        boxes = torch.empty(B, n, 10, device=dev)
        L.call("rd_decode3d_bbox", lv.contiguous().data_ptr(), pc.data_ptr(), boxes.data_ptr(), B, n, 8, 0, st)
        k0 = sum(NREAL // len(STRIDES) + (1 if j < NREAL % len(STRIDES) else 0) for j in range(l))
        gt[:, k0:k0 + take] = (boxes[bid, pickd, :8] + 0.2).cpu()
        inbox = rnd(B, n) < 0.1
        inbox[bi, pick] = True
        train["pc_vehicle_frame_s%d" % s] = pc
        train["range_image_mask_s%d" % s] = (rnd(B, 1, H, Wl) >= 0.15).float().to(dev)
        w = torch.tensor([3., 1, 1, 1, 1, 1, 1, 1])[None, :, None] * inbox[:, None, :]
        nw = (inbox / torch.randint(1, 50, (B, n), generator=g))[:, None, :].repeat(1, 8, 1)
        u = torch.where(rnd(B, n, 8) < 0.5, rnd(B, n, 8) * 0.1 - 0.05, rnd(B, n, 8) * 4 - 2).to(dev)
        train["rpn_reg_target_s%d" % s] = (lv + u).permute(0, 2, 1).reshape(B, 8, H, Wl).contiguous()
        train["rpn_reg_weight_s%d" % s] = w.reshape(B, 8, H, Wl).contiguous().to(dev)
        train["reg_normalize_weight_s%d" % s] = nw.reshape(B, 8, H, Wl).contiguous().to(dev)
        off += n
    train["gt_bbox_veh_for_iou_pred"] = gt.to(dev)
    return logits, deltas, train


class TorchRoute:
    """What a user of the library had before rd_rpn_loss: two library launches per level for the IoU target, the rest in torch."""

    def __init__(self, L, st, P, B):
        self.L, self.st, self.P = L, st, P
        self.boxes = {s: None for s in STRIDES}
        self.B = B

    def level(self, x, d, pc, gt, m, t, w, nw, s):
        L, P, B, n = self.L, self.P, self.B, x.shape[1]
        if self.boxes[s] is None:
            self.boxes[s] = (torch.empty(B, n, 10, device=x.device), torch.empty(B, n, device=x.device))
        boxes, iou = self.boxes[s]
        L.call("rd_decode3d_bbox", d.data_ptr(), pc.data_ptr(), boxes.data_ptr(), B, n, 8, 0, self.st)
        L.call("rd_batch_rotated_iou", boxes.data_ptr(), 10, gt.data_ptr(), iou.data_ptr(), None, B, n, gt.shape[1], self.st)
        lo, hi = 1e-6, float(np.float32(1) - np.float32(1e-6))
        p = torch.sigmoid(x)
        ge = x >= 0
        Lm = torch.where(ge, -x, torch.zeros_like(x)) - torch.log1p(torch.exp(torch.where(ge, -x, x)))
        L0 = -1.0 * (0.5 * iou * torch.log(p.clamp(lo, hi)) + 0.5 * (1 - iou) * Lm) * 2.0
        c = ((p >= lo) & (p <= hi)).float()
        dL0 = -(iou * c * (1 - p) - (1 - iou) * p)
        pos = iou > 0
        vfl = torch.where(pos, L0 * iou, L0 * P.alpha * p ** P.gamma)
        dvfl = torch.where(pos, iou * dL0, P.alpha * (dL0 * p ** P.gamma + L0 * P.gamma * p ** (P.gamma - 1) * p * (1 - p)))
        norm_cls, norm_reg = m.sum() + 1, nw.sum() + 1
        cls_loss = vfl * m / norm_cls
        d_logit = P.scale_loss_shift * P.cls_loss_weight * m / norm_cls * dvfl
        xr = d.permute(0, 2, 1) - t
        sig2 = P.smooth_l1_scalar ** 2
        inside = xr.abs() < 1 / sig2
        sl1 = torch.where(inside, 0.5 * sig2 * xr * xr, xr.abs() - 0.5 / sig2)
        dsl1 = torch.where(inside, sig2 * xr, torch.sign(xr))
        reg_loss = sl1 * w * nw / norm_reg * P.reg_loss_weight
        d_delta = (P.scale_loss_shift * P.reg_loss_weight * w * nw / norm_reg * dsl1).permute(0, 2, 1).contiguous()
        return cls_loss, reg_loss, d_logit, d_delta, iou, cls_loss.sum(), reg_loss.sum()

    def __call__(self, logits, deltas, train):
        out, off = {}, 0
        for s in STRIDES:
            m = train["range_image_mask_s%d" % s]
            B, _, Hh, Wl = m.shape
            n = Hh * Wl
            out[s] = self.level(logits[:, off:off + n], deltas[:, off:off + n].contiguous(), train["pc_vehicle_frame_s%d" % s],
                                train["gt_bbox_veh_for_iou_pred"], m.reshape(B, n), train["rpn_reg_target_s%d" % s].reshape(B, 8, n),
                                train["rpn_reg_weight_s%d" % s].reshape(B, 8, n), train["reg_normalize_weight_s%d" % s].reshape(B, 8, n), s)
            off += n
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_timing.json"))
    a = ap.parse_args()
    A, L = TorchAllocator(), rdlib.get_lib()
    dev, st, B = A.device, A.stream, a.batch
    logits, deltas, train = make_inputs(B, dev, L, st)
    fused = RpnLoss(lib=L, alloc=A)
    P = fused.param
    route = TorchRoute(L, st, P, B)
    run_fused, run_torch = (lambda: fused(logits, deltas, train)), (lambda: route(logits, deltas, train))
    # the same results first (the torch route decodes in a kernel of its own: the same operations, so the IoU targets agree bit for bit
    # unless the compiler contracted one of the two decodes differently)
    f, t = run_fused(), run_torch()
    torch.cuda.synchronize()
    agree, off = {}, 0
    for s in STRIDES:
        cls, reg, dl, dd, iou, _, _ = t[s]
        n = iou.shape[1]
        same = (f["iou_target_s%d" % s].reshape(B, n) - iou).abs() < 1e-5
        rel = lambda g, w: float(((g - w).abs() / (w.abs() + 1e-12))[w.abs() > 1e-9].max().cpu()) if (w.abs() > 1e-9).any() else 0.0   # noqa: E731
        agree["s%d" % s] = dict(
            iou_pixels_beyond_1e_5=int((~same).sum().cpu()), positives=int((iou > 0).sum().cpu()),
            cls_loss_rel=rel(f["rpn_cls_loss_s%d" % s].reshape(B, n)[same], cls[same]),
            reg_loss_rel=rel(f["rpn_reg_loss_s%d" % s].reshape(B, 8, n), reg),
            d_delta_rel=rel(f["d_delta"][:, off:off + n], dd),
            d_logit_max_abs=float((f["d_logit"][:, off:off + n][same] - dl[same]).abs().max().cpu()))
        off += n
    for _ in range(3):
        run_fused(), run_torch()
    torch.cuda.synchronize()
    med, raw = series({"fused": run_fused, "torch": run_torch}, a.iters, a.repeats)
    res = dict(tool="tools/loss_timing.py", source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), batch=B, shape=[H, WP],
               strides=list(STRIDES), n_gt=NGT, real_boxes=NREAL, iters=a.iters, repeats=a.repeats, series=raw,
               fused_ms=med["fused"], torch_route_ms=med["torch"], torch_over_fused=med["torch"] / med["fused"], agreement=agree)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

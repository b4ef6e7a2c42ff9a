"""float64 NumPy restatement of the RPN loss head, from the reference lines it replaces (all relative to the reference tree):
rangedet/symbol/head/loss.py:4-30 (sigmoid_bce_loss_with_logits, vari_focal_loss), rangedet/symbol/head/builder.py:350-379 (get_vfl_loss),
:381-422 (get_normalize_reg_loss), and what MakeLoss with grad_scale sends back (:374-378,417-421).  It takes float32 inputs and a GIVEN
IoU-target map (the target itself is checked against the oracle's decode and IoU, tests/test_loss.py).  TEST INFRASTRUCTURE ONLY.

MXNet is not installed; the operator semantics restated here are unpinned: smooth_l1(x, scalar = sigma) = 0.5 (sigma x)^2 for
|x| < 1 / sigma^2, else |x| - 0.5 / sigma^2; the gradient of clip is 1 on the closed interval; softrelu(x) = log(1 + exp(x)); MakeLoss
forward is the identity and its backward is grad_scale."""
import numpy as np

F64 = np.float64
# the float32 values MXNet's clip holds for a_min = 1e-6, a_max = 1 - 1e-6
CLIP_LO, CLIP_HI = float(np.float32(1e-6)), float(np.float32(1.0) - np.float32(1e-6))
DEFAULT = dict(alpha=1.0, gamma=2.0, cls_loss_weight=10.0, reg_loss_weight=8.0, smooth_l1_scalar=3.0, scale_loss_shift=128.0, l1=0)


def varifocal(x, s, alpha, gamma):
    """loss.py:4-30 with loss_scale = 1: (vfl, d vfl / d x); s (the score) is behind block_grad, pred_sigmoid is not."""
    x, s = np.asarray(x, F64), np.asarray(s, F64)
    p = 1.0 / (1.0 + np.exp(-x))                                            # :5, :23
    ge = x >= 0                                                             # :6
    Lm = np.where(ge, -x, 0.0) - np.log1p(np.exp(np.where(ge, -x, x)))      # :7-12
    Lp = np.log(np.clip(p, CLIP_LO, CLIP_HI))                               # :14
    L0 = -1.0 * (0.5 * s * Lp + 0.5 * (1.0 - s) * Lm) * 2.0                 # :13-18 with alpha = 0.5, then :24
    c = ((p >= CLIP_LO) & (p <= CLIP_HI)).astype(F64)
    dL0 = -(s * c * (1.0 - p) - (1.0 - s) * p)
    pos = s > 0                                                             # :25-29
    vfl = np.where(pos, L0 * s, L0 * alpha * np.abs(s - p) ** gamma)
    dvfl = np.where(pos, s * dL0, alpha * (dL0 * p ** gamma + L0 * gamma * p ** (gamma - 1.0) * p * (1.0 - p)))
    return vfl, dvfl


def loss_model(logit, iou, mask, delta, target, weight, norm_weight, P=DEFAULT):
    """logit, iou, mask (B,n); delta (B,n,8); target, weight, norm_weight (B,8,n).  float64 results:
    norm_cls, norm_reg, cls_loss (B,n), reg_loss (B,8,n), d_logit (B,n), d_delta (B,n,8), sum_cls, sum_reg."""
    x, s, m = (np.asarray(a, F64) for a in (logit, iou, mask))
    d, t, w, nw = (np.asarray(a, F64) for a in (delta, target, weight, norm_weight))
    norm_cls, norm_reg = m.sum() + 1.0, nw.sum() + 1.0                      # builder.py:366, :411 (over the whole batch)
    vfl, dvfl = varifocal(x, s, float(P["alpha"]), float(P["gamma"]))
    cls_loss = vfl * m / norm_cls                                           # :371-372
    d_logit = P["scale_loss_shift"] * P["cls_loss_weight"] * m / norm_cls * dvfl       # :374-376
    xr = d.transpose(0, 2, 1) - t                                           # channel c of pixel i pairs with target[b, c, i]
    sig2 = float(P["smooth_l1_scalar"]) ** 2
    if P["l1"]:                                                             # :397-401
        sl1, dsl1 = np.abs(xr), np.sign(xr)
    else:                                                                   # :403-407
        inside = np.abs(xr) < 1.0 / sig2
        sl1 = np.where(inside, 0.5 * sig2 * xr * xr, np.abs(xr) - 0.5 / sig2)
        dsl1 = np.where(inside, sig2 * xr, np.sign(xr))
    reg_loss = sl1 * w * nw / norm_reg * P["reg_loss_weight"]               # :413-416
    d_delta = (P["scale_loss_shift"] * P["reg_loss_weight"] * w * nw / norm_reg * dsl1).transpose(0, 2, 1)   # :417-419
    return dict(norm_cls=norm_cls, norm_reg=norm_reg, cls_loss=cls_loss, reg_loss=reg_loss, d_logit=d_logit, d_delta=d_delta,
                sum_cls=cls_loss.sum(), sum_reg=reg_loss.sum())

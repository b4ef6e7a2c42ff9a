"""Restatement of the residual batch norm, the 1x1 weight gradient and a whole backbone BasicBlock in training mode (include/rangedet_hip.h:
rd_affine_add_relu, rd_bn_add_relu_bwd, rd_conv1x1_bwd_weight; rangedet_amd.backbone_train), with the bounds the tests hold the launches
to.  Plain module, imported by test_basic_block_train.py; built on norm_model.py and convbwd_model.py, which it does not change.
Activations are (n, C) or (B, H, W, C) arrays of values already rounded to the 16-bit type; n = B H W.  Nothing here looks at a kernel's
output to size a tolerance.

Exact restatements (float32, compared bit for bit):
  add_pre_f32       v = fma32(z, a, b) + u with u = r (identity shortcut) or fma32(r, ar, br) (projection): two or three roundings, the
                    sum one of its own
  add_relu_f32      h16_round(max(v, 0)), rd_affine_add_relu
  add_mask_f32      [v > 0], the mask rd_bn_add_relu_bwd recomputes
Backward (bn_add_bwd): norm_model.bn_bwd on that mask, and for a projection zhr = (r - mean_r) rstd_r, dgamma_r = sum gy zhr with the sum
of the absolute terms; dbeta_r is dbeta.  Bounds, as in norm_model:
  dbeta, dgamma, dgamma_r    convbwd_model.sum_bound(n, sum |terms|)
  dz, projection dr          norm_model.bn_dz on zh (zhr) and the launch's own sums: half an ulp of the type + DZ_K u |gr| (|gy| + |c1| + |zh c2|)
  identity dr                the bits of g where the mask is set, +0 elsewhere
1x1 weight gradient (weight_grad1x1): a float64 einsum over the pixels, held to sum_bound(n, sum |dz x|); parts1x1 is the number of partial
sums the launch reports: min(split or min(512, ceil(tiles / 8)), tiles) with tiles = ceil(n / 64).
block_backward: the whole block in float64, forward and backward, for the comparison with torch.autograd."""
import numpy as np

import norm_model as N
from emu_util import h16_round

F32 = np.float32
PT, MIN_CHUNKS, WG_TARGET = 64, 8, 512        # k_convbwd.h BW_PT, BW1_MIN_CHUNKS, BW_WG_TARGET


def add_pre_f32(z, a, b, r, ar=None, br=None):
    t = N.fma32(z, a, b)
    u = np.asarray(r, F32) if ar is None else N.fma32(r, ar, br)
    return (t + u).astype(F32)


def add_relu_f32(z, a, b, r, ar, br, dt, relu=True):
    v = add_pre_f32(z, a, b, r, ar, br)
    return h16_round(np.maximum(v, F32(0)) if relu else v, dt)


def add_mask_f32(z, a, b, r, ar=None, br=None):
    return add_pre_f32(z, a, b, r, ar, br) > 0


def bn_add_bwd(g, z, r, mask, mean, rstd, mean_r=None, rstd_r=None):
    """norm_model.bn_bwd, and with mean_r / rstd_r also zhr (n, C), dgamma_r, dgamma_r_abs (C)"""
    m = N.bn_bwd(g, z, mask, mean, rstd)
    if mean_r is not None:
        zhr = (np.asarray(r, np.float64) - np.asarray(mean_r, np.float64)) * np.asarray(rstd_r, np.float64)
        m.update(zhr=zhr, dgamma_r=(m["gy"] * zhr).sum(0), dgamma_r_abs=np.abs(m["gy"] * zhr).sum(0))
    return m


def bn_dr(m, gamma_r, rstd_r, dgamma_r, dbeta, n):
    """the projection's dr: norm_model.bn_dz with zhr in the place of zh -> (v, the sum the tolerance scales with)"""
    return N.bn_dz(dict(gy=m["gy"], zh=m["zhr"]), gamma_r, rstd_r, dgamma_r, dbeta, n)


def parts1x1(npix, split):
    tiles = -(-npix // PT)
    cap = split if split > 0 else min(WG_TARGET, -(-tiles // MIN_CHUNKS))
    return min(tiles, cap)


def weight_grad1x1(x, dz, want_abs=True):
    """-> dW (cout, cin) float64, sum |dz x| of the same shape (None without want_abs), the number of terms n"""
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    x2, z2 = x.reshape(-1, x.shape[-1]), dz.reshape(-1, dz.shape[-1])
    dW = np.einsum("po,pi->oi", z2, x2)
    return dW, (np.einsum("po,pi->oi", np.abs(z2), np.abs(x2)) if want_abs else None), x2.shape[0]


def _conv3(v, k):
    B, H, W = v.shape[:3]
    vp = np.zeros((B, H + 2, W + 2, v.shape[3]))
    vp[:, 1:-1, 1:-1] = v
    return sum(vp[:, i:i + H, j:j + W] @ k[:, :, i, j].T for i in range(3) for j in range(3))


def _bn(z, gamma, beta, eps):
    mean, var = N.stats(z)
    rstd = 1.0 / np.sqrt(var + eps)
    return mean, rstd, (z - mean) * rstd * gamma + beta


def block_backward(x, w1, bn1, w2, bn2, eps, g, ws=None, bns=None):
    """One BasicBlock in float64: x (B, H, W, cin), w1 (cout, cin, 3, 3), w2 (cout, cout, 3, 3), ws (cout, cin) or None, bn* = (gamma, beta),
    g = dL/dy -> dict y, pre (the pre-activations of both ReLUs, for the tie check), dx and the gradients by their short names.
      y1 = relu(BN1(conv1 x));  v = BN2(conv2 y1) + u,  u = x or BNs(conv1x1 x);  y = relu(v)          (add BEFORE the last ReLU)
      gy = g [v > 0] feeds BN2's backward AND the shortcut: dr = gy (identity), or BNs's backward of gy on zs (projection), whose
      dbeta is BN2's dbeta"""
    from convbwd_model import flip_weight, weight_grad
    x, w1, w2, g = (np.asarray(v, np.float64) for v in (x, w1, w2, g))
    B, H, W, cin = x.shape
    cout = w1.shape[0]
    n = B * H * W
    z1 = _conv3(x, w1).reshape(n, cout)
    mean1, rstd1, t1 = _bn(z1, bn1[0], bn1[1], eps)
    y1 = np.maximum(t1, 0.0)
    z2 = _conv3(y1.reshape(B, H, W, cout), w2).reshape(n, cout)
    mean2, rstd2, t2 = _bn(z2, bn2[0], bn2[1], eps)
    if ws is None:
        u = x.reshape(n, cin)
    else:
        ws = np.asarray(ws, np.float64)
        zs = x.reshape(n, cin) @ ws.T
        means, rstds, u = _bn(zs, bns[0], bns[1], eps)
    v = t2 + u
    y = np.maximum(v, 0.0)
    mask = v > 0
    g2 = g.reshape(n, cout)
    out = dict(y=y.reshape(B, H, W, cout), pre=np.concatenate([t1.ravel(), v.ravel()]))
    if ws is None:
        m2 = bn_add_bwd(g2, z2, None, mask, mean2, rstd2)
        dshort = m2["gy"]
    else:
        m2 = bn_add_bwd(g2, z2, zs, mask, mean2, rstd2, means, rstds)
        dr = bn_dr(m2, bns[0], rstds, m2["dgamma_r"], m2["dbeta"], n)[0]
        out.update(sc_bn_gamma=m2["dgamma_r"], sc_bn_beta=m2["dbeta"], sc_weight=dr.T @ x.reshape(n, cin))
        dshort = dr @ ws
    dz2 = N.bn_dz(m2, bn2[0], rstd2, m2["dgamma"], m2["dbeta"], n)[0].reshape(B, H, W, cout)
    g1 = _conv3(dz2, flip_weight(w2)).reshape(n, cout)
    m1 = N.bn_bwd(g1, z1, t1 > 0, mean1, rstd1)
    dz1 = N.bn_dz(m1, bn1[0], rstd1, m1["dgamma"], m1["dbeta"], n)[0].reshape(B, H, W, cout)
    out.update(bn2_gamma=m2["dgamma"], bn2_beta=m2["dbeta"], conv2_weight=weight_grad(y1.reshape(B, H, W, cout), dz2, want_abs=False)[0],
               bn1_gamma=m1["dgamma"], bn1_beta=m1["dbeta"], conv1_weight=weight_grad(x, dz1, want_abs=False)[0],
               dx=_conv3(dz1, flip_weight(w1)) + dshort.reshape(B, H, W, cin))
    return out

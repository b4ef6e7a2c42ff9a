"""Restatement of an aggregation stage in training mode (include/rangedet_hip.h: rd_deconv_bwd_weight, rd_pack_deconv_data_grad_host,
rd_pack_deconv_dev, rd_affine_relu_add; rangedet_amd.backbone_train.AggStageTrain), with what the tests hold the launches to.  Plain module,
imported by test_agg_stage_train.py; built on norm_model.py and convbwd_model.py, which it does not change.  Activations are (B, H, W, C)
arrays of values already rounded to the 16-bit type.  The transposed conv has kernel (3, KW), stride (1, s), pad (1, p) with KW - 2 p == s:
x is (B, H, Win, Cin), W (Cin, Cout, 3, KW) in MXNet's Deconvolution layout, z and dz (B, H, s Win, Cout).  Nothing here looks at a
kernel's output to size a tolerance.

  deconv            z[b,hi-1+kh,s wi-p+kw,co] += x[b,hi,wi,ci] W[ci,co,kh,kw]                    float64 scatter
  weight_grad       dW[ci,co,kh,kw] = sum_{b,hi,wi} x[b,hi,wi,ci] dz[b,hi-1+kh,s wi-p+kw,co] (dz zero outside the image), the sum of the
                    absolute products, and the number of terms per tap (tap_terms); held to convbwd_model.sum_bound
  parts             the partial sums rd_deconv_bwd_weight reports: min(split or 512 / (KW Cin / 64), chunks), chunks = B ceil(H / 16)
                    ceil(Win / 64) counted on the x grid
  data_grad         dx[b,hi,wi,ci] = sum_{co,kh,kw} dz[b,hi-1+kh,s wi-p+kw,co] W[ci,co,kh,kw], float64; the launch rounds the weight to the
                    type first, the caller passes it rounded; held to conv_model.conv_tol
  view_weight       Wv (Cin, s Cout, 3, 3) with Wv[ci, e Cout + co, kh, dwv + 1] = W[ci,co,kh, s dwv + e + p] where that column exists, else
                    0: the weight of the 3x3 stride-1 conv over dz read as (B, H, Win, s Cout) that the data gradient's launch is
  relu_add_f32      h16_round(max(fma32(z, a, b), 0) + r) with max(t, 0) = t where t > 0, else +0: rd_affine_relu_add's exact result
  stage_backward    the whole stage without its res stage in float64, forward and backward, for the comparison with torch.autograd"""
import numpy as np

import norm_model as N
from emu_util import h16_round

F32 = np.float32
PT, RH, WG_TARGET = 64, 16, 512        # k_convbwd.h BW_PT, BW_RH, BW_WG_TARGET
FORMS = {4: (2, 1), 8: (4, 2)}         # KW -> (s, p)


def _cols(kw, s, p, Win):
    """the padded-image columns tap column kw pairs with the input columns 0 .. Win - 1: s wi - p + kw, shifted by the left pad p"""
    return slice(kw, kw + s * Win, s)


def _padded(B, H, Win, C, KW, s, p):
    return np.zeros((B, H + 2, s * Win + KW, C))     # rows -1 .. H, columns -p .. s Win + KW - p - 1


def deconv(x, w, s, p):
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, H, Win, _ = x.shape
    KW = w.shape[3]
    zp = _padded(B, H, Win, w.shape[1], KW, s, p)
    for kh in range(3):
        for kw in range(KW):
            zp[:, kh:kh + H, _cols(kw, s, p, Win)] += x @ w[:, :, kh, kw]
    return zp[:, 1:1 + H, p:p + s * Win]


def _pad_dz(dz, KW, s, p):
    B, H, Wout, C = dz.shape
    zp = _padded(B, H, Wout // s, C, KW, s, p)
    zp[:, 1:1 + H, p:p + Wout] = dz
    return zp


def tap_terms(B, H, Win, KW, s, p):
    """terms of tap (kh, kw): the (hi, wi) whose output pixel (hi - 1 + kh, s wi - p + kw) lies in the image"""
    cols = [sum(1 for wi in range(Win) if 0 <= s * wi - p + kw < s * Win) for kw in range(KW)]
    return np.array([[B * (H - abs(kh - 1)) * c for c in cols] for kh in range(3)], np.int64)


def weight_grad(x, dz, KW, s, p, want_abs=True):
    """-> dW (Cin, Cout, 3, KW) float64, sum |x dz| of the same shape (None without want_abs), tap_terms"""
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    B, H, Win, cin = x.shape
    cout = dz.shape[3]
    assert dz.shape[:3] == (B, H, s * Win) and KW - 2 * p == s
    zp = _pad_dz(dz, KW, s, p)
    dW, sabs = np.zeros((cin, cout, 3, KW)), np.zeros((cin, cout, 3, KW)) if want_abs else None
    xt, axt = x.reshape(-1, cin).T, np.abs(x).reshape(-1, cin).T
    for kh in range(3):
        for kw in range(KW):
            zs = zp[:, kh:kh + H, _cols(kw, s, p, Win)].reshape(-1, cout)
            dW[:, :, kh, kw] = xt @ zs
            if want_abs:
                sabs[:, :, kh, kw] = axt @ np.abs(zs)
    return dW, sabs, tap_terms(B, H, Win, KW, s, p)


def parts(B, H, Win, cin, KW, split):
    chunks = B * -(-H // RH) * -(-Win // PT)
    cap = split if split > 0 else WG_TARGET // (KW * (cin // 64))
    return min(chunks, cap)


def data_grad(dz, w, s, p):
    """dz (B, H, s Win, Cout), w (Cin, Cout, 3, KW) -> dx (B, H, Win, Cin) float64"""
    dz, w = np.asarray(dz, np.float64), np.asarray(w, np.float64)
    B, H, Wout, _ = dz.shape
    KW, Win = w.shape[3], Wout // s
    zp = _pad_dz(dz, KW, s, p)
    return sum(zp[:, kh:kh + H, _cols(kw, s, p, Win)] @ w[:, :, kh, kw].T for kh in range(3) for kw in range(KW))


def view_weight(w, s, p):
    w = np.asarray(w, F32)
    cin, cout, _, KW = w.shape
    wv = np.zeros((cin, s * cout, 3, 3), F32)
    for e in range(s):
        for d in range(3):
            kx = s * (d - 1) + e + p
            if 0 <= kx < KW:
                wv[:, e * cout:(e + 1) * cout, :, d] = w[:, :, :, kx]
    return wv


def relu_add_f32(z, a, b, r, dt):
    t = N.fma32(z, a, b)
    return h16_round((np.where(t > 0, t, F32(0)).astype(F32) + np.asarray(r, F32)).astype(F32), dt)


def stage_backward(skip, up, w, bn, eps, g, s, p):
    """Deconvolution -> BatchNorm (batch statistics) -> ReLU -> add(skip, .) in float64: up (B, H, Win, Cin), skip and g = dL/dt (B, H, s Win,
    Cout), w (Cin, Cout, 3, KW), bn = (gamma, beta) -> dict t, pre (the pre-activations), d_skip, d_up and the gradients by short name"""
    skip, up, w, g = (np.asarray(v, np.float64) for v in (skip, up, w, g))
    B, H, Win, _ = up.shape
    cout, KW = w.shape[1], w.shape[3]
    n = B * H * s * Win
    z = deconv(up, w, s, p).reshape(n, cout)
    mean, var = N.stats(z)
    rstd = 1.0 / np.sqrt(var + eps)
    pre = (z - mean) * rstd * bn[0] + bn[1]
    t = np.maximum(pre, 0.0).reshape(skip.shape) + skip
    m = N.bn_bwd(g.reshape(n, cout), z, pre > 0, mean, rstd)
    dz = N.bn_dz(m, bn[0], rstd, m["dgamma"], m["dbeta"], n)[0].reshape(B, H, s * Win, cout)
    return dict(t=t, pre=pre, d_skip=g, d_up=data_grad(dz, w, s, p), deconv_weight=weight_grad(up, dz, KW, s, p, want_abs=False)[0],
                deconv_bn_gamma=m["dgamma"], deconv_bn_beta=m["dbeta"], dz=dz)

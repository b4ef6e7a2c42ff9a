"""float64 restatement of the head-tower backward primitives (include/rangedet_hip.h: rd_relu_affine_bwd, rd_conv3x3_bwd_weight,
rd_head_out_bwd, and the data gradient as the forward launch on the flipped weight).  Plain module, imported by test_conv_backward.py.
Activations are channels-last (B, H, W, C) arrays of values already rounded to the 16-bit type.  No tiling, no fragment order, and nothing
here looks at a kernel's output to size a tolerance.

  relu_affine_bwd   h16_round(float32(g) * float32(s)) where y > 0, +0 elsewhere: the launch's exact result
  weight_grad       dW (cout, cin, 3, 3), the sum of the absolute products, and the number of terms per tap
  tap_terms         B (H - |dh|) (W - |dw|): the terms of a tap, fewer than B H W off the centre
  flip_weight       (cout, cin, 3, 3) -> (cin, cout, 3, 3) with the taps flipped: the data gradient is conv_model.conv_ref64 of it
  head_out_bwd      dx before mask and scale, dw, dbias, each with the sum of the absolute products
  sum_bound         2 n u sum |terms|, u = 2^-24: any order of n float32 additions of float32-rounded products stays within n u sum |terms|
                    to first order; the factor 2 is for the MFMA's internal multi-term adder, which is not specified as rounding to
                    nearest per addition
"""
import numpy as np

from emu_util import h16_round

U = 2.0 ** -24


def relu_affine_bwd(g, y, s, dt):
    g = np.asarray(g, np.float32)
    v = g if s is None else g * np.asarray(s, np.float32)       # one float32 product
    r = h16_round(v.astype(np.float32), dt)
    return r if y is None else np.where(np.asarray(y) > 0, r, np.float32(0.0)).astype(np.float32)


def tap_terms(B, H, W):
    return np.array([[B * (H - abs(dh)) * (W - abs(dw)) for dw in (-1, 0, 1)] for dh in (-1, 0, 1)], np.int64)


def weight_grad(x, dz, want_abs=True):
    """-> dW (cout, cin, 3, 3) float64, sum |dz x| of the same shape (None without want_abs), tap_terms"""
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    B, H, W, cin = x.shape
    cout = dz.shape[3]
    xp = np.zeros((B, H + 2, W + 2, cin))
    xp[:, 1:-1, 1:-1] = x
    dW, sabs = np.zeros((cout, cin, 3, 3)), np.zeros((cout, cin, 3, 3)) if want_abs else None
    zt, azt = dz.reshape(-1, cout).T, np.abs(dz).reshape(-1, cout).T
    for dh in (-1, 0, 1):
        for dw in (-1, 0, 1):
            xs = xp[:, 1 + dh:1 + dh + H, 1 + dw:1 + dw + W].reshape(-1, cin)
            dW[:, :, dh + 1, dw + 1] = zt @ xs
            if want_abs:
                sabs[:, :, dh + 1, dw + 1] = azt @ np.abs(xs)
    return dW, sabs, tap_terms(B, H, W)


def flip_weight(w):
    return np.ascontiguousarray(np.asarray(w).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def head_out_bwd(d_out, x, w):
    """d_out (B, P, nout) float32 values, x (B, P, cin), w (nout, cin) -> dict of float64: dx, dx_abs (B, P, cin), dw, dw_abs (nout, cin),
    dbias, dbias_abs (nout)"""
    d, x, w = np.asarray(d_out, np.float64), np.asarray(x, np.float64), np.asarray(w, np.float64)
    nout, cin = w.shape
    d2, x2 = d.reshape(-1, nout), x.reshape(-1, cin)
    return dict(dx=(d2 @ w).reshape(x.shape), dx_abs=(np.abs(d2) @ np.abs(w)).reshape(x.shape), dw=d2.T @ x2, dw_abs=np.abs(d2).T @ np.abs(x2),
                dbias=d2.sum(0), dbias_abs=np.abs(d2).sum(0))


def sum_bound(n, sabs):
    return 2.0 * np.asarray(n, np.float64) * U * np.asarray(sabs, np.float64)

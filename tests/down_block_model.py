"""Restatement of the stride-(1,2) BasicBlock in training mode (include/rangedet_hip.h: rd_conv3x3_bwd_weight_ex, the strided images of
rd_sgd_tensor_t; rangedet_amd.backbone_train.DownBlockTrain), with what the tests hold the launches to.  Plain module, imported by
test_down_block_train.py; built on block_model.py, norm_model.py and convbwd_model.py, which it does not change.  Activations are
(B, H, W, C) arrays of values already rounded to the 16-bit type.  x is (B, H, Win, cin) with Win even, Wo = Win / 2.  Nothing here looks
at a kernel's output to size a tolerance.

  conv3_s2          z[b,h,wo,co] = sum x[b,h+ky-1,2wo+kx-1,ci] W[co,ci,ky,kx]                 float64, x zero outside the image
  weight_grad_s2    dW[co,ci,ky,kx] = sum_{b,h,wo} dz[b,h,wo,co] x[b,h+ky-1,2wo+kx-1,ci], the sum of the absolute products, and the number
                    of terms per tap (tap_terms_s2: the column kx = 0 misses wo = 0, the rows ky = 0 / 2 miss one row); held to
                    convbwd_model.sum_bound
  parts3x3          the partial sums rd_conv3x3_bwd_weight(_ex) reports: min(split or 512 / (3 cout / 64), chunks) with chunks =
                    B ceil(H / 16) ceil(Wd / 64) counted on the dz grid, Wd = Win / stride_w
  data_grad_s2      g1[b,h,w,ci] = sum over (wo, kx) with 2wo+kx-1 = w, ky, co of dz[b,h-ky+1,wo,co] W[co,ci,ky,kx]: a scatter of every dz pixel,
                    float64; the launch rounds the weight to the type first, the caller passes it rounded; held to conv_model.conv_tol
  deconv_weight     W (cout, cin, 3, 3) -> the (Cin, Cout, 3, 4) transposed-conv weight the data gradient's launch is given: W unchanged with a
                    zero column at kx = 3
  table_v11         the optimizer table as the library wrote it before rd_sgd_tensor_t had stride_w (k_optim.h: header, entries, element
                    chunks, image chunks), from the eleven fields of each tensor: a table of entries without a stride must still be these
                    bytes
  block_backward    the whole strided block in float64, forward and backward, for the comparison with torch.autograd"""
import struct

import numpy as np

import block_model as BM
import norm_model as N

F32 = np.float32
PT, RH, WG_TARGET = 64, 16, 512        # k_convbwd.h BW_PT, BW_RH, BW_WG_TARGET


def _pad(x):
    B, H, W, C = x.shape
    xp = np.zeros((B, H + 2, W + 2, C))
    xp[:, 1:-1, 1:-1] = x
    return xp


def conv3_s2(x, w):
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, H, W, _ = x.shape
    xp = _pad(x)
    return sum(xp[:, ky:ky + H, kx:kx + W:2] @ w[:, :, ky, kx].T for ky in range(3) for kx in range(3))


def tap_terms_s2(B, H, Win):
    Wo = Win // 2
    return np.array([[B * (H - abs(ky - 1)) * (Wo - (1 if kx == 0 else 0)) for kx in range(3)] for ky in range(3)], np.int64)


def weight_grad_s2(x, dz, want_abs=True):
    """-> dW (cout, cin, 3, 3) float64, sum |dz x| of the same shape (None without want_abs), tap_terms_s2"""
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    B, H, Win, cin = x.shape
    cout = dz.shape[3]
    assert Win % 2 == 0 and dz.shape[:3] == (B, H, Win // 2)
    xp = _pad(x)
    dW, sabs = np.zeros((cout, cin, 3, 3)), np.zeros((cout, cin, 3, 3)) if want_abs else None
    zt, azt = dz.reshape(-1, cout).T, np.abs(dz).reshape(-1, cout).T
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, ky:ky + H, kx:kx + Win:2].reshape(-1, cin)
            dW[:, :, ky, kx] = zt @ xs
            if want_abs:
                sabs[:, :, ky, kx] = azt @ np.abs(xs)
    return dW, sabs, tap_terms_s2(B, H, Win)


def parts3x3(B, H, Wd, cout, split):
    chunks = B * -(-H // RH) * -(-Wd // PT)
    cap = split if split > 0 else WG_TARGET // (3 * (cout // 64))
    return min(chunks, cap)


def data_grad_s2(dz, w):
    """dz (B, H, Wo, cout), w (cout, cin, 3, 3) -> g1 (B, H, 2 Wo, cin) float64"""
    dz, w = np.asarray(dz, np.float64), np.asarray(w, np.float64)
    B, H, Wo, _ = dz.shape
    gp = np.zeros((B, H + 2, 2 * Wo + 2, w.shape[1]))
    for ky in range(3):
        for kx in range(3):
            gp[:, ky:ky + H, kx:kx + 2 * Wo:2] += dz @ w[:, :, ky, kx]
    return gp[:, 1:-1, 1:-1]


def deconv_weight(w):
    w = np.asarray(w, F32)
    wd = np.zeros(w.shape[:2] + (3, 4), F32)
    wd[..., :3] = w
    return wd


# ---- the optimizer table before stride_w -------------------------------------------------------------------------------------------------------
SGD_CHUNK, SGD_PACK_SLOTS, SGD_MAGIC, CONV_TAIL = 1024, 256, 0x52445347, 256


def table_v11(tensors, dtype):
    """tensors: dicts of the eleven fields (weight, grad, mom, n, lr_mult, wd_mult, cout, cin, pack_fwd, pack_bwd, fold_scale; pointers as
    ints, 0 for NULL) -> the table bytes: SgdHeader (64 bytes: magic, nt, n_chunks, n_pack, dtype, off_entries, off_chunks, off_pack, bytes,
    7 words of padding) | SgdEntry[nt] (w, g, m, n: 8 bytes each; lr_mult, wd_mult, cout, cin: 4 each; fwd, bwd, fold: 8 each) |
    SgdChunk[n_chunks] (tensor, chunk) | SgdPackChunk[n_pack] (tensor, image 0 forward / 1 data gradient, run of 256 slots, 0)"""
    entries, chunks, packs = b"", b"", b""
    for i, t in enumerate(tensors):
        entries += struct.pack("<QQQqffiiQQQ", t["weight"], t["grad"], t["mom"], t["n"], t["lr_mult"], t["wd_mult"], t["cout"], t["cin"],
                               t["pack_fwd"], t["pack_bwd"], t["fold_scale"])
        for k in range(-(-t["n"] // SGD_CHUNK)):
            chunks += struct.pack("<ii", i, k)
        if t["pack_fwd"] or t["pack_bwd"]:
            slots = (t["n"] * 2 + CONV_TAIL) // 16
            per = -(-slots // SGD_PACK_SLOTS)
            for im, key in enumerate(("pack_fwd", "pack_bwd")):
                if t[key]:
                    for k in range(per):
                        packs += struct.pack("<iiii", i, im, k, 0)
    nt, nc, npk = len(tensors), len(chunks) // 8, len(packs) // 16
    off_e = 64
    off_c = off_e + len(entries)
    off_p = off_c + len(chunks)
    total = off_p + len(packs)
    header = struct.pack("<IiiiiIIII", SGD_MAGIC, nt, nc, npk, dtype, off_e, off_c, off_p, total) + b"\0" * 28
    return np.frombuffer(header + entries + chunks + packs, np.uint8)


# ---- the whole block in float64 ------------------------------------------------------------------------------------------------------------------
def block_backward(x, w1, bn1, w2, bn2, eps, g, ws, bns):
    """The strided block in float64: x (B, H, Win, cin), w1 (cout, cin, 3, 3), w2 (cout, cout, 3, 3), ws (cout, cin), bn* = (gamma, beta),
    g = dL/dy (B, H, Wo, cout) -> dict y, pre (the pre-activations of both ReLUs), dx and the gradients by their short names.
      y1 = relu(BN1(conv1 x));  v = BN2(conv2_s2 y1) + BNs(conv1x1 of x's even pixels);  y = relu(v)"""
    from convbwd_model import flip_weight, weight_grad
    x, w1, w2, g, ws = (np.asarray(v, np.float64) for v in (x, w1, w2, g, ws))
    B, H, Win, cin = x.shape
    cout, Wo = w1.shape[0], Win // 2
    n1, n = B * H * Win, B * H * Wo
    z1 = BM._conv3(x, w1).reshape(n1, cout)
    mean1, rstd1, t1 = BM._bn(z1, bn1[0], bn1[1], eps)
    y1 = np.maximum(t1, 0.0).reshape(B, H, Win, cout)
    z2 = conv3_s2(y1, w2).reshape(n, cout)
    mean2, rstd2, t2 = BM._bn(z2, bn2[0], bn2[1], eps)
    xe = x[:, :, 0::2].reshape(n, cin)
    zs = xe @ ws.T
    means, rstds, u = BM._bn(zs, bns[0], bns[1], eps)
    v = t2 + u
    mask = v > 0
    g2 = g.reshape(n, cout)
    out = dict(y=np.maximum(v, 0.0).reshape(B, H, Wo, cout), pre=np.concatenate([t1.ravel(), v.ravel()]))
    m2 = BM.bn_add_bwd(g2, z2, zs, mask, mean2, rstd2, means, rstds)
    dr = BM.bn_dr(m2, bns[0], rstds, m2["dgamma_r"], m2["dbeta"], n)[0]
    dz2 = N.bn_dz(m2, bn2[0], rstd2, m2["dgamma"], m2["dbeta"], n)[0].reshape(B, H, Wo, cout)
    g1 = data_grad_s2(dz2, w2).reshape(n1, cout)
    m1 = N.bn_bwd(g1, z1, t1 > 0, mean1, rstd1)
    dz1 = N.bn_dz(m1, bn1[0], rstd1, m1["dgamma"], m1["dbeta"], n1)[0].reshape(B, H, Win, cout)
    ds = np.zeros((B, H, Win, cin))
    ds[:, :, 0::2] = (dr @ ws).reshape(B, H, Wo, cin)
    out.update(sc_bn_gamma=m2["dgamma_r"], sc_bn_beta=m2["dbeta"], sc_weight=dr.T @ xe, bn2_gamma=m2["dgamma"], bn2_beta=m2["dbeta"],
               conv2_weight=weight_grad_s2(y1, dz2, want_abs=False)[0], bn1_gamma=m1["dgamma"], bn1_beta=m1["dbeta"],
               conv1_weight=weight_grad(x, dz1, want_abs=False)[0], dx=BM._conv3(dz1, flip_weight(w1)) + ds)
    return out

"""float64 restatement of the training-mode batch norm of a head-tower layer (include/rangedet_hip.h: rd_bn_stats, rd_bn_fold, rd_affine_relu,
rd_bn_relu_bwd; the operation order is the one written in rangedet_amd/csrc/k_norm.h), with the error bounds the tests hold the launches
to.  Plain module, imported by test_batch_norm.py.  Activations are (n, C) or (B, H, W, C) arrays of values already rounded to the 16-bit
type; n = B H W.  Nothing here looks at a kernel's output to size a tolerance.  u = 2^-24 (float32 round to nearest).

Exact restatements (float32, compared bit for bit):
  fma32             fmaf: the product of two float32 values is exact in float64, the sum rounds once there and once to float32
  fold_f32          rd_bn_fold, every operation in float32 in the order of the header
  affine_relu_f32   h16_round(max(fma32(z, a, b), 0))
  mask_f32          [fma32(z, a, b) > 0], the mask rd_bn_relu_bwd recomputes

Statistics (stats, stats_bound).  The launch has P = parts(n, split) workgroups; workgroup k owns the pixels [k n / P, (k + 1) n / P),
n_k of them, takes a pilot p_k (the mean of PL = 2048 / C of its pixels, evenly spread) and sums d = z - p_k and d^2.  With D1_k = sum |z - p_k|,
D2_k = sum (z - p_k)^2, s_k = sum (z - p_k) over the run, all exact, to first order in u:
  S1_k   one rounding per subtraction, n_k additions in some order           E1_k = (n_k + 1) u D1_k
  S2_k   d carries u, d^2 2 u; one rounding per fmaf, n_k additions           E2_k = (n_k + 3) u D2_k
  q_k = S1_k / n_k,  m_k = p_k + q_k                                          em_k = E1_k / n_k + u |q_k| + u |m_k|
  M2_k = fmaf(-S1_k, q_k, S2_k)                                               eM_k = E2_k + 2 |q_k| E1_k + u s_k^2 / n_k + u |M2_k|
  A_k = n_k (m_k - m_0)                                                       eA_k = n_k em_k + n_k u |m_k - m_0| + u |A_k|
      (sum_k n_k (m_k - c) / n + c is the mean for ANY c: the error of m_0 itself does not enter)
  mean = m_0 + tree(A) / n     the tree has T = ceil(P / 32) + 5 levels       emean = (sum eA_k + T u sum |A_k|) / n + u |sum A_k / n| + u |mean|
  e_k = m_k - mean                                                            ee_k = em_k + emean + u |e_k|
  B_k = fmaf(n_k e_k, e_k, M2_k)                                              eB_k = eM_k + 2 n_k |e_k| ee_k + 2 u n_k e_k^2 + u |B_k|
  var = tree(B) / n                                                           evar = (sum eB_k + T u sum |B_k|) / n + u var
Both bounds are doubled for the second-order terms (the largest is n_k u times a first-order one; n_k u < 2^-10 below 16384 pixels a run)
and for the pilot, which the launch holds in float32 and this file in float64.  They are in terms of n_k, sum |z - p_k| and sum (z - p_k)^2
per run -- the quantities the one-sweep form depends on -- and, through u |m_k| and u |mean|, of |mean| <= sum |z| / n.
naive_var_f32 is what the launch must NOT compute: E[z^2] - E[z]^2 about zero, float32, added pixel by pixel.

Backward (bn_bwd).  gy = g mask, zh = (z - mean) rstd; dbeta = sum gy, dgamma = sum gy zh with the sums of absolute terms.
  dbeta, dgamma     convbwd_model.sum_bound(n, sum |terms|) = 2 n u sum |terms|: any order of n additions is n u sum |terms|, the factor 2
                    covers the two roundings zh carries into every product and the one of each fmaf (n >= 3)
  dz                v = gr (gy - c1 - zh c2) from the launch's own dgamma, dbeta: c1 = dbeta / n, c2 = dgamma / n, gr = gamma rstd.  Roundings
                    on the way of each term: c1 1 (division), zh c2 3 (two in zh, one in c2); then the subtraction gy - c1, the fmaf, gr and
                    the final product, 1 each: at most 3 + 1 (fmaf) + 1 (gr) + 1 (product) = 6 for zh c2, 5 for c1, 4 for gy ->
                    dz_tol = half an ulp of the type at v + DZ_K u |gr| (|gy| + |c1| + |zh c2|), DZ_K = 6
"""
import numpy as np

from emu_util import h16_round

U = 2.0 ** -24
MIN_PIXELS, MAX_PARTS, KL = 64, 1024, 32      # k_norm.h NM_MIN_PIXELS, NM_MAX_PARTS, NM_KL
DZ_K = 6.0
F32 = np.float32


def parts(n, split):
    return min(split if split > 0 else MAX_PARTS, -(-n // MIN_PIXELS))


def runs(n, P):
    return [(k * n // P, (k + 1) * n // P) for k in range(P)]


def fma32(a, b, c):
    return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64) + np.asarray(c, F32).astype(np.float64)).astype(F32)


def stats(z):
    """z (n, C) -> exact mean and biased variance (float64)"""
    z = np.asarray(z, np.float64)
    m = z.mean(0)
    return m, ((z - m) ** 2).mean(0)


def naive_var_f32(z):
    z = np.asarray(z, F32)
    n = F32(z.shape[0])
    s, ss = np.cumsum(z, axis=0, dtype=F32)[-1], np.cumsum(z * z, axis=0, dtype=F32)[-1]      # cumsum adds sequentially in float32
    m = s / n
    return ss / n - m * m


def stats_bound(z, P):
    """-> (bound on |mean - exact|, bound on |var - exact|) per channel, for the launch with P partial sums (module docstring)"""
    z = np.asarray(z, np.float64)
    n, C = z.shape
    PL = 2048 // C
    mean, var = stats(z)
    rows = []
    for lo, hi in runs(n, P):
        r, nk = z[lo:hi], hi - lo
        p = r[[j * nk // PL for j in range(PL)]].mean(0)
        d = r - p
        D1, D2, s = np.abs(d).sum(0), (d * d).sum(0), d.sum(0)
        E1, E2, q = (nk + 1) * U * D1, (nk + 3) * U * D2, s / nk
        mk, M2 = p + q, D2 - s * q
        rows.append(dict(nk=nk, mk=mk, M2=M2, em=E1 / nk + U * np.abs(q) + U * np.abs(mk),
                         eM=E2 + 2 * np.abs(q) * E1 + U * s * s / nk + U * np.abs(M2)))
    T, m0 = -(-P // KL) + 5, rows[0]["mk"]
    A = [r["nk"] * (r["mk"] - m0) for r in rows]
    eA = sum(r["nk"] * r["em"] + r["nk"] * U * np.abs(r["mk"] - m0) + U * np.abs(a) for r, a in zip(rows, A))
    emean = (eA + T * U * sum(np.abs(a) for a in A)) / n + U * np.abs(sum(A) / n) + U * np.abs(mean)
    eB, sB = 0.0, 0.0
    for r in rows:
        e = r["mk"] - mean
        Bk = r["M2"] + r["nk"] * e * e
        eB = eB + r["eM"] + 2 * r["nk"] * np.abs(e) * (r["em"] + emean + U * np.abs(e)) + 2 * U * r["nk"] * e * e + U * np.abs(Bk)
        sB = sB + np.abs(Bk)
    evar = (eB + T * U * sB) / n + U * var
    return 2 * emean, 2 * evar


def fold_f32(mean, var, gamma, beta, eps, momentum, n, unbiased, moving_mean, moving_var):
    """rd_bn_fold in float32 -> dict rstd, a, b, moving_mean, moving_var"""
    mean, var, gamma, beta, mm, mv = (np.asarray(v, F32) for v in (mean, var, gamma, beta, moving_mean, moving_var))
    eps, mom = F32(eps), F32(momentum)
    rstd = F32(1) / np.sqrt(var + eps)
    a = gamma * rstd
    om = F32(1) - mom
    vu = var * (F32(n) / F32(n - 1)) if unbiased else var
    return dict(rstd=rstd, a=a, b=fma32(-mean, a, beta), moving_mean=fma32(mm, mom, mean * om), moving_var=fma32(mv, mom, vu * om))


def fold_ab_f32(mean, rstd, gamma, beta):
    """a and b from a given rstd (the launch's own, where its 1 / sqrtf is not correctly rounded)"""
    a = np.asarray(gamma, F32) * np.asarray(rstd, F32)
    return a, fma32(-np.asarray(mean, F32), a, beta)


def affine_relu_f32(z, a, b, dt, relu=True):
    t = fma32(z, a, b)
    return h16_round(np.maximum(t, F32(0)) if relu else t, dt)


def mask_f32(z, a, b):
    return fma32(z, a, b) > 0


def bn_bwd(g, z, mask, mean, rstd):
    """g, z (n, C) values, mask (n, C) bool or None, mean / rstd the float32 vectors the launch read -> dict of float64: gy, zh (n, C),
    dbeta, dbeta_abs, dgamma, dgamma_abs (C)"""
    g, z = np.asarray(g, np.float64), np.asarray(z, np.float64)
    gy = g if mask is None else g * mask
    zh = (z - np.asarray(mean, np.float64)) * np.asarray(rstd, np.float64)
    return dict(gy=gy, zh=zh, dbeta=gy.sum(0), dbeta_abs=np.abs(gy).sum(0), dgamma=(gy * zh).sum(0), dgamma_abs=np.abs(gy * zh).sum(0))


def bn_dz(m, gamma, rstd, dgamma, dbeta, n):
    """m = bn_bwd(...) -> (v, the sum |gr| (|gy| + |c1| + |zh c2|) the tolerance scales with)"""
    gr = np.asarray(gamma, np.float64) * np.asarray(rstd, np.float64)
    c1, c2 = np.asarray(dbeta, np.float64) / n, np.asarray(dgamma, np.float64) / n
    return gr * (m["gy"] - c1 - m["zh"] * c2), np.abs(gr) * (np.abs(m["gy"]) + np.abs(c1) + np.abs(m["zh"] * c2))


def layer_backward(x, w, gamma, beta, eps, g):
    """the formulas above on one conv3x3 + batch norm + ReLU layer in float64, for the autograd check: x (B, H, W, cin), w (cout, cin, 3, 3),
    g = dL/dy (B, H, W, cout) -> dict y, dz, dgamma, dbeta, dW, dx"""
    from convbwd_model import flip_weight, weight_grad
    x, w, g = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(g, np.float64)
    B, H, W, cin = x.shape
    cout = w.shape[0]

    def conv(v, k):
        vp = np.zeros((B, H + 2, W + 2, v.shape[3]))
        vp[:, 1:-1, 1:-1] = v
        return sum(vp[:, i:i + H, j:j + W] @ k[:, :, i, j].T for i in range(3) for j in range(3))
    z = conv(x, w).reshape(-1, cout)
    n = z.shape[0]
    mean, var = stats(z)
    rstd = 1.0 / np.sqrt(var + eps)
    y = np.maximum((z - mean) * rstd * gamma + beta, 0.0)
    m = bn_bwd(g.reshape(n, cout), z, y > 0, mean, rstd)
    dz = bn_dz(m, gamma, rstd, m["dgamma"], m["dbeta"], n)[0].reshape(B, H, W, cout)
    return dict(y=y.reshape(B, H, W, cout), dz=dz, dgamma=m["dgamma"], dbeta=m["dbeta"], dW=weight_grad(x, dz, want_abs=False)[0],
                dx=conv(dz, flip_weight(w)))

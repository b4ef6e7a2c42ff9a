"""float64 model of the Meta-Kernel unit in training mode (include/rangedet_hip.h: rd_meta_kernel_stats, rd_meta_kernel_fwd_train,
rd_meta_kernel_bwd_sums, rd_meta_kernel_bwd_params_train, rd_meta_kernel_bwd_data_train; the arithmetic contract is the header comment of
rangedet_amd/csrc/k_metatrain.h).  Plain module, imported by test_meta_train.py.  Nothing here looks at a kernel's output.

  front           the forward up to q = data[n_k] * w_k.  u is formed exactly as the kernels form it (float32 differences, the fmaf chain of
                  mb_hidden), so h = relu(round16(u)) has the kernels' bits; everything behind h is float64
  model           the whole contract with GIVEN tables a1, bb1, mean1, rstd1, c1, c2 (arrays of 576, index c 9 + k), sums exact:
                  z, dA, dbeta1, dgamma1, dW1, db1, dW0, db0, ddata
  exact_case      metabwd_model.exact_case's integers with s1 = 1, t1 = 0 and representable tables (a1, rstd1 powers of two, bb1, mean1
                  small integers, c1, c2 small dyadic values); check_exact asserts the family's two conditions on the model alone
  stats_bound     per-element bounds on mean1 / var1, built as norm_model.stats_bound builds rd_bn_stats's from the launch's own runs and
                  pilots, plus the float32 error q itself carries (one 33-term MFMA accumulation for w, one product)
  stats_f64       the documented statistics scheme restated in float64 (the model margin test)"""
import numpy as np

import metabwd_model as MB
from emu_util import h16_round
from norm_model import U, fma32

F32 = np.float32
WAVES, SPLIT = 4, 64            # k_metabwd.h MB_WAVES, MB_SPLIT


def unit(prm):
    """the parameters with s1 = s2 = 1, t1 = t2 = 0: what the training kernels' packed blocks are made from"""
    return dict(prm, s1=np.ones(576, F32), t1=np.zeros(576, F32), s2=np.ones(64, F32), t2=np.zeros(64, F32))


def taps(a):
    """(B, C, H, W) -> (B, C, 9, H, W): the 3 x 3 neighbourhood with zero padding, tap k = 3 (dh + 1) + (dw + 1)"""
    B, C, H, W = a.shape
    p = np.zeros((B, C, H + 2, W + 2), a.dtype)
    p[:, :, 1:-1, 1:-1] = a
    return np.stack([p[:, :, k // 3:k // 3 + H, k % 3:k % 3 + W] for k in range(9)], 2)


def centre_const(prm):
    """the packer's fold of the centre tap, in double in the host loop's order, rounded to float32"""
    w = prm["b1"].astype(np.float64).copy()
    for j in range(32):
        w = w + prm["w1"][:, j].astype(np.float64) * float(max(prm["b0"][j], 0.0))
    return w.astype(F32).astype(np.float64)


def front(data, coord, prm, dt, hmap=None):
    """hmap: u (float32 values) -> h, in place of the contract's relu(round16(u))"""
    data, coord = np.asarray(data, F32), np.asarray(coord, F32)
    x = taps(data).astype(np.float64)                                     # (B, 64, 9, H, W)
    rel = (taps(coord) - coord[:, :, None]).astype(F32)                   # float32 differences
    w0, b0 = prm["w0"].astype(F32), prm["b0"].astype(F32)
    r0, r1, r2 = (rel[:, None, i] for i in range(3))                      # (B, 1, 9, H, W)
    col = lambda v: v.reshape(1, 32, 1, 1, 1)
    u = fma32(col(w0[:, 0]), r0, fma32(col(w0[:, 1]), r1, fma32(col(w0[:, 2]), r2, col(b0))))
    h = np.maximum(h16_round(u, dt), 0).astype(np.float64) if hmap is None else hmap(u.astype(np.float64))
    W1 = h16_round(prm["w1"], dt).astype(np.float64)
    w = np.einsum("cj,bjkhw->bckhw", W1, h) + prm["b1"].astype(np.float64).reshape(1, 64, 1, 1, 1)
    wabs = np.einsum("cj,bjkhw->bckhw", np.abs(W1), h) + np.abs(prm["b1"]).astype(np.float64).reshape(1, 64, 1, 1, 1)
    cc = centre_const(prm).reshape(1, 64, 1, 1)
    w[:, :, 4], wabs[:, :, 4] = cc, 0.0                                   # the constant carries no float32 accumulation
    hc = h.copy()
    hc[:, :, 4] = np.maximum(b0, 0).astype(np.float64).reshape(1, 32, 1, 1)
    return dict(x=x, rel=rel.astype(np.float64), u=u.astype(np.float64), h=h, hc=hc, w=w, wabs=wabs, q=x * w, W1=W1,
                A=h16_round(prm["agg"], dt).astype(np.float64).reshape(64, 64, 9))


def tab(v):
    return np.asarray(v, np.float64).reshape(1, 64, 9, 1, 1)


def fold_taps(t):
    """(B, 64, 9, H, W) contributions of source pixel p to its neighbour n_k = p + d_k -> (B, H, W, 64) sums at the neighbours"""
    B, C, _, H, W = t.shape
    out = np.zeros((B, C, H + 2, W + 2))
    for k in range(9):
        out[:, :, k // 3:k // 3 + H, k % 3:k % 3 + W] += t[:, :, k]
    return out[:, :, 1:-1, 1:-1].transpose(0, 2, 3, 1).copy()


def model(data, coord, dz, prm, tabs, dt, f=None):
    """tabs: dict a1, bb1, mean1, rstd1, c1, c2 (576 each).  dz (B, 64, H, W) rounded values.  -> dict of float64 arrays; z and ddata are
    (B, H, W, 64) BEFORE their one rounding; 'parts' holds the intermediates check_exact looks at"""
    f = f or front(data, coord, prm, dt)
    dz = np.asarray(dz, np.float64)
    a1, bb1, mu, rs, c1, c2 = (tab(tabs[k]) for k in ("a1", "bb1", "mean1", "rstd1", "c1", "c2"))
    x, q, w, A = f["x"], f["q"], f["w"], f["A"]
    r = q * a1 + bb1
    a = np.maximum(r, 0)
    z = np.einsum("ock,bckhw->bhwo", A, a)
    da = np.einsum("ock,bohw->bckhw", A, dz)
    gy = da * (r > 0)
    xh = (q - mu) * rs
    dq = a1 * (gy - c1 - xh * c2)
    e = dq * x
    nc = np.ones(9)
    nc[4] = 0.0
    du = (f["u"] > 0) * np.einsum("cj,bckhw->bjkhw", f["W1"], e) * nc.reshape(1, 1, 9, 1, 1)
    P4 = e[:, :, 4].sum((0, 2, 3))
    db0 = du.sum((0, 2, 3, 4)) + (prm["b0"] > 0) * (prm["w1"].astype(np.float64) * P4[:, None]).sum(0)
    return dict(z=z, dA=np.einsum("bohw,bckhw->ock", dz, a).reshape(64, 576), dbeta1=gy.sum((0, 3, 4)).reshape(576),
                dgamma1=(gy * xh).sum((0, 3, 4)).reshape(576), dW1=np.einsum("bckhw,bjkhw->cj", e, f["hc"]), db1=e.sum((0, 2, 3, 4)),
                dW0=np.einsum("bjkhw,bikhw->ji", du, f["rel"]), db0=db0, ddata=fold_taps(w * dq),
                parts=dict(r=r, a=a, gy=gy, xh=xh, dq=dq, e=e, da=da, du=du))


GRADS = ("dA", "dbeta1", "dgamma1", "dW1", "db1", "dW0", "db0")


def exact_case(B, H, W, dt, seed=0, centre_only=False):
    prm, data, coord, dz = MB.exact_case(B, H, W, dt, seed=seed, centre_only=centre_only)
    rng = np.random.default_rng(9000 + seed)
    tabs = dict(a1=rng.choice([1.0, 2.0], 576), bb1=rng.integers(-2, 3, 576), mean1=rng.integers(-2, 3, 576), rstd1=rng.choice([1.0, 2.0], 576),
                c1=rng.choice([-0.5, 0.0, 0.5], 576), c2=rng.choice([-0.25, 0.0, 0.25], 576))
    return unit(prm), data, coord, dz, {k: v.astype(F32) for k, v in tabs.items()}


def check_exact(data, coord, dz, prm, tabs, dt):
    """every documented 16-bit value is representable; every float32 value on the way is exact and every float32 sum stays below 2^24"""
    f = front(data, coord, prm, dt)
    m = model(data, coord, dz, prm, tabs, dt, f)
    p = m["parts"]
    for name, v in (("h", f["h"]), ("W1", f["W1"]), ("A", f["A"]), ("a", p["a"]), ("e", p["e"])):
        v32 = v.astype(F32)
        assert (v32 == v).all() and (h16_round(v32, dt) == v32).all(), name
    for name in ("u", "w", "q"):
        assert (f[name].astype(F32) == f[name]).all(), name
    for name in ("r", "xh", "dq", "gy"):
        assert (p[name].astype(F32) == p[name]).all(), name
    # sums of absolute terms: any order of additions stays exact below 2^24 units of the finest term (1 / 4: gy is an integer, c1 a half, xh c2 a quarter, a1 1 or 2)
    dz = np.abs(np.asarray(dz, np.float64))
    abs_sums = dict(z=np.einsum("ock,bckhw->bhwo", np.abs(f["A"]), p["a"]), dA=np.einsum("bohw,bckhw->ock", dz, p["a"]),
                    dbeta1=np.abs(p["gy"]).sum((0, 3, 4)), dgamma1=np.abs(p["gy"] * p["xh"]).sum((0, 3, 4)),
                    dW1=np.einsum("bckhw,bjkhw->cj", np.abs(p["e"]), f["hc"]), db1=np.abs(p["e"]).sum((0, 2, 3, 4)),
                    dW0=np.einsum("bjkhw,bikhw->ji", np.abs(p["du"]), np.abs(f["rel"])), db0=np.abs(p["du"]).sum((0, 2, 3, 4)) +
                    (np.abs(prm["w1"]).astype(np.float64) * np.abs(p["e"][:, :, 4]).sum((0, 2, 3))[:, None]).sum(0),
                    ddata=fold_taps(np.abs(f["w"] * p["dq"])), da=np.einsum("ock,bohw->bckhw", np.abs(f["A"]), dz),
                    du=np.einsum("cj,bckhw->bjkhw", np.abs(f["W1"]), np.abs(p["e"])))
    for name, v in abs_sums.items():
        assert float(v.max()) * 4 < 2.0 ** 24, name
    for name in GRADS + ("z", "ddata"):
        assert (m[name] * 4 == np.round(m[name] * 4)).all(), name
    return m


# ---- statistics -------------------------------------------------------------------------------------------------------------------------
def runs(B, H, W, split):
    """the statistics launch's work split -> [(live pixel indices of the run, the 128 pilot sample indices)], flat index (b H + h) W + w"""
    nfw = (W + 31) // 32
    nfrag = B * H * nfw
    nch = (nfrag + WAVES - 1) // WAVES
    S = min(split if split > 0 else SPLIT, nch)

    def lanes(f):
        row, col = divmod(f, nfw)
        w = col * 32 + np.arange(32)
        return np.where((f < nfrag) & (w < W), row * W + w, -1)
    out = []
    for s in range(S):
        lo, hi = s * nch // S, (s + 1) * nch // S
        px = np.concatenate([lanes(f) for f in range(lo * WAVES, hi * WAVES)])
        first = px[:32 * WAVES].copy()
        first[first < 0] = px[0]
        out.append((px[px >= 0], first))
    return out


def q_matrix(f):
    """(n, 576): q per pixel (flat index) and (c, k)"""
    B, C, K, H, W = f["q"].shape
    perm = lambda t: t.transpose(0, 3, 4, 1, 2).reshape(B * H * W, 576)
    eq = np.abs(f["x"]) * (33 * U * f["wabs"]) + U * np.abs(f["q"])       # float32: the MFMA accumulation of w, then one product
    return perm(f["q"]), perm(eq)


def stats_exact(Q):
    m = Q.mean(0)
    return m, ((Q - m) ** 2).mean(0)


def stats_bound(Q, EQ, rr):
    """norm_model.stats_bound on the launch's own runs and pilots; the merge is a sequential sum of S terms (T = S levels); plus the error of
    q itself: mean |eq| on the mean, 2 mean(|q - mean| eq) on the variance.  -> (bound on mean, bound on var), 576 each"""
    n = Q.shape[0]
    mean, var = stats_exact(Q)
    rows = []
    for idx, pidx in rr:
        r, nk = Q[idx], len(idx)
        p = Q[pidx].mean(0)
        d = r - p
        D1, D2, s = np.abs(d).sum(0), (d * d).sum(0), d.sum(0)
        E1, E2, q = (nk + 1) * U * D1, (nk + 3) * U * D2, s / nk
        mk, M2 = p + q, D2 - s * q
        rows.append(dict(nk=nk, mk=mk, M2=M2, em=E1 / nk + U * np.abs(q) + U * np.abs(mk),
                         eM=E2 + 2 * np.abs(q) * E1 + U * s * s / nk + U * np.abs(M2)))
    T, m0 = len(rr), rows[0]["mk"]
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
    return 2 * emean + EQ.mean(0), 2 * evar + 2 * (np.abs(Q - mean) * EQ).mean(0)


def stats_f64(Q, rr):
    """the documented scheme (pilot, shifted sums per run, the merge formulas) with float32 roundings at every operation but the long sums,
    which are exact: how far the SCHEME sits inside stats_bound"""
    n = F32(Q.shape[0])
    Q32 = Q.astype(F32)
    rows = []
    for idx, pidx in rr:
        p = (Q32[pidx].astype(np.float64).sum(0) / 128).astype(F32)
        d = (Q32[idx] - p).astype(F32).astype(np.float64)
        rows.append((F32(len(idx)), p, d.sum(0).astype(F32), (d * d).sum(0).astype(F32)))
    mk = [p + S1 / nf for nf, p, S1, S2 in rows]
    mean = mk[0] + (sum((nf * (m - mk[0])).astype(np.float64) for (nf, _, _, _), m in zip(rows, mk)).astype(F32)) / n
    acc = 0.0
    for (nf, p, S1, S2), m in zip(rows, mk):
        q, e = S1 / nf, m - mean
        acc = acc + fma32(nf * e, e, fma32(-S1, q, S2)).astype(np.float64)
    return mean, np.maximum(acc.astype(F32) / n, 0)


# ---- the unit against autograd -------------------------------------------------------------------------------------------------------------
def autograd_reference(data, coord, g, prm, gamma1, beta1, gamma2, beta2, dt, eps, round_h=True):
    """float64 torch autograd of the un-fused formulation with F.batch_norm(training=True) on both norms, on the packer's rounded weights and
    with h rounded as the contract rounds it (a constant offset for autograd).  data, coord NCHW, g (B, 64, H, W) -> {name: float64 numpy}"""
    import torch
    import torch.nn.functional as F
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    f = front(data, coord, prm, dt, None if round_h else (lambda u: np.maximum(u, 0)))
    leaves = dict(w0=D(prm["w0"]), b0=D(prm["b0"]), w1=D(prm["w1"]), b1=D(prm["b1"]), A=D(f["A"]), gamma1=D(gamma1), beta1=D(beta1),
                  gamma2=D(gamma2), beta2=D(beta2), data=D(data))
    for v in leaves.values():
        v.requires_grad_(True)
    L = leaves
    B, _, H, W = data.shape
    x = F.unfold(L["data"], 3, padding=1).view(B, 64, 9, H, W)
    rel = D(f["rel"])
    u = torch.einsum("ji,bikhw->bjkhw", L["w0"], rel) + L["b0"].view(1, 32, 1, 1, 1)
    h = F.relu(u + (D(f["h"]) - F.relu(u)).detach() * (u > 0))            # the contract's rounded h, gradient of relu(u)
    W1 = L["w1"] + (D(f["W1"]) - L["w1"].detach())                        # the packer's rounded W1, gradient of W1
    w = torch.einsum("cj,bjkhw->bckhw", W1, h) + L["b1"].view(1, 64, 1, 1, 1)
    wc = L["w1"] @ F.relu(L["b0"]) + L["b1"]
    wc = (wc + (D(centre_const(prm)) - wc).detach()).view(1, 64, 1, 1).expand(B, 64, H, W)      # the packer's float32 constant
    w = torch.cat([w[:, :, :4], wc.unsqueeze(2), w[:, :, 5:]], 2)
    q = (x * w).reshape(B, 576, H, W)
    r = F.batch_norm(q, None, None, L["gamma1"], L["beta1"], training=True, eps=eps)
    z = torch.einsum("oc,bchw->bohw", L["A"].view(64, 576), F.relu(r))
    y = F.relu(F.batch_norm(z, None, None, L["gamma2"], L["beta2"], training=True, eps=eps))
    (y * D(g)).sum().backward()
    out = {k: v.grad.numpy() for k, v in leaves.items()}
    out.update(y=y.detach().numpy(), z=z.detach().numpy(), q=q.detach().numpy())
    return out


def model_with_batch_tables(data, coord, g, prm, gamma1, beta1, gamma2, beta2, dt, eps):
    """the contract's formulas (model) fed with the batch's own tables, all float64: what MetaUnitTrain computes, nothing rounded behind h"""
    f = front(data, coord, prm, dt)
    B, _, K, H, W = f["q"].shape
    n = B * H * W
    q = f["q"]
    mean1 = q.mean((0, 3, 4)).reshape(576)
    var1 = q.var((0, 3, 4)).reshape(576)
    rstd1 = 1.0 / np.sqrt(var1 + eps)
    a1 = np.asarray(gamma1, np.float64) * rstd1
    tabs = dict(a1=a1, bb1=np.asarray(beta1, np.float64) - mean1 * a1, mean1=mean1, rstd1=rstd1, c1=np.zeros(576), c2=np.zeros(576))
    z = model(data, coord, np.zeros((B, 64, H, W)), prm, tabs, dt, f)["z"]            # (B, H, W, 64)
    m2, v2 = z.mean((0, 1, 2)), z.var((0, 1, 2))
    rstd2 = 1.0 / np.sqrt(v2 + eps)
    zh = (z - m2) * rstd2
    yv = zh * gamma2 + beta2
    gy = np.transpose(np.asarray(g, np.float64), (0, 2, 3, 1)) * (yv > 0)
    dbeta2, dgamma2 = gy.sum((0, 1, 2)), (gy * zh).sum((0, 1, 2))
    dz = gamma2 * rstd2 * (gy - dbeta2 / n - zh * dgamma2 / n)
    dzn = np.ascontiguousarray(dz.transpose(0, 3, 1, 2))
    first = model(data, coord, dzn, prm, tabs, dt, f)                                  # pass A: c1 = c2 = 0 does not enter its sums
    tabs.update(c1=first["dbeta1"] / n, c2=first["dgamma1"] / n)
    out = model(data, coord, dzn, prm, tabs, dt, f)
    out.update(y=np.maximum(yv, 0), dgamma2=dgamma2, dbeta2=dbeta2)
    return out


# ---- the whole unit: the contract with a hook at every rounding point, and the tolerance derived from it ---------------------------------------
ROUNDED = ("h", "a", "z", "y", "dz", "e", "ddata")          # k_metatrain.h (1), (4t), (7t), rd_affine_relu, rd_bn_relu_bwd, (5t), (6)
TABLES = ("mean1", "var1", "mean2", "var2")                 # float32 statistics: a few float32 roundings each
UNIT_OUT = ("y", "ddata", "dA", "dW1", "db1", "dW0", "db0", "dgamma1", "dbeta1", "dgamma2", "dbeta2", "mm1", "mv1", "mm2", "mv2")


def hv(x, u):
    """meta_model._hv in numpy: the variance of one round-to-nearest of x to the type, by x's own binade"""
    ax = np.abs(x)
    e = np.floor(np.log2(np.maximum(ax, 1e-300)))
    return np.where(ax == 0, 0.0, (2.0 * u * np.exp2(e)) ** 2 / 3.0)


def contract(data, coord, g, prm, norm, moving, dt, eps, momentum, hook, masks=None, want_abs=False):
    """The unit's forward and backward as k_metatrain.h, k_norm.h and MetaUnitTrain compose them, float64, sums exact, with hook(site, x)
    applied at every point where the device rounds to 16 bits (ROUNDED), at the float32 statistics (TABLES) and at the two ReLU masks
    (mask_r, mask_y).  hook = identity: the reference function itself (equal to autograd).  g (B, H, W, 64).  masks: fixed (mask_r, mask_y,
    u > 0) in place of the ones this run would compute.  -> outputs by UNIT_OUT, plus 'rec' (r, ypre, masks) and, with want_abs, 'abs': the
    sums of absolute terms behind every float32 sum."""
    gamma1, beta1, gamma2, beta2 = (np.asarray(v, np.float64) for v in norm)
    f = front(data, coord, prm, dt, hmap=lambda u: hook("h", np.maximum(u, 0)))
    x, q, w, A, h = f["x"], f["q"], f["w"], f["A"], f["h"]
    B, _, _, H, W = q.shape
    n = B * H * W
    mean1, var1 = hook("mean1", q.mean((0, 3, 4)).reshape(576)), hook("var1", q.var((0, 3, 4)).reshape(576))
    rstd1 = 1.0 / np.sqrt(var1 + eps)
    a1 = gamma1 * rstd1
    bb1 = beta1 - mean1 * a1
    r = q * tab(a1) + tab(bb1)
    m_r = (r > 0).astype(np.float64) if masks is None else masks["mask_r"]
    a = hook("a", hook("gate_a", m_r * r))          # a flipped gate moves the VALUE by up to |r| + its threshold ...
    m_r = hook("mask_r", m_r)                       # ... and the gradient's mask by one
    z = hook("z", np.einsum("ock,bckhw->bhwo", A, a))
    mean2, var2 = hook("mean2", z.mean((0, 1, 2))), hook("var2", z.var((0, 1, 2)))
    rstd2 = 1.0 / np.sqrt(var2 + eps)
    a2 = gamma2 * rstd2
    ypre = z * a2 + (beta2 - mean2 * a2)
    m_y = (ypre > 0).astype(np.float64) if masks is None else masks["mask_y"]
    y = hook("y", hook("gate_y", m_y * ypre))
    m_y = hook("mask_y", m_y)
    gy2 = np.asarray(g, np.float64) * m_y
    zh = (z - mean2) * rstd2
    dbeta2, dgamma2 = gy2.sum((0, 1, 2)), (gy2 * zh).sum((0, 1, 2))
    dz = hook("dz", a2 * (gy2 - dbeta2 / n - zh * dgamma2 / n))
    dzn = dz.transpose(0, 3, 1, 2)
    da = np.einsum("ock,bohw->bckhw", A, dzn)
    gy = da * m_r
    xh = (q - tab(mean1)) * tab(rstd1)
    dbeta1, dgamma1 = gy.sum((0, 3, 4)).reshape(576), (gy * xh).sum((0, 3, 4)).reshape(576)
    dq = tab(a1) * (gy - tab(dbeta1 / n) - xh * tab(dgamma1 / n))
    e = dq * x
    e16 = hook("e", e)
    nc = np.ones(9)
    nc[4] = 0.0
    nck = nc.reshape(1, 1, 9, 1, 1)
    um = (f["u"] > 0) if masks is None else masks["u"]
    b0, w1 = prm["b0"].astype(np.float64), prm["w1"].astype(np.float64)
    du = um * np.einsum("cj,bckhw->bjkhw", f["W1"], e16) * nck
    P4 = e[:, :, 4].sum((0, 2, 3))
    hb = np.maximum(b0, 0)
    unb = n / max(n - 1.0, 1.0)
    mm = [np.asarray(v, np.float64) for v in moving]
    out = dict(y=y, ddata=hook("ddata", fold_taps(w * dq)), dA=np.einsum("bohw,bckhw->ock", dzn, a).reshape(64, 576),
               dW1=np.einsum("bckhw,bjkhw->cj", e16 * nck, h) + P4[:, None] * hb[None], db1=e.sum((0, 2, 3, 4)),
               dW0=np.einsum("bjkhw,bikhw->ji", du, f["rel"]), db0=du.sum((0, 2, 3, 4)) + (b0 > 0) * (w1 * P4[:, None]).sum(0),
               dgamma1=dgamma1, dbeta1=dbeta1, dgamma2=dgamma2, dbeta2=dbeta2,
               mm1=mm[0] * momentum + mean1 * (1 - momentum), mv1=mm[1] * momentum + var1 * unb * (1 - momentum),
               mm2=mm[2] * momentum + mean2 * (1 - momentum), mv2=mm[3] * momentum + var2 * unb * (1 - momentum))
    out["rec"] = dict(r=r, ypre=ypre, mask_r=(r > 0).astype(np.float64), mask_y=(ypre > 0).astype(np.float64), u=f["u"] > 0, da=da, g=np.asarray(g, np.float64),
                      q=q, a1=a1, bb1=bb1)
    if want_abs:
        adz, ae = np.abs(dzn), np.abs(e)
        adu = um * np.einsum("cj,bckhw->bjkhw", np.abs(f["W1"]), ae) * nck
        zabs = np.einsum("ock,bckhw->bhwo", np.abs(A), np.abs(a))
        out["abs"] = dict(y=np.abs(a2) * zabs, ddata=fold_taps(np.abs(w * dq)), dA=np.einsum("bohw,bckhw->ock", adz, np.abs(a)).reshape(64, 576),
                          dW1=np.einsum("bckhw,bjkhw->cj", ae, f["hc"] * 0 + np.where(nck > 0, h, hb.reshape(1, 32, 1, 1, 1))), db1=ae.sum((0, 2, 3, 4)),
                          dW0=np.einsum("bjkhw,bikhw->ji", adu, np.abs(f["rel"])),
                          db0=adu.sum((0, 2, 3, 4)) + (np.abs(w1) * ae[:, :, 4].sum((0, 2, 3))[:, None]).sum(0),
                          dgamma1=np.abs(gy * xh).sum((0, 3, 4)).reshape(576), dbeta1=np.abs(gy).sum((0, 3, 4)).reshape(576),
                          dgamma2=np.abs(gy2 * zh).sum((0, 1, 2)), dbeta2=np.abs(gy2).sum((0, 1, 2)),
                          mm1=np.abs(mean1), mv1=np.abs(var1), mm2=np.abs(mean2), mv2=np.abs(var2))
    return out


def identity_hook(site, x):
    return x


def rounding_hook(dt):
    return lambda site, x: h16_round(np.asarray(x, F32), dt).astype(np.float64) if site in ROUNDED else x


class PerturbHook:
    """x + eps * xi * s at every site, xi independent signs: s = the rounding's standard deviation by binade (ROUNDED), 8 u32 |x| (TABLES:
    a pilot subtraction, a division, a product, an fmaf and the merge's few more, each u32 = 2^-24 relative), or the given gate
    deviations (mask sites; none: 0).  A site asked twice gets the same xi."""

    def __init__(self, uu, eps, rng, gates=None):
        self.uu, self.eps, self.rng, self.gates, self.xi = uu, eps, rng, gates or {}, {}

    def __call__(self, site, x):
        if site in ROUNDED:
            s = np.sqrt(hv(x, self.uu))
        elif site in TABLES:
            s = 8 * U * np.abs(x)
        elif site in self.gates:
            s = self.gates[site]
        else:
            return x
        if site not in self.xi:
            self.xi[site] = self.rng.choice([-1.0, 1.0], np.shape(x))
        return x + self.eps * self.xi[site] * s


def unit_sigma(args, dt, uu, K=32, seed=1):
    """args: contract's (data, coord, g, prm, norm, moving, dt, eps, momentum).  The first-order standard deviation of every output element:
    sigma_i^2 = sum_s (d out_i / d x_s)^2 var_s over all sources s, estimated WITHOUT bias as the mean over K directional derivatives of
    the contract along random sign vectors scaled by the sources' deviations (E (sum_s J_is s_s xi_s)^2 = sum_s J_is^2 s_s^2); the
    relative deviation of such an estimate of sigma is 1 / sqrt(2 K) = 12.5 % at K = 32.  Every propagation path is in it by
    construction, the ones through mean1 / rstd1 / c1 / c2 and the second norm's statistics included.  Two phases: first the roundings
    alone, which gives sigma_r and sigma_ypre and with them the gate triples |r| <= 7 sigma_r + 4 u32 (|q a1| + |bb1|) (and the same for
    the output ReLU); then again with every gate triple as two more sources: a whole flip of the gradient's mask (+- 1), and the value
    behind the gate moving by |r| + its threshold (|ypre| + its threshold), as metabwd_model.bounds prices a flipped gate in dA.
    -> (reference outputs with 'abs', {name: sigma}, (share of r gates, share of y gates))"""
    ref = contract(*args, identity_hook, want_abs=True)
    rec = ref["rec"]
    masks = dict(mask_r=rec["mask_r"], mask_y=rec["mask_y"], u=rec["u"])
    eps = 1e-3

    def sample(gates, keys, rng):
        acc = {}
        for _ in range(K):
            got = contract(*args, PerturbHook(uu, eps, rng, gates), masks=masks)
            for k in keys:
                a, b = (got["rec"][k], rec[k]) if k in ("r", "ypre") else (got[k], ref[k])
                acc[k] = acc.get(k, 0.0) + ((a - b) / eps) ** 2 / K
        return {k: np.sqrt(v) for k, v in acc.items()}
    s1 = sample(None, ("r", "ypre"), np.random.default_rng(seed))
    thr_r = 7 * s1["r"] + 4 * U * (np.abs(rec["q"] * tab(rec["a1"])) + np.abs(tab(rec["bb1"])))
    thr_y = 7 * s1["ypre"] + 4 * U * np.abs(rec["ypre"])
    gr, gy = (np.abs(rec["r"]) <= thr_r).astype(np.float64), (np.abs(rec["ypre"]) <= thr_y).astype(np.float64)
    gates = dict(mask_r=gr, mask_y=gy, gate_a=gr * (np.abs(rec["r"]) + thr_r), gate_y=gy * (np.abs(rec["ypre"]) + thr_y))
    sig = sample(gates, UNIT_OUT, np.random.default_rng(seed + 1))
    return ref, sig, (float(gr.mean()), float(gy.mean()))

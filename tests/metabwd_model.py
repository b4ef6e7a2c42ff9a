"""float64 model of the Meta-Kernel unit's backward (include/rangedet_hip.h: rd_meta_kernel_bwd_data, rd_meta_kernel_bwd_params; the
arithmetic contract is the header comment of rangedet_amd/csrc/k_metabwd.h).  Plain module, imported by test_meta_backward.py.

  folded / packer_weights   the unit's parameters from the reference's dict, BatchNorm folded to s1, t1; the PACKER's rounded s1 W1 and A
  reference                 torch autograd (float64) of oracle/graph_ref.meta_kernel_unit up to z, restated as meta_model.meta_rounded_model
                            restates it, on the packer's weights and the rounded dz: every gradient, nothing rounded on the way
  bounds                    per output element: the standard deviation the contract's roundings imply (each priced by its own binade,
                            meta_model._hv), the bound of the float32 sums (convbwd_model.sum_bound), and the sum of |contribution| over
                            the triples whose gate [r_k > 0] or [u_k > 0] the roundings can flip
  rounded_model             the contract itself in float64 with a round-to-nearest at each documented point: used ONLY to measure how far the
                            contract moves from the reference under `bounds` (never compared with a kernel's output)
  exact_case                the integer family: every documented 16-bit value representable, every float32 sum below 2^24 (both asserted here)

Roundings (k_metabwd.h): (1) h = relu(round(u))  (4) a = relu(round(r)) in dA  (5) e = round(dr x) in dW1 and du  (6) ddata.  (2), (3) are the
packer's s1 W1 and A, which the reference uses as they are.  The centre tap has no rounding at all.
Float32 sums: every product passes through at most n additions -- 64 in each of the two MFMA contractions over channels (da, du), one per
pixel of the lane's run and one per partial (at most 2 B H W together), 128 pixel lanes, 9 taps, 8 for the fused multiply-adds around them:
SUM_N(npix) = 2 npix + 64 + 64 + 128 + 9 + 8.  Nothing here looks at a kernel's output."""
import numpy as np
import torch
import torch.nn.functional as F

import convbwd_model as CB
import meta_model as MM
from emu_util import h16_round
from oracle import graph_ref as G
from rangedet_amd.runtime import bn_affine

NAMES = ("ddata", "dA", "dW1", "db1", "dW0", "db0", "dt1", "dq1")


def SUM_N(npix):
    return 2 * npix + 64 + 64 + 128 + 9 + 8


def folded(P, name, W):
    pre = "%s_%d" % (name, W)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    s1, t1 = bn_affine(P, name + "point_wise_mlp_bn1", G.EPS)
    s2, t2 = bn_affine(P, name + "aggregation_bn1", G.EPS)
    return dict(w0=f(P[pre + "_mlp0_weight"]).reshape(32, 3), b0=f(P[pre + "_mlp0_bias"]), w1=f(P[pre + "_mlp1_weight"]).reshape(64, 32),
                b1=f(P[pre + "_mlp1_bias"]), s1=f(s1), t1=f(t1), agg=f(P[name + "aggregation_conv1_weight"]).reshape(64, 576), s2=f(s2), t2=f(t2))


def pack_args(prm):
    return [prm[k] for k in ("w0", "b0", "w1", "b1", "s1", "t1", "agg", "s2", "t2")]


def packer_weights(prm, dt):
    """(s1 W1)_k as the packers round it, (9, 64, 32): one float32 product, one rounding; A rounded, (64 o, 64 c, 9 k)"""
    s1 = prm["s1"].reshape(64, 9)
    w1s = h16_round((s1.T[:, :, None] * prm["w1"][None]).astype(np.float32), dt)
    return w1s.astype(np.float64), h16_round(prm["agg"], dt).astype(np.float64).reshape(64, 64, 9)


def _D(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _forward(data, coord, prm, dt, leaves=None, rnd=None):
    """the unit up to z, float64.  leaves: tensors that replace the parameters (autograd); rnd(x, point): the contract's roundings"""
    rnd = rnd or (lambda x, p: x)
    L = leaves or {}
    B, C, H, W = data.shape
    w1s16, A16 = (_D(v) for v in packer_weights(prm, dt))
    W0, b0, W1, b1 = (L.get(k, _D(prm[k])) for k in ("w0", "b0", "w1", "b1"))
    s1, t1 = _D(prm["s1"]).view(64, 9), L.get("t1", _D(prm["t1"]).view(64, 9))
    A, q1 = L.get("A", A16), L.get("q1", torch.ones(64, 9, dtype=torch.float64))
    cs = F.unfold(coord, 3, padding=1).view(B, 3, 9, H, W)
    rel = cs - coord.unsqueeze(2)
    u = torch.einsum("ji,bikhw->bjkhw", W0, rel) + b0.view(1, 32, 1, 1, 1)
    h = F.relu(rnd(u, "h"))
    # d(s1 W1 rounded) / dW1 = s1: the rounding offset is a constant
    W1k = s1.t().reshape(9, 64, 1) * W1.view(1, 64, 32) + (w1s16 - s1.t().reshape(9, 64, 1) * W1.detach().view(1, 64, 32))
    w = torch.einsum("kcj,bjkhw->bckhw", W1k, h) + (s1 * b1.view(64, 1)).view(1, 64, 9, 1, 1)
    wc = (s1[:, 4] * (W1 @ F.relu(b0) + b1)).view(1, 64, 1, 1).expand(B, 64, H, W)
    w = torch.cat([w[:, :, :4], wc.unsqueeze(2), w[:, :, 5:]], 2)
    ds = F.unfold(data, 3, padding=1).view(B, C, 9, H, W)
    xw = ds * w
    r = q1.view(1, 64, 9, 1, 1) * xw + t1.view(1, 64, 9, 1, 1)
    a = F.relu(rnd(r, "a"))
    z = torch.einsum("ock,bckhw->bohw", A, a)
    return dict(rel=rel, u=u, h=h, W1k=W1k, w=w, ds=ds, xw=xw, r=r, a=a, z=z, A16=A16, s1=s1)


def reference(data, coord, dz, prm, dt):
    """data (B, 64, H, W), coord (B, 3, H, W), dz (B, 64, H, W): values already rounded -> {name: float64 numpy}, the reference's shapes;
    ddata is (B, H, W, 64)"""
    data, coord, dz = (torch.as_tensor(v, dtype=torch.float64) for v in (data, coord, dz))
    leaves = dict(w0=_D(prm["w0"]), b0=_D(prm["b0"]), w1=_D(prm["w1"]), b1=_D(prm["b1"]), t1=_D(prm["t1"]).view(64, 9),
                  A=_D(packer_weights(prm, dt)[1]), q1=torch.ones(64, 9, dtype=torch.float64))
    for v in leaves.values():
        v.requires_grad_(True)
    data = data.clone().requires_grad_(True)
    f = _forward(data, coord, prm, dt, leaves)
    (f["z"] * dz).sum().backward()
    g = lambda t: (torch.zeros_like(t) if t.grad is None else t.grad).numpy()
    return dict(ddata=g(data).transpose(0, 2, 3, 1).copy(), dA=g(leaves["A"]).reshape(64, 576), dW1=g(leaves["w1"]), db1=g(leaves["b1"]),
                dW0=g(leaves["w0"]), db0=g(leaves["b0"]), dt1=g(leaves["t1"]).reshape(576), dq1=g(leaves["q1"]).reshape(576))


def bounds(data, coord, dz, prm, dt, gates=True):
    """-> {name: (sigma, sum bound, gate term)} float64 numpy in the shapes of reference(), and the shares of gate triples (r, u).
    sigma: the contract's roundings, first order, independent.  gate term: sum of |contribution| of the triples (p, c, k) with
    |r_k| <= 7 sigma_r + float32 slack -- and of the (p, j, k) with |u_k| within the float32 slack of 0 -- to that output."""
    uu = MM.half_ulp(dt)
    data, coord, dz = (torch.as_tensor(v, dtype=torch.float64) for v in (data, coord, dz))
    B, C, H, W = data.shape
    n = SUM_N(B * H * W)
    with torch.no_grad():
        f = _forward(data, coord, prm, dt)
        rel, u, h, W1k, w, x, xw, r, a, A, s1 = (f[k] for k in ("rel", "u", "h", "W1k", "w", "ds", "xw", "r", "a", "A16", "s1"))
        W0, b0, t1 = _D(prm["w0"]), _D(prm["b0"]), _D(prm["t1"]).view(1, 64, 9, 1, 1)
        s1k = s1.view(1, 64, 9, 1, 1)
        hv = MM._hv
        var_w = torch.einsum("kcj,bjkhw->bckhw", W1k ** 2, hv(h, uu))
        var_w[:, :, 4] = 0.0
        mask = (r > 0).to(torch.float64)
        da = torch.einsum("ock,bohw->bckhw", A, dz)
        daabs = torch.einsum("ock,bohw->bckhw", A.abs(), dz.abs())
        dr, e = da * mask, da * mask * x
        eabs = daabs * mask * x.abs()
        nc = torch.ones(9, dtype=torch.float64)
        nc[4] = 0.0                                               # the centre tap's MLP terms are float32 only
        nck, ncj = nc.view(1, 1, 9, 1, 1), nc.view(1, 1, 9, 1, 1)
        umask = (u > 0).to(torch.float64)
        var_e = hv(e, uu) * nck
        var_du = umask * torch.einsum("kcj,bckhw->bjkhw", W1k ** 2, var_e)
        du_abs = umask * torch.einsum("kcj,bckhw->bjkhw", W1k.abs(), eabs) * ncj
        fold = lambda t: F.fold(t.reshape(B, 64 * 9, H * W), (H, W), 3, padding=1).permute(0, 2, 3, 1)
        # gate triples
        sig_r = (x * x * var_w).sqrt()
        thr_r = 7.0 * sig_r + 4.0 * CB.U * (xw.abs() + t1.abs())
        gr = (r.abs() <= thr_r).to(torch.float64) if gates else torch.zeros_like(r)
        thr_u = 4.0 * CB.U * (torch.einsum("ji,bikhw->bjkhw", W0.abs(), rel.abs()) + b0.abs().view(1, 32, 1, 1, 1))
        gu = (u.abs() <= thr_u).to(torch.float64) * ncj if gates else torch.zeros_like(u)
        g_da, g_ex = gr * da.abs(), gr * (da * x).abs()           # |dr| and |e| of a triple whose mask may flip
        g_du = umask * torch.einsum("kcj,bckhw->bjkhw", W1k.abs(), g_ex) + gu * torch.einsum("kcj,bckhw->bjkhw", W1k, e).abs()
        hc = h.clone()
        hc[:, :, 4] = F.relu(b0).view(1, 32, 1, 1)
        c_db0 = (b0 > 0).to(torch.float64)                        # the centre tap's db0 term, [b0 > 0] sum_c |s1 W1| |.|
        cen = lambda t: c_db0 * torch.einsum("cj,bchw->j", W1k[4].abs(), t[:, :, 4])
        sm = lambda t, dims: t.sum(dims)
        out = {}
        out["ddata"] = (fold(mask * da * da * var_w).sqrt(), CB.sum_bound(9 * 65 + 8, fold(w.abs() * mask * daabs)), fold(gr * (w * da).abs()))
        out["dA"] = (torch.einsum("bohw,bckhw->ock", dz * dz, x * x * var_w * mask + hv(a, uu)).sqrt().reshape(64, 576),
                     CB.sum_bound(n, torch.einsum("bohw,bckhw->ock", dz.abs(), a).reshape(64, 576)),
                     torch.einsum("bohw,bckhw->ock", dz.abs(), gr * (r.abs() + thr_r)).reshape(64, 576))
        out["dt1"] = (torch.zeros(576, dtype=torch.float64), CB.sum_bound(n, sm(daabs * mask, (0, 3, 4)).reshape(576)), sm(g_da, (0, 3, 4)).reshape(576))
        out["dq1"] = (sm(e * e * var_w, (0, 3, 4)).sqrt().reshape(576), CB.sum_bound(n, sm(eabs * w.abs(), (0, 3, 4)).reshape(576)),
                      sm(g_ex * w.abs(), (0, 3, 4)).reshape(576))
        out["db1"] = (torch.zeros(64, dtype=torch.float64), CB.sum_bound(n, sm(s1k.abs() * eabs, (0, 2, 3, 4))), sm(s1k.abs() * g_ex, (0, 2, 3, 4)))
        out["dW1"] = (torch.einsum("bckhw,bjkhw->cj", s1k ** 2 * var_e, h * h) .add(torch.einsum("bckhw,bjkhw->cj", s1k ** 2 * e * e * nck, hv(h, uu))).sqrt(),
                      CB.sum_bound(n, torch.einsum("bckhw,bjkhw->cj", s1k.abs() * eabs, hc)), torch.einsum("bckhw,bjkhw->cj", s1k.abs() * g_ex, hc))
        out["db0"] = (sm(var_du, (0, 2, 3, 4)).sqrt(), CB.sum_bound(n, sm(du_abs, (0, 2, 3, 4)) + cen(eabs)), sm(g_du * ncj, (0, 2, 3, 4)) + cen(g_ex))
        relT = rel.abs().permute(0, 2, 3, 4, 1)                   # (B, 9, H, W, 3)
        out["dW0"] = (torch.einsum("bjkhw,bkhwi->ji", var_du, relT ** 2).sqrt(), CB.sum_bound(n, torch.einsum("bjkhw,bkhwi->ji", du_abs, relT)),
                      torch.einsum("bjkhw,bkhwi->ji", g_du * ncj, relT))
        shares = (float(gr.mean()), float(gu.sum() / (8.0 * gu[:, :, 0].numel())))   # (the centre tap has no u gate)
    return {k: tuple(np.asarray(t, dtype=np.float64) for t in v) for k, v in out.items()}, shares


def rounded_model(data, coord, dz, prm, dt):
    """The contract in float64: every documented rounding applied, sums exact.  Measures the bounds' margin; never meets a kernel."""
    data, coord, dz = (torch.as_tensor(v, dtype=torch.float64) for v in (data, coord, dz))
    B, C, H, W = data.shape
    rn = lambda t: MM._rne(t, dt)
    with torch.no_grad():
        f = _forward(data, coord, prm, dt, rnd=lambda t, p: rn(t) if p == "h" else t)     # r in float32: only h is rounded on the way
        rel, u, h, W1k, w, x, xw, r, A, s1 = (f[k] for k in ("rel", "u", "h", "W1k", "w", "ds", "xw", "r", "A16", "s1"))
        W1, b0 = _D(prm["w1"]), _D(prm["b0"])
        s1k = s1.view(1, 64, 9, 1, 1)
        mask = (r > 0).to(torch.float64)
        a16 = F.relu(rn(r))
        da = torch.einsum("ock,bohw->bckhw", A, dz)
        dr = da * mask
        e = dr * x
        e16 = rn(e)
        du = (u > 0) * torch.einsum("kcj,bckhw->bjkhw", W1k, e16)
        du[:, :, 4] = 0.0
        P4 = e[:, :, 4].sum((0, 2, 3))
        E = torch.einsum("bckhw,bjkhw->kcj", e16, h)
        E[4] = P4.view(64, 1) * F.relu(b0).view(1, 32)
        out = dict(ddata=F.fold((w * dr).reshape(B, 576, H * W), (H, W), 3, padding=1).permute(0, 2, 3, 1),
                   dA=torch.einsum("bohw,bckhw->ock", dz, a16).reshape(64, 576), dt1=dr.sum((0, 3, 4)).reshape(576),
                   dq1=(dr * xw).sum((0, 3, 4)).reshape(576), db1=(s1k * e).sum((0, 2, 3, 4)), dW1=(s1.t().reshape(9, 64, 1) * E).sum(0),
                   db0=du.sum((0, 2, 3, 4)) + (b0 > 0) * ((s1[:, 4].view(64, 1) * W1) * P4.view(64, 1)).sum(0),
                   dW0=torch.einsum("bjkhw,bikhw->ji", du, rel))
    return {k: v.numpy() for k, v in out.items()}


def open_gate(prm, data, coord, dt):
    """t1 raised to the smallest power of two for which every r_k of the float64 reference exceeds 7 sigma_r (+ the float32 slack)"""
    uu = MM.half_ulp(dt)
    data, coord = (torch.as_tensor(v, dtype=torch.float64) for v in (data, coord))
    with torch.no_grad():
        f = _forward(data, coord, dict(prm, t1=np.zeros(576, np.float32)), dt)
        var_w = torch.einsum("kcj,bjkhw->bckhw", f["W1k"] ** 2, MM._hv(f["h"], uu))
        var_w[:, :, 4] = 0.0
        sig = (f["ds"] ** 2 * var_w).sqrt()
        for m in range(-4, 40):
            T = 2.0 ** m
            if bool((f["xw"] + T > 7.0 * sig + 4.0 * CB.U * (f["xw"].abs() + T)).all()):
                return dict(prm, t1=np.full(576, T, np.float32))
    raise AssertionError("no power of two opens every gate")


def exact_case(B, H, W, dt, seed=0, centre_only=False):
    """Integers: coordinates -2 .. 2, W0 in {-1, 0, 1}, b0 -1 .. 2, two +-1 entries per row of W1, b1 -1 .. 1, data 0 .. 2, s1 = 1, t1 -2 .. 2,
    A in {-1, 0, 1} with one entry in eight set, dz in {-1, 0, 1}.  -> prm, data, coord, dz (NCHW float32).  The two conditions of the
    exact family are asserted in check_exact."""
    rng = np.random.default_rng(4000 + seed)
    w1 = np.zeros((64, 32), np.float32)
    for c in range(64):
        w1[c, rng.choice(32, 2, replace=False)] = rng.choice([-1.0, 1.0], 2)
    agg = (rng.integers(-1, 2, (64, 64, 9)) * (rng.random((64, 64, 9)) < 0.25)).astype(np.float32)
    if centre_only:
        agg[:, :, [0, 1, 2, 3, 5, 6, 7, 8]] = 0.0
    prm = dict(w0=rng.integers(-1, 2, (32, 3)).astype(np.float32), b0=rng.integers(-1, 3, 32).astype(np.float32), w1=w1,
               b1=rng.integers(-1, 2, 64).astype(np.float32), s1=np.ones(576, np.float32), t1=rng.integers(-2, 3, 576).astype(np.float32),
               agg=agg.reshape(64, 576), s2=np.ones(64, np.float32), t2=np.zeros(64, np.float32))
    data = rng.integers(0, 3, (B, 64, H, W)).astype(np.float32)
    coord = rng.integers(-2, 3, (B, 3, H, W)).astype(np.float32)
    dz = rng.integers(-1, 2, (B, 64, H, W)).astype(np.float32)
    return prm, data, coord, dz


def check_exact(data, coord, dz, prm, dt):
    """the exact family's two conditions: every documented 16-bit value is representable, every float32 sum stays below 2^24"""
    with torch.no_grad():
        f = _forward(*(torch.as_tensor(v, dtype=torch.float64) for v in (data, coord)), prm, dt)
        da = torch.einsum("ock,bohw->bckhw", f["A16"], torch.as_tensor(dz, dtype=torch.float64))
        e = da * (f["r"] > 0) * f["ds"]
    for name, t in (("h", f["h"]), ("s1 W1", f["W1k"]), ("A", f["A16"]), ("a", f["a"]), ("e", e), ("w", f["w"]), ("u", f["u"])):
        v = t.numpy().astype(np.float32)
        assert (h16_round(v, dt) == v).all() and (v == np.round(v)).all(), name
    bnd, _ = bounds(data, coord, dz, prm, dt, gates=False)
    for name, (sig, sb, _) in bnd.items():
        n = 9 * 65 + 8 if name == "ddata" else SUM_N(data.shape[0] * data.shape[2] * data.shape[3])
        assert float((sb / (2.0 * n * CB.U)).max()) < 2.0 ** 24, name        # sum_bound = 2 n U sum |terms|

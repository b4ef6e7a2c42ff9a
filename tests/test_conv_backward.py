"""The head-tower backward primitives (csrc/k_convbwd.h: rd_relu_affine_bwd, rd_conv3x3_bwd_weight, rd_head_out_bwd; the data gradient as
the forward launch on the flipped weight; rangedet_amd.backward.HeadTowerBackward) against tests/convbwd_model.py, the float64 restatement
of the formulas in include/rangedet_hip.h.  Through the C ABI: every output buffer and the workspace are pre-filled with 0xFF bytes and
carry a guard tail; the tail and the channels outside [coff, coff + C) must be unchanged afterwards.

Each step is compared with the model fed THE KERNEL'S OWN inputs to that step (its saved activations, its own dz), so that no ReLU mask
can disagree and no error compounds (the pattern of test_loss.py).  Tolerances, u = 2^-24, n = the terms of a sum:
  rd_relu_affine_bwd        bit-equal to h16_round(float32(g) * float32(s)) where y > 0, +0 elsewhere (y == 0 and -0 included)
  dW, dw, dbias, random     |got - want| <= 2 n u sum |terms| per element (convbwd_model.sum_bound: any summation order; the factor 2 for
                            the MFMA's internal adder); inputs normal, and ReLU-sparse x with half zeros
  the same, exact inputs    x, dz, d_out integers in -3 .. 3: every partial sum in any order is an integer below 2^24 -> equal to the model
                            in every bit (-0 and +0 taken as equal).  This catches one dropped or doubled pixel at any reduction length.
  data gradient             conv_model.conv_tol on the float64 conv of the kernel's own dz with the rounded, flipped weight
  output-conv dx            v = (sum_o d_o w_oc) [x > 0] s_c:  half an ulp of the type at v + 2 nout u |s_c| sum_o |d_o w_oc| + u |v| with a scale
                            (the sum's error passes through the multiplication by s_c, which adds one float32 rounding)
  determinism               two calls of each reducing launch on 0xFF-filled outputs and workspace give identical bytes
"""
import numpy as np
import pytest

import conv_model as CM
import convbwd_model as M
from conftest import BOTH, HIP_ONLY
from rangedet_amd import lib as R
from train_util import DTS, back, back_image, check_hob, check_wgrad, dev16, ff, from_bits, image, rnd, same_bits, to_bits, train_inputs, vals16

PT, RH = 64, 16        # the weight-gradient kernel's pixel tile and row strip (k_convbwd.h BW_PT, BW_RH)


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------------
def run_wgrad(be, dt, x, dz, xcs=None, xco=0, zcs=None, zco=0, split=0, twice=False):
    L = be.lib
    B, H, W, cin = x.shape
    cout = dz.shape[3]
    nws = L.raw("rd_conv3x3_bwd_weight_workspace_bytes")(B, H, W, cin, cout, split)
    assert nws > 0 and nws % (36 * cin * cout) == 0
    xd, zd = be.up(image(x, dt, xcs, xco)), be.up(image(dz, dt, zcs, zco))
    outs = []
    for _ in range(2 if twice else 1):
        dW, ws = ff(be, cout * cin * 36), ff(be, nws)
        L.call("rd_conv3x3_bwd_weight", be.ptr(xd), xcs or cin, xco, be.ptr(zd), zcs or cout, zco, be.ptr(dW), B, H, W, cin, cout, split, dt,
               be.ptr(ws), nws, be.stream)
        back(be, ws, nws, "workspace")
        outs.append(back(be, dW, cout * cin * 36, "dW"))
    if twice:
        assert outs[0].tobytes() == outs[1].tobytes(), "two calls differ"
    return outs[0].view(np.float32).reshape(cout, cin, 3, 3).copy(), nws // (36 * cin * cout)


def wgrad_case(be, dt, shape, cin, cout, what, split=0, **lay):
    """one shape: normal inputs, ReLU-sparse x, exact inputs"""
    B, H, W = shape
    for kind, zkind, exact in (("normal", "normal", False), ("relu", "normal", False), ("ints", "ints", True)):
        x, dz = rnd(kind, (B, H, W, cin), dt, 11), rnd(zkind, (B, H, W, cout), dt, 12)
        if kind == "relu":
            assert 0.4 < (x == 0).mean() < 0.6
        got, _ = run_wgrad(be, dt, x, dz, split=split, **lay)
        check_wgrad(got, x, dz, exact, "%s %s %s" % (what, kind, be.name))


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (128, 64), (128, 128)])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_weight_grad_channel_pairs(be, dt, cin, cout):
    """B 2, 3 x 37: the top and the bottom row, an interior row, a width that fills no pixel tile; two partial sums"""
    wgrad_case(be, dt, (2, 3, 37), cin, cout, "2x3x37 %d->%d" % (cin, cout))


@pytest.mark.parametrize("shape", [(2, 1, 37), (2, 3, 1), (1, 2, PT - 1), (1, 2, PT), (1, 2, PT + 1)], ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_weight_grad_edge_shapes(be, dt, shape):
    """one row, one column, and a width one below, at and one above the 64-pixel tile"""
    wgrad_case(be, dt, shape, 64, 64, "%dx%dx%d" % shape)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_weight_grad_channel_stride_and_offset(be, dt):
    """x: 128 channels at offset 8 of 136; dz: 64 channels at offset 16 of 88"""
    wgrad_case(be, dt, (1, 3, 37), 128, 64, "1x3x37 strided", xcs=136, xco=8, zcs=88, zco=16)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_weight_grad_reduction_split(be, dt):
    """B 2, 17 x 70: two row strips (the second starts on real data above it) times two pixel tiles = 8 chunks.  split 3: runs of 2, 3 and 3
    chunks per workgroup (8 does not divide by 3); the library's own split: one chunk each; split 1: one sum.  Exact inputs: all three equal
    the model in every bit; random inputs within the bound."""
    shape, cin, cout = (2, 17, 70), 64, 64
    x, dz = rnd("ints", shape + (cin,), dt, 21), rnd("ints", shape + (cout,), dt, 22)
    for split, parts in ((3, 3), (0, 8), (1, 1)):
        got, S = run_wgrad(be, dt, x, dz, split=split)
        assert S == parts
        check_wgrad(got, x, dz, True, "2x17x70 split %d %s" % (split, be.name))
    x, dz = rnd("relu", shape + (cin,), dt, 23), rnd("normal", shape + (cout,), dt, 24)
    check_wgrad(run_wgrad(be, dt, x, dz, split=3)[0], x, dz, False, "2x17x70 split 3 random %s" % be.name)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_weight_grad_every_tap_has_its_edge_terms(be, dt):
    """x = dz = 1: the dW of tap (dh, dw) is the number of its terms, B (H - |dh|) (W - |dw|) -- fewer than B H W off the centre, asserted
    per tap; and two calls give the same bytes"""
    B, H, W = 2, 3, 37
    x, dz = np.ones((B, H, W, 64), np.float32), np.ones((B, H, W, 64), np.float32)
    got, _ = run_wgrad(be, dt, x, dz, twice=True)
    n = M.tap_terms(B, H, W)
    for i in range(3):
        for j in range(3):
            assert (i, j) == (1, 1) or n[i, j] < B * H * W
            assert (got[:, :, i, j] == n[i, j]).all(), ("tap", i - 1, j - 1, np.unique(got[:, :, i, j]), n[i, j])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_weight_grad_determinism(be, dt):
    x, dz = rnd("relu", (2, 3, 37, 128), dt, 31), rnd("normal", (2, 3, 37, 128), dt, 32)
    run_wgrad(be, dt, x, dz, twice=True)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
def test_weight_grad_many_splits_exact(be, dt):
    """B 2, 64 x 332, 128 -> 128, exact inputs: 48 chunks, 48 partial sums per element"""
    x, dz = rnd("ints", (2, 64, 332, 128), dt, 41), rnd("ints", (2, 64, 332, 128), dt, 42)
    got, S = run_wgrad(be, dt, x, dz, twice=True)
    assert S == 2 * 4 * 6
    check_wgrad(got, x, dz, True, "2x64x332 128->128")


# ---- rd_relu_affine_bwd ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_relu_affine_bwd_bits(be, dt):
    """B 2, 3 x 37, 64 channels at offset 8 of 80 (g), 16 of 96 (y), 24 of 88 (dz): with mask and scale, without the mask, without the
    scale, with neither.  y holds +0, -0 and negative values."""
    L = be.lib
    B, H, W, C = 2, 3, 37, 64
    g = rnd("normal", (B, H, W, C), dt, 51)
    y = rnd("normal", (B, H, W, C), dt, 52).copy()
    y[..., ::3] = 0.0
    ybits = image(y, dt, 96, 16)
    ybits[..., 16:16 + C:6] = 0x8000                                              # -0
    yv = from_bits(ybits[..., 16:16 + C], dt)
    assert (yv == 0).mean() > 0.3 and (yv < 0).mean() > 0.2 and (yv > 0).mean() > 0.2 and (ybits[..., 16:16 + C] == 0x8000).any()
    s = np.random.default_rng(53).uniform(0.5, 1.5, C).astype(np.float32)
    gd, yd, sd = be.up(image(g, dt, 80, 8)), be.up(ybits), be.up(s)
    for use_y, use_s in ((True, True), (False, True), (True, False), (False, False)):
        out = ff(be, B * H * W * 88 * 2)
        L.call("rd_relu_affine_bwd", be.ptr(gd), 80, 8, be.ptr(yd) if use_y else None, 96, 16, be.ptr(sd) if use_s else None, be.ptr(out), 88, 24,
               B, H, W, C, dt, be.stream)
        got = back_image(be, out, (B, H, W, C), 88, 24, dt, "dz")
        want = to_bits(M.relu_affine_bwd(g, yv if use_y else None, s if use_s else None, dt), dt)
        assert (got == want).all(), (use_y, use_s, int((got != want).sum()))
        if use_y:
            assert (got[yv <= 0] == 0).all()


# ---- output-conv backward ----------------------------------------------------------------------------------------------------------------
def run_hob(be, dt, d, x, w, n_off=0, tail=0, scale=None, mask=False, xcs=None, xco=0, dcs=None, dco=0, twice=False):
    """d (B, P, nout) sits at pixel offset n_off of flat (B, (n_off + P + tail) * nout) buffers filled with 7 elsewhere"""
    L = be.lib
    B, H, W, cin = x.shape
    nout, P = d.shape[2], H * W
    obs = (n_off + P + tail) * nout
    flat = np.full((B, obs), 7.0, np.float32)
    flat[:, n_off * nout:(n_off + P) * nout] = d.reshape(B, -1)
    nws = L.raw("rd_head_out_bwd_workspace_bytes")(B, H, W, cin, nout)
    assert nws > 0 and nws % 4 == 0
    dcs = dcs or cin
    dd, xd, wd = be.up(flat), be.up(image(x, dt, xcs, xco)), be.up(np.ascontiguousarray(w, dtype=np.float32))
    sd = None if scale is None else be.up(np.ascontiguousarray(scale, dtype=np.float32))
    outs = []
    for _ in range(2 if twice else 1):
        dx, dw, db, ws = ff(be, B * P * dcs * 2), ff(be, nout * cin * 4), ff(be, nout * 4), ff(be, nws)
        L.call("rd_head_out_bwd", be.ptr(dd), obs, n_off, be.ptr(xd), xcs or cin, xco, be.ptr(wd), 1 if mask else 0, be.ptr(sd), be.ptr(dx), dcs, dco,
               be.ptr(dw), be.ptr(db), B, H, W, cin, nout, dt, be.ptr(ws), nws, be.stream)
        back(be, ws, nws, "workspace")
        outs.append((from_bits(back_image(be, dx, (B, H, W, cin), dcs, dco, dt, "dx"), dt),
                     back(be, dw, nout * cin * 4, "dw").view(np.float32).reshape(nout, cin).copy(),
                     back(be, db, nout * 4, "dbias").view(np.float32).copy()))
    if twice:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs)), "two calls differ"
    assert (be.down(dd, np.float32, (B, obs)) == flat).all()
    return outs[0]


def hob_inputs(dt, B, H, W, cin, nout, exact, seed):
    rng = np.random.default_rng(seed)
    if exact:
        return (rng.integers(-3, 4, (B, H * W, nout)).astype(np.float32), rnd("ints", (B, H, W, cin), dt, seed + 1),
                rng.integers(-3, 4, (nout, cin)).astype(np.float32))
    return (rng.standard_normal((B, H * W, nout)).astype(np.float32), rnd("relu", (B, H, W, cin), dt, seed + 1),
            (rng.standard_normal((nout, cin)) / np.sqrt(cin)).astype(np.float32))


@pytest.mark.parametrize("nout", [1, 8])
@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_head_out_bwd(be, dt, cin, nout):
    """B 2, 3 x 37 = 222 pixels in four blocks: the level at pixel 50 of a wider flat buffer (batch stride beyond the level) with the fused
    mask and scale, twice; dense without them; exact inputs; x at a channel offset and dx at another"""
    B, H, W = 2, 3, 37
    s = np.random.default_rng(61).uniform(0.5, 1.5, cin).astype(np.float32)
    d, x, w = hob_inputs(dt, B, H, W, cin, nout, False, 62)
    what = "hob %d->%d %s" % (cin, nout, be.name)
    check_hob(run_hob(be, dt, d, x, w, n_off=50, tail=20, scale=s, mask=True, twice=True), d, x, w, dt, s, True, False, what + " mask+scale")
    check_hob(run_hob(be, dt, d, x, w), d, x, w, dt, None, False, False, what + " plain")
    check_hob(run_hob(be, dt, d, x, w, n_off=3, mask=True, xcs=cin + 8, xco=8, dcs=cin + 24, dco=16), d, x, w, dt, None, True, False, what + " strided")
    d, x, w = hob_inputs(dt, B, H, W, cin, nout, True, 63)
    check_hob(run_hob(be, dt, d, x, w, n_off=50, tail=20), d, x, w, dt, None, False, True, what + " exact")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
def test_head_out_bwd_many_blocks_exact(be, dt):
    """B 2, 64 x 664, nout 8, exact inputs: 1024 workspace slots"""
    d, x, w = hob_inputs(dt, 2, 64, 664, 128, 8, True, 71)
    check_hob(run_hob(be, dt, d, x, w, twice=True), d, x, w, dt, None, False, True, "hob 2x64x664")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_status_codes(be):
    """cin 96, nout 9, a workspace one byte short, null pointers, misaligned channel offsets: each its code, the message set, nothing
    launched (one zeroed buffer stands for every device pointer and stays zero)."""
    L = be.lib
    buf = be.empty(1 << 20)
    p = be.ptr(buf)
    assert p % 16 == 0
    BF = R.RD_BF16
    ww, wh = L.raw("rd_conv3x3_bwd_weight_workspace_bytes"), L.raw("rd_head_out_bwd_workspace_bytes")

    def wgrad(x=p, dz=p, dW=p, ws=p, cin=64, cout=64, B=1, H=2, W=8, xcs=None, xco=0, split=0, dt=BF, nws=None):
        need = ww(1, 2, 8, 64, 64, split) if nws is None else nws
        return L.raw("rd_conv3x3_bwd_weight")(x, xcs or cin, xco, dz, cout, 0, dW, B, H, W, cin, cout, split, dt, ws, need, be.stream)

    def hob(d=p, x=p, w=p, dx=p, dw=p, db=p, ws=p, cin=64, nout=8, B=1, H=2, W=8, obs=128, n_off=0, dco=0, dt=BF, nws=None):
        need = wh(1, 2, 8, 64, 8) if nws is None else nws
        return L.raw("rd_head_out_bwd")(d, obs, n_off, x, cin, 0, w, 1, p, dx, cin, dco, dw, db, B, H, W, cin, nout, dt, ws, need, be.stream)

    def rab(g=p, y=p, dz=p, C=64, B=1, H=2, W=8, co=0, dt=BF):
        return L.raw("rd_relu_affine_bwd")(g, C, co, y, C, 0, p, dz, C, 0, B, H, W, C, dt, be.stream)
    assert ww(1, 2, 8, 64, 64, 0) == 36 * 64 * 64 and ww(1, 2, 8, 96, 64, 0) == 0 and ww(0, 2, 8, 64, 64, 0) == 0
    assert ww(4, 64, 128, 128, 128, 0) == 32 * 36 * 128 * 128 and ww(4, 64, 128, 128, 128, 5) == 5 * 36 * 128 * 128
    assert wh(1, 2, 8, 64, 8) == (8 * 64 + 8) * 4 and wh(1, 2, 8, 96, 8) == 0 and wh(1, 2, 8, 64, 9) == 0
    for kw in (dict(cin=96), dict(cout=32), dict(cin=256), dict(B=0), dict(H=0), dict(W=0), dict(xco=4, xcs=72), dict(xcs=60)):
        assert wgrad(**kw) == R.RD_ESHAPE, kw
        assert L.rd_last_error_string().decode().startswith("conv3x3_bwd_weight")
    for kw in (dict(nout=9), dict(nout=0), dict(cin=96), dict(B=0), dict(obs=127), dict(n_off=1), dict(dco=4)):
        assert hob(**kw) == R.RD_ESHAPE, kw
        assert L.rd_last_error_string().decode().startswith("head_out_bwd")
    for kw in (dict(C=12), dict(B=0), dict(co=8)):
        assert rab(**kw) == R.RD_ESHAPE, kw
    for name in ("x", "dz", "dW", "ws"):
        assert wgrad(**{name: None}) == R.RD_EINVAL and "null" in L.rd_last_error_string().decode(), name
    for name in ("d", "x", "w", "dw", "db", "ws"):
        assert hob(**{name: None}) == R.RD_EINVAL and "null" in L.rd_last_error_string().decode(), name
    for name in ("g", "dz"):
        assert rab(**{name: None}) == R.RD_EINVAL, name
    assert wgrad(dt=R.RD_F32) == R.RD_EINVAL and hob(dt=R.RD_F32) == R.RD_EINVAL and rab(dt=R.RD_F32) == R.RD_EINVAL
    assert wgrad(split=-1, nws=1 << 20) == R.RD_EINVAL
    assert wgrad(nws=ww(1, 2, 8, 64, 64, 0) - 1) == R.RD_EWORKSPACE and "workspace" in L.rd_last_error_string().decode()
    assert hob(nws=wh(1, 2, 8, 64, 8) - 1) == R.RD_EWORKSPACE and "workspace" in L.rd_last_error_string().decode()
    for rc in (wgrad(x=p + 8), hob(x=p + 8), rab(g=p + 8)):
        assert rc == R.RD_EINVAL and "aligned" in L.rd_last_error_string().decode()
    assert not be.down(buf, np.uint8, (1 << 20,)).any()           # nothing ran


# ---- HeadTowerBackward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_head_tower_backward(be, dt):
    """B 1, 4 x 37: a cls tower (nout 1) and a reg tower (nout 8) of two 128 -> 128 layers; d_logit / d_delta from a real RpnLoss call on
    the towers' own outputs; every returned gradient and every intermediate checked step by step on the kernels' own inputs."""
    from rangedet_amd.backward import HeadTowerBackward
    from rangedet_amd.loss import RpnLoss
    A, L = be.alloc, be.lib
    B, H, W, C = 1, 4, 37, 128
    rng = np.random.default_rng(81)
    x = dev16(be, to_bits(rnd("relu", (B, H, W, C), dt, 82), dt), dt)
    towers, outs = {}, {}
    for kind, nout in (("cls", 1), ("reg", 8)):
        ws = [(rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C / 2)).astype(np.float32) for _ in range(2)]
        ss = [rng.uniform(0.5, 1.5, C).astype(np.float32) for _ in range(2)]
        ts = [(0.1 * rng.standard_normal(C)).astype(np.float32) for _ in range(2)]
        ow, ob = (rng.standard_normal((nout, C, 1, 1)) / np.sqrt(C)).astype(np.float32), (0.1 * rng.standard_normal(nout)).astype(np.float32)
        t = HeadTowerBackward(ws, ss, ts, ow, ob, kind=kind, level=1, first_conv=2, dtype=dt, lib=L, alloc=A)
        outs[kind] = t.forward(x)
        towers[kind] = (t, ws, ss, ow)
    assert tuple(outs["cls"].shape) == (B, H * W, 1) and tuple(outs["reg"].shape) == (B, H * W, 8)
    loss = RpnLoss(strides=(1,), lib=L, alloc=A)(outs["cls"].reshape(B, H * W), outs["reg"], train_inputs(B, H, W))
    A.sync()
    for kind, dname in (("cls", "d_logit"), ("reg", "d_delta")):
        t, ws, ss, ow = towers[kind]
        nout = ow.shape[0]
        dx, grads = t.backward(loss[dname], n_off=0)
        A.sync()
        d = np.array(A.to_numpy(loss[dname])).reshape(B, H * W, nout)
        assert np.isfinite(d).all() and (d != 0).mean() > 0.2, kind
        stem, oname = "rpn_%s_conv_%%d_lvl_1_weight" % kind, "rpn_cls_logit_lvl_1" if kind == "cls" else "rpn_reg_delta_lvl_1"
        assert sorted(grads) == sorted([stem % 2, stem % 3, oname + "_weight", oname + "_bias"])
        g = {k: np.array(A.to_numpy(v)) for k, v in grads.items()}
        assert g[oname + "_weight"].shape == (nout, C, 1, 1) and g[oname + "_bias"].shape == (nout,) and g[stem % 2].shape == (C, C, 3, 3)
        acts = [vals16(be, a, dt) for a in t.acts]
        dzs, dxs = [vals16(be, a, dt) for a in t.dzs], [vals16(be, a, dt) for a in t.dxs]
        assert (acts[2] > 0).mean() > 0.2 and (acts[2] == 0).mean() > 0.2
        what = "tower %s %s" % (kind, be.name)
        # output conv: its dx is the dz of the last tower conv
        check_hob((dzs[1], g[oname + "_weight"].reshape(nout, C), g[oname + "_bias"]), d, acts[2], ow.reshape(nout, C), dt, ss[1], True, False, what)
        for i in (1, 0):
            check_wgrad(g[stem % (2 + i)], acts[i], dzs[i], False, "%s dW %d" % (what, i))
            ref = CM.conv_ref64(dzs[i].transpose(0, 3, 1, 2), M.flip_weight(ws[i]), dt, fold=True).transpose(0, 2, 3, 1)
            over, worst = CM.conv_check(dxs[i], ref, dt)
            print("%s dx %d: over tolerance %d, worst err / tol %.3g" % (what, i, over, worst))
            assert over == 0, (what, i, over, worst)
            if i > 0:
                want = M.relu_affine_bwd(dxs[i], acts[i], ss[i - 1], dt)
                assert (to_bits(dzs[i - 1], dt) == to_bits(want, dt)).all(), (what, i)
        assert vals16(be, dx, dt).tobytes() == dxs[0].tobytes()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_single_step_functions(be, dt):
    """the module's functions for the single steps (B 1, 2 x 9, 64 -> 64, integer inputs): weight gradient and output-conv backward equal
    to the model in every bit, the data gradient within conv_model.conv_tol"""
    from rangedet_amd import backward as BK
    A, L = be.alloc, be.lib
    B, H, W, C = 1, 2, 9, 64
    xv, zv = rnd("ints", (B, H, W, C), dt, 91), rnd("ints", (B, H, W, C), dt, 92)
    x, dz = dev16(be, to_bits(xv, dt), dt), dev16(be, to_bits(zv, dt), dt)
    rng = np.random.default_rng(93)
    w = rng.integers(-3, 4, (C, C, 3, 3)).astype(np.float32)
    dW = BK.conv3x3_weight_grad(x, dz, dtype=dt, lib=L, alloc=A)
    dx = BK.conv3x3_data_grad(dz, w, dtype=dt, lib=L, alloc=A)
    A.sync()
    assert same_bits(np.array(A.to_numpy(dW)), M.weight_grad(xv, zv, want_abs=False)[0])
    ref = CM.conv_ref64(zv.transpose(0, 3, 1, 2), M.flip_weight(w), dt, fold=True).transpose(0, 2, 3, 1)
    assert CM.conv_check(vals16(be, dx, dt), ref, dt)[0] == 0
    ow, d = rng.integers(-3, 4, (8, C)).astype(np.float32), rng.integers(-3, 4, (B, 5 + H * W, 8)).astype(np.float32)
    dxo, dw, db = BK.head_out_backward(A.as_device_f32(d), x, ow, n_off=5, dtype=dt, lib=L, alloc=A)
    A.sync()
    m = M.head_out_bwd(d[:, 5:], xv.reshape(B, H * W, C), ow)
    assert same_bits(np.array(A.to_numpy(dw)), m["dw"]) and same_bits(np.array(A.to_numpy(db)), m["dbias"])
    assert same_bits(vals16(be, dxo, dt).reshape(B, H * W, C), m["dx"])


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_head_tower_backward_refusals(be):
    from rangedet_amd.backward import HeadTowerBackward
    A, L = be.alloc, be.lib
    one, zero = np.ones(128, np.float32), np.zeros(128, np.float32)
    ow, ob = np.zeros((1, 128), np.float32), np.zeros(1, np.float32)
    with pytest.raises(NotImplementedError, match="concat"):        # the level-0 conv_0: 64 + 8 input channels
        HeadTowerBackward([np.zeros((128, 72, 3, 3), np.float32)], [one], [zero], ow, ob, level=0, lib=L, alloc=A)
    with pytest.raises(NotImplementedError, match="3x3"):
        HeadTowerBackward([np.zeros((128, 128, 1, 1), np.float32)], [one], [zero], ow, ob, lib=L, alloc=A)
    with pytest.raises(NotImplementedError, match="16-bit"):
        HeadTowerBackward([np.zeros((128, 128, 3, 3), np.float32)], [one], [zero], ow, ob, dtype=R.RD_F32, lib=L, alloc=A)
    with pytest.raises(NotImplementedError, match="outputs"):
        HeadTowerBackward([np.zeros((128, 128, 3, 3), np.float32)], [one], [zero], np.zeros((7, 128), np.float32), np.zeros(7, np.float32), lib=L, alloc=A)
    t = HeadTowerBackward([np.zeros((128, 128, 3, 3), np.float32)], [one], [zero], ow, ob, lib=L, alloc=A)
    with pytest.raises(RuntimeError, match="forward"):
        t.backward(np.zeros((1, 8), np.float32))

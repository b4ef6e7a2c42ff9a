"""A backbone BasicBlock in training mode (csrc/k_norm.h: rd_affine_add_relu, rd_bn_add_relu_bwd; csrc/k_convbwd.h: rd_conv1x1_bwd_weight;
csrc/k_optim.h: the images of a 1x1 weight; rangedet_amd.backbone_train.BasicBlockTrain / ResStageTrain) against tests/block_model.py,
the restatement of the formulas in include/rangedet_hip.h.  Through the C ABI, in the style of test_batch_norm.py and
test_conv_backward.py: every output buffer and the workspace are pre-filled with 0xFF bytes and carry a guard tail; the tail and the
channels outside [coff, coff + C) must be unchanged afterwards; each step is compared with the model fed THE KERNEL'S OWN inputs to it.

  rd_affine_add_relu      bit-equal to h16_round(max(fma32(z, a, b) + u, 0)), u = r or fma32(r, ar, br); relu 0 and 1; in place
  rd_bn_add_relu_bwd      the identity dr is g under the restated mask in every bit (that IS the mask); dbeta, dgamma, dgamma_r within
                          convbwd_model.sum_bound on random inputs and bit-equal on integer inputs at every shape and split; dbeta_r has the
                          bytes of dbeta; dz and the projection dr within norm_model's dz tolerance of the formula on the launch's own sums
  rd_conv1x1_bwd_weight   a float64 einsum, sum_bound; exact inputs equal in every bit at every split, the partial count asserted
  optimizer               the images of (cout, cin, 1, 1) weights equal the host packer on the downloaded master, byte for byte
  BasicBlockTrain         every kept intermediate step by step on the block's own previous tensors; dx = round16(data gradient + shortcut
                          gradient) within conv_model.conv_tol of the float64 sum of the launch's own inputs
  the model itself        block_model.block_backward against torch.autograd in float64, to a relative 1e-9
"""
import numpy as np
import pytest

import block_model as BM
import conv_model as CM
import convbwd_model as M
import norm_model as N
import optim_model as OM
from conftest import BOTH, HIP_ONLY
from rangedet_amd import lib as R
from train_util import DTS, GUARD, back, back_image, check_wgrad, dev16, ff, from_bits, image, rnd, same_bits, to_bits, vals16

F32 = np.float32
EPS, MOM = 1e-5 + 1e-10, 0.9
SHAPES = [(1, 2, 9, 64), (2, 3, 37, 128), (2, 5, 70, 64), (1, 4, 70, 128)]        # 18, 222, 700 pixels: 1, 4 and 11 partial sums
SPLITS = (1, 2, 3, 7, 0)
STRIDED = dict(cs=136, co=8)
PT = BM.PT
IDS = dict(ids=lambda s: "x".join(str(v) for v in s))


def fvec(be, buf, C, what):
    return back(be, buf, C * 4, what).view(F32).copy()


def ulps(a, b):
    ua, ub = (np.ascontiguousarray(v, dtype=F32).view(np.uint32).astype(np.int64) for v in (a, b))
    return np.abs(ua - ub)


_Z = {}


def zcase(shape, dt, seed):
    """mean 0.3 s, deviation s per channel (s in 0.5 .. 2), rounded to dt, made once"""
    key = (tuple(shape), dt, seed)
    if key not in _Z:
        rng = np.random.default_rng(seed)
        s = rng.uniform(0.5, 2.0, shape[3])
        v = from_bits(to_bits((0.3 * s + s * rng.standard_normal(shape)).astype(F32), dt), dt)
        v.setflags(write=False)
        _Z[key] = v
    return _Z[key]


def fold_of(v, dt, seed):
    """mean, rstd of v itself (float32), gamma in 0.5 .. 1.5, beta small -> a, b, mean, rstd, gamma"""
    C = v.shape[-1]
    rng = np.random.default_rng(seed)
    m, var = N.stats(v.reshape(-1, C))
    mean, rstd = m.astype(F32), (1.0 / np.sqrt(var + EPS)).astype(F32)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(F32), rng.normal(0, 0.05, C).astype(F32)
    a, b = N.fold_ab_f32(mean, rstd, gamma, beta)
    return a, b, mean, rstd, gamma


def within(got, want, bound, what):
    """|got - want| <= bound per element, equal where the bound is zero -> worst err / bound"""
    err = np.abs(np.asarray(got, np.float64) - want)
    assert np.isfinite(err).all(), what
    assert (err[bound == 0] == 0).all(), what
    worst = float((err[bound > 0] / bound[bound > 0]).max(initial=0))
    print(what, "worst err / bound %.3g" % worst)
    assert worst <= 1, (what, worst)


# ---- rd_affine_add_relu ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_affine_add_relu_bits(be, dt):
    L = be.lib
    for (B, H, W, C), lay in [(s, {}) for s in SHAPES] + [((2, 3, 37, 128), STRIDED)]:
        z, r = zcase((B, H, W, C), dt, 1301), rnd("normal", (B, H, W, C), dt, 1302)
        rng = np.random.default_rng(1303)
        a, b = rng.uniform(-1.5, 1.5, C).astype(F32), rng.normal(0, 0.5, C).astype(F32)
        ar, br = rng.uniform(-1.5, 1.5, C).astype(F32), rng.normal(0, 0.5, C).astype(F32)
        cs, co = lay.get("cs", C), lay.get("co", 0)
        zd, rd, vd = be.up(image(z, dt, cs, co)), be.up(image(r, dt, cs + 16, co + 16)), [be.up(v) for v in (a, b, ar, br)]
        for proj in (False, True):
            for relu in (1, 0):
                out = ff(be, B * H * W * (cs + 8) * 2)
                L.call("rd_affine_add_relu", be.ptr(zd), cs, co, be.ptr(vd[0]), be.ptr(vd[1]), be.ptr(rd), cs + 16, co + 16,
                       be.ptr(vd[2]) if proj else None, be.ptr(vd[3]) if proj else None, relu, be.ptr(out), cs + 8, co + 8, B, H, W, C, dt, be.stream)
                got = back_image(be, out, (B, H, W, C), cs + 8, co + 8, dt, "y")
                want = to_bits(BM.add_relu_f32(z, a, b, r, ar if proj else None, br if proj else None, dt, bool(relu)), dt)
                same = (got == want) | ((from_bits(got, dt) == 0) & (from_bits(want, dt) == 0))
                assert same.all(), ((B, H, W, C), proj, relu, int((~same).sum()))
                if relu:
                    assert 0.3 < (from_bits(got, dt) == 0).mean() < 0.7            # about half of the sums are negative
        # in place: y is z
        zbuf = be.up(image(z, dt, cs, co))
        L.call("rd_affine_add_relu", be.ptr(zbuf), cs, co, be.ptr(vd[0]), be.ptr(vd[1]), be.ptr(rd), cs + 16, co + 16, be.ptr(vd[2]), be.ptr(vd[3]), 1,
               be.ptr(zbuf), cs, co, B, H, W, C, dt, be.stream)
        raw = be.down(zbuf, np.uint16, (B, H, W, cs))
        want = to_bits(BM.add_relu_f32(z, a, b, r, ar, br, dt), dt)
        got = raw[..., co:co + C]
        assert ((got == want) | ((from_bits(got, dt) == 0) & (from_bits(want, dt) == 0))).all(), ("in place", (B, H, W, C))
        outside = np.ones(cs, bool)
        outside[co:co + C] = False
        assert (raw[..., outside] == CM.PAD_PATTERN).all()


# ---- rd_bn_add_relu_bwd ------------------------------------------------------------------------------------------------------------------------
def run_add_bwd(be, dt, g, z, r, main, sc=None, split=0, cs=None, co=0, twice=False):
    """main = (a, b, mean, rstd, gamma); sc = (ar, br, mean_r, rstd_r, gamma_r) or None -> dz, dr (values), dgamma, dbeta, dgamma_r, dbeta_r"""
    L = be.lib
    B, H, W, C = z.shape
    proj = sc is not None
    nws = L.raw("rd_bn_add_relu_bwd_workspace_bytes")(B, H, W, C, split, 1 if proj else 0)
    assert nws > 0 and nws == N.parts(B * H * W, split) * (3 if proj else 2) * C * 4
    cs = cs or C
    gd, zd, rd = be.up(image(g, dt, cs, co)), be.up(image(z, dt, cs + 8, co + 8)), be.up(image(r, dt, cs + 24, co + 24))
    vecs = [be.ptr(be.up(np.ascontiguousarray(v, dtype=F32))) for v in main] + ([be.ptr(be.up(np.ascontiguousarray(v, dtype=F32))) for v in sc] if proj else [None] * 5)
    outs = []
    for _ in range(2 if twice else 1):
        dz, dr, ws = ff(be, B * H * W * (cs + 16) * 2), ff(be, B * H * W * (cs + 32) * 2), ff(be, nws)
        dg, db, dgr, dbr = (ff(be, C * 4) for _ in range(4))
        L.call("rd_bn_add_relu_bwd", be.ptr(gd), cs, co, be.ptr(zd), cs + 8, co + 8, be.ptr(rd), cs + 24, co + 24, *vecs, be.ptr(dz), cs + 16, co + 16,
               be.ptr(dr), cs + 32, co + 32, be.ptr(dg), be.ptr(db), be.ptr(dgr) if proj else None, be.ptr(dbr) if proj else None, B, H, W, C, split,
               dt, be.ptr(ws), nws, be.stream)
        back(be, ws, nws, "workspace")
        res = [from_bits(back_image(be, dz, (B, H, W, C), cs + 16, co + 16, dt, "dz"), dt),
               from_bits(back_image(be, dr, (B, H, W, C), cs + 32, co + 32, dt, "dr"), dt), fvec(be, dg, C, "dgamma"), fvec(be, db, C, "dbeta")]
        if proj:
            res += [fvec(be, dgr, C, "dgamma_r"), fvec(be, dbr, C, "dbeta_r")]
        else:
            assert (back(be, dgr, C * 4, "dgamma_r") == 0xFF).all() and (back(be, dbr, C * 4, "dbeta_r") == 0xFF).all()
            res += [None, None]
        outs.append(res)
    if twice:
        assert all(x is None or x.tobytes() == y.tobytes() for x, y in zip(*outs)), "two calls differ"
    return outs[0]


def check_dz(dz, m, gamma, rstd, dgamma, dbeta, n, dt, what, zh="zh"):
    v, scale = N.bn_dz(dict(gy=m["gy"], zh=m[zh]), gamma, rstd, dgamma, dbeta, n)
    within(dz.reshape(v.shape), v, CM.half_ulp_of(v, dt) + N.DZ_K * N.U * scale, what)


def check_add_bwd(got, g, z, r, main, sc, dt, exact, what):
    """g, z, r: the values the launch read -> the fraction of the mask that is zero"""
    dz, dr, dgamma, dbeta, dgamma_r, dbeta_r = got
    a, b, mean, rstd, gamma = main
    C = z.shape[-1]
    g2, z2, r2 = g.reshape(-1, C), z.reshape(-1, C), r.reshape(-1, C)
    n = z2.shape[0]
    proj = sc is not None
    mask = BM.add_mask_f32(z2, a, b, r2, sc[0] if proj else None, sc[1] if proj else None)
    m = BM.bn_add_bwd(g2, z2, r2, mask, mean, rstd, sc[2] if proj else None, sc[3] if proj else None)
    sums = [("dbeta", dbeta), ("dgamma", dgamma)] + ([("dgamma_r", dgamma_r)] if proj else [])
    for name, got_ in sums:
        if exact:
            assert same_bits(got_, m[name]), (what, name)
        else:
            within(got_, m[name], M.sum_bound(n, m[name + "_abs"]), "%s %s" % (what, name))
    check_dz(dz, m, gamma, rstd, dgamma, dbeta, n, dt, what + " dz")
    if proj:
        assert dbeta_r.tobytes() == dbeta.tobytes(), what
        check_dz(dr, m, sc[4], sc[3], dgamma_r, dbeta, n, dt, what + " dr", zh="zhr")
    else:
        want = np.where(mask, g2, F32(0)).astype(F32)                    # the restated mask, bit for bit: g is non-zero almost everywhere
        assert same_bits(dr.reshape(n, C), want), (what, "identity dr", int((dr.reshape(n, C) != want).sum()))
    off = ~mask
    if off.any() and not exact:          # a masked pixel still carries -gamma rstd (c1 + zh c2)
        assert (dz.reshape(n, C)[off] != 0).mean() > 0.5, what
    return float(off.mean())


def sc_case(shape, dt, seed):
    r = zcase(shape, dt, seed)
    return r, fold_of(r, dt, seed + 1)


@pytest.mark.parametrize("shape", SHAPES, **IDS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_bn_add_relu_bwd_random(be, dt, shape):
    z, g = zcase(shape, dt, 1401), rnd("normal", shape, dt, 1402)
    main = fold_of(z, dt, 1403)
    rid = rnd("normal", shape, dt, 1404)
    rpr, sc = sc_case(shape, dt, 1405)
    for r, s, kind in ((rid, None, "identity"), (rpr, sc, "projection")):
        for split in (0, 3):
            got = run_add_bwd(be, dt, g, z, r, main, s, split=split, twice=split == 0)
            zero = check_add_bwd(got, g, z, r, main, s, dt, False, "add bwd %s %r split %d %s" % (kind, shape, split, be.name))
            assert 0.35 < zero < 0.65, zero


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_bn_add_relu_bwd_channel_stride_and_offset(be, dt):
    shape = (2, 3, 37, 128)
    z, g = zcase(shape, dt, 1411), rnd("normal", shape, dt, 1412)
    main = fold_of(z, dt, 1413)
    r, sc = sc_case(shape, dt, 1414)
    for s in (None, sc):
        got = run_add_bwd(be, dt, g, z, r, main, s, split=2, **STRIDED)
        check_add_bwd(got, g, z, r, main, s, dt, False, "add bwd strided %s %s" % ("projection" if s else "identity", be.name))


@pytest.mark.parametrize("shape", SHAPES, **IDS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_bn_add_relu_bwd_exact_every_split(be, dt, shape):
    """g, z, r integers in -3 .. 3, means 0, rstd 1, a = ar = 1, b 0 or -0.5, br 0.5: every partial sum is an integer below 2^24, the two or
    three sums equal the model in every bit at every split -- one dropped or doubled pixel shows"""
    C = shape[3]
    g, z, r = (rnd("ints", shape, dt, s) for s in (1421, 1422, 1423))
    one, zero = np.ones(C, F32), np.zeros(C, F32)
    gamma, gamma_r = (np.random.default_rng(s).uniform(0.5, 1.5, C).astype(F32) for s in (1424, 1425))
    for split in SPLITS:
        for bval in (0.0, -0.5):
            main = (one, np.full(C, bval, F32), zero, one, gamma)
            for sc in (None, (one, np.full(C, 0.5, F32), zero, one, gamma_r)):
                got = run_add_bwd(be, dt, g, z, r, main, sc, split=split)
                check_add_bwd(got, g, z, r, main, sc, dt, True, "add bwd exact %r split %d b %g %s" % (shape, split, bval, be.name))


# ---- rd_conv1x1_bwd_weight ---------------------------------------------------------------------------------------------------------------------
def run_wgrad1(be, dt, x, dz, xcs=None, xco=0, zcs=None, zco=0, split=0, twice=False):
    L = be.lib
    B, H, W, cin = x.shape
    cout = dz.shape[3]
    nws = L.raw("rd_conv1x1_bwd_weight_workspace_bytes")(B, H, W, cin, cout, split)
    assert nws > 0 and nws % (4 * cin * cout) == 0
    xd, zd = be.up(image(x, dt, xcs, xco)), be.up(image(dz, dt, zcs, zco))
    outs = []
    for _ in range(2 if twice else 1):
        dW, ws = ff(be, cout * cin * 4), ff(be, nws)
        L.call("rd_conv1x1_bwd_weight", be.ptr(xd), xcs or cin, xco, be.ptr(zd), zcs or cout, zco, be.ptr(dW), B, H, W, cin, cout, split, dt,
               be.ptr(ws), nws, be.stream)
        back(be, ws, nws, "workspace")
        outs.append(back(be, dW, cout * cin * 4, "dW"))
    if twice:
        assert outs[0].tobytes() == outs[1].tobytes(), "two calls differ"
    S = nws // (4 * cin * cout)
    assert S == BM.parts1x1(B * H * W, split)
    return outs[0].view(F32).reshape(cout, cin).copy(), S


def check_wgrad1(got, x, dz, exact, what):
    want, sabs, n = BM.weight_grad1x1(x, dz, want_abs=not exact)
    assert np.isfinite(got).all(), what
    if exact:
        assert same_bits(got, want), (what, int((got != want.astype(F32)).sum()))
    else:
        within(got, want, M.sum_bound(n, sabs), what)


def wgrad1_case(be, dt, shape, cin, cout, what, split=0, **lay):
    """one shape: normal inputs, ReLU-sparse x, exact inputs"""
    B, H, W = shape
    for kind, zkind, exact in (("normal", "normal", False), ("relu", "normal", False), ("ints", "ints", True)):
        x, dz = rnd(kind, (B, H, W, cin), dt, 1511), rnd(zkind, (B, H, W, cout), dt, 1512)
        if kind == "relu":
            assert 0.4 < (x == 0).mean() < 0.6
        got, _ = run_wgrad1(be, dt, x, dz, split=split, **lay)
        check_wgrad1(got, x, dz, exact, "%s %s %s" % (what, kind, be.name))


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (128, 64), (128, 128)])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_weight_grad1x1_channel_pairs(be, dt, cin, cout):
    """B 2, 3 x 37 = 222 pixels: three full pixel tiles and one of 30"""
    wgrad1_case(be, dt, (2, 3, 37), cin, cout, "1x1 2x3x37 %d->%d" % (cin, cout))


@pytest.mark.parametrize("shape", [(2, 1, 37), (2, 3, 1), (1, 1, PT - 1), (1, 1, PT), (1, 1, PT + 1)], **IDS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_weight_grad1x1_edge_shapes(be, dt, shape):
    """one row, one column (six pixels), and a run of pixels one below, at and one above the 64-pixel tile"""
    wgrad1_case(be, dt, shape, 64, 64, "1x1 %dx%dx%d" % shape)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_weight_grad1x1_channel_stride_and_offset(be, dt):
    """x: 128 channels at offset 8 of 136; dz: 64 channels at offset 16 of 88"""
    wgrad1_case(be, dt, (1, 3, 37), 128, 64, "1x1 1x3x37 strided", xcs=136, xco=8, zcs=88, zco=16)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_weight_grad1x1_reduction_split(be, dt):
    """B 2, 17 x 70 = 2380 pixels = 38 tiles (the last of 12 pixels).  split 3: runs of 12, 13 and 13 tiles; the library's own split:
    ceil(38 / 8) = 5 workgroups of 7 or 8 tiles; split 1: one sum.  Exact inputs: all three equal the model in every bit."""
    shape, cin, cout = (2, 17, 70), 64, 128
    x, dz = rnd("ints", shape + (cin,), dt, 1521), rnd("ints", shape + (cout,), dt, 1522)
    for split, parts in ((3, 3), (0, 5), (1, 1)):
        got, S = run_wgrad1(be, dt, x, dz, split=split)
        assert S == parts
        check_wgrad1(got, x, dz, True, "1x1 2x17x70 split %d %s" % (split, be.name))
    x, dz = rnd("relu", shape + (cin,), dt, 1523), rnd("normal", shape + (cout,), dt, 1524)
    check_wgrad1(run_wgrad1(be, dt, x, dz, split=3)[0], x, dz, False, "1x1 2x17x70 split 3 random %s" % be.name)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_weight_grad1x1_determinism(be, dt):
    x, dz = rnd("relu", (2, 3, 37, 128), dt, 1531), rnd("normal", (2, 3, 37, 128), dt, 1532)
    run_wgrad1(be, dt, x, dz, twice=True)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
def test_weight_grad1x1_many_splits_exact(be, dt):
    """B 2, 64 x 332, 128 -> 128, exact inputs: 664 tiles, 83 partial sums per element"""
    x, dz = rnd("ints", (2, 64, 332, 128), dt, 1541), rnd("ints", (2, 64, 332, 128), dt, 1542)
    got, S = run_wgrad1(be, dt, x, dz, twice=True)
    assert S == 83
    check_wgrad1(got, x, dz, True, "1x1 2x64x332 128->128")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_status_codes(be):
    """null pointers, bad channel counts, a workspace one byte short, a misaligned channel offset: each its code, nothing launched (one
    buffer of 0xFF bytes stands for every device pointer and keeps its fill)"""
    L = be.lib
    n = 1 << 20
    buf = be.up(np.full(n, 0xFF, np.uint8))
    p = be.ptr(buf)
    assert p % 16 == 0
    BF = R.RD_BF16
    ws_b, ws_w = L.raw("rd_bn_add_relu_bwd_workspace_bytes"), L.raw("rd_conv1x1_bwd_weight_workspace_bytes")

    def aff(z=p, a=p, r=p, ar=p, br=p, y=p, C=64, B=1, co=0, dt=BF):
        return L.raw("rd_affine_add_relu")(z, C, co, a, p, r, C, 0, ar, br, 1, y, C, 0, B, 2, 8, C, dt, be.stream)

    def bwd(g=p, z=p, r=p, a=p, ar=p, gamma_r=p, dz=p, dr=p, dg=p, dgr=p, dbr=p, ws=p, C=64, B=1, co=0, split=0, dt=BF, nws=n):
        return L.raw("rd_bn_add_relu_bwd")(g, C, co, z, C, 0, r, C, 0, a, p, p, p, p, ar, p if ar else None, p if ar else None, p if ar else None,
                                           gamma_r if ar else None, dz, C, 0, dr, C, 0, dg, p, dgr if ar else None, dbr if ar else None, B, 2, 8, C,
                                           split, dt, ws, nws, be.stream)

    def wg(x=p, dz=p, dW=p, ws=p, cin=64, cout=64, B=1, H=2, W=8, xcs=None, xco=0, split=0, dt=BF, nws=None):
        need = ws_w(1, 2, 8, 64, 64, split) if nws is None else nws
        return L.raw("rd_conv1x1_bwd_weight")(x, xcs or cin, xco, dz, cout, 0, dW, B, H, W, cin, cout, split, dt, ws, need, be.stream)
    assert ws_b(1, 2, 8, 64, 0, 0) == 2 * 64 * 4 and ws_b(1, 2, 8, 64, 0, 1) == 3 * 64 * 4 and ws_b(2, 5, 70, 128, 3, 1) == 3 * 3 * 128 * 4
    assert ws_b(2, 5, 70, 128, 0, 0) == 11 * 2 * 128 * 4 and ws_b(1, 2, 8, 96, 0, 0) == 0 and ws_b(0, 2, 8, 64, 0, 0) == 0 and ws_b(1, 2, 8, 64, -1, 0) == 0
    assert ws_w(1, 2, 8, 64, 64, 0) == 4 * 64 * 64 and ws_w(1, 2, 8, 96, 64, 0) == 0 and ws_w(0, 2, 8, 64, 64, 0) == 0
    assert ws_w(8, 64, 2656, 64, 64, 0) == 512 * 4 * 64 * 64 and ws_w(8, 64, 166, 128, 128, 0) == 166 * 4 * 128 * 128 and ws_w(4, 64, 128, 128, 128, 5) == 5 * 4 * 128 * 128
    for kw in (dict(C=24), dict(C=96), dict(B=0), dict(co=8), dict(co=4)):
        assert aff(**kw) == R.RD_ESHAPE and L.rd_last_error_string().decode().startswith("affine_add_relu"), kw
        assert bwd(**kw) == R.RD_ESHAPE and L.rd_last_error_string().decode().startswith("bn_add_relu_bwd"), kw
    for kw in (dict(cin=96), dict(cout=32), dict(cin=256), dict(B=0), dict(H=0), dict(W=0), dict(xco=4, xcs=72), dict(xcs=60)):
        assert wg(**kw) == R.RD_ESHAPE and L.rd_last_error_string().decode().startswith("conv1x1_bwd_weight"), kw
    for name in ("z", "a", "r", "y"):
        assert aff(**{name: None}) == R.RD_EINVAL and "null" in L.rd_last_error_string().decode(), name
    assert aff(br=None) == R.RD_EINVAL and "together" in L.rd_last_error_string().decode()
    for name in ("g", "z", "r", "a", "dz", "dr", "dg", "ws"):
        assert bwd(**{name: None}) == R.RD_EINVAL and "null" in L.rd_last_error_string().decode(), name
    for name in ("gamma_r", "dgr", "dbr"):
        assert bwd(**{name: None}) == R.RD_EINVAL and "together" in L.rd_last_error_string().decode(), name
    for name in ("x", "dz", "dW", "ws"):
        assert wg(**{name: None}) == R.RD_EINVAL and "null" in L.rd_last_error_string().decode(), name
    assert aff(dt=R.RD_F32) == R.RD_EINVAL and bwd(dt=R.RD_F32) == R.RD_EINVAL and wg(dt=R.RD_F32) == R.RD_EINVAL
    assert bwd(split=-1) == R.RD_EINVAL and wg(split=-1, nws=n) == R.RD_EINVAL
    assert bwd(nws=ws_b(1, 2, 8, 64, 0, 1) - 1) == R.RD_EWORKSPACE and "workspace" in L.rd_last_error_string().decode()
    assert wg(nws=ws_w(1, 2, 8, 64, 64, 0) - 1) == R.RD_EWORKSPACE and "workspace" in L.rd_last_error_string().decode()
    for rc in (aff(z=p + 8), aff(r=p + 8), bwd(g=p + 8), bwd(dr=p + 8), wg(x=p + 8)):
        assert rc == R.RD_EINVAL and "aligned" in L.rd_last_error_string().decode()
    assert (be.down(buf, np.uint8, (n,)) == 0xFF).all()           # nothing ran


# ---- optimizer: the images of a 1x1 weight -------------------------------------------------------------------------------------------------
def fup(be, arr):
    raw = np.ascontiguousarray(arr, dtype=F32).view(np.uint8).reshape(-1)
    return be.up(np.concatenate([raw, np.full(GUARD, 0xFF, np.uint8)]))


def image1x1(L, w, dt, transposed=False):
    w2 = np.asarray(w, F32).reshape(w.shape[0], w.shape[1])
    w2 = np.ascontiguousarray(w2.T if transposed else w2)
    return L.pack_conv_weight(w2.reshape(w2.shape + (1, 1)), dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_optimizer_images_of_1x1_weights(be, dt):
    """a table of a (64, 64, 1, 1) and a (128, 64, 1, 1) weight with both images (the first on exact rounding ties of the type), a
    (64, 128, 3, 3) weight with both images and a bias of 5 elements: after each of two steps every master and momentum equals
    optim_model.sgd_step in every bit and every image equals the host packer on the downloaded master, the zero tail included"""
    L = be.lib
    rng = np.random.default_rng(1601)
    shapes = [(64, 64, 1, 1), (128, 64, 1, 1), (64, 128, 3, 3), (5,)]
    w = [rng.standard_normal(s).astype(F32) for s in shapes]
    ties = OM.tie_values(shapes[0], dt, rng, dt == R.RD_BF16)
    w[0] = ties.copy()
    m = [(0.1 * rng.standard_normal(s)).astype(F32) for s in shapes]
    m[0] = np.zeros(shapes[0], F32)
    wd_mult = [0.0, 1.0, 1.0, 0.0]
    nimg = [L.cdll.rd_conv_packed_bytes(1, 64, 64, dt), L.cdll.rd_conv_packed_bytes(1, 64, 128, dt), 9 * 64 * 128 * 2 + 256]
    assert nimg[0] == 64 * 64 * 2 + 256 and nimg[1] == 128 * 64 * 2 + 256
    wdv, mdv = [fup(be, v) for v in w], [fup(be, v) for v in m]
    grads = [[np.zeros(shapes[0], F32)] + [(10 * rng.standard_normal(s)).astype(F32) for s in shapes[1:]],
             [(10 * rng.standard_normal(s)).astype(F32) for s in shapes]]
    for step, (g, lr) in enumerate(zip(grads, (0.1, 0.05))):
        gdv = [fup(be, v) for v in g]
        fwd, bwd = [ff(be, nb) for nb in nimg] + [None], [ff(be, nb) for nb in nimg] + [None]
        ts = [R.SgdTensor(be.ptr(wdv[i]), be.ptr(gdv[i]), be.ptr(mdv[i]), int(np.prod(s)), 1.0, wd_mult[i], s[0] if len(s) == 4 else 0,
                          s[1] if len(s) == 4 else 0, be.ptr(fwd[i]), be.ptr(bwd[i]), None) for i, s in enumerate(shapes)]
        host = L.sgd_table(ts, dt)
        L.call("rd_sgd_mom_update", be.ptr(be.up(host)), host.ctypes.data, lr, 0.9, 1e-5, 1.0, 35.0, be.stream)
        for i, s in enumerate(shapes):
            w[i], m[i] = OM.sgd_step(w[i], g[i], m[i], lr, 0.9, 1e-5, 1.0, 35.0, 1.0, wd_mult[i])
            got_w = back(be, wdv[i], w[i].nbytes, "weight %d" % i).view(F32).reshape(s)
            got_m = back(be, mdv[i], m[i].nbytes, "mom %d" % i).view(F32).reshape(s)
            assert got_w.tobytes() == w[i].tobytes() and got_m.tobytes() == m[i].tobytes(), ("step", step, "tensor", i)
            if len(s) != 4:
                continue
            if s[2:] == (1, 1):
                want = (image1x1(L, got_w, dt), image1x1(L, got_w, dt, transposed=True))
            else:
                want = (OM.forward_image(L, got_w, None, dt), OM.data_grad_image(L, got_w, dt))
            for img, wt, name in ((fwd[i], want[0], "forward"), (bwd[i], want[1], "data-gradient")):
                assert wt.size == nimg[i]
                got = back(be, img, nimg[i], "%s image %d" % (name, i))
                assert int((got != wt).sum()) == 0 and not got[-256:].any(), ("step", step, "tensor", i, name, int((got != wt).sum()))
        if step == 0:
            assert w[0].tobytes() == ties.tobytes()                   # zero gradient, zero momentum, no decay: tensor 0 still sits on the ties
        else:
            assert (w[0] != ties).mean() > 0.9


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_optimizer_refusals_unchanged(be):
    """an image entry whose n is neither 9 x nor 1 x cout x cin, and channel counts outside {64, 128}, are refused as before"""
    L = be.lib
    buf = be.empty(1 << 16)
    p = be.ptr(buf)
    for n, co, ci, words in ((64 * 64 * 4, 64, 64, "9 x"), (64 * 64, 64, 16, "body form"), (72 * 64, 64, 72, "concat")):
        t = R.SgdTensor(p, p, p, n, 1.0, 1.0, co, ci, p, None, None)
        with pytest.raises(R.RangeDetError, match=words) as e:
            L.sgd_table([t], R.RD_BF16)
        assert e.value.code == R.RD_ESHAPE


# ---- BasicBlockTrain ---------------------------------------------------------------------------------------------------------------------------
def dvec(A, buf, C):
    return np.array(A.to_numpy(A.view_f32(buf, (C,)))).astype(F32)


def block_params(name, cin, cout, proj, seed):
    rng = np.random.default_rng(seed)

    def bn():
        return dict(gamma=rng.uniform(0.5, 1.5, cout).astype(F32), beta=(0.1 * rng.standard_normal(cout)).astype(F32),
                    moving_mean=rng.normal(0, 1, cout).astype(F32), moving_var=rng.uniform(0.5, 2, cout).astype(F32))
    p = dict(name=name, conv1_w=(rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin / 2)).astype(F32), bn1=bn(),
             conv2_w=(rng.standard_normal((cout, cout, 3, 3)) / np.sqrt(9 * cout / 2)).astype(F32), bn2=bn())
    if proj:
        p.update(sc_w=(rng.standard_normal((cout, cin, 1, 1)) / np.sqrt(cin)).astype(F32), sc_bn=bn())
    return p


def make_block(be, dt, p):
    from rangedet_amd.backbone_train import BasicBlockTrain
    return BasicBlockTrain(p["name"], p["conv1_w"], p["conv2_w"], p["bn1"], p["bn2"], p.get("sc_w"), p.get("sc_bn"), dtype=dt, lib=be.lib, alloc=be.alloc)


def nchw(v):
    return v.transpose(0, 3, 1, 2)


def conv_close(got, ref_nchw, dt, what):
    over, worst = CM.conv_check(got, ref_nchw.transpose(0, 2, 3, 1), dt)
    print("%s: over tolerance %d, worst err / tol %.3g" % (what, over, worst))
    assert over == 0, (what, over, worst)


def check_norm(be, A, z, s, bn, n, C, dt, what):
    """statistics within norm_model.stats_bound, rstd within 2 ulp, a and b bit-equal through the launch's own rstd -> the vectors"""
    mean, var, rstd, a, b = (dvec(A, s[k], C) for k in ("mean", "var", "rstd", "a", "b"))
    z2 = z.reshape(-1, C)
    m, v = N.stats(z2)
    bm, bv = N.stats_bound(z2, N.parts(n, 0))
    within(mean, m, bm, what + " mean")
    within(var, v, bv, what + " var")
    want = N.fold_f32(mean, var, bn["gamma"], bn["beta"], EPS, MOM, n, True, mean, var)
    assert int(ulps(rstd, want["rstd"]).max()) <= (0 if be.name == "emu" else 2), what
    a_own, b_own = N.fold_ab_f32(mean, rstd, bn["gamma"], bn["beta"])
    assert same_bits(a, a_own) and same_bits(b, b_own), what
    return mean, var, rstd, a, b


@pytest.mark.parametrize("cin,cout,proj", [(64, 64, False), (128, 128, False), (64, 64, True), (64, 128, True)],
                         ids=["identity64", "identity128", "projection64", "projection64to128"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_basic_block_train(be, dt, cin, cout, proj):
    """B 2, 3 x 37: forward twice (the moving statistics after one and after two), backward twice (the same bytes); every kept tensor
    against the model fed the block's own previous tensors"""
    A = be.alloc
    B, H, W = 2, 3, 37
    n = B * H * W
    name = "agg1_res_unit1" if proj else "res2a_unit2"
    p = block_params(name, cin, cout, proj, 1700 + cin + 2 * cout)
    blk = make_block(be, dt, p)
    x = dev16(be, to_bits(rnd("relu", (B, H, W, cin), dt, 1701), dt), dt)
    g = dev16(be, to_bits(rnd("normal", (B, H, W, cout), dt, 1702), dt), dt)
    bnkeys = ("bn1", "bn2") + (("sc_bn",) if proj else ())
    blk.forward(x)
    A.sync()
    aux1 = {k: np.array(A.to_numpy(v)).copy() for k, v in blk.aux().items()}
    assert sorted(aux1) == sorted("%s_%s_moving_%s" % (name, k, s) for k in bnkeys for s in ("mean", "var"))
    y1st = vals16(be, blk.y, dt).copy()
    dx1st, grads1st = blk.backward(g)
    A.sync()
    first = [vals16(be, dx1st, dt).tobytes()] + [np.array(A.to_numpy(grads1st[k])).tobytes() for k in sorted(grads1st)]
    y = blk.forward(x)
    dx, grads = blk.backward(g)
    A.sync()
    aux2 = {k: np.array(A.to_numpy(v)).copy() for k, v in blk.aux().items()}
    assert vals16(be, y, dt).tobytes() == y1st.tobytes()
    assert [vals16(be, dx, dt).tobytes()] + [np.array(A.to_numpy(grads[k])).tobytes() for k in sorted(grads)] == first, "a second forward / backward differs"
    what = "block %s %d->%d %s" % ("projection" if proj else "identity", cin, cout, be.name)
    # ---- forward
    xv, z1, y1, z2, yv = (vals16(be, v, dt) for v in (blk.x, blk.z1, blk.y1, blk.z2, blk.y))
    zs = vals16(be, blk.zs, dt) if proj else None
    conv_close(z1, CM.conv_ref64(nchw(xv), p["conv1_w"], dt, fold=True), dt, what + " z1")
    vec = {}
    for key, z in (("bn1", z1), ("bn2", z2)) + ((("sc_bn", zs),) if proj else ()):
        vec[key] = check_norm(be, A, z, blk.saved[key], p[key], n, cout, dt, "%s %s" % (what, key))
        mean, var = vec[key][:2]
        f1 = N.fold_f32(mean, var, p[key]["gamma"], p[key]["beta"], EPS, MOM, n, True, p[key]["moving_mean"], p[key]["moving_var"])
        f2 = N.fold_f32(mean, var, p[key]["gamma"], p[key]["beta"], EPS, MOM, n, True, f1["moving_mean"], f1["moving_var"])
        for aux, f in ((aux1, f1), (aux2, f2)):
            assert same_bits(aux["%s_%s_moving_mean" % (name, key)], f["moving_mean"]) and same_bits(aux["%s_%s_moving_var" % (name, key)], f["moving_var"])
    a1, b1 = vec["bn1"][3:]
    assert same_bits(y1, N.affine_relu_f32(z1, a1, b1, dt)), what
    assert 0.2 < (y1 == 0).mean() < 0.8
    conv_close(z2, CM.conv_ref64(nchw(y1), p["conv2_w"], dt, fold=True), dt, what + " z2")
    if proj:
        conv_close(zs, CM.conv_ref64(nchw(xv), p["sc_w"], dt), dt, what + " zs")
    r = zs if proj else xv
    a2, b2 = vec["bn2"][3:]
    ars, brs = vec["sc_bn"][3:] if proj else (None, None)
    assert same_bits(yv, BM.add_relu_f32(z2, a2, b2, r, ars, brs, dt)), what
    assert 0.2 < (yv == 0).mean() < 0.8
    # ---- backward
    want_names = ["%s_%s" % (name, s) for s in ("conv1_weight", "bn1_gamma", "bn1_beta", "conv2_weight", "bn2_gamma", "bn2_beta")]
    if proj:
        want_names += ["%s_%s" % (name, s) for s in ("sc_weight", "sc_bn_gamma", "sc_bn_beta")]
    assert sorted(grads) == sorted(want_names)
    gr = {k[len(name) + 1:]: np.array(A.to_numpy(v)) for k, v in grads.items()}
    assert gr["conv1_weight"].shape == (cout, cin, 3, 3) and gr["conv2_weight"].shape == (cout, cout, 3, 3) and gr["bn2_gamma"].shape == (cout,)
    gv, dz2, dr, g1, dz1, dxv = (vals16(be, v, dt) for v in (blk.g, blk.dz2, blk.dr, blk.g1, blk.dz1, blk.dx))
    main = (a2, b2) + vec["bn2"][0:1] + vec["bn2"][2:3] + (p["bn2"]["gamma"],)
    sc = (ars, brs, vec["sc_bn"][0], vec["sc_bn"][2], p["sc_bn"]["gamma"]) if proj else None
    got = (dz2, dr, gr["bn2_gamma"], gr["bn2_beta"], gr.get("sc_bn_gamma"), gr.get("sc_bn_beta"))
    zero = check_add_bwd(got, gv, z2, r, main, sc, dt, False, what + " bn2")
    assert 0.2 < zero < 0.8
    check_wgrad(gr["conv2_weight"], y1, dz2, False, what + " dW2")
    conv_close(g1, CM.conv_ref64(nchw(dz2), M.flip_weight(p["conv2_w"]), dt, fold=True), dt, what + " g1")
    mean1, rstd1 = vec["bn1"][0], vec["bn1"][2]
    m1 = N.bn_bwd(g1.reshape(n, cout), z1.reshape(n, cout), N.mask_f32(z1.reshape(n, cout), a1, b1), mean1, rstd1)
    within(gr["bn1_beta"], m1["dbeta"], M.sum_bound(n, m1["dbeta_abs"]), what + " dbeta1")
    within(gr["bn1_gamma"], m1["dgamma"], M.sum_bound(n, m1["dgamma_abs"]), what + " dgamma1")
    check_dz(dz1, m1, p["bn1"]["gamma"], rstd1, gr["bn1_gamma"], gr["bn1_beta"], n, dt, what + " dz1")
    check_wgrad(gr["conv1_weight"], xv, dz1, False, what + " dW1")
    if proj:
        assert gr["sc_weight"].shape == (cout, cin, 1, 1)
        check_wgrad1(gr["sc_weight"].reshape(cout, cin), xv, dr, False, what + " dWs")
        ds = vals16(be, blk.ds, dt)
        conv_close(ds, CM.conv_ref64(nchw(dr), np.ascontiguousarray(p["sc_w"].transpose(1, 0, 2, 3)), dt), dt, what + " ds")
    short = ds if proj else dr
    conv_close(dxv, CM.conv_ref64(nchw(dz1), M.flip_weight(p["conv1_w"]), dt, fold=True, flags=R.RD_ADD, res=nchw(short)), dt, what + " dx")
    assert float(np.abs(short).max()) > 0 and vals16(be, dx, dt).tobytes() == dxv.tobytes()


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_basic_block_train_refusals(be):
    from rangedet_amd.backbone_train import BasicBlockTrain
    A, L = be.alloc, be.lib
    bn = dict(gamma=np.ones(64, F32), beta=np.zeros(64, F32), moving_mean=np.zeros(64, F32), moving_var=np.ones(64, F32))
    bn128 = {k: np.resize(v, 128) for k, v in bn.items()}
    w = np.zeros((64, 64, 3, 3), F32)

    def make(w1=w, w2=w, b1=bn, b2=bn, **kw):
        return BasicBlockTrain("res2_unit1", w1, w2, b1, b2, lib=L, alloc=A, **kw)
    with pytest.raises(NotImplementedError, match="strided"):
        make(stride=(1, 2), sc_w=np.zeros((64, 64, 1, 1), F32), sc_bn=bn)
    with pytest.raises(NotImplementedError, match="fewer than 64 input channels"):
        make(w1=np.zeros((64, 8, 3, 3), F32), sc_w=np.zeros((64, 8, 1, 1), F32), sc_bn=bn)
    with pytest.raises(NotImplementedError, match="Meta-Kernel"):
        make(meta_kernel=True)
    with pytest.raises(NotImplementedError, match="64 or 128"):
        make(w1=np.zeros((256, 64, 3, 3), F32), w2=np.zeros((256, 256, 3, 3), F32))
    with pytest.raises(NotImplementedError, match="identity shortcut"):
        make(w1=np.zeros((128, 64, 3, 3), F32), w2=np.zeros((128, 128, 3, 3), F32), b1=bn128, b2=bn128)
    with pytest.raises(NotImplementedError, match="16-bit"):
        make(dtype=R.RD_F32)
    with pytest.raises(RuntimeError, match="forward"):
        make().backward(np.zeros((1, 2, 8, 64), np.uint16))


# ---- ResStageTrain -----------------------------------------------------------------------------------------------------------------------------
def host_params(A, blk, p):
    """the block's parameters as they are on the device now, in block_params's form"""
    q = dict(name=p["name"])
    for key, wkey, shape in (("conv1", "conv1_w", p["conv1_w"].shape), ("conv2", "conv2_w", p["conv2_w"].shape)) + (
            (("sc", "sc_w", p["sc_w"].shape),) if "sc_w" in p else ()):
        q[wkey] = np.array(A.to_numpy(A.view_f32(blk.convs[key]["master"], shape))).astype(F32)
    for key in blk.bns:
        q[key] = {k: dvec(A, blk.bns[key][k], blk.cout) for k in ("gamma", "beta", "moving_mean", "moving_var")}
    return q


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_res_stage_train_and_sgd(be, dt):
    """a projection block 64 -> 128 then an identity block at 128 (B 1, 3 x 37): all gradient names; after SGD.attach(stage), step(), the
    next forward equals, bit for bit, the forward of a fresh stage built from the downloaded masters and vectors"""
    from rangedet_amd.backbone_train import ResStageTrain
    from rangedet_amd.optim import SGD
    A = be.alloc
    B, H, W = 1, 3, 37
    ps = [block_params("agg2_res_unit1", 64, 128, True, 1801), block_params("agg2_res_unit2", 128, 128, False, 1802)]
    stage = ResStageTrain([make_block(be, dt, p) for p in ps])
    x = dev16(be, to_bits(rnd("relu", (B, H, W, 64), dt, 1803), dt), dt)
    g = dev16(be, to_bits(rnd("normal", (B, H, W, 128), dt, 1804), dt), dt)
    opt = SGD(lr=0.05, lib=be.lib, alloc=A)
    opt.attach(stage)
    y0 = vals16(be, stage.forward(x), dt).copy()
    dx, grads = stage.backward(g)
    A.sync()
    names = ["agg2_res_unit%d_%s" % (u, s) for u in (1, 2) for s in ("conv1_weight", "bn1_gamma", "bn1_beta", "conv2_weight", "bn2_gamma", "bn2_beta")]
    names += ["agg2_res_unit1_%s" % s for s in ("sc_weight", "sc_bn_gamma", "sc_bn_beta")]
    assert sorted(grads) == sorted(names) and sorted(opt.state()) == sorted(names)
    assert tuple(dx.shape) == (B, H, W, 64) and all(np.isfinite(np.array(A.to_numpy(v))).all() and np.array(A.to_numpy(v)).any() for v in grads.values())
    assert sorted(stage.aux()) == sorted(["agg2_res_unit%d_%s_moving_%s" % (u, k, s) for u in (1, 2) for k in ("bn1", "bn2") for s in ("mean", "var")]
                                         + ["agg2_res_unit1_sc_bn_moving_%s" % s for s in ("mean", "var")])
    # the second block's input gradient is what the first block's backward read
    assert vals16(be, stage.blocks[0].g, dt).tobytes() == vals16(be, stage.blocks[1].dx, dt).tobytes()
    before = [host_params(A, b, p) for b, p in zip(stage.blocks, ps)]
    opt.step()
    y1 = vals16(be, stage.forward(x), dt).copy()
    A.sync()
    after = [host_params(A, b, p) for b, p in zip(stage.blocks, ps)]
    for q0, q1 in zip(before, after):
        for k in ("conv1_w", "conv2_w") + (("sc_w",) if "sc_w" in q0 else ()):
            assert (q0[k] != q1[k]).mean() > 0.9, k
        assert (q0["bn2"]["gamma"] != q1["bn2"]["gamma"]).mean() > 0.9
    assert (y1 != y0).mean() > 0.3
    fresh = ResStageTrain([make_block(be, dt, q) for q in after])
    yf = vals16(be, fresh.forward(x), dt)
    assert yf.tobytes() == y1.tobytes(), int((yf != y1).sum())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_single_step_functions(be, dt):
    """the module's functions for the single steps (B 2, 3 x 37, 64 channels) against the model"""
    from rangedet_amd import backbone_train as BT
    from rangedet_amd import backward as BK
    A, L = be.alloc, be.lib
    shape = (2, 3, 37, 64)
    C, n = 64, 222
    zv, gv = zcase(shape, dt, 1901), rnd("normal", shape, dt, 1902)
    rv, sc = sc_case(shape, dt, 1903)
    main = fold_of(zv, dt, 1905)
    z, g, r = (dev16(be, to_bits(v, dt), dt) for v in (zv, gv, rv))
    y = BT.batch_norm_add_relu_forward(z, main[0], main[1], r, sc[0], sc[1], dtype=dt, lib=L, alloc=A)
    A.sync()
    assert same_bits(vals16(be, y, dt), BM.add_relu_f32(zv, main[0], main[1], rv, sc[0], sc[1], dt))
    up = lambda v: A.upload(np.ascontiguousarray(v, dtype=F32))
    saved, saved_r = (dict(a=up(s[0]), b=up(s[1]), mean=up(s[2]), rstd=up(s[3])) for s in (main, sc))
    for s_r, s_c in ((None, None), (saved_r, sc)):
        got = BT.batch_norm_add_relu_backward(g, z, r, saved, main[4], s_r, None if s_c is None else s_c[4], dtype=dt, lib=L, alloc=A)
        A.sync()
        got = [vals16(be, got[0], dt), vals16(be, got[1], dt)] + [None if v is None else np.array(A.to_numpy(v)) for v in got[2:]]
        check_add_bwd(got, gv, zv, rv, main, s_c, dt, False, "single-step add bwd %s" % be.name)
    xv, dzv = rnd("ints", shape, dt, 1906), rnd("ints", (2, 3, 37, 128), dt, 1907)
    xd, dzd = dev16(be, to_bits(xv, dt), dt), dev16(be, to_bits(dzv, dt), dt)
    dW = BT.conv1x1_weight_grad(xd, dzd, dtype=dt, lib=L, alloc=A)
    w = np.random.default_rng(1908).integers(-3, 4, (128, 64, 1, 1)).astype(F32)
    dx = BT.conv1x1_data_grad(dzd, w, dtype=dt, lib=L, alloc=A)
    A.sync()
    assert tuple(dW.shape) == (128, 64, 1, 1) and same_bits(np.array(A.to_numpy(dW)).reshape(128, 64), BM.weight_grad1x1(xv, dzv, want_abs=False)[0])
    conv_close(vals16(be, dx, dt), CM.conv_ref64(nchw(dzv), np.ascontiguousarray(w.transpose(1, 0, 2, 3)), dt), dt, "single-step 1x1 data gradient")


# ---- the formulas ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proj", [False, True], ids=["identity", "projection"])
def test_model_block_matches_autograd(proj):
    """CPU only, no library: block_model.block_backward against torch float64 autograd on conv2d, batch_norm(training=True), add, relu with a
    linear loss on top, to 1e-9 of the largest value of each gradient.  No pre-activation of either ReLU lies within 1e-6 of zero, so no
    mask can tie.  This pins the add-before-ReLU order and the shortcut BatchNorm's gradient, which somebody typed."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(2001 + proj)
    B, H, W, cin = 2, 4, 5, 6
    cout = 7 if proj else 6
    x = rng.standard_normal((B, H, W, cin))
    w1, w2 = rng.standard_normal((cout, cin, 3, 3)) / 7, rng.standard_normal((cout, cout, 3, 3)) / 7
    bns = [(rng.uniform(0.5, 1.5, cout), rng.normal(0, 0.3, cout)) for _ in range(3)]
    ws = rng.standard_normal((cout, cin)) / 2 if proj else None
    lin = rng.standard_normal((B, H, W, cout))
    arrs = dict(x=x.transpose(0, 3, 1, 2), w1=w1, w2=w2, g1=bns[0][0], b1=bns[0][1], g2=bns[1][0], b2=bns[1][1])
    if proj:
        arrs.update(ws=ws.reshape(cout, cin, 1, 1), gs=bns[2][0], bs=bns[2][1])
    t = {k: torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, requires_grad=True) for k, v in arrs.items()}
    y1 = F.relu(F.batch_norm(F.conv2d(t["x"], t["w1"], padding=1), None, None, t["g1"], t["b1"], training=True, eps=EPS))
    main = F.batch_norm(F.conv2d(y1, t["w2"], padding=1), None, None, t["g2"], t["b2"], training=True, eps=EPS)
    short = F.batch_norm(F.conv2d(t["x"], t["ws"]), None, None, t["gs"], t["bs"], training=True, eps=EPS) if proj else t["x"]
    y = F.relu(main + short)
    (y * torch.tensor(lin.transpose(0, 3, 1, 2))).sum().backward()
    m = BM.block_backward(x, w1, bns[0], w2, bns[1], EPS, lin, ws, bns[2] if proj else None)
    assert float(np.abs(m["pre"]).min()) > 1e-6, "a pre-activation within 1e-6 of zero: choose another seed"
    pairs = [("y", m["y"], y.detach().numpy().transpose(0, 2, 3, 1)), ("dx", m["dx"], t["x"].grad.numpy().transpose(0, 2, 3, 1)),
             ("conv1_weight", m["conv1_weight"], t["w1"].grad.numpy()), ("conv2_weight", m["conv2_weight"], t["w2"].grad.numpy()),
             ("bn1_gamma", m["bn1_gamma"], t["g1"].grad.numpy()), ("bn1_beta", m["bn1_beta"], t["b1"].grad.numpy()),
             ("bn2_gamma", m["bn2_gamma"], t["g2"].grad.numpy()), ("bn2_beta", m["bn2_beta"], t["b2"].grad.numpy())]
    if proj:
        pairs += [("sc_weight", m["sc_weight"], t["ws"].grad.numpy().reshape(cout, cin)), ("sc_bn_gamma", m["sc_bn_gamma"], t["gs"].grad.numpy()),
                  ("sc_bn_beta", m["sc_bn_beta"], t["bs"].grad.numpy())]
    for name, got, want in pairs:
        rel = float(np.abs(got - want).max() / np.abs(want).max())
        print(name, "relative difference %.3g" % rel)
        assert rel < 1e-9, (name, rel)
    assert 0.3 < float((m["y"] == 0).mean()) < 0.7

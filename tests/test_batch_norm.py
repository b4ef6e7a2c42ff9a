"""Training-mode batch norm of a head-tower layer (csrc/k_norm.h: rd_bn_stats, rd_bn_fold, rd_affine_relu, rd_bn_relu_bwd;
rangedet_amd.backward.HeadTowerTrain and the single-step functions) against tests/norm_model.py, the float64 restatement of the formulas in
include/rangedet_hip.h with the bounds derived from the operation order.  Through the C ABI, in the style of test_conv_backward.py: every
output buffer and the workspace are pre-filled with 0xFF bytes and carry a guard tail; the tail and the channels outside [coff, coff + C)
must be unchanged afterwards; each step is compared with the model fed THE KERNEL'S OWN inputs to that step.

  statistics        |mean - exact|, |var - exact| within norm_model.stats_bound (normal inputs, a mean of 16 standard deviations -- where the
                    naive float32 E[z^2] - E[z]^2 is asserted to lie OUTSIDE the bound --, an outlier of 100 standard deviations at pixel 0);
                    a constant channel gives its value in every bit and var == 0; two calls give the same bytes
  fold              a, b, both moving statistics bit-equal to the float32 restatement (a and b through the launch's own rstd); rstd within
                    2 ulp: sqrtf is documented to 1 ulp on the device, the division adds half of one
  rd_affine_relu    bit-equal to h16_round(max(fmaf(z, a, b), 0))
  dgamma, dbeta     within convbwd_model.sum_bound on random inputs (about half the ReLU mask zero), bit-equal on integer inputs at every shape
                    and split
  dz                per element within norm_model's dz tolerance of the formula on the launch's own dgamma and dbeta; masked pixels still
                    carry -gamma rstd (c1 + zh c2)
"""
import numpy as np
import pytest

import conv_model as CM
import convbwd_model as M
import norm_model as N
from conftest import BOTH
from rangedet_amd import lib as R
from train_util import DTS, back, back_image, check_hob, check_wgrad, dev16, ff, from_bits, image, rnd, same_bits, to_bits, train_inputs, vals16

F32 = np.float32
EPS, MOM = 1e-5 + 1e-10, 0.9
# B 1-2, H 2-5, W in {9, 37, 70}, C in {64, 128}: 18 pixels (one workgroup whatever the split), 222 (4 with the library's split), 700 (11)
SHAPES = [(1, 2, 9, 64), (2, 3, 37, 128), (2, 5, 70, 64), (1, 4, 70, 128)]
SPLITS = (1, 2, 3, 7, 0)
STRIDED = dict(cs=136, co=8)


def f32bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def ulps(a, b):
    return np.abs(f32bits(a).astype(np.int64) - f32bits(b).astype(np.int64))


def fvec(be, buf, C, what):
    return back(be, buf, C * 4, what).view(F32).copy()


# ---- statistics --------------------------------------------------------------------------------------------------------------------------
def run_stats(be, dt, z, cs=None, co=0, split=0, twice=False):
    """-> mean, var (float32), the number of partial sums"""
    L = be.lib
    B, H, W, C = z.shape
    nws = L.raw("rd_bn_stats_workspace_bytes")(B, H, W, C, split)
    assert nws > 0 and nws % (12 * C) == 0
    P = nws // (12 * C)
    assert P == N.parts(B * H * W, split)
    zd = be.up(image(z, dt, cs, co))
    outs = []
    for _ in range(2 if twice else 1):
        mean, var, ws = ff(be, C * 4), ff(be, C * 4), ff(be, nws)
        L.call("rd_bn_stats", be.ptr(zd), cs or C, co, be.ptr(mean), be.ptr(var), B, H, W, C, split, dt, be.ptr(ws), nws, be.stream)
        back(be, ws, nws, "workspace")
        outs.append((fvec(be, mean, C, "mean"), fvec(be, var, C, "var")))
    if twice:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs)), "two calls differ"
    return outs[0][0], outs[0][1], P


def check_stats(mean, var, z, P, what):
    z2 = z.reshape(-1, z.shape[-1])
    m, v = N.stats(z2)
    bm, bv = N.stats_bound(z2, P)
    assert np.isfinite(mean).all() and np.isfinite(var).all() and (var >= 0).all(), what
    em, ev = np.abs(mean.astype(np.float64) - m), np.abs(var.astype(np.float64) - v)
    wm, wv = float((em[bm > 0] / bm[bm > 0]).max(initial=0)), float((ev[bv > 0] / bv[bv > 0]).max(initial=0))
    print(what, "P %d: mean err / bound %.3g, var err / bound %.3g" % (P, wm, wv))
    assert (em[bm == 0] == 0).all() and (ev[bv == 0] == 0).all() and wm <= 1 and wv <= 1, (what, wm, wv)
    return bv, v


_Z = {}


def zcase(kind, shape, dt, seed):
    """'normal': mean 0.3 s, deviation s per channel (s in 0.5 .. 2);  'cancel': mean 16 s;  'outlier': pixel 0 of frame 0 at mean + 100 s"""
    key = (kind, shape, dt, seed)
    if key not in _Z:
        rng = np.random.default_rng(seed)
        s = rng.uniform(0.5, 2.0, shape[3])
        v = (16.0 if kind == "cancel" else 0.3) * s + s * rng.standard_normal(shape)
        if kind == "outlier":
            v[0, 0, 0] = 0.3 * s + 100.0 * s
        v = from_bits(to_bits(v.astype(F32), dt), dt)
        v.setflags(write=False)
        _Z[key] = v
    return _Z[key]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_stats_normal_inputs_every_split(be, dt, shape):
    z = zcase("normal", shape, dt, 101)
    for split in SPLITS:
        mean, var, P = run_stats(be, dt, z, split=split)
        check_stats(mean, var, z, P, "stats %r split %d %s" % (shape, split, be.name))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_stats_channel_stride_and_offset(be, dt):
    z = zcase("normal", (2, 3, 37, 128), dt, 102)
    mean, var, P = run_stats(be, dt, z, split=3, **STRIDED)
    check_stats(mean, var, z, P, "stats strided %s" % be.name)


def test_cancellation_case_is_discriminating():
    """CPU only, before any launch: at a mean of 16 standard deviations the naive float32 E[z^2] - E[z]^2 misses the variance bound in most
    channels, for both types and for the splits the launch test uses"""
    for dt in (R.RD_BF16, R.RD_F16):
        z = zcase("cancel", (2, 5, 70, 128), dt, 103).reshape(-1, 128)
        m, v = N.stats(z)
        assert 12 < float((np.abs(m) / np.sqrt(v)).min()) and float((np.abs(m) / np.sqrt(v)).max()) < 20
        naive = np.abs(N.naive_var_f32(z).astype(np.float64) - v)
        assert (naive > 0).mean() > 0.9, "the float32 sums of this case are exact: it would show nothing"
        for split in (0, 1):
            outside = float((naive > N.stats_bound(z, N.parts(z.shape[0], split))[1]).mean())
            print("dtype %d split %d: naive variance outside the bound in %.0f %% of the channels" % (dt, split, 100 * outside))
            assert outside > 0.5, (dt, split, outside)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_stats_cancellation(be, dt):
    """mean = 16 standard deviations, B 2, 5 x 70, 128 channels: within the bound that the naive form misses"""
    z = zcase("cancel", (2, 5, 70, 128), dt, 103)
    for split in (0, 1):
        mean, var, P = run_stats(be, dt, z, split=split)
        bv, v = check_stats(mean, var, z, P, "stats cancel split %d %s" % (split, be.name))
        naive = np.abs(N.naive_var_f32(z.reshape(-1, 128)).astype(np.float64) - v)
        assert (naive > bv).mean() > 0.5


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_stats_outlier_at_pixel_zero(be, dt):
    z = zcase("outlier", (2, 5, 70, 64), dt, 104)
    m, v = N.stats(z.reshape(-1, 64)[1:])                            # mean and deviation of every other pixel
    assert float(((z[0, 0, 0] - m) / np.sqrt(v)).min()) > 90
    for split in (0, 1, 3):
        mean, var, P = run_stats(be, dt, z, split=split)
        check_stats(mean, var, z, P, "stats outlier split %d %s" % (split, be.name))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_stats_constant_channels_and_determinism(be, dt):
    """channel c holds the integer (c % 7) - 3 everywhere: the mean is that integer in every bit, the variance exactly zero; every third
    channel keeps random values; two calls give the same bytes"""
    for shape in ((2, 5, 70, 64), (2, 3, 37, 128)):
        z = zcase("normal", shape, dt, 105).copy()
        C = shape[3]
        const = np.arange(C) % 3 != 0
        ints = ((np.arange(C) % 7) - 3).astype(F32)
        z[..., const] = ints[const]
        for split in (0, 3):
            mean, var, P = run_stats(be, dt, z, split=split, twice=True)
            assert same_bits(mean[const], ints[const]) and (var[const] == 0).all(), (shape, split)
            check_stats(mean, var, z, P, "stats const %r split %d %s" % (shape, split, be.name))


# ---- fold ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unbiased", [0, 1])
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_fold_bits(be, unbiased):
    L = be.lib
    for C, n in ((128, 222), (64, 1359872), (24, 2)):
        rng = np.random.default_rng(200 + C)
        mean, var = rng.normal(0, 2, C).astype(F32), rng.uniform(0, 3, C).astype(F32)
        var[::5] = 0
        gamma, beta = rng.uniform(0.5, 1.5, C).astype(F32), rng.normal(0, 0.1, C).astype(F32)
        mm, mv = rng.normal(0, 1, C).astype(F32), rng.uniform(0.5, 2, C).astype(F32)
        ins = [be.up(v) for v in (mean, var, gamma, beta)]
        mmd, mvd = be.up(np.concatenate([mm, np.full(16, 7, F32)])), be.up(np.concatenate([mv, np.full(16, 7, F32)]))
        rstd, a, b = ff(be, C * 4), ff(be, C * 4), ff(be, C * 4)
        L.call("rd_bn_fold", *[be.ptr(v) for v in ins], EPS, MOM, n, unbiased, be.ptr(rstd), be.ptr(a), be.ptr(b), be.ptr(mmd), be.ptr(mvd), C, be.stream)
        rstd, a, b = fvec(be, rstd, C, "rstd"), fvec(be, a, C, "a"), fvec(be, b, C, "b")
        mm1, mv1 = be.down(mmd, F32, (C + 16,)), be.down(mvd, F32, (C + 16,))
        assert (mm1[C:] == 7).all() and (mv1[C:] == 7).all()
        want = N.fold_f32(mean, var, gamma, beta, EPS, MOM, n, unbiased, mm, mv)
        worst = int(ulps(rstd, want["rstd"]).max())
        print("fold C %d %s: 1 / sqrtf differs from the correctly rounded value by at most %d ulp" % (C, be.name, worst))
        assert worst <= (0 if be.name == "emu" else 2)
        a_own, b_own = N.fold_ab_f32(mean, rstd, gamma, beta)
        assert same_bits(a, a_own) and same_bits(b, b_own)
        assert same_bits(mm1[:C], want["moving_mean"]) and same_bits(mv1[:C], want["moving_var"])


# ---- rd_affine_relu --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_affine_relu_bits(be, dt):
    L = be.lib
    for (B, H, W, C), lay in [(s, {}) for s in SHAPES] + [((2, 3, 37, 128), STRIDED)]:
        z = zcase("normal", (B, H, W, C), dt, 301)
        rng = np.random.default_rng(302)
        a, b = rng.uniform(-1.5, 1.5, C).astype(F32), rng.normal(0, 0.5, C).astype(F32)
        cs, co = lay.get("cs", C), lay.get("co", 0)
        zd, ad, bd = be.up(image(z, dt, cs, co)), be.up(a), be.up(b)
        for relu in (1, 0):
            out = ff(be, B * H * W * (cs + 8) * 2)
            L.call("rd_affine_relu", be.ptr(zd), cs, co, be.ptr(ad), be.ptr(bd), relu, be.ptr(out), cs + 8, co + 8, B, H, W, C, dt, be.stream)
            got = back_image(be, out, (B, H, W, C), cs + 8, co + 8, dt, "y")
            want = to_bits(N.affine_relu_f32(z, a, b, dt, bool(relu)), dt)
            same = (got == want) | ((from_bits(got, dt) == 0) & (from_bits(want, dt) == 0))
            assert same.all(), ((B, H, W, C), relu, int((~same).sum()))
            if relu:
                assert 0.2 < (from_bits(got, dt) == 0).mean() < 0.8


# ---- backward ----------------------------------------------------------------------------------------------------------------------------
def run_bwd(be, dt, g, z, a, b, mean, rstd, gamma, relu=1, split=0, cs=None, co=0, twice=False):
    L = be.lib
    B, H, W, C = z.shape
    nws = L.raw("rd_bn_relu_bwd_workspace_bytes")(B, H, W, C, split)
    assert nws > 0 and nws // (8 * C) == N.parts(B * H * W, split)
    cs = cs or C
    gd, zd = be.up(image(g, dt, cs, co)), be.up(image(z, dt, cs + 8, co + 8))
    vecs = [be.up(np.ascontiguousarray(v, dtype=F32)) for v in (a, b, mean, rstd, gamma)]
    outs = []
    for _ in range(2 if twice else 1):
        dz, dg, db, ws = ff(be, B * H * W * (cs + 16) * 2), ff(be, C * 4), ff(be, C * 4), ff(be, nws)
        L.call("rd_bn_relu_bwd", be.ptr(gd), cs, co, be.ptr(zd), cs + 8, co + 8, *[be.ptr(v) for v in vecs], relu, be.ptr(dz), cs + 16, co + 16,
               be.ptr(dg), be.ptr(db), B, H, W, C, split, dt, be.ptr(ws), nws, be.stream)
        back(be, ws, nws, "workspace")
        outs.append((from_bits(back_image(be, dz, (B, H, W, C), cs + 16, co + 16, dt, "dz"), dt), fvec(be, dg, C, "dgamma"), fvec(be, db, C, "dbeta")))
    if twice:
        assert all(x.tobytes() == y.tobytes() for x, y in zip(*outs)), "two calls differ"
    return outs[0]


def check_bwd(got, g, z, a, b, mean, rstd, gamma, relu, dt, exact, what):
    """g, z: the values the launch read; -> the fraction of the mask that is zero"""
    dz, dgamma, dbeta = got
    C = z.shape[-1]
    g2, z2 = g.reshape(-1, C), z.reshape(-1, C)
    n = z2.shape[0]
    mask = N.mask_f32(z2, a, b) if relu else None
    m = N.bn_bwd(g2, z2, mask, mean, rstd)
    assert np.isfinite(dz).all() and np.isfinite(dgamma).all() and np.isfinite(dbeta).all(), what
    if exact:
        assert same_bits(dbeta, m["dbeta"]) and same_bits(dgamma, m["dgamma"]), what
    else:
        for name, got_, key in (("dbeta", dbeta, "dbeta"), ("dgamma", dgamma, "dgamma")):
            bound = M.sum_bound(n, m[key + "_abs"])
            err = np.abs(got_.astype(np.float64) - m[key])
            assert (err[bound == 0] == 0).all(), (what, name)
            worst = float((err[bound > 0] / bound[bound > 0]).max(initial=0))
            print(what, name, "worst err / bound %.3g" % worst)
            assert worst <= 1, (what, name, worst)
    v, scale = N.bn_dz(m, gamma, rstd, dgamma, dbeta, n)
    tol = CM.half_ulp_of(v, dt) + N.DZ_K * N.U * scale
    err = np.abs(dz.reshape(n, C).astype(np.float64) - v)
    assert (err[tol == 0] == 0).all(), what
    worst = float((err[tol > 0] / tol[tol > 0]).max(initial=0))
    print(what, "dz worst err / tol %.3g" % worst)
    assert worst <= 1, (what, worst)
    if mask is None:
        return 0.0
    off = ~mask
    if off.any() and not exact:          # a masked pixel still carries -gamma rstd (c1 + zh c2)
        assert (dz.reshape(n, C)[off] != 0).mean() > 0.5, what
    return float(off.mean())


def bwd_params(z, dt, seed):
    """mean, rstd of z itself (float32), gamma in 0.5 .. 1.5, beta small: about half of fmaf(z, a, b) is positive"""
    C = z.shape[-1]
    rng = np.random.default_rng(seed)
    m, v = N.stats(z.reshape(-1, C))
    mean, rstd = m.astype(F32), (1.0 / np.sqrt(v + EPS)).astype(F32)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(F32), rng.normal(0, 0.05, C).astype(F32)
    a, b = N.fold_ab_f32(mean, rstd, gamma, beta)
    return a, b, mean, rstd, gamma


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_bn_relu_bwd_random(be, dt, shape):
    z, g = zcase("normal", shape, dt, 401), rnd("normal", shape, dt, 402)
    a, b, mean, rstd, gamma = bwd_params(z, dt, 403)
    for split in (0, 3):
        got = run_bwd(be, dt, g, z, a, b, mean, rstd, gamma, split=split, twice=split == 0)
        zero = check_bwd(got, g, z, a, b, mean, rstd, gamma, 1, dt, False, "bwd %r split %d %s" % (shape, split, be.name))
        assert 0.35 < zero < 0.65, zero
    got = run_bwd(be, dt, g, z, None, None, mean, rstd, gamma, relu=0)
    check_bwd(got, g, z, a, b, mean, rstd, gamma, 0, dt, False, "bwd %r no relu %s" % (shape, be.name))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_bn_relu_bwd_channel_stride_and_offset(be, dt):
    shape = (2, 3, 37, 128)
    z, g = zcase("normal", shape, dt, 411), rnd("normal", shape, dt, 412)
    a, b, mean, rstd, gamma = bwd_params(z, dt, 413)
    got = run_bwd(be, dt, g, z, a, b, mean, rstd, gamma, split=2, **STRIDED)
    check_bwd(got, g, z, a, b, mean, rstd, gamma, 1, dt, False, "bwd strided %s" % be.name)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_bn_relu_bwd_exact_every_split(be, dt, shape):
    """g, z integers in -3 .. 3, mean 0, rstd 1, a 1, b 0 or -0.5: every partial sum is an integer below 2^24, dgamma and dbeta equal the
    model in every bit at every split -- one dropped or doubled pixel shows"""
    C = shape[3]
    g, z = rnd("ints", shape, dt, 421), rnd("ints", shape, dt, 422)
    one, zero = np.ones(C, F32), np.zeros(C, F32)
    gamma = np.random.default_rng(423).uniform(0.5, 1.5, C).astype(F32)
    for split in SPLITS:
        for bval in (0.0, -0.5):
            b = np.full(C, bval, F32)
            got = run_bwd(be, dt, g, z, one, b, zero, one, gamma, split=split)
            check_bwd(got, g, z, one, b, zero, one, gamma, 1, dt, True, "bwd exact %r split %d b %g %s" % (shape, split, bval, be.name))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_status_codes(be):
    """C 24, a zero extent, a workspace one byte short, null pointers, float32, misaligned tensors: each its code, nothing launched (one
    zeroed buffer stands for every device pointer and stays zero)"""
    L = be.lib
    buf = be.empty(1 << 20)
    p = be.ptr(buf)
    BF = R.RD_BF16
    ws_s, ws_b = L.raw("rd_bn_stats_workspace_bytes"), L.raw("rd_bn_relu_bwd_workspace_bytes")

    def stats(z=p, mean=p, var=p, ws=p, C=64, B=1, H=2, W=8, cs=None, co=0, split=0, dt=BF, nws=1 << 20):
        return L.raw("rd_bn_stats")(z, cs or C, co, mean, var, B, H, W, C, split, dt, ws, nws, be.stream)

    def fold(mean=p, rstd=p, C=64, n=16, unbiased=1):
        return L.raw("rd_bn_fold")(mean, p, p, p, EPS, MOM, n, unbiased, rstd, p, p, p, p, C, be.stream)

    def aff(z=p, a=p, y=p, C=64, B=1, co=0, dt=BF):
        return L.raw("rd_affine_relu")(z, C, co, a, p, 1, y, C, 0, B, 2, 8, C, dt, be.stream)

    def bwd(g=p, z=p, a=p, dz=p, dg=p, ws=p, C=64, B=1, co=0, split=0, dt=BF, relu=1, nws=1 << 20):
        return L.raw("rd_bn_relu_bwd")(g, C, co, z, C, 0, a, p, p, p, p, relu, dz, C, 0, dg, p, B, 2, 8, C, split, dt, ws, nws, be.stream)
    assert ws_s(1, 2, 8, 64, 0) == 3 * 64 * 4 and ws_s(2, 5, 70, 128, 0) == 11 * 3 * 128 * 4 and ws_s(2, 5, 70, 128, 7) == 7 * 3 * 128 * 4
    assert ws_s(8, 64, 2656, 128, 0) == 1024 * 3 * 128 * 4 and ws_s(1, 2, 8, 24, 0) == 0 and ws_s(0, 2, 8, 64, 0) == 0 and ws_s(1, 2, 8, 64, -1) == 0
    assert ws_b(1, 2, 8, 64, 0) == 2 * 64 * 4 and ws_b(2, 5, 70, 128, 3) == 3 * 2 * 128 * 4 and ws_b(1, 2, 8, 96, 0) == 0
    for kw in (dict(C=24), dict(C=96), dict(C=512), dict(B=0), dict(co=4, cs=72), dict(cs=60)):
        assert stats(**kw) == R.RD_ESHAPE, kw
        assert L.rd_last_error_string().decode().startswith("bn_stats")
    for kw in (dict(C=0), dict(n=0), dict(n=1)):
        assert fold(**kw) == R.RD_ESHAPE, kw
    for kw in (dict(C=24), dict(B=0), dict(co=8)):
        assert aff(**kw) == R.RD_ESHAPE and bwd(**kw) == R.RD_ESHAPE, kw
    for name in ("z", "mean", "var", "ws"):
        assert stats(**{name: None}) == R.RD_EINVAL and "null" in L.rd_last_error_string().decode(), name
    for name in ("mean", "rstd"):
        assert fold(**{name: None}) == R.RD_EINVAL, name
    for name in ("z", "a", "y"):
        assert aff(**{name: None}) == R.RD_EINVAL, name
    for name in ("g", "z", "a", "dz", "dg", "ws"):
        assert bwd(**{name: None}) == R.RD_EINVAL, name
    assert stats(dt=R.RD_F32) == R.RD_EINVAL and aff(dt=R.RD_F32) == R.RD_EINVAL and bwd(dt=R.RD_F32) == R.RD_EINVAL
    assert stats(split=-1) == R.RD_EINVAL and bwd(split=-1) == R.RD_EINVAL
    assert stats(nws=ws_s(1, 2, 8, 64, 0) - 1) == R.RD_EWORKSPACE and "workspace" in L.rd_last_error_string().decode()
    assert bwd(nws=ws_b(1, 2, 8, 64, 0) - 1) == R.RD_EWORKSPACE and "workspace" in L.rd_last_error_string().decode()
    for rc in (stats(z=p + 8), aff(z=p + 8), bwd(g=p + 8)):
        assert rc == R.RD_EINVAL and "aligned" in L.rd_last_error_string().decode()
    assert not be.down(buf, np.uint8, (1 << 20,)).any()           # nothing ran


# ---- the formulas --------------------------------------------------------------------------------------------------------------------------
def test_model_backward_matches_autograd():
    """CPU only: norm_model.layer_backward (conv3x3 + batch norm with batch statistics + ReLU) against torch float64 autograd with a 1x1 conv
    and a linear loss on top, to 1e-9 of the largest value of each gradient.  This establishes the formulas the launches are held to."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(501)
    B, H, W, cin, cout, nout = 2, 4, 5, 6, 7, 3
    x, w = rng.standard_normal((B, H, W, cin)), rng.standard_normal((cout, cin, 3, 3)) / 7
    gamma, beta = rng.uniform(0.5, 1.5, cout), rng.normal(0, 0.3, cout)
    ow, lin = rng.standard_normal((nout, cout)), rng.standard_normal((B, H, W, nout))
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in dict(x=x.transpose(0, 3, 1, 2), w=w, gamma=gamma, beta=beta).items()}
    z = F.conv2d(t["x"], t["w"], padding=1)
    y = F.relu(F.batch_norm(z, None, None, t["gamma"], t["beta"], training=True, eps=EPS))
    y.retain_grad()
    out = F.conv2d(y, torch.tensor(ow.reshape(nout, cout, 1, 1)))
    (out * torch.tensor(lin.transpose(0, 3, 1, 2))).sum().backward()
    m = N.layer_backward(x, w, gamma, beta, EPS, lin @ ow)
    for name, got, want in (("y", m["y"], y.detach().numpy().transpose(0, 2, 3, 1)), ("dgamma", m["dgamma"], t["gamma"].grad.numpy()),
                            ("dbeta", m["dbeta"], t["beta"].grad.numpy()), ("dW", m["dW"], t["w"].grad.numpy()),
                            ("dx", m["dx"], t["x"].grad.numpy().transpose(0, 2, 3, 1))):
        rel = float(np.abs(got - want).max() / np.abs(want).max())
        print(name, "relative difference %.3g" % rel)
        assert rel < 1e-9, (name, rel)
    assert 0.3 < float((m["y"] == 0).mean()) < 0.7


# ---- HeadTowerTrain ----------------------------------------------------------------------------------------------------------------------
def dvec(A, buf, C):
    return np.array(A.to_numpy(A.view_f32(buf, (C,)))).astype(F32)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_head_tower_train(be, dt):
    """B 1, 4 x 37: a cls tower (nout 1) and a reg tower (nout 8) of two 128 -> 128 layers; d_logit / d_delta from a real RpnLoss call on the
    towers' own outputs; every step checked on the kernels' own inputs; the moving statistics after one and after two forwards"""
    from rangedet_amd.backward import HeadTowerTrain
    from rangedet_amd.loss import RpnLoss
    A, L = be.alloc, be.lib
    B, H, W, C = 1, 4, 37, 128
    n, P = B * H * W, N.parts(B * H * W, 0)
    rng = np.random.default_rng(601)
    x = dev16(be, to_bits(rnd("relu", (B, H, W, C), dt, 602), dt), dt)
    towers, outs = {}, {}
    for kind, nout in (("cls", 1), ("reg", 8)):
        ws = [(rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C / 2)).astype(F32) for _ in range(2)]
        gs = [rng.uniform(0.5, 1.5, C).astype(F32) for _ in range(2)]
        bs = [(0.1 * rng.standard_normal(C)).astype(F32) for _ in range(2)]
        mms, mvs = [rng.normal(0, 1, C).astype(F32) for _ in range(2)], [rng.uniform(0.5, 2, C).astype(F32) for _ in range(2)]
        ow, ob = (rng.standard_normal((nout, C, 1, 1)) / np.sqrt(C)).astype(F32), (0.1 * rng.standard_normal(nout)).astype(F32)
        t = HeadTowerTrain(ws, gs, bs, mms, mvs, ow, ob, kind=kind, level=1, first_conv=2, dtype=dt, lib=L, alloc=A)
        stem = "rpn_%s_conv_%%d_lvl_1" % kind
        t.forward(x)
        A.sync()
        st1 = [(dvec(A, s["mean"], C), dvec(A, s["var"], C)) for s in t.saved]
        aux1 = {k: np.array(A.to_numpy(v)).copy() for k, v in t.aux().items()}
        assert sorted(aux1) == sorted([stem % i + s for i in (2, 3) for s in ("_bn_moving_mean", "_bn_moving_var")])
        outs[kind] = t.forward(x)
        A.sync()
        aux2 = {k: np.array(A.to_numpy(v)).copy() for k, v in t.aux().items()}
        for i in range(2):
            mean, var = st1[i]
            assert dvec(A, t.saved[i]["mean"], C).tobytes() == mean.tobytes() and dvec(A, t.saved[i]["var"], C).tobytes() == var.tobytes()
            f1 = N.fold_f32(mean, var, gs[i], bs[i], EPS, MOM, n, True, mms[i], mvs[i])
            f2 = N.fold_f32(mean, var, gs[i], bs[i], EPS, MOM, n, True, f1["moving_mean"], f1["moving_var"])
            name = stem % (2 + i)
            assert same_bits(aux1[name + "_bn_moving_mean"], f1["moving_mean"]) and same_bits(aux1[name + "_bn_moving_var"], f1["moving_var"])
            assert same_bits(aux2[name + "_bn_moving_mean"], f2["moving_mean"]) and same_bits(aux2[name + "_bn_moving_var"], f2["moving_var"])
        towers[kind] = (t, ws, gs, bs, ow)
    assert tuple(outs["cls"].shape) == (B, H * W, 1) and tuple(outs["reg"].shape) == (B, H * W, 8)
    loss = RpnLoss(strides=(1,), lib=L, alloc=A)(outs["cls"].reshape(B, H * W), outs["reg"], train_inputs(B, H, W))
    A.sync()
    for kind, dname in (("cls", "d_logit"), ("reg", "d_delta")):
        t, ws, gs, bs, ow = towers[kind]
        nout = ow.shape[0]
        dx, grads = t.backward(loss[dname], n_off=0)
        A.sync()
        d = np.array(A.to_numpy(loss[dname])).reshape(B, H * W, nout)
        assert np.isfinite(d).all() and (d != 0).mean() > 0.2, kind
        stem, oname = "rpn_%s_conv_%%d_lvl_1" % kind, "rpn_cls_logit_lvl_1" if kind == "cls" else "rpn_reg_delta_lvl_1"
        assert sorted(grads) == sorted([stem % i + s for i in (2, 3) for s in ("_weight", "_bn_gamma", "_bn_beta")] + [oname + "_weight", oname + "_bias"])
        gr = {k: np.array(A.to_numpy(v)) for k, v in grads.items()}
        assert gr[oname + "_weight"].shape == (nout, C, 1, 1) and gr[oname + "_bias"].shape == (nout,) and gr[stem % 2 + "_weight"].shape == (C, C, 3, 3)
        assert gr[stem % 3 + "_bn_gamma"].shape == (C,) and gr[stem % 3 + "_bn_beta"].shape == (C,)
        acts, zs = [vals16(be, v, dt) for v in t.acts], [vals16(be, v, dt) for v in t.zs]
        gsv, dzs, dxs = ([vals16(be, v, dt) for v in lst] for lst in (t.gs, t.dzs, t.dxs))
        what = "train tower %s %s" % (kind, be.name)
        # the output conv: its dx is dL/dy of the last layer, no mask and no scale
        check_hob((gsv[1], gr[oname + "_weight"].reshape(nout, C), gr[oname + "_bias"]), d, acts[2], ow.reshape(nout, C), dt, None, False, False, what)
        for i in (1, 0):
            s = t.saved[i]
            mean, var, rstd, a, b = (dvec(A, s[k], C) for k in ("mean", "var", "rstd", "a", "b"))
            ref = CM.conv_ref64(acts[i].transpose(0, 3, 1, 2), ws[i], dt, fold=True).transpose(0, 2, 3, 1)
            over, worst = CM.conv_check(zs[i], ref, dt)
            print("%s z %d: over tolerance %d, worst err / tol %.3g" % (what, i, over, worst))
            assert over == 0, (what, i, over, worst)
            check_stats(mean, var, zs[i], P, "%s stats %d" % (what, i))
            assert int(ulps(rstd, N.fold_f32(mean, var, gs[i], bs[i], EPS, MOM, n, True, mean, var)["rstd"]).max()) <= (0 if be.name == "emu" else 2)
            a_own, b_own = N.fold_ab_f32(mean, rstd, gs[i], bs[i])
            assert same_bits(a, a_own) and same_bits(b, b_own)
            want = to_bits(N.affine_relu_f32(zs[i], a, b, dt), dt)
            got = to_bits(acts[i + 1], dt)
            assert ((got == want) | ((acts[i + 1] == 0) & (from_bits(want, dt) == 0))).all(), (what, i)
            assert 0.2 < (acts[i + 1] == 0).mean() < 0.8
            stemi = stem % (2 + i)
            check_bwd((dzs[i], gr[stemi + "_bn_gamma"], gr[stemi + "_bn_beta"]), gsv[i], zs[i], a, b, mean, rstd, gs[i], 1, dt, False, "%s bn %d" % (what, i))
            check_wgrad(gr[stemi + "_weight"], acts[i], dzs[i], False, "%s dW %d" % (what, i))
            ref = CM.conv_ref64(dzs[i].transpose(0, 3, 1, 2), M.flip_weight(ws[i]), dt, fold=True).transpose(0, 2, 3, 1)
            over, worst = CM.conv_check(dxs[i], ref, dt)
            print("%s dx %d: over tolerance %d, worst err / tol %.3g" % (what, i, over, worst))
            assert over == 0, (what, i, over, worst)
            if i > 0:
                assert gsv[i - 1].tobytes() == dxs[i].tobytes()
        assert vals16(be, dx, dt).tobytes() == dxs[0].tobytes()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_single_step_functions(be, dt):
    """batch_norm_stats, batch_norm_relu_forward and batch_norm_relu_backward (B 2, 3 x 37, 64 channels) against the model"""
    from rangedet_amd import backward as BK
    A, L = be.alloc, be.lib
    shape = (2, 3, 37, 64)
    C, n = 64, 222
    zv, gv = zcase("normal", shape, dt, 701), rnd("normal", shape, dt, 702)
    z, g = dev16(be, to_bits(zv, dt), dt), dev16(be, to_bits(gv, dt), dt)
    rng = np.random.default_rng(703)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(F32), rng.normal(0, 0.05, C).astype(F32)
    mm, mv = np.zeros(C, F32), np.ones(C, F32)
    mean, var = BK.batch_norm_stats(z, dtype=dt, lib=L, alloc=A)
    A.sync()
    mean, var = np.array(A.to_numpy(mean)).copy(), np.array(A.to_numpy(var)).copy()
    check_stats(mean, var, zv, N.parts(n, 0), "single-step stats %s" % be.name)
    y, saved = BK.batch_norm_relu_forward(z, gamma, beta, mm, mv, dtype=dt, lib=L, alloc=A)
    dz, dgamma, dbeta = BK.batch_norm_relu_backward(g, z, saved, gamma, dtype=dt, lib=L, alloc=A)
    A.sync()
    a, b, rstd = (dvec(A, saved[k], C) for k in ("a", "b", "rstd"))
    assert dvec(A, saved["mean"], C).tobytes() == mean.tobytes()
    f = N.fold_f32(mean, var, gamma, beta, EPS, MOM, n, True, mm, mv)
    assert same_bits(np.array(A.to_numpy(saved["moving_mean"])), f["moving_mean"]) and same_bits(np.array(A.to_numpy(saved["moving_var"])), f["moving_var"])
    want = N.affine_relu_f32(zv, a, b, dt)
    assert (vals16(be, y, dt) == want).all()
    check_bwd((vals16(be, dz, dt), np.array(A.to_numpy(dgamma)), np.array(A.to_numpy(dbeta))), gv, zv, a, b, mean, rstd, gamma, 1, dt, False,
              "single-step bwd %s" % be.name)


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_head_tower_train_refusals(be):
    from rangedet_amd.backward import HeadTowerTrain
    A, L = be.alloc, be.lib
    one, zero = [np.ones(128, F32)], [np.zeros(128, F32)]
    ow, ob = np.zeros((1, 128), F32), np.zeros(1, F32)

    def make(w, out_w=ow, out_b=ob, **kw):
        return HeadTowerTrain([w], one, zero, zero, one, out_w, out_b, lib=L, alloc=A, **kw)
    with pytest.raises(NotImplementedError, match="concat"):        # the level-0 conv_0: 64 + 8 input channels
        make(np.zeros((128, 72, 3, 3), F32), level=0)
    with pytest.raises(NotImplementedError, match="3x3"):
        make(np.zeros((128, 128, 1, 1), F32))
    with pytest.raises(NotImplementedError, match="16-bit"):
        make(np.zeros((128, 128, 3, 3), F32), dtype=R.RD_F32)
    with pytest.raises(NotImplementedError, match="outputs"):
        make(np.zeros((128, 128, 3, 3), F32), out_w=np.zeros((7, 128), F32), out_b=np.zeros(7, F32))
    t = make(np.zeros((128, 128, 3, 3), F32))
    with pytest.raises(RuntimeError, match="forward"):
        t.backward(np.zeros((1, 8), F32))

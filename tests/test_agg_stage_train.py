"""An aggregation stage in training mode (csrc/k_convbwd.h: rd_deconv_bwd_weight; csrc/k_norm.h: rd_affine_relu_add; csrc/k_optim.h:
rd_pack_deconv_dev; rangedet_amd.backward.TowerOps: the transposed-conv steps; rangedet_amd.backbone_train.AggStageTrain) against
tests/agg_model.py, the restatement of the formulas in include/rangedet_hip.h.  Through the C ABI, in the style of test_down_block_train.py:
every output buffer and the workspace are pre-filled with 0xFF bytes and carry a guard tail; the tail and the channels outside
[coff, coff + C) must be unchanged afterwards; each step is compared with the model fed THE KERNEL'S OWN inputs to it.  The input of the
transposed conv is (B, H, Win, Cin -> Cout); the shapes:

  (3,4) s2 p1   (1, 2, 1, 64 -> 64)       the tap columns kw 0 and 3 lie wholly outside the image
                (2, 3, 9, 128 -> 64)      a small general case
                (2, 5, 70, 64 -> 64)      a full 64-pixel tile and one of 6 pixels; at wi 69, kw 3 reads column 140, outside, kw 2 the last one
                (1, 17, 37, 128 -> 64)    H crosses the 16-row strip
  (3,8) s4 p2   (1, 2, 1, 128 -> 128)     kw 0, 1, 6, 7 wholly outside
                (2, 3, 5, 128 -> 64)      a small general case
                (2, 5, 70, 128 -> 64)     a full 64-pixel tile and one of 6 pixels; Wout = 280
                (1, 17, 37, 128 -> 128)   H crosses the 16-row strip

  rd_deconv_bwd_weight     a float64 einsum within convbwd_model.sum_bound at every shape and split; exact inputs equal in every bit at every
                           split; the workspace is partials x 3 KW x Cin x Cout x 4 bytes with the model's partial count; two calls give the
                           same bytes; channel strides and offsets; 3 KW distinct integer tap patterns come back each in its own (kh, kw) slot;
                           rd_conv3x3_bwd_weight_ex at stride 1 and 2 still equals its model in every bit
  the data gradient        the host image is rd_pack_conv3x3_ex_host of the restated view weight; the float64 scatter on the packer-rounded
                           weight within conv_model.conv_tol; impulses at wo = 0, Wout - 1 and inside: the footprint's columns; a residual: one
                           float32 add, one rounding (exact on integers)
  rd_affine_relu_add       bit-equal to the float32 restatement: negative pre-activations with a non-zero skip, -0 results, y aliasing z,
                           channel strides and offsets
  rd_pack_deconv_dev       both images equal the host packers byte for byte, both forms, both types, zero tails included
  AggStageTrain            every kept intermediate step by step on the stage's own previous tensors; d_skip is the res stage's input gradient
                           (g itself without a res stage); add_to_up; after SGD.step() the masters equal optim_model's step, both deconv
                           images the host packers on the downloaded master, and the next forward differs; from_params; the refusals
  the model itself         agg_model.stage_backward against torch.autograd in float64, to a relative 1e-9
"""
import numpy as np
import pytest

import agg_model as AM
import conv_model as CM
import convbwd_model as M
import down_block_model as DM
import norm_model as N
import optim_model as OM
import test_basic_block_train as TB
import test_down_block_train as TD
from conftest import BOTH
from rangedet_amd import lib as R
from train_util import DTS, back, back_image, check_wgrad, dev16, ff, from_bits, image, rnd, same_bits, to_bits, vals16

F32 = np.float32
EPS, MOM = TB.EPS, TB.MOM
S2, S4 = (4, 2, 1), (8, 4, 2)                      # (KW, s, p)
# (form, B, H, Win, Cin, Cout)
SHAPES = [(S2, 1, 2, 1, 64, 64), (S2, 2, 3, 9, 128, 64), (S2, 2, 5, 70, 64, 64), (S2, 1, 17, 37, 128, 64),
          (S4, 1, 2, 1, 128, 128), (S4, 2, 3, 5, 128, 64), (S4, 2, 5, 70, 128, 64), (S4, 1, 17, 37, 128, 128)]
SPLITS = (1, 2, 3, 7, 0)
IDS = dict(ids=lambda c: "k%ds%d-%s-%dto%d" % (c[0][0], c[0][1], "x".join(str(v) for v in c[1:4]), c[4], c[5]))
within, close = TB.within, TD.close


def shapes_of(case):
    (KW, s, p), B, H, Win, cin, cout = case
    return (B, H, Win, cin), (B, H, s * Win, cout)


# ---- rd_deconv_bwd_weight ------------------------------------------------------------------------------------------------------------------------
def run_dwgrad(be, dt, x, dz, form, split=0, xcs=None, xco=0, zcs=None, zco=0, twice=False):
    """-> dW (Cin, Cout, 3, KW), the partial count the workspace size implies, the workspace size"""
    L = be.lib
    KW, s, p = form
    B, H, Win, cin = x.shape
    cout = dz.shape[3]
    nws = L.raw("rd_deconv_bwd_weight_workspace_bytes")(B, H, Win, cin, cout, KW, s, p, split)
    per = 3 * KW * cin * cout * 4
    assert nws > 0 and nws % per == 0
    xd, zd = be.up(image(x, dt, xcs, xco)), be.up(image(dz, dt, zcs, zco))
    outs = []
    for _ in range(2 if twice else 1):
        dW, ws = ff(be, per), ff(be, nws)
        L.call("rd_deconv_bwd_weight", be.ptr(xd), xcs or cin, xco, be.ptr(zd), zcs or cout, zco, be.ptr(dW), B, H, Win, cin, cout, KW, s, p, split,
               dt, be.ptr(ws), nws, be.stream)
        back(be, ws, nws, "workspace")
        outs.append(back(be, dW, per, "dW"))
    if twice:
        assert outs[0].tobytes() == outs[1].tobytes(), "two calls differ"
    return outs[0].view(F32).reshape(cin, cout, 3, KW).copy(), nws // per, nws


def check_dwgrad(got, x, dz, form, exact, what):
    want, sabs, n = AM.weight_grad(x, dz, *form, want_abs=not exact)
    assert np.isfinite(got).all(), what
    if exact:
        bad = int((got != want.astype(F32)).sum())
        print(what, "exact: elements that differ", bad)
        assert same_bits(got, want), (what, bad)
    else:
        within(got, want, M.sum_bound(n[None, None], sabs), what)


@pytest.mark.parametrize("case", SHAPES, **IDS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_deconv_weight_grad_every_split(be, dt, case):
    """ReLU-sparse x against normal dz within sum_bound, and integer inputs equal in every bit, at every split; the workspace is the model's
    partial count; two calls agree"""
    form, (B, H, Win, cin, cout) = case[0], case[1:]
    xs, zs = shapes_of(case)
    xr, zr = rnd("relu", xs, dt, 3101), rnd("normal", zs, dt, 3102)
    xi, zi = rnd("ints", xs, dt, 3103), rnd("ints", zs, dt, 3104)
    for split in SPLITS:
        what = "deconv wgrad %r split %d %s" % (case, split, be.name)
        got, S, nws = run_dwgrad(be, dt, xr, zr, form, split=split, twice=split == 0)
        assert S == AM.parts(B, H, Win, cin, form[0], split) and nws == S * 3 * form[0] * cin * cout * 4, (what, S)
        check_dwgrad(got, xr, zr, form, False, what + " random")
        got, _, _ = run_dwgrad(be, dt, xi, zi, form, split=split)
        check_dwgrad(got, xi, zi, form, True, what)


@pytest.mark.parametrize("form", [S2, S4], ids=["k4s2", "k8s4"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_deconv_weight_grad_channel_stride_and_offset(be, dt, form):
    """x: 128 channels at offset 8 of 136; dz: 64 channels at offset 16 of 88"""
    KW, s, p = form
    xs, zs = (2, 3, 9, 128), (2, 3, 9 * s, 64)
    for kind, exact in (("relu", False), ("ints", True)):
        x, dz = rnd(kind, xs, dt, 3111), rnd("normal" if kind == "relu" else "ints", zs, dt, 3112)
        got, _, _ = run_dwgrad(be, dt, x, dz, form, split=2, xcs=136, xco=8, zcs=88, zco=16)
        check_dwgrad(got, x, dz, form, exact, "deconv wgrad strided %r %s %s" % (form, kind, be.name))


@pytest.mark.parametrize("form", [S2, S4], ids=["k4s2", "k8s4"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_deconv_weight_grad_tap_probe(be, dt, form):
    """x is a single 1 at one pixel (channel 3), dz holds KW kh + kw + 1 (channel 7) at the output pixel (h0 - 1 + kh, s wi - p + kw) that
    tap (kh, kw) pairs with it: all 3 KW taps fit in one launch, so dW[3, 7, kh, kw] = KW kh + kw + 1 and every other element is zero.  A
    mirrored or shifted tap column shows as a permutation."""
    KW, s, p = form
    B, H, Win, cin, cout = 1, 5, 6, 128, 64
    h0, wi = 2, 3
    x, dz = np.zeros((B, H, Win, cin), F32), np.zeros((B, H, s * Win, cout), F32)
    x[0, h0, wi, 3] = 1
    expect = np.zeros((cin, cout, 3, KW), F32)
    for kh in range(3):
        for kw in range(KW):
            dz[0, h0 - 1 + kh, s * wi - p + kw, 7] = expect[3, 7, kh, kw] = KW * kh + kw + 1
    got, _, _ = run_dwgrad(be, dt, x, dz, form)
    assert same_bits(got, expect), got[3, 7]
    assert same_bits(got, AM.weight_grad(x, dz, *form, want_abs=False)[0])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_conv_weight_grad_ex_unchanged(be, dt):
    """rd_conv3x3_bwd_weight_ex at one stride-1 and one stride-2 shape through test_down_block_train.run_wgrad: the same model, the same
    partial counts, integer inputs equal in every bit"""
    shape, cout = (2, 3, 37, 64), 128
    xi, zi = rnd("ints", shape, dt, 3121), rnd("ints", shape[:3] + (cout,), dt, 3122)
    xr, zr = rnd("relu", shape, dt, 3123), rnd("normal", shape[:3] + (cout,), dt, 3124)
    for split in (0, 3):
        got, S, nws = TD.run_wgrad(be, dt, xi, zi, stride_w=1, split=split, twice=True)
        assert S == DM.parts3x3(2, 3, 37, cout, split) and nws == S * 9 * 64 * cout * 4
        check_wgrad(got, xi, zi, True, "stride 1 %s" % be.name)
        check_wgrad(TD.run_wgrad(be, dt, xr, zr, stride_w=1, split=split)[0], xr, zr, False, "stride 1 random %s" % be.name)
    shape = (2, 5, 140, 64)
    xi, zi = rnd("ints", shape, dt, 3125), rnd("ints", (2, 5, 70, 64), dt, 3126)
    xr, zr = rnd("relu", shape, dt, 3127), rnd("normal", (2, 5, 70, 64), dt, 3128)
    for split in (0, 3):
        got, S, nws = TD.run_wgrad(be, dt, xi, zi, stride_w=2, split=split, twice=True)
        assert S == DM.parts3x3(2, 5, 70, 64, split) and nws == S * 9 * 64 * 64 * 4
        TD.check_wgrad_s2(got, xi, zi, True, "stride 2 %s" % be.name)
        TD.check_wgrad_s2(TD.run_wgrad(be, dt, xr, zr, stride_w=2, split=split)[0], xr, zr, False, "stride 2 random %s" % be.name)


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_deconv_weight_grad_status_codes(be):
    """another form, another channel pair, a workspace one byte short, null pointers, a bad type: each its code, nothing launched"""
    L = be.lib
    n = 1 << 20
    buf = be.up(np.full(n, 0xFF, np.uint8))
    p = be.ptr(buf)
    ws_w = L.raw("rd_deconv_bwd_weight_workspace_bytes")

    def wg(x=p, dz=p, dW=p, ws=p, cin=64, cout=64, B=1, H=2, Win=4, form=S2, xcs=None, xco=0, split=0, dt=R.RD_BF16, nws=n):
        return L.raw("rd_deconv_bwd_weight")(x, xcs or cin, xco, dz, cout, 0, dW, B, H, Win, cin, cout, *form, split, dt, ws, nws, be.stream)

    def msg():
        return L.rd_last_error_string().decode()
    assert ws_w(1, 2, 4, 64, 64, 4, 2, 1, 0) == 12 * 64 * 64 * 4 and ws_w(1, 2, 4, 128, 128, 8, 4, 2, 0) == 24 * 128 * 128 * 4
    assert ws_w(8, 64, 664, 128, 64, 8, 4, 2, 0) == 32 * 24 * 128 * 64 * 4 and ws_w(8, 64, 1328, 64, 64, 4, 2, 1, 0) == 128 * 12 * 64 * 64 * 4
    assert ws_w(1, 2, 4, 64, 64, 4, 2, 2, 0) == 0 and ws_w(1, 2, 4, 64, 128, 4, 2, 1, 0) == 0 and ws_w(1, 2, 4, 64, 64, 8, 4, 2, 0) == 0
    assert ws_w(1, 2, 4, 64, 64, 4, 2, 1, -1) == 0 and ws_w(0, 2, 4, 64, 64, 4, 2, 1, 0) == 0
    for kw in (dict(form=(4, 2, 2)), dict(form=(3, 1, 1)), dict(form=(8, 2, 3)), dict(cout=128), dict(cin=64, form=S4), dict(cin=96), dict(B=0),
               dict(H=0), dict(Win=0), dict(xco=4, xcs=72), dict(xcs=60)):
        assert wg(**kw) == R.RD_ESHAPE and msg().startswith("deconv_bwd_weight"), (kw, msg())
    for name in ("x", "dz", "dW", "ws"):
        assert wg(**{name: None}) == R.RD_EINVAL and msg().startswith("deconv_bwd_weight") and "null" in msg(), name
    assert wg(dt=R.RD_F32) == R.RD_EINVAL and wg(split=-1) == R.RD_EINVAL and msg().startswith("deconv_bwd_weight")
    assert wg(nws=ws_w(1, 2, 4, 64, 64, 4, 2, 1, 0) - 1) == R.RD_EWORKSPACE and "workspace" in msg()
    assert wg(x=p + 8) == R.RD_EINVAL and "aligned" in msg()
    assert (be.down(buf, np.uint8, (n,)) == 0xFF).all()           # nothing ran


# ---- the data gradient ---------------------------------------------------------------------------------------------------------------------------
def dweight(cin, cout, KW, seed):
    return (np.random.default_rng(seed).standard_normal((cin, cout, 3, KW)) / np.sqrt(3 * KW * cout / 4)).astype(F32)


@pytest.mark.parametrize("cin,cout,form", [(64, 64, S2), (128, 64, S2), (128, 64, S4), (128, 128, S4)], ids=["64to64k4", "128to64k4", "128to64k8", "128to128k8"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_deconv_images_host_and_device(be, dt, cin, cout, form):
    """the host data-gradient image is rd_pack_conv3x3_ex_host of the restated view weight, byte for byte; rd_pack_deconv_dev writes that
    image and the s forward phase images of rd_pack_deconv_weight_folded_host, zero tails included, into 0xFF-prefilled buffers (the first
    weight on exact rounding ties)"""
    L = be.lib
    KW, s, p = form
    rng = np.random.default_rng(3201 + cin + cout + KW)
    for w in (OM.tie_values((cin, cout, 3, KW), dt, rng, dt == R.RD_BF16), dweight(cin, cout, KW, 3202)):
        host = L.pack_deconv_data_grad(w, s, p, dt)
        want = L.pack_conv3x3_ex(AM.view_weight(w, s, p), 1, s * cout, fold_scale=None, dtype=dt)
        assert host.size == 18 * s * cin * cout + 256 and host.tobytes() == want.tobytes() and host.any() and not host[-256:].any()
        wd = TB.fup(be, w)
        out = ff(be, host.size)
        L.call("rd_pack_deconv_dev", be.ptr(wd), cin, cout, KW, s, p, 1, 0, dt, be.ptr(out), be.stream)
        got = back(be, out, host.size, "data-gradient image")
        assert int((got != host).sum()) == 0
        phases = [L.pack_deconv_weight(w, s, p, q, dt) for q in range(s)]
        nb = phases[0].size
        assert nb == L.cdll.rd_conv_packed_bytes(6, cin, cout, dt) == 12 * cin * cout + 256
        for stride in (nb, nb + 64):                   # packed back to back, and with a gap the launch must leave alone
            out = ff(be, stride * s)
            L.call("rd_pack_deconv_dev", be.ptr(wd), cin, cout, KW, s, p, 0, stride, dt, be.ptr(out), be.stream)
            got = back(be, out, stride * s, "phase images").reshape(s, stride)
            for q in range(s):
                assert int((got[q, :nb] != phases[q]).sum()) == 0 and not got[q, nb - 256:nb].any() and phases[q].any(), (q, stride)
                assert (got[q, nb:] == 0xFF).all()
        assert back(be, wd, w.nbytes, "master").tobytes() == w.tobytes()
    bad = L.raw("rd_pack_deconv_dev")
    assert bad(be.ptr(wd), cin, cout, KW, s, p, 0, nb - 16, dt, be.ptr(out), be.stream) == R.RD_EINVAL
    assert bad(be.ptr(wd), cin, 2 * cout + 64, KW, s, p, 1, 0, dt, be.ptr(out), be.stream) == R.RD_ESHAPE
    assert bad(be.ptr(wd), cin, cout, KW, s, p + 1, 1, 0, dt, be.ptr(out), be.stream) == R.RD_ESHAPE
    assert bad(None, cin, cout, KW, s, p, 1, 0, dt, be.ptr(out), be.stream) == R.RD_EINVAL


def ops_of(be, dt):
    from rangedet_amd.backward import TowerOps
    return TowerOps(dt, be.lib, be.alloc)


@pytest.mark.parametrize("case", SHAPES, **IDS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_deconv_data_grad(be, dt, case):
    """the gradient of the transposed conv's input against the float64 scatter on the rounded weight, alone and with a residual added in the
    epilogue; the same sum as the stride-1 conv of the view the launch is"""
    (KW, s, p), B, H, Win, cin, cout = case
    xs, zs = shapes_of(case)
    o = ops_of(be, dt)
    w = dweight(cin, cout, KW, 3301)
    dzv, rv = rnd("normal", zs, dt, 3302), rnd("normal", xs, dt, 3303)
    packed = o.pack_deconv_data_grad(w, s, p)
    dz, res = dev16(be, to_bits(dzv, dt), dt), dev16(be, to_bits(rv, dt), dt)
    ref = AM.data_grad(dzv, CM.h16_round(w, dt), s, p)
    for r, rval in ((None, 0.0), (res, rv)):
        got = vals16(be, o.deconv_data_grad(dz, packed, residual=r), dt)
        assert got.shape == xs
        over, worst = CM.conv_check(got, ref + rval, dt)
        print("deconv_data_grad %r %s residual %s: over %d, worst err / tol %.3g" % (case, be.name, r is not None, over, worst))
        assert over == 0, (case, over, worst)
    alt = CM.conv_ref64(dzv.reshape(B, H, Win, s * cout).transpose(0, 3, 1, 2), AM.view_weight(w, s, p), dt, fold=True).transpose(0, 2, 3, 1)
    assert alt.shape == xs and np.abs(alt - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("form,cin,cout", [(S2, 64, 64), (S4, 128, 64)], ids=["k4s2", "k8s4"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_deconv_data_grad_impulse_and_residual(be, dt, form, cin, cout):
    """one non-zero dz pixel at wo = 0, at wo = Wout - 1 and inside, exact values (integer weights, distinct columns): the footprint is the
    input columns wi with 0 <= wo + p - s wi < KW, and equals the scatter in every bit; with an integer residual the sum is exact too: one
    float32 add, one rounding"""
    KW, s, p = form
    B, H, Win = 1, 3, 6
    Wout = s * Win
    o = ops_of(be, dt)
    w = np.random.default_rng(3311).integers(-3, 4, (cin, cout, 3, KW)).astype(F32)
    w += (8 * (np.arange(KW) + 1)).astype(F32)            # distinct columns, none zero: a mirrored or shifted footprint cannot pass
    packed = o.pack_deconv_data_grad(w, s, p)
    rv = rnd("ints", (B, H, Win, cin), dt, 3312)
    res = dev16(be, to_bits(rv, dt), dt)
    for wo in (0, Wout - 1, 2 * s + 1):
        dzv = np.zeros((B, H, Wout, cout), F32)
        dzv[0, 1, wo, 5] = 1
        dz = dev16(be, to_bits(dzv, dt), dt)
        got = vals16(be, o.deconv_data_grad(dz, packed), dt).copy()
        ref = AM.data_grad(dzv, w, s, p)
        assert same_bits(got, ref), wo
        cols = np.flatnonzero(np.abs(got).sum((0, 1, 3)))
        assert list(cols) == [wi for wi in range(Win) if 0 <= wo + p - s * wi < KW], (wo, cols)
        for wi in cols:
            assert (got[0, 1, wi] == w[:, 5, 1, wo + p - s * wi]).all()
        assert same_bits(vals16(be, o.deconv_data_grad(dz, packed, residual=res), dt), ref + rv), wo


# ---- rd_affine_relu_add --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_affine_relu_add_bits(be, dt):
    """bit-equal to agg_model.relu_add_f32 (-0 and +0 told apart): about half of the pre-activations are negative under a skip that is not
    zero; the planted pixels give t = -0 with r = -0 (+0: the ReLU's zero is +0), t < 0 with r = -0 (+0) and, in fp16, a sum below the
    half of its smallest subnormal (-0); channel strides and offsets; y aliasing z"""
    L = be.lib
    for (B, H, W, C), lay in [((1, 2, 5, 64), {}), ((2, 3, 37, 128), dict(cs=152, co=16)), ((1, 17, 70, 64), {}), ((2, 3, 9, 8), dict(cs=24, co=8))]:
        z, r = TB.zcase((B, H, W, C), dt, 3401).copy(), rnd("normal", (B, H, W, C), dt, 3402).copy()
        rng = np.random.default_rng(3403)
        a, b = rng.uniform(-1.5, 1.5, C).astype(F32), rng.normal(0, 0.5, C).astype(F32)
        a[0], b[0] = 1.0 - 2.0 ** -12, -0.0
        z[0, 0, 0, 0], r[0, 0, 0, 0] = -0.0, -0.0                 # t = fmaf(-0, a, -0) = -0, r = -0: the ReLU's zero is +0, the sum +0
        z[0, 0, 1, 0], r[0, 0, 1, 0] = -1.0, -0.0                 # t < 0, r = -0: +0
        z[0, 0, 2, 0], r[0, 0, 2, 0] = 2.0 ** -14, -2.0 ** -14    # t = 2^-14 - 2^-26 exactly, the float32 sum -2^-26: -0 in fp16
        r = from_bits(to_bits(r, dt), dt)
        cs, co = lay.get("cs", C), lay.get("co", 0)
        zd, rd, ad, bd = be.up(image(z, dt, cs, co)), be.up(image(r, dt, cs + 16, co + 16)), be.up(a), be.up(b)
        want = to_bits(AM.relu_add_f32(z, a, b, r, dt), dt)
        assert want[0, 0, 0, 0] == 0 and want[0, 0, 1, 0] == 0 and (N.fma32(z, a, b) < 0).mean() > 0.2
        assert want[0, 0, 2, 0] == (0x8000 if dt == R.RD_F16 else to_bits(np.array([-2.0 ** -26], F32), dt)[0])
        out = ff(be, B * H * W * (cs + 8) * 2)
        L.call("rd_affine_relu_add", be.ptr(zd), cs, co, be.ptr(ad), be.ptr(bd), be.ptr(rd), cs + 16, co + 16, be.ptr(out), cs + 8, co + 8, B, H, W, C,
               dt, be.stream)
        got = back_image(be, out, (B, H, W, C), cs + 8, co + 8, dt, "y")
        assert (got == want).all(), ((B, H, W, C), int((got != want).sum()))
        zbuf = be.up(image(z, dt, cs, co))                         # in place: y is z
        L.call("rd_affine_relu_add", be.ptr(zbuf), cs, co, be.ptr(ad), be.ptr(bd), be.ptr(rd), cs + 16, co + 16, be.ptr(zbuf), cs, co, B, H, W, C, dt,
               be.stream)
        raw = be.down(zbuf, np.uint16, (B, H, W, cs))
        assert (raw[..., co:co + C] == want).all(), ("in place", (B, H, W, C))
        outside = np.ones(cs, bool)
        outside[co:co + C] = False
        assert (raw[..., outside] == CM.PAD_PATTERN).all()
    bad = L.raw("rd_affine_relu_add")
    p = be.ptr(zd)
    assert bad(p, 64, 0, be.ptr(ad), be.ptr(bd), p, 64, 0, p, 64, 0, 1, 1, 1, 24, dt, be.stream) == R.RD_ESHAPE
    assert bad(p, 64, 0, be.ptr(ad), be.ptr(bd), None, 64, 0, p, 64, 0, 1, 1, 1, 8, dt, be.stream) == R.RD_EINVAL
    assert bad(p, 64, 0, be.ptr(ad), be.ptr(bd), p, 64, 4, p, 64, 0, 1, 1, 1, 8, dt, be.stream) == R.RD_ESHAPE
    assert bad(p, 64, 0, be.ptr(ad), be.ptr(bd), p, 64, 0, p, 64, 0, 1, 1, 1, 8, R.RD_F32, be.stream) == R.RD_EINVAL


# ---- AggStageTrain -------------------------------------------------------------------------------------------------------------------------------
def agg_params(stage, cin, cout, KW, num_block, seed):
    """a synthetic (arg_params, aux_params) pair of an `agg` stage under the reference's names, and the deconv's own parameters"""
    rng = np.random.default_rng(seed)
    arg, aux, units = TD.stage_params(stage + "_res", cout, cout, num_block, seed + 10)
    w = dweight(cin, cout, KW, seed + 1)
    bn = dict(gamma=rng.uniform(0.5, 1.5, cout).astype(F32), beta=(0.1 * rng.standard_normal(cout)).astype(F32),
              moving_mean=rng.normal(0, 1, cout).astype(F32), moving_var=rng.uniform(0.5, 2, cout).astype(F32))
    arg[stage + "_deconv_weight"] = w
    arg[stage + "_deconv_bn_gamma"], arg[stage + "_deconv_bn_beta"] = bn["gamma"], bn["beta"]
    aux[stage + "_deconv_bn_moving_mean"], aux[stage + "_deconv_bn_moving_var"] = bn["moving_mean"], bn["moving_var"]
    return arg, aux, units, w, bn


@pytest.mark.parametrize("stage,case", [("agg3", (S2, 2, 3, 9, 64, 64)), ("agg2a", (S2, 2, 3, 9, 128, 64)), ("agg1", (S4, 2, 3, 5, 128, 64))],
                         ids=["agg3", "agg2a", "agg1"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_agg_stage_train(be, dt, stage, case):
    """one agg stage with a one-block res stage, forward and backward twice (the same bytes); every kept tensor against the model fed the
    stage's own previous tensors; d_skip is the res stage's input gradient; add_to_up joins d_up in the launch's epilogue; then
    SGD.attach(stage), step(): the masters are optim_model's float32 step, both deconv images the host packers on the downloaded master,
    and the next forward runs on the new weights"""
    from rangedet_amd.backbone_train import AggStageTrain, BasicBlockTrain
    from rangedet_amd.optim import SGD
    A, L = be.alloc, be.lib
    (KW, s, p), B, H, Win, cin, cout = case
    xs, zs = shapes_of(case)
    n = B * H * s * Win
    arg, aux, units, w, bn = agg_params(stage, cin, cout, KW, 1, 3500 + cin + KW)
    st = AggStageTrain.from_params(stage, arg, aux, 1, dtype=dt, lib=L, alloc=A)
    assert (st.kw, st.s, st.p, st.cin, st.cout) == (KW, s, p, cin, cout) and [type(b) for b in st.res.blocks] == [BasicBlockTrain]
    up = dev16(be, to_bits(rnd("relu", xs, dt, 3501), dt), dt)
    skip = dev16(be, to_bits(rnd("relu", zs, dt, 3502), dt), dt)
    g = dev16(be, to_bits(rnd("normal", zs, dt, 3503), dt), dt)
    opt = SGD(lr=0.05, lib=L, alloc=A)
    opt.attach(st)

    def run():
        y = st.forward(skip, up)
        d_skip, d_up, grads = st.backward(g)
        A.sync()
        return [vals16(be, v, dt).tobytes() for v in (y, d_skip, d_up)] + [np.array(A.to_numpy(grads[k])).tobytes() for k in sorted(grads)], d_skip, d_up, grads
    first = run()[0]
    again, d_skip, d_up, grads = run()
    assert again == first, "a second forward / backward differs"
    what = "%s %r %s" % (stage, case, be.name)
    # ---- forward
    upv, skv, z, t = (vals16(be, v, dt) for v in (st.up, st.skip, st.z, st.t))
    assert z.shape == t.shape == zs
    TB.conv_close(z, CM.conv_ref64(TB.nchw(upv), w, dt, fold=True, deconv=(s, p)), dt, what + " z (launch model)")
    close(z, AM.deconv(upv, CM.h16_round(w, dt), s, p), dt, what + " z")
    mean, var, rstd, a, b = TB.check_norm(be, A, z, st.saved, bn, n, cout, dt, what + " deconv_bn")
    assert (to_bits(t, dt) == to_bits(AM.relu_add_f32(z, a, b, skv, dt), dt)).all(), what
    assert 0.2 < (N.fma32(z, a, b) <= 0).mean() < 0.8
    blk = st.res.blocks[0]
    assert vals16(be, blk.x, dt).tobytes() == t.tobytes() and vals16(be, st.y, dt).tobytes() == vals16(be, blk.y, dt).tobytes()
    # ---- backward
    own = ["%s_deconv_%s" % (stage, k) for k in ("weight", "bn_gamma", "bn_beta")]
    res_names = ["%s_res_unit1_%s" % (stage, k) for k in ("conv1_weight", "bn1_gamma", "bn1_beta", "conv2_weight", "bn2_gamma", "bn2_beta", "sc_weight",
                                                          "sc_bn_gamma", "sc_bn_beta")]
    assert sorted(grads) == sorted(own + res_names) and sorted(opt.state()) == sorted(own + res_names)
    assert sorted(st.aux()) == sorted(["%s_deconv_bn_moving_%s" % (stage, k) for k in ("mean", "var")] + list(st.res.aux()))
    gr = {k: np.array(A.to_numpy(v)) for k, v in grads.items()}
    g_t, dz, d_upv = (vals16(be, v, dt) for v in (st.g_t, st.dz, st.d_up))
    assert vals16(be, d_skip, dt).tobytes() == g_t.tobytes() == vals16(be, blk.dx, dt).tobytes() and vals16(be, st.g, dt).tobytes() == vals16(be, g, dt).tobytes()
    m = N.bn_bwd(g_t.reshape(n, cout), z.reshape(n, cout), N.mask_f32(z.reshape(n, cout), a, b), mean, rstd)
    within(gr[own[2]], m["dbeta"], M.sum_bound(n, m["dbeta_abs"]), what + " dbeta")
    within(gr[own[1]], m["dgamma"], M.sum_bound(n, m["dgamma_abs"]), what + " dgamma")
    TB.check_dz(dz, m, bn["gamma"], rstd, gr[own[1]], gr[own[2]], n, dt, what + " dz")
    assert gr[own[0]].shape == (cin, cout, 3, KW)
    check_dwgrad(gr[own[0]], upv, dz, (KW, s, p), False, what + " dW")
    ref_up = AM.data_grad(dz, CM.h16_round(w, dt), s, p)
    close(d_upv, ref_up, dt, what + " d_up")
    assert vals16(be, d_up, dt).tobytes() == d_upv.tobytes() and float(np.abs(d_upv).max()) > 0
    # ---- add_to_up: the same backward with another gradient of `up`
    other = rnd("normal", xs, dt, 3504)
    _, d_up2, _ = st.backward(g, add_to_up=dev16(be, to_bits(other, dt), dt))
    A.sync()
    d_up2 = vals16(be, d_up2, dt).copy()
    close(d_up2, ref_up + other, dt, what + " d_up + add_to_up")
    assert vals16(be, st.dz, dt).tobytes() == dz.tobytes() and (d_up2 != d_upv).mean() > 0.5
    # ---- SGD
    st.backward(g)                                   # (the gradient buffers hold the first backward's values again)
    A.sync()
    y0 = vals16(be, st.y, dt).copy()
    z0 = z.copy()
    shape = (cin, cout, 3, KW)
    w0 = np.array(A.to_numpy(A.view_f32(st.master, shape))).astype(F32)
    v0 = {k: TB.dvec(A, st.bn[k], cout) for k in ("gamma", "beta")}
    assert w0.tobytes() == w.tobytes()
    lr = opt.step()
    A.sync()
    w1 = np.array(A.to_numpy(A.view_f32(st.master, shape))).astype(F32)
    want_w, want_m = OM.sgd_step(w0, gr[own[0]], np.zeros(shape, F32), lr, 0.9, 1e-5, 1.0, 35.0, 1.0, 1.0)
    assert w1.tobytes() == want_w.tobytes() and (w1 != w0).mean() > 0.9
    assert np.array(A.to_numpy(opt.state()[own[0]])).astype(F32).tobytes() == want_m.tobytes()
    for k, name, wdm in (("gamma", own[1], 1.0), ("beta", own[2], 0.0)):
        want_v, _ = OM.sgd_step(v0[k], gr[name], np.zeros(cout, F32), lr, 0.9, 1e-5, 1.0, 35.0, 1.0, wdm)
        assert TB.dvec(A, st.bn[k], cout).tobytes() == want_v.tobytes(), k
    phases = np.concatenate([L.pack_deconv_weight(w1, s, p, q, dt) for q in range(s)])
    assert st.fwd[2] * s == phases.size
    assert be.down(st.fwd[0], np.uint8, (phases.size,)).tobytes() == phases.tobytes()
    dgrad = L.pack_deconv_data_grad(w1, s, p, dt)
    assert be.down(st.bwd[0], np.uint8, (dgrad.size,)).tobytes() == dgrad.tobytes()
    y1 = vals16(be, st.forward(skip, up), dt).copy()
    A.sync()
    z1 = vals16(be, st.z, dt)
    assert (z1 != z0).mean() > 0.3 and (y1 != y0).mean() > 0.3
    close(z1, AM.deconv(upv, CM.h16_round(w1, dt), s, p), dt, what + " z after the step")
    assert opt.table_builds == 1


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_agg_stage_without_res_and_single_steps(be):
    """res_stage=None: the stage ends at the add, d_skip is g itself; the module's single-step functions against the model"""
    from rangedet_amd import backbone_train as BT
    A, L, dt = be.alloc, be.lib, R.RD_BF16
    case = (S4, 2, 3, 5, 128, 128)
    (KW, s, p), B, H, Win, cin, cout = case
    xs, zs = shapes_of(case)
    _, _, _, w, bn = agg_params("agg2", cin, cout, KW, 1, 3600)
    st = BT.AggStageTrain("agg2", w, bn, None, (3, KW), (1, s), (1, p), dtype=dt, lib=L, alloc=A)
    up = dev16(be, to_bits(rnd("relu", xs, dt, 3601), dt), dt)
    skip = dev16(be, to_bits(rnd("relu", zs, dt, 3602), dt), dt)
    g = dev16(be, to_bits(rnd("normal", zs, dt, 3603), dt), dt)
    y = st.forward(skip, up)
    d_skip, d_up, grads = st.backward(g)
    A.sync()
    assert d_skip is g and y is st.t and sorted(grads) == ["agg2_deconv_bn_beta", "agg2_deconv_bn_gamma", "agg2_deconv_weight"]
    assert sorted(st.aux()) == ["agg2_deconv_bn_moving_mean", "agg2_deconv_bn_moving_var"] and len(list(st.optimizer_entries())) == 3
    dzv = vals16(be, st.dz, dt)
    close(vals16(be, d_up, dt), AM.data_grad(dzv, CM.h16_round(w, dt), s, p), dt, "d_up without a res stage")
    xi, zi = rnd("ints", xs, dt, 3604), rnd("ints", zs, dt, 3605)
    dW = BT.deconv_weight_grad(dev16(be, to_bits(xi, dt), dt), dev16(be, to_bits(zi, dt), dt), (3, KW), (1, s), (1, p), dtype=dt, lib=L, alloc=A)
    dx = BT.deconv_data_grad(dev16(be, to_bits(zi, dt), dt), w, (1, s), (1, p), dtype=dt, lib=L, alloc=A)
    a, b = np.linspace(-1, 1, cout).astype(F32), np.linspace(0.5, -0.5, cout).astype(F32)
    t = BT.batch_norm_relu_add_forward(dev16(be, to_bits(zi, dt), dt), a, b, skip, dtype=dt, lib=L, alloc=A)
    A.sync()
    assert same_bits(np.array(A.to_numpy(dW)), AM.weight_grad(xi, zi, KW, s, p, want_abs=False)[0])
    close(vals16(be, dx, dt), AM.data_grad(zi, CM.h16_round(w, dt), s, p), dt, "single-step data gradient")
    assert (to_bits(vals16(be, t, dt), dt) == to_bits(AM.relu_add_f32(zi, a, b, vals16(be, skip, dt), dt), dt)).all()


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_agg_stage_refusals(be):
    from rangedet_amd.backbone_train import AggStageTrain
    from rangedet_amd.optim import SGD
    A, L = be.alloc, be.lib
    bn = dict(gamma=np.ones(64, F32), beta=np.zeros(64, F32), moving_mean=np.zeros(64, F32), moving_var=np.ones(64, F32))
    bn128 = {k: np.resize(v, 128) for k, v in bn.items()}

    def make(w=np.zeros((64, 64, 3, 4), F32), b=bn, kernel=(3, 4), stride=(1, 2), pad=(1, 1), **kw):
        return AggStageTrain("agg3", w, b, None, kernel, stride, pad, lib=L, alloc=A, **kw)
    for kw in (dict(kernel=(3, 3), w=np.zeros((64, 64, 3, 3), F32)), dict(stride=(1, 4)), dict(pad=(1, 2)), dict(stride=(2, 2)), dict(kernel=(3, 8)),
               dict(w=np.zeros((64, 128, 3, 4), F32), b=bn128), dict(w=np.zeros((64, 64, 3, 8), F32), kernel=(3, 8), stride=(1, 4), pad=(1, 2)),
               dict(w=np.zeros((256, 64, 3, 4), F32)), dict(dtype=R.RD_F32)):
        with pytest.raises(NotImplementedError):
            make(**kw)
    st = make()
    up = np.zeros((1, 2, 4, 64), np.uint16)
    for shape in ((1, 2, 4, 64), (1, 2, 8, 128), (1, 3, 8, 64), (2, 2, 8, 64), (1, 2, 16, 64)):
        with pytest.raises(NotImplementedError, match="skip"):
            st.forward(np.zeros(shape, np.uint16), up)
    with pytest.raises(RuntimeError, match="forward"):
        st.backward(np.zeros((1, 2, 8, 64), np.uint16))
    assert make(w=np.zeros((128, 128, 3, 8), F32), b=bn128, kernel=(3, 8), stride=(1, 4), pad=(1, 2)).cout == 128
    opt = SGD(lr=0.1, lib=L, alloc=A)
    buf = A.alloc(64 * 64 * 36 * 4)
    v = A.view_f32(buf, (64, 64, 3, 3))
    with pytest.raises(NotImplementedError, match="deconv"):
        opt.add("x_weight", v, v, pack=dict(deconv=(4, 2, 1), fwd=None, bwd=None))
    with pytest.raises(NotImplementedError, match="deconv"):
        opt.add("x_weight", A.view_f32(buf, (64, 64, 3, 4)), A.view_f32(buf, (64, 64, 3, 4)), pack=dict(deconv=(4, 2, 2)))


# ---- the formulas --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [S2, S4], ids=["k4s2", "k8s4"])
def test_model_agg_stage_matches_autograd(form):
    """CPU only, no library: agg_model.stage_backward against torch float64 autograd on conv_transpose2d, batch_norm(training=True), relu and
    add with a linear loss on top, to 1e-9 of the largest value of each gradient; no pre-activation lies within 1e-6 of zero.  Also the view
    form of the data gradient: the stride-1 conv of dz read as (B, H, Win, s Cout) with agg_model.view_weight"""
    import torch
    import torch.nn.functional as F
    KW, s, p = form
    rng = np.random.default_rng(3701 + KW)
    B, H, Win, cin, cout = 2, 4, 5, 6, 7
    up, skip = rng.standard_normal((B, H, Win, cin)), rng.standard_normal((B, H, s * Win, cout))
    w = rng.standard_normal((cin, cout, 3, KW)) / 5
    gamma, beta = rng.uniform(0.5, 1.5, cout), rng.normal(0, 0.3, cout)
    lin = rng.standard_normal((B, H, s * Win, cout))
    arrs = dict(up=up.transpose(0, 3, 1, 2), skip=skip.transpose(0, 3, 1, 2), w=w, gamma=gamma, beta=beta)
    t = {k: torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, requires_grad=True) for k, v in arrs.items()}
    zt = F.conv_transpose2d(t["up"], t["w"], stride=(1, s), padding=(1, p))
    out = F.relu(F.batch_norm(zt, None, None, t["gamma"], t["beta"], training=True, eps=EPS)) + t["skip"]
    (out * torch.tensor(lin.transpose(0, 3, 1, 2))).sum().backward()
    m = AM.stage_backward(skip, up, w, (gamma, beta), EPS, lin, s, p)
    assert float(np.abs(m["pre"]).min()) > 1e-6, "a pre-activation within 1e-6 of zero: choose another seed"
    assert np.abs(AM.deconv(up, w, s, p) - zt.detach().numpy().transpose(0, 2, 3, 1)).max() < 1e-12
    pairs = [("t", m["t"], out.detach().numpy().transpose(0, 2, 3, 1)), ("d_up", m["d_up"], t["up"].grad.numpy().transpose(0, 2, 3, 1)),
             ("d_skip", m["d_skip"], t["skip"].grad.numpy().transpose(0, 2, 3, 1)), ("deconv_weight", m["deconv_weight"], t["w"].grad.numpy()),
             ("deconv_bn_gamma", m["deconv_bn_gamma"], t["gamma"].grad.numpy()), ("deconv_bn_beta", m["deconv_bn_beta"], t["beta"].grad.numpy())]
    for name, got, want in pairs:
        rel = float(np.abs(got - want).max() / np.abs(want).max())
        print(name, "relative difference %.3g" % rel)
        assert rel < 1e-9, (name, rel)
    view = F.conv2d(torch.tensor(m["dz"].reshape(B, H, Win, s * cout).transpose(0, 3, 1, 2)), torch.tensor(AM.view_weight(w, s, p).astype(np.float64)),
                    padding=1).numpy().transpose(0, 2, 3, 1)
    assert np.abs(view - AM.data_grad(m["dz"], w.astype(F32), s, p)).max() < 1e-6 * np.abs(view).max()
    assert 0.3 < float((m["pre"] <= 0).mean()) < 0.7
    assert (AM.tap_terms(B, H, Win, KW, s, p) > 0).all() and AM.tap_terms(1, 2, 1, KW, s, p)[0].tolist() == [0] * p + [1] * s + [0] * p

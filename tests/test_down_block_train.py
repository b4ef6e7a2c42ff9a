"""The stride-(1,2) BasicBlock in training mode (csrc/k_convbwd.h: rd_conv3x3_bwd_weight_ex; csrc/k_optim.h: the strided images of an
optimizer entry; rangedet_amd.backward.TowerOps: the strided steps; rangedet_amd.backbone_train.DownBlockTrain / ResStageTrain.from_params)
against tests/down_block_model.py, the restatement of the formulas in include/rangedet_hip.h.  Through the C ABI, in the style of
test_basic_block_train.py (whose checks of the unchanged steps are used as they are): every output buffer and the workspace are pre-filled
with 0xFF bytes and carry a guard tail; the tail and the channels outside [coff, coff + C) must be unchanged afterwards; each step is
compared with the model fed THE KERNEL'S OWN inputs to it.  x is (B, H, Win, C); the shapes:

  (1, 2, 2, 64)      Wo = 1: the tap column dw = -1 lies entirely outside the image
  (2, 3, 18, 128)    a small general case
  (2, 5, 140, 64)    Wo = 70: a full 64-pixel tile and one of 6 pixels, dw = +1 at the last output pixel reads the last input column
  (1, 17, 74, 128)   H crosses the 16-row strip; Wo = 37

  rd_conv3x3_bwd_weight_ex   stride 2: a float64 einsum within convbwd_model.sum_bound at every shape and split; exact inputs equal in every
                             bit at every split; the workspace is partials x 9 x cout x cin x 4 bytes with the model's partial count; two
                             calls give the same bytes; nine distinct integer tap patterns come back each in its own (ky, kx) slot; stride 1:
                             the bytes and the workspace of rd_conv3x3_bwd_weight
  data_grad_s2               the float64 scatter on the packer-rounded weight within conv_model.conv_tol; impulses at wo = 0, Wo - 1 and
                             inside: the footprint's columns
  optimizer                  after a step the strided images equal the host packers on the downloaded master byte for byte; a table of
                             entries without a stride has the bytes of the layout before the field
  DownBlockTrain             every kept intermediate step by step on the block's own previous tensors, dx under the documented rounding
                             sequence; the next forward after SGD.step() runs on the new weights; a stage of a down block and an identity
                             block; ResStageTrain.from_params
  the model itself           down_block_model.block_backward against torch.autograd in float64, to a relative 1e-9
"""
import ctypes

import numpy as np
import pytest

import block_model as BM
import conv_model as CM
import convbwd_model as M
import down_block_model as DM
import norm_model as N
import optim_model as OM
import test_basic_block_train as TB
from conftest import BOTH
from rangedet_amd import lib as R
from train_util import DTS, back, check_wgrad, dev16, ff, image, rnd, same_bits, to_bits, vals16

F32 = np.float32
EPS, MOM = TB.EPS, TB.MOM
SHAPES = [(1, 2, 2, 64), (2, 3, 18, 128), (2, 5, 140, 64), (1, 17, 74, 128)]
SPLITS = (1, 2, 3, 7, 0)
IDS = dict(ids=lambda s: "x".join(str(v) for v in s))
within = TB.within


# ---- rd_conv3x3_bwd_weight_ex ------------------------------------------------------------------------------------------------------------------
def run_wgrad(be, dt, x, dz, stride_w=2, split=0, xcs=None, xco=0, zcs=None, zco=0, twice=False, entry="ex"):
    """-> dW (cout, cin, 3, 3), the partial count the workspace size implies, the workspace size"""
    L = be.lib
    B, H, Win, cin = x.shape
    cout = dz.shape[3]
    if entry == "ex":
        nws = L.raw("rd_conv3x3_bwd_weight_ex_workspace_bytes")(B, H, Win, cin, cout, stride_w, split)
    else:
        nws = L.raw("rd_conv3x3_bwd_weight_workspace_bytes")(B, H, Win, cin, cout, split)
    assert nws > 0 and nws % (36 * cin * cout) == 0
    xd, zd = be.up(image(x, dt, xcs, xco)), be.up(image(dz, dt, zcs, zco))
    outs = []
    for _ in range(2 if twice else 1):
        dW, ws = ff(be, cout * cin * 36), ff(be, nws)
        if entry == "ex":
            L.call("rd_conv3x3_bwd_weight_ex", be.ptr(xd), xcs or cin, xco, be.ptr(zd), zcs or cout, zco, be.ptr(dW), B, H, Win, cin, cout, stride_w,
                   split, dt, be.ptr(ws), nws, be.stream)
        else:
            L.call("rd_conv3x3_bwd_weight", be.ptr(xd), xcs or cin, xco, be.ptr(zd), zcs or cout, zco, be.ptr(dW), B, H, Win, cin, cout, split, dt,
                   be.ptr(ws), nws, be.stream)
        back(be, ws, nws, "workspace")
        outs.append(back(be, dW, cout * cin * 36, "dW"))
    if twice:
        assert outs[0].tobytes() == outs[1].tobytes(), "two calls differ"
    return outs[0].view(F32).reshape(cout, cin, 3, 3).copy(), nws // (36 * cin * cout), nws


def check_wgrad_s2(got, x, dz, exact, what):
    want, sabs, n = DM.weight_grad_s2(x, dz, want_abs=not exact)
    assert np.isfinite(got).all(), what
    if exact:
        bad = int((got != want.astype(F32)).sum())
        print(what, "exact: elements that differ", bad)
        assert same_bits(got, want), (what, bad)
    else:
        within(got, want, M.sum_bound(n[None, None], sabs), what)


@pytest.mark.parametrize("shape", SHAPES, **IDS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_weight_grad_s2_every_split(be, dt, shape):
    """ReLU-sparse x against normal dz within sum_bound, and integer inputs equal in every bit, at every split; the workspace is the model's
    partial count; two calls agree.  cout = cin at these shapes, and once 64 -> 128 and 128 -> 64 at the library's own split"""
    B, H, Win, C = shape
    zshape = (B, H, Win // 2, C)
    xr, zr = rnd("relu", shape, dt, 2101), rnd("normal", zshape, dt, 2102)
    xi, zi = rnd("ints", shape, dt, 2103), rnd("ints", zshape, dt, 2104)
    for split in SPLITS:
        what = "wgrad s2 %r split %d %s" % (shape, split, be.name)
        got, S, nws = run_wgrad(be, dt, xr, zr, split=split, twice=split == 0)
        assert S == DM.parts3x3(B, H, Win // 2, C, split) and nws == S * 9 * C * C * 4, (what, S)
        check_wgrad_s2(got, xr, zr, False, what + " random")
        got, _, _ = run_wgrad(be, dt, xi, zi, split=split)
        check_wgrad_s2(got, xi, zi, True, what)
    cout = 192 - C
    zo = rnd("ints", (B, H, Win // 2, cout), dt, 2105)
    got, S, _ = run_wgrad(be, dt, xi, zo)
    assert S == DM.parts3x3(B, H, Win // 2, cout, 0)
    check_wgrad_s2(got, xi, zo, True, "wgrad s2 %r %d->%d %s" % (shape, C, cout, be.name))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_weight_grad_s2_channel_stride_and_offset(be, dt):
    """x: 128 channels at offset 8 of 136; dz: 128 channels at offset 16 of 152"""
    shape = (2, 3, 18, 128)
    for kind, exact in (("relu", False), ("ints", True)):
        x, dz = rnd(kind, shape, dt, 2111), rnd("normal" if kind == "relu" else "ints", (2, 3, 9, 128), dt, 2112)
        got, _, _ = run_wgrad(be, dt, x, dz, split=2, xcs=136, xco=8, zcs=152, zco=16)
        check_wgrad_s2(got, x, dz, exact, "wgrad s2 strided %s %s" % (kind, be.name))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_weight_grad_s2_tap_probe(be, dt):
    """x is a single 1 at one pixel (channel 3), dz holds 3 ky + kx + 1 (channel 7) at the output pixel that tap (ky, kx) pairs with it:
    h = h0 - ky + 1, wo = (w - kx + 1) / 2.  An odd input column meets kx 0 and kx 2, an even one kx 1, so two launches cover the nine taps;
    every dz pixel meets the input pixel through exactly one tap, so dW[7, 3, ky, kx] = 3 ky + kx + 1 and every other element is zero: a
    swapped or mirrored tap column or row shows as a permutation."""
    B, H, Win, C = 1, 5, 12, 64
    x, dz = np.zeros((B, H, Win, C), F32), np.zeros((B, H, Win // 2, C), F32)
    h0, w_odd, w_even = 2, 5, 6
    for w_in, taps in ((w_odd, (0, 2)), (w_even, (1,))):
        x1 = np.zeros_like(x)
        x1[0, h0, w_in, 3] = 1
        d1 = np.zeros_like(dz)
        for ky in range(3):
            for kx in taps:
                d1[0, h0 - ky + 1, (w_in - kx + 1) // 2, 7] = 3 * ky + kx + 1
        got, _, _ = run_wgrad(be, dt, x1, d1)
        expect = np.zeros((C, C, 3, 3), F32)
        for ky in range(3):
            for kx in taps:
                expect[7, 3, ky, kx] = 3 * ky + kx + 1
        assert same_bits(got, expect), (w_in, got[7, 3])
        assert same_bits(got, DM.weight_grad_s2(x1, d1, want_abs=False)[0])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_weight_grad_stride1_through_ex(be, dt):
    """stride_w = 1 through the new entry point: the bytes and the workspace size of rd_conv3x3_bwd_weight on the same inputs"""
    for shape, cout, split in (((2, 3, 37, 64), 128, 0), ((1, 17, 70, 128), 128, 3)):
        x, dz = rnd("relu", shape, dt, 2121), rnd("normal", shape[:3] + (cout,), dt, 2122)
        old, S0, n0 = run_wgrad(be, dt, x, dz, split=split, entry="old")
        new, S1, n1 = run_wgrad(be, dt, x, dz, stride_w=1, split=split)
        assert new.tobytes() == old.tobytes() and (S0, n0) == (S1, n1)
        check_wgrad(new, x, dz, False, "stride 1 through ex %r %s" % (shape, be.name))


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_weight_grad_ex_status_codes(be):
    """odd Win with stride 2, stride 3, bad channels, a workspace one byte short, null pointers: each its code, the message names the entry,
    nothing launched"""
    L = be.lib
    n = 1 << 20
    buf = be.up(np.full(n, 0xFF, np.uint8))
    p = be.ptr(buf)
    ws_w = L.raw("rd_conv3x3_bwd_weight_ex_workspace_bytes")

    def wg(x=p, dz=p, dW=p, ws=p, cin=64, cout=64, B=1, H=2, Win=8, sw=2, xcs=None, xco=0, split=0, dt=R.RD_BF16, nws=n):
        return L.raw("rd_conv3x3_bwd_weight_ex")(x, xcs or cin, xco, dz, cout, 0, dW, B, H, Win, cin, cout, sw, split, dt, ws, nws, be.stream)

    def msg():
        return L.rd_last_error_string().decode()
    assert ws_w(1, 2, 8, 64, 64, 2, 0) == 9 * 64 * 64 * 4 and ws_w(1, 2, 8, 64, 64, 1, 0) == 9 * 64 * 64 * 4
    assert ws_w(1, 2, 7, 64, 64, 2, 0) == 0 and ws_w(1, 2, 8, 64, 64, 3, 0) == 0 and ws_w(1, 2, 8, 96, 64, 2, 0) == 0 and ws_w(1, 2, 8, 64, 64, 2, -1) == 0
    assert ws_w(8, 64, 2656, 64, 64, 2, 0) == 170 * 9 * 64 * 64 * 4 and ws_w(8, 64, 332, 128, 128, 2, 0) == 85 * 9 * 128 * 128 * 4
    for kw in (dict(Win=7), dict(sw=3), dict(sw=0), dict(cin=96), dict(cout=32), dict(cin=256), dict(B=0), dict(H=0), dict(Win=0), dict(xco=4, xcs=72),
               dict(xcs=60)):
        assert wg(**kw) == R.RD_ESHAPE and msg().startswith("conv3x3_bwd_weight_ex"), (kw, msg())
    for name in ("x", "dz", "dW", "ws"):
        assert wg(**{name: None}) == R.RD_EINVAL and msg().startswith("conv3x3_bwd_weight_ex") and "null" in msg(), name
    assert wg(dt=R.RD_F32) == R.RD_EINVAL and wg(split=-1) == R.RD_EINVAL and msg().startswith("conv3x3_bwd_weight_ex")
    for sw in (1, 2):
        assert wg(sw=sw, nws=ws_w(1, 2, 8, 64, 64, sw, 0) - 1) == R.RD_EWORKSPACE and msg().startswith("conv3x3_bwd_weight_ex") and "workspace" in msg()
    assert wg(x=p + 8) == R.RD_EINVAL and "aligned" in msg()
    assert (be.down(buf, np.uint8, (n,)) == 0xFF).all()           # nothing ran


# ---- the data gradient -------------------------------------------------------------------------------------------------------------------------
def ops_of(be, dt):
    from rangedet_amd.backward import TowerOps
    return TowerOps(dt, be.lib, be.alloc)


def weight(cout, cin, seed):
    return (np.random.default_rng(seed).standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin / 2)).astype(F32)


@pytest.mark.parametrize("shape", SHAPES, **IDS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_data_grad_s2(be, dt, shape):
    """g1 of the strided conv against the float64 scatter on the rounded weight, alone and with a residual added in the epilogue"""
    B, H, Win, C = shape
    o = ops_of(be, dt)
    w = weight(C, C, 2201)
    dzv, rv = rnd("normal", (B, H, Win // 2, C), dt, 2202), rnd("normal", shape, dt, 2203)
    packed = o.pack_data_grad_s2(w)
    dz, res = dev16(be, to_bits(dzv, dt), dt), dev16(be, to_bits(rv, dt), dt)
    ref = DM.data_grad_s2(dzv, CM.h16_round(w, dt))
    for r, rval in ((None, 0.0), (res, rv)):
        got = vals16(be, o.data_grad_s2(dz, packed, residual=r), dt)
        assert got.shape == shape
        over, worst = CM.conv_check(got, ref + rval, dt)
        print("data_grad_s2 %r %s residual %s: over %d, worst err / tol %.3g" % (shape, be.name, r is not None, over, worst))
        assert over == 0, (shape, over, worst)
    # the same sum as the transposed conv the launch is: the model of the deconv launches agrees with the scatter
    alt = CM.conv_ref64(dzv.transpose(0, 3, 1, 2), DM.deconv_weight(w), dt, fold=True, deconv=(2, 1)).transpose(0, 2, 3, 1)
    assert alt.shape == shape and np.abs(alt - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_data_grad_s2_impulse(be, dt):
    """one non-zero dz pixel at wo = 0, at wo = Wo - 1 and inside, exact values (integer weights): the footprint is the columns 2wo-1 .. 2wo+1
    that lie in the image -- column Win does not exist, the buffer's guard is intact -- and equals the scatter in every bit"""
    B, H, Win, C = 1, 3, 10, 64
    Wo = Win // 2
    o = ops_of(be, dt)
    w = np.random.default_rng(2211).integers(-3, 4, (C, C, 3, 3)).astype(F32)
    w[:, :, :, 0] += 8            # distinct columns: a mirrored footprint cannot pass
    packed = o.pack_data_grad_s2(w)
    for wo in (0, Wo - 1, 2):
        dzv = np.zeros((B, H, Wo, C), F32)
        dzv[0, 1, wo, 5] = 1
        got = vals16(be, o.data_grad_s2(dev16(be, to_bits(dzv, dt), dt), packed), dt)
        ref = DM.data_grad_s2(dzv, w)
        assert same_bits(got, ref), wo
        cols = np.flatnonzero(np.abs(got).sum((0, 1, 3)))
        assert list(cols) == [c for c in (2 * wo - 1, 2 * wo, 2 * wo + 1) if 0 <= c < Win], (wo, cols)
        assert (got[0, 1, 2 * wo] == w[5, :, 1, 1]).all()


def test_forward_s2_matches_model_of_launch():
    """CPU only: down_block_model.conv3_s2 is conv_model.conv_ref64 with stride 2 (torch conv2d, stride (1, 2), padding 1)"""
    rng = np.random.default_rng(2221)
    x, w = rng.standard_normal((2, 3, 8, 5)), rng.standard_normal((4, 5, 3, 3))
    import torch
    import torch.nn.functional as F
    ref = F.conv2d(torch.tensor(x.transpose(0, 3, 1, 2)), torch.tensor(w), stride=(1, 2), padding=1).numpy().transpose(0, 2, 3, 1)
    assert np.abs(DM.conv3_s2(x, w) - ref).max() < 1e-12


# ---- optimizer ---------------------------------------------------------------------------------------------------------------------------------
def s2_images(L, w, fold, dt):
    C = w.shape[0]
    fwd = L.pack_conv3x3_ex(w, 2, C, fold_scale=fold, dtype=dt)
    wd = DM.deconv_weight(w)
    return fwd, np.concatenate([L.pack_deconv_weight(wd, 2, 1, p, dt) for p in (0, 1)])


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_optimizer_strided_images(be, dt, C):
    """a table of two (C, C, 3, 3) weights with stride_w = 2 -- one with a fold scale, one without (the first on exact rounding ties) -- a
    stride-1 weight of the same shape and a bias: after each of two steps every master and momentum equals optim_model.sgd_step in every
    bit and every image equals the host packers on the downloaded master, zero fill and zero tails included"""
    L = be.lib
    rng = np.random.default_rng(2301 + C)
    shapes = [(C, C, 3, 3), (C, C, 3, 3), (C, C, 3, 3), (5,)]
    stride = [2, 2, 1, 0]
    w = [rng.standard_normal(s).astype(F32) for s in shapes]
    w[1] = OM.tie_values(shapes[1], dt, rng, dt == R.RD_BF16)
    m = [(0.1 * rng.standard_normal(s)).astype(F32) for s in shapes]
    fold = [rng.uniform(0.5, 1.5, C).astype(F32), None, None, None]
    n_fwd = [L.cdll.rd_conv3x3_ex_packed_bytes(C, C, 2, C)] * 2 + [9 * C * C * 2 + 256]
    n_bwd = [2 * L.cdll.rd_conv_packed_bytes(6, C, C, dt)] * 2 + [9 * C * C * 2 + 256]
    assert n_fwd[0] == 24 * C * C + 256 and n_bwd[0] == 2 * (12 * C * C + 256)
    wdv, mdv = [TB.fup(be, v) for v in w], [TB.fup(be, v) for v in m]
    fdv = [None if f is None else TB.fup(be, f) for f in fold]
    for step, lr in enumerate((0.1, 0.05)):
        g = [(10 * rng.standard_normal(s)).astype(F32) for s in shapes]
        gdv = [TB.fup(be, v) for v in g]
        fwd, bwd = [ff(be, nb) for nb in n_fwd] + [None], [ff(be, nb) for nb in n_bwd] + [None]
        ts = [R.SgdTensor(be.ptr(wdv[i]), be.ptr(gdv[i]), be.ptr(mdv[i]), int(np.prod(s)), 1.0, 1.0, s[0] if len(s) == 4 else 0,
                          s[1] if len(s) == 4 else 0, be.ptr(fwd[i]), be.ptr(bwd[i]), be.ptr(fdv[i]), stride[i]) for i, s in enumerate(shapes)]
        host = L.sgd_table(ts, dt)
        L.call("rd_sgd_mom_update", be.ptr(be.up(host)), host.ctypes.data, lr, 0.9, 1e-5, 1.0, 35.0, be.stream)
        for i, s in enumerate(shapes):
            w[i], m[i] = OM.sgd_step(w[i], g[i], m[i], lr, 0.9, 1e-5, 1.0, 35.0, 1.0, 1.0)
            got_w = back(be, wdv[i], w[i].nbytes, "weight %d" % i).view(F32).reshape(s)
            got_m = back(be, mdv[i], m[i].nbytes, "mom %d" % i).view(F32).reshape(s)
            assert got_w.tobytes() == w[i].tobytes() and got_m.tobytes() == m[i].tobytes(), ("step", step, "tensor", i)
            if len(s) != 4:
                continue
            want = s2_images(L, got_w, fold[i], dt) if stride[i] == 2 else (OM.forward_image(L, got_w, None, dt), OM.data_grad_image(L, got_w, dt))
            for img, wt, nb, name in ((fwd[i], want[0], n_fwd[i], "forward"), (bwd[i], want[1], n_bwd[i], "data-gradient")):
                assert wt.size == nb
                got = back(be, img, nb, "%s image %d" % (name, i))
                assert int((got != wt).sum()) == 0 and not got[-256:].any() and wt.any(), ("step", step, "tensor", i, name, int((got != wt).sum()))


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_optimizer_table_without_stride_is_unchanged(be):
    """eleven-field constructions (a 3x3 weight with both images and a fold scale, a 1x1 weight with one image, a vector) give the bytes of the
    table layout before the field, restated in down_block_model.table_v11; stride_w = 1 gives the same bytes; the struct grew at its end only"""
    L = be.lib
    buf = be.empty(1 << 16)
    p = be.ptr(buf)
    fields = [dict(weight=p, grad=p + 64, mom=p + 128, n=9 * 64 * 128, lr_mult=1.0, wd_mult=1.0, cout=128, cin=64, pack_fwd=p + 256, pack_bwd=p + 512, fold_scale=p + 16),
              dict(weight=p + 32, grad=p, mom=p, n=64 * 64, lr_mult=0.5, wd_mult=0.0, cout=64, cin=64, pack_fwd=0, pack_bwd=p + 1024, fold_scale=0),
              dict(weight=p, grad=p, mom=p, n=1029, lr_mult=2.0, wd_mult=1.0, cout=0, cin=0, pack_fwd=0, pack_bwd=0, fold_scale=0)]
    order = ("weight", "grad", "mom", "n", "lr_mult", "wd_mult", "cout", "cin", "pack_fwd", "pack_bwd", "fold_scale")
    ts = [R.SgdTensor(*[(t[k] or None) if k.startswith("pack") or k == "fold_scale" else t[k] for k in order]) for t in fields]
    assert all(t.stride_w == 0 for t in ts)
    want = DM.table_v11(fields, R.RD_F16)
    got = L.sgd_table(ts, R.RD_F16)
    assert got.tobytes() == want.tobytes()
    for t in ts:
        t.stride_w = 1
    assert L.sgd_table(ts, R.RD_F16).tobytes() == want.tobytes()
    assert [f[0] for f in R.SgdTensor._fields_][:11] == list(order) and R.SgdTensor._fields_[11][0] == "stride_w"
    assert R.SgdTensor.fold_scale.offset == 64 and R.SgdTensor.stride_w.offset == 72 and ctypes.sizeof(R.SgdTensor) == 80


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_optimizer_strided_refusals(be):
    """stride_w = 2 with cin != cout or on a 1x1 weight, and a stride outside 0 .. 2, are refused; the refusals from before keep their words"""
    L = be.lib
    buf = be.empty(1 << 16)
    p = be.ptr(buf)
    for n, co, ci, sw, code, words in ((9 * 64 * 128, 128, 64, 2, R.RD_ESHAPE, "stride_w 2"), (64 * 64, 64, 64, 2, R.RD_ESHAPE, "stride_w 2"),
                                       (9 * 64 * 64, 64, 64, 3, R.RD_EINVAL, "stride_w 3"), (64 * 64, 64, 16, 2, R.RD_ESHAPE, "body form"),
                                       (64 * 64 * 4, 64, 64, 2, R.RD_ESHAPE, "9 x")):
        t = R.SgdTensor(p, p, p, n, 1.0, 1.0, co, ci, p, None, None, sw)
        with pytest.raises(R.RangeDetError, match=words) as e:
            L.sgd_table([t], R.RD_BF16)
        assert e.value.code == code
    # without an image the field is not read
    assert L.sgd_table([R.SgdTensor(p, p, p, 100, 1.0, 1.0, 0, 0, None, None, None, 2)], R.RD_BF16).size > 0


# ---- DownBlockTrain ------------------------------------------------------------------------------------------------------------------------------
def make_down(be, dt, p):
    from rangedet_amd.backbone_train import DownBlockTrain
    return DownBlockTrain(p["name"], p["conv1_w"], p["conv2_w"], p["bn1"], p["bn2"], p["sc_w"], p["sc_bn"], dtype=dt, lib=be.lib, alloc=be.alloc)


def nchw(v):
    return v.transpose(0, 3, 1, 2)


def close(got, ref, dt, what):
    over, worst = CM.conv_check(got, ref, dt)
    print("%s: over tolerance %d, worst err / tol %.3g" % (what, over, worst))
    assert over == 0, (what, over, worst)


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (128, 128)], ids=["64", "64to128", "128"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_down_block_train(be, dt, cin, cout):
    """B 2, 3 x 38 -> 19: forward and backward twice (the same bytes); every kept tensor against the model fed the block's own previous
    tensors; dx under the class's rounding sequence: ds rounded once onto the even pixels, +0 on the odd ones, then one float32 add in
    conv1's data gradient and one rounding"""
    A = be.alloc
    B, H, Win = 2, 3, 38
    Wo = Win // 2
    n1, n = B * H * Win, B * H * Wo
    name = "res2_unit1"
    p = TB.block_params(name, cin, cout, True, 2400 + cin + 2 * cout)
    blk = make_down(be, dt, p)
    x = dev16(be, to_bits(rnd("relu", (B, H, Win, cin), dt, 2401), dt), dt)
    g = dev16(be, to_bits(rnd("normal", (B, H, Wo, cout), dt, 2402), dt), dt)
    blk.forward(x)
    dx1st, grads1st = blk.backward(g)
    A.sync()
    first = [vals16(be, blk.y, dt).tobytes(), vals16(be, dx1st, dt).tobytes()] + [np.array(A.to_numpy(grads1st[k])).tobytes() for k in sorted(grads1st)]
    y = blk.forward(x)
    dx, grads = blk.backward(g)
    A.sync()
    again = [vals16(be, y, dt).tobytes(), vals16(be, dx, dt).tobytes()] + [np.array(A.to_numpy(grads[k])).tobytes() for k in sorted(grads)]
    assert again == first, "a second forward / backward differs"
    what = "down block %d->%d %s" % (cin, cout, be.name)
    # ---- forward
    xv, z1, y1, z2, zs, yv = (vals16(be, v, dt) for v in (blk.x, blk.z1, blk.y1, blk.z2, blk.zs, blk.y))
    assert z1.shape == (B, H, Win, cout) and z2.shape == zs.shape == yv.shape == (B, H, Wo, cout)
    TB.conv_close(z1, CM.conv_ref64(nchw(xv), p["conv1_w"], dt, fold=True), dt, what + " z1")
    vec = {}
    for key, z, cnt in (("bn1", z1, n1), ("bn2", z2, n), ("sc_bn", zs, n)):
        vec[key] = TB.check_norm(be, A, z, blk.saved[key], p[key], cnt, cout, dt, "%s %s" % (what, key))
    a1, b1 = vec["bn1"][3:]
    assert same_bits(y1, N.affine_relu_f32(z1, a1, b1, dt)), what
    close(z2, DM.conv3_s2(y1, CM.h16_round(p["conv2_w"], dt)), dt, what + " z2")
    TB.conv_close(z2, CM.conv_ref64(nchw(y1), p["conv2_w"], dt, fold=True, stride=2), dt, what + " z2 (launch model)")
    close(zs, xv[:, :, 0::2].astype(np.float64) @ CM.h16_round(p["sc_w"].reshape(cout, cin), dt).astype(np.float64).T, dt, what + " zs")
    a2, b2 = vec["bn2"][3:]
    ars, brs = vec["sc_bn"][3:]
    assert same_bits(yv, BM.add_relu_f32(z2, a2, b2, zs, ars, brs, dt)), what
    assert 0.2 < (yv == 0).mean() < 0.8
    # ---- backward
    want_names = ["%s_%s" % (name, s) for s in ("conv1_weight", "bn1_gamma", "bn1_beta", "conv2_weight", "bn2_gamma", "bn2_beta", "sc_weight",
                                                "sc_bn_gamma", "sc_bn_beta")]
    assert sorted(grads) == sorted(want_names)
    gr = {k[len(name) + 1:]: np.array(A.to_numpy(v)) for k, v in grads.items()}
    assert gr["conv1_weight"].shape == (cout, cin, 3, 3) and gr["conv2_weight"].shape == (cout, cout, 3, 3) and gr["sc_weight"].shape == (cout, cin, 1, 1)
    gv, dz2, dr, g1, dz1, ds, dxv = (vals16(be, v, dt) for v in (blk.g, blk.dz2, blk.dr, blk.g1, blk.dz1, blk.ds, blk.dx))
    assert dz2.shape == dr.shape == (B, H, Wo, cout) and g1.shape == dz1.shape == (B, H, Win, cout) and ds.shape == dxv.shape == (B, H, Win, cin)
    main = (a2, b2) + vec["bn2"][0:1] + vec["bn2"][2:3] + (p["bn2"]["gamma"],)
    sc = (ars, brs, vec["sc_bn"][0], vec["sc_bn"][2], p["sc_bn"]["gamma"])
    zero = TB.check_add_bwd((dz2, dr, gr["bn2_gamma"], gr["bn2_beta"], gr["sc_bn_gamma"], gr["sc_bn_beta"]), gv, z2, zs, main, sc, dt, False, what + " bn2")
    assert 0.2 < zero < 0.8
    check_wgrad_s2(gr["conv2_weight"], y1, dz2, False, what + " dW2")
    close(g1, DM.data_grad_s2(dz2, CM.h16_round(p["conv2_w"], dt)), dt, what + " g1")
    mean1, rstd1 = vec["bn1"][0], vec["bn1"][2]
    m1 = N.bn_bwd(g1.reshape(n1, cout), z1.reshape(n1, cout), N.mask_f32(z1.reshape(n1, cout), a1, b1), mean1, rstd1)
    within(gr["bn1_beta"], m1["dbeta"], M.sum_bound(n1, m1["dbeta_abs"]), what + " dbeta1")
    within(gr["bn1_gamma"], m1["dgamma"], M.sum_bound(n1, m1["dgamma_abs"]), what + " dgamma1")
    TB.check_dz(dz1, m1, p["bn1"]["gamma"], rstd1, gr["bn1_gamma"], gr["bn1_beta"], n1, dt, what + " dz1")
    check_wgrad(gr["conv1_weight"], xv, dz1, False, what + " dW1")
    TB.check_wgrad1(gr["sc_weight"].reshape(cout, cin), xv[:, :, 0::2], dr, False, what + " dWs")
    wsT = CM.h16_round(p["sc_w"].reshape(cout, cin), dt).astype(np.float64)
    close(ds[:, :, 0::2], dr.astype(np.float64) @ wsT, dt, what + " ds")
    assert not to_bits(ds[:, :, 1::2], dt).any(), "ds on the odd pixels is +0"
    assert float(np.abs(ds).max()) > 0
    TB.conv_close(dxv, CM.conv_ref64(nchw(dz1), M.flip_weight(p["conv1_w"]), dt, fold=True, flags=R.RD_ADD, res=nchw(ds)), dt, what + " dx")
    assert vals16(be, dx, dt).tobytes() == dxv.tobytes()


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_down_block_refusals(be):
    from rangedet_amd.backbone_train import BasicBlockTrain, DownBlockTrain
    A, L = be.alloc, be.lib
    bn = dict(gamma=np.ones(64, F32), beta=np.zeros(64, F32), moving_mean=np.zeros(64, F32), moving_var=np.ones(64, F32))
    bn128 = {k: np.resize(v, 128) for k, v in bn.items()}
    w, ws = np.zeros((64, 64, 3, 3), F32), np.zeros((64, 64, 1, 1), F32)

    def make(w1=w, w2=w, b1=bn, b2=bn, sc_w=ws, sc_bn=bn, **kw):
        return DownBlockTrain("res2_unit1", w1, w2, b1, b2, sc_w, sc_bn, lib=L, alloc=A, **kw)
    with pytest.raises(NotImplementedError, match="projection"):
        make(sc_w=None, sc_bn=None)
    with pytest.raises(NotImplementedError, match="64 -> 64, 64 -> 128 and 128 -> 128"):
        make(w1=np.zeros((64, 128, 3, 3), F32), sc_w=np.zeros((64, 128, 1, 1), F32))
    with pytest.raises(NotImplementedError, match="64 or 128"):
        make(w1=np.zeros((256, 64, 3, 3), F32), w2=np.zeros((256, 256, 3, 3), F32))
    with pytest.raises(NotImplementedError, match="fewer than 64 input channels"):
        make(w1=np.zeros((64, 8, 3, 3), F32), sc_w=np.zeros((64, 8, 1, 1), F32))
    with pytest.raises(NotImplementedError, match="16-bit"):
        make(dtype=R.RD_F32)
    with pytest.raises(NotImplementedError, match="even width"):
        make().forward(np.zeros((1, 2, 7, 64), np.uint16))
    with pytest.raises(RuntimeError, match="forward"):
        make().backward(np.zeros((1, 2, 4, 64), np.uint16))
    with pytest.raises(NotImplementedError, match="strided.*DownBlockTrain"):
        BasicBlockTrain("res2_unit1", w, w, bn, bn, ws, bn, stride=(1, 2), lib=L, alloc=A)
    assert make(w1=np.zeros((128, 64, 3, 3), F32), w2=np.zeros((128, 128, 3, 3), F32), b1=bn128, b2=bn128, sc_w=np.zeros((128, 64), F32), sc_bn=bn128).cout == 128


def stage_params(stage, cin, cout, num_block, seed):
    """a synthetic (arg_params, aux_params) pair of a `res` stage under the reference's names, and the per-unit dicts of block_params"""
    arg, aux, units = {}, {}, []
    for i in range(1, num_block + 1):
        unit = "%s_unit%d" % (stage, i)
        p = TB.block_params(unit, cin if i == 1 else cout, cout, i == 1, seed + i)
        units.append(p)
        for key in ("conv1", "conv2") + (("sc",) if i == 1 else ()):
            arg["%s_%s_weight" % (unit, key)] = p[key + "_w"]
        for key in ("bn1", "bn2") + (("sc_bn",) if i == 1 else ()):
            arg["%s_%s_gamma" % (unit, key)], arg["%s_%s_beta" % (unit, key)] = p[key]["gamma"], p[key]["beta"]
            aux["%s_%s_moving_mean" % (unit, key)], aux["%s_%s_moving_var" % (unit, key)] = p[key]["moving_mean"], p[key]["moving_var"]
    return arg, aux, units


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_down_stage_train_and_sgd(be, dt):
    """ResStageTrain.from_params on a synthetic res2 (a 64 -> 128 down block, then an identity block; B 1, 3 x 38 -> 19): all gradient names;
    it equals the stage built from the two classes by hand; after SGD.attach(stage), step(), the next forward runs on the new weights --
    the down block's z2 changes and is the strided conv of its y1 with the updated master, and the whole forward equals, bit for bit,
    that of a fresh stage built from the downloaded masters and vectors"""
    from rangedet_amd.backbone_train import BasicBlockTrain, DownBlockTrain, ResStageTrain
    from rangedet_amd.optim import SGD
    A = be.alloc
    B, H, Win = 1, 3, 38
    arg, aux, ps = stage_params("res2", 64, 128, 2, 2500)
    stage = ResStageTrain.from_params("res2", arg, aux, 2, stride=(1, 2), dtype=dt, lib=be.lib, alloc=A)
    assert [type(b) for b in stage.blocks] == [DownBlockTrain, BasicBlockTrain] and [b.name for b in stage.blocks] == ["res2_unit1", "res2_unit2"]
    flat = ResStageTrain.from_params("res2", arg, aux, 2, dtype=dt, lib=be.lib, alloc=A)
    assert [type(b) for b in flat.blocks] == [BasicBlockTrain, BasicBlockTrain] and flat.blocks[0].proj and not flat.blocks[1].proj
    x = dev16(be, to_bits(rnd("relu", (B, H, Win, 64), dt, 2501), dt), dt)
    g = dev16(be, to_bits(rnd("normal", (B, H, Win // 2, 128), dt, 2502), dt), dt)
    opt = SGD(lr=0.05, lib=be.lib, alloc=A)
    opt.attach(stage)
    y0 = vals16(be, stage.forward(x), dt).copy()
    z2_0 = vals16(be, stage.blocks[0].z2, dt).copy()
    dx, grads = stage.backward(g)
    A.sync()
    hand = ResStageTrain([make_down(be, dt, ps[0]), TB.make_block(be, dt, ps[1])])
    assert vals16(be, hand.forward(x), dt).tobytes() == y0.tobytes()
    names = ["res2_unit%d_%s" % (u, s) for u in (1, 2) for s in ("conv1_weight", "bn1_gamma", "bn1_beta", "conv2_weight", "bn2_gamma", "bn2_beta")]
    names += ["res2_unit1_%s" % s for s in ("sc_weight", "sc_bn_gamma", "sc_bn_beta")]
    assert sorted(grads) == sorted(names) and sorted(opt.state()) == sorted(names)
    assert tuple(dx.shape) == (B, H, Win, 64) and all(np.isfinite(np.array(A.to_numpy(v))).all() and np.array(A.to_numpy(v)).any() for v in grads.values())
    assert vals16(be, stage.blocks[0].g, dt).tobytes() == vals16(be, stage.blocks[1].dx, dt).tobytes()
    before = [TB.host_params(A, b, p) for b, p in zip(stage.blocks, ps)]
    opt.step()
    y1 = vals16(be, stage.forward(x), dt).copy()
    A.sync()
    after = [TB.host_params(A, b, p) for b, p in zip(stage.blocks, ps)]
    for q0, q1 in zip(before, after):
        for k in ("conv1_w", "conv2_w") + (("sc_w",) if "sc_w" in q0 else ()):
            assert (q0[k] != q1[k]).mean() > 0.9, k
    blk = stage.blocks[0]
    z2_1, y1_1 = vals16(be, blk.z2, dt), vals16(be, blk.y1, dt)
    assert (z2_1 != z2_0).mean() > 0.3 and (y1 != y0).mean() > 0.3
    close(z2_1, DM.conv3_s2(y1_1, CM.h16_round(after[0]["conv2_w"], dt)), dt, "z2 after the step %s" % be.name)
    fresh = ResStageTrain([make_down(be, dt, after[0]), TB.make_block(be, dt, after[1])])
    yf = vals16(be, fresh.forward(x), dt)
    assert yf.tobytes() == y1.tobytes(), int((yf != y1).sum())
    # the data-gradient images were re-packed too: the two stages' backward agree in every bit
    dxs, _ = stage.backward(g)
    dxf, _ = fresh.backward(g)
    A.sync()
    assert vals16(be, dxs, dt).tobytes() == vals16(be, dxf, dt).tobytes()


# ---- the formulas --------------------------------------------------------------------------------------------------------------------------------
def test_model_down_block_matches_autograd():
    """CPU only, no library: down_block_model.block_backward against torch float64 autograd on conv2d (stride (1, 2) for conv2 and the
    shortcut), batch_norm(training=True), add, relu with a linear loss on top, to 1e-9 of the largest value of each gradient.  No
    pre-activation of either ReLU lies within 1e-6 of zero, so no mask can tie."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(2601)
    B, H, Win, cin, cout = 2, 4, 6, 5, 7
    x = rng.standard_normal((B, H, Win, cin))
    w1, w2 = rng.standard_normal((cout, cin, 3, 3)) / 7, rng.standard_normal((cout, cout, 3, 3)) / 7
    bns = [(rng.uniform(0.5, 1.5, cout), rng.normal(0, 0.3, cout)) for _ in range(3)]
    ws = rng.standard_normal((cout, cin)) / 2
    lin = rng.standard_normal((B, H, Win // 2, cout))
    arrs = dict(x=x.transpose(0, 3, 1, 2), w1=w1, w2=w2, g1=bns[0][0], b1=bns[0][1], g2=bns[1][0], b2=bns[1][1], ws=ws.reshape(cout, cin, 1, 1),
                gs=bns[2][0], bs=bns[2][1])
    t = {k: torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, requires_grad=True) for k, v in arrs.items()}
    y1 = F.relu(F.batch_norm(F.conv2d(t["x"], t["w1"], padding=1), None, None, t["g1"], t["b1"], training=True, eps=EPS))
    main = F.batch_norm(F.conv2d(y1, t["w2"], padding=1, stride=(1, 2)), None, None, t["g2"], t["b2"], training=True, eps=EPS)
    short = F.batch_norm(F.conv2d(t["x"], t["ws"], stride=(1, 2)), None, None, t["gs"], t["bs"], training=True, eps=EPS)
    y = F.relu(main + short)
    (y * torch.tensor(lin.transpose(0, 3, 1, 2))).sum().backward()
    m = DM.block_backward(x, w1, bns[0], w2, bns[1], EPS, lin, ws, bns[2])
    assert float(np.abs(m["pre"]).min()) > 1e-6, "a pre-activation within 1e-6 of zero: choose another seed"
    pairs = [("y", m["y"], y.detach().numpy().transpose(0, 2, 3, 1)), ("dx", m["dx"], t["x"].grad.numpy().transpose(0, 2, 3, 1)),
             ("conv1_weight", m["conv1_weight"], t["w1"].grad.numpy()), ("conv2_weight", m["conv2_weight"], t["w2"].grad.numpy()),
             ("bn1_gamma", m["bn1_gamma"], t["g1"].grad.numpy()), ("bn1_beta", m["bn1_beta"], t["b1"].grad.numpy()),
             ("bn2_gamma", m["bn2_gamma"], t["g2"].grad.numpy()), ("bn2_beta", m["bn2_beta"], t["b2"].grad.numpy()),
             ("sc_weight", m["sc_weight"], t["ws"].grad.numpy().reshape(cout, cin)), ("sc_bn_gamma", m["sc_bn_gamma"], t["gs"].grad.numpy()),
             ("sc_bn_beta", m["sc_bn_beta"], t["bs"].grad.numpy())]
    for name, got, want in pairs:
        rel = float(np.abs(got - want).max() / np.abs(want).max())
        print(name, "relative difference %.3g" % rel)
        assert rel < 1e-9, (name, rel)
    assert 0.3 < float((m["y"] == 0).mean()) < 0.7

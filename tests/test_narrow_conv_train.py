"""The weight gradient of the convs that read the range image (csrc/k_convbwd_narrow.h: rd_conv_bwd_weight_narrow, and the concat form
rd_conv3x3_bwd_weight_cat) against tests/convbwd_model.py, through the C ABI: every output buffer and the workspace are pre-filled with
0xFF bytes and carry a guard tail; the tail and every element outside the written channels must be unchanged afterwards.  The x image
is a 16-channel slot of which the first cin channels belong to the conv; the others hold a finite non-zero pattern (train_util.image)
and must reach no written element.

Tolerances, u = 2^-24, n = the terms of a sum (convbwd_model.tap_terms):
  exact inputs     x, dz integers in -3 .. 3: every partial sum in any order is an integer below 2^24 -> equal to the float64 model in
                   every bit (-0 and +0 taken as equal)
  random inputs    normal values, and ReLU-sparse x with 40 - 60 % zeros (asserted): |got - want| <= 2 n u sum |terms| per element
  determinism      two calls on 0xFF-filled outputs and workspace give identical bytes
Then the device packers of these convs (rd_pack_conv_narrow_dev, rd_pack_conv3x3_cat_dev: byte-equal to the host packers over a 0xFF
pre-fill, zero tail included), the two pack= forms of rangedet_amd.optim.SGD, and the two classes built on them --
rangedet_amd.backbone_train.StemBlockTrain and rangedet_amd.backward.Level0TowerTrain -- each step against the model fed the kernels' own
inputs to that step, in the pattern of test_basic_block_train.py and test_batch_norm.py, whose helpers are imported unchanged.
"""
import numpy as np
import pytest

import block_model as BM
import conv_model as CM
import convbwd_model as M
import norm_model as N
import optim_model as OM
import test_basic_block_train as TB
import test_batch_norm as TBN
from conftest import BOTH, HIP_ONLY
from rangedet_amd import lib as R
from test_optimizer import poke
from train_util import DTS, back, check_hob, check_wgrad, dev16, ff, image, rnd, same_bits, to_bits, vals16

F32 = np.float32
EPS, MOM = TB.EPS, TB.MOM
PT, RH = 64, 16        # the narrow weight-gradient kernel's pixel tile and row strip (k_convbwd_narrow.h NW_PT, NW_RH)
SLOT = 16              # channels of the range-image slot the kernel reads (NW_SLOT)


def model(x, dz, ksize, want_abs):
    """-> dW (cout, cin, k, k) float64, sum |terms| (or None), terms per tap (k, k)"""
    want, sabs, n = M.weight_grad(x, dz, want_abs=want_abs)
    if ksize == 1:
        return want[:, :, 1:2, 1:2], None if sabs is None else sabs[:, :, 1:2, 1:2], n[1:2, 1:2]
    return want, sabs, n


def check(got, x, dz, ksize, exact, what):
    want, sabs, n = model(x, dz, ksize, not exact)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    if exact:
        bad = int((got != want.astype(np.float32)).sum())
        print(what, "exact: elements that differ", bad)
        assert same_bits(got, want), (what, bad)
        return
    bound = M.sum_bound(n[None, None], sabs)
    err = np.abs(got.astype(np.float64) - want)
    assert (err[bound == 0] == 0).all(), what
    worst = float((err[bound > 0] / bound[bound > 0]).max())
    print(what, "worst err / bound %.3g" % worst)
    assert worst <= 1, (what, worst)


def take_dw(be, buf, cout, dcs, dco, cin, ksize, what):
    """the written channels of a 0xFF-prefilled (cout, dcs, k, k) float32 gradient; everything else and the guard must be untouched"""
    T = ksize * ksize
    raw = back(be, buf, cout * dcs * T * 4, what).view(np.uint32).reshape(cout, dcs, T)
    outside = np.ones(dcs, bool)
    outside[dco:dco + cin] = False
    assert (raw[:, outside] == 0xFFFFFFFF).all(), "%s: channels outside [off, off + cin) written" % what
    return raw[:, dco:dco + cin].copy().view(np.float32).reshape(cout, cin, ksize, ksize)


def run_narrow(be, dt, x, dz, ksize, xcs=SLOT, xco=0, zcs=None, zco=0, dcs=None, dco=0, split=0, twice=False):
    L = be.lib
    B, H, W, cin = x.shape
    cout, T = dz.shape[3], ksize * ksize
    dcs = dcs or cin
    nws = L.raw("rd_conv_bwd_weight_narrow_workspace_bytes")(B, H, W, cin, cout, ksize, split)
    assert nws > 0 and nws % (4 * T * cin * cout) == 0
    xd, zd = be.up(image(x, dt, xcs, xco)), be.up(image(dz, dt, zcs, zco))
    outs = []
    for _ in range(2 if twice else 1):
        dW, ws = ff(be, cout * dcs * T * 4), ff(be, nws)
        L.call("rd_conv_bwd_weight_narrow", be.ptr(xd), xcs, xco, be.ptr(zd), zcs or cout, zco, be.ptr(dW), dcs, dco, B, H, W, cin, cout, ksize,
               split, dt, be.ptr(ws), nws, be.stream)
        back(be, ws, nws, "workspace")
        outs.append(take_dw(be, dW, cout, dcs, dco, cin, ksize, "dW"))
    if twice:
        assert outs[0].tobytes() == outs[1].tobytes(), "two calls differ"
    return outs[0], nws // (4 * T * cin * cout)


KINDS = (("normal", "normal", False), ("relu", "normal", False), ("ints", "ints", True))


def narrow_case(be, dt, shape, cin, cout, ksize, what, kinds=KINDS, **kw):
    B, H, W = shape
    for kind, zkind, exact in kinds:
        x, dz = rnd(kind, (B, H, W, cin), dt, 111), rnd(zkind, (B, H, W, cout), dt, 112)
        if kind == "relu":
            assert 0.4 < (x == 0).mean() < 0.6
        got, _ = run_narrow(be, dt, x, dz, ksize, **kw)
        check(got, x, dz, ksize, exact, "%s k%d %s %s" % (what, ksize, kind, be.name))


# ---- 1. channel pairs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ksize", [3, 1])
@pytest.mark.parametrize("cin,cout", [(5, 64), (8, 64), (16, 64), (5, 128), (8, 128), (16, 128)])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_narrow_channel_pairs(be, dt, cin, cout, ksize):
    """B 2, 3 x 37: the top and the bottom row, an interior row, a width that fills no pixel tile; two partial sums.  The slot channels at
    or above cin hold the non-zero pattern of train_util.image."""
    narrow_case(be, dt, (2, 3, 37), cin, cout, ksize, "2x3x37 %d->%d" % (cin, cout))


# ---- 2. edge shapes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ksize", [3, 1])
@pytest.mark.parametrize("shape", [(2, 1, 37), (2, 3, 1), (1, 2, PT - 1), (1, 2, PT), (1, 2, PT + 1), (1, RH, 9), (1, RH + 1, 9)],
                         ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_narrow_edge_shapes(be, dt, shape, ksize):
    """one row, one column, a width one below, at and one above the pixel tile, RH rows and RH + 1 (the second strip starts on real data
    above it); exact inputs"""
    narrow_case(be, dt, shape, 8, 64, ksize, "%dx%dx%d" % shape, kinds=KINDS[2:])


# ---- 3. every tap has its edge terms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_narrow_every_tap_has_its_edge_terms(be, dt):
    """x = dz = 1: the dW of tap (dh, dw) is the number of its terms, B (H - |dh|) (W - |dw|) -- fewer than B H W off the centre, asserted
    per tap; ksize 1: B H W"""
    B, H, W = 2, 3, 37
    x, dz = np.ones((B, H, W, 8), np.float32), np.ones((B, H, W, 64), np.float32)
    got, _ = run_narrow(be, dt, x, dz, 3, twice=True)
    n = M.tap_terms(B, H, W)
    for i in range(3):
        for j in range(3):
            assert (i, j) == (1, 1) or n[i, j] < B * H * W
            assert (got[:, :, i, j] == n[i, j]).all(), ("tap", i - 1, j - 1, np.unique(got[:, :, i, j]), n[i, j])
    got, _ = run_narrow(be, dt, x, dz, 1, twice=True)
    assert (got == B * H * W).all(), np.unique(got)


# ---- 4. strides and offsets -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ksize", [3, 1])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_narrow_strides_and_offsets(be, dt, ksize):
    """x: the slot at offset 8 of 24; dz: 64 channels at offset 16 of 88; dW written at dw_cin_off 64 of dw_cin_stride 72 -- every byte
    outside the written channels and the guard tail stays 0xFF (take_dw)"""
    narrow_case(be, dt, (2, 3, 37), 8, 64, ksize, "2x3x37 strided", xcs=24, xco=8, zcs=88, zco=16, dcs=72, dco=64)


# ---- 5. split -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ksize", [3, 1])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_narrow_reduction_split(be, dt, ksize):
    """B 2, 17 x 70: two row strips times two pixel tiles = 8 chunks.  split 3: runs of 2, 3 and 3 chunks per workgroup (8 does not divide
    by 3); the library's own split: one chunk each; split 1: one sum.  Exact inputs: all three equal the model in every bit; the workspace
    size is that of the partial count; two calls give the same bytes.  Random inputs within the bound."""
    shape, cin, cout = (2, 17, 70), 8, 64
    x, dz = rnd("ints", shape + (cin,), dt, 121), rnd("ints", shape + (cout,), dt, 122)
    for split, parts in ((3, 3), (0, 8), (1, 1)):
        got, S = run_narrow(be, dt, x, dz, ksize, split=split, twice=True)
        assert S == parts
        check(got, x, dz, ksize, True, "2x17x70 k%d split %d %s" % (ksize, split, be.name))
    x, dz = rnd("relu", shape + (cin,), dt, 123), rnd("normal", shape + (cout,), dt, 124)
    check(run_narrow(be, dt, x, dz, ksize, split=3)[0], x, dz, ksize, False, "2x17x70 k%d split 3 random %s" % (ksize, be.name))


# ---- 6. one larger case -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
def test_narrow_many_splits_exact(be, dt):
    """B 2, 64 x 332, 8 -> 128, exact inputs: 48 chunks, 48 partial sums per element, twice"""
    x, dz = rnd("ints", (2, 64, 332, 8), dt, 141), rnd("ints", (2, 64, 332, 128), dt, 142)
    got, S = run_narrow(be, dt, x, dz, 3, twice=True)
    assert S == 2 * 4 * 6
    check(got, x, dz, 3, True, "2x64x332 8->128")


# ---- 7. the concat conv -------------------------------------------------------------------------------------------------------------------
def run_wide(be, dt, x, dz, split):
    """rd_conv3x3_bwd_weight on dense tensors -> dW (cout, cin, 3, 3)"""
    L = be.lib
    B, H, W, cin = x.shape
    cout = dz.shape[3]
    nws = L.raw("rd_conv3x3_bwd_weight_workspace_bytes")(B, H, W, cin, cout, split)
    dW, ws = ff(be, cout * cin * 36), ff(be, nws)
    L.call("rd_conv3x3_bwd_weight", be.ptr(be.up(image(x, dt))), cin, 0, be.ptr(be.up(image(dz, dt))), cout, 0, be.ptr(dW), B, H, W, cin, cout, split,
           dt, be.ptr(ws), nws, be.stream)
    return back(be, dW, cout * cin * 36, "dW wide").view(np.float32).reshape(cout, cin, 3, 3).copy()


def run_cat(be, dt, x1, x2, dz, split=0, twice=False):
    L = be.lib
    B, H, W, cin1 = x1.shape
    cin2, cout = x2.shape[3], dz.shape[3]
    nws = L.raw("rd_conv3x3_bwd_weight_cat_workspace_bytes")(B, H, W, cin1, cin2, cout, split)
    assert nws == (L.raw("rd_conv3x3_bwd_weight_workspace_bytes")(B, H, W, cin1, cout, split)
                   + L.raw("rd_conv_bwd_weight_narrow_workspace_bytes")(B, H, W, cin2, cout, 3, split))
    x1d, x2d, zd = be.up(image(x1, dt)), be.up(image(x2, dt, SLOT, 0)), be.up(image(dz, dt))
    outs = []
    for _ in range(2 if twice else 1):
        dW, ws = ff(be, cout * (cin1 + cin2) * 36), ff(be, nws)
        L.call("rd_conv3x3_bwd_weight_cat", be.ptr(x1d), cin1, 0, cin1, be.ptr(x2d), SLOT, 0, cin2, be.ptr(zd), cout, 0, be.ptr(dW), B, H, W, cout,
               split, dt, be.ptr(ws), nws, be.stream)
        back(be, ws, nws, "workspace")
        outs.append(back(be, dW, cout * (cin1 + cin2) * 36, "dW cat").view(np.float32).reshape(cout, cin1 + cin2, 3, 3).copy())
    if twice:
        assert outs[0].tobytes() == outs[1].tobytes(), "two calls differ"
    return outs[0]


@pytest.mark.parametrize("cin2", [8, 16])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_cat_weight_grad(be, dt, cin2):
    """64 + cin2 -> 128 at B 2, 3 x 37: channels [0, 64) byte-equal to rd_conv3x3_bwd_weight on (x1, dz) with the same split, the others
    byte-equal to the narrow call; exact inputs: the whole gradient equals the model on the concatenated input in every bit"""
    shape, cout = (2, 3, 37), 128
    for kind, zkind, exact in KINDS[1:]:
        x1, x2 = rnd(kind, shape + (64,), dt, 151), rnd(kind, shape + (cin2,), dt, 152)
        dz = rnd(zkind, shape + (cout,), dt, 153)
        for split in (0, 1):
            got = run_cat(be, dt, x1, x2, dz, split=split, twice=True)
            assert got[:, :64].tobytes() == run_wide(be, dt, x1, dz, split).tobytes(), (kind, split)
            assert got[:, 64:].tobytes() == run_narrow(be, dt, x2, dz, 3, split=split)[0].tobytes(), (kind, split)
            check(got, np.concatenate([x1, x2], 3), dz, 3, exact, "cat 64+%d split %d %s %s" % (cin2, split, kind, be.name))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_cat_weight_grad_padded_stride(be, dt):
    """rd_conv3x3_bwd_weight_cat_padded, 64 + 5 -> 128 into a gradient of channel stride 72 at B 2, 3 x 37: channels [0, 69) byte-equal to
    rd_conv3x3_bwd_weight_cat, channels 69 .. 71 and the guard tail still 0xFF; a stride below 69 is refused"""
    L = be.lib
    shape, cout, cin2, cs = (2, 3, 37), 128, 5, 72
    x1, x2, dz = rnd("relu", shape + (64,), dt, 155), rnd("ints", shape + (cin2,), dt, 156), rnd("ints", shape + (cout,), dt, 157)
    want = run_cat(be, dt, x1, x2, dz)
    B, H, W = shape
    nws = L.raw("rd_conv3x3_bwd_weight_cat_workspace_bytes")(B, H, W, 64, cin2, cout, 0)
    x1d, x2d, zd = be.up(image(x1, dt)), be.up(image(x2, dt, SLOT, 0)), be.up(image(dz, dt))
    dW, ws = ff(be, cout * cs * 36), ff(be, nws)
    args = (be.ptr(x1d), 64, 0, 64, be.ptr(x2d), SLOT, 0, cin2, be.ptr(zd), cout, 0, be.ptr(dW))
    tail = (B, H, W, cout, 0, dt, be.ptr(ws), nws, be.stream)
    assert L.raw("rd_conv3x3_bwd_weight_cat_padded")(*args, 68, *tail) == R.RD_ESHAPE
    assert (back(be, dW, cout * cs * 36, "dW") == 0xFF).all()
    L.call("rd_conv3x3_bwd_weight_cat_padded", *args, cs, *tail)
    raw = back(be, dW, cout * cs * 36, "dW padded").view(np.uint32).reshape(cout, cs, 9)
    assert (raw[:, 64 + cin2:] == 0xFFFFFFFF).all(), "a padding column was written"
    assert raw[:, :64 + cin2].copy().view(np.float32).reshape(cout, 64 + cin2, 3, 3).tobytes() == want.tobytes()


# ---- the Python steps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_tower_ops_steps(be, dt):
    """TowerOps.weight_grad_narrow (ksize 3 and 1) and weight_grad_cat at B 1, 2 x 9 with c = 5, integer inputs: equal to the model in every
    bit, in the reference's shapes"""
    from rangedet_amd.backward import TowerOps
    o = TowerOps(dtype=dt, lib=be.lib, alloc=be.alloc)
    B, H, W, c = 1, 2, 9, 5
    xv, x1v, zv = rnd("ints", (B, H, W, c), dt, 161), rnd("ints", (B, H, W, 64), dt, 162), rnd("ints", (B, H, W, 128), dt, 163)
    slot = dev16(be, image(xv, dt, SLOT, 0), dt)
    x1, dz = dev16(be, to_bits(x1v, dt), dt), dev16(be, to_bits(zv, dt), dt)
    for ksize in (3, 1):
        dW = o.weight_grad_narrow(slot, dz, c, ksize)
        be.alloc.sync()
        got = np.array(be.alloc.to_numpy(dW))
        assert got.shape == (128, c, ksize, ksize)
        check(got, xv, zv, ksize, True, "TowerOps narrow k%d" % ksize)
    dW = o.weight_grad_cat(x1, slot, c, dz)
    be.alloc.sync()
    got = np.array(be.alloc.to_numpy(dW))
    assert got.shape == (128, 64 + c, 3, 3)
    check(got, np.concatenate([x1v, xv], 3), zv, 3, True, "TowerOps cat")
    with pytest.raises(NotImplementedError, match="slot"):
        o.weight_grad_narrow(x1, dz, 8, 3)
    with pytest.raises(NotImplementedError, match="slot"):
        o.weight_grad_cat(x1, slot, 17, dz)


# ---- 11. refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_narrow_status_codes(be):
    """cin 0 and 17, ksize 2, cout 32, a slot that runs past the channel stride, cin1 != 64, null and unaligned pointers, a workspace one
    byte short, a float32 dtype: each its code, the message set, nothing launched (one zeroed buffer stands for every device pointer and
    stays zero)"""
    L = be.lib
    buf = be.empty(1 << 20)
    p = be.ptr(buf)
    assert p % 16 == 0
    BF = R.RD_BF16
    wn, wc = L.raw("rd_conv_bwd_weight_narrow_workspace_bytes"), L.raw("rd_conv3x3_bwd_weight_cat_workspace_bytes")

    def narrow(x=p, dz=p, dW=p, ws=p, cin=8, cout=64, ksize=3, B=1, H=2, W=8, xcs=16, xco=0, dcs=None, dco=0, split=0, dt=BF, nws=None):
        need = wn(1, 2, 8, 8, 64, 3, split) if nws is None else nws
        return L.raw("rd_conv_bwd_weight_narrow")(x, xcs, xco, dz, cout, 0, dW, dcs or cin, dco, B, H, W, cin, cout, ksize, split, dt, ws, need,
                                                  be.stream)

    def cat(x1=p, x2=p, dz=p, dW=p, ws=p, cin1=64, cin2=8, cout=128, B=1, H=2, W=8, x2cs=16, x2co=0, split=0, dt=BF, nws=None):
        need = wc(1, 2, 8, 64, 8, 128, split) if nws is None else nws
        return L.raw("rd_conv3x3_bwd_weight_cat")(x1, cin1, 0, cin1, x2, x2cs, x2co, cin2, dz, cout, 0, dW, B, H, W, cout, split, dt, ws, need,
                                                  be.stream)
    assert wn(1, 2, 8, 8, 64, 3, 0) == 4 * 9 * 64 * 8 and wn(1, 2, 8, 8, 64, 1, 0) == 4 * 64 * 8 and wn(4, 64, 128, 5, 128, 3, 5) == 5 * 4 * 9 * 128 * 5
    assert wn(1, 2, 8, 0, 64, 3, 0) == 0 and wn(1, 2, 8, 17, 64, 3, 0) == 0 and wn(1, 2, 8, 8, 32, 3, 0) == 0 and wn(1, 2, 8, 8, 64, 2, 0) == 0
    assert wn(0, 2, 8, 8, 64, 3, 0) == 0 and wc(1, 2, 8, 128, 8, 128, 0) == 0 and wc(1, 2, 8, 64, 17, 128, 0) == 0
    for kw in (dict(cin=0), dict(cin=17), dict(ksize=2), dict(ksize=5), dict(cout=32), dict(B=0), dict(H=0), dict(W=0), dict(xcs=16, xco=8),
               dict(xcs=24, xco=4), dict(xcs=20), dict(dcs=4), dict(dcs=72, dco=65)):
        assert narrow(**kw) == R.RD_ESHAPE, kw
        assert L.rd_last_error_string().decode().startswith("conv_bwd_weight_narrow")
    for kw in (dict(cin1=128), dict(cin1=32), dict(cin2=0), dict(cin2=17), dict(cout=32), dict(B=0), dict(x2cs=16, x2co=8)):
        assert cat(**kw) == R.RD_ESHAPE, kw
        assert L.rd_last_error_string().decode().startswith("conv3x3_bwd_weight_cat")
    for name in ("x", "dz", "dW", "ws"):
        assert narrow(**{name: None}) == R.RD_EINVAL and "null" in L.rd_last_error_string().decode(), name
    for name in ("x1", "x2", "dz", "dW", "ws"):
        assert cat(**{name: None}) == R.RD_EINVAL and "null" in L.rd_last_error_string().decode(), name
    assert narrow(dt=R.RD_F32) == R.RD_EINVAL and cat(dt=R.RD_F32) == R.RD_EINVAL
    assert narrow(split=-1, nws=1 << 20) == R.RD_EINVAL and cat(split=-1, nws=1 << 20) == R.RD_EINVAL
    assert narrow(nws=wn(1, 2, 8, 8, 64, 3, 0) - 1) == R.RD_EWORKSPACE and "workspace" in L.rd_last_error_string().decode()
    assert cat(nws=wc(1, 2, 8, 64, 8, 128, 0) - 1) == R.RD_EWORKSPACE and "workspace" in L.rd_last_error_string().decode()
    for rc in (narrow(x=p + 8), narrow(dz=p + 8), cat(x1=p + 8), cat(x2=p + 8)):
        assert rc == R.RD_EINVAL and "aligned" in L.rd_last_error_string().decode()
    assert not be.down(buf, np.uint8, (1 << 20,)).any()           # nothing ran


# ---- 8. device packers ------------------------------------------------------------------------------------------------------------------
def packed(be, call, want, *args):
    """one device packer launch over a 0xFF pre-fill -> the buffer; byte-equal to the host image `want`, zero tail included"""
    out = ff(be, want.size)
    be.lib.call(call, *args, be.ptr(out), be.stream)
    got = back(be, out, want.size, call)
    assert int((got != want).sum()) == 0 and not got[-256:].any(), (call, args[2:], int((got != want).sum()))
    return out


@pytest.mark.parametrize("cout", [64, 128])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_device_packers(be, dt, cout):
    """every row of the header's table: narrow ksize 3 (with a fold scale and without: the host packer then takes ones) and ksize 1 at cin
    5, 8, 16; the concat forward image (likewise) and its data-gradient image at cin2 8, 16 -- on weights that sit on exact rounding ties
    of the type and on normal ones; the masters are not written"""
    L = be.lib
    rng = np.random.default_rng(1900 + cout)
    fold, ones = rng.uniform(0.5, 1.5, cout).astype(F32), np.ones(cout, F32)
    foldd = TB.fup(be, fold)
    for cin in (5, 8, 16):
        for ksize in (3, 1):
            shape = (cout, cin, ksize, ksize)
            for w in (OM.tie_values(shape, dt, rng, dt == R.RD_BF16), rng.standard_normal(shape).astype(F32)):
                wd = TB.fup(be, w)
                if ksize == 1:
                    want = L.pack_conv_weight(w, dt)
                    assert want.size == L.cdll.rd_conv_packed_bytes(1, cin, cout, dt)
                    packed(be, "rd_pack_conv_narrow_dev", want, be.ptr(wd), None, cout, cin, 1, dt)
                else:
                    for fs, fh in ((None, ones), (foldd, fold)):
                        want = L.pack_conv3x3_ex(w, 1, cin, fold_scale=fh, dtype=dt)
                        assert want.size == L.cdll.rd_conv3x3_ex_packed_bytes(cin, cout, 1, cin)
                        packed(be, "rd_pack_conv_narrow_dev", want, be.ptr(wd), be.ptr(fs), cout, cin, 3, dt)
                assert back(be, wd, w.nbytes, "w").tobytes() == w.tobytes()
    for cin2 in (8, 16):
        shape = (cout, 64 + cin2, 3, 3)
        for w in (OM.tie_values(shape, dt, rng, dt == R.RD_BF16), rng.standard_normal(shape).astype(F32)):
            wd = TB.fup(be, w)
            for fs, fh in ((None, ones), (foldd, fold)):
                want = L.pack_conv3x3_cat(w, 64, cin2, fold_scale=fh, dtype=dt)
                packed(be, "rd_pack_conv3x3_cat_dev", want, be.ptr(wd), be.ptr(fs), cout, 64, cin2, 0, dt)
            want = L.pack_conv3x3_ex(OM.flip_weight(w[:, :64]), 1, cout, fold_scale=None, dtype=dt)
            packed(be, "rd_pack_conv3x3_cat_dev", want, be.ptr(wd), None, cout, 64, cin2, 1, dt)
            assert back(be, wd, w.nbytes, "w").tobytes() == w.tobytes()
    # c = 5 of the concat's data-gradient image: cin2 only sets the master's channel stride there
    w = rng.standard_normal((cout, 69, 3, 3)).astype(F32)
    want = L.pack_conv3x3_ex(OM.flip_weight(w[:, :64]), 1, cout, fold_scale=None, dtype=dt)
    packed(be, "rd_pack_conv3x3_cat_dev", want, be.ptr(TB.fup(be, w)), None, cout, 64, 5, 1, dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_forward_on_device_packed_images(be, dt):
    """a forward launch on the device-packed image is bit-equal to one on the host-packed image: the narrow 3x3 and 1x1 convs at c = 5, the
    concat conv at 64 + 8, its data gradient (B 1, 3 x 9)"""
    from rangedet_amd.backward import TowerOps
    L, A = be.lib, be.alloc
    o = TowerOps(dtype=dt, lib=L, alloc=A)
    rng = np.random.default_rng(1950)
    B, H, W, c = 1, 3, 9, 5
    slot = dev16(be, image(rnd("normal", (B, H, W, c), dt, 1951), dt, SLOT, 0), dt)
    x1 = dev16(be, to_bits(rnd("relu", (B, H, W, 64), dt, 1952), dt), dt)
    dz = dev16(be, to_bits(rnd("normal", (B, H, W, 128), dt, 1953), dt), dt)

    def dev_image(call, nbytes, *args):
        out = ff(be, nbytes)
        L.call(call, *args, be.ptr(out), be.stream)
        return out
    w3 = (rng.standard_normal((64, c, 3, 3)) / 4).astype(F32)
    host = o.pack_narrow(w3, 3)
    mine = dev_image("rd_pack_conv_narrow_dev", L.cdll.rd_conv3x3_ex_packed_bytes(c, 64, 1, c), be.ptr(TB.fup(be, w3)), None, 64, c, 3, dt)
    want = vals16(be, o.conv_unscaled(slot, host, c, 64, x_cs=SLOT), dt).copy()
    assert np.abs(want).max() > 0 and vals16(be, o.conv_unscaled(slot, (mine, host[1]), c, 64, x_cs=SLOT), dt).tobytes() == want.tobytes()
    ref = CM.conv_ref64(rnd("normal", (B, H, W, c), dt, 1951).transpose(0, 3, 1, 2), w3, dt, fold=True).transpose(0, 2, 3, 1)
    assert CM.conv_check(want, ref, dt)[0] == 0              # the slot's pattern channels met zero weights only
    w1 = (rng.standard_normal((64, c, 1, 1)) / 2).astype(F32)
    mine = dev_image("rd_pack_conv_narrow_dev", L.cdll.rd_conv_packed_bytes(1, c, 64, dt), be.ptr(TB.fup(be, w1)), None, 64, c, 1, dt)
    want = vals16(be, o.conv1x1(slot, o.pack_narrow(w1, 1), c, 64, ("zs", 0), x_cs=SLOT), dt).copy()
    assert np.abs(want).max() > 0 and vals16(be, o.conv1x1(slot, mine, c, 64, ("zs", 0), x_cs=SLOT), dt).tobytes() == want.tobytes()
    wc = (rng.standard_normal((128, 72, 3, 3)) / 16).astype(F32)
    wcd = TB.fup(be, wc)
    slot8 = dev16(be, image(rnd("normal", (B, H, W, 8), dt, 1954), dt, SLOT, 0), dt)
    host = o.pack_cat(wc, 8)
    mine = dev_image("rd_pack_conv3x3_cat_dev", L.cdll.rd_conv3x3_cat_packed_bytes(64, 8, 128), be.ptr(wcd), None, 128, 64, 8, 0, dt)
    want = vals16(be, o.conv3x3_cat(x1, slot8, 8, host, 128), dt).copy()
    assert np.abs(want).max() > 0 and vals16(be, o.conv3x3_cat(x1, slot8, 8, (mine, host[1]), 128), dt).tobytes() == want.tobytes()
    host = o.pack_data_grad(wc[:, :64])
    mine = dev_image("rd_pack_conv3x3_cat_dev", L.cdll.rd_conv3x3_ex_packed_bytes(128, 64, 1, 128), be.ptr(wcd), None, 128, 64, 8, 1, dt)
    want = vals16(be, o.data_grad(dz, host), dt).copy()
    assert np.abs(want).max() > 0 and vals16(be, o.data_grad(dz, (mine, host[1], host[2])), dt).tobytes() == want.tobytes()


# ---- 9. optimizer -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_optimizer_narrow_and_cat_forms(be, dt):
    """a narrow 3x3 weight, a narrow 1x1 weight and a concat weight (with a fold scale) registered with the new pack= forms beside a bias:
    after two steps the masters and momenta are bit-equal to optim_model.sgd_step and every image is byte-equal to host packing of the
    stepped masters; the table was built once"""
    from rangedet_amd.optim import SGD
    A, L = be.alloc, be.lib
    rng = np.random.default_rng(2001)
    names = ["res1_unit1_conv1_weight", "res1_unit1_sc_weight", "rpn_cls_conv_0_lvl_0_weight", "rpn_cls_logit_lvl_0_bias"]
    shapes = [(64, 8, 3, 3), (64, 5, 1, 1), (128, 72, 3, 3), (7,)]
    w = [rng.standard_normal(s).astype(F32) for s in shapes]
    m = [np.zeros(s, F32) for s in shapes]
    fold = rng.uniform(0.5, 1.5, 128).astype(F32)
    foldd = TB.fup(be, fold)
    wdv, gdv = [TB.fup(be, v) for v in w], [TB.fup(be, np.zeros(s, F32)) for s in shapes]
    nimg = [L.cdll.rd_conv3x3_ex_packed_bytes(8, 64, 1, 8), L.cdll.rd_conv_packed_bytes(1, 5, 64, dt), L.cdll.rd_conv3x3_cat_packed_bytes(64, 8, 128),
            L.cdll.rd_conv3x3_ex_packed_bytes(128, 64, 1, 128)]
    img = [ff(be, nb) for nb in nimg]
    view = [(A.view_f32(wdv[i], s), A.view_f32(gdv[i], s)) for i, s in enumerate(shapes)]
    opt = SGD(lr=0.05, lib=L, alloc=A)
    opt.add(names[0], *view[0], pack=dict(narrow=3, fwd=img[0], dtype=dt))
    opt.add(names[1], *view[1], pack=dict(narrow=1, fwd=img[1], dtype=dt))
    opt.add(names[2], *view[2], pack=dict(cat=(64, 8), fwd=img[2], bwd=img[3], fold_scale=foldd, dtype=dt))
    opt.add(names[3], *view[3])
    for step in range(2):
        g = [(10 * rng.standard_normal(s)).astype(F32) for s in shapes]
        for i in range(4):
            poke(be, gdv[i], g[i])
        lr = opt.step()
        for i in range(4):
            w[i], m[i] = OM.sgd_step(w[i], g[i], m[i], lr, 0.9, 1e-5, 1.0, 35.0, 1.0, 0.0 if i == 3 else 1.0)
    A.sync()
    mom = opt.state()
    for i, s in enumerate(shapes):
        got_w = back(be, wdv[i], w[i].nbytes, "weight %d" % i).view(F32).reshape(s)
        assert got_w.tobytes() == w[i].tobytes(), ("weight", i, int((got_w != w[i]).sum()))
        assert np.array(A.to_numpy(mom[names[i]])).astype(F32).tobytes() == m[i].tobytes(), ("momentum", i)
    want = [L.pack_conv3x3_ex(w[0], 1, 8, fold_scale=np.ones(64, F32), dtype=dt), L.pack_conv_weight(w[1], dt),
            L.pack_conv3x3_cat(w[2], 64, 8, fold_scale=fold, dtype=dt), L.pack_conv3x3_ex(OM.flip_weight(w[2][:, :64]), 1, 128, fold_scale=None, dtype=dt)]
    for i in range(4):
        assert want[i].size == nimg[i]
        got = back(be, img[i], nimg[i], "image %d" % i)
        assert int((got != want[i]).sum()) == 0 and not got[-256:].any(), ("image", i, int((got != want[i]).sum()))
    assert opt.table_builds == 1
    with pytest.raises(NotImplementedError, match="narrow"):
        opt.add("x_weight", A.view_f32(wdv[2], shapes[2]), A.view_f32(gdv[2], shapes[2]), pack=dict(narrow=3, fwd=img[2], dtype=dt))
    with pytest.raises(NotImplementedError, match="cat"):
        opt.add("y_weight", *view[0], pack=dict(cat=(64, 8), fwd=img[0], dtype=dt))
    with pytest.raises(ValueError, match="fold scale"):
        opt.add("z_weight", *view[1], pack=dict(narrow=1, fwd=img[1], fold_scale=foldd, dtype=dt))


# ---- 10. StemBlockTrain and Level0TowerTrain ------------------------------------------------------------------------------------------------
def stem_params(c, seed):
    p = TB.block_params("res1_unit1", c, 64, True, seed)
    return p


def make_stem(be, dt, p):
    from rangedet_amd.backbone_train import StemBlockTrain
    return StemBlockTrain(p["name"], p["conv1_w"], p["conv2_w"], p["bn1"], p["bn2"], p["sc_w"], p["sc_bn"], dtype=dt, lib=be.lib, alloc=be.alloc)


@pytest.mark.parametrize("c", [8, 5])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_stem_block_train(be, dt, c):
    """res1_unit1 at B 2, 3 x 37 with c range-image channels in the 16-channel slot (the other slot channels hold a non-zero pattern):
    every kept tensor against the model fed the block's own previous tensors, the gradients under the reference's names and shapes, no dx;
    after SGD.attach + step() the next forward equals that of a fresh block built from the stepped masters in every bit"""
    from rangedet_amd.optim import SGD
    A = be.alloc
    B, H, W, C = 2, 3, 37, 64
    n, name = B * H * W, "res1_unit1"
    p = stem_params(c, 2100 + c)
    blk = make_stem(be, dt, p)
    xv = rnd("normal", (B, H, W, c), dt, 2101)
    x = dev16(be, image(xv, dt, SLOT, 0), dt)
    g = dev16(be, to_bits(rnd("normal", (B, H, W, C), dt, 2102), dt), dt)
    opt = SGD(lr=0.05, lib=be.lib, alloc=A)
    opt.attach(blk)
    blk.forward(x)
    dx, grads = blk.backward(g)
    A.sync()
    assert dx is None
    what = "stem c %d %s" % (c, be.name)
    nchw = TB.nchw
    z1, y1, z2, zs, yv = (vals16(be, v, dt) for v in (blk.z1, blk.y1, blk.z2, blk.zs, blk.y))
    y0 = yv.copy()
    TB.conv_close(z1, CM.conv_ref64(nchw(xv), p["conv1_w"], dt, fold=True), dt, what + " z1")
    vec = {key: TB.check_norm(be, A, z, blk.saved[key], p[key], n, C, dt, "%s %s" % (what, key)) for key, z in (("bn1", z1), ("bn2", z2), ("sc_bn", zs))}
    a1, b1 = vec["bn1"][3:]
    assert same_bits(y1, N.affine_relu_f32(z1, a1, b1, dt)) and 0.2 < (y1 == 0).mean() < 0.8
    TB.conv_close(z2, CM.conv_ref64(nchw(y1), p["conv2_w"], dt, fold=True), dt, what + " z2")
    TB.conv_close(zs, CM.conv_ref64(nchw(xv), p["sc_w"], dt), dt, what + " zs")
    a2, b2 = vec["bn2"][3:]
    ars, brs = vec["sc_bn"][3:]
    assert same_bits(yv, BM.add_relu_f32(z2, a2, b2, zs, ars, brs, dt)) and 0.2 < (yv == 0).mean() < 0.8
    want_names = ["%s_%s" % (name, s) for s in ("conv1_weight", "bn1_gamma", "bn1_beta", "conv2_weight", "bn2_gamma", "bn2_beta", "sc_weight",
                                                "sc_bn_gamma", "sc_bn_beta")]
    assert sorted(grads) == sorted(want_names) and sorted(opt.state()) == sorted(want_names)
    gr = {k[len(name) + 1:]: np.array(A.to_numpy(v)) for k, v in grads.items()}
    assert gr["conv1_weight"].shape == (C, c, 3, 3) and gr["sc_weight"].shape == (C, c, 1, 1) and gr["conv2_weight"].shape == (C, C, 3, 3)
    gv, dz2, dr, g1, dz1 = (vals16(be, v, dt) for v in (blk.g, blk.dz2, blk.dr, blk.g1, blk.dz1))
    main = (a2, b2) + vec["bn2"][0:1] + vec["bn2"][2:3] + (p["bn2"]["gamma"],)
    sc = (ars, brs, vec["sc_bn"][0], vec["sc_bn"][2], p["sc_bn"]["gamma"])
    got = (dz2, dr, gr["bn2_gamma"], gr["bn2_beta"], gr["sc_bn_gamma"], gr["sc_bn_beta"])
    assert 0.2 < TB.check_add_bwd(got, gv, z2, zs, main, sc, dt, False, what + " bn2") < 0.8
    check_wgrad(gr["conv2_weight"], y1, dz2, False, what + " dW2")
    TB.conv_close(g1, CM.conv_ref64(nchw(dz2), M.flip_weight(p["conv2_w"]), dt, fold=True), dt, what + " g1")
    mean1, rstd1 = vec["bn1"][0], vec["bn1"][2]
    m1 = N.bn_bwd(g1.reshape(n, C), z1.reshape(n, C), N.mask_f32(z1.reshape(n, C), a1, b1), mean1, rstd1)
    TB.within(gr["bn1_beta"], m1["dbeta"], M.sum_bound(n, m1["dbeta_abs"]), what + " dbeta1")
    TB.within(gr["bn1_gamma"], m1["dgamma"], M.sum_bound(n, m1["dgamma_abs"]), what + " dgamma1")
    TB.check_dz(dz1, m1, p["bn1"]["gamma"], rstd1, gr["bn1_gamma"], gr["bn1_beta"], n, dt, what + " dz1")
    check(gr["conv1_weight"], xv, dz1, 3, False, what + " dW1")
    check(gr["sc_weight"], xv, dr, 1, False, what + " dWs")
    # ---- the step
    before = TB.host_params(A, blk, p)
    opt.step()
    y1st = vals16(be, blk.forward(x), dt).copy()
    A.sync()
    after = TB.host_params(A, blk, p)
    for k in ("conv1_w", "conv2_w", "sc_w"):
        assert (before[k] != after[k]).mean() > 0.9, k
    assert (y1st != y0).mean() > 0.3
    fresh = make_stem(be, dt, after)
    yf = vals16(be, fresh.forward(x), dt)
    assert yf.tobytes() == y1st.tobytes(), int((yf != y1st).sum())


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_stem_and_level0_refusals(be):
    from rangedet_amd.backbone_train import StemBlockTrain
    from rangedet_amd.backward import Level0TowerTrain
    A, L = be.alloc, be.lib
    p = stem_params(8, 2150)

    def make(**kw):
        q = dict(p, **kw)
        return StemBlockTrain(q["name"], q["conv1_w"], q["conv2_w"], q["bn1"], q["bn2"], q.get("sc_w"), q.get("sc_bn"), lib=L, alloc=A)
    with pytest.raises(NotImplementedError, match="BasicBlockTrain"):
        make(conv1_w=np.zeros((64, 64, 3, 3), F32))
    with pytest.raises(NotImplementedError, match="projection"):
        make(sc_w=None, sc_bn=None)
    with pytest.raises(RuntimeError, match="forward"):
        make().backward(np.zeros((1, 2, 8, 64), np.uint16))
    with pytest.raises(ValueError, match="slot"):
        make().forward(np.zeros((1, 2, 8, 8), np.uint16))
    one, zero = np.ones(128, F32), np.zeros(128, F32)
    ow, ob = np.zeros((1, 128), F32), np.zeros(1, F32)
    with pytest.raises(NotImplementedError, match="concat"):
        Level0TowerTrain([np.zeros((128, 81, 3, 3), F32)], [one], [zero], [zero], [one], ow, ob, lib=L, alloc=A)
    with pytest.raises(NotImplementedError, match="concat"):
        Level0TowerTrain([np.zeros((128, 128, 3, 3), F32)], [one], [zero], [zero], [one], ow, ob, lib=L, alloc=A)


def make_level0(be, dt, prm):
    from rangedet_amd.backward import Level0TowerTrain
    return Level0TowerTrain(prm["ws"], prm["gs"], prm["bs"], prm["mms"], prm["mvs"], prm["ow"], prm["ob"], kind="reg", level=0, first_conv=0, dtype=dt,
                            lib=be.lib, alloc=be.alloc)


@pytest.mark.parametrize("c", [8, 5])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_level0_tower_train(be, dt, c):
    """the reg tower of level 0 with c = 8 (Waymo) and c = 5 (KITTI: the master padded to 64 + 8 columns) at B 2, 3 x 37: the concat conv
    64 + c -> 128 and one 128 -> 128 layer; every step checked on the kernels' own inputs, the concat weight's gradient in the reference's
    shape (128, 64 + c, 3, 3) against the model on the concatenated input; after SGD.attach + two step() calls the master's padding columns
    and their momenta are still exactly zero, and the next forward equals that of a fresh tower built from the stepped masters.  The slot
    channels at or above c hold a non-zero pattern."""
    from rangedet_amd.optim import SGD
    A = be.alloc
    B, H, W, C, nout = 2, 3, 37, 128, 8
    c8 = (c + 7) // 8 * 8
    n, P = B * H * W, N.parts(B * H * W, 0)
    rng = np.random.default_rng(2201)
    prm = dict(ws=[(rng.standard_normal((C, 64 + c, 3, 3)) / np.sqrt(9 * (64 + c) / 2)).astype(F32), (rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C / 2)).astype(F32)],
               gs=[rng.uniform(0.5, 1.5, C).astype(F32) for _ in range(2)], bs=[(0.1 * rng.standard_normal(C)).astype(F32) for _ in range(2)],
               mms=[rng.normal(0, 1, C).astype(F32) for _ in range(2)], mvs=[rng.uniform(0.5, 2, C).astype(F32) for _ in range(2)],
               ow=(rng.standard_normal((nout, C, 1, 1)) / np.sqrt(C)).astype(F32), ob=(0.1 * rng.standard_normal(nout)).astype(F32))
    t = make_level0(be, dt, prm)
    xv, dv = rnd("relu", (B, H, W, 64), dt, 2202), rnd("normal", (B, H, W, c), dt, 2203)
    x, data = dev16(be, to_bits(xv, dt), dt), dev16(be, image(dv, dt, SLOT, 0), dt)
    d = rng.standard_normal((B, H * W, nout)).astype(F32)
    opt = SGD(lr=0.05, lib=be.lib, alloc=A)
    opt.attach(t)
    out0 = np.array(A.to_numpy(t.forward(x, data))).copy()
    dx, grads = t.backward(A.as_device_f32(d))
    A.sync()
    stem, oname = "rpn_reg_conv_%d_lvl_0", "rpn_reg_delta_lvl_0"
    names = [stem % i + s for i in (0, 1) for s in ("_weight", "_bn_gamma", "_bn_beta")] + [oname + "_weight", oname + "_bias"]
    assert sorted(grads) == sorted(names) and sorted(opt.state()) == sorted(names)
    gr = {k: np.array(A.to_numpy(v)) for k, v in grads.items()}
    assert gr[stem % 0 + "_weight"].shape == (C, 64 + c, 3, 3) and gr[stem % 1 + "_weight"].shape == (C, C, 3, 3) and tuple(dx.shape) == (B, H, W, 64)
    acts, zs = [vals16(be, v, dt) for v in t.acts], [vals16(be, v, dt) for v in t.zs]
    gsv, dzs, dxs = ([vals16(be, v, dt) for v in lst] for lst in (t.gs, t.dzs, t.dxs))
    what = "level-0 tower %s" % be.name
    check_hob((gsv[1], gr[oname + "_weight"].reshape(nout, C), gr[oname + "_bias"]), d, acts[2], prm["ow"].reshape(nout, C), dt, None, False, False, what)
    cat_in = np.concatenate([xv, dv], 3)
    for i in (1, 0):
        s = t.saved[i]
        mean, var, rstd, a, b = (TBN.dvec(A, s[k], C) for k in ("mean", "var", "rstd", "a", "b"))
        src = acts[i] if i else cat_in
        TB.conv_close(zs[i], CM.conv_ref64(TB.nchw(src), prm["ws"][i], dt, fold=True), dt, "%s z %d" % (what, i))
        TBN.check_stats(mean, var, zs[i], P, "%s stats %d" % (what, i))
        assert int(TB.ulps(rstd, N.fold_f32(mean, var, prm["gs"][i], prm["bs"][i], EPS, MOM, n, True, mean, var)["rstd"]).max()) <= (0 if be.name == "emu" else 2)
        a_own, b_own = N.fold_ab_f32(mean, rstd, prm["gs"][i], prm["bs"][i])
        assert same_bits(a, a_own) and same_bits(b, b_own)
        assert same_bits(acts[i + 1], N.affine_relu_f32(zs[i], a, b, dt)) and 0.2 < (acts[i + 1] == 0).mean() < 0.8
        stemi = stem % i
        TBN.check_bwd((dzs[i], gr[stemi + "_bn_gamma"], gr[stemi + "_bn_beta"]), gsv[i], zs[i], a, b, mean, rstd, prm["gs"][i], 1, dt, False, "%s bn %d" % (what, i))
        check(gr[stemi + "_weight"], src, dzs[i], 3, False, "%s dW %d" % (what, i))
        wdx = prm["ws"][i] if i else prm["ws"][0][:, :64]
        TB.conv_close(dxs[i], CM.conv_ref64(TB.nchw(dzs[i]), M.flip_weight(wdx), dt, fold=True), dt, "%s dx %d" % (what, i))
    assert gsv[0].tobytes() == dxs[1].tobytes() and vals16(be, dx, dt).tobytes() == dxs[0].tobytes()
    # ---- two steps (the second on the gradients of a second backward: the momenta carry)
    opt.step()
    t.forward(x, data)
    t.backward(A.as_device_f32(d))
    opt.step()
    out1 = np.array(A.to_numpy(t.forward(x, data))).copy()
    A.sync()
    assert (out1 != out0).mean() > 0.3 and opt.table_builds == 1
    ly = t.layers
    master = np.array(A.to_numpy(A.view_f32(ly[0]["master"], (C, 64 + c8, 3, 3)))).astype(F32)
    mom = np.array(A.to_numpy(opt.state()[stem % 0 + "_weight"])).astype(F32)
    assert master.shape == mom.shape == (C, 64 + c8, 3, 3)
    assert not master[:, 64 + c:].view(np.uint32).any() and not mom[:, 64 + c:].view(np.uint32).any(), "a padding column moved"
    assert (mom[:, :64 + c] != 0).mean() > 0.9
    after = dict(ws=[np.ascontiguousarray(master[:, :64 + c]),
                     np.array(A.to_numpy(A.view_f32(ly[1]["master"], (C, C, 3, 3)))).astype(F32)],
                 gs=[TBN.dvec(A, l["gamma"], C) for l in ly], bs=[TBN.dvec(A, l["beta"], C) for l in ly],
                 mms=[TBN.dvec(A, l["mmean"], C) for l in ly], mvs=[TBN.dvec(A, l["mvar"], C) for l in ly],
                 ow=np.array(A.to_numpy(A.view_f32(t.out_w, (nout, C)))).astype(F32), ob=np.array(A.to_numpy(A.view_f32(t.out_b, (nout,)))).astype(F32))
    assert (after["ws"][0] != prm["ws"][0]).mean() > 0.9 and (after["ws"][0][:, 64:] != prm["ws"][0][:, 64:]).mean() > 0.9
    fresh = make_level0(be, dt, after)
    outf = np.array(A.to_numpy(fresh.forward(x, data)))
    assert outf.tobytes() == out1.tobytes(), int((outf != out1).sum())


# ---- 11. refusals of the packers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_packer_status_codes(be):
    """cin 0 and 17, ksize 2, cout 32, cin1 != 64, a concat forward image at cin2 5, a fold scale where none is allowed, null and unaligned
    pointers, float32: each its code, nothing launched"""
    L = be.lib
    buf = be.empty(1 << 20)
    p = be.ptr(buf)
    BF = R.RD_BF16

    def narrow(w=p, fold=None, cout=64, cin=8, ksize=3, dt=BF, out=p):
        return L.raw("rd_pack_conv_narrow_dev")(w, fold, cout, cin, ksize, dt, out, be.stream)

    def cat(w=p, fold=None, cout=128, cin1=64, cin2=8, dg=0, dt=BF, out=p):
        return L.raw("rd_pack_conv3x3_cat_dev")(w, fold, cout, cin1, cin2, dg, dt, out, be.stream)
    for kw in (dict(cin=0), dict(cin=17), dict(ksize=2), dict(cout=32)):
        assert narrow(**kw) == R.RD_ESHAPE and L.rd_last_error_string().decode().startswith("pack_conv_narrow_dev"), kw
    for kw in (dict(cin1=128), dict(cin2=0), dict(cin2=17), dict(cin2=5), dict(cout=32)):
        assert cat(**kw) == R.RD_ESHAPE and L.rd_last_error_string().decode().startswith("pack_conv3x3_cat_dev"), kw
    assert narrow(ksize=1, fold=p) == R.RD_EINVAL and "fold" in L.rd_last_error_string().decode()
    assert cat(dg=1, fold=p) == R.RD_EINVAL and "fold" in L.rd_last_error_string().decode()
    for rc in (narrow(w=None), narrow(out=None), cat(w=None), cat(out=None)):
        assert rc == R.RD_EINVAL and "null" in L.rd_last_error_string().decode()
    for rc in (narrow(out=p + 8), narrow(w=p + 2), cat(out=p + 8), cat(fold=p + 2)):
        assert rc == R.RD_EINVAL and "aligned" in L.rd_last_error_string().decode()
    assert narrow(dt=R.RD_F32) == R.RD_EINVAL and cat(dt=R.RD_F32) == R.RD_EINVAL
    assert not be.down(buf, np.uint8, (1 << 20,)).any()           # nothing ran

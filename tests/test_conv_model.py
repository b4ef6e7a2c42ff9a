"""The conv-family checker (conv_model.py) has teeth: CPU only, no library.  The "kernel" is torch's fp32 conv on the packer's weights
followed by a round-to-nearest-even to the type -- correct arithmetic in some summation order -- and each planted fault is one a kernel
or a packer could really have.  Shape (2, 9, 70), 64 -> 128 channels, folded scale, residual, ReLU.

The clean result must have no element over conv_tol; every fault at least one.  For a wrong output rounding and a lost low half of the
shift the whole-tensor bound of the older assertions (test_kernels.py _tol, x 1.5 for folded weights) is asserted NOT to notice: that
is the gap the per-element assertions close."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_model as CM
from emu_util import h16_round
from rangedet_amd import lib as R

BF16, F16 = R.RD_BF16, R.RD_F16
B, H, W, CIN, COUT = 2, 9, 70, 64, 128
FL = R.RD_ADD | R.RD_RELU_POST
DTS = [pytest.param(BF16, id="bf16"), pytest.param(F16, id="f16")]


def _trunc(v, dt):
    """float32 -> the type, rounding toward zero"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if dt == BF16:
        return (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    h = v.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(v)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float32)


_CACHE = {}


def _problem(kind, dt):
    """inputs, the float64 reference and the pieces of the fp32 "kernel", once per (kind, type)"""
    if (kind, dt) not in _CACHE:
        x = CM.make_input(kind, (B, CIN, H, W), dt, seed=1)
        w = CM.make_weight(kind, (COUT, CIN, 3, 3), CIN * 9, seed=1)
        s, t = CM.make_affine(kind, COUT, seed=1)
        res = CM.make_residual(kind, (B, COUT, H, W), dt, seed=1)
        ref = CM.conv_ref64(x, w, dt, scale=s, shift=t, fold=True, flags=FL, res=res)
        CM.assert_fp16_range(ref, dt)
        wq = CM.fold_round(w, s, dt)
        acc = F.conv2d(torch.from_numpy(x), torch.from_numpy(wq), padding=1).numpy()          # fp32 accumulation
        for a in (x, wq, t, res, ref, acc):
            a.setflags(write=False)
        _CACHE[kind, dt] = dict(x=x, wq=wq, t=t, res=res, ref=ref, acc=acc)
    return _CACHE[kind, dt]


def _kernel(p, dt, fault=None):
    acc, t, res, x, wq = p["acc"], p["t"], p["res"], p["x"], p["wq"]
    if fault == "shift_rounded":                       # the packer keeps the high half of the shift only
        t = h16_round(t, dt)
    if fault == "product_missing":                     # one input channel skipped at one pixel (centre tap), every output channel
        acc = acc.copy()
        acc[1, :, 4, 37] -= wq[:, 13, 1, 1] * x[1, 13, 4, 37]
    if fault == "tap_missing":                         # the tap to the right missing at one pixel of the left border
        acc = acc.copy()
        acc[0, :, 5, 0] -= wq[:, :, 1, 2] @ x[0, :, 5, 1]
    pre = acc + t[None, :, None, None]
    out = (np.maximum(pre, 0) + res) if fault == "relu_side" else np.maximum(pre + res, 0)
    return _trunc(out, dt) if fault == "truncate" else h16_round(out.astype(np.float32), dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", CM.KINDS)
def test_correct_arithmetic_has_no_element_over(kind, dt):
    p = _problem(kind, dt)
    nover, worst = CM.conv_check(_kernel(p, dt), p["ref"], dt, p["t"])
    print("conv-model clean %s %s: worst err / tol %.3f" % (kind, "bf16" if dt == BF16 else "f16", worst))
    assert nover == 0 and worst <= 1.0, (nover, worst)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("fault", ["truncate", "shift_rounded", "product_missing", "tap_missing", "relu_side"])
def test_planted_fault_is_caught(fault, dt):
    p = _problem("normal", dt)
    got = _kernel(p, dt, fault)
    nover, worst = CM.conv_check(got, p["ref"], dt, p["t"])
    old = float(np.abs(got - p["ref"]).max()) / CM.whole_tensor_bound(p["ref"], dt, 1.5)
    print("conv-model %s %s: %d over, worst err / tol %.2f; err / whole-tensor bound %.2f" % (fault, "bf16" if dt == BF16 else "f16", nover, worst, old))
    assert nover >= 1 and worst > 1.0, (fault, nover, worst)
    if fault in ("truncate", "shift_rounded"):
        assert old <= 1.0, (fault, old)              # the whole-tensor bound lets these through: the gap


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", ["relu_sparse", "scaled"])
def test_planted_fault_is_caught_on_the_other_inputs(kind, dt):
    """the two arithmetic faults on the sparse and the eight-binade inputs (the addressing faults depend on one pixel's values only)"""
    p = _problem(kind, dt)
    for fault in ("truncate", "shift_rounded"):
        nover, worst = CM.conv_check(_kernel(p, dt, fault), p["ref"], dt, p["t"])
        assert nover >= 1, (kind, fault, worst)


@pytest.mark.parametrize("dt", DTS)
def test_error_of_one_relative_unit_below_a_binade_top_is_caught(dt):
    """What the binade pricing is for: an error of u |ref| (u = 2^-8 bf16, 2^-11 fp16) on a value in the upper quarter of its binade is
    1.75 to 2 half-ulps.  The relative form u |ref| + 1e-5 max |ref| (test_production_layers.py _check) accepts it by construction."""
    p = _problem("normal", dt)
    ref = p["ref"]
    u = 2.0 ** -8 if dt == BF16 else 2.0 ** -11
    a = np.abs(ref)
    top = (a > 0.25) & (a / np.exp2(np.floor(np.log2(np.where(a > 0, a, 1.0)))) >= 1.75)
    assert top.sum() > 100
    got = np.where(top, ref + u * a, _kernel(p, dt))
    nover, worst = CM.conv_check(got, ref, dt, p["t"])
    assert nover >= 1 and worst > 1.0, (nover, worst)
    assert np.all(np.abs(got - ref) <= u * a + 1e-5 * max(1.0, a.max()))


def test_half_ulp_and_tolerance_values():
    r = np.array([0.0, 1.0, 1.999, 2.0, -3.0, 2.0 ** -20, 0.75])
    assert np.array_equal(CM.half_ulp_of(r, BF16), [0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 2.0 ** -28, 2.0 ** -9])
    assert np.array_equal(CM.half_ulp_of(r, F16), [0.0, 2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -10, 2.0 ** -25, 2.0 ** -12])
    sh = np.array([-4.0, 1.0], np.float32)
    assert np.allclose(CM.conv_tol(r, BF16, sh) - CM.half_ulp_of(r, BF16), 1e-5 * 3.0 + 2.0 ** -14, rtol=1e-12, atol=0)
    assert np.allclose(CM.conv_tol(r, F16, sh) - CM.half_ulp_of(r, F16), 1e-5 * 3.0, rtol=1e-12, atol=0)
    assert CM.conv_check(r, r, BF16) == (0, 0.0)


def test_reference_forms_agree_with_plain_torch():
    """conv_ref64's launch forms against torch written out longhand (float64): un-folded stride 2 with RELU_PRE + ADD, folded with a
    projection shortcut, a transposed conv"""
    dt = BF16
    T = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    x = CM.make_input("normal", (1, 16, 3, 10), dt)
    w = CM.make_weight("normal", (64, 16, 3, 3), 144)
    s, t = CM.make_affine("normal", 64)
    res = CM.make_residual("normal", (1, 64, 3, 5), dt)
    want = torch.relu(F.conv2d(T(x), T(h16_round(w, dt)), stride=(1, 2), padding=1) * T(s).view(1, -1, 1, 1) + T(t).view(1, -1, 1, 1)) + T(res)
    got = CM.conv_ref64(x, w, dt, scale=s, shift=t, stride=2, flags=R.RD_RELU_PRE | R.RD_ADD, res=res)
    assert np.array_equal(got, want.numpy())
    x0 = CM.make_input("normal", (1, 8, 3, 10), dt, seed=2)
    wsc = CM.make_weight("normal", (64, 8), 8, seed=2)
    ss = CM.make_affine("normal", 64, seed=2)[0]
    want = F.conv2d(T(x), T(h16_round(w * s[:, None, None, None], dt)), padding=1) + T(t).view(1, -1, 1, 1)
    want = torch.relu(want + F.conv2d(T(x0), T(h16_round(wsc * ss[:, None], dt))[:, :, None, None]))
    got = CM.conv_ref64(x, w, dt, scale=s, shift=t, fold=True, flags=R.RD_ADD | R.RD_RELU_POST, sc_x=x0, sc_w=wsc, sc_scale=ss)
    assert np.array_equal(got, want.numpy())
    wd = CM.make_weight("normal", (16, 64, 3, 4), 96, out_axis=1)
    want = torch.relu(F.conv_transpose2d(T(x), T(h16_round(wd * s[None, :, None, None], dt)), stride=(1, 2), padding=(1, 1)) + T(t).view(1, -1, 1, 1))
    got = CM.conv_ref64(x, wd, dt, scale=s, shift=t, fold=True, flags=R.RD_RELU_POST, deconv=(2, 1))
    assert np.array_equal(got, want.numpy())


def test_inputs_are_what_they_say():
    for dt in (BF16, F16):
        x = CM.make_input("relu_sparse", (2, 72, 5, 9), dt)
        assert (x >= 0).all() and not x[:, :, :, :2].any() and not x[:, :, :, -2:].any() and not x[:, :, -1].any() and not x[:, 32:64].any()
        assert x[:, :32, :-1, 2:-2].any() and x[:, 64:].any() and np.array_equal(x, h16_round(x, dt))
        x = CM.make_input("scaled", (1, 24, 4, 50), dt)
        sd = x.std(axis=(0, 2, 3))
        assert np.all(np.abs(np.log2(sd) - ((np.arange(24) % 12) - 6)) < 0.5) and np.isfinite(x).all()
        w = CM.make_weight("scaled", (16, 8, 3, 3), 1.0)
        assert np.all(np.abs(np.log2(w.std(axis=(1, 2, 3))) - ((np.arange(16) % 8) - 4)) < 0.5)
    b = CM.nhwc_filled(CM.make_input("normal", (1, 72, 2, 3), BF16), BF16, 80)
    assert not b[..., 72:].any()                                        # 72 in 80: inside the last 16-channel slot, read, zero
    b = CM.nhwc_filled(CM.make_input("normal", (1, 64, 2, 3), BF16), BF16, 96, coff=16)
    assert (b[..., :16] == CM.PAD_PATTERN).all() and (b[..., 80:] == CM.PAD_PATTERN).all() and b[..., 16:80].any()
    b = CM.nhwc_filled(CM.make_input("normal", (1, 5, 2, 3), F16), F16, 24)
    assert not b[..., 5:16].any() and (b[..., 16:] == CM.PAD_PATTERN).all()

"""Per-element error model and inputs of the conv-family parity tests (plain module, imported by test_kernels.py and test_conv_model.py).

  conv_ref64      the float64 reference of ONE conv-family launch on the weights the packer actually makes: h16_round(w * s) with the
                  product in float32 for folded scales (rd_api.hip: `fold_scale[co] * w[...]` in float, then rounded), conv(x, h16_round(w))
                  * s + t for un-folded ones; 1x1 projection shortcut, residual, RD_RELU_PRE / RD_ADD / RD_RELU_POST, stride (1, 2),
                  transposed conv.  A restatement of the operation: no tiling, no fragment order.
  half_ulp_of     half an ulp of the output type in the reference value's OWN binade
  conv_tol        half_ulp_of + 1e-5 max(1, max |ref|) + 2^-16 max |shift| (bf16); the last two terms are _check's of test_production_layers.py
  conv_check      (elements over the tolerance, worst err / tol)
  head_ref64 / head_check   the fp32 outputs of a fused tower output conv: computed from ROUNDED activations, so the tolerance is
                  1e-5 max(1, max |ref|) + 4 u max |act| max |hw| per element (test_production_layers.py's model)
  make_input / make_weight / make_residual   seeded inputs, rounded to the type, all finite: "normal", "relu_sparse", "scaled"
  nhwc_filled     the channels-last device image of an input with the padding channels set as the launch contract allows

Nothing here reads the reference tree, and nothing here looks at a kernel's output to size a tolerance."""
import numpy as np
import torch
import torch.nn.functional as F

from emu_util import h16_round, to_nhwc
from rangedet_amd import lib as R

BF16, F16 = R.RD_BF16, R.RD_F16
KINDS = ("normal", "relu_sparse", "scaled")
F16_MAX = 65504.0


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def fold_round(w, s, dt, out_axis=0):
    """the weights a folding packer stores: s[co] * w in float32, rounded to the type (rd_pack_conv3x3_ex_host & co.)"""
    shape = [1] * w.ndim
    shape[out_axis] = -1
    return h16_round(np.asarray(s, np.float32).reshape(shape) * np.asarray(w, np.float32), dt)


def conv_ref64(x, w, dt, scale=None, shift=None, fold=False, stride=1, flags=0, res=None, sc_x=None, sc_w=None, sc_scale=None, deconv=None):
    """float64 reference of one launch.  x (B, cin, H, W) and res / sc_x: values already rounded to dt.  w: (cout, cin, k, k) float32, or
    (cin, cout, kh, kw) with deconv = (stride_w, pad_w).  scale / shift: the float32 arrays the packer / the device get (None: 1 / 0).
    fold: the scale is in the rounded weights.  sc_w (cout, sc_cin) with sc_scale: the 1x1 projection shortcut of sc_x at the output
    grid, its scale always folded; its sum joins the accumulators BEFORE the activation (rd_conv3x3_bn_act_ex).  -> numpy float64 NCHW"""
    oa = 1 if deconv else 0
    cout = w.shape[oa]
    s = np.ones(cout, np.float32) if scale is None else np.asarray(scale, np.float32)
    wq = fold_round(w, s, dt, oa) if fold else h16_round(np.asarray(w, np.float32), dt)
    if deconv:
        y = F.conv_transpose2d(_t64(x), _t64(wq), stride=(1, deconv[0]), padding=(1, deconv[1]))
    else:
        k = w.shape[2]
        y = F.conv2d(_t64(x), _t64(wq), stride=(1, stride), padding=k // 2)
    if not fold:
        y = y * _t64(s).view(1, -1, 1, 1)
    if shift is not None:
        y = y + _t64(shift).view(1, -1, 1, 1)
    if sc_w is not None:
        wsq = fold_round(sc_w, np.ones(cout, np.float32) if sc_scale is None else sc_scale, dt)
        y = y + F.conv2d(_t64(sc_x), _t64(wsq)[:, :, None, None], stride=(1, stride))
    if flags & R.RD_RELU_PRE:
        y = torch.relu(y)
    if (flags & R.RD_ADD) and res is not None:
        y = y + _t64(res)
    if flags & R.RD_RELU_POST:
        y = torch.relu(y)
    return y.numpy()


def half_ulp_of(ref, dt):
    """half an ulp of dt at each reference value: 2^(floor(log2 |ref|) - 8) for bf16 (8 significant bits), 2^(floor(log2 |ref|) - 11) for
    fp16 and never below 2^-25 there (its subnormals); 0 where ref == 0"""
    ref = np.asarray(ref, np.float64)
    a = np.abs(ref)
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    h = np.exp2(e - (8 if dt == BF16 else 11))
    if dt == F16:
        h = np.maximum(h, 2.0 ** -25)
    return np.where(a > 0, h, 0.0)


def conv_tol(ref, dt, shift=None):
    """per element: the output rounding + fp32 summation order (1e-5 of the largest value) + the bf16 hi + lo pair that carries the shift
    through the accumulators (2^-16 of the largest shift; fp16's pair is exact to 2^-22: nothing).  A value within summation noise of a
    rounding boundary may round the other way: half an ulp plus the noise, which is this sum."""
    ref = np.asarray(ref, np.float64)
    sh = float(np.abs(shift).max()) if (shift is not None and dt == BF16) else 0.0
    return half_ulp_of(ref, dt) + 1e-5 * max(1.0, float(np.abs(ref).max())) + 2.0 ** -16 * sh


def _count(got, ref, tol):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    assert np.isfinite(err).all(), "non-finite output or reference"
    return int((err > tol).sum()), float((err / tol).max())


def conv_check(got, ref, dt, shift=None):
    """-> (elements over tolerance, worst err / tol)"""
    return _count(got, ref, conv_tol(ref, dt, shift))


def whole_tensor_bound(ref, dt, factor=1.0):
    """test_kernels.py's _tol for the 16-bit types (restated for test_conv_model.py, which documents what it lets through)"""
    u = 2.0 ** -8 if dt == BF16 else 2.0 ** -11
    return factor * (u * max(1.0, float(np.abs(ref).max())) + (2e-5 if dt == F16 else 0.0))


def head_ref64(act64, hw, hb, dt):
    """the fused 1x1 output conv on the tower activation ROUNDED to dt (through float32, as on the device); fp32 weights and bias exact.
    -> (ref (B, H*W, nout) float64, the rounded activation)"""
    act = h16_round(np.asarray(act64, np.float64).astype(np.float32), dt).astype(np.float64)
    B = act.shape[0]
    return np.einsum("oc,bchw->bhwo", np.asarray(hw, np.float64), act).reshape(B, -1, hw.shape[0]) + np.asarray(hb, np.float64), act


def head_check(got, ref, act, hw, dt):
    """an activation within fp32 noise of a rounding boundary may round the other way: one unit (2u |act|) times its weight, a few per
    output at most -> tol = 1e-5 max(1, max |ref|) + 4 u max |act| max |hw|, applied to every element"""
    u = 2.0 ** -8 if dt == BF16 else 2.0 ** -11
    tol = 1e-5 * max(1.0, float(np.abs(ref).max())) + 4 * u * float(np.abs(act).max()) * float(np.abs(hw).max())
    return _count(got, ref, tol)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
IN_EXP = (12, 6)      # "scaled": input channel c times 2^((c % 12) - 6)
OUT_EXP = (8, 4)      # "scaled": the weights of output channel o times 2^((o % 8) - 4) -> outputs over eight binades


def make_input(kind, shape, dt, seed=0):
    """(B, C, H, W) float32, rounded to dt.
      normal       standard normal (the inputs of the older tests)
      relu_sparse  max(normal, 0); the first and last two columns and the last row of every image exactly zero, as a padded range image
                   has; input channels [32, 64) -- one whole 32-channel chunk -- zero when there are at least 64
      scaled       normal, channel c times 2^((c % 12) - 6)"""
    assert kind in KINDS, kind
    rng = np.random.default_rng(7000 + seed)
    x = rng.standard_normal(shape)
    if kind == "relu_sparse":
        x = np.maximum(x, 0.0)
        x[..., :2] = 0.0
        x[..., -2:] = 0.0
        x[:, :, -1, :] = 0.0
        if shape[1] >= 64:
            x[:, 32:64] = 0.0
    elif kind == "scaled":
        x = x * np.exp2((np.arange(shape[1]) % IN_EXP[0]) - IN_EXP[1]).reshape(1, -1, 1, 1)
    return h16_round(x.astype(np.float32), dt)


def out_scale(kind, cout):
    return np.exp2((np.arange(cout) % OUT_EXP[0]) - OUT_EXP[1]).astype(np.float32) if kind == "scaled" else np.ones(cout, np.float32)


def make_weight(kind, shape, fan_in, seed=0, out_axis=0):
    """float32 weights of std 1 / sqrt(fan_in) (NOT rounded: the packers round); "scaled": output channel o times 2^((o % 8) - 4)"""
    rng = np.random.default_rng(8000 + seed)
    w = rng.standard_normal(shape) / np.sqrt(fan_in)
    sh = [1] * len(shape)
    sh[out_axis] = -1
    return (w * out_scale(kind, shape[out_axis]).reshape(sh)).astype(np.float32)


def make_residual(kind, shape, dt, seed=0):
    """a residual at the output's own scale per channel ("scaled": times 2^((o % 8) - 4) like the weights)"""
    rng = np.random.default_rng(9000 + seed)
    r = rng.standard_normal(shape) * out_scale(kind, shape[1]).reshape(1, -1, 1, 1)
    if kind == "relu_sparse":
        r = np.maximum(r, 0.0)
    return h16_round(r.astype(np.float32), dt)


def make_affine(kind, cout, seed=0):
    """BatchNorm scale in [0.5, 1.5) and a shift at the output's scale"""
    rng = np.random.default_rng(9500 + seed)
    return rng.uniform(0.5, 1.5, cout).astype(np.float32), (rng.standard_normal(cout) * out_scale(kind, cout)).astype(np.float32)


PAD_PATTERN = 0x4B4B      # finite and far from zero in both types: 1.3e7 as bf16, 14.6 as fp16


def nhwc_filled(x, dt, cs, coff=0):
    """to_nhwc with the channels of the cs-wide buffer that are NOT x's set by the launch contract (include/rangedet_hip.h, rd_api.hip):
    the conv family rounds cin up to the 16-channel k-slot and requires ZEROS there (they are read: 72 channels in an 80-wide buffer are
    all inside slots, so that buffer's padding is zero); channels beyond the last slot, and before coff, are never read and get
    PAD_PATTERN.  A kernel that reads them, or a packer that leaves a weight on them, shows at once."""
    B, C, H, W = x.shape
    buf = to_nhwc(x, dt, cstride=cs, coff=coff)
    read_to = coff + -(-C // 16) * 16
    buf[..., :coff] = PAD_PATTERN
    buf[..., read_to:] = PAD_PATTERN
    return buf


def assert_fp16_range(ref, dt):
    """fp16 only: no reference value may overflow the type (narrow IN_EXP / OUT_EXP if one ever does)"""
    if dt == F16:
        assert float(np.abs(ref).max()) < F16_MAX, float(np.abs(ref).max())

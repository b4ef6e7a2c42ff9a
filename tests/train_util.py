"""Helpers the training-path tests share (test_conv_backward.py, test_batch_norm.py): seeded inputs in the two 16-bit types, 0xFF-prefilled
output buffers with a guard tail, device tensors of the activation type, and the checks of the output-conv backward and the weight gradient
against tests/convbwd_model.py."""
import numpy as np
import pytest

import conv_model as CM
import convbwd_model as M
from emu_util import bf16_bits_to_f32, f16_bits_to_f32, f32_to_bf16_bits, f32_to_f16_bits, h16_round
from rangedet_amd import lib as R

GUARD = 64
DTS = [pytest.param(R.RD_BF16, id="bf16"), pytest.param(R.RD_F16, id="f16")]


def to_bits(a, dt):
    return f32_to_bf16_bits(a) if dt == R.RD_BF16 else f32_to_f16_bits(a)


def from_bits(b, dt):
    return bf16_bits_to_f32(b) if dt == R.RD_BF16 else f16_bits_to_f32(b)


def image(v, dt, cs=None, coff=0):
    """(B, H, W, C) float32 values -> (B, H, W, cs) uint16 image, the channels outside [coff, coff + C) set to a finite, non-zero pattern"""
    C = v.shape[3]
    buf = np.full(v.shape[:3] + (cs or C,), CM.PAD_PATTERN, np.uint16)
    buf[..., coff:coff + C] = to_bits(v, dt)
    return buf


def ff(be, nbytes):
    return be.up(np.full(nbytes + GUARD, 0xFF, np.uint8))


def back(be, buf, nbytes, what):
    raw = be.down(buf, np.uint8, (nbytes + GUARD,))
    assert (raw[nbytes:] == 0xFF).all(), "%s: written past its end" % what
    return raw[:nbytes]


def back_image(be, buf, shape, cs, coff, dt, what):
    """the (B, H, W, C) values of a 0xFF-prefilled (B, H, W, cs) output image; its other channels and its guard must be untouched"""
    B, H, W, C = shape
    raw = back(be, buf, B * H * W * cs * 2, what).view(np.uint16).reshape(B, H, W, cs)
    outside = np.ones(cs, bool)
    outside[coff:coff + C] = False
    assert (raw[..., outside] == 0xFFFF).all(), "%s: channels outside [coff, coff + C) written" % what
    return raw[..., coff:coff + C]


_INPUTS = {}


def rnd(kind, shape, dt, seed):
    """seeded (B, H, W, C) values rounded to dt, made once: 'normal', 'relu' (max(normal, 0): half zeros), 'ints' (-3 .. 3)"""
    key = (kind, tuple(shape), dt, seed)
    if key not in _INPUTS:
        rng = np.random.default_rng(seed)
        if kind == "ints":
            v = rng.integers(-3, 4, shape).astype(np.float32)
        else:
            v = rng.standard_normal(shape)
            v = h16_round((np.maximum(v, 0.0) if kind == "relu" else v).astype(np.float32), dt)
        v.setflags(write=False)
        _INPUTS[key] = v
    return _INPUTS[key]


def same_bits(got, want64):
    """float32 arrays equal in every bit once -0 is +0"""
    return ((np.asarray(got, np.float32) + np.float32(0)).tobytes() == (np.asarray(want64).astype(np.float32) + np.float32(0)).tobytes())


def check_wgrad(got, x, dz, exact, what):
    want, sabs, n = M.weight_grad(x, dz, want_abs=not exact)
    assert np.isfinite(got).all(), what
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


def check_hob(got, d, x, w, dt, scale, mask, exact, what):
    """x: the values the launch read (B, H, W, cin)"""
    dx, dw, db = got
    B, H, W, cin = x.shape
    nout = w.shape[0]
    m = M.head_out_bwd(d, x.reshape(B, H * W, cin), w)
    n = B * H * W
    if exact:
        assert same_bits(dw, m["dw"]) and same_bits(db, m["dbias"]), what
    else:
        for name, g_, key in (("dw", dw, "dw"), ("dbias", db, "dbias")):
            bound = M.sum_bound(n, m[key + "_abs"])
            err = np.abs(g_.astype(np.float64) - m[key])
            assert (err[bound == 0] == 0).all(), (what, name)
            worst = float((err[bound > 0] / bound[bound > 0]).max(initial=0))
            print(what, name, "worst err / bound %.3g" % worst)
            assert worst <= 1, (what, name, worst)
    s = np.ones(cin) if scale is None else np.asarray(scale, np.float64)
    keep = (x.reshape(B, H * W, cin) > 0) if mask else np.ones((B, H * W, cin), bool)
    v = m["dx"] * keep * s
    tol = CM.half_ulp_of(v, dt) + M.sum_bound(nout, m["dx_abs"] * keep * np.abs(s)) + (M.U * np.abs(v) if scale is not None else 0.0)
    err = np.abs(dx.reshape(B, H * W, cin).astype(np.float64) - v)
    assert (err[tol == 0] == 0).all(), what
    worst = float((err[tol > 0] / tol[tol > 0]).max(initial=0))
    print(what, "dx worst err / tol %.3g" % worst)
    assert worst <= 1, (what, worst)
    if exact and scale is None:
        assert same_bits(dx.reshape(v.shape), v), what


def dev16(be, bits, dt):
    """uint16 bits -> a (B, H, W, C) device tensor of the activation type (emu: the numpy bits themselves)"""
    buf = be.up(bits)
    if be.name == "emu":
        return buf[:bits.size * 2].view(np.uint16).reshape(bits.shape)
    import torch
    return buf[:bits.size * 2].view(torch.bfloat16 if dt == R.RD_BF16 else torch.float16).view(*bits.shape)


def vals16(be, t, dt):
    """a 16-bit device tensor -> float32 values"""
    if isinstance(t, np.ndarray):
        return from_bits(t, dt)
    import torch
    return from_bits(t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), dt)


def train_inputs(B, H, W, n_gt=10, seed=5):
    """the training inputs of one level at stride 1, built the way test_loss.make_case builds them (seeded; mask with 15 % zeros, regression
    weights 3 / 1 on 40 % of the pixels over 1 .. 49 points, targets within 2 of a unit normal, 8 GT boxes of 2 m x 4 m and padding rows)"""
    rng = np.random.default_rng(seed)
    n = H * W
    r, az = rng.uniform(10, 60, (B, n)), rng.uniform(-np.pi, np.pi, (B, n))
    pc = np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-1, 2, (B, n))], -1).astype(np.float32)
    gt = np.tile(np.array([0, 0, 0, 1e-3, 1e-3, 1e-3, 1e-3, 0], np.float32), (B, n_gt, 1))
    for b in range(B):
        for j, i in enumerate(rng.choice(n, 8, replace=False)):
            cx, cy = pc[b, i, 0], pc[b, i, 1]
            gt[b, j] = [cx - 2, cy - 1, cx - 2, cy + 1, cx + 2, cy + 1, cx + 2, cy - 1]
    mask = (rng.random((B, n)) >= 0.15).astype(np.float32)
    boxpix = rng.random((B, n)) < 0.4
    weight = (np.array([3, 1, 1, 1, 1, 1, 1, 1], np.float32)[None, :, None] * boxpix[:, None, :]).astype(np.float32)
    norm_weight = np.repeat((boxpix / rng.integers(1, 50, (B, n))).astype(np.float32)[:, None, :], 8, 1)
    target = rng.normal(0, 1, (B, 8, n)).astype(np.float32)
    return {"gt_bbox_veh_for_iou_pred": gt, "pc_vehicle_frame_s1": pc, "range_image_mask_s1": mask.reshape(B, 1, H, W),
            "rpn_reg_target_s1": target.reshape(B, 8, H, W), "rpn_reg_weight_s1": weight.reshape(B, 8, H, W),
            "reg_normalize_weight_s1": norm_weight.reshape(B, 8, H, W)}

"""Float64 restatements and error bounds of the post-forward chain (plain module, imported by test_post_forward.py): rd_head_out,
rd_sorted_foreground's sigmoid, rd_decode3d_bbox, rd_dets12_to_8.  Each bound is derived here from the precision of the number formats,
the operation count and the device math library's documented accuracy -- never from what a kernel returns.

  U = 2^-24      half an ulp of float32 relative to the value: one correctly rounded float32 operation (+, -, *, /, fma) has relative
                 error <= U.  eps32 = 2^-23 = 2 U.
  device libm    the ROCm HIP math API reference lists the maximum error of expf, sinf, cosf, atan2f and sqrtf as 1 ulp each: relative error
                 <= 2 U of the result (glibc's, on the emulator tier, are within 1 ulp too).  Float division is correctly rounded as the
                 library is built (no fast-math; hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt).

  SIGMOID_REL = 4 U     s = 1 / (1 + expf(-x)):  e = expf(-x) is off by <= 2 U e;  t = 1 + e by (2 U e + U t) / t <= 3 U relative;  the
                        division adds U.  (+ 8 U^2 for the products of the terms.)
  DECODE_C    = 7       corners, in units of U (|x| + |y| + |dx| + |dy| + l/2 + w/2) (1 + A), A = |az| + |yaw_r| (decode3d_ref64)
  DECODE_CZ   = 5       z outputs, in units of U (|z terms| + h)
  DETS8_C     = 3 / 1 / 4   centre / cz / length and width of rd_dets12_to_8, in units of U times the sum of the operands' magnitudes
                        (= 1.5 / 0.5 / 2 eps32)

Nothing here reads the reference tree."""
import numpy as np

from emu_util import h16_round
from rangedet_amd import lib as R

BF16, F16 = R.RD_BF16, R.RD_F16
U = 2.0 ** -24
SIGMOID_REL = 4 * U + 8 * U * U
DECODE_C = 7.0
DECODE_CZ = 5.0
DETS8_C_CENTRE, DETS8_C_CZ, DETS8_C_LEN = 3.0, 1.0, 4.0


def _f64(a):
    return np.asarray(a, np.float64)


def ratio(got, ref, tol):
    """-> (elements over the tolerance, worst err / tol); an element with tol == 0 must be exact"""
    err = np.abs(_f64(got) - _f64(ref))
    assert np.isfinite(err).all(), "non-finite output or reference"
    r = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    return int((r > 1.0).sum()), float(r.max())


# ---- sigmoid of the sort key ---------------------------------------------------------------------------------------------------------------
def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-_f64(x)))


def sigmoid_order(logit, mask, k):
    """the order the sigmoid path must return for one frame, libm-free: sigmoid is monotonic, and every logit >= 17.4 rounds to exactly
    1.0f (expf(-x) < 2^-25), so: stable argsort, descending, of min(logit, 20) with masked-out points last (their score is exactly 0, below
    every sigmoid of a logit > -87).  Valid for logits that are either >= 17.4 or spaced so widely that their float32 sigmoids differ."""
    key = np.where(np.asarray(mask) > 0, np.minimum(_f64(logit), 20.0), -np.inf)
    return np.argsort(-key, kind="stable")[:k]


# ---- rd_decode3d_bbox ------------------------------------------------------------------------------------------------------------------------
def decode3d_ref64(delta, pc, is_bin):
    """decode_3d_bbox's Map() in float64 on the float32 inputs.  delta (..., 8 | 7), pc (..., 3) -> (ref (..., 10), tol (..., 10)).

    Corner bound, per point, with S = |x| + |y| + |dx| + |dy| + l/2 + w/2 and A = |az| + |yaw_r| (the magnitudes of the two angles that are
    added; for the bin type |az| + |d6|; A >= |yaw|):
      yaw = atan2f(d5, d4) + az     two 1-ulp atan2f (2 U |yaw_r| + 2 U |az|) + the add (U |yaw|)                     <= 3 U A
      sinf / cosf (yaw)             the angle's error (slope <= 1) + 1 ulp of a value <= 1                            <= U (3 A + 2)
      l/2, w/2                      0.5 * expf: 1 ulp (the halving in double is exact)                                <= 2 U relative
      hx * c - hy * s               each product: h U (3 A + 2) + 2 U h + U h; the subtraction U (hl + hw)            <= U (hl + hw) (3 A + 6)
      cosf / sinf (az)              2 U |az| + 2 U                                                                    <= U (2 A + 2)
      dx = d0 |d0|, dx ca - dy sa   dx: U; each product U (2 A + 2) + U + U; the subtraction U                        <= U (|dx| + |dy|) (2 A + 5)
      cx = x + dxl                  U (|x| + |dx| + |dy|)
      (...) + cx                    U (hl + hw + |x| + |dx| + |dy|)
    sum <= U [(hl + hw) (3 A + 7) + (|dx| + |dy|) (2 A + 7) + 2 |x|] <= 7 U S (1 + A): DECODE_C = 7.  FMA contraction only removes roundings.

    z bound.  Regular type: o8 = d6 exactly (tol 0); o9 = d6 + expf(d7): 2 U h + U (|d6| + h).  Bin type: cz = z + d2: U (|z| + |d2|);
    o8 = float(cz - h/2): that + U h (expf) + the rounding U (|z| + |d2| + h/2); o9 = o8 + h: o8's error + 2 U h + U (|z| + |d2| + 1.5 h)
    <= U (3 (|z| + |d2|) + 5 h).  All <= 5 U (|z terms| + h): DECODE_CZ = 5."""
    d, p = _f64(delta), _f64(pc)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    az = np.arctan2(y, x)
    if is_bin:
        dx, dy = d[..., 0], d[..., 1]
        w, l, h = np.exp(d[..., 3]), np.exp(d[..., 4]), np.exp(d[..., 5])
        cz = z + d[..., 2]
        z0 = cz - h / 2.0
        yaw_r = d[..., 6]
        zmag = np.abs(z) + np.abs(d[..., 2])
    else:
        dx, dy = d[..., 0] * np.abs(d[..., 0]), d[..., 1] * np.abs(d[..., 1])
        w, l, h = np.exp(d[..., 2]), np.exp(d[..., 3]), np.exp(d[..., 7])
        z0 = d[..., 6]
        yaw_r = np.arctan2(d[..., 5], d[..., 4])
        zmag = np.abs(z0)
    yaw = yaw_r + az
    ca, sa = np.cos(az), np.sin(az)
    cx, cy = x + (dx * ca - dy * sa), y + (dx * sa + dy * ca)
    s, c = np.sin(yaw), np.cos(yaw)
    hl, hw = 0.5 * l, 0.5 * w
    ref = np.empty(d.shape[:-1] + (10,), np.float64)
    for k, (hx, hy) in enumerate(((hl, -hw), (-hl, -hw), (-hl, hw), (hl, hw))):
        ref[..., 2 * k] = (hx * c - hy * s) + cx
        ref[..., 2 * k + 1] = (hx * s + hy * c) + cy
    ref[..., 8] = z0
    ref[..., 9] = z0 + h
    S = np.abs(x) + np.abs(y) + np.abs(dx) + np.abs(dy) + hl + hw
    A = np.abs(az) + np.abs(yaw_r)
    tol = np.empty_like(ref)
    tol[..., :8] = (DECODE_C * U * S * (1.0 + A))[..., None]
    tz = DECODE_CZ * U * (zmag + h)
    tol[..., 8] = tz if is_bin else 0.0
    tol[..., 9] = tz
    return ref, tol


# ---- rd_dets12_to_8 --------------------------------------------------------------------------------------------------------------------------
def dets8_ref64(d12):
    """bbox3d_12dim_to_8dim in float64 on the float32 rows.  d12 (n, 12) -> (ref (n, 8), tol (n, 8)); tol 0 = a copied column.
      centre   ((a + b) + c + d) / 4: three adds, each U times a partial sum <= the sum of magnitudes; / 4 is exact      3 U sum |d|
      cz       d9 + d10 / 2: the halving is exact, one add                                                              U (|d9| + |d10| / 2)
      length   sqrtf(ax^2 + ay^2), ax = d2 - d0, ay = d3 - d1; M = |d0| + |d1| + |d2| + |d3| >= the length L:
               the two differences carry U M into L (slope <= 1); squares and their sum <= 2 U of the radicand (with or without an fma),
               halved by the root: U L; sqrtf 1 ulp: 2 U L                                                              U M + 3 U L <= 4 U M"""
    d = _f64(d12)
    ref = np.zeros((d.shape[0], 8), np.float64)
    tol = np.zeros_like(ref)
    a = np.abs(d)
    ref[:, 0] = (d[:, 0] + d[:, 2] + d[:, 4] + d[:, 6]) / 4.0
    ref[:, 1] = (d[:, 1] + d[:, 3] + d[:, 5] + d[:, 7]) / 4.0
    tol[:, 0] = DETS8_C_CENTRE * U * (a[:, 0] + a[:, 2] + a[:, 4] + a[:, 6])
    tol[:, 1] = DETS8_C_CENTRE * U * (a[:, 1] + a[:, 3] + a[:, 5] + a[:, 7])
    ref[:, 2] = d[:, 9] + d[:, 10] / 2.0
    tol[:, 2] = DETS8_C_CZ * U * (a[:, 9] + a[:, 10] / 2.0)
    ref[:, 3] = np.sqrt((d[:, 2] - d[:, 0]) ** 2 + (d[:, 3] - d[:, 1]) ** 2)
    ref[:, 4] = np.sqrt((d[:, 2] - d[:, 4]) ** 2 + (d[:, 3] - d[:, 5]) ** 2)
    tol[:, 3] = DETS8_C_LEN * U * (a[:, 0] + a[:, 1] + a[:, 2] + a[:, 3])
    tol[:, 4] = DETS8_C_LEN * U * (a[:, 2] + a[:, 3] + a[:, 4] + a[:, 5])
    ref[:, 5], ref[:, 6], ref[:, 7] = d[:, 10], d[:, 8], d[:, 11]
    return ref, tol


# ---- rd_head_out -----------------------------------------------------------------------------------------------------------------------------
def head_uses_matrix_cores(dt, nout, cin, cstride, coff):
    """rd_head_out's dispatch (rd_api.hip): the matrix-core streaming variant, else the generic kernel"""
    return dt in R.H16 and nout > 1 and cin % 16 == 0 and cstride % 8 == 0 and coff % 8 == 0


def head_ref64(x, w, b, dt, matrix_cores):
    """x (B, HW, cin) float32 values already rounded to dt, w (nout, cin) and b (nout) float32 -> (ref, tol), both (B, HW, nout) float64.
      fp32 accumulation in any order over cin products and the bias, each product rounded (or fused): (cin + 2) U (sum |x w| + |b|),
      and the final rounding U |ref|;
      matrix cores: the weight enters as a sum of terms of the 16-bit type.  bf16: 2^-18 sum |x w| -- what hi + lo of 8 significant
      bits each were specified to keep; two round-to-nearest terms guarantee only 2^-17 |w| (hi to 2^-8, lo to 2^-9 of a residual below
      2^-8 |w|), so the kernel adds a third term and the sum is the fp32 weight; a kernel that drops the third term shows where enough
      pixels meet a bad weight row (test_head_out_grid_stride).  fp16: hi + lo, 11 + 11 bits, 2^-24 sum |x w|, but lo may fall among
      fp16's subnormals (spacing 2^-24, error <= 2^-25 per weight) -> + 2^-25 sum |x|."""
    x64, w64 = _f64(x), _f64(w)
    cin = x64.shape[-1]
    ref = np.einsum("bpc,oc->bpo", x64, w64) + _f64(b)
    sxw = np.einsum("bpc,oc->bpo", np.abs(x64), np.abs(w64))
    tol = (cin + 2) * U * (sxw + np.abs(_f64(b))) + U * np.abs(ref)
    if matrix_cores:
        if dt == BF16:
            tol = tol + 2.0 ** -18 * sxw
        else:
            tol = tol + 2.0 ** -24 * sxw + 2.0 ** -25 * np.abs(x64).sum(-1)[..., None]
    return ref, tol


def head_input(rng, B, HW, cin, dt):
    return h16_round(rng.standard_normal((B, HW, cin)).astype(np.float32), dt)

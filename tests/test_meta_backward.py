"""The Meta-Kernel unit's backward (rd_meta_kernel_bwd_data, rd_meta_kernel_bwd_params, rangedet_amd.backward.MetaUnitBackward) against
tests/metabwd_model.py, in both tiers.  The kernels work on FRAGMENTS of 32 consecutive pixels of an image row (4 per chunk in the parameter
kernel, 8 per run in the data kernel), not on 8 x 32 tiles, so the edge shapes are: (1, 1, 1) all neighbours padded; (1, 8, 32) exactly two
chunks / one run; (1, 3, 31) a short fragment and a half-empty chunk; (2, 9, 33) a second fragment of one column per row, neighbours across
fragment seams, rows and the image index; (2, 17, 70) 102 fragments = 26 chunks with split 1, 3 (does not divide 26) and 0."""
import functools

import numpy as np
import pytest
import torch

import conv_model as CM
import meta_model as MM
import metabwd_model as M
import train_util as TU
from conftest import BOTH, HIP_ONLY
from rangedet_amd import lib as R

DTS = TU.DTS
PSHAPES = dict(dA=(64, 576), dW1=(64, 32), db1=(64,), dW0=(32, 3), db0=(32,), dt1=(576,), dq1=(576,))
PORDER = ("dA", "dW1", "db1", "dW0", "db0", "dt1", "dq1")


def nhwc(a):
    return np.ascontiguousarray(np.transpose(np.asarray(a, np.float32), (0, 2, 3, 1)))


def launch(be, prm, data, coord, dz, dt, split=0, layout=None, residual=None, what="data params"):
    """data, coord, dz NCHW float32 values (data, dz already rounded).  layout: (d_cs, d_co, z_cs, z_co, g_cs, g_co).  Every output and the
    workspace are 0xFF-prefilled with a guard tail.  -> {name: float32 array}"""
    L = be.lib
    B, _, H, W = data.shape
    d_cs, d_co, z_cs, z_co, g_cs, g_co = layout or (64, 0, 64, 0, 64, 0)
    packed = be.up(L.pack_meta_bwd(*M.pack_args(prm), dt))
    d_buf, z_buf = be.up(TU.image(nhwc(data), dt, d_cs, d_co)), be.up(TU.image(nhwc(dz), dt, z_cs, z_co))
    c_buf = be.up(np.ascontiguousarray(coord, dtype=np.float32))
    out = {}
    if "data" in what:
        g_buf = TU.ff(be, B * H * W * g_cs * 2)
        r_buf = None if residual is None else be.up(TU.image(residual, dt))
        L.call("rd_meta_kernel_bwd_data", be.ptr(z_buf), z_cs, z_co, be.ptr(d_buf), d_cs, d_co, be.ptr(c_buf), be.ptr(packed), be.ptr(r_buf), 64, 0,
               be.ptr(g_buf), g_cs, g_co, B, H, W, dt, be.stream)
        out["ddata_bits"] = TU.back_image(be, g_buf, (B, H, W, 64), g_cs, g_co, dt, "ddata").copy()
        out["ddata"] = TU.from_bits(out["ddata_bits"], dt)
    if "params" in what:
        nws = L.raw("rd_meta_kernel_bwd_workspace_bytes")(B, H, W, split)
        assert 0 < nws <= 9 * 6464 * 4 * max(1, min(split or 64, (B * H * ((W + 31) // 32) + 3) // 4))
        ws = TU.ff(be, nws)
        bufs = {k: TU.ff(be, int(np.prod(PSHAPES[k])) * 4) for k in PORDER}
        L.call("rd_meta_kernel_bwd_params", be.ptr(z_buf), z_cs, z_co, be.ptr(d_buf), d_cs, d_co, be.ptr(c_buf), be.ptr(packed),
               *[be.ptr(bufs[k]) for k in PORDER], B, H, W, split, dt, be.ptr(ws), nws, be.stream)
        TU.back(be, ws, nws, "workspace")
        for k in PORDER:
            out[k] = TU.back(be, bufs[k], int(np.prod(PSHAPES[k])) * 4, k).view(np.float32).reshape(PSHAPES[k]).copy()
    return out


# ---- exact family -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact(B, H, W, dt, centre_only=False):
    prm, data, coord, dz = M.exact_case(B, H, W, dt, seed=B + H + W, centre_only=centre_only)
    M.check_exact(data, coord, dz, prm, dt)
    ref = M.reference(data, coord, dz, prm, dt)
    for v in ref.values():
        v.setflags(write=False)
    return prm, data, coord, dz, ref


def assert_exact(got, ref, dt, what):
    for k in PORDER:
        bad = int((got[k] != ref[k].astype(np.float32)).sum())
        print(what, k, "elements that differ", bad, "max |ref|", float(np.abs(ref[k]).max()))
        assert TU.same_bits(got[k], ref[k]), (what, k, bad)
    want = TU.h16_round(ref["ddata"].astype(np.float32), dt)
    bad = int((got["ddata"] != want).sum())
    print(what, "ddata elements that differ", bad)
    assert TU.same_bits(got["ddata"], want), (what, bad)


EXACT = [(1, 1, 1, 0), (1, 8, 32, 0), (1, 3, 31, 0), (2, 9, 33, 0), (2, 17, 70, 1), (2, 17, 70, 3), (2, 17, 70, 0)]


@pytest.mark.parametrize("case", EXACT, ids=lambda c: "B%d_%dx%d_split%d" % c)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_exact(be, dt, case):
    """Integer inputs (metabwd_model.exact_case): every parameter gradient equals the float64 reference in every bit (-0 == +0) and ddata is
    its exact integer rounded once -- one dropped or doubled pixel, tap, fragment or partial shows at any reduction length."""
    B, H, W, split = case
    prm, data, coord, dz, ref = exact(B, H, W, dt)
    assert_exact(launch(be, prm, data, coord, dz, dt, split), ref, dt, "exact %r" % (case,))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_exact_in_wider_buffers(be, dt):
    """data at channels 16 .. 79 of an 80-channel buffer, dz at 64 .. 127 of 128, ddata at 8 .. 71 of 96: bytes outside stay as they were"""
    prm, data, coord, dz, ref = exact(2, 9, 33, dt)
    assert_exact(launch(be, prm, data, coord, dz, dt, 0, layout=(80, 16, 128, 64, 96, 8)), ref, dt, "wider buffers")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
def test_exact_full_width(be, dt):
    """(1, 8, 2656): the 83rd fragment of a row, several runs per workgroup, 166 chunks over 64 partials"""
    prm, data, coord, dz, ref = exact(1, 8, 2656, dt)
    assert_exact(launch(be, prm, data, coord, dz, dt, 0), ref, dt, "full width")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_centre_tap(be, dt):
    """A is zero off the centre tap: only w_4 = s1 (W1 relu(b0) + b1), a constant the packer folds, carries gradient.  dW1, db1 and db0 are
    non-zero and match the reference; dW0 is exactly zero (rel = 0 at the centre)."""
    prm, data, coord, dz, ref = exact(2, 9, 33, dt, centre_only=True)
    got = launch(be, prm, data, coord, dz, dt, 0, what="params")
    for k in ("dW1", "db1", "db0"):
        assert np.abs(ref[k]).max() > 0 and TU.same_bits(got[k], ref[k]), k
    assert (ref["dW0"] == 0).all() and (got["dW0"] == 0).all()
    assert TU.same_bits(got["dA"], ref["dA"]) and TU.same_bits(got["dt1"], ref["dt1"]) and TU.same_bits(got["dq1"], ref["dq1"])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_determinism_and_residual(be, dt):
    """two calls of each launch on 0xFF-filled outputs give identical bytes; the residual form equals float32(sum) + residual rounded once"""
    prm, data, coord, dz, ref = exact(2, 9, 33, dt)
    a, b = launch(be, prm, data, coord, dz, dt, 3), launch(be, prm, data, coord, dz, dt, 3)
    for k in PORDER + ("ddata_bits",):
        assert a[k].tobytes() == b[k].tobytes(), k
    res = TU.rnd("normal", (2, 9, 33, 64), dt, 77)
    got = launch(be, prm, data, coord, dz, dt, residual=res, what="data")
    want = TU.h16_round((ref["ddata"].astype(np.float32) + res).astype(np.float32), dt)      # the exact integer sum is a float32
    assert TU.same_bits(got["ddata"], want)


# ---- open-gate and realistic families -------------------------------------------------------------------------------------------------
CASES = [("range", 2, 9, 33, 1), ("cancel", 2, 9, 33, 0), ("normal", 2, 9, 33, 0), ("range", 1, 10, 70, 2)]
SHARE_CAP = {R.RD_BF16: 0.02, R.RD_F16: 0.003}


@functools.lru_cache(maxsize=None)
def synth_case(kind, B, H, W, pad, dt, open_gate):
    prm = M.folded(MM.weights(W), MM.NAME, W)
    data, coord = MM.make_inputs(kind, B, H, W, pad, dt)
    assert bool(torch.isfinite(data).all()) and bool(torch.isfinite(coord).all())
    dz = TU.h16_round(np.random.default_rng(31).standard_normal((B, 64, H, W)).astype(np.float32), dt)
    if open_gate:
        prm = M.open_gate(prm, data, coord, dt)
    ref = M.reference(data, coord, dz, prm, dt)
    bnd, shares = M.bounds(data, coord, dz, prm, dt)
    return prm, data.numpy(), coord.numpy(), dz, ref, bnd, shares


def judge(got, ref, bnd, dt, what, gate_term):
    """meta_model.per_element_stats / within_bounds with sigma' = sigma + (sum bound + gate term) / 7, so that its tol = 7 sigma' + u |ref| +
    1e-5 is 7 sigma + sum bound + gate term + u |ref| + 1e-5; u = half an ulp of the type on ddata, 0 on the float32 gradients"""
    ok = True
    for k in M.NAMES:
        sig, sb, gt = bnd[k]
        extra = sb + (gt if gate_term else 0.0)
        if k == "ddata":
            extra = extra + CM.half_ulp_of(ref[k], dt)             # half an ulp of the type, of the element's own binade
        u = 0.0
        worst, rms, nover, n = MM.per_element_stats(got[k], ref[k], sig + extra / 7.0, u)
        print("%s %-5s worst %.3f rms %.3f nover %d / %d" % (what, k, worst, rms, nover, n))
        ok = ok and MM.within_bounds(worst, rms, nover, n)
    return ok


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s_B%d_%dx%d" % c[:4])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_open_gate(be, dt, case):
    """synth weights with t1 = the smallest power of two that keeps every r_k of the reference above 7 sigma_r: no [r > 0] mask can disagree.
    Per element: 7 sigma of the documented roundings (own binade each) + the float32 sum bound + half an ulp on ddata; the [u > 0] gates within
    float32 slack of 0 add their |contribution|.
    Rounded float64 model of the contract (metabwd_model.rounded_model) against the reference under this bound, measured on the CPU over
    the four cases, both types and the eight gradients (test_model_margin prints every figure), worst / largest rms per gradient:
      gates open   ddata 0.55 / 0.82, dA 0.45 / 0.71, dW1 0.35 / 0.66, dW0 0.12 / 0.36, db0 0.09 / 0.23, dq1 0.32 / 0.65; dt1 and db1 carry no
                   rounding at all (0 / 0)
      as they are  ddata 1.03 / 0.83, dA 0.64 / 0.90, dW1 0.94 / 0.90, db1 0.62 / 0.85, dW0 0.38 / 1.04, db0 0.29 / 0.61, dt1 0.99 / 1.07,
                   dq1 0.86 / 0.83 (test_realistic; an element near 1 is one whose whole error is a flipped gate, i.e. the gate term itself)
    against the bounds worst <= 4, rms < 1.5 of meta_model.within_bounds."""
    prm, data, coord, dz, ref, bnd, shares = synth_case(*case, dt, True)
    assert shares[0] == 0.0
    assert judge(launch(be, prm, data, coord, dz, dt, 0), ref, bnd, dt, "open %s" % (case,), True)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s_B%d_%dx%d" % c[:4])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_realistic(be, dt, case):
    """synth weights and t1 as they are: the same tolerance plus the sum of |contribution| over the triples (p, c, k) with |r_k| <= 7 sigma_r.
    The cap on such triples is asserted on the reference alone: 2 % (bf16), 0.3 % (fp16)."""
    prm, data, coord, dz, ref, bnd, shares = synth_case(*case, dt, False)
    print("gate triples: r %.4f %%, u %.4f %%" % (100 * shares[0], 100 * shares[1]))
    assert shares[0] <= SHARE_CAP[dt] and shares[1] <= SHARE_CAP[dt]
    assert judge(launch(be, prm, data, coord, dz, dt, 0), ref, bnd, dt, "real %s" % (case,), True)


@pytest.mark.parametrize("dt", DTS)
def test_model_margin(dt):
    """the contract's own roundings (metabwd_model.rounded_model, float64) stay inside the bounds the kernels are held to"""
    for open_gate in (True, False):
        for case in CASES:
            prm, data, coord, dz, ref, bnd, shares = synth_case(*case, dt, open_gate)
            assert judge(M.rounded_model(data, coord, dz, prm, dt), ref, bnd, dt, "model open=%d %s" % (open_gate, case), True)


# ---- error paths ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_error_paths(be):
    """RD_F32, null pointers, misaligned strides and a short workspace are refused with their status codes before any launch: the outputs
    keep their 0xFF fill"""
    L, dt = be.lib, R.RD_BF16
    prm, data, coord, dz, ref = exact(1, 3, 31, dt)
    assert L.raw("rd_meta_bwd_packed_bytes")(R.RD_F32) == 0 and L.raw("rd_meta_bwd_packed_bytes")(dt) > 0
    arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in M.pack_args(prm)]
    scratch = np.zeros(L.raw("rd_meta_bwd_packed_bytes")(dt), np.uint8)
    assert L.raw("rd_pack_meta_bwd_host")(*[a.ctypes.data for a in arrs], R.RD_F32, scratch.ctypes.data) == R.RD_EINVAL
    B, H, W = 1, 3, 31
    packed = be.up(L.pack_meta_bwd(*M.pack_args(prm), dt))
    d, z, c = be.up(TU.image(nhwc(data), dt)), be.up(TU.image(nhwc(dz), dt)), be.up(coord)
    g = TU.ff(be, B * H * W * 128)
    nws = L.raw("rd_meta_kernel_bwd_workspace_bytes")(B, H, W, 0)
    ws = TU.ff(be, nws)
    outs = [TU.ff(be, int(np.prod(PSHAPES[k])) * 4) for k in PORDER]
    P = be.ptr

    def data_call(**kw):
        a = dict(dz=P(z), zcs=64, zco=0, data=P(d), dcs=64, dco=0, coord=P(c), packed=P(packed), res=None, gd=P(g), gcs=64, gco=0, dt=dt)
        a.update(kw)
        return L.raw("rd_meta_kernel_bwd_data")(a["dz"], a["zcs"], a["zco"], a["data"], a["dcs"], a["dco"], a["coord"], a["packed"], a["res"], 64, 0,
                                                a["gd"], a["gcs"], a["gco"], B, H, W, a["dt"], be.stream)

    def params_call(**kw):
        a = dict(dz=P(z), zcs=64, data=P(d), outs=[P(o) for o in outs], split=0, dt=dt, ws=P(ws), nws=nws)
        a.update(kw)
        return L.raw("rd_meta_kernel_bwd_params")(a["dz"], a["zcs"], 0, a["data"], 64, 0, P(c), P(packed), *a["outs"], B, H, W, a["split"], a["dt"],
                                                  a["ws"], a["nws"], be.stream)

    assert data_call(dt=R.RD_F32) == R.RD_EINVAL and params_call(dt=R.RD_F32) == R.RD_EINVAL
    assert data_call(dz=None) == R.RD_EINVAL and data_call(gd=None) == R.RD_EINVAL and data_call(packed=None) == R.RD_EINVAL
    assert params_call(data=None) == R.RD_EINVAL and params_call(ws=None) == R.RD_EINVAL
    assert params_call(outs=[P(o) for o in outs[:3]] + [None] + [P(o) for o in outs[4:]]) == R.RD_EINVAL
    assert data_call(zcs=68) == R.RD_ESHAPE and data_call(gco=4) == R.RD_ESHAPE and data_call(dcs=64, dco=8) == R.RD_ESHAPE
    assert params_call(zcs=60) == R.RD_ESHAPE and params_call(split=-1) == R.RD_EINVAL
    assert params_call(nws=nws - 4) == R.RD_EWORKSPACE
    assert b"workspace" in L.rd_last_error_string()
    assert L.raw("rd_meta_kernel_bwd_workspace_bytes")(0, 3, 31, 0) == 0
    for buf, n in [(g, B * H * W * 128), (ws, nws)] + [(o, int(np.prod(PSHAPES[k])) * 4) for o, k in zip(outs, PORDER)]:
        assert (TU.back(be, buf, n, "refused call") == 0xFF).all()


def test_workspace_cap():
    """partial sums only: below 64 MiB at B = 8, 64 x 2656 with the library's own split"""
    from emu_util import emu_lib
    n = emu_lib().raw("rd_meta_kernel_bwd_workspace_bytes")(8, 64, 2656, 0)
    assert 0 < n < 64 << 20


# ---- MetaUnitBackward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_meta_unit_backward(be, dt):
    from rangedet_amd.backward import MetaUnitBackward, meta_kernel_data_grad, meta_kernel_param_grads
    B, H, W = 2, 9, 33
    P = MM.weights(W)
    name = MM.NAME
    prm = M.folded(P, name, W)
    data, coord = MM.make_inputs("range", B, H, W, 1, dt)
    unit = MetaUnitBackward(name, P, W, dtype=dt, lib=be.lib, alloc=be.alloc)
    x = TU.dev16(be, TU.to_bits(nhwc(data.numpy()), dt), dt)
    cd = be.up(coord.numpy())
    cview = be.alloc.view_f32(cd, (B, 3, H, W))
    g = TU.dev16(be, TU.to_bits(TU.rnd("normal", (B, H, W, 64), dt, 5), dt), dt)
    with pytest.raises(RuntimeError):
        unit.backward(g)
    y = unit.forward(x, cview)
    # forward() is rd_meta_kernel_fwd, byte for byte
    packed = be.up(be.lib.pack_meta(*M.pack_args(prm), dt))
    ybuf = TU.ff(be, B * H * W * 128)
    be.lib.call("rd_meta_kernel_fwd", R.ptr(x), 64, 0, be.ptr(cd), be.ptr(packed), be.ptr(ybuf), 64, 0, B, H, W, dt, be.stream)
    yraw = TU.back(be, ybuf, B * H * W * 128, "y").view(np.uint16).reshape(B, H, W, 64)
    ybits = TU.to_bits(TU.vals16(be, y, dt), dt)
    assert ybits.tobytes() == yraw.tobytes()
    res = TU.dev16(be, TU.to_bits(TU.rnd("normal", (B, H, W, 64), dt, 6), dt), dt)
    ddata, grads = unit.backward(g, residual=res)
    shapes = {"%s_%d_mlp0_weight" % (name, W): (32, 3, 1, 1), "%s_%d_mlp0_bias" % (name, W): (32,), "%s_%d_mlp1_weight" % (name, W): (64, 32, 1, 1),
              "%s_%d_mlp1_bias" % (name, W): (64,), name + "point_wise_mlp_bn1_gamma": (576,), name + "point_wise_mlp_bn1_beta": (576,),
              name + "aggregation_conv1_weight": (64, 576, 1, 1)}
    assert set(grads) == set(shapes)
    gn = {k: np.array(be.alloc.to_numpy(v), np.float32) for k, v in grads.items()}
    for k, s in shapes.items():
        assert gn[k].shape == s and gn[k].dtype == np.float32 and np.isfinite(gn[k]).all(), k
    # the single steps give the same bytes, and gamma / beta follow from dq1 / dt1
    yv, gv = TU.vals16(be, y, dt), TU.vals16(be, g, dt)
    import convbwd_model as CB
    dzv = CB.relu_affine_bwd(gv, yv, prm["s2"], dt)
    dz = TU.dev16(be, TU.to_bits(dzv, dt), dt)
    single = meta_kernel_param_grads(dz, x, cview, prm, dtype=dt, lib=be.lib, alloc=be.alloc)
    single = {k: np.array(be.alloc.to_numpy(v), np.float32) for k, v in single.items()}
    assert single["dA"].tobytes() == gn[name + "aggregation_conv1_weight"].tobytes()
    assert single["dt1"].tobytes() == gn[name + "point_wise_mlp_bn1_beta"].tobytes()
    gamma = np.asarray(P[name + "point_wise_mlp_bn1_gamma"], np.float32)
    assert np.array_equal(gn[name + "point_wise_mlp_bn1_gamma"], single["dq1"] / gamma)
    dd = meta_kernel_data_grad(dz, x, cview, prm, residual=res, dtype=dt, lib=be.lib, alloc=be.alloc)
    assert TU.to_bits(TU.vals16(be, dd, dt), dt).tobytes() == TU.to_bits(TU.vals16(be, ddata, dt), dt).tobytes()
    P0 = dict(P)
    P0[name + "point_wise_mlp_bn1_gamma"] = np.array(gamma)
    P0[name + "point_wise_mlp_bn1_gamma"][5] = 0.0
    with pytest.raises(ValueError):
        MetaUnitBackward(name, P0, W, dtype=dt, lib=be.lib, alloc=be.alloc)

"""The Meta-Kernel unit in training mode (rd_meta_kernel_stats, rd_meta_kernel_fwd_train, rd_meta_kernel_bwd_sums,
rd_meta_kernel_bwd_params_train, rd_meta_kernel_bwd_data_train, rd_pack_meta_dev; rangedet_amd.backward.MetaUnitTrain and the optimizer's
re-pack) against tests/metatrain_model.py, in both tiers.  The kernels work on fragments of 32 consecutive pixels of an image row, so the
shapes are test_meta_backward.py's: (1, 1, 1) every neighbour padded; (1, 8, 32) two chunks / one run; (1, 3, 31) a short fragment;
(2, 9, 33) a second fragment of one column per row, seams across fragments, rows and images -- and the 8 x 32 edge in both axes;
(2, 17, 70) 26 chunks with split 1, 3 and 0; (1, 8, 2656) on the GPU only: the 83rd fragment of a row, several runs per workgroup."""
import functools

import numpy as np
import pytest

import meta_model as MM
import metabwd_model as MB
import metatrain_model as T
import optim_model as OM
import train_util as TU
from conftest import BOTH, HIP_ONLY
from rangedet_amd import lib as R

DTS = TU.DTS
TABS = ("a1", "bb1", "mean1", "rstd1", "c1", "c2")
SHAPES = dict(dA=(64, 576), dbeta1=(576,), dgamma1=(576,), c1=(576,), c2=(576,), dW1=(64, 32), db1=(64,), dW0=(32, 3), db0=(32,))
SUMS, PARAMS = ("dA", "dbeta1", "dgamma1", "c1", "c2"), ("dW1", "db1", "dW0", "db0")
MASTERS = ("w0", "b0", "w1", "b1", "agg")


def nhwc(a):
    return np.ascontiguousarray(np.transpose(np.asarray(a, np.float32), (0, 2, 3, 1)))


def blocks(be, prm, dt):
    L = be.lib
    return be.up(L.pack_meta(*MB.pack_args(T.unit(prm)), dt)), be.up(L.pack_meta_bwd(*MB.pack_args(T.unit(prm)), dt))


def launch(be, prm, data, coord, dz, tabs, dt, split=0, layout=None, residual=None, what="stats fwd sums params data"):
    """data, coord, dz NCHW float32 values (data, dz already rounded); tabs: the six tables.  layout: (d_cs, d_co, z_cs, z_co, g_cs, g_co),
    z_* for dz and for the forward's z, g_* for ddata.  Every output and workspace is 0xFF-prefilled with a guard tail."""
    L, P = be.lib, be.ptr
    B, _, H, W = data.shape
    d_cs, d_co, z_cs, z_co, g_cs, g_co = layout or (64, 0, 64, 0, 64, 0)
    pf, pb = blocks(be, prm, dt)
    d_buf, c_buf = be.up(TU.image(nhwc(data), dt, d_cs, d_co)), be.up(np.ascontiguousarray(coord, dtype=np.float32))
    z_buf = be.up(TU.image(nhwc(dz), dt, z_cs, z_co))
    t = {k: be.up(np.ascontiguousarray(tabs[k], dtype=np.float32)) for k in TABS} if tabs is not None else {}
    out = {}

    def f32(bufs, names):
        for k in names:
            out[k] = TU.back(be, bufs[k], int(np.prod(SHAPES[k])) * 4, k).view(np.float32).reshape(SHAPES[k]).copy()
    if "stats" in what:
        nws = L.raw("rd_meta_kernel_stats_workspace_bytes")(B, H, W, split)
        assert 0 < nws <= 9 * 256 * 4 * max(1, min(split or 64, (B * H * ((W + 31) // 32) + 3) // 4))
        ws, mean, var = TU.ff(be, nws), TU.ff(be, 576 * 4), TU.ff(be, 576 * 4)
        L.call("rd_meta_kernel_stats", P(d_buf), d_cs, d_co, P(c_buf), P(pb), P(mean), P(var), B, H, W, split, dt, P(ws), nws, be.stream)
        TU.back(be, ws, nws, "stats workspace")
        out["mean1"] = TU.back(be, mean, 576 * 4, "mean1").view(np.float32).copy()
        out["var1"] = TU.back(be, var, 576 * 4, "var1").view(np.float32).copy()
    if "fwd" in what:
        zo = TU.ff(be, B * H * W * z_cs * 2)
        L.call("rd_meta_kernel_fwd_train", P(d_buf), d_cs, d_co, P(c_buf), P(pf), P(pb), P(t["a1"]), P(t["bb1"]), P(zo), z_cs, z_co, B, H, W, dt,
               be.stream)
        out["z_bits"] = TU.back_image(be, zo, (B, H, W, 64), z_cs, z_co, dt, "z").copy()
        out["z"] = TU.from_bits(out["z_bits"], dt)
    nws = L.raw("rd_meta_kernel_bwd_train_workspace_bytes")(B, H, W, split)
    assert 0 < nws <= 9 * 4224 * 4 * max(1, min(split or 64, (B * H * ((W + 31) // 32) + 3) // 4))
    if "sums" in what:
        ws = TU.ff(be, nws)
        bufs = {k: TU.ff(be, int(np.prod(SHAPES[k])) * 4) for k in SUMS}
        L.call("rd_meta_kernel_bwd_sums", P(z_buf), z_cs, z_co, P(d_buf), d_cs, d_co, P(c_buf), P(pb), *[P(t[k]) for k in TABS[:4]],
               *[P(bufs[k]) for k in SUMS], B, H, W, split, dt, P(ws), nws, be.stream)
        TU.back(be, ws, nws, "pass A workspace")
        f32(bufs, SUMS)
    if "params" in what:
        ws = TU.ff(be, nws)
        bufs = {k: TU.ff(be, int(np.prod(SHAPES[k])) * 4) for k in PARAMS}
        L.call("rd_meta_kernel_bwd_params_train", P(z_buf), z_cs, z_co, P(d_buf), d_cs, d_co, P(c_buf), P(pb), *[P(t[k]) for k in TABS],
               *[P(bufs[k]) for k in PARAMS], B, H, W, split, dt, P(ws), nws, be.stream)
        TU.back(be, ws, nws, "pass B workspace")
        f32(bufs, PARAMS)
    if "data" in what:
        g_buf = TU.ff(be, B * H * W * g_cs * 2)
        r_buf = None if residual is None else be.up(TU.image(residual, dt))
        L.call("rd_meta_kernel_bwd_data_train", P(z_buf), z_cs, z_co, P(d_buf), d_cs, d_co, P(c_buf), P(pb), *[P(t[k]) for k in TABS], P(r_buf), 64, 0,
               P(g_buf), g_cs, g_co, B, H, W, dt, be.stream)
        out["ddata_bits"] = TU.back_image(be, g_buf, (B, H, W, 64), g_cs, g_co, dt, "ddata").copy()
        out["ddata"] = TU.from_bits(out["ddata_bits"], dt)
    return out


# ---- exact family, with given tables -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact(B, H, W, dt, centre_only=False):
    prm, data, coord, dz, tabs = T.exact_case(B, H, W, dt, seed=B + H + W, centre_only=centre_only)
    ref = T.check_exact(data, coord, dz, prm, tabs, dt)
    return prm, data, coord, dz, tabs, ref


def assert_exact(got, ref, tabs, n, dt, what):
    for k in T.GRADS:
        bad = int((got[k] != ref[k].astype(np.float32)).sum())
        print(what, k, "elements that differ", bad, "max |ref|", float(np.abs(ref[k]).max()))
        assert TU.same_bits(got[k], ref[k]), (what, k, bad)
    assert TU.same_bits(got["c1"], ref["dbeta1"].astype(np.float32) / np.float32(n))
    assert TU.same_bits(got["c2"], ref["dgamma1"].astype(np.float32) / np.float32(n))
    for k in ("z", "ddata"):
        want = TU.h16_round(ref[k].astype(np.float32), dt)               # the exact value is a float32; one rounding to the type
        bad = int((got[k] != want).sum())
        print(what, k, "elements that differ", bad)
        assert TU.same_bits(got[k], want), (what, k, bad)


def judge_exact_stats(got, prm, data, coord, dt, split, what):
    """mean1 / var1 of the exact family's q (integers: float64 statistics are exact) under metatrain_model.stats_bound"""
    B, _, H, W = data.shape
    Q, EQ = T.q_matrix(T.front(data, coord, prm, dt))
    (m, v), (bm, bv) = T.stats_exact(Q), T.stats_bound(Q, EQ, T.runs(B, H, W, split))
    em, ev = np.abs(got["mean1"].astype(np.float64) - m), np.abs(got["var1"].astype(np.float64) - v)
    ratio = lambda e, b: float(np.where(b > 0, e / np.where(b > 0, b, 1.0), np.where(e > 0, np.inf, 0.0)).max())     # a zero bound: an exact value
    print("%s mean worst err / bound %.3f, var %.3f" % (what, ratio(em, bm), ratio(ev, bv)))
    return bool((em <= bm).all() and (ev <= bv).all())


EXACT = [(1, 1, 1, 0), (1, 8, 32, 0), (1, 3, 31, 0), (2, 9, 33, 0), (2, 17, 70, 1), (2, 17, 70, 3), (2, 17, 70, 0)]
BWD = "fwd sums params data"


@pytest.mark.parametrize("case", EXACT, ids=lambda c: "B%d_%dx%d_split%d" % c)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_exact(be, dt, case):
    """Integer inputs and representable tables (metatrain_model.exact_case): z, dA, dbeta1, dgamma1, dW1, db1, dW0, db0 equal the float64
    model in every bit, ddata and z are the exact value rounded once.  The tables are GIVEN (not the batch's): c1 != 0 and c2 != 0 in two
    thirds of the channels, so every masked tap carries a non-zero dq."""
    B, H, W, split = case
    prm, data, coord, dz, tabs, ref = exact(B, H, W, dt)
    assert_exact(launch(be, prm, data, coord, dz, tabs, dt, split, what=BWD), ref, tabs, B * H * W, dt, "exact %r" % (case,))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_masked_and_border_taps_carry_dq(be, dt):
    """the term a frozen-statistics kernel gets wrong: triples with gy = 0 (mask closed, or dz making da = 0) whose dq = -a1 (c1 + xh c2) is
    not zero and whose data is not zero exist in the case (asserted on the model), and the gradients that sum them are exact"""
    prm, data, coord, dz, tabs, ref = exact(2, 9, 33, dt)
    p = ref["parts"]
    x = T.front(data, coord, prm, dt)["x"]
    closed = (p["gy"] == 0) & (p["dq"] != 0) & (x != 0)
    print("triples with gy = 0, dq != 0, data != 0: %d of %d" % (int(closed.sum()), closed.size))
    assert closed.sum() > closed.size // 20
    border = (x == 0).all(1, keepdims=True) & (p["dq"] != 0)           # a padded tap: data = 0, r = bb1, dq != 0, e = 0
    assert border.sum() > 0
    got = launch(be, prm, data, coord, dz, tabs, dt, 0, what="sums params data")
    for k in ("dbeta1", "dgamma1", "dW1", "db1", "dW0", "db0"):
        assert TU.same_bits(got[k], ref[k]), k
    assert TU.same_bits(got["ddata"], TU.h16_round(ref["ddata"].astype(np.float32), dt))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_exact_in_wider_buffers(be, dt):
    """data at channels 16 .. 79 of an 80-channel buffer, dz and z at 64 .. 127 of 128, ddata at 8 .. 71 of 96: bytes outside stay"""
    prm, data, coord, dz, tabs, ref = exact(2, 9, 33, dt)
    got = launch(be, prm, data, coord, dz, tabs, dt, 0, layout=(80, 16, 128, 64, 96, 8), what=BWD + " stats")
    assert_exact(got, ref, tabs, 2 * 9 * 33, dt, "wider")
    assert judge_exact_stats(got, prm, data, coord, dt, 0, "wider")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
def test_exact_full_width(be, dt):
    """(1, 8, 2656): the 83rd fragment of a row, several runs per workgroup, 166 chunks over 64 partials"""
    prm, data, coord, dz, tabs, ref = exact(1, 8, 2656, dt)
    got = launch(be, prm, data, coord, dz, tabs, dt, 0, what=BWD + " stats")
    assert_exact(got, ref, tabs, 8 * 2656, dt, "full width")
    assert judge_exact_stats(got, prm, data, coord, dt, 0, "full width")      # 166 chunks over 64 runs, every row ends in a full fragment


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_centre_tap(be, dt):
    """A is zero off the centre tap: only the packer's folded constant w_4 carries gradient; dW0 is exactly zero"""
    prm, data, coord, dz, tabs, ref = exact(2, 9, 33, dt, centre_only=True)
    got = launch(be, prm, data, coord, dz, dict(tabs, c1=np.zeros(576, np.float32), c2=np.zeros(576, np.float32)), dt, 0, what="sums params")
    ref0 = T.model(data, coord, dz, prm, dict(tabs, c1=np.zeros(576), c2=np.zeros(576)), dt)
    for k in ("dW1", "db1", "db0"):
        assert np.abs(ref0[k]).max() > 0 and TU.same_bits(got[k], ref0[k]), k
    assert (ref0["dW0"] == 0).all() and (got["dW0"] == 0).all()
    assert TU.same_bits(got["dA"], ref0["dA"]) and TU.same_bits(got["dbeta1"], ref0["dbeta1"]) and TU.same_bits(got["dgamma1"], ref0["dgamma1"])
    assert_exact(launch(be, prm, data, coord, dz, tabs, dt, 0, what=BWD), ref, tabs, 2 * 9 * 33, dt, "centre only, c1 c2 != 0")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_determinism_and_residual(be, dt):
    """two calls of every launch on 0xFF-filled outputs give identical bytes; the residual form equals float32(sum) + residual rounded once"""
    prm, data, coord, dz, tabs, ref = exact(2, 9, 33, dt)
    a, b = launch(be, prm, data, coord, dz, tabs, dt, 3), launch(be, prm, data, coord, dz, tabs, dt, 3)
    for k in SUMS + PARAMS + ("ddata_bits", "z_bits", "mean1", "var1"):
        assert a[k].tobytes() == b[k].tobytes(), k
    res = TU.rnd("normal", (2, 9, 33, 64), dt, 77)
    got = launch(be, prm, data, coord, dz, tabs, dt, residual=res, what="data")
    want = TU.h16_round((ref["ddata"].astype(np.float32) + res).astype(np.float32), dt)
    assert TU.same_bits(got["ddata"], want)


# ---- statistics ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 3, 31), (2, 9, 33), (2, 17, 70)], ids=lambda s: "B%d_%dx%d" % s)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_stats_constant_centre_tap(be, dt, shape):
    """data is 3 everywhere: the centre tap's q is the constant 3 w_4[c] (synth weights: w_4 is no integer), so mean1[c, 4] is that float32
    product in every bit and var1[c, 4] is exactly 0 -- a pilot that is not one of the values, or sums about zero, cannot give that"""
    B, H, W = shape
    prm = T.unit(MB.folded(MM.weights(W), MM.NAME, W))
    data = np.full((B, 64, H, W), 3.0, np.float32)
    coord = (np.random.default_rng(B + H + W).standard_normal((B, 3, H, W)) * 20).astype(np.float32)   # (the centre tap reads none of it)
    got = launch(be, prm, data, coord, data, None, dt, 3, what="stats")
    want = (np.float32(3.0) * T.centre_const(prm).astype(np.float32)).astype(np.float32)
    assert TU.same_bits(got["mean1"].reshape(64, 9)[:, 4], want)
    assert (got["var1"].reshape(64, 9)[:, 4] == 0).all()


STAT_CASES = [("range", 2, 9, 33, 1, 0), ("cancel", 2, 9, 33, 0, 3), ("normal", 2, 17, 70, 0, 0), ("range", 1, 10, 70, 2, 1)]


@functools.lru_cache(maxsize=None)
def stat_case(kind, B, H, W, pad, split, dt):
    prm = T.unit(MB.folded(MM.weights(W), MM.NAME, W))
    data, coord = MM.make_inputs(kind, B, H, W, pad, dt)
    f = T.front(data.numpy(), coord.numpy(), prm, dt)
    Q, EQ = T.q_matrix(f)
    rr = T.runs(B, H, W, split)
    return prm, data.numpy(), coord.numpy(), Q, T.stats_exact(Q), T.stats_bound(Q, EQ, rr), rr


def judge_stats(mean, var, case, what):
    (m, v), (bm, bv) = case[4], case[5]
    em, ev = np.abs(mean.astype(np.float64) - m), np.abs(var.astype(np.float64) - v)
    wm, wv = float((em / bm).max()), float((ev / bv).max())
    print("%s mean worst err / bound %.3f, var %.3f" % (what, wm, wv))
    return wm <= 1 and wv <= 1


@pytest.mark.parametrize("case", STAT_CASES, ids=lambda c: "%s_B%d_%dx%d" % c[:4])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_stats_per_element(be, dt, case):
    """mean1 and var1 per element against float64 statistics of the model's q (which shares contract points 1 - 3 bit for bit), under
    metatrain_model.stats_bound: norm_model's construction on this launch's runs and pilots, float32 sum terms only.
    The documented scheme restated with exact long sums (test_stats_model_margin, CPU, both types, four cases) uses at most 0.009 of the
    mean's bound and 0.008 of the variance's; the launches themselves, on the MI355X, at most 0.022 and 0.053."""
    c = stat_case(*case, dt)
    got = launch(be, c[0], c[1], c[2], c[1], None, dt, case[5], what="stats")
    assert judge_stats(got["mean1"], got["var1"], c, "stats %r" % (case,))


@pytest.mark.parametrize("dt", DTS)
def test_stats_model_margin(dt):
    for case in STAT_CASES:
        c = stat_case(*case, dt)
        mean, var = T.stats_f64(c[3], c[6])
        assert judge_stats(mean, var, c, "scheme %r" % (case,))


# ---- the device packer -------------------------------------------------------------------------------------------------------------------
def pack_sets(W=70):
    rng = np.random.default_rng(3)
    synth = MB.folded(MM.weights(W), MM.NAME, W)
    neg = dict(synth, b0=np.where(np.arange(32) % 3 == 0, 0.0, -np.abs(synth["b0"]) * (np.arange(32) % 3 - 1.5)).astype(np.float32))
    low = dict(synth, w0=(synth["w0"] * np.float32(1 + 2.0 ** -9) + np.float32(2.0 ** -11)).astype(np.float32),
               b0=(rng.standard_normal(32) * 1.2345678).astype(np.float32))
    ints = MB.exact_case(1, 1, 1, R.RD_BF16, seed=5)[0]
    return dict(synth=synth, neg_zero_b0=neg, low_part=low, ints=ints)


@pytest.mark.parametrize("which", ["synth", "neg_zero_b0", "low_part", "ints"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_pack_meta_dev(be, dt, which):
    """both blocks byte-equal to rd_pack_meta_host / rd_pack_meta_bwd_host with s1 = s2 = 1, t1 = t2 = 0: the 16-bit roundings, the high + low
    split of W0 / b0 and the centre tap's fold in double"""
    L, prm = be.lib, T.unit(pack_sets()[which])
    if which == "low_part":
        hi = TU.h16_round(prm["w0"], dt)
        assert (TU.h16_round(prm["w0"] - hi, dt) != 0).any()
    want_f, want_b = L.pack_meta(*MB.pack_args(prm), dt), L.pack_meta_bwd(*MB.pack_args(prm), dt)
    nf, nb = L.raw("rd_meta_packed_bytes")(dt), L.raw("rd_meta_bwd_packed_bytes")(dt)
    pf, pb = TU.ff(be, nf), TU.ff(be, nb)
    m = [be.up(np.ascontiguousarray(prm[k], dtype=np.float32)) for k in MASTERS]
    L.call("rd_pack_meta_dev", *[be.ptr(v) for v in m], be.ptr(pf), be.ptr(pb), dt, be.stream)
    got_f, got_b = TU.back(be, pf, nf, "forward block"), TU.back(be, pb, nb, "backward block")
    assert got_f.tobytes() == np.asarray(want_f).tobytes()[:nf], "forward block: %d bytes differ" % int((got_f != np.asarray(want_f)[:nf]).sum())
    assert got_b.tobytes() == np.asarray(want_b).tobytes()[:nb], "backward block: %d bytes differ" % int((got_b != np.asarray(want_b)[:nb]).sum())


# ---- error paths -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_error_paths(be):
    """RD_F32, null pointers, misaligned strides, a short workspace and split < 0 are refused with their status codes before any launch:
    the outputs keep their 0xFF fill"""
    L, dt, P = be.lib, R.RD_BF16, be.ptr
    prm, data, coord, dz, tabs, ref = exact(1, 3, 31, dt)
    B, H, W = 1, 3, 31
    pf, pb = blocks(be, prm, dt)
    d, z, c = be.up(TU.image(nhwc(data), dt)), be.up(TU.image(nhwc(dz), dt)), be.up(coord)
    t = [P(be.up(np.ascontiguousarray(tabs[k], dtype=np.float32))) for k in TABS]
    nimg = B * H * W * 128
    g, zo = TU.ff(be, nimg), TU.ff(be, nimg)
    nst, nws = L.raw("rd_meta_kernel_stats_workspace_bytes")(B, H, W, 0), L.raw("rd_meta_kernel_bwd_train_workspace_bytes")(B, H, W, 0)
    wst, ws = TU.ff(be, nst), TU.ff(be, nws)
    o = {k: TU.ff(be, int(np.prod(SHAPES[k])) * 4) for k in SUMS + PARAMS}
    mv = [TU.ff(be, 576 * 4), TU.ff(be, 576 * 4)]
    fp, fb = TU.ff(be, L.raw("rd_meta_packed_bytes")(dt)), TU.ff(be, L.raw("rd_meta_bwd_packed_bytes")(dt))
    m = [P(be.up(np.ascontiguousarray(prm[k], dtype=np.float32))) for k in MASTERS]

    def stats(data=P(d), dcs=64, dco=0, pb_=P(pb), mean=P(mv[0]), split=0, dt_=dt, ws_=P(wst), n=nst):
        return L.raw("rd_meta_kernel_stats")(data, dcs, dco, P(c), pb_, mean, P(mv[1]), B, H, W, split, dt_, ws_, n, be.stream)

    def fwd(data=P(d), pf_=P(pf), a1=t[0], zo_=P(zo), zcs=64, zco=0, dt_=dt):
        return L.raw("rd_meta_kernel_fwd_train")(data, 64, 0, P(c), pf_, P(pb), a1, t[1], zo_, zcs, zco, B, H, W, dt_, be.stream)

    def sums(dz_=P(z), zcs=64, tab0=t[0], dA=P(o["dA"]), split=0, dt_=dt, ws_=P(ws), n=nws):
        return L.raw("rd_meta_kernel_bwd_sums")(dz_, zcs, 0, P(d), 64, 0, P(c), P(pb), tab0, *t[1:4], dA, *[P(o[k]) for k in SUMS[1:]], B, H, W, split,
                                                dt_, ws_, n, be.stream)

    def params(dz_=P(z), dcs=64, c2=t[5], db0=P(o["db0"]), split=0, dt_=dt, ws_=P(ws), n=nws):
        return L.raw("rd_meta_kernel_bwd_params_train")(dz_, 64, 0, P(d), dcs, 0, P(c), P(pb), *t[:5], c2, *[P(o[k]) for k in PARAMS[:3]], db0, B, H, W,
                                                        split, dt_, ws_, n, be.stream)

    def dgrad(dz_=P(z), mean=t[2], gd=P(g), gcs=64, gco=0, dt_=dt):
        return L.raw("rd_meta_kernel_bwd_data_train")(dz_, 64, 0, P(d), 64, 0, P(c), P(pb), t[0], t[1], mean, *t[3:], None, 64, 0, gd, gcs, gco, B, H, W,
                                                      dt_, be.stream)

    def pack(w0=m[0], fwd_=P(fp), dt_=dt):
        return L.raw("rd_pack_meta_dev")(w0, *m[1:], fwd_, P(fb), dt_, be.stream)

    E, S, WS = R.RD_EINVAL, R.RD_ESHAPE, R.RD_EWORKSPACE
    for call in (stats, fwd, sums, params, dgrad, pack):
        assert call(dt_=R.RD_F32) == E, call.__name__
    assert stats(data=None) == E and stats(pb_=None) == E and stats(mean=None) == E and stats(ws_=None) == E
    assert fwd(pf_=None) == E and fwd(a1=None) == E and fwd(zo_=None) == E
    assert sums(dz_=None) == E and sums(tab0=None) == E and sums(dA=None) == E and sums(ws_=None) == E
    assert params(dz_=None) == E and params(c2=None) == E and params(db0=None) == E
    assert dgrad(dz_=None) == E and dgrad(mean=None) == E and dgrad(gd=None) == E
    assert pack(w0=None) == E and pack(fwd_=None) == E
    assert stats(dcs=68) == S and stats(dcs=64, dco=8) == S and fwd(zcs=60) == S and fwd(zco=4) == S
    assert sums(zcs=68) == S and params(dcs=60) == S and dgrad(gco=4) == S and dgrad(gcs=72, gco=16) == S
    assert stats(split=-1) == E and sums(split=-1) == E and params(split=-1) == E
    assert stats(n=nst - 4) == WS and sums(n=nws - 4) == WS and params(n=nws - 4) == WS
    assert b"workspace" in L.rd_last_error_string()
    assert L.raw("rd_meta_kernel_stats_workspace_bytes")(0, 3, 31, 0) == 0 and L.raw("rd_meta_kernel_bwd_train_workspace_bytes")(1, 3, 31, -1) == 0
    sizes = [(g, nimg), (zo, nimg), (wst, nst), (ws, nws), (mv[0], 2304), (mv[1], 2304), (fp, L.raw("rd_meta_packed_bytes")(dt)),
             (fb, L.raw("rd_meta_bwd_packed_bytes")(dt))] + [(o[k], int(np.prod(SHAPES[k])) * 4) for k in o]
    for buf, n in sizes:
        assert (TU.back(be, buf, n, "refused call") == 0xFF).all()


def test_workspace_cap():
    """partial sums only: split x 9 x 256 floats (statistics) and split x 9 x 4224 floats (both backward passes), split 64 by default"""
    from emu_util import emu_lib
    L = emu_lib()
    assert L.raw("rd_meta_kernel_stats_workspace_bytes")(8, 64, 2656, 0) == 64 * 9 * 256 * 4
    assert L.raw("rd_meta_kernel_bwd_train_workspace_bytes")(8, 64, 2656, 0) == 64 * 9 * 4224 * 4
    assert L.raw("rd_meta_kernel_bwd_train_workspace_bytes")(8, 64, 2656, 7) == 7 * 9 * 4224 * 4
    assert L.raw("rd_meta_kernel_bwd_train_workspace_bytes")(1, 1, 1, 0) == 9 * 4224 * 4


# ---- the contract's formulas are the gradient of the batch-statistics unit -----------------------------------------------------------------
def unit_case(B, H, W, dt, seed=11):
    P = MM.weights(W)
    name = MM.NAME
    prm = T.unit(MB.folded(P, name, W))
    data, coord = MM.make_inputs("range", B, H, W, 1, dt)
    g = TU.rnd("normal", (B, H, W, 64), dt, seed)
    norm = [np.asarray(P[name + k], np.float32) for k in ("point_wise_mlp_bn1_gamma", "point_wise_mlp_bn1_beta", "aggregation_bn1_gamma",
                                                          "aggregation_bn1_beta")]
    return P, name, prm, data.numpy(), coord.numpy(), g, norm


@pytest.mark.parametrize("dt", DTS)
def test_model_is_the_batch_norm_gradient(dt):
    """MODEL-ONLY check (no kernel runs; the kernels meet autograd in test_unit_against_autograd).
    metatrain_model.model fed with the batch's own tables (float64, nothing rounded behind h) against float64 torch autograd of the un-fused
    formulation with F.batch_norm(training=True) on both norms: the two-pass formulas with c1, c2 ARE the gradient, for all eleven parameters,
    ddata and y.  Both sides are float64 (u = 1.1e-16) over sums of at most 3.5e5 terms; 1e-9 of the output's largest magnitude leaves
    four decades for the normalisations' conditioning.  The kernels meet this model bit for bit on the exact family (test_exact)."""
    from rangedet_amd.backward import BN_EPS
    B, H, W = 2, 9, 33
    P, name, prm, data, coord, g, norm = unit_case(B, H, W, dt)
    gn = np.ascontiguousarray(g.transpose(0, 3, 1, 2))
    ref = T.autograd_reference(data, coord, gn, prm, *norm, dt, BN_EPS)
    got = T.model_with_batch_tables(data, coord, gn, prm, *norm, dt, BN_EPS)
    pairs = dict(dA=ref["A"].reshape(64, 576), dW1=ref["w1"], db1=ref["b1"], dW0=ref["w0"], db0=ref["b0"], dbeta1=ref["beta1"],
                 dgamma1=ref["gamma1"], dgamma2=ref["gamma2"], dbeta2=ref["beta2"], ddata=ref["data"].transpose(0, 2, 3, 1),
                 y=ref["y"].transpose(0, 2, 3, 1))
    for k, want in pairs.items():
        err, scale = float(np.abs(got[k] - want).max()), float(np.abs(want).max())
        print("%-8s max |err| %.3g of max |ref| %.3g" % (k, err, scale))
        assert scale > 0 and err <= 1e-9 * scale, k


# ---- MetaUnitTrain -------------------------------------------------------------------------------------------------------------------------
def f32_of(be, buf, n=576):
    return be.down(buf, np.float32, (n,)) if not hasattr(buf, "shape") or buf.dtype == np.uint8 or str(buf.dtype) == "torch.uint8" \
        else np.array(be.alloc.to_numpy(buf), np.float32).reshape(-1)


def make_unit(be, P, name, W, dt):
    from rangedet_amd.backward import MetaUnitTrain
    return MetaUnitTrain(name, P, W, dtype=dt, lib=be.lib, alloc=be.alloc)


def unit_io(be, data, coord, g, dt):
    B, _, H, W = data.shape
    x = TU.dev16(be, TU.to_bits(nhwc(data), dt), dt)
    cview = be.alloc.view_f32(be.up(coord), (B, 3, H, W))
    return x, cview, TU.dev16(be, TU.to_bits(g, dt), dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_meta_unit_train(be, dt):
    """MetaUnitTrain.forward / backward equal the composition of the separately tested launches bit for bit: the statistics, rd_bn_fold's
    tables and moving statistics (norm_model.fold_f32), z, y, and -- from the unit's own dz and tables -- all nine Meta gradients and ddata
    with a residual.  The eleven gradient names and shapes are the reference's."""
    import norm_model as NM
    from rangedet_amd.backward import BN_EPS, BN_MOMENTUM
    B, H, W = 2, 9, 33
    n = B * H * W
    P, name, prm, data, coord, g, norm = unit_case(B, H, W, dt)
    unit = make_unit(be, P, name, W, dt)
    pf, pb = be.lib.pack_meta(*MB.pack_args(prm), dt), be.lib.pack_meta_bwd(*MB.pack_args(prm), dt)
    assert be.down(unit.packed_fwd, np.uint8, (len(pf),)).tobytes() == pf.tobytes()
    assert be.down(unit.packed_bwd, np.uint8, (len(pb),)).tobytes() == pb.tobytes()
    x, cview, gd = unit_io(be, data, coord, g, dt)
    with pytest.raises(RuntimeError):
        unit.backward(gd)
    y = unit.forward(x, cview)
    res_v = TU.rnd("normal", (B, H, W, 64), dt, 6)
    ddata, grads = unit.backward(gd, residual=TU.dev16(be, TU.to_bits(res_v, dt), dt))
    pre = "%s_%d" % (name, W)
    shapes = {pre + "_mlp0_weight": (32, 3, 1, 1), pre + "_mlp0_bias": (32,), pre + "_mlp1_weight": (64, 32, 1, 1), pre + "_mlp1_bias": (64,),
              name + "aggregation_conv1_weight": (64, 576, 1, 1), name + "point_wise_mlp_bn1_gamma": (576,), name + "point_wise_mlp_bn1_beta": (576,),
              name + "aggregation_bn1_gamma": (64,), name + "aggregation_bn1_beta": (64,)}
    assert set(grads) == set(shapes)
    gn = {k: np.array(be.alloc.to_numpy(v), np.float32) for k, v in grads.items()}
    for k, s in shapes.items():
        assert gn[k].shape == s and np.isfinite(gn[k]).all(), k
    aux = {k: np.array(be.alloc.to_numpy(v), np.float32) for k, v in unit.aux().items()}
    assert set(aux) == {name + b + s for b in ("point_wise_mlp_bn1", "aggregation_bn1") for s in ("_moving_mean", "_moving_var")}
    # statistics and fold
    tb = {k: f32_of(be, v) for k, v in unit.saved["tabs"].items()}
    single = launch(be, prm, data, coord, data, None, dt, 0, what="stats")
    assert single["mean1"].tobytes() == tb["mean1"].tobytes() and single["var1"].tobytes() == tb["var1"].tobytes()
    bn1 = name + "point_wise_mlp_bn1"
    fold = NM.fold_f32(tb["mean1"], tb["var1"], norm[0], norm[1], BN_EPS, BN_MOMENTUM, n, True, P[bn1 + "_moving_mean"], P[bn1 + "_moving_var"])
    assert TU.same_bits(tb["rstd1"], fold["rstd"]) and TU.same_bits(tb["a1"], fold["a"]) and TU.same_bits(tb["bb1"], fold["b"])
    assert TU.same_bits(aux[bn1 + "_moving_mean"], fold["moving_mean"]) and TU.same_bits(aux[bn1 + "_moving_var"], fold["moving_var"])
    # z, y
    zv = TU.vals16(be, unit.saved["z"], dt)
    tabs = dict(tb, c1=np.zeros(576, np.float32), c2=np.zeros(576, np.float32))
    assert launch(be, prm, data, coord, data, tabs, dt, 0, what="fwd")["z"].tobytes() == zv.tobytes()
    b2 = {k: f32_of(be, v, 64) for k, v in unit.saved["bn2"].items()}
    assert TU.same_bits(TU.vals16(be, y, dt), NM.affine_relu_f32(zv.reshape(-1, 64), b2["a"], b2["b"], dt).reshape(B, H, W, 64))
    # backward: the unit's own dz through the single launches
    dzv = np.ascontiguousarray(TU.vals16(be, unit.dz, dt).transpose(0, 3, 1, 2))
    s = launch(be, prm, data, coord, dzv, tabs, dt, 0, what="sums")
    tabs.update(c1=s["c1"], c2=s["c2"])
    s.update(launch(be, prm, data, coord, dzv, tabs, dt, 0, residual=res_v, what="params data"))
    for k, pname in (("dA", name + "aggregation_conv1_weight"), ("dgamma1", bn1 + "_gamma"), ("dbeta1", bn1 + "_beta"), ("dW1", pre + "_mlp1_weight"),
                     ("db1", pre + "_mlp1_bias"), ("dW0", pre + "_mlp0_weight"), ("db0", pre + "_mlp0_bias")):
        assert s[k].tobytes() == gn[pname].tobytes(), k
    assert s["ddata"].tobytes() == TU.vals16(be, ddata, dt).tobytes()
    assert np.abs(s["c1"]).max() > 0 and np.abs(s["c2"]).max() > 0


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_unit_one_pixel(be, dt):
    """(1, 1, 1): every neighbour padded, n = 1 (unbiased=False): var1 = 0, the launches run and give finite values"""
    P, name, prm, data, coord, g, norm = unit_case(1, 3, 31, dt)
    data, coord, g = data[:, :, :1, :1].copy(), coord[:, :, :1, :1].copy(), g[:, :1, :1].copy()
    unit = make_unit(be, P, name, 31, dt)
    x, cview, gd = unit_io(be, data, coord, g, dt)
    y = unit.forward(x, cview, unbiased=False)
    ddata, grads = unit.backward(gd)
    assert (f32_of(be, unit.saved["tabs"]["var1"]) == 0).all()
    assert np.isfinite(TU.vals16(be, y, dt)).all() and np.isfinite(TU.vals16(be, ddata, dt)).all()
    assert all(np.isfinite(np.array(be.alloc.to_numpy(v), np.float32)).all() for v in grads.values())


# ---- optimizer -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_sgd_step_repacks_the_unit(be, dt):
    """one SGD.step() over a MetaUnitTrain: every master is bit-equal to optim_model.sgd_step, both blocks are byte-equal to the host packers
    on the updated masters, and a second forward differs from the first and equals a fresh unit built from the updated parameters"""
    from rangedet_amd.optim import SGD, default_wd_mult
    B, H, W = 2, 9, 33
    P, name, prm, data, coord, g, norm = unit_case(B, H, W, dt)
    unit = make_unit(be, P, name, W, dt)
    opt = SGD(lr=0.05, momentum=0.9, wd=1e-4, rescale_grad=0.5, clip_gradient=2.0, lib=be.lib, alloc=be.alloc)
    opt.attach(unit)
    x, cview, gd = unit_io(be, data, coord, g, dt)
    y1 = TU.vals16(be, unit.forward(x, cview), dt).copy()
    _, grads = unit.backward(gd)
    gn = {k: np.array(be.alloc.to_numpy(v), np.float32).copy() for k, v in grads.items()}
    opt.step()
    be.alloc.sync()
    P2 = dict(P)
    for pname, (shape, master, _, _) in unit.table.items():
        w0 = np.asarray(P[pname], np.float32).reshape(shape)
        want, _ = OM.sgd_step(w0, gn[pname], np.zeros(shape, np.float32), 0.05, 0.9, 1e-4, 0.5, 2.0, wd_mult=default_wd_mult(pname))
        got = np.array(be.alloc.to_numpy(master), np.float32).reshape(shape)
        assert got.tobytes() == want.tobytes(), pname
        assert (got != w0).any(), pname
        P2[pname] = got
    for k, v in unit.aux().items():
        P2[k] = np.array(be.alloc.to_numpy(v), np.float32)
    prm2 = T.unit(MB.folded(P2, name, W))
    pf, pb = be.lib.pack_meta(*MB.pack_args(prm2), dt), be.lib.pack_meta_bwd(*MB.pack_args(prm2), dt)
    assert be.down(unit.packed_fwd, np.uint8, (len(pf),)).tobytes() == pf.tobytes()
    assert be.down(unit.packed_bwd, np.uint8, (len(pb),)).tobytes() == pb.tobytes()
    y2 = TU.vals16(be, unit.forward(x, cview), dt).copy()
    assert (y2 != y1).any()
    fresh = make_unit(be, P2, name, W, dt)
    assert TU.vals16(be, fresh.forward(x, cview), dt).tobytes() == y2.tobytes()


# ---- MetaBlockTrain, Res1StageTrain --------------------------------------------------------------------------------------------------------
def golden_res1_names(W):
    """(trainable argument names, auxiliary names) that start with res1_ in tests/golden/graph_veh_test.json, the MLP's width replaced by W"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_veh_test.json")) as f:
        nodes = json.load(f)["nodes"]
    names = [n["name"].replace("_2656_", "_%d_" % W) for n in nodes if n["op"] == "var" and n["name"].startswith("res1_")]
    aux = {n for n in names if n.endswith("_moving_mean") or n.endswith("_moving_var")}
    return set(names) - aux, aux


def bytes_of(be, t):
    """a device tensor or view -> its bytes"""
    if isinstance(t, np.ndarray):
        return np.ascontiguousarray(t).tobytes()
    if t.element_size() == 2:
        import torch
        return t.contiguous().view(torch.int16).cpu().numpy().tobytes()
    return np.array(be.alloc.to_numpy(t)).tobytes()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_meta_block_and_res1_stage(be, dt):
    """MetaBlockTrain equals MetaUnitTrain followed by the separately tested steps of a BasicBlock (conv2, bn2, identity add, ReLU; the
    shortcut's gradient as the residual of the Meta data gradient); Res1StageTrain equals StemBlockTrain then MetaBlockTrain -- forward and
    backward, bit for bit.  The gradient keys are the trainable res1_* arguments of the golden graph, aux() its res1_* auxiliary states."""
    from rangedet_amd.backbone_train import MetaBlockTrain, Res1StageTrain, StemBlockTrain
    from rangedet_amd.backward import BN_EPS, BN_MOMENTUM, MetaUnitTrain, TowerOps
    B, H, W = 1, 9, 33
    P = MM.weights(W)
    name = MM.NAME
    kw = dict(dtype=dt, lib=be.lib, alloc=be.alloc)
    aux_p = {k: v for k, v in P.items() if k.endswith("_moving_mean") or k.endswith("_moving_var")}
    arg_p = {k: v for k, v in P.items() if k not in aux_p}
    _, coord = MM.make_inputs("range", B, H, W, 1, dt)
    x16 = TU.dev16(be, TU.to_bits(TU.rnd("normal", (B, H, W, 16), dt, 3), dt), dt)
    cview = be.alloc.view_f32(be.up(coord.numpy()), (B, 3, H, W))
    gd = TU.dev16(be, TU.to_bits(TU.rnd("normal", (B, H, W, 64), dt, 4), dt), dt)
    stage = Res1StageTrain.from_params(arg_p, aux_p, W, **kw)
    y = stage.forward(x16, cview)
    none, grads = stage.backward(gd)
    want_args, want_aux = golden_res1_names(W)
    assert none is None and set(grads) == want_args and set(stage.aux()) == want_aux
    assert {e["name"] for e in stage.optimizer_entries()} == want_args
    # the stage is the stem, then the block
    bn = lambda key: tuple(P["res1_unit1_%s_%s" % (key, k)] for k in ("gamma", "beta", "moving_mean", "moving_var"))
    stem = StemBlockTrain("res1_unit1", P["res1_unit1_conv1_weight"], P["res1_unit1_conv2_weight"], bn("bn1"), bn("bn2"), P["res1_unit1_sc_weight"],
                          bn("sc_bn"), **kw)
    block = MetaBlockTrain(name, P, W, **kw)
    ys = stem.forward(x16)
    yb = block.forward(ys, cview)
    assert bytes_of(be, yb) == bytes_of(be, y)
    dx, gb = block.backward(gd)
    _, gs = stem.backward(dx)
    for k, v in dict(gb, **gs).items():
        assert bytes_of(be, v) == bytes_of(be, grads[k]), k
    # the block is the unit, then a BasicBlock's second half
    unit, o = MetaUnitTrain(name, P, W, **kw), TowerOps(dt, be.lib, be.alloc)
    w2 = np.ascontiguousarray(P[name + "_conv2_weight"], dtype=np.float32)
    y1 = unit.forward(ys, cview)
    z2 = o.conv_unscaled(y1, o.pack_unscaled(w2), 64, 64, tag=2)
    up = lambda k: be.alloc.upload(np.ascontiguousarray(P[name + "_bn2_" + k], dtype=np.float32))
    gamma2 = up("gamma")
    mean, var = o.bn_stats(z2, tag=2)
    rstd, a, b = o.bn_fold(mean, var, gamma2, up("beta"), up("moving_mean"), up("moving_var"), B * H * W, 64, BN_EPS, BN_MOMENTUM, True, tag=2)
    assert bytes_of(be, o.affine_add_relu(z2, a, b, ys)) == bytes_of(be, yb)
    dz2, dr, dg2, db2, _, _ = o.bn_add_relu_bwd(gd, z2, ys, dict(a=a, b=b, mean=mean, rstd=rstd), gamma2, None, None, tag=2)
    dW2 = o.weight_grad(y1, dz2, tag=2)
    dxu, gu = unit.backward(o.data_grad(dz2, o.pack_data_grad(w2), tag=2), residual=dr)
    assert bytes_of(be, dxu) == bytes_of(be, dx)
    for k, v in dict(gu, **{name + "_conv2_weight": dW2, name + "_bn2_gamma": dg2, name + "_bn2_beta": db2}).items():
        assert bytes_of(be, v) == bytes_of(be, gb[k]), k


# ---- the whole unit against autograd, per element ------------------------------------------------------------------------------------------
SHARE_CAP = {R.RD_BF16: 0.02, R.RD_F16: 0.003}
UNIT_SHAPE = (2, 9, 33)


@functools.lru_cache(maxsize=None)
def unit_reference(dt):
    """-> (P, name, data, coord, g, ref {UNIT_OUT name: float64 autograd value}, sigma, sum bounds, gate shares, the contract's args)"""
    import convbwd_model as CB
    from rangedet_amd.backward import BN_EPS, BN_MOMENTUM
    B, H, W = UNIT_SHAPE
    n = B * H * W
    P, name, prm, data, coord, g, norm = unit_case(B, H, W, dt)
    bn1, bn2 = name + "point_wise_mlp_bn1", name + "aggregation_bn1"
    moving = [np.asarray(P[k], np.float64) for k in (bn1 + "_moving_mean", bn1 + "_moving_var", bn2 + "_moving_mean", bn2 + "_moving_var")]
    args = (data, coord, g, prm, norm, moving, dt, BN_EPS, BN_MOMENTUM)
    con, sig, shares = T.unit_sigma(args, dt, MM.half_ulp(dt))
    auto = T.autograd_reference(data, coord, np.ascontiguousarray(g.transpose(0, 3, 1, 2)), prm, *norm, dt, BN_EPS, round_h=False)
    q, z, om, unb = auto["q"], auto["z"], 1 - BN_MOMENTUM, n / (n - 1.0)
    ref = dict(y=auto["y"].transpose(0, 2, 3, 1), ddata=auto["data"].transpose(0, 2, 3, 1), dA=auto["A"].reshape(64, 576), dW1=auto["w1"], db1=auto["b1"],
               dW0=auto["w0"], db0=auto["b0"], dgamma1=auto["gamma1"], dbeta1=auto["beta1"], dgamma2=auto["gamma2"], dbeta2=auto["beta2"],
               mm1=moving[0] * BN_MOMENTUM + q.mean((0, 2, 3)) * om, mv1=moving[1] * BN_MOMENTUM + q.var((0, 2, 3)) * unb * om,
               mm2=moving[2] * BN_MOMENTUM + z.mean((0, 2, 3)) * om, mv2=moving[3] * BN_MOMENTUM + z.var((0, 2, 3)) * unb * om)
    for k in T.UNIT_OUT:                       # the hooked contract with identity hooks IS the autograd function
        assert np.abs(con[k] - ref[k]).max() <= 1e-9 * np.abs(ref[k]).max(), k
    nsum = dict(y=576 + 8, ddata=9 * 65 + 8, mm1=8, mv1=8, mm2=8, mv2=8)
    sb = {k: CB.sum_bound(nsum.get(k, MB.SUM_N(n)), con["abs"][k]) for k in T.UNIT_OUT}
    return P, name, data, coord, g, ref, sig, sb, shares, args


def judge_unit(got, dt, what):
    """meta_model.per_element_stats / within_bounds with sigma' = sigma + sum bound / 7: tol = 7 sigma + sum bound + 1e-5.  sigma holds the
    documented roundings (each by its own binade), the float32 statistics and the gate triples (metatrain_model.unit_sigma)."""
    ref, sig, sb = unit_reference(dt)[5:8]
    ok = True
    for k in T.UNIT_OUT:
        worst, rms, nover, n = MM.per_element_stats(got[k], ref[k], sig[k] + sb[k] / 7.0, 0.0)
        print("%s %-8s worst %.3f rms %.3f nover %d / %d" % (what, k, worst, rms, nover, n))
        ok = ok and MM.within_bounds(worst, rms, nover, n)
    return ok


@pytest.mark.parametrize("dt", DTS)
def test_unit_gate_share(dt):
    """the share of gate triples |r| <= 7 sigma_r (and of output-ReLU gates) on the reference alone: 2 % (bf16), 0.3 % (fp16)"""
    shares = unit_reference(dt)[8]
    print("gate triples: r %.4f %%, y %.4f %%" % (100 * shares[0], 100 * shares[1]))
    assert shares[0] <= SHARE_CAP[dt] and shares[1] <= SHARE_CAP[dt]


@pytest.mark.parametrize("dt", DTS)
def test_unit_model_margin(dt):
    """the contract's own roundings (metatrain_model.contract with rounding_hook, float64 sums) against the bounds the kernels are held to.
    Measured on the CPU at (2, 9, 33), 'range' inputs, synth weights, worst / rms per output against worst <= 4, rms < 1.5:
      bf16  y 0.63 / 0.85, ddata 0.35 / 0.25, dA 0.31 / 0.23, dW1 0.15 / 0.24, db1 0.09 / 0.22, dW0 0.17 / 0.34, db0 0.08 / 0.27,
            dgamma1 0.16 / 0.23, dbeta1 0.15 / 0.24, dgamma2 0.17 / 0.35, dbeta2 0.10 / 0.22; moving mean1 0.33 / 0.96, var1 0.41 / 0.98,
            mean2 0.36 / 1.17, var2 0.21 / 0.68
      fp16  y 0.54 / 0.84, ddata 0.41 / 0.31, dA 0.50 / 0.50, dW1 0.18 / 0.25, db1 0.10 / 0.25, dW0 0.09 / 0.20, db0 0.06 / 0.25,
            dgamma1 0.20 / 0.29, dbeta1 0.19 / 0.30, dgamma2 0.16 / 0.43, dbeta2 0.14 / 0.31; moving mean1 0.18 / 0.49, var1 0.32 / 0.90,
            mean2 0.29 / 1.18, var2 0.18 / 0.82
    (the gradients sit at a quarter of sigma because sigma prices every gate triple at a whole flip; gate shares: r 0.34 %, y 1.61 % in bf16,
    0.04 % / 0.20 % in fp16).  This model is never compared with a kernel."""
    args = unit_reference(dt)[9]
    assert judge_unit(T.contract(*args, T.rounding_hook(dt)), dt, "model")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_unit_against_autograd(be, dt):
    """MetaUnitTrain.forward / backward per element against float64 torch autograd of the un-fused formulation with
    F.batch_norm(training=True) on both norms, on the packer's rounded weights: y, ddata, the eleven gradients, the four moving statistics.
    Tolerance: 7 sigma + the float32 sum bound (+ 1e-5), sigma from metatrain_model.unit_sigma -- first order, every documented rounding
    priced by its own binade, the float32 statistics, and every gate triple as a source of one whole flip; all propagation paths (mean1,
    rstd1, c1, c2, the second norm) are in it because it is taken from the contract's own directional derivatives."""
    P, name, data, coord, g, ref = unit_reference(dt)[:6]
    B, H, W = UNIT_SHAPE
    unit = make_unit(be, P, name, W, dt)
    x, cview, gd = unit_io(be, data, coord, g, dt)
    y = unit.forward(x, cview)
    ddata, grads = unit.backward(gd)
    pre, bn1, bn2 = "%s_%d" % (name, W), name + "point_wise_mlp_bn1", name + "aggregation_bn1"
    f = lambda t, shape: np.array(be.alloc.to_numpy(t), np.float64).reshape(shape)
    aux = unit.aux()
    got = dict(y=TU.vals16(be, y, dt), ddata=TU.vals16(be, ddata, dt), dA=f(grads[name + "aggregation_conv1_weight"], (64, 576)),
               dW1=f(grads[pre + "_mlp1_weight"], (64, 32)), db1=f(grads[pre + "_mlp1_bias"], (64,)), dW0=f(grads[pre + "_mlp0_weight"], (32, 3)),
               db0=f(grads[pre + "_mlp0_bias"], (32,)), dgamma1=f(grads[bn1 + "_gamma"], (576,)), dbeta1=f(grads[bn1 + "_beta"], (576,)),
               dgamma2=f(grads[bn2 + "_gamma"], (64,)), dbeta2=f(grads[bn2 + "_beta"], (64,)), mm1=f(aux[bn1 + "_moving_mean"], (576,)),
               mv1=f(aux[bn1 + "_moving_var"], (576,)), mm2=f(aux[bn2 + "_moving_mean"], (64,)), mv2=f(aux[bn2 + "_moving_var"], (64,)))
    assert judge_unit(got, dt, "unit %s" % be.name)


def test_build_refuses_scratch_in_the_two_passes():
    """rangedet_amd.build reads the compiler's resource remarks: pass A and pass B must be there and must use no scratch"""
    from rangedet_amd import build
    line = "rd_api.hip:1:1: remark: %s [-Rpass-analysis=kernel-resource-usage]"
    def remarks(sums, params):
        rows = []
        for name, sc in (("_ZN2rd22meta_train_sums_kernelILi1EEEvNS_13MetaTrainArgsE", sums), ("_ZN2rd24meta_train_params_kernelILi2EEEvNS_13MetaTrainArgsE", params),
                         ("_ZN2rd22meta_train_data_kernelILi1EEEvNS_13MetaTrainArgsE", 56)):
            rows += [line % ("Function Name: " + name), line % "    VGPRs: 200", line % ("    ScratchSize [bytes/lane]: %d" % sc)]
        return "\n".join(rows)
    assert build.scratch_bytes(remarks(0, 0))["_ZN2rd22meta_train_data_kernelILi1EEEvNS_13MetaTrainArgsE"] == 56
    build.check_no_scratch(remarks(0, 0))
    for bad in (remarks(8, 0), remarks(0, 4), "no remarks at all"):
        with pytest.raises(RuntimeError):
            build.check_no_scratch(bad)

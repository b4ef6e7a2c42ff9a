"""The parameter update on the device (csrc/k_optim.h: rd_sgd_table_bytes / rd_sgd_table_host, rd_sgd_mom_update, rd_pack_conv3x3_dev;
rangedet_amd.optim.SGD and its schedulers; the towers' optimizer_entries) against tests/optim_model.py, the NumPy float32 restatement of
the update with one rounding per operation.  Through the C ABI in the style of test_batch_norm.py: every image buffer is pre-filled with
0xFF bytes, every buffer carries a guard tail that must be unchanged afterwards, and buffers the table does not name stay as they were.

  update            weights and momenta bit-equal to the model over three steps with a different learning rate each, for tensors of 1 .. 1153
                    elements and two conv weights in ONE table, with clipping on both sides (asserted from the inputs), without clipping,
                    without momentum, with wd_mult 0 and lr_mult 0.1 entries; two runs give the same bytes
  images            the forward image (with and without a fold scale) and the data-gradient image, zero tail included, byte-equal to the
                    host packers on the updated weight for every (cout, cin) in {64, 128}^2 and both types, also for weights that sit on
                    exact rounding ties of the 16-bit type; rd_pack_conv3x3_dev the same on un-updated weights
  refusals          cin 72, a (64, 8, 3, 3) weight, a misaligned pointer, n = 0: the table builder's codes and the Python layer's errors,
                    nothing written
  tower loop        three iterations of forward, backward, step on an attached tower; after each step a fresh tower built on the host-pack
                    path from the model's weights gives the attached tower's next output and input gradient in every bit
  schedulers        closed-form values at the updates where the formulas change"""
import ctypes
import math

import numpy as np
import pytest

import optim_model as OM
from conftest import BOTH
from rangedet_amd import lib as R
from rangedet_amd import optim as O
from train_util import DTS, GUARD, back, dev16, ff, rnd, same_bits, to_bits, vals16

F32 = np.float32
CHUNK = 1024
SIZES = (1, 8, 64, 128, 1024, 1153)         # 1153: two chunks, 1153 % 4 == 1
MULTS = {1: (1.0, 0.0), 8: (0.1, 1.0), 64: (0.1, 0.0)}      # n -> (lr_mult, wd_mult); every other tensor (1, 1)
LRS = (0.01, 0.02, 0.005)


def fup(be, arr):
    """float32 values -> a device buffer with a 0xFF guard tail"""
    raw = np.ascontiguousarray(arr, dtype=F32).view(np.uint8).reshape(-1)
    return be.up(np.concatenate([raw, np.full(GUARD, 0xFF, np.uint8)]))


def fback(be, buf, shape, what):
    return back(be, buf, int(np.prod(shape)) * 4, what).view(F32).reshape(shape).copy()


def poke(be, buf, arr):
    raw = np.ascontiguousarray(arr, dtype=F32).view(np.uint8).reshape(-1)
    if be.name == "emu":
        buf[:raw.size] = raw
    else:
        import torch
        buf[:raw.size].copy_(torch.from_numpy(raw.copy()))


def image_bytes(cout, cin):
    return 9 * cout * cin * 2 + 256


class Case:
    """tensors on the device with their host twins: specs = [dict(shape, lr_mult, wd_mult, fwd, bwd, fold)]"""

    def __init__(self, be, dt, specs, seed, wvals=None):
        self.be, self.dt, self.specs = be, dt, specs
        rng = np.random.default_rng(seed)
        self.w = [(wvals[i] if wvals and wvals.get(i) is not None else rng.standard_normal(s["shape"])).astype(F32) for i, s in enumerate(specs)]
        self.m = [(0.1 * rng.standard_normal(s["shape"])).astype(F32) for s in specs]
        self.g = [np.zeros(s["shape"], F32) for s in specs]
        self.fold = [rng.uniform(0.5, 1.5, s["shape"][0]).astype(F32) if s.get("fold") else None for s in specs]
        self.wd, self.md, self.gd = ([fup(be, v) for v in lst] for lst in (self.w, self.m, self.g))
        self.foldd = [None if f is None else fup(be, f) for f in self.fold]
        self.fwd = [ff(be, image_bytes(*s["shape"][:2])) if s.get("fwd") else None for s in specs]
        self.bwd = [ff(be, image_bytes(*s["shape"][:2])) if s.get("bwd") else None for s in specs]
        self.bystander = be.up(np.arange(4096, dtype=np.uint8))
        ts = []
        for i, s in enumerate(specs):
            n = int(np.prod(s["shape"]))
            co, ci = (s["shape"][:2] if len(s["shape"]) == 4 else (0, 0))
            ts.append(R.SgdTensor(be.ptr(self.wd[i]), be.ptr(self.gd[i]), be.ptr(self.md[i]), n, s.get("lr_mult", 1.0), s.get("wd_mult", 1.0), co, ci,
                                  be.ptr(self.fwd[i]), be.ptr(self.bwd[i]), be.ptr(self.foldd[i])))
        self.tensors = ts
        self.host = be.lib.sgd_table(ts, dt)
        assert self.host.size == be.lib.cdll.rd_sgd_table_bytes(ctypes.addressof((R.SgdTensor * len(ts))(*ts)), len(ts))
        self.dev = be.up(self.host)

    def step(self, grads, lr, momentum, wd, rescale, clip):
        """new gradients in, one step on the device and on the host twins"""
        be = self.be
        for i, g in enumerate(grads):
            self.g[i] = np.asarray(g, F32)
            poke(be, self.gd[i], self.g[i])
        be.lib.call("rd_sgd_mom_update", be.ptr(self.dev), self.host.ctypes.data, lr, momentum, wd, rescale, clip, be.stream)
        for i, s in enumerate(self.specs):
            self.w[i], self.m[i] = OM.sgd_step(self.w[i], self.g[i], self.m[i], lr, momentum, wd, rescale, clip, s.get("lr_mult", 1.0), s.get("wd_mult", 1.0))

    def check(self, what):
        """-> the bytes of everything the step wrote"""
        be, L, out = self.be, self.be.lib, []
        for i, s in enumerate(self.specs):
            shp = s["shape"]
            w, m, g = (fback(be, d, shp, "%s %s %d" % (what, k, i)) for d, k in ((self.wd[i], "weight"), (self.md[i], "mom"), (self.gd[i], "grad")))
            assert g.tobytes() == self.g[i].tobytes(), (what, i, "the gradient was written")
            bad = int((w.view(np.uint32) != self.w[i].view(np.uint32)).sum()), int((m.view(np.uint32) != self.m[i].view(np.uint32)).sum())
            assert bad == (0, 0), (what, "tensor %d %r: weight / momentum elements that differ from the model" % (i, shp), bad)
            out += [w.tobytes(), m.tobytes()]
            if self.fold[i] is not None:
                assert fback(be, self.foldd[i], self.fold[i].shape, "fold").tobytes() == self.fold[i].tobytes()
            for img, want in ((self.fwd[i], lambda: OM.forward_image(L, self.w[i], self.fold[i], self.dt)),
                              (self.bwd[i], lambda: OM.data_grad_image(L, self.w[i], self.dt))):
                if img is not None:
                    want = want()
                    got = back(be, img, want.size, "%s image %d" % (what, i))
                    nbad = int((got != want).sum())
                    assert nbad == 0, (what, "tensor %d %r: image bytes that differ from the host packer" % (i, shp), nbad)
                    assert not got[-256:].any()
                    out.append(got.tobytes())
        assert (be.down(self.bystander, np.uint8, (4096,)) == np.arange(4096, dtype=np.uint8)).all(), "a buffer outside the table was written"
        assert be.down(self.dev, np.uint8, (self.host.size,)).tobytes() == self.host.tobytes(), "the table was written"
        return b"".join(out)


def mixed_specs():
    specs = [dict(shape=(n,), lr_mult=MULTS.get(n, (1.0, 1.0))[0], wd_mult=MULTS.get(n, (1.0, 1.0))[1]) for n in SIZES]
    specs.append(dict(shape=(64, 64, 3, 3), fwd=True, bwd=True))
    specs.append(dict(shape=(128, 128, 3, 3), fwd=True, bwd=True, fold=True, lr_mult=0.1))
    return specs


_GRADS = {}


def mixed_grads(step):
    """gradients of scale 100 for every tensor of mixed_specs, made once per step"""
    if step not in _GRADS:
        rng = np.random.default_rng(900 + step)
        _GRADS[step] = [(100.0 * rng.standard_normal(s["shape"])).astype(F32) for s in mixed_specs()]
        for g in _GRADS[step]:
            g.setflags(write=False)
    return _GRADS[step]


def run_mixed(be, dt, momentum, wd, rescale, clip, what):
    c = Case(be, dt, mixed_specs(), 801)
    for k, lr in enumerate(LRS):
        c.step(mixed_grads(k), lr, momentum, wd, rescale, clip)
    return c.check(what)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_update_bits_clipped(be, dt):
    """rescale_grad 0.5, clip 35, momentum 0.9, wd 1e-5 (the reference's): a share of the scaled gradients is clipped on either side; three
    steps carry the momentum; a second run from the same state gives the same bytes"""
    g = np.concatenate([0.5 * v.reshape(-1) for k in range(3) for v in mixed_grads(k)])
    hi, lo = float((g > 35).mean()), float((g < -35).mean())
    print("clipped above %.3f, below %.3f of the scaled gradients" % (hi, lo))
    assert hi > 0.15 and lo > 0.15 and float((np.abs(g) < 35).mean()) > 0.3
    first = run_mixed(be, dt, 0.9, 1e-5, 0.5, 35.0, "clipped %s" % be.name)
    assert run_mixed(be, dt, 0.9, 1e-5, 0.5, 35.0, "clipped again %s" % be.name) == first


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_update_bits_no_clip_and_no_momentum(be):
    """clip_gradient -1 (nothing clipped: the momenta pass 35 lr), a weight decay large enough to move every bit; then momentum 0"""
    run_mixed(be, R.RD_BF16, 0.9, 1e-2, 0.5, -1.0, "no clip %s" % be.name)
    run_mixed(be, R.RD_F16, 0.0, 1e-3, 1.0, 35.0, "no momentum %s" % be.name)


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_nan_and_inf_gradients_propagate(be):
    """a NaN gradient makes its weight NaN with and without clipping; inf is clipped like any large value, and propagates without clipping"""
    for clip in (35.0, -1.0):
        c = Case(be, R.RD_BF16, [dict(shape=(8,))], 811)
        g = np.array([np.nan, np.inf, -np.inf, 1, 2, 3, 4, 5], F32)
        c.step([g], 0.01, 0.9, 1e-5, 1.0, clip)
        w = fback(be, c.wd[0], (8,), "w")
        assert np.isnan(w[0]) and np.isfinite(w[3:]).all()
        assert np.isfinite(w[1:3]).all() if clip >= 0 else (np.isinf(w[1:3]).all() and w[1] < 0 < w[2])
        assert same_bits(w[1:], c.w[0][1:]) and np.isnan(c.w[0][0])


# ---- images --------------------------------------------------------------------------------------------------------------------------------
PAIRS = [(64, 64), (64, 128), (128, 64), (128, 128)]


@pytest.mark.parametrize("cout,cin", PAIRS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_images_after_a_step(be, dt, cout, cin):
    """tensor 0: forward image without a scale and the data-gradient image; tensor 1: forward image with a fold scale.  Step 1 leaves the
    weights as they are (zero gradients, wd_mult 0, zero momenta) -- tensor 0 sits on exact rounding ties of the type; step 2 moves them"""
    shape = (cout, cin, 3, 3)
    rng = np.random.default_rng(820 + cout + 2 * cin)
    ties = OM.tie_values(shape, dt, rng, dt == R.RD_BF16)
    c = Case(be, dt, [dict(shape=shape, fwd=True, bwd=True, wd_mult=0.0), dict(shape=shape, fwd=True, fold=True, wd_mult=0.0)], 821, wvals={0: ties})
    for i in range(2):
        c.m[i] = np.zeros(shape, F32)
        poke(be, c.md[i], c.m[i])
    c.step([np.zeros(shape, F32)] * 2, 0.1, 0.9, 1e-5, 1.0, 35.0)
    assert c.w[0].tobytes() == ties.tobytes()
    c.check("ties %r %s" % (shape, be.name))
    for img in (c.fwd[0], c.bwd[0], c.fwd[1]):                # a fresh 0xFF fill: step 2 must write every byte again
        if be.name == "emu":
            img[:] = 0xFF
        else:
            img.fill_(0xFF)
    c.step([(10 * rng.standard_normal(shape)).astype(F32) for _ in range(2)], 0.05, 0.9, 1e-5, 1.0, 35.0)
    assert (c.w[0] != ties).mean() > 0.9
    c.check("moved %r %s" % (shape, be.name))


@pytest.mark.parametrize("cout,cin", PAIRS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_pack_conv3x3_dev(be, dt, cout, cin):
    L = be.lib
    rng = np.random.default_rng(830 + cout + 2 * cin)
    shape = (cout, cin, 3, 3)
    fold = rng.uniform(0.5, 1.5, cout).astype(F32)
    foldd = fup(be, fold)
    for w in (OM.tie_values(shape, dt, rng, dt == R.RD_BF16), rng.standard_normal(shape).astype(F32)):
        wd = fup(be, w)
        for flip, fs, want in ((0, None, OM.forward_image(L, w, None, dt)), (0, foldd, OM.forward_image(L, w, fold, dt)), (1, None, OM.data_grad_image(L, w, dt))):
            assert want.size == image_bytes(cout, cin) == L.cdll.rd_conv3x3_ex_packed_bytes(cin, cout, 1, cin)
            out = ff(be, want.size)
            L.call("rd_pack_conv3x3_dev", be.ptr(wd), be.ptr(fs), cout, cin, flip, dt, be.ptr(out), be.stream)
            got = back(be, out, want.size, "image")
            assert int((got != want).sum()) == 0, (shape, flip, fs is not None)
        assert fback(be, wd, shape, "w").tobytes() == w.tobytes()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_refusals(be):
    L = be.lib
    buf = be.empty(1 << 21)
    p = be.ptr(buf)
    assert p % 16 == 0

    def table(**kw):
        """-> (rd_sgd_table_bytes, rd_sgd_table_host's code, the output buffer untouched)"""
        f = dict(weight=p, grad=p, mom=p, n=64, lr_mult=1.0, wd_mult=1.0, cout=0, cin=0, pack_fwd=None, pack_bwd=None, fold_scale=None)
        f.update(kw)
        dt = f.pop("dt", R.RD_BF16)
        arr = (R.SgdTensor * 2)(R.SgdTensor(p, p, p, 8, 1.0, 1.0, 0, 0, None, None, None), R.SgdTensor(**f))
        out = np.full(4096, 0xAB, np.uint8)
        nbytes = L.cdll.rd_sgd_table_bytes(ctypes.addressof(arr), 2)
        rc = L.cdll.rd_sgd_table_host(ctypes.addressof(arr), 2, dt, out.ctypes.data)
        return nbytes, rc, bool((out == 0xAB).all())
    nbytes, rc, clean = table()
    assert nbytes > 0 and rc == R.RD_OK and not clean
    for kw, code, word in ((dict(cout=128, cin=72, n=9 * 128 * 72, pack_fwd=p), R.RD_ESHAPE, "concat"),
                           (dict(cout=64, cin=8, n=9 * 64 * 8, pack_fwd=p, pack_bwd=p), R.RD_ESHAPE, "body form"),
                           (dict(cout=64, cin=64, n=9 * 64 * 64 - 1, pack_bwd=p), R.RD_ESHAPE, "9 x"),
                           (dict(weight=p + 8), R.RD_EINVAL, "aligned"), (dict(grad=p + 4), R.RD_EINVAL, "aligned"), (dict(mom=p + 8), R.RD_EINVAL, "aligned"),
                           (dict(cout=64, cin=64, n=9 * 64 * 64, pack_fwd=p + 8), R.RD_EINVAL, "aligned"),
                           (dict(n=0), R.RD_EINVAL, "n 0"), (dict(n=-4), R.RD_EINVAL, "n -4"), (dict(weight=None), R.RD_EINVAL, "null"),
                           (dict(fold_scale=p), R.RD_EINVAL, "fold scale"),
                           (dict(cout=64, cin=64, n=9 * 64 * 64, pack_fwd=p, dt=R.RD_F32), R.RD_EINVAL, "dtype")):
        nbytes, rc, clean = table(**kw)
        msg = L.rd_last_error_string().decode()
        assert rc == code and word in msg and msg.startswith("sgd_table") and clean, (kw, rc, msg)
        assert nbytes == 0 or "dt" in kw, kw
    assert L.cdll.rd_sgd_table_bytes(None, 1) == 0 and L.cdll.rd_sgd_table_host(None, 0, R.RD_BF16, p) == R.RD_EINVAL
    # the step: a host copy that is no table, null pointers
    upd = L.raw("rd_sgd_mom_update")
    zeros = np.zeros(256, np.uint8)
    assert upd(p, zeros.ctypes.data, 0.1, 0.9, 0.0, 1.0, -1.0, be.stream) == R.RD_EINVAL and "table" in L.rd_last_error_string().decode()
    assert upd(None, zeros.ctypes.data, 0.1, 0.9, 0.0, 1.0, -1.0, be.stream) == R.RD_EINVAL
    assert upd(p, None, 0.1, 0.9, 0.0, 1.0, -1.0, be.stream) == R.RD_EINVAL
    pk = L.raw("rd_pack_conv3x3_dev")
    assert pk(p, None, 128, 72, 0, R.RD_BF16, p, be.stream) == R.RD_ESHAPE and pk(p, None, 64, 8, 0, R.RD_BF16, p, be.stream) == R.RD_ESHAPE
    assert pk(p, None, 64, 64, 0, R.RD_F32, p, be.stream) == R.RD_EINVAL and pk(p, None, 64, 64, 0, R.RD_BF16, p + 8, be.stream) == R.RD_EINVAL
    assert pk(None, None, 64, 64, 0, R.RD_BF16, p, be.stream) == R.RD_EINVAL and pk(p, p, 64, 64, 1, R.RD_BF16, p, be.stream) == R.RD_EINVAL
    # the Python layer
    A = be.alloc
    opt = O.SGD(0.1, lib=L, alloc=A)
    img = dict(fwd=buf, bwd=buf, dtype=R.RD_BF16)
    with pytest.raises(NotImplementedError, match="concat"):
        opt.add("rpn_cls_conv_0_lvl_0_weight", A.view_f32(buf, (128, 72, 3, 3)), A.view_f32(buf, (128, 72, 3, 3)), pack=img)
    with pytest.raises(NotImplementedError, match="body form"):
        opt.add("conv_weight", A.view_f32(buf, (64, 8, 3, 3)), A.view_f32(buf, (64, 8, 3, 3)), pack=img)
    with pytest.raises(ValueError, match="aligned"):
        opt.add("a_weight", A.view_f32(buf, (65,))[1:], A.view_f32(buf, (64,)))
    with pytest.raises(ValueError, match="aligned"):
        opt.add("a_weight", A.view_f32(buf, (64,)), A.view_f32(buf, (66,))[2:])
    with pytest.raises(ValueError, match="at least one"):
        opt.add("a_weight", A.view_f32(buf, (0,)), A.view_f32(buf, (0,)))
    with pytest.raises(ValueError, match="16-bit type"):
        opt.add("b_weight", A.view_f32(buf, (64, 64, 3, 3)), A.view_f32(buf, (64, 64, 3, 3)), pack=dict(fwd=buf, dtype=R.RD_F32))
    assert opt.state() == {}
    with pytest.raises(RuntimeError, match="no tensor"):
        opt.step()
    assert not be.down(buf, np.uint8, (1 << 21,)).any()            # nothing ran


# ---- the optimizer's surface -----------------------------------------------------------------------------------------------------------------
def host(A, t):
    return np.array(A.to_numpy(t)).copy()


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_optimizer_surface(be):
    """w = 1, zero gradients, lr 1, wd 0.5, no momentum: a decayed tensor becomes 0.5, an undecayed one stays 1 -- the default wd_mult by
    name; state() gives the momenta; the table is built once and again when a buffer has moved"""
    A, L = be.alloc, be.lib
    assert [O.default_wd_mult(n) for n in ("rpn_cls_conv_0_lvl_1_weight", "rpn_cls_conv_0_lvl_1_bn_gamma", "rpn_cls_conv_0_lvl_1_bn_beta",
                                           "rpn_cls_logit_lvl_1_bias", "x_moving_mean")] == [1.0, 1.0, 0.0, 0.0, 0.0]
    names = ("x_weight", "x_bn_gamma", "x_bn_beta", "x_bias")
    opt = O.SGD(1.0, momentum=0.0, wd=0.5, clip_gradient=None, lib=L, alloc=A)
    ws = {n: A.as_device_f32(np.ones(12, F32)) for n in names}
    gs = {n: A.as_device_f32(np.zeros(12, F32)) for n in names}
    for n in names:
        opt.add(n, ws[n], gs[n])
    assert opt.step() == 1.0 and opt.num_update == 1 and opt.table_builds == 1
    A.sync()
    for n, want in zip(names, (0.5, 0.5, 1.0, 1.0)):
        assert (host(A, ws[n]) == want).all(), n
    st = opt.state()
    assert list(st) == list(names) and all(tuple(v.shape) == (12,) for v in st.values())
    assert (host(A, st["x_weight"]) == -0.5).all() and (host(A, st["x_bias"]) == 0).all()
    opt.step()
    assert opt.table_builds == 1 and opt.num_update == 2
    # explicit multipliers, a scheduler, and a gradient buffer that moved: the momentum stays, the new buffer is read
    g2 = A.as_device_f32(np.full(12, 2.0, F32))
    opt.add("x_bias", ws["x_bias"], g2, lr_mult=0.5, wd_mult=0.0)
    opt.lr_scheduler = lambda u: {3: 0.25}[u]
    assert opt.step() == 0.25 and opt.table_builds == 2
    A.sync()
    assert (host(A, ws["x_bias"]) == 1.0 - 0.25 * 0.5 * 2.0).all() and (host(A, opt.state()["x_bias"]) == -0.25).all()
    w, m = np.ones(12, F32), np.zeros(12, F32)
    for lr in (1.0, 1.0, 0.25):
        w, m = OM.sgd_step(w, np.zeros(12, F32), m, lr, 0.0, 0.5, 1.0, -1.0)
    assert same_bits(host(A, ws["x_weight"]), w)
    with pytest.raises(ValueError, match="elements"):
        opt.add("x_bias", A.as_device_f32(np.ones(16, F32)), A.as_device_f32(np.ones(16, F32)))


# ---- the tower loop ------------------------------------------------------------------------------------------------------------------------
def tower_params(C, nout, seed):
    rng = np.random.default_rng(seed)
    P = dict(ws=[(rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C / 2)).astype(F32) for _ in range(2)],
             gs=[rng.uniform(0.5, 1.5, C).astype(F32) for _ in range(2)], bs=[(0.1 * rng.standard_normal(C)).astype(F32) for _ in range(2)],
             mms=[rng.normal(0, 1, C).astype(F32) for _ in range(2)], mvs=[rng.uniform(0.5, 2, C).astype(F32) for _ in range(2)],
             ow=(rng.standard_normal((nout, C, 1, 1)) / np.sqrt(C)).astype(F32), ob=(0.1 * rng.standard_normal(nout)).astype(F32))
    return P


def tower_loop(be, dt, train, B, H, W, C, nout):
    from rangedet_amd.backward import HeadTowerBackward, HeadTowerTrain
    A, L = be.alloc, be.lib
    kind = "cls" if nout == 1 else "reg"
    P = tower_params(C, nout, 950 + C + nout)
    stems = ["rpn_%s_conv_%d_lvl_1" % (kind, i) for i in range(2)]
    oname = "rpn_cls_logit_lvl_1" if kind == "cls" else "rpn_reg_delta_lvl_1"

    def make(P, aux=None):
        if train:
            mms = P["mms"] if aux is None else [aux[s + "_bn_moving_mean"] for s in stems]
            mvs = P["mvs"] if aux is None else [aux[s + "_bn_moving_var"] for s in stems]
            return HeadTowerTrain(P["ws"], P["gs"], P["bs"], mms, mvs, P["ow"], P["ob"], kind=kind, level=1, dtype=dt, lib=L, alloc=A)
        return HeadTowerBackward(P["ws"], P["gs"], P["bs"], P["ow"], P["ob"], kind=kind, level=1, dtype=dt, lib=L, alloc=A)     # gs, bs: scale, shift

    def run(t):
        out = t.forward(x)
        dx, grads = t.backward(d_out)
        A.sync()
        return host(A, out), vals16(be, dx, dt).copy(), {k: host(A, v) for k, v in grads.items()}
    x = dev16(be, to_bits(rnd("relu", (B, H, W, C), dt, 951), dt), dt)
    d_out = A.as_device_f32(np.random.default_rng(952).standard_normal((B, H * W, nout)).astype(F32))
    tower = make(P)
    lrs = (0.005, 0.01, 0.002)                 # (a tower with a fixed scale has no normalisation to absorb a large step: fp16 stays finite)
    opt = O.SGD(lrs[0], momentum=0.9, wd=1e-3, rescale_grad=1.0, clip_gradient=35, lr_scheduler=lambda u: lrs[u - 1], lib=L, alloc=A)
    opt.attach(tower)
    # host masters keyed by the reference's names
    Wh = {stems[i] + "_weight": P["ws"][i] for i in range(2)}
    Wh.update({oname + "_weight": P["ow"], oname + "_bias": P["ob"]})
    if train:
        Wh.update({stems[i] + "_bn_gamma": P["gs"][i] for i in range(2)})
        Wh.update({stems[i] + "_bn_beta": P["bs"][i] for i in range(2)})
    assert sorted(opt.state()) == sorted(Wh)
    Mh = {k: np.zeros_like(v) for k, v in Wh.items()}
    expect = None
    for it in range(4):
        out, dx, grads = run(tower)
        assert sorted(grads) == sorted(Wh)
        if expect is not None:
            assert np.isfinite(out).all() and out.tobytes() == expect[0].tobytes(), "iteration %d: the output differs from the fresh tower's" % it
            assert dx.tobytes() == expect[1].tobytes(), "iteration %d: the input gradient differs from the fresh tower's" % it
            assert (out != first_out).mean() > 0.9                # the weights did move
        else:
            first_out = out
        if it == 3:
            break
        assert opt.step() == lrs[it]
        A.sync()
        for k in Wh:
            Wh[k], Mh[k] = OM.sgd_step(Wh[k], grads[k].reshape(Wh[k].shape), Mh[k], lrs[it], 0.9, 1e-3, 1.0, 35.0, 1.0, O.default_wd_mult(k))
        state = opt.state()
        for kw in tower.optimizer_entries():
            assert host(A, kw["weight"]).tobytes() == Wh[kw["name"]].tobytes(), kw["name"]
            assert host(A, state[kw["name"]]).tobytes() == Mh[kw["name"]].tobytes(), kw["name"]
        P2 = dict(P, ws=[Wh[s + "_weight"] for s in stems], ow=Wh[oname + "_weight"], ob=Wh[oname + "_bias"])
        if train:
            P2.update(gs=[Wh[s + "_bn_gamma"] for s in stems], bs=[Wh[s + "_bn_beta"] for s in stems])
        fresh = make(P2, {k: host(A, v) for k, v in tower.aux().items()} if train else None)
        expect = run(fresh)
    assert opt.table_builds == 1 and opt.num_update == 3


@pytest.mark.parametrize("shape", [(1, 3, 9, 64, 8), (2, 2, 37, 128, 1)], ids=["64ch-reg", "128ch-cls"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_tower_loop_train(be, dt, shape):
    tower_loop(be, dt, True, *shape)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_tower_loop_folded_scale(be, dt):
    """HeadTowerBackward: the forward image carries the layer's fold scale"""
    tower_loop(be, dt, False, 1, 3, 9, 64, 8)


# ---- schedulers ------------------------------------------------------------------------------------------------------------------------------
def test_warmup_cosine_values():
    """5 warm-up updates from 0 to 0.02 (N = 4), then 21 cosine updates (N = 20) to 0; the update is clamped to 25"""
    s = O.WarmupCosine(0.02, 0.0, 5, 26)
    ap = lambda v: pytest.approx(v, rel=1e-12, abs=1e-17)       # noqa: E731
    assert s(0) == ap(0.0) and s(1) == ap(0.005) and s(2) == ap(0.01)
    assert s(4) == ap(0.02)                       # the last warm-up update: T = N
    assert s(5) == ap(0.02)                       # the first cosine update: T = 0
    assert s(6) == ap(0.02 * (1 + math.cos(math.pi / 20)) / 2) and s(6) == ap(0.019876883405951378)
    assert s(10) == ap(0.02 * (1 + math.sqrt(0.5)) / 2)          # T / N = 1 / 4
    assert s(15) == ap(0.01)                      # the midpoint: cos(pi / 2)
    assert s(25) == ap(0.0) and s(26) == ap(0.0) and s(1000) == ap(0.0)
    assert all(s(u) >= s(u + 1) for u in range(5, 30))
    w = O.WarmupCosine(0.02, 0.004, 5, 26)        # a warm-up that starts above zero
    assert w(0) == ap(0.004) and w(2) == ap(0.012) and w(4) == ap(0.02)
    n = O.WarmupCosine(0.02, 0.0, 0, 21)          # no warm-up
    assert n(0) == ap(0.02) and n(10) == ap(0.01) and n(20) == ap(0.0)
    for bad in ((5, 6), (1, 26), (-1, 26)):
        with pytest.raises(ValueError):
            O.WarmupCosine(0.02, 0.0, *bad)


def test_warmup_multi_factor_values():
    ap = lambda v: pytest.approx(v, rel=1e-12, abs=1e-17)       # noqa: E731
    g = O.WarmupMultiFactor(0.1, [10, 20], 0.1, "gradual", 0.01, 4)
    assert g(0) == ap(0.01) and g(1) == ap(0.0325) and g(4) == ap(0.1) and g(5) == ap(0.1)
    assert g(10) == ap(0.1) and g(11) == ap(0.01)                # a step takes effect AFTER its update
    assert g(20) == ap(0.01) and g(21) == ap(0.001) and g(500) == ap(0.001)
    c = O.WarmupMultiFactor(0.1, [10, 20], 0.5, "constant", 0.01, 4)
    assert c(0) == 0.01 and c(4) == 0.01 and c(5) == ap(0.1) and c(11) == ap(0.05) and c(21) == ap(0.025)
    assert g(21) == ap(0.001) and g(5) == ap(0.1)                # stateless: any order of calls
    for kw in (dict(step=[10, 10]), dict(step=[10, 20], factor=1.5), dict(step=[10, 20], warmup_type="linear"), dict(step=[10, 20], warmup_step=10)):
        with pytest.raises(ValueError):
            O.WarmupMultiFactor(0.1, **kw)

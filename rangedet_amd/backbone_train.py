"""A backbone BasicBlock in training mode on the device: the step below rangedet_amd.backward's towers.  The DLA backbone is built almost
entirely of `basicblock` units (rangedet_amd/symbol/backbone/dla_backbone.py:31-45, the reference's dla_backbone.py:18-56):

    conv1 3x3 -> BN -> ReLU -> conv2 3x3 -> BN -> (+ shortcut) -> ReLU        shortcut: the block input, or BN(conv 1x1) of it

every BatchNorm with the batch's own statistics (normalizer_factory(type="localbn")).  BasicBlockTrain runs one stride-1 block at 64 or
128 channels forward and backward, DownBlockTrain the stride-(1,2) block that opens res2a, res2, res3a and res3 (its docstring has the
strided steps), ResStageTrain a list of either (ResStageTrain.from_params: a whole `res` stage from the reference's parameter dicts);
with x the input, n = B H W, all arithmetic float32 (csrc/k_norm.h):

    forward   z1 = conv3x3(x, W1); a1, b1 = fold(stats(z1)); y1 = relu(a1 z1 + b1)              conv_unscaled, bn_stats, bn_fold, affine_relu
              z2 = conv3x3(y1, W2); a2, b2 = fold(stats(z2))
              zs = conv1x1(x, Ws); as, bs = fold(stats(zs))                                      projection only
              y = relu(a2 z2 + b2 + u),  u = x  or  as zs + bs                                   affine_add_relu (rd_affine_add_relu)
    backward  dz2, dr, dgamma2, dbeta2 (, dgamma_s, dbeta_s) from g = dL/dy, z2 and r = x or zs  bn_add_relu_bwd (rd_bn_add_relu_bwd)
              dW2 = weight_grad(y1, dz2); g1 = data_grad(dz2, W2)
              dz1, dgamma1, dbeta1 = bn_relu_bwd(g1, z1)
              dW1 = weight_grad(x, dz1)
              dWs = weight_grad1x1(x, dr); ds = conv1x1(dr, Ws transposed)                       projection only
              dx = data_grad(dz1, W1) + (dr or ds)                                               data_grad_add: the add is in that launch's epilogue

The last step passes the shortcut gradient as the persistent conv launch's residual with RD_SCALE_FOLDED | RD_ADD and no ReLU: one float32
add on the accumulator, one rounding (the launch takes that flag combination at every shape: its epilogue reads the flags it is given).
Everything runs on the allocator's current stream without a host synchronisation; buffers are reused between calls of the same shape.
A block keeps float32 masters and both 16-bit images of each conv weight on the device, and optimizer_entries() lists every trainable
parameter the way the towers do: rangedet_amd.optim.SGD.attach(block) registers them and the forward() after a step() runs on the new
weights.  Refused with NotImplementedError: fewer than 64 input channels (res1_unit1), the Meta-Kernel unit, channel counts outside
{64, 128}, an identity shortcut between different channel counts, a strided unit handed to BasicBlockTrain.
AggStageTrain is a whole `agg` stage -- the transposed conv, its BatchNorm and ReLU, the add of the skip, then a ResStageTrain -- forward
and backward (its docstring has the steps), so the gradient of the head levels reaches the `res` stages below.  StemBlockTrain is res1_unit1, the block that reads
the range image itself (1 .. 16 input channels in the 16-channel slot; no dx).
"""
import numpy as np

from . import lib as rdlib
from .backward import BN_EPS, BN_MOMENTUM, TowerOps, _check16, _ops, _vec

_BN_KEYS = ("gamma", "beta", "moving_mean", "moving_var")


# ---- the single steps as functions (host parameters are uploaded on every call: keep a BasicBlockTrain for repeated use) ----------------------
def batch_norm_add_relu_forward(z, a, b, r, ar=None, br=None, relu=True, dtype=rdlib.RD_BF16, lib=None, alloc=None):
    """y = relu(fmaf(z, a, b) + u), u = r or fmaf(r, ar, br); a, b (and ar, br) float32 host vectors of C values"""
    o = _ops(dtype, lib, alloc)
    C = int(z.shape[3])
    av, bv = _vec(o, a, C, "a"), _vec(o, b, C, "b")
    arv, brv = (None, None) if ar is None else (_vec(o, ar, C, "ar"), _vec(o, br, C, "br"))
    return o.affine_add_relu(z, av, bv, r, arv, brv, relu)


def batch_norm_add_relu_backward(g, z, r, saved, gamma, saved_r=None, gamma_r=None, split=0, dtype=rdlib.RD_BF16, lib=None, alloc=None):
    """g = dL/dy; saved (and saved_r for a projection shortcut): dicts of the device buffers a, b, mean, rstd as batch_norm_relu_forward
    returns them; gamma (gamma_r) float32 host vectors -> (dz, dr, dgamma, dbeta, dgamma_r, dbeta_r), the last two None without saved_r"""
    o = _ops(dtype, lib, alloc)
    C = int(z.shape[3])
    return o.bn_add_relu_bwd(g, z, r, saved, _vec(o, gamma, C, "gamma"), saved_r, None if saved_r is None else _vec(o, gamma_r, C, "gamma_r"), split)


def conv1x1_weight_grad(x, dz, dtype=rdlib.RD_BF16, split=0, lib=None, alloc=None):
    """dL/dW (cout, cin, 1, 1) float32 of a stride-1 1x1 conv from its input x and dz; deterministic"""
    return _ops(dtype, lib, alloc).weight_grad1x1(x, dz, split=split)


def conv1x1_data_grad(dz, w_oi, dtype=rdlib.RD_BF16, lib=None, alloc=None):
    """dL/dx of a stride-1 1x1 conv: the 1x1 forward launch on the transposed weight"""
    o = _ops(dtype, lib, alloc)
    w = np.asarray(w_oi, np.float32).reshape(w_oi.shape[0], -1)
    return o.conv1x1(dz, o.pack_conv1x1(np.ascontiguousarray(w.T)), w.shape[0], w.shape[1], ("ds", 0))


def deconv_weight_grad(x, dz, kernel, stride, pad, dtype=rdlib.RD_BF16, split=0, lib=None, alloc=None):
    """dL/dW (Cin, Cout, 3, KW) float32 of a transposed conv with kernel (3, KW), stride (1, s), pad (1, p) from its input x (B, H, Win, Cin)
    and dz (B, H, s Win, Cout); deterministic"""
    return _ops(dtype, lib, alloc).deconv_weight_grad(x, dz, tuple(kernel)[1], tuple(stride)[1], tuple(pad)[1], split=split)


def deconv_data_grad(dz, w_iohw, stride, pad, residual=None, dtype=rdlib.RD_BF16, lib=None, alloc=None):
    """dL/dx (B, H, Win, Cin) of the same transposed conv: one 3x3 launch on dz read as (B, H, Win, s Cout); w (Cin, Cout, 3, KW) float32 on
    the host (packed on every call); residual: another gradient of x, added in the epilogue"""
    o = _ops(dtype, lib, alloc)
    return o.deconv_data_grad(dz, o.pack_deconv_data_grad(w_iohw, tuple(stride)[1], tuple(pad)[1]), residual)


def batch_norm_relu_add_forward(z, a, b, r, dtype=rdlib.RD_BF16, lib=None, alloc=None):
    """y = relu(fmaf(z, a, b)) + r, the join of an aggregation stage; a, b float32 host vectors of C values"""
    o = _ops(dtype, lib, alloc)
    C = int(z.shape[3])
    return o.affine_relu_add(z, _vec(o, a, C, "a"), _vec(o, b, C, "b"), r)


def _bn_params(bn, what):
    if isinstance(bn, dict):
        missing = [k for k in _BN_KEYS if k not in bn]
        if missing:
            raise ValueError("%s: missing %s (a dict of gamma, beta, moving_mean, moving_var)" % (what, ", ".join(missing)))
        return tuple(bn[k] for k in _BN_KEYS)
    if bn is None or len(bn) != 4:
        raise ValueError("%s: (gamma, beta, moving_mean, moving_var)" % what)
    return tuple(bn)


def _block_weights(name, conv1_w, conv2_w):
    """the checks both block kinds share -> (w1, w2, cin, cout)"""
    w1, w2 = np.asarray(conv1_w, np.float32), np.asarray(conv2_w, np.float32)
    if w1.ndim != 4 or w1.shape[2:] != (3, 3) or w2.ndim != 4 or w2.shape[2:] != (3, 3):
        raise ValueError("%s: conv1 and conv2 are (cout, cin, 3, 3) weights, got %r and %r" % (name, w1.shape, w2.shape))
    cout, cin = w1.shape[:2]
    if cin < 64:
        raise NotImplementedError("%s: %d input channels -- fewer than 64 input channels (res1_unit1: the <= 16-channel body form) has no "
                                  "backward here" % (name, cin))
    if cin not in (64, 128) or cout not in (64, 128):
        raise NotImplementedError("%s: %d -> %d channels; the backward kernels run 64 or 128 on either side" % (name, cin, cout))
    if w2.shape[:2] != (cout, cout):
        raise ValueError("%s: conv2 %r after a conv1 with %d outputs" % (name, w2.shape, cout))
    return w1, w2, cin, cout


class _BlockTrain:
    """What BasicBlockTrain (sw = 1) and DownBlockTrain (sw = 2: conv2 and the projection have stride (1, sw)) share: the device copies of
    the parameters, the forward and backward step lists, aux() and optimizer_entries().  A subclass's __init__ makes its own checks and
    calls _build."""
    sw = 1

    def _build(self, name, w1, w2, cin, cout, bn1, bn2, sc_w, sc_bn, dtype, eps, momentum, lib, alloc):
        if (sc_w is None) != (sc_bn is None):
            raise ValueError("%s: sc_w and sc_bn go together" % name)
        self.name = name
        self.ops = o = TowerOps(dtype, lib, alloc)
        self.cin, self.cout, self.proj = cin, cout, sc_w is not None
        self.eps, self.momentum = float(eps), float(momentum)
        A = o.A
        conv2 = dict(fwd=o.pack_unscaled_s2(w2), bwd=o.pack_data_grad_s2(w2)) if self.sw == 2 else dict(fwd=o.pack_unscaled(w2), bwd=o.pack_data_grad(w2))
        self.convs = {"conv1": dict(cin=cin, cout=cout, fwd=o.pack_unscaled(w1), bwd=o.pack_data_grad(w1), master=A.upload(np.ascontiguousarray(w1))),
                      "conv2": dict(conv2, cin=cout, cout=cout, master=A.upload(np.ascontiguousarray(w2)))}
        self.bns = {"bn1": self._bn(bn1, "bn1"), "bn2": self._bn(bn2, "bn2")}
        if self.proj:
            ws = np.asarray(sc_w, np.float32)
            ws = np.ascontiguousarray(ws.reshape(ws.shape[0], -1))
            if ws.shape != (cout, cin):
                raise ValueError("%s: the projection is a (%d, %d[, 1, 1]) weight, got %r" % (name, cout, cin, np.asarray(sc_w).shape))
            self.convs["sc"] = dict(cin=cin, cout=cout, fwd=o.pack_conv1x1(ws), bwd=o.pack_conv1x1(np.ascontiguousarray(ws.T)), master=A.upload(ws))
            self.bns["sc_bn"] = self._bn(sc_bn, "sc_bn")
        self.x = self.saved = None

    def _bn(self, bn, key):
        o, C = self.ops, self.cout
        what = "%s_%s" % (self.name, key)
        return {k: _vec(o, v, C, "%s_%s" % (what, k)) for k, v in zip(_BN_KEYS, _bn_params(bn, what))}

    def _norm(self, z, key, tag, unbiased):
        o, bn = self.ops, self.bns[key]
        mean, var = o.bn_stats(z, tag=tag)
        rstd, a, b = o.bn_fold(mean, var, bn["gamma"], bn["beta"], bn["moving_mean"], bn["moving_var"], int(np.prod(z.shape[:3])), self.cout,
                               self.eps, self.momentum, unbiased, tag=tag)
        return dict(a=a, b=b, mean=mean, var=var, rstd=rstd)

    def forward(self, x, unbiased=True):
        o, cv = self.ops, self.convs
        if _check16(x, "x")[3] != self.cin:
            raise ValueError("%s: %d input channels, conv1 takes %d" % (self.name, int(x.shape[3]), self.cin))
        if int(x.shape[2]) % self.sw:
            raise NotImplementedError("%s: an input of width %d -- the stride-(1,2) unit takes an even width (Wo = Win / 2)" % (self.name, int(x.shape[2])))
        pair = self.sw == 2
        saved = {}
        z1 = o.conv_unscaled(x, cv["conv1"]["fwd"], self.cin, self.cout, tag=1)
        saved["bn1"] = self._norm(z1, "bn1", 1, unbiased)
        y1 = o.affine_relu(z1, saved["bn1"]["a"], saved["bn1"]["b"], tag=1)
        z2 = o.conv_unscaled_s2(y1, cv["conv2"]["fwd"], self.cout, tag=2) if pair else o.conv_unscaled(y1, cv["conv2"]["fwd"], self.cout, self.cout, tag=2)
        saved["bn2"] = self._norm(z2, "bn2", 2, unbiased)
        zs = None
        if self.proj:
            zs = o.conv1x1(x, cv["sc"]["fwd"], self.cin, self.cout, ("zs", 0), pair="in" if pair else None)
            saved["sc_bn"] = self._norm(zs, "sc_bn", "s", unbiased)
        s2, ss = saved["bn2"], saved.get("sc_bn")
        y = o.affine_add_relu(z2, s2["a"], s2["b"], zs if self.proj else x, ss and ss["a"], ss and ss["b"])
        self.x, self.z1, self.y1, self.z2, self.zs, self.saved, self.y = x, z1, y1, z2, zs, saved, y
        return y

    def backward(self, g):
        if self.x is None:
            raise RuntimeError("backward before forward: the activations are kept by forward(x)")
        o, cv, bn, sv, nm = self.ops, self.convs, self.bns, self.saved, self.name
        grads = {}
        r = self.zs if self.proj else self.x
        dz2, dr, grads[nm + "_bn2_gamma"], grads[nm + "_bn2_beta"], dgs, dbs = o.bn_add_relu_bwd(
            g, self.z2, r, sv["bn2"], bn["bn2"]["gamma"], sv.get("sc_bn"), bn["sc_bn"]["gamma"] if self.proj else None, tag=2)
        pair = self.sw == 2
        grads[nm + "_conv2_weight"] = o.weight_grad(self.y1, dz2, tag=2, stride_w=self.sw)
        g1 = o.data_grad_s2(dz2, cv["conv2"]["bwd"], tag=2) if pair else o.data_grad(dz2, cv["conv2"]["bwd"], tag=2)
        dz1, grads[nm + "_bn1_gamma"], grads[nm + "_bn1_beta"] = o.bn_relu_bwd(g1, self.z1, sv["bn1"], bn["bn1"]["gamma"], tag=1)
        grads[nm + "_conv1_weight"] = o.weight_grad(self.x, dz1, tag=1)
        ds = None
        if self.proj:
            grads[nm + "_sc_bn_gamma"], grads[nm + "_sc_bn_beta"] = dgs, dbs
            grads[nm + "_sc_weight"] = o.weight_grad1x1(self.x, dr, tag="s", pair=pair)
            ds = o.conv1x1(dr, cv["sc"]["bwd"], self.cout, self.cin, ("ds", 0), pair="out" if pair else None)
        dx = o.data_grad_add(dz1, cv["conv1"]["bwd"], ds if self.proj else dr, tag=1)
        self.g, self.dz2, self.dr, self.g1, self.dz1, self.ds, self.dx = g, dz2, dr, g1, dz1, ds, dx
        return dx, grads

    def aux(self):
        A, out = self.ops.A, {}
        for key, bn in self.bns.items():
            out["%s_%s_moving_mean" % (self.name, key)] = A.view_f32(bn["moving_mean"], (self.cout,))
            out["%s_%s_moving_var" % (self.name, key)] = A.view_f32(bn["moving_var"], (self.cout,))
        return out

    def optimizer_entries(self):
        """one dict of SGD.add's arguments per trainable parameter: its reference name, the float32 master, the gradient buffer backward()
        fills (keyed by step and tag: its address does not depend on the input shape) and, for a conv weight, the two images a step re-packs"""
        o, nm = self.ops, self.name
        A = o.A
        for key, bkey, tag in (("conv1", "bn1", 1), ("conv2", "bn2", 2)):
            cv = self.convs[key]
            shape = (cv["cout"], cv["cin"], 3, 3)
            pack = dict(fwd=cv["fwd"][0], bwd=cv["bwd"][0], dtype=o.dt)
            if key == "conv2" and self.sw == 2:       # the strided images; the ones select the body form the folded launch reads
                pack.update(stride_w=2, fold_scale=cv["fwd"][2])
            yield dict(name="%s_%s_weight" % (nm, key), weight=A.view_f32(cv["master"], shape),
                       grad=A.view_f32(o.buf(("dW", tag), cv["cout"] * cv["cin"] * 36), shape), pack=pack)
            yield from self._norm_entries(bkey, ("bn_dgamma", tag), ("bn_dbeta", tag))
        if self.proj:
            cv = self.convs["sc"]
            shape = (cv["cout"], cv["cin"], 1, 1)
            yield dict(name=nm + "_sc_weight", weight=A.view_f32(cv["master"], shape),
                       grad=A.view_f32(o.buf(("dW1", "s"), cv["cout"] * cv["cin"] * 4), shape), pack=dict(fwd=cv["fwd"], bwd=cv["bwd"], dtype=o.dt))
            yield from self._norm_entries("sc_bn", ("bn_dgamma_r", 2), ("bn_dbeta_r", 2))

    def _norm_entries(self, bkey, gkey, bkey_grad):
        o, C = self.ops, self.cout
        for k, grad in (("gamma", gkey), ("beta", bkey_grad)):
            yield dict(name="%s_%s_%s" % (self.name, bkey, k), weight=o.A.view_f32(self.bns[bkey][k], (C,)), grad=o.A.view_f32(o.buf(grad, C * 4), (C,)))


class BasicBlockTrain(_BlockTrain):
    """One stride-1 BasicBlock as the reference trains it.
      name               the unit's name in the graph (res2a_unit2, agg1_res_unit1, ...): parameters are <name>_conv1_weight, <name>_bn1_gamma|beta,
                         <name>_conv2_weight, <name>_bn2_gamma|beta and, with a projection, <name>_sc_weight, <name>_sc_bn_gamma|beta
      conv1_w, conv2_w   (cout, cin, 3, 3) and (cout, cout, 3, 3) float32
      bn1, bn2, sc_bn    (gamma, beta, moving_mean, moving_var) or a dict of these: cout values each; the moving statistics are copied to the
                         device once and updated there by every forward()
      sc_w               (cout, cin[, 1, 1]) for a projection shortcut (with sc_bn), None for an identity one
      stride, meta_kernel   what the graph says of the unit; anything but (1, 1) / False is refused (stride (1, 2): DownBlockTrain)
    forward(x) -> y; backward(g) -> (dx, {reference parameter name: float32 gradient}); aux() -> {name: float32 device vector} of the
    moving statistics.  Keeps x, z1, y1, z2, zs and the folded vectors (self.saved) from forward(), and g, dz2, dr, g1, dz1, ds, dx from
    backward()."""

    def __init__(self, name, conv1_w, conv2_w, bn1, bn2, sc_w=None, sc_bn=None, dtype=rdlib.RD_BF16, eps=BN_EPS, momentum=BN_MOMENTUM,
                 stride=(1, 1), meta_kernel=False, lib=None, alloc=None):
        if meta_kernel or conv1_w is None:
            raise NotImplementedError("%s: a Meta-Kernel unit -- its first conv is the Meta-Kernel: rangedet_amd.backward.MetaUnitBackward carries its backward (folded normalisation)" % name)
        if tuple(stride) != (1, 1):
            raise NotImplementedError("%s: stride %r -- this class runs stride-1 units; the strided conv2 and the strided shortcut of a "
                                      "stride-(1, 2) unit (unit 1 of res2a .. res3) are DownBlockTrain" % (name, tuple(stride)))
        w1, w2, cin, cout = _block_weights(name, conv1_w, conv2_w)
        if sc_w is None and cin != cout:
            raise NotImplementedError("%s: an identity shortcut from %d to %d channels -- different channel counts need the projection "
                                      "(sc_w, sc_bn)" % (name, cin, cout))
        self._build(name, w1, w2, cin, cout, bn1, bn2, sc_w, sc_bn, dtype, eps, momentum, lib, alloc)


class StemBlockTrain(_BlockTrain):
    """res1_unit1 as the reference trains it: the BasicBlock that reads the range image itself, c -> 64 with the projection shortcut.  The
    constructor, aux(), the gradient names and optimizer_entries() are BasicBlockTrain's; c = conv1_w.shape[1] is 1 .. 16 (8 for Waymo, 5
    for KITTI) and x is the (B, H, W, 16) range-image slot, of which only the first c channels meet a non-zero weight.

        forward   z1 = conv3x3(x, W1)          conv_unscaled on the <= 16-channel body form (pack_narrow), x_cs = 16
                  y1, z2, zs, y                 as in BasicBlockTrain; zs = conv1x1(x, Ws) on the slot
        backward  dz2, dr, ... = bn_add_relu_bwd(g, z2, zs);  dW2 = weight_grad(y1, dz2);  g1 = data_grad(dz2, W2)
                  dz1, ... = bn_relu_bwd(g1, z1)
                  dW1 = weight_grad_narrow(x, dz1, c, 3);  dWs = weight_grad_narrow(x, dr, c, 1)       rd_conv_bwd_weight_narrow
                  no dx: the range image takes no gradient, backward(g) returns (None, grads)

    optimizer_entries() names conv1 and the projection with pack=dict(narrow=3 | 1, fwd=...): SGD.step() re-packs their forward images from
    the masters (rd_pack_conv_narrow_dev); neither has a data-gradient image.  Keeps x, z1, y1, z2, zs, saved, y from forward() and g, dz2,
    dr, g1, dz1 from backward()."""

    def __init__(self, name, conv1_w, conv2_w, bn1, bn2, sc_w=None, sc_bn=None, dtype=rdlib.RD_BF16, eps=BN_EPS, momentum=BN_MOMENTUM,
                 stride=(1, 1), meta_kernel=False, lib=None, alloc=None):
        if meta_kernel or conv1_w is None or tuple(stride) != (1, 1):
            raise NotImplementedError("%s: a Meta-Kernel or strided unit -- the stem is the stride-1 BasicBlock on the range image" % name)
        w1, w2 = np.ascontiguousarray(conv1_w, dtype=np.float32), np.ascontiguousarray(conv2_w, dtype=np.float32)
        if w1.ndim != 4 or w1.shape[2:] != (3, 3) or w2.shape != (w1.shape[0], w1.shape[0], 3, 3):
            raise ValueError("%s: conv1 (cout, c, 3, 3) and conv2 (cout, cout, 3, 3), got %r and %r" % (name, w1.shape, w2.shape))
        cout, c = w1.shape[:2]
        if not 1 <= c <= 16 or cout != 64:
            raise NotImplementedError("%s: %d -> %d channels; the stem is 1 .. 16 range-image channels -> 64 (64 or more input channels: "
                                      "BasicBlockTrain)" % (name, c, cout))
        if sc_w is None or sc_bn is None:
            raise NotImplementedError("%s: the stem without a projection -- %d channels cannot be added to %d (sc_w, sc_bn)" % (name, c, cout))
        ws = np.asarray(sc_w, np.float32)
        ws = np.ascontiguousarray(ws.reshape(ws.shape[0], -1))
        if ws.shape != (cout, c):
            raise ValueError("%s: the projection is a (%d, %d[, 1, 1]) weight, got %r" % (name, cout, c, np.asarray(sc_w).shape))
        self.name = name
        self.ops = o = TowerOps(dtype, lib, alloc)
        self.cin, self.cout, self.proj = c, cout, True
        self.eps, self.momentum = float(eps), float(momentum)
        A = o.A
        self.convs = {"conv1": dict(cin=c, cout=cout, fwd=o.pack_narrow(w1, 3), master=A.upload(w1)),
                      "conv2": dict(cin=cout, cout=cout, fwd=o.pack_unscaled(w2), bwd=o.pack_data_grad(w2), master=A.upload(w2)),
                      "sc": dict(cin=c, cout=cout, fwd=o.pack_narrow(ws.reshape(cout, c, 1, 1), 1), master=A.upload(ws))}
        self.bns = {"bn1": self._bn(bn1, "bn1"), "bn2": self._bn(bn2, "bn2"), "sc_bn": self._bn(sc_bn, "sc_bn")}
        self.x = self.saved = None

    def forward(self, x, unbiased=True):
        o, cv, c, C = self.ops, self.convs, self.cin, self.cout
        if _check16(x, "x")[3] != 16:
            raise ValueError("%s: %d input channels -- x is the (B, H, W, 16) range-image slot" % (self.name, int(x.shape[3])))
        saved = {}
        z1 = o.conv_unscaled(x, cv["conv1"]["fwd"], c, C, tag=1, x_cs=16)
        saved["bn1"] = self._norm(z1, "bn1", 1, unbiased)
        y1 = o.affine_relu(z1, saved["bn1"]["a"], saved["bn1"]["b"], tag=1)
        z2 = o.conv_unscaled(y1, cv["conv2"]["fwd"], C, C, tag=2)
        saved["bn2"] = self._norm(z2, "bn2", 2, unbiased)
        zs = o.conv1x1(x, cv["sc"]["fwd"], c, C, ("zs", 0), x_cs=16)
        saved["sc_bn"] = self._norm(zs, "sc_bn", "s", unbiased)
        s2, ss = saved["bn2"], saved["sc_bn"]
        y = o.affine_add_relu(z2, s2["a"], s2["b"], zs, ss["a"], ss["b"])
        self.x, self.z1, self.y1, self.z2, self.zs, self.saved, self.y = x, z1, y1, z2, zs, saved, y
        return y

    def backward(self, g):
        if self.x is None:
            raise RuntimeError("backward before forward: the activations are kept by forward(x)")
        o, cv, bn, sv, nm = self.ops, self.convs, self.bns, self.saved, self.name
        grads = {}
        dz2, dr, grads[nm + "_bn2_gamma"], grads[nm + "_bn2_beta"], grads[nm + "_sc_bn_gamma"], grads[nm + "_sc_bn_beta"] = o.bn_add_relu_bwd(
            g, self.z2, self.zs, sv["bn2"], bn["bn2"]["gamma"], sv["sc_bn"], bn["sc_bn"]["gamma"], tag=2)
        grads[nm + "_conv2_weight"] = o.weight_grad(self.y1, dz2, tag=2)
        g1 = o.data_grad(dz2, cv["conv2"]["bwd"], tag=2)
        dz1, grads[nm + "_bn1_gamma"], grads[nm + "_bn1_beta"] = o.bn_relu_bwd(g1, self.z1, sv["bn1"], bn["bn1"]["gamma"], tag=1)
        grads[nm + "_conv1_weight"] = o.weight_grad_narrow(self.x, dz1, self.cin, 3, tag=1)
        grads[nm + "_sc_weight"] = o.weight_grad_narrow(self.x, dr, self.cin, 1, tag="s")
        self.g, self.dz2, self.dr, self.g1, self.dz1 = g, dz2, dr, g1, dz1
        return None, grads

    def optimizer_entries(self):
        o, nm, c, C = self.ops, self.name, self.cin, self.cout
        A, cv = o.A, self.convs
        yield dict(name=nm + "_conv1_weight", weight=A.view_f32(cv["conv1"]["master"], (C, c, 3, 3)),
                   grad=A.view_f32(o.buf(("dWn", 1), C * c * 36), (C, c, 3, 3)), pack=dict(narrow=3, fwd=cv["conv1"]["fwd"][0], dtype=o.dt))
        yield from self._norm_entries("bn1", ("bn_dgamma", 1), ("bn_dbeta", 1))
        yield dict(name=nm + "_conv2_weight", weight=A.view_f32(cv["conv2"]["master"], (C, C, 3, 3)),
                   grad=A.view_f32(o.buf(("dW", 2), C * C * 36), (C, C, 3, 3)), pack=dict(fwd=cv["conv2"]["fwd"][0], bwd=cv["conv2"]["bwd"][0], dtype=o.dt))
        yield from self._norm_entries("bn2", ("bn_dgamma", 2), ("bn_dbeta", 2))
        yield dict(name=nm + "_sc_weight", weight=A.view_f32(cv["sc"]["master"], (C, c, 1, 1)),
                   grad=A.view_f32(o.buf(("dWn", "s"), C * c * 4), (C, c, 1, 1)), pack=dict(narrow=1, fwd=cv["sc"]["fwd"], dtype=o.dt))
        yield from self._norm_entries("sc_bn", ("bn_dgamma_r", 2), ("bn_dbeta_r", 2))


class DownBlockTrain(_BlockTrain):
    """The down-sampling BasicBlock (unit 1 of res2a, res2, res3a, res3): conv2 is 3x3 with stride (1,2) and the mandatory projection
    shortcut 1x1 with stride (1,2).  x is (B, H, Win, cin) with Win even, y (B, H, Win / 2, cout); 64 -> 64, 64 -> 128 or 128 -> 128
    channels.  The arguments, the interface, the parameter names and the kept intermediates are those of BasicBlockTrain; z2, zs, g, dz2,
    dr and y are at half width, x, z1, y1, g1, dz1, ds and dx at full width.  With n = B H Wo for bn2 / sc_bn and B H Win for bn1:

        forward   z1, y1 as in BasicBlockTrain
                  z2 = conv3x3 stride (1,2) of y1        conv_unscaled_s2: the persistent launch on the pixel-pair view of y1
                  zs = conv1x1 of x's even pixels         conv1x1(pair='in')
                  y  = relu(a2 z2 + b2 + as zs + bs)
        backward  dz2, dr, dgamma2, dbeta2, dgamma_s, dbeta_s = bn_add_relu_bwd(g, z2, zs)
                  dW2 = weight_grad(y1, dz2, stride_w=2)                        rd_conv3x3_bwd_weight_ex
                  g1 = data_grad_s2(dz2, W2)                                     the (3,4) / stride 2 / pad 1 transposed conv on W2 with a zero
                                                                                 fourth column (rd_deconv2d_bn_act_all), full width
                  dz1, dgamma1, dbeta1 = bn_relu_bwd(g1, z1);  dW1 = weight_grad(x, dz1)
                  dWs = weight_grad1x1(x, dr, pair=True);  ds = conv1x1(dr, Ws transposed, pair='out')
                  dx = data_grad_add(dz1, W1, ds)

    The rounding sequence of dx: ds[b, h, 2 wo] = round16(float32 sum over co of dr Ws), one rounding per element, written to the even pixels
    of a full-width buffer that is zeroed once when it is made and whose odd pixels no launch writes (+0); then conv1's data gradient adds it
    in its epilogue, dx = round16(float32 accumulator of the 3x3 sum + float32(ds)): one float32 add, one rounding -- on the odd pixels the
    add of +0 changes nothing.  Everything else is rounded as in BasicBlockTrain (every conv output and every dz once, to the activation
    type).  No torch operation and no host synchronisation is on that path.
    optimizer_entries() gives conv2 stride_w = 2 and a device vector of ones as its fold scale (the strided forward image is the folded
    launch's body form, which the packers write only with a scale), so the forward() after SGD.step() runs on the new weights.
    Refused with NotImplementedError: a missing projection, other channel counts, an odd input width (at forward)."""
    sw = 2

    def __init__(self, name, conv1_w, conv2_w, bn1, bn2, sc_w, sc_bn, dtype=rdlib.RD_BF16, eps=BN_EPS, momentum=BN_MOMENTUM, lib=None, alloc=None):
        if conv1_w is None:
            raise NotImplementedError("%s: a Meta-Kernel unit -- its first conv is the Meta-Kernel: rangedet_amd.backward.MetaUnitBackward carries its backward (folded normalisation)" % name)
        if sc_w is None or sc_bn is None:
            raise NotImplementedError("%s: a stride-(1,2) unit without a projection -- the identity cannot halve the width; the reference gives "
                                      "every strided unit the 1x1 shortcut (sc_w, sc_bn)" % name)
        w1, w2, cin, cout = _block_weights(name, conv1_w, conv2_w)
        if (cin, cout) not in ((64, 64), (64, 128), (128, 128)):
            raise NotImplementedError("%s: %d -> %d channels; the strided units of the network are 64 -> 64, 64 -> 128 and 128 -> 128" % (name, cin, cout))
        self._build(name, w1, w2, cin, cout, bn1, bn2, sc_w, sc_bn, dtype, eps, momentum, lib, alloc)


class AggStageTrain:
    """One `agg` stage of the DLA backbone in training mode (dla_backbone.py agg_stage, _AGG_PLAN):

        Deconvolution(up) -> BatchNorm (batch statistics) -> ReLU -> add(skip, .) -> res stage

      name               the stage's name (agg1, agg2, agg2a, agg3): parameters are <name>_deconv_weight, <name>_deconv_bn_gamma | beta, the
                         auxiliary states <name>_deconv_bn_moving_mean | moving_var, and those of the res stage (<name>_res_unit*)
      deconv_w           (Cin, Cout, 3, KW) float32, MXNet's Deconvolution layout
      deconv_bn          (gamma, beta, moving_mean, moving_var) or a dict of these, Cout values each
      res_stage          the ResStageTrain that follows the add (Cout -> Cout, stride 1), or None: the stage ends at the add
      kernel, stride, pad   (3, KW), (1, s), (1, p): (3, 4) / (1, 2) / (1, 1) or (3, 8) / (1, 4) / (1, 2), at the channel pairs of the shipped
                         configs -- 128 -> 128 and 128 -> 64 for (3, 8), 128 -> 64 and 64 -> 64 for (3, 4)
    up is (B, H, Win, Cin), skip (B, H, s Win, Cout).

        forward(skip, up) -> y       z = deconv(up)                          deconv_unscaled (rd_deconv2d_bn_act_all, unscaled, no activation)
                                     a, b = fold(stats(z))                   bn_stats, bn_fold (the moving statistics move on the device)
                                     t = relu(a z + b) + skip                affine_relu_add (rd_affine_relu_add: the ReLU before the add)
                                     y = res_stage.forward(t)
        backward(g, add_to_up=None) -> (d_skip, d_up, grads)
                                     g_t, grads = res_stage.backward(g)
                                     d_skip = g_t                            the same tensor, no copy
                                     dz, dgamma, dbeta = bn_relu_bwd(g_t, z) the mask [a z + b > 0] is recomputed from z
                                     dW = deconv_weight_grad(up, dz)         rd_deconv_bwd_weight, (Cin, Cout, 3, KW) float32
                                     d_up = deconv_data_grad(dz)             ONE persistent 3x3 launch on dz read as (B, H, Win, s Cout)

    add_to_up (B, H, Win, Cin) is another gradient arriving at `up` (res2 and agg2 feed two consumers each in the graph): it is the residual
    of the data-gradient launch, one float32 add on the accumulator and one rounding.  Every conv output and every dz is rounded once to the
    activation type, as in BasicBlockTrain.  The data-gradient launch multiplies the structurally zero third of its weight image too.
    Keeps skip, up, z, t, saved, y from forward() and g, g_t, dz, d_up from backward().  aux() and optimizer_entries() as in the blocks; the
    deconv weight's entry asks for a re-pack of both images (pack=dict(deconv=(KW, s, p), ...)), so the forward() after SGD.step() runs on
    the new weights.  Nothing synchronises with the host.
    Refused with NotImplementedError: other kernels, strides, pads or channel pairs; a skip whose shape is not (B, H, s Win, Cout)."""

    def __init__(self, name, deconv_w, deconv_bn, res_stage, kernel, stride, pad, dtype=rdlib.RD_BF16, eps=BN_EPS, momentum=BN_MOMENTUM,
                 lib=None, alloc=None):
        kernel, stride, pad = tuple(kernel), tuple(stride), tuple(pad)
        if len(kernel) != 2 or len(stride) != 2 or len(pad) != 2 or kernel[0] != 3 or stride[0] != 1 or pad[0] != 1:
            raise NotImplementedError("%s: kernel %r, stride %r, pad %r -- (3, KW), (1, s), (1, p)" % (name, kernel, stride, pad))
        w = np.ascontiguousarray(deconv_w, dtype=np.float32)
        if w.ndim != 4 or tuple(w.shape[2:]) != kernel:
            raise NotImplementedError("%s: a (Cin, Cout, %d, %d) weight for kernel %r, got %r" % (name, kernel[0], kernel[1], kernel, w.shape))
        self.name = name
        self.ops = o = TowerOps(dtype, lib, alloc)
        self.fwd = o.pack_deconv_unscaled(w, stride[1], pad[1])          # (the form and channel checks)
        self.bwd = o.pack_deconv_data_grad(w, stride[1], pad[1])
        self.cin, self.cout, self.kw, self.s, self.p = self.fwd[3]
        self.master = o.A.upload(w)
        what = name + "_deconv_bn"
        self.bn = {k: _vec(o, v, self.cout, "%s_%s" % (what, k)) for k, v in zip(_BN_KEYS, _bn_params(deconv_bn, what))}
        self.eps, self.momentum = float(eps), float(momentum)
        self.res = res_stage
        self.up = self.saved = None

    @classmethod
    def from_params(cls, stage, arg_params, aux_params, num_block, dtype=rdlib.RD_BF16, lib=None, alloc=None):
        """An `agg` stage of the reference from its parameter dicts: <stage>_deconv_weight, <stage>_deconv_bn_gamma | beta in arg_params,
        <stage>_deconv_bn_moving_mean | moving_var in aux_params, and the units <stage>_res_unit1 .. <stage>_res_unit<num_block>
        (ResStageTrain.from_params).  Kernel, stride and pad are those of the stage's name in the backbone's plan."""
        from .symbol.backbone.dla_backbone import _AGG_PLAN
        plan = {row[0]: row[3:] for row in _AGG_PLAN}
        if stage not in plan:
            raise ValueError("%s: not an agg stage of the backbone (%s)" % (stage, ", ".join(sorted(plan))))
        kernel, stride, pad = plan[stage]
        pre = stage + "_deconv_bn_"
        bn = dict(gamma=arg_params[pre + "gamma"], beta=arg_params[pre + "beta"], moving_mean=aux_params[pre + "moving_mean"],
                  moving_var=aux_params[pre + "moving_var"])
        res = ResStageTrain.from_params(stage + "_res", arg_params, aux_params, num_block, dtype=dtype, lib=lib, alloc=alloc)
        return cls(stage, arg_params[stage + "_deconv_weight"], bn, res, kernel, stride, pad, dtype=dtype, lib=lib, alloc=alloc)

    def forward(self, skip, up, unbiased=True):
        o, bn = self.ops, self.bn
        B, H, Win, C = _check16(up, "up")
        if C != self.cin:
            raise ValueError("%s: up has %d channels, the transposed conv takes %d" % (self.name, C, self.cin))
        if _check16(skip, "skip") != (B, H, self.s * Win, self.cout):
            raise NotImplementedError("%s: skip %r with up %r -- the skip is (B, H, %d Win, %d) = %r" % (
                self.name, tuple(skip.shape), tuple(up.shape), self.s, self.cout, (B, H, self.s * Win, self.cout)))
        z = o.deconv_unscaled(up, self.fwd)
        mean, var = o.bn_stats(z, tag="d")
        rstd, a, b = o.bn_fold(mean, var, bn["gamma"], bn["beta"], bn["moving_mean"], bn["moving_var"], B * H * self.s * Win, self.cout,
                               self.eps, self.momentum, unbiased, tag="d")
        t = o.affine_relu_add(z, a, b, skip)
        y = t if self.res is None else self.res.forward(t, unbiased)
        self.skip, self.up, self.z, self.t, self.saved, self.y = skip, up, z, t, dict(a=a, b=b, mean=mean, var=var, rstd=rstd), y
        return y

    def backward(self, g, add_to_up=None):
        if self.up is None:
            raise RuntimeError("backward before forward: the activations are kept by forward(skip, up)")
        o, nm = self.ops, self.name
        g_t, grads = (g, {}) if self.res is None else self.res.backward(g)
        dz, grads[nm + "_deconv_bn_gamma"], grads[nm + "_deconv_bn_beta"] = o.bn_relu_bwd(g_t, self.z, self.saved, self.bn["gamma"], tag="d")
        grads[nm + "_deconv_weight"] = o.deconv_weight_grad(self.up, dz, self.kw, self.s, self.p)
        d_up = o.deconv_data_grad(dz, self.bwd, residual=add_to_up)
        self.g, self.g_t, self.dz, self.d_up = g, g_t, dz, d_up
        return g_t, d_up, grads

    def aux(self):
        A = self.ops.A
        out = {"%s_deconv_bn_%s" % (self.name, k): A.view_f32(self.bn[k], (self.cout,)) for k in ("moving_mean", "moving_var")}
        if self.res is not None:
            out.update(self.res.aux())
        return out

    def optimizer_entries(self):
        """the deconv weight with a re-pack request for both of its images, the BatchNorm vectors, then the res stage's entries"""
        o, nm = self.ops, self.name
        A, shape, C = o.A, (self.cin, self.cout, 3, self.kw), self.cout
        yield dict(name=nm + "_deconv_weight", weight=A.view_f32(self.master, shape),
                   grad=A.view_f32(o.buf(("dWd", 0), self.cin * self.cout * 3 * self.kw * 4), shape),
                   pack=dict(deconv=(self.kw, self.s, self.p), fwd=self.fwd[0], bwd=self.bwd[0], phase_bytes=self.fwd[2], dtype=o.dt))
        for k, grad in (("gamma", "bn_dgamma"), ("beta", "bn_dbeta")):
            yield dict(name="%s_deconv_bn_%s" % (nm, k), weight=A.view_f32(self.bn[k], (C,)), grad=A.view_f32(o.buf((grad, "d"), C * 4), (C,)))
        if self.res is not None:
            yield from self.res.optimizer_entries()


class ResStageTrain:
    """A run of BasicBlockTrain / DownBlockTrain units: forward through the list, backward in reverse with each block's dx fed to the one
    before it; the gradient dicts merged, optimizer_entries() and aux() chained."""

    def __init__(self, blocks):
        self.blocks = list(blocks)
        if not self.blocks:
            raise ValueError("ResStageTrain: at least one block")

    @classmethod
    def from_params(cls, stage, arg_params, aux_params, num_block, stride=(1, 1), dtype=rdlib.RD_BF16, lib=None, alloc=None):
        """The `res` stage of the reference (dla_backbone.py resstage) from its parameter dicts: units <stage>_unit1 .. <stage>_unit<num_block>
        under the reference's names (<unit>_conv1_weight, <unit>_bn1_gamma | beta in arg_params, <unit>_bn1_moving_mean | moving_var in
        aux_params, ...).  Unit 1 has the projection (<unit>_sc_weight, <unit>_sc_bn_*) and the stage's stride: (1, 2) makes it a
        DownBlockTrain; the other units are identity BasicBlockTrain."""
        stride = tuple(stride)
        if stride not in ((1, 1), (1, 2)):
            raise NotImplementedError("%s: stride %r -- (1, 1) or (1, 2)" % (stage, stride))
        if num_block < 1:
            raise ValueError("%s: at least one unit" % stage)

        def bn(unit, key):
            pre = "%s_%s_" % (unit, key)
            return dict(gamma=arg_params[pre + "gamma"], beta=arg_params[pre + "beta"], moving_mean=aux_params[pre + "moving_mean"],
                        moving_var=aux_params[pre + "moving_var"])
        blocks = []
        for i in range(1, num_block + 1):
            unit = "%s_unit%d" % (stage, i)
            args = [unit, arg_params[unit + "_conv1_weight"], arg_params[unit + "_conv2_weight"], bn(unit, "bn1"), bn(unit, "bn2")]
            kw = dict(dtype=dtype, lib=lib, alloc=alloc)
            if i > 1:
                blocks.append(BasicBlockTrain(*args, **kw))
            elif stride == (1, 2):
                blocks.append(DownBlockTrain(*args, arg_params[unit + "_sc_weight"], bn(unit, "sc_bn"), **kw))
            else:
                blocks.append(BasicBlockTrain(*args, arg_params[unit + "_sc_weight"], bn(unit, "sc_bn"), **kw))
        return cls(blocks)

    def forward(self, x, unbiased=True):
        for b in self.blocks:
            x = b.forward(x, unbiased)
        return x

    def backward(self, g):
        grads = {}
        for b in reversed(self.blocks):
            g, gb = b.backward(g)
            grads.update(gb)
        return g, grads

    def optimizer_entries(self):
        for b in self.blocks:
            yield from b.optimizer_entries()

    def aux(self):
        out = {}
        for b in self.blocks:
            out.update(b.aux())
        return out


class MetaBlockTrain(_BlockTrain):
    """res1_unit2 as the reference trains it: the BasicBlock whose first conv is the Meta-Kernel (dla_backbone.py:92-97).
    rangedet_amd.backward.MetaUnitTrain stands in for conv1 + bn1 + relu1 -- both of its BatchNorms with the batch's own statistics --
    then conv2, bn2, the identity add and the ReLU are BasicBlockTrain's steps.
      name, params, W    the unit's name, the reference's parameter dict (arguments and auxiliary states in one dict) and the width the
                         MLP's parameter names carry: <name>_<W>_mlp0|1_weight|bias, <name>point_wise_mlp_bn1_*, <name>aggregation_conv1_weight,
                         <name>aggregation_bn1_*, <name>_conv2_weight, <name>_bn2_*
    forward(x, coord) -> y, x (B, H, W, 64), coord (B, 3, H, W) float32; backward(g) -> (dx, grads): the shortcut's gradient goes in as the
    residual of the Meta-Kernel's data-gradient launch, so dx is rounded once.  aux() and optimizer_entries() chain the unit's."""

    def __init__(self, name, params, W, dtype=rdlib.RD_BF16, eps=BN_EPS, momentum=BN_MOMENTUM, lib=None, alloc=None):
        from .backward import MetaUnitTrain
        w2 = np.ascontiguousarray(params[name + "_conv2_weight"], dtype=np.float32)
        if w2.shape != (64, 64, 3, 3):
            raise ValueError("%s: conv2 is a (64, 64, 3, 3) weight, got %r" % (name, w2.shape))
        self.name = name
        self.meta = MetaUnitTrain(name, params, W, eps=eps, momentum=momentum, dtype=dtype, lib=lib, alloc=alloc)
        self.ops = o = TowerOps(dtype, lib, alloc)
        self.cin = self.cout = 64
        self.proj = False
        self.eps, self.momentum = float(eps), float(momentum)
        self.convs = {"conv2": dict(cin=64, cout=64, fwd=o.pack_unscaled(w2), bwd=o.pack_data_grad(w2), master=o.A.upload(w2))}
        self.bns = {"bn2": self._bn(tuple(params["%s_bn2_%s" % (name, k)] for k in _BN_KEYS), "bn2")}
        self.x = self.saved = None

    def forward(self, x, coord, unbiased=True):
        o, cv = self.ops, self.convs
        y1 = self.meta.forward(x, coord, unbiased)
        z2 = o.conv_unscaled(y1, cv["conv2"]["fwd"], 64, 64, tag=2)
        saved = {"bn2": self._norm(z2, "bn2", 2, unbiased)}
        y = o.affine_add_relu(z2, saved["bn2"]["a"], saved["bn2"]["b"], x)
        self.x, self.y1, self.z2, self.saved, self.y = x, y1, z2, saved, y
        return y

    def backward(self, g):
        if self.x is None:
            raise RuntimeError("backward before forward: the activations are kept by forward(x, coord)")
        o, cv, nm = self.ops, self.convs, self.name
        grads = {}
        dz2, dr, grads[nm + "_bn2_gamma"], grads[nm + "_bn2_beta"], _, _ = o.bn_add_relu_bwd(g, self.z2, self.x, self.saved["bn2"],
                                                                                             self.bns["bn2"]["gamma"], None, None, tag=2)
        grads[nm + "_conv2_weight"] = o.weight_grad(self.y1, dz2, tag=2)
        g1 = o.data_grad(dz2, cv["conv2"]["bwd"], tag=2)
        dx, gm = self.meta.backward(g1, residual=dr)
        grads.update(gm)
        self.g, self.dz2, self.dr, self.g1, self.dx = g, dz2, dr, g1, dx
        return dx, grads

    def aux(self):
        return dict(self.meta.aux(), **super().aux())

    def optimizer_entries(self):
        o, cv = self.ops, self.convs["conv2"]
        yield from self.meta.optimizer_entries()
        yield dict(name=self.name + "_conv2_weight", weight=o.A.view_f32(cv["master"], (64, 64, 3, 3)),
                   grad=o.A.view_f32(o.buf(("dW", 2), 64 * 64 * 36), (64, 64, 3, 3)), pack=dict(fwd=cv["fwd"][0], bwd=cv["bwd"][0], dtype=o.dt))
        yield from self._norm_entries("bn2", ("bn_dgamma", 2), ("bn_dbeta", 2))


class Res1StageTrain:
    """The `res1` stage: StemBlockTrain (res1_unit1, on the range-image slot) then MetaBlockTrain (res1_unit2).  forward(x, coord) with x the
    (B, H, W, 16) range-image slot and coord (B, 3, H, W) float32; backward(g) -> (None, grads): the range image takes no gradient.  The
    rest is ResStageTrain's interface."""

    def __init__(self, stem, meta):
        self.blocks = [stem, meta]

    @classmethod
    def from_params(cls, arg_params, aux_params, W, stage="res1", dtype=rdlib.RD_BF16, lib=None, alloc=None):
        """from the reference's parameter dicts: <stage>_unit1_* is the stem, <stage>_unit2* the Meta-Kernel unit whose MLP names carry W"""
        u1, u2 = stage + "_unit1", stage + "_unit2"

        def bn(key):
            pre = "%s_%s_" % (u1, key)
            return dict(gamma=arg_params[pre + "gamma"], beta=arg_params[pre + "beta"], moving_mean=aux_params[pre + "moving_mean"],
                        moving_var=aux_params[pre + "moving_var"])
        kw = dict(dtype=dtype, lib=lib, alloc=alloc)
        stem = StemBlockTrain(u1, arg_params[u1 + "_conv1_weight"], arg_params[u1 + "_conv2_weight"], bn("bn1"), bn("bn2"),
                              arg_params[u1 + "_sc_weight"], bn("sc_bn"), **kw)
        return cls(stem, MetaBlockTrain(u2, dict(arg_params, **aux_params), W, **kw))

    def forward(self, x, coord, unbiased=True):
        return self.blocks[1].forward(self.blocks[0].forward(x, unbiased), coord, unbiased)

    def backward(self, g):
        g, grads = self.blocks[1].backward(g)
        _, gs = self.blocks[0].backward(g)
        grads.update(gs)
        return None, grads

    def optimizer_entries(self):
        for b in self.blocks:
            yield from b.optimizer_entries()

    def aux(self):
        out = {}
        for b in self.blocks:
            out.update(b.aux())
        return out

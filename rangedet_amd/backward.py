"""Backward through a head tower on the device: the step after rangedet_amd.loss.RpnLoss, which hands back d_logit and d_delta.  A tower
of the reference's head (rangedet/symbol/head/builder.py:221-255) is four `3x3 conv (no bias) + norm + ReLU` layers at 128 channels
and a 1x1 output conv with bias; this module carries the gradient of the output conv down to the tower's input and returns the float32
gradients of every conv weight and of the output bias (the optimiser keeps float32 weights under multi_precision, tools/train.py:358-360).

    out = RpnLoss()(logits, deltas, train)
    tower = HeadTowerBackward(conv_w, scales, shifts, out_w, out_b, kind='cls', level=1, dtype=RD_BF16)
    logit = tower.forward(x)                                   # the unfused launches: every activation is kept
    dx, grads = tower.backward(out['d_logit'], n_off=...)      # grads['rpn_cls_conv_3_lvl_1_weight'], ...

For one layer with z = conv3x3(x, W), y = relu(s z + t) (s, t the folded normalisation) and g = dL/dy:
    dz = g [y > 0] s                     relu_affine_bwd  (the output conv's backward emits the last layer's dz itself)
    dW = sum over pixels of dz x         conv3x3_weight_grad: MFMA kernel, partial sums in a workspace, added in a fixed order
    dx = conv3x3(dz, W flipped)          conv3x3_data_grad: the persistent forward launch on the weight with its channel axes swapped and
                                         its taps flipped (that launch rounds the weight to the activation type)
Everything runs on the allocator's current stream without a host synchronisation; buffers are reused between calls of the same shape,
so a result is valid until the next such call.  TowerOps holds the single steps, one method per library call (conv3x3 is the one forward
conv launch: the towers' forward, the unscaled conv and the data gradient all go through it).  _HeadTower is the skeleton both towers
share -- the layer checks, the parameter names, the output conv, the forward and backward loops; a tower adds its layer parameters, one
layer's forward and the step from dL/dy to dz.  HeadTowerBackward is the tower with inference-mode normalisation (fixed folded s and t);
the level-0 conv_0 (input: the un-materialised 64 + 8 channel concat) and strided / transposed convs are refused there; Level0TowerTrain
is the training-mode tower whose first layer is that concat conv.

HeadTowerTrain is the tower as the reference trains it (normalizer_factory(type="localbn"), mxnext/complicate.py:26-45: BatchNorm with the
batch's own statistics after every conv).  With z = conv3x3(x, W) rounded to the activation type, n = B H W, float32 (csrc/k_norm.h):
    mean, var = statistics of z over B, H, W                       batch_norm_stats (rd_bn_stats: one sweep, deterministic)
    rstd = 1 / sqrt(var + eps), a = gamma rstd, b = beta - mean a   rd_bn_fold, which also updates the moving statistics on the device
    y = relu(a z + b)                                               rd_affine_relu          -- the three: batch_norm_relu_forward
    gy = g [a z + b > 0], zh = (z - mean) rstd
    dbeta = sum gy, dgamma = sum gy zh
    dz = gamma rstd (gy - dbeta / n - zh dgamma / n)                batch_norm_relu_backward (rd_bn_relu_bwd)
and dz feeds the weight and data gradients above directly.

Every tower also keeps float32 master copies of its conv weights on the device next to the two 16-bit images made from them (the output
conv's weight and bias, gamma and beta are float32 device vectors anyway), and optimizer_entries() lists each trainable parameter with
its master, its gradient buffer and its images: rangedet_amd.optim.SGD.attach(tower) registers them, and after SGD.step() the next
forward() and backward() run on the new weights -- no host copy, no new tower.  A tower that is never attached behaves as before.

TowerOps also holds the steps of a backbone BasicBlock (the residual batch norm forward and backward, the 1x1 conv, its weight gradient, the
data gradient with a residual added in its epilogue) and those of its stride-(1,2) form (the strided 3x3 conv, its weight and data
gradients, the 1x1 calls on the pixel-pair view): rangedet_amd.backbone_train builds BasicBlockTrain, DownBlockTrain and ResStageTrain
from them.  The last group is the transposed conv of an aggregation stage -- its unscaled forward, its weight gradient
(rd_deconv_bwd_weight), its data gradient as one 3x3 launch on the s-pixel view of dz -- and the stage's join, relu(a z + b) + skip:
rangedet_amd.backbone_train.AggStageTrain.

The Meta-Kernel unit (res1_unit2) has its own fused backward (csrc/k_metabwd.h): meta_kernel_data_grad and meta_kernel_param_grads are
the single steps, MetaUnitBackward the unit with inference-mode normalisation, forward through rd_meta_kernel_fwd.
"""
import numpy as np

from . import lib as rdlib

_NP16 = np.uint16


def _stream(A):
    return A.stream_ptr(None) if hasattr(A, "stream_ptr") else A.stream


def _view16(A, buf, shape, dtype):
    """(B, H, W, C) view of a byte buffer in the activation type (numpy: raw uint16 bits)"""
    n = int(np.prod(shape)) * 2
    if isinstance(buf, np.ndarray):
        return buf[:n].view(_NP16).reshape(shape)
    t = A.torch
    return buf[:n].view(t.bfloat16 if dtype == rdlib.RD_BF16 else t.float16).view(*shape)


def _check16(x, what):
    if len(x.shape) != 4:
        raise ValueError("%s: a dense channels-last (B, H, W, C) tensor of the 16-bit activation type, got shape %r" % (what, tuple(x.shape)))
    if hasattr(x, "is_contiguous") and not x.is_contiguous():
        raise ValueError("%s: not contiguous" % what)
    item = x.itemsize if isinstance(x, np.ndarray) else x.element_size()
    if item != 2:
        raise ValueError("%s: 2-byte elements (bf16 / fp16 bits), got %d-byte ones" % (what, item))
    return tuple(int(v) for v in x.shape)


class TowerOps:
    """The single steps on one (lib, allocator, dtype); buffers keyed by (step, shape, tag)."""

    def __init__(self, dtype=rdlib.RD_BF16, lib=None, alloc=None):
        if dtype not in rdlib.H16:
            raise NotImplementedError("backward: 16-bit activations only (RD_BF16 / RD_F16); float32 is the accumulator and weight-gradient type")
        self.dt = dtype
        self.L = lib or rdlib.get_lib()
        if alloc is None:
            from .runtime import TorchAllocator
            alloc = TorchAllocator()
        self.A = alloc
        self._bufs = {}

    def buf(self, key, nbytes, zero=False):
        """zero: zeroed when it is first made (a buffer of which only a part is ever written keeps zeros elsewhere)"""
        k = (key, nbytes)
        if k not in self._bufs:
            self._bufs[k] = self.A.alloc(nbytes, zero=True) if zero else self.A.alloc(nbytes)
        return self._bufs[k]

    def pack_data_grad(self, w_oihw):
        """the forward launch's weight image of the data gradient: axes swapped, taps flipped, no scale"""
        w = np.asarray(w_oihw, np.float32)
        cout, cin = w.shape[:2]
        wf = np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])
        return self.A.upload(self.L.pack_conv3x3_ex(wf, 1, cout, fold_scale=None, dtype=self.dt)), self.A.upload(np.zeros(cin, np.float32)), cin

    def conv3x3(self, x, image, shift, cin, cout, flags, key, x_cs=None):
        """the persistent forward launch: x (B, H, W, cin) -> (B, H, W, cout) in the buffer `key`; image a packed weight, shift cout float32.
        x_cs: the channel stride of x when it is wider than cin (the 16-channel range-image slot)"""
        A = self.A
        B, H, W = _check16(x, "x")[:3]
        out = self.buf(key, B * H * W * cout * 2)
        self.L.call("rd_conv3x3_bn_act_ex", rdlib.ptr(x), x_cs or cin, 0, A.ptr(image), None, A.ptr(shift), None, 0, 0, None, 0, 0, 0, None,
                    A.ptr(out), cout, 0, B, H, W, cin, cout, 1, flags, self.dt, _stream(A))
        return _view16(A, out, (B, H, W, cout), self.dt)

    def data_grad(self, dz, packed, tag=0):
        """dz (B, H, W, cout) -> dx (B, H, W, cin); packed = pack_data_grad(W)"""
        img, zero_shift, cin = packed
        return self.conv3x3(dz, img, zero_shift, _check16(dz, "dz")[3], cin, rdlib.RD_SCALE_FOLDED, ("dx", tag))

    def weight_grad(self, x, dz, tag=0, split=0, stride_w=1):
        """x (B, H, W, cin), dz (B, H, W / stride_w, cout) -> dW (cout, cin, 3, 3) float32; stride_w 2: the stride-(1,2) conv
        (rd_conv3x3_bwd_weight_ex), W even"""
        A, L = self.A, self.L
        B, H, W, cin = _check16(x, "x")
        if stride_w not in (1, 2) or W % stride_w:
            raise NotImplementedError("weight_grad: stride_w %r with W %d -- 1, or 2 with an even width" % (stride_w, W))
        if _check16(dz, "dz")[:3] != (B, H, W // stride_w):
            raise ValueError("weight_grad: x %r and dz %r differ in B, H or W / %d" % (tuple(x.shape), tuple(dz.shape), stride_w))
        cout = int(dz.shape[3])
        if cin not in (64, 128) or cout not in (64, 128):
            raise NotImplementedError("weight_grad: %d -> %d channels; the kernel runs 64 or 128 on either side" % (cin, cout))
        if stride_w == 2:
            nws = L.raw("rd_conv3x3_bwd_weight_ex_workspace_bytes")(B, H, W, cin, cout, 2, split)
            ws, out = self.buf(("bww_ws", 0), nws), self.buf(("dW", tag), cout * cin * 36)
            L.call("rd_conv3x3_bwd_weight_ex", rdlib.ptr(x), cin, 0, rdlib.ptr(dz), cout, 0, A.ptr(out), B, H, W, cin, cout, 2, split, self.dt,
                   A.ptr(ws), nws, _stream(A))
            return A.view_f32(out, (cout, cin, 3, 3))
        nws = L.raw("rd_conv3x3_bwd_weight_workspace_bytes")(B, H, W, cin, cout, split)
        ws, out = self.buf(("bww_ws", 0), nws), self.buf(("dW", tag), cout * cin * 36)
        L.call("rd_conv3x3_bwd_weight", rdlib.ptr(x), cin, 0, rdlib.ptr(dz), cout, 0, A.ptr(out), B, H, W, cin, cout, split, self.dt, A.ptr(ws),
               nws, _stream(A))
        return A.view_f32(out, (cout, cin, 3, 3))

    def weight_grad_narrow(self, x, dz, cin, ksize, tag=0, split=0):
        """x (B, H, W, 16): the range-image slot, of which the first cin channels are the conv's input; dz (B, H, W, cout) -> dW (cout, cin,
        ksize, ksize) float32 (rd_conv_bwd_weight_narrow: ksize 3 pad 1, or ksize 1)"""
        A, L = self.A, self.L
        B, H, W, slot = _check16(x, "x")
        if _check16(dz, "dz")[:3] != (B, H, W):
            raise ValueError("weight_grad_narrow: x %r and dz %r differ in B, H or W" % (tuple(x.shape), tuple(dz.shape)))
        cout = int(dz.shape[3])
        if slot != 16 or not 1 <= cin <= 16 or cout not in (64, 128) or ksize not in (1, 3):
            raise NotImplementedError("weight_grad_narrow: %d of %d slot channels -> %d, ksize %r; the kernel reads a 16-channel slot with 1 .. 16 "
                                      "input channels, 64 or 128 output channels, ksize 1 or 3" % (cin, slot, cout, ksize))
        nws = L.raw("rd_conv_bwd_weight_narrow_workspace_bytes")(B, H, W, cin, cout, ksize, split)
        ws, out = self.buf(("bwn_ws", 0), nws), self.buf(("dWn", tag), cout * cin * ksize * ksize * 4)
        L.call("rd_conv_bwd_weight_narrow", rdlib.ptr(x), 16, 0, rdlib.ptr(dz), cout, 0, A.ptr(out), cin, 0, B, H, W, cin, cout, ksize, split, self.dt,
               A.ptr(ws), nws, _stream(A))
        return A.view_f32(out, (cout, cin, ksize, ksize))

    def weight_grad_cat(self, x1, x2, cin2, dz, tag=0, split=0, cin_stride=None):
        """the concat conv [x1 | first cin2 channels of x2] -> cout: x1 (B, H, W, 64), x2 (B, H, W, 16) the range-image slot, dz (B, H, W, cout)
        -> dW (cout, 64 + cin2, 3, 3) float32 (rd_conv3x3_bwd_weight_cat).  cin_stride > 64 + cin2: dW is (cout, cin_stride, 3, 3), a buffer
        zeroed when it is made whose channels from 64 + cin2 on no launch writes (rd_conv3x3_bwd_weight_cat_padded)"""
        A, L = self.A, self.L
        B, H, W, cin1 = _check16(x1, "x1")
        if _check16(x2, "x2")[:3] != (B, H, W) or _check16(dz, "dz")[:3] != (B, H, W):
            raise ValueError("weight_grad_cat: x1 %r, x2 %r and dz %r differ in B, H or W" % (tuple(x1.shape), tuple(x2.shape), tuple(dz.shape)))
        cout = int(dz.shape[3])
        if cin1 != 64 or int(x2.shape[3]) != 16 or not 1 <= cin2 <= 16 or cout not in (64, 128):
            raise NotImplementedError("weight_grad_cat: %d + %d of %d slot channels -> %d; 64 + (1 .. 16 of a 16-channel slot) -> 64 or 128"
                                      % (cin1, cin2, int(x2.shape[3]), cout))
        nws = L.raw("rd_conv3x3_bwd_weight_cat_workspace_bytes")(B, H, W, cin1, cin2, cout, split)
        cs = cin_stride or cin1 + cin2
        if cs < cin1 + cin2:
            raise ValueError("weight_grad_cat: cin_stride %d below %d + %d channels" % (cs, cin1, cin2))
        ws, out = self.buf(("bwc_ws", 0), nws), self.buf(("dWc", tag), cout * cs * 36, zero=True)
        if cs == cin1 + cin2:
            L.call("rd_conv3x3_bwd_weight_cat", rdlib.ptr(x1), cin1, 0, cin1, rdlib.ptr(x2), 16, 0, cin2, rdlib.ptr(dz), cout, 0, A.ptr(out), B, H, W,
                   cout, split, self.dt, A.ptr(ws), nws, _stream(A))
        else:
            L.call("rd_conv3x3_bwd_weight_cat_padded", rdlib.ptr(x1), cin1, 0, cin1, rdlib.ptr(x2), 16, 0, cin2, rdlib.ptr(dz), cout, 0, A.ptr(out), cs,
                   B, H, W, cout, split, self.dt, A.ptr(ws), nws, _stream(A))
        return A.view_f32(out, (cout, cs, 3, 3))

    # The launch images of these convs.  The forward launches read the <= 16-channel and the concat body forms, which the host packers write
    # only when they are given a fold scale: the unscaled training image is packed with a vector of ones (1.0f * w is w), and the device
    # packers take fold = None to mean exactly that.
    def pack_narrow(self, w, ksize):
        """(cout, cin, ksize, ksize), cin <= 16 -> ksize 3: (image, zero shift) for conv_unscaled(x, ., cin, cout, x_cs=16); ksize 1: the
        image conv1x1(x, ., cin, cout, key, x_cs=16) reads"""
        w = np.ascontiguousarray(w, dtype=np.float32)
        cout, cin = w.shape[:2]
        if w.shape[2:] != (ksize, ksize) or ksize not in (1, 3) or not 1 <= cin <= 16 or cout not in (64, 128):
            raise NotImplementedError("pack_narrow: a (cout, cin, %r, %r) weight with ksize 1 or 3, cin 1 .. 16, cout 64 or 128, got %r" % (ksize, ksize, w.shape))
        if ksize == 1:
            return self.pack_conv1x1(w)
        image = self.L.pack_conv3x3_ex(w, 1, cin, fold_scale=np.ones(cout, np.float32), dtype=self.dt)
        return self.A.upload(image), self.A.upload(np.zeros(cout, np.float32))

    def pack_narrow_dev(self, master, cout, cin, ksize, image, fold_scale=None):
        """the same image from the device-resident float32 master, one launch (rd_pack_conv_narrow_dev)"""
        self.L.call("rd_pack_conv_narrow_dev", rdlib.ptr(master), None if fold_scale is None else rdlib.ptr(fold_scale), cout, cin, ksize, self.dt,
                    rdlib.ptr(image), _stream(self.A))

    def pack_cat(self, w, cin2):
        """(cout, 64 + cin2, 3, 3), cin2 8 or 16 -> (image, zero shift) of the unscaled concat conv (conv3x3_cat)"""
        w = np.ascontiguousarray(w, dtype=np.float32)
        cout = w.shape[0]
        if w.shape[1:] != (64 + cin2, 3, 3) or cin2 not in (8, 16) or cout not in (64, 128):
            raise NotImplementedError("pack_cat: a (cout, 64 + cin2, 3, 3) weight with cin2 8 or 16 (the forward reads a multiple of 8) and cout 64 "
                                      "or 128, got %r with cin2 %r" % (w.shape, cin2))
        image = self.L.pack_conv3x3_cat(w, 64, cin2, fold_scale=np.ones(cout, np.float32), dtype=self.dt)
        return self.A.upload(image), self.A.upload(np.zeros(cout, np.float32))

    def pack_cat_dev(self, master, cout, cin2, data_grad, image, fold_scale=None):
        """the forward image (data_grad False) or the image of the data gradient towards x1 (True) of the concat conv from the device-resident
        (cout, 64 + cin2, 3, 3) master, one launch (rd_pack_conv3x3_cat_dev)"""
        self.L.call("rd_pack_conv3x3_cat_dev", rdlib.ptr(master), None if fold_scale is None else rdlib.ptr(fold_scale), cout, 64, cin2,
                    1 if data_grad else 0, self.dt, rdlib.ptr(image), _stream(self.A))

    def conv3x3_cat(self, x1, x2, cin2, packed, cout, tag=0):
        """z = conv3x3([x1 | first cin2 channels of x2], W) rounded to the activation type, unscaled (rd_conv3x3_bn_act_cat on the never-written
        concat): x1 (B, H, W, 64), x2 (B, H, W, 16) the range-image slot, cin2 8 or 16, packed = pack_cat(W, cin2)"""
        A = self.A
        B, H, W, cin1 = _check16(x1, "x1")
        if _check16(x2, "x2") != (B, H, W, 16) or cin1 != 64 or cin2 not in (8, 16):
            raise NotImplementedError("conv3x3_cat: x1 %r, x2 %r, cin2 %r -- (B, H, W, 64), the (B, H, W, 16) slot, 8 or 16" % (tuple(x1.shape), tuple(x2.shape), cin2))
        out = self.buf(("z", tag), B * H * W * cout * 2)
        self.L.call("rd_conv3x3_bn_act_cat", rdlib.ptr(x1), cin1, 0, cin1, rdlib.ptr(x2), 16, 0, cin2, A.ptr(packed[0]), A.ptr(packed[1]), A.ptr(out),
                    cout, 0, B, H, W, cout, rdlib.RD_SCALE_FOLDED, self.dt, _stream(A))
        return _view16(A, out, (B, H, W, cout), self.dt)

    def relu_affine_bwd(self, g, y, scale, tag=0):
        """g, y (B, H, W, C), scale a device float32 buffer of C values or None -> dz"""
        A, L = self.A, self.L
        B, H, W, C = _check16(g, "g")
        out = self.buf(("dz", tag), B * H * W * C * 2)
        L.call("rd_relu_affine_bwd", rdlib.ptr(g), C, 0, None if y is None else rdlib.ptr(y), C, 0, None if scale is None else A.ptr(scale),
               A.ptr(out), C, 0, B, H, W, C, self.dt, _stream(A))
        return _view16(A, out, (B, H, W, C), self.dt)

    def head_out_bwd(self, d_out, x, w_dev, nout, n_off=0, out_batch_stride=None, scale=None, relu_mask=False, tag=0):
        """d_out: float32 device tensor (B, ...) holding [n_off + pixel][nout] per frame; x (B, H, W, cin); w_dev: (nout, cin) float32 device
        buffer -> dx (B, H, W, cin) (times [x > 0] with relu_mask, times scale[c] with scale), dw (nout, cin), dbias (nout)"""
        A, L = self.A, self.L
        B, H, W, cin = _check16(x, "x")
        if cin not in (64, 128) or not 1 <= nout <= 8:
            raise NotImplementedError("head_out_bwd: cin %d (64 or 128), nout %d (1..8)" % (cin, nout))
        obs = int(np.prod(d_out.shape[1:])) if out_batch_stride is None else int(out_batch_stride)
        if int(d_out.shape[0]) != B or obs < (n_off + H * W) * nout:
            raise ValueError("head_out_bwd: d_out %r does not hold %d frames of (%d + %d) x %d values" % (tuple(d_out.shape), B, n_off, H * W, nout))
        nws = L.raw("rd_head_out_bwd_workspace_bytes")(B, H, W, cin, nout)
        ws, dx = self.buf(("hob_ws", 0), nws), self.buf(("hob_dx", tag), B * H * W * cin * 2)
        dw, db = self.buf(("hob_dw", tag), nout * cin * 4), self.buf(("hob_db", tag), nout * 4)
        L.call("rd_head_out_bwd", rdlib.ptr(d_out), obs, n_off, rdlib.ptr(x), cin, 0, A.ptr(w_dev), 1 if relu_mask else 0,
               None if scale is None else A.ptr(scale), A.ptr(dx), cin, 0, A.ptr(dw), A.ptr(db), B, H, W, cin, nout, self.dt, A.ptr(ws), nws,
               _stream(A))
        return _view16(A, dx, (B, H, W, cin), self.dt), A.view_f32(dw, (nout, cin)), A.view_f32(db, (nout,))

    # ---- training-mode batch norm (csrc/k_norm.h); every vector below is a device buffer of C float32 values ------------------------------
    def conv_unscaled(self, x, packed, cin, cout, tag=0, x_cs=None):
        """z = conv3x3(x, W) rounded to the activation type: the persistent launch on an unscaled weight image, zero shift, no activation;
        packed = (image, zero shift) as pack_unscaled (or, for at most 16 input channels in a slot of x_cs, pack_narrow) makes them"""
        return self.conv3x3(x, packed[0], packed[1], cin, cout, rdlib.RD_SCALE_FOLDED, ("z", tag), x_cs)

    def pack_unscaled(self, w_oihw):
        w = np.asarray(w_oihw, np.float32)
        cout, cin = w.shape[:2]
        return self.A.upload(self.L.pack_conv3x3_ex(w, 1, cin, fold_scale=None, dtype=self.dt)), self.A.upload(np.zeros(cout, np.float32))

    def _norm_ws(self, entry, z, split):
        B, H, W, C = _check16(z, "z")
        nws = self.L.raw(entry)(B, H, W, C, split)
        if not nws:
            raise NotImplementedError("%s: %d channels (8, 16, 32, 64, 128 or 256) with split %d" % (entry[:-16], C, split))
        return (B, H, W, C), self.buf(("norm_ws", 0), nws), nws

    def bn_stats(self, z, split=0, tag=0):
        """z (B, H, W, C) -> the buffers of mean and biased variance over B, H, W"""
        A, L = self.A, self.L
        (B, H, W, C), ws, nws = self._norm_ws("rd_bn_stats_workspace_bytes", z, split)
        mean, var = self.buf(("bn_mean", tag), C * 4), self.buf(("bn_var", tag), C * 4)
        L.call("rd_bn_stats", rdlib.ptr(z), C, 0, A.ptr(mean), A.ptr(var), B, H, W, C, split, self.dt, A.ptr(ws), nws, _stream(A))
        return mean, var

    def bn_fold(self, mean, var, gamma, beta, moving_mean, moving_var, n, C, eps, momentum, unbiased=True, tag=0):
        """-> the buffers rstd, a, b; moving_mean / moving_var (buffers or None) are updated in place"""
        A = self.A
        rstd, a, b = (self.buf((k, tag), C * 4) for k in ("bn_rstd", "bn_a", "bn_b"))
        self.L.call("rd_bn_fold", A.ptr(mean), A.ptr(var), A.ptr(gamma), A.ptr(beta), eps, momentum, n, 1 if unbiased else 0, A.ptr(rstd), A.ptr(a),
                    A.ptr(b), None if moving_mean is None else A.ptr(moving_mean), None if moving_var is None else A.ptr(moving_var), C, _stream(A))
        return rstd, a, b

    def affine_relu(self, z, a, b, relu=True, tag=0):
        A = self.A
        B, H, W, C = _check16(z, "z")
        out = self.buf(("bn_y", tag), B * H * W * C * 2)
        self.L.call("rd_affine_relu", rdlib.ptr(z), C, 0, A.ptr(a), A.ptr(b), 1 if relu else 0, A.ptr(out), C, 0, B, H, W, C, self.dt, _stream(A))
        return _view16(A, out, (B, H, W, C), self.dt)

    def bn_relu_bwd(self, g, z, saved, gamma, relu=True, split=0, tag=0):
        """g, z (B, H, W, C); saved: the dict of buffers a, b, mean, rstd the forward kept -> dz, dgamma (C,), dbeta (C,)"""
        A, L = self.A, self.L
        (B, H, W, C), ws, nws = self._norm_ws("rd_bn_relu_bwd_workspace_bytes", z, split)
        if _check16(g, "g") != (B, H, W, C):
            raise ValueError("bn_relu_bwd: g %r and z %r differ" % (tuple(g.shape), tuple(z.shape)))
        dz, dg, db = self.buf(("bn_dz", tag), B * H * W * C * 2), self.buf(("bn_dgamma", tag), C * 4), self.buf(("bn_dbeta", tag), C * 4)
        L.call("rd_bn_relu_bwd", rdlib.ptr(g), C, 0, rdlib.ptr(z), C, 0, A.ptr(saved["a"]), A.ptr(saved["b"]), A.ptr(saved["mean"]), A.ptr(saved["rstd"]),
               A.ptr(gamma), 1 if relu else 0, A.ptr(dz), C, 0, A.ptr(dg), A.ptr(db), B, H, W, C, split, self.dt, A.ptr(ws), nws, _stream(A))
        return _view16(A, dz, (B, H, W, C), self.dt), A.view_f32(dg, (C,)), A.view_f32(db, (C,))

    # ---- the residual BatchNorm and the 1x1 conv of a backbone BasicBlock (rangedet_amd.backbone_train) ------------------------------------
    def affine_add_relu(self, z, a, b, r, ar=None, br=None, relu=True, tag=0):
        """y = relu(fmaf(z, a, b) + u), u = r (identity shortcut) or fmaf(r, ar, br) (projection); z, r (B, H, W, C)"""
        A = self.A
        B, H, W, C = _check16(z, "z")
        if _check16(r, "r") != (B, H, W, C):
            raise ValueError("affine_add_relu: z %r and r %r differ" % (tuple(z.shape), tuple(r.shape)))
        out = self.buf(("bn_add_y", tag), B * H * W * C * 2)
        self.L.call("rd_affine_add_relu", rdlib.ptr(z), C, 0, A.ptr(a), A.ptr(b), rdlib.ptr(r), C, 0, None if ar is None else A.ptr(ar),
                    None if br is None else A.ptr(br), 1 if relu else 0, A.ptr(out), C, 0, B, H, W, C, self.dt, _stream(A))
        return _view16(A, out, (B, H, W, C), self.dt)

    def bn_add_relu_bwd(self, g, z, r, saved, gamma, saved_r=None, gamma_r=None, split=0, tag=0):
        """g, z, r (B, H, W, C); saved (and, for a projection shortcut, saved_r): the dicts of buffers a, b, mean, rstd the forward kept ->
        dz, dr, dgamma, dbeta, and dgamma_r, dbeta_r (None for an identity shortcut)"""
        A, L = self.A, self.L
        B, H, W, C = _check16(z, "z")
        if _check16(g, "g") != (B, H, W, C) or _check16(r, "r") != (B, H, W, C):
            raise ValueError("bn_add_relu_bwd: g %r, z %r and r %r differ" % (tuple(g.shape), tuple(z.shape), tuple(r.shape)))
        proj = saved_r is not None
        nws = L.raw("rd_bn_add_relu_bwd_workspace_bytes")(B, H, W, C, split, 1 if proj else 0)
        if not nws:
            raise NotImplementedError("rd_bn_add_relu_bwd: %d channels (8, 16, 32, 64, 128 or 256) with split %d" % (C, split))
        ws = self.buf(("norm_ws", 0), nws)
        dz, dr = self.buf(("bn_add_dz", tag), B * H * W * C * 2), self.buf(("bn_add_dr", tag), B * H * W * C * 2)
        dg, db = self.buf(("bn_dgamma", tag), C * 4), self.buf(("bn_dbeta", tag), C * 4)
        dgr, dbr = (self.buf(("bn_dgamma_r", tag), C * 4), self.buf(("bn_dbeta_r", tag), C * 4)) if proj else (None, None)
        sr = [A.ptr(saved_r[k]) for k in ("a", "b", "mean", "rstd")] + [A.ptr(gamma_r)] if proj else [None] * 5
        L.call("rd_bn_add_relu_bwd", rdlib.ptr(g), C, 0, rdlib.ptr(z), C, 0, rdlib.ptr(r), C, 0, A.ptr(saved["a"]), A.ptr(saved["b"]),
               A.ptr(saved["mean"]), A.ptr(saved["rstd"]), A.ptr(gamma), *sr, A.ptr(dz), C, 0, A.ptr(dr), C, 0, A.ptr(dg), A.ptr(db),
               None if dgr is None else A.ptr(dgr), None if dbr is None else A.ptr(dbr), B, H, W, C, split, self.dt, A.ptr(ws), nws, _stream(A))
        v16, vf = (lambda b_: _view16(A, b_, (B, H, W, C), self.dt)), (lambda b_: None if b_ is None else A.view_f32(b_, (C,)))
        return v16(dz), v16(dr), vf(dg), vf(db), vf(dgr), vf(dbr)

    def pack_conv1x1(self, w_oi):
        """the image rd_conv2d_bn_act reads for a 1x1 conv with the (cout, cin) weight: no scale, one tap"""
        w = np.ascontiguousarray(np.asarray(w_oi, np.float32).reshape(w_oi.shape[0], -1))
        return self.A.upload(self.L.pack_conv_weight(w.reshape(w.shape + (1, 1)), self.dt))

    def conv1x1(self, x, image, cin, cout, key, pair=None, x_cs=None):
        """x (B, H, W, cin) -> conv1x1(x, W) rounded to the activation type, in the buffer `key`; image = pack_conv1x1(W).  With the image of
        the transposed weight this is the 1x1 conv's data gradient.  The stride-(1,2) 1x1 conv runs the same launch on the pixel-pair view,
        a row of W pixels read as W / 2 pixels of twice the channel stride whose first cin (cout) channels are the even pixel:
          pair='in'    x (B, H, W, cin), W even -> (B, H, W / 2, cout): the conv of the even pixels, the strided forward
          pair='out'   x (B, H, Wo, cin) -> (B, H, 2 Wo, cout): the result on the even pixels, +0 on the odd ones (the buffer is zeroed when
                       it is made and its odd pixels are never written), the strided conv's data gradient
        x_cs: the channel stride of x when it is wider than cin (the 16-channel range-image slot)"""
        A = self.A
        B, H, W = _check16(x, "x")[:3]
        if pair not in (None, "in", "out") or (pair == "in" and W % 2):
            raise NotImplementedError("conv1x1: pair %r with W %d -- None, 'in' with an even width, or 'out'" % (pair, W))
        Wl, Wout = (W // 2, W // 2) if pair == "in" else (W, 2 * W if pair == "out" else W)
        out = self.buf(key, B * H * Wout * cout * 2, zero=pair == "out")
        self.L.call("rd_conv2d_bn_act", rdlib.ptr(x), (x_cs or cin) * (2 if pair == "in" else 1), 0, A.ptr(image), None, None, None, 0, 0, A.ptr(out),
                    cout * (2 if pair == "out" else 1), 0, B, H, Wl, cin, cout, 1, 1, 1, 0, self.dt, _stream(A))
        return _view16(A, out, (B, H, Wout, cout), self.dt)

    def weight_grad1x1(self, x, dz, tag=0, split=0, pair=False):
        """x (B, H, W, cin), dz (B, H, W, cout) -> dW (cout, cin, 1, 1) float32.  pair: the stride-(1,2) conv -- dz (B, H, W / 2, cout) against
        the even pixels of x, read through the pixel-pair view (channel stride 2 cin; W even keeps the flat pixel axis whole)"""
        A, L = self.A, self.L
        B, H, W, cin = _check16(x, "x")
        if pair and W % 2:
            raise NotImplementedError("weight_grad1x1: the pixel-pair view of a row of %d pixels (an even width)" % W)
        Wl = W // 2 if pair else W
        if _check16(dz, "dz")[:3] != (B, H, Wl):
            raise ValueError("weight_grad1x1: x %r and dz %r differ in B, H or W%s" % (tuple(x.shape), tuple(dz.shape), " / 2" if pair else ""))
        cout = int(dz.shape[3])
        if cin not in (64, 128) or cout not in (64, 128):
            raise NotImplementedError("weight_grad1x1: %d -> %d channels; the kernel runs 64 or 128 on either side" % (cin, cout))
        nws = L.raw("rd_conv1x1_bwd_weight_workspace_bytes")(B, H, Wl, cin, cout, split)
        ws, out = self.buf(("bww_ws", 0), nws), self.buf(("dW1", tag), cout * cin * 4)
        L.call("rd_conv1x1_bwd_weight", rdlib.ptr(x), cin * (2 if pair else 1), 0, rdlib.ptr(dz), cout, 0, A.ptr(out), B, H, Wl, cin, cout, split,
               self.dt, A.ptr(ws), nws, _stream(A))
        return A.view_f32(out, (cout, cin, 1, 1))

    # ---- the stride-(1,2) 3x3 conv of a down-sampling BasicBlock (C -> C, C 64 or 128) -----------------------------------------------------
    def pack_unscaled_s2(self, w_oihw):
        """(image, zero shift, ones) of the strided conv: rd_pack_conv3x3_ex_host on the pixel-pair view.  The packer writes the body form a
        RD_SCALE_FOLDED launch reads only when it is given a fold scale, so it gets a vector of ones (1.0f * w is w); the same vector on
        the device is the entry's fold_scale, with which an optimizer step re-packs that form"""
        w = np.asarray(w_oihw, np.float32)
        C = w.shape[0]
        if w.shape != (C, C, 3, 3) or C not in (64, 128):
            raise NotImplementedError("pack_unscaled_s2: a (C, C, 3, 3) weight with C 64 or 128, got %r" % (w.shape,))
        ones = np.ones(C, np.float32)
        return self.A.upload(self.L.pack_conv3x3_ex(w, 2, C, fold_scale=ones, dtype=self.dt)), self.A.upload(np.zeros(C, np.float32)), self.A.upload(ones)

    def conv_unscaled_s2(self, x, packed, C, tag=0):
        """z = conv3x3 stride (1,2) of x (B, H, W, C), W even -> (B, H, W / 2, C) rounded to the activation type; packed = pack_unscaled_s2(W)"""
        A = self.A
        B, H, W, cx = _check16(x, "x")
        if W % 2 or cx != C:
            raise NotImplementedError("conv_unscaled_s2: x %r -- an even width and %d channels" % (tuple(x.shape), C))
        out = self.buf(("z", tag), B * H * (W // 2) * C * 2)
        self.L.call("rd_conv3x3_bn_act_ex", rdlib.ptr(x), C, 0, A.ptr(packed[0]), None, A.ptr(packed[1]), None, 0, 0, None, 0, 0, 0, None,
                    A.ptr(out), C, 0, B, H, W, C, C, 2, rdlib.RD_SCALE_FOLDED, self.dt, _stream(A))
        return _view16(A, out, (B, H, W // 2, C), self.dt)

    def pack_data_grad_s2(self, w_oihw):
        """the images of the strided conv's data gradient: it is the transposed conv with kernel (3,4), stride (1,2), pad (1,1) whose weight
        is W (cout, cin, 3, 3) read as (Cin, Cout, KH, KW) with a zero column at kx = 3 -- no flip, no axis swap; both convs map
        w = 2 wo - 1 + kx.  -> (the two phase images one after the other, zero shift, cin, bytes of a phase)"""
        w = np.asarray(w_oihw, np.float32)
        cout, cin = w.shape[:2]
        wd = np.zeros((cout, cin, 3, 4), np.float32)
        wd[..., :3] = w
        if not self.L.raw("rd_deconv2d_all_phases_ok")(3, 4, 2, 1, cin, self.dt):
            raise NotImplementedError("pack_data_grad_s2: %d input channels -- the all-phases transposed conv launch does not take them" % cin)
        ph = [self.L.pack_deconv_weight(wd, 2, 1, p, self.dt) for p in (0, 1)]
        return self.A.upload(np.concatenate(ph)), self.A.upload(np.zeros(cin, np.float32)), cin, int(ph[0].nbytes)

    def data_grad_s2(self, dz, packed, residual=None, tag=0):
        """dz (B, H, Wo, cout) -> the input gradient (B, H, 2 Wo, cin) of the strided conv; packed = pack_data_grad_s2(W).  residual
        (B, H, 2 Wo, cin): added in the launch's epilogue, one float32 add and one rounding, as data_grad_add does"""
        A = self.A
        img, zero_shift, cin, phase_bytes = packed
        B, H, Wo, cout = _check16(dz, "dz")
        if residual is not None and _check16(residual, "residual") != (B, H, 2 * Wo, cin):
            raise ValueError("data_grad_s2: residual %r, the input gradient is %r" % (tuple(residual.shape), (B, H, 2 * Wo, cin)))
        out = self.buf(("dx", tag), B * H * 2 * Wo * cin * 2)
        flags = rdlib.RD_SCALE_FOLDED | (rdlib.RD_ADD if residual is not None else 0)
        self.L.call("rd_deconv2d_bn_act_all", rdlib.ptr(dz), cout, 0, A.ptr(img), phase_bytes, A.ptr(zero_shift),
                    None if residual is None else rdlib.ptr(residual), cin, 0, A.ptr(out), cin, 0, B, H, Wo, cout, cin, 3, 4, 2, 1, flags, self.dt,
                    _stream(A))
        return _view16(A, out, (B, H, 2 * Wo, cin), self.dt)

    def data_grad_add(self, dz, packed, residual, tag=0):
        """data_grad with `residual` (B, H, W, cin) added in the launch's epilogue: one float32 add, one rounding (RD_ADD, no ReLU)"""
        A = self.A
        img, zero_shift, cin = packed
        B, H, W, cout = _check16(dz, "dz")
        if _check16(residual, "residual") != (B, H, W, cin):
            raise ValueError("data_grad_add: residual %r, the input gradient is %r" % (tuple(residual.shape), (B, H, W, cin)))
        out = self.buf(("dx", tag), B * H * W * cin * 2)
        self.L.call("rd_conv3x3_bn_act_ex", rdlib.ptr(dz), cout, 0, A.ptr(img), None, A.ptr(zero_shift), rdlib.ptr(residual), cin, 0, None, 0, 0, 0,
                    None, A.ptr(out), cin, 0, B, H, W, cout, cin, 1, rdlib.RD_SCALE_FOLDED | rdlib.RD_ADD, self.dt, _stream(A))
        return _view16(A, out, (B, H, W, cin), self.dt)


    # ---- the transposed conv and the join of an aggregation stage (rangedet_amd.backbone_train.AggStageTrain) --------------------------------
    def _deconv_form(self, w_shape, stride, pad, what):
        """the checks of the two transposed-conv forms -> (cin, cout, kw, s, p)"""
        if len(w_shape) != 4 or w_shape[2] != 3:
            raise NotImplementedError("%s: a (Cin, Cout, 3, KW) transposed-conv weight, got %r" % (what, tuple(w_shape)))
        cin, cout, _, kw = (int(v) for v in w_shape)
        s, p = int(stride), int(pad)
        if (kw, s, p) not in ((4, 2, 1), (8, 4, 2)):
            raise NotImplementedError("%s: kernel (3,%d), stride (1,%d), pad (1,%d) -- the network's forms are (3,4) / 2 / 1 and (3,8) / 4 / 2"
                                      % (what, kw, s, p))
        if (cin, cout) not in (((128, 128), (128, 64)) if kw == 8 else ((128, 64), (64, 64))):
            raise NotImplementedError("%s: %d -> %d channels with kernel (3,%d) -- (3,8): 128 -> 128 or 128 -> 64; (3,4): 128 -> 64 or 64 -> 64"
                                      % (what, cin, cout, kw))
        return cin, cout, kw, s, p

    def pack_deconv_unscaled(self, w_iohw, stride, pad):
        """the forward images of a transposed conv with the (Cin, Cout, 3, KW) weight: its `stride` phase images one after the other, no
        scale -> (images, zero shift, bytes of a phase, (cin, cout, kw, s, p))"""
        w = np.ascontiguousarray(w_iohw, dtype=np.float32)
        form = cin, cout, kw, s, p = self._deconv_form(w.shape, stride, pad, "pack_deconv_unscaled")
        ph = [self.L.pack_deconv_weight(w, s, p, q, self.dt) for q in range(s)]
        return self.A.upload(np.concatenate(ph)), self.A.upload(np.zeros(cout, np.float32)), int(ph[0].nbytes), form

    def deconv_unscaled(self, x, packed, tag=0):
        """z = the transposed conv of x (B, H, Win, cin) -> (B, H, s Win, cout) rounded to the activation type: rd_deconv2d_bn_act_all on the
        unscaled phase images, zero shift, no activation; packed = pack_deconv_unscaled(W, stride, pad)"""
        A = self.A
        img, zero_shift, phase_bytes, (cin, cout, kw, s, p) = packed
        B, H, Win, cx = _check16(x, "x")
        if cx != cin:
            raise ValueError("deconv_unscaled: x %r, the transposed conv takes %d channels" % (tuple(x.shape), cin))
        out = self.buf(("dcz", tag), B * H * s * Win * cout * 2)
        self.L.call("rd_deconv2d_bn_act_all", rdlib.ptr(x), cin, 0, A.ptr(img), phase_bytes, A.ptr(zero_shift), None, 0, 0, A.ptr(out), cout, 0,
                    B, H, Win, cin, cout, 3, kw, s, p, rdlib.RD_SCALE_FOLDED, self.dt, _stream(A))
        return _view16(A, out, (B, H, s * Win, cout), self.dt)

    def deconv_weight_grad(self, x, dz, kernel_w, stride, pad, tag=0, split=0):
        """x (B, H, Win, cin), dz (B, H, s Win, cout) -> dW (cin, cout, 3, KW) float32, MXNet's Deconvolution layout (rd_deconv_bwd_weight)"""
        A, L = self.A, self.L
        B, H, Win, cin = _check16(x, "x")
        cout = _check16(dz, "dz")[3]
        _, _, kw, s, p = self._deconv_form((cin, cout, 3, kernel_w), stride, pad, "deconv_weight_grad")
        if tuple(dz.shape[:3]) != (B, H, s * Win):
            raise ValueError("deconv_weight_grad: x %r and dz %r -- dz is (B, H, %d Win, cout)" % (tuple(x.shape), tuple(dz.shape), s))
        nws = L.raw("rd_deconv_bwd_weight_workspace_bytes")(B, H, Win, cin, cout, kw, s, p, split)
        ws, out = self.buf(("bww_ws", 0), nws), self.buf(("dWd", tag), cin * cout * 3 * kw * 4)
        L.call("rd_deconv_bwd_weight", rdlib.ptr(x), cin, 0, rdlib.ptr(dz), cout, 0, A.ptr(out), B, H, Win, cin, cout, kw, s, p, split, self.dt,
               A.ptr(ws), nws, _stream(A))
        return A.view_f32(out, (cin, cout, 3, kw))

    def pack_deconv_data_grad(self, w_iohw, stride, pad):
        """the image of the transposed conv's data gradient (rd_pack_deconv_data_grad_host): a 3x3 stride-1 conv from the s cout channels of
        dz read as (B, H, Win, s cout) to cin -> (image, zero shift, (cin, cout, kw, s, p))"""
        w = np.ascontiguousarray(w_iohw, dtype=np.float32)
        form = self._deconv_form(w.shape, stride, pad, "pack_deconv_data_grad")
        return self.A.upload(self.L.pack_deconv_data_grad(w, form[3], form[4], self.dt)), self.A.upload(np.zeros(form[0], np.float32)), form

    def deconv_data_grad(self, dz, image, residual=None, tag=0):
        """dz (B, H, s Win, cout) -> the gradient (B, H, Win, cin) of the transposed conv's input; image = pack_deconv_data_grad(W, stride,
        pad).  One persistent 3x3 launch on the s-pixel view of dz.  residual (B, H, Win, cin): another gradient of the same tensor, added
        in the launch's epilogue -- one float32 add, one rounding, as data_grad_add does"""
        A = self.A
        img, zero_shift, (cin, cout, kw, s, p) = image
        B, H, Wout, cz = _check16(dz, "dz")
        if cz != cout or Wout % s:
            raise ValueError("deconv_data_grad: dz %r -- (B, H, %d Win, %d)" % (tuple(dz.shape), s, cout))
        Win = Wout // s
        if residual is not None and _check16(residual, "residual") != (B, H, Win, cin):
            raise ValueError("deconv_data_grad: residual %r, the input gradient is %r" % (tuple(residual.shape), (B, H, Win, cin)))
        out = self.buf(("dcx", tag), B * H * Win * cin * 2)
        flags = rdlib.RD_SCALE_FOLDED | (rdlib.RD_ADD if residual is not None else 0)
        self.L.call("rd_conv3x3_bn_act_ex", rdlib.ptr(dz), s * cout, 0, A.ptr(img), None, A.ptr(zero_shift),
                    None if residual is None else rdlib.ptr(residual), cin, 0, None, 0, 0, 0, None, A.ptr(out), cin, 0, B, H, Win, s * cout, cin, 1,
                    flags, self.dt, _stream(A))
        return _view16(A, out, (B, H, Win, cin), self.dt)

    def affine_relu_add(self, z, a, b, r, tag=0):
        """y = relu(fmaf(z, a, b)) + r, the join of an aggregation stage (rd_affine_relu_add); z, r (B, H, W, C)"""
        A = self.A
        B, H, W, C = _check16(z, "z")
        if _check16(r, "r") != (B, H, W, C):
            raise ValueError("affine_relu_add: z %r and r %r differ" % (tuple(z.shape), tuple(r.shape)))
        out = self.buf(("bn_relu_add_y", tag), B * H * W * C * 2)
        self.L.call("rd_affine_relu_add", rdlib.ptr(z), C, 0, A.ptr(a), A.ptr(b), rdlib.ptr(r), C, 0, A.ptr(out), C, 0, B, H, W, C, self.dt,
                    _stream(A))
        return _view16(A, out, (B, H, W, C), self.dt)

    # ---- the Meta-Kernel unit (csrc/k_metabwd.h; MetaUnitBackward below) -----------------------------------------------------------------------
    def _meta_check(self, dz, data, coord, what):
        B, H, W, C = _check16(data, "data")
        if C != 64 or _check16(dz, "dz") != (B, H, W, 64):
            raise ValueError("%s: data %r and dz %r -- both (B, H, W, 64)" % (what, tuple(data.shape), tuple(dz.shape)))
        if tuple(coord.shape) != (B, 3, H, W) or (coord.itemsize if isinstance(coord, np.ndarray) else coord.element_size()) != 4:
            raise ValueError("%s: coord %r -- a float32 (B, 3, H, W) tensor" % (what, tuple(coord.shape)))
        return B, H, W

    def meta_data_grad(self, dz, data, coord, packed_bwd, residual=None, tag=0):
        """dz, data (B, H, W, 64), coord (B, 3, H, W) float32, packed_bwd the uploaded block of Lib.pack_meta_bwd -> ddata (B, H, W, 64);
        residual (B, H, W, 64): added in float32 before the one rounding"""
        A = self.A
        B, H, W = self._meta_check(dz, data, coord, "meta_data_grad")
        if residual is not None and _check16(residual, "residual") != (B, H, W, 64):
            raise ValueError("meta_data_grad: residual %r, the input gradient is %r" % (tuple(residual.shape), (B, H, W, 64)))
        out = self.buf(("meta_ddata", tag), B * H * W * 128)
        self.L.call("rd_meta_kernel_bwd_data", rdlib.ptr(dz), 64, 0, rdlib.ptr(data), 64, 0, rdlib.ptr(coord), A.ptr(packed_bwd),
                    None if residual is None else rdlib.ptr(residual), 64, 0, A.ptr(out), 64, 0, B, H, W, self.dt, _stream(A))
        return _view16(A, out, (B, H, W, 64), self.dt)

    def meta_param_grads(self, dz, data, coord, packed_bwd, split=0, tag=0):
        """-> float32 device views dA (64, 576), dW1 (64, 32), db1 (64,), dW0 (32, 3), db0 (32,), dt1 (576,), dq1 (576,), by name"""
        A, L = self.A, self.L
        B, H, W = self._meta_check(dz, data, coord, "meta_param_grads")
        nws = L.raw("rd_meta_kernel_bwd_workspace_bytes")(B, H, W, split)
        ws = self.buf(("meta_ws", 0), nws)
        shapes = (("dA", (64, 576)), ("dW1", (64, 32)), ("db1", (64,)), ("dW0", (32, 3)), ("db0", (32,)), ("dt1", (576,)), ("dq1", (576,)))
        bufs = [self.buf(("meta_" + k, tag), int(np.prod(shp)) * 4) for k, shp in shapes]
        L.call("rd_meta_kernel_bwd_params", rdlib.ptr(dz), 64, 0, rdlib.ptr(data), 64, 0, rdlib.ptr(coord), A.ptr(packed_bwd),
               *[A.ptr(b) for b in bufs], B, H, W, split, self.dt, A.ptr(ws), nws, _stream(A))
        return {k: A.view_f32(b, shp) for (k, shp), b in zip(shapes, bufs)}

    def meta_forward(self, data, coord, packed_fwd, tag=0):
        """y = rd_meta_kernel_fwd(data, coord) (B, H, W, 64); packed_fwd the uploaded block of Lib.pack_meta"""
        A = self.A
        B, H, W, C = _check16(data, "data")
        if C != 64 or tuple(coord.shape) != (B, 3, H, W):
            raise ValueError("meta_forward: data %r, coord %r -- (B, H, W, 64) and (B, 3, H, W)" % (tuple(data.shape), tuple(coord.shape)))
        out = self.buf(("meta_y", tag), B * H * W * 128)
        self.L.call("rd_meta_kernel_fwd", rdlib.ptr(data), 64, 0, rdlib.ptr(coord), A.ptr(packed_fwd), A.ptr(out), 64, 0, B, H, W, self.dt, _stream(A))
        return _view16(A, out, (B, H, W, 64), self.dt)

    # ---- the Meta-Kernel unit in training mode (csrc/k_metatrain.h; MetaUnitTrain below).  Tables: float32 device buffers of 576, c 9 + k ----
    def _meta_train_ws(self, entry, B, H, W, split):
        nws = self.L.raw(entry)(B, H, W, split)
        return self.buf(("meta_train_ws", 0), nws), nws

    def meta_stats(self, data, coord, packed_bwd, split=0, tag=0):
        """-> the buffers mean1, var1 (576, biased) of q = data[n_k] * w_k over all pixels"""
        A = self.A
        B, H, W = self._meta_check(data, data, coord, "meta_stats")
        ws, nws = self._meta_train_ws("rd_meta_kernel_stats_workspace_bytes", B, H, W, split)
        mean, var = self.buf(("meta_mean1", tag), 576 * 4), self.buf(("meta_var1", tag), 576 * 4)
        self.L.call("rd_meta_kernel_stats", rdlib.ptr(data), 64, 0, rdlib.ptr(coord), A.ptr(packed_bwd), A.ptr(mean), A.ptr(var), B, H, W, split,
                    self.dt, A.ptr(ws), nws, _stream(A))
        return mean, var

    def meta_forward_train(self, data, coord, packed_fwd, packed_bwd, a1, bb1, tag=0):
        """-> z (B, H, W, 64): the aggregation conv's output, before its BatchNorm"""
        A = self.A
        B, H, W = self._meta_check(data, data, coord, "meta_forward_train")
        out = self.buf(("meta_z", tag), B * H * W * 128)
        self.L.call("rd_meta_kernel_fwd_train", rdlib.ptr(data), 64, 0, rdlib.ptr(coord), A.ptr(packed_fwd), A.ptr(packed_bwd), A.ptr(a1), A.ptr(bb1),
                    A.ptr(out), 64, 0, B, H, W, self.dt, _stream(A))
        return _view16(A, out, (B, H, W, 64), self.dt)

    def meta_bwd_sums(self, dz, data, coord, packed_bwd, tabs, split=0, tag=0):
        """pass A.  tabs: the dict of buffers a1, bb1, mean1, rstd1 -> float32 device views dA (64, 576), dbeta1, dgamma1, c1, c2 (576,)"""
        A = self.A
        B, H, W = self._meta_check(dz, data, coord, "meta_bwd_sums")
        ws, nws = self._meta_train_ws("rd_meta_kernel_bwd_train_workspace_bytes", B, H, W, split)
        shapes = (("dA", (64, 576)), ("dbeta1", (576,)), ("dgamma1", (576,)), ("c1", (576,)), ("c2", (576,)))
        bufs = [self.buf(("meta_t_" + k, tag), int(np.prod(shp)) * 4) for k, shp in shapes]
        self.L.call("rd_meta_kernel_bwd_sums", rdlib.ptr(dz), 64, 0, rdlib.ptr(data), 64, 0, rdlib.ptr(coord), A.ptr(packed_bwd),
                    *[A.ptr(tabs[k]) for k in ("a1", "bb1", "mean1", "rstd1")], *[A.ptr(b) for b in bufs], B, H, W, split, self.dt, A.ptr(ws), nws,
                    _stream(A))
        return {k: A.view_f32(b, shp) for (k, shp), b in zip(shapes, bufs)}

    def meta_bwd_params_train(self, dz, data, coord, packed_bwd, tabs, split=0, tag=0):
        """pass B.  tabs: a1, bb1, mean1, rstd1, c1, c2 -> float32 device views dW1 (64, 32), db1 (64,), dW0 (32, 3), db0 (32,)"""
        A = self.A
        B, H, W = self._meta_check(dz, data, coord, "meta_bwd_params_train")
        ws, nws = self._meta_train_ws("rd_meta_kernel_bwd_train_workspace_bytes", B, H, W, split)
        shapes = (("dW1", (64, 32)), ("db1", (64,)), ("dW0", (32, 3)), ("db0", (32,)))
        bufs = [self.buf(("meta_t_" + k, tag), int(np.prod(shp)) * 4) for k, shp in shapes]
        self.L.call("rd_meta_kernel_bwd_params_train", rdlib.ptr(dz), 64, 0, rdlib.ptr(data), 64, 0, rdlib.ptr(coord), A.ptr(packed_bwd),
                    *[rdlib.ptr(tabs[k]) for k in ("a1", "bb1", "mean1", "rstd1", "c1", "c2")], *[A.ptr(b) for b in bufs], B, H, W, split, self.dt,
                    A.ptr(ws), nws, _stream(A))
        return {k: A.view_f32(b, shp) for (k, shp), b in zip(shapes, bufs)}

    def meta_bwd_data_train(self, dz, data, coord, packed_bwd, tabs, residual=None, tag=0):
        """ddata (B, H, W, 64), rounded once; residual is added in float32 before that rounding"""
        A = self.A
        B, H, W = self._meta_check(dz, data, coord, "meta_bwd_data_train")
        if residual is not None and _check16(residual, "residual") != (B, H, W, 64):
            raise ValueError("meta_bwd_data_train: residual %r, the input gradient is %r" % (tuple(residual.shape), (B, H, W, 64)))
        out = self.buf(("meta_t_ddata", tag), B * H * W * 128)
        self.L.call("rd_meta_kernel_bwd_data_train", rdlib.ptr(dz), 64, 0, rdlib.ptr(data), 64, 0, rdlib.ptr(coord), A.ptr(packed_bwd),
                    *[rdlib.ptr(tabs[k]) for k in ("a1", "bb1", "mean1", "rstd1", "c1", "c2")], None if residual is None else rdlib.ptr(residual),
                    64, 0, A.ptr(out), 64, 0, B, H, W, self.dt, _stream(A))
        return _view16(A, out, (B, H, W, 64), self.dt)

    def pack_meta_dev(self, masters, packed_fwd, packed_bwd):
        """both blocks of the unit from the float32 device masters w0, b0, w1, b1, agg (a dict), with s1 = s2 = 1 and t1 = t2 = 0"""
        A = self.A
        self.L.call("rd_pack_meta_dev", *[rdlib.ptr(masters[k]) for k in ("w0", "b0", "w1", "b1", "agg")], A.ptr(packed_fwd), A.ptr(packed_bwd),
                    self.dt, _stream(A))


BN_EPS = 1e-5 + 1e-10      # mxnext/complicate.py:26-45 (normalizer_factory(type="localbn"))
BN_MOMENTUM = 0.9

_OPS = {}


def _ops(dtype, lib, alloc):
    if lib is not None or alloc is not None:
        return TowerOps(dtype, lib, alloc)
    if dtype not in _OPS:
        _OPS[dtype] = TowerOps(dtype)
    return _OPS[dtype]


def conv3x3_data_grad(dz, w_oihw, dtype=rdlib.RD_BF16, lib=None, alloc=None):
    """dL/dx of a stride-1, pad-1 3x3 conv: dz (B, H, W, cout) device tensor of the activation type, w the (cout, cin, 3, 3) float32 weight
    on the host (packed on every call: keep a HeadTowerBackward, or TowerOps.pack_data_grad, for repeated use)"""
    o = _ops(dtype, lib, alloc)
    return o.data_grad(dz, o.pack_data_grad(w_oihw))


def conv3x3_weight_grad(x, dz, dtype=rdlib.RD_BF16, split=0, lib=None, alloc=None):
    """dL/dW (cout, cin, 3, 3) float32 of the same conv from its input x and dz; deterministic"""
    return _ops(dtype, lib, alloc).weight_grad(x, dz, split=split)


def head_out_backward(d_out, x, w, n_off=0, out_batch_stride=None, scale=None, relu_mask=False, dtype=rdlib.RD_BF16, lib=None, alloc=None):
    """backward of rd_head_out: (dx, dw, dbias); w (nout, cin) and scale (cin) float32 on the host"""
    o = _ops(dtype, lib, alloc)
    w = np.ascontiguousarray(np.asarray(w, np.float32).reshape(len(w), -1))
    sc = None if scale is None else o.A.upload(np.ascontiguousarray(scale, dtype=np.float32))
    return o.head_out_bwd(d_out, x, o.A.upload(w), w.shape[0], n_off, out_batch_stride, sc, relu_mask)


def _vec(o, v, C, what):
    v = np.ascontiguousarray(v, dtype=np.float32)
    if v.shape != (C,):
        raise ValueError("%s: %d float32 values, got shape %r" % (what, C, v.shape))
    return o.A.upload(v)


def batch_norm_stats(z, split=0, dtype=rdlib.RD_BF16, lib=None, alloc=None):
    """(mean, var) of a (B, H, W, C) device tensor of the activation type over B, H, W: float32 device vectors, the variance biased"""
    o = _ops(dtype, lib, alloc)
    C = int(z.shape[3])
    mean, var = o.bn_stats(z, split)
    return o.A.view_f32(mean, (C,)), o.A.view_f32(var, (C,))


def batch_norm_relu_forward(z, gamma, beta, moving_mean, moving_var, eps=BN_EPS, momentum=BN_MOMENTUM, unbiased=True, relu=True, split=0,
                            dtype=rdlib.RD_BF16, lib=None, alloc=None):
    """y = relu(gamma (z - mean) / sqrt(var + eps) + beta) with the batch's own statistics (mx.sym.BatchNorm, use_global_stats=False) ->
    (y, saved).  gamma, beta and the moving statistics are float32 host vectors; saved holds the device buffers a, b, mean, var, rstd that
    batch_norm_relu_backward needs, and float32 device views 'moving_mean' / 'moving_var' of the updated moving statistics
    (moving = moving * momentum + batch * (1 - momentum)).
    unbiased=True feeds the moving variance var * n / (n - 1).  That is what the GPU batch-norm implementations the reference runs on do
    (cuDNN's running variance, and MXNet's own CUDA kernel, use the unbiased estimate; its CPU operator uses the biased one) -- read from
    their sources, not pinned by a run of the reference.  The normalisation itself always uses the biased variance."""
    o = _ops(dtype, lib, alloc)
    B, H, W, C = _check16(z, "z")
    gd, bd, mm, mv = (_vec(o, v, C, k) for v, k in ((gamma, "gamma"), (beta, "beta"), (moving_mean, "moving_mean"), (moving_var, "moving_var")))
    mean, var = o.bn_stats(z, split)
    rstd, a, b = o.bn_fold(mean, var, gd, bd, mm, mv, B * H * W, C, eps, momentum, unbiased)
    saved = dict(a=a, b=b, mean=mean, var=var, rstd=rstd, relu=relu, moving_mean=o.A.view_f32(mm, (C,)), moving_var=o.A.view_f32(mv, (C,)))
    return o.affine_relu(z, a, b, relu), saved


def batch_norm_relu_backward(g, z, saved, gamma, split=0, dtype=rdlib.RD_BF16, lib=None, alloc=None):
    """g = dL/dy, z and saved as batch_norm_relu_forward had them, gamma a float32 host vector -> (dz, dgamma, dbeta)"""
    o = _ops(dtype, lib, alloc)
    return o.bn_relu_bwd(g, z, saved, _vec(o, gamma, int(z.shape[3]), "gamma"), saved.get("relu", True), split)


_META_KEYS = ("w0", "b0", "w1", "b1", "s1", "t1", "agg", "s2", "t2")


def _meta_packed_bwd(o, prm):
    """prm: the nine arrays of Lib.pack_meta by name (w0 (32, 3), b0, w1 (64, 32), b1, s1, t1 (576), agg (64, 576), s2, t2)"""
    return o.A.upload(o.L.pack_meta_bwd(*[prm[k] for k in _META_KEYS], o.dt))


def meta_kernel_data_grad(dz, data, coord, prm, residual=None, dtype=rdlib.RD_BF16, lib=None, alloc=None):
    """dL/ddata of the Meta-Kernel unit up to z (rd_meta_kernel_bwd_data): dz, data (B, H, W, 64) device tensors of the activation type, coord
    (B, 3, H, W) float32 on the device, prm the folded parameters on the host (packed on every call: keep a MetaUnitBackward for repeated
    use); residual is added in float32 before the one rounding"""
    o = _ops(dtype, lib, alloc)
    return o.meta_data_grad(dz, data, coord, _meta_packed_bwd(o, prm), residual)


def meta_kernel_param_grads(dz, data, coord, prm, split=0, dtype=rdlib.RD_BF16, lib=None, alloc=None):
    """{dA, dW1, db1, dW0, db0, dt1, dq1}: the float32 parameter gradients of the Meta-Kernel unit up to z (rd_meta_kernel_bwd_params);
    deterministic"""
    o = _ops(dtype, lib, alloc)
    return o.meta_param_grads(dz, data, coord, _meta_packed_bwd(o, prm), split)


class MetaUnitBackward:
    """The Meta-Kernel unit (res1_unit2: meta_kernel.py:166-240 + dla_backbone.py:92-97) with inference-mode normalisation, forward and
    backward, built from the reference's parameter dict:
      <name>_<W>_mlp0_weight | bias, <name>_<W>_mlp1_weight | bias      the 3 -> 32 -> 64 MLP (1x1 convs)
      <name>point_wise_mlp_bn1_*                                        the 576-channel BatchNorm, folded to s1, t1 with its moving statistics
      <name>aggregation_conv1_weight, <name>aggregation_bn1_*           the 576 -> 64 conv and its BatchNorm, folded to s2, t2
    forward(data, coord) -> y (B, H, W, 64) through rd_meta_kernel_fwd (data a (B, H, W, 64) device tensor of the activation type, coord
    (B, 3, H, W) float32).  backward(g, residual=None) -> (ddata, grads): dz = rd_relu_affine_bwd(g, y, s2), then the two fused launches of
    csrc/k_metabwd.h; residual (the identity shortcut's gradient) is added to ddata in float32 before its one rounding.  grads: float32
    device tensors under the reference's names and shapes for the two MLP convs and the aggregation conv, and -- under the frozen
    statistics -- point_wise_mlp_bn1_beta = dt1, point_wise_mlp_bn1_gamma = dq1 / gamma.  The gradients of aggregation_bn1's gamma and beta
    need z, which the fused forward never writes: they come with the training-mode form, MetaUnitTrain below, which also carries the
    batch-statistics form of the 576-channel BatchNorm, the device re-pack and optimizer_entries()."""

    def __init__(self, name, params, W, dtype=rdlib.RD_BF16, lib=None, alloc=None, eps=BN_EPS):
        from .runtime import bn_affine
        self.ops = o = TowerOps(dtype, lib, alloc)
        self.name, self.W = name, int(W)
        pre = "%s_%d" % (name, self.W)
        f = lambda k, shape: np.ascontiguousarray(params[k], dtype=np.float32).reshape(shape)
        s1, t1 = bn_affine(params, name + "point_wise_mlp_bn1", eps)
        s2, t2 = bn_affine(params, name + "aggregation_bn1", eps)
        self.prm = dict(w0=f(pre + "_mlp0_weight", (32, 3)), b0=f(pre + "_mlp0_bias", (32,)), w1=f(pre + "_mlp1_weight", (64, 32)),
                        b1=f(pre + "_mlp1_bias", (64,)), s1=s1, t1=t1, agg=f(name + "aggregation_conv1_weight", (64, 576)), s2=s2, t2=t2)
        gamma = f(name + "point_wise_mlp_bn1_gamma", (576,))
        if (gamma == 0).any():
            raise ValueError("%spoint_wise_mlp_bn1_gamma has a zero: its gradient dq1 / gamma does not exist" % name)
        self.names = dict(dW0=(pre + "_mlp0_weight", (32, 3, 1, 1)), db0=(pre + "_mlp0_bias", (32,)), dW1=(pre + "_mlp1_weight", (64, 32, 1, 1)),
                          db1=(pre + "_mlp1_bias", (64,)), dA=(name + "aggregation_conv1_weight", (64, 576, 1, 1)),
                          dt1=(name + "point_wise_mlp_bn1_beta", (576,)), dq1=(name + "point_wise_mlp_bn1_gamma", (576,)))
        self.packed_fwd = o.A.upload(o.L.pack_meta(*[self.prm[k] for k in _META_KEYS], dtype))
        self.packed_bwd = _meta_packed_bwd(o, self.prm)
        self.s2 = o.A.upload(np.ascontiguousarray(s2, dtype=np.float32))
        self.gamma = o.A.view_f32(o.A.upload(gamma), (576,))
        self.saved = None

    def forward(self, data, coord):
        self.saved = (data, coord, self.ops.meta_forward(data, coord, self.packed_fwd))
        return self.saved[2]

    def backward(self, g, residual=None, split=0):
        if self.saved is None:
            raise RuntimeError("backward before forward: the input and the output are kept by forward(data, coord)")
        o = self.ops
        data, coord, y = self.saved
        self.dz = dz = o.relu_affine_bwd(g, y, self.s2, tag="meta")
        raw = o.meta_param_grads(dz, data, coord, self.packed_bwd, split)
        grads = {}
        for k, (pname, shape) in self.names.items():
            v = raw[k]
            if k == "dq1":
                v = v / self.gamma                 # d r / d gamma = (r - t1) / gamma under the frozen statistics
            grads[pname] = v.reshape(shape)
        return o.meta_data_grad(dz, data, coord, self.packed_bwd, residual), grads


class MetaUnitTrain:
    """The Meta-Kernel unit as the reference trains it: both BatchNorms (the 576-channel point_wise_mlp_bn1 and the 64-channel
    aggregation_bn1) normalise with the batch's own statistics.  Built from the same parameter dict and names as MetaUnitBackward, plus the
    four moving statistics.  Every parameter lives on the device as a float32 master; the two packed blocks are made from the masters with
    s1 = s2 = 1, t1 = t2 = 0 by rd_pack_meta_dev, here and after every optimizer step (optimizer_entries()).
      forward(data, coord, unbiased=True) -> y (B, H, W, 64): rd_meta_kernel_stats, rd_bn_fold (C = 576), rd_meta_kernel_fwd_train, then
          rd_bn_stats, rd_bn_fold, rd_affine_relu on z.  unbiased as in batch_norm_relu_forward (n = 1 needs unbiased=False).
      backward(g, residual=None, split=0) -> (ddata, grads): rd_bn_relu_bwd gives dz and aggregation_bn1's gradients, then pass A
          (rd_meta_kernel_bwd_sums: dA, point_wise_mlp_bn1's true batch-statistics gradients, c1, c2), pass B
          (rd_meta_kernel_bwd_params_train) and rd_meta_kernel_bwd_data_train; residual is added to ddata in float32 before its one rounding.
          grads: float32 device tensors under the reference's eleven names and shapes.
      aux() -> the four moving statistics by name.  Nothing synchronises with the host."""

    def __init__(self, name, params, W, eps=BN_EPS, momentum=BN_MOMENTUM, dtype=rdlib.RD_BF16, lib=None, alloc=None):
        self.ops = o = TowerOps(dtype, lib, alloc)
        A = o.A
        self.name, self.W, self.eps, self.momentum = name, int(W), float(eps), float(momentum)
        pre = "%s_%d" % (name, self.W)
        f = lambda k, shape: np.ascontiguousarray(params[k], dtype=np.float32).reshape(shape)
        up = lambda k, shape: A.view_f32(A.upload(f(k, shape)), shape)
        bn1, bn2 = name + "point_wise_mlp_bn1", name + "aggregation_bn1"
        self.masters = dict(w0=up(pre + "_mlp0_weight", (32, 3)), b0=up(pre + "_mlp0_bias", (32,)), w1=up(pre + "_mlp1_weight", (64, 32)),
                            b1=up(pre + "_mlp1_bias", (64,)), agg=up(name + "aggregation_conv1_weight", (64, 576)))
        self.norm = {k: up(k, (C,)) for bn, C in ((bn1, 576), (bn2, 64)) for k in (bn + "_gamma", bn + "_beta", bn + "_moving_mean", bn + "_moving_var")}
        self.bn1, self.bn2 = bn1, bn2
        # reference name -> (shape, the master, the TowerOps buffer key backward() writes the gradient to, the gradient's name in backward())
        self.table = {pre + "_mlp0_weight": ((32, 3, 1, 1), self.masters["w0"], ("meta_t_dW0", 0), "dW0"),
                      pre + "_mlp0_bias": ((32,), self.masters["b0"], ("meta_t_db0", 0), "db0"),
                      pre + "_mlp1_weight": ((64, 32, 1, 1), self.masters["w1"], ("meta_t_dW1", 0), "dW1"),
                      pre + "_mlp1_bias": ((64,), self.masters["b1"], ("meta_t_db1", 0), "db1"),
                      name + "aggregation_conv1_weight": ((64, 576, 1, 1), self.masters["agg"], ("meta_t_dA", 0), "dA"),
                      bn1 + "_gamma": ((576,), self.norm[bn1 + "_gamma"], ("meta_t_dgamma1", 0), "dgamma1"),
                      bn1 + "_beta": ((576,), self.norm[bn1 + "_beta"], ("meta_t_dbeta1", 0), "dbeta1"),
                      bn2 + "_gamma": ((64,), self.norm[bn2 + "_gamma"], ("bn_dgamma", "meta2"), "dgamma2"),
                      bn2 + "_beta": ((64,), self.norm[bn2 + "_beta"], ("bn_dbeta", "meta2"), "dbeta2")}
        self.packed_fwd = A.alloc(o.L.raw("rd_meta_packed_bytes")(dtype))
        self.packed_bwd = A.alloc(o.L.raw("rd_meta_bwd_packed_bytes")(dtype))
        o.pack_meta_dev(self.masters, self.packed_fwd, self.packed_bwd)
        self.saved = None

    def aux(self):
        return {bn + k: self.norm[bn + k] for bn in (self.bn1, self.bn2) for k in ("_moving_mean", "_moving_var")}

    def optimizer_entries(self):
        """SGD.add's arguments per trainable parameter; the aggregation weight's entry carries the unit's re-pack request"""
        o = self.ops
        for pname, (shape, master, key, _) in self.table.items():
            n = int(np.prod(shape))
            kw = dict(name=pname, weight=master.reshape(shape), grad=o.A.view_f32(o.buf(key, n * 4), shape))
            if pname.endswith("aggregation_conv1_weight"):
                kw["pack"] = dict(meta=self.masters, fwd=self.packed_fwd, bwd=self.packed_bwd, dtype=o.dt)
            yield kw

    def forward(self, data, coord, unbiased=True):
        o, nm = self.ops, self.norm
        B, H, W, _ = _check16(data, "data")
        n = B * H * W
        mean1, var1 = o.meta_stats(data, coord, self.packed_bwd)
        rstd1, a1, bb1 = o.bn_fold(mean1, var1, nm[self.bn1 + "_gamma"], nm[self.bn1 + "_beta"], nm[self.bn1 + "_moving_mean"],
                                   nm[self.bn1 + "_moving_var"], n, 576, self.eps, self.momentum, unbiased, tag="meta1")
        z = o.meta_forward_train(data, coord, self.packed_fwd, self.packed_bwd, a1, bb1)
        mean2, var2 = o.bn_stats(z, tag="meta2")
        rstd2, a2, b2 = o.bn_fold(mean2, var2, nm[self.bn2 + "_gamma"], nm[self.bn2 + "_beta"], nm[self.bn2 + "_moving_mean"],
                                  nm[self.bn2 + "_moving_var"], n, 64, self.eps, self.momentum, unbiased, tag="meta2")
        self.saved = dict(data=data, coord=coord, z=z, tabs=dict(a1=a1, bb1=bb1, mean1=mean1, var1=var1, rstd1=rstd1),
                          bn2=dict(a=a2, b=b2, mean=mean2, var=var2, rstd=rstd2))
        return o.affine_relu(z, a2, b2, tag="meta2")

    def backward(self, g, residual=None, split=0):
        if self.saved is None:
            raise RuntimeError("backward before forward: the input, z and the batch statistics are kept by forward(data, coord)")
        o, s = self.ops, self.saved
        data, coord, tabs = s["data"], s["coord"], dict(s["tabs"])
        self.dz, dg2, db2 = o.bn_relu_bwd(g, s["z"], s["bn2"], self.norm[self.bn2 + "_gamma"], split=split, tag="meta2")
        sums = o.meta_bwd_sums(self.dz, data, coord, self.packed_bwd, tabs, split)
        tabs.update(c1=sums["c1"], c2=sums["c2"])
        pg = o.meta_bwd_params_train(self.dz, data, coord, self.packed_bwd, tabs, split)
        raw = dict(pg, dA=sums["dA"], dgamma1=sums["dgamma1"], dbeta1=sums["dbeta1"], dgamma2=dg2, dbeta2=db2)
        grads = {pname: raw[rname].reshape(shape) for pname, (shape, _, _, rname) in self.table.items()}
        return o.meta_bwd_data_train(self.dz, data, coord, self.packed_bwd, tabs, residual), grads


class _HeadTower:
    """What the two towers share: the layer checks and the reference's parameter names, the output conv, and the forward and backward
    loops.  A subclass supplies _layer (one layer's device parameters), _layer_forward, _dz (dL/dy -> dz of a layer), _out_bwd_kwargs, and
    for optimizer_entries() _fwd_image (a layer's forward image and fold scale) and _norm_entries (its trainable normalisation parameters).
    `params`: one sequence per normalisation parameter, each with one entry per conv weight; `what` names them in the refusal."""

    def __init__(self, conv_weights, params, what, out_weight, out_bias, kind, level, first_conv, dtype, lib, alloc):
        if kind not in ("cls", "reg"):
            raise ValueError("kind: 'cls' or 'reg', got %r" % (kind,))
        self.ops = o = TowerOps(dtype, lib, alloc)
        if any(len(p) != len(conv_weights) for p in params) or not conv_weights:
            raise ValueError("one %s per conv weight, at least one layer" % what)
        self._stems, self.layers = [], []
        chans = None
        for i, w in enumerate(conv_weights):
            w = np.asarray(w, np.float32)
            name = "rpn_%s_conv_%d_lvl_%d" % (kind, first_conv + i, level)
            if w.ndim != 4 or w.shape[2:] != (3, 3):
                raise NotImplementedError("%s: kernel %r -- 3x3, stride 1, pad 1 only (no strided or transposed conv)" % (name, w.shape[2:]))
            cout, cin = self._layer_channels(i, w, name)
            if chans is not None and cin != chans:
                raise ValueError("%s: %d input channels after a layer with %d outputs" % (name, cin, chans))
            chans = cout
            self._stems.append(name)
            self.layers.append(dict(self._layer(w, name, *(p[i] for p in params)), cin=cin, cout=cout, **self._weight_images(i, w)))
        ow = np.asarray(out_weight, np.float32)
        ow = np.ascontiguousarray(ow.reshape(ow.shape[0], -1))
        ob = np.ascontiguousarray(out_bias, dtype=np.float32)
        self.nout = int(ow.shape[0])
        if ow.shape[1] != chans or ob.shape != (self.nout,):
            raise ValueError("output conv: weight (nout, %d) and bias (nout), got %r and %r" % (chans, ow.shape, ob.shape))
        if self.nout not in (1, 8):
            raise NotImplementedError("output conv with %d outputs: rpn_cls_logit has 1, rpn_reg_delta 8" % self.nout)
        out_name = "rpn_cls_logit_lvl_%d" % level if kind == "cls" else "rpn_reg_delta_lvl_%d" % level
        self.out_names = (out_name + "_weight", out_name + "_bias")
        self.out_w, self.out_b = o.A.upload(ow), o.A.upload(ob)
        self.acts = None

    def _layer_channels(self, i, w, name):
        """the channel check of layer i -> (cout, cin as the tower's input sees it)"""
        cout, cin = w.shape[:2]
        if cin not in (64, 128) or cout not in (64, 128):
            why = " (the level-0 conv_0 reads the un-materialised concat of 64 + 8 channels: the concat conv has no backward here)" \
                if cin == 72 else ""
            raise NotImplementedError("%s: %d -> %d channels; the backward kernels run 64 or 128 on either side%s" % (name, cin, cout, why))
        return cout, cin

    def _weight_images(self, i, w):
        """layer i's data-gradient image and float32 master (a subclass whose layer has other images overrides this and _layer)"""
        return dict(bwd=self.ops.pack_data_grad(w), master=self.ops.A.upload(np.ascontiguousarray(w)))

    def _weight_entry(self, i, stem, ly):
        """SGD.add's arguments for layer i's conv weight"""
        o = self.ops
        shape = (ly["cout"], ly["cin"], 3, 3)
        return dict(name=stem + "_weight", weight=o.A.view_f32(ly["master"], shape), grad=o.A.view_f32(o.buf(("dW", i), ly["cout"] * ly["cin"] * 36), shape),
                    pack=dict(self._fwd_image(ly), bwd=ly["bwd"][0], dtype=o.dt))

    def optimizer_entries(self):
        """What rangedet_amd.optim.SGD.attach registers, one dict of SGD.add's arguments per trainable parameter: its reference name, the
        float32 master weight and the gradient buffer backward() fills (the buffers TowerOps keys by step and layer: their addresses do not
        depend on the input shape), and for a conv weight the two images the step re-packs from the master -- `fwd`, which forward() reads
        (with the layer's fold scale, if it has one), and `bwd`, which the data gradient reads."""
        o = self.ops
        A, n = o.A, len(self.layers)
        for i, (stem, ly) in enumerate(zip(self._stems, self.layers)):
            yield self._weight_entry(i, stem, ly)
            yield from self._norm_entries(i, stem, ly)
        cin = self.layers[n - 1]["cout"]
        yield dict(name=self.out_names[0], weight=A.view_f32(self.out_w, (self.nout, cin, 1, 1)),
                   grad=A.view_f32(o.buf(("hob_dw", 0), self.nout * cin * 4), (self.nout, cin, 1, 1)))
        yield dict(name=self.out_names[1], weight=A.view_f32(self.out_b, (self.nout,)), grad=A.view_f32(o.buf(("hob_db", 0), self.nout * 4), (self.nout,)))

    def forward(self, x):
        o = self.ops
        A, last = o.A, self.layers[-1]
        B, H, W, C = _check16(x, "x")
        if C != self.layers[0]["cin"]:
            raise ValueError("forward: %d input channels, the first conv takes %d" % (C, self.layers[0]["cin"]))
        acts = [x]
        for i in range(len(self.layers)):
            acts.append(self._layer_forward(i, acts[-1]))
        out = o.buf(("out", 0), B * H * W * self.nout * 4)
        o.L.call("rd_head_out", rdlib.ptr(acts[-1]), last["cout"], 0, A.ptr(self.out_w), A.ptr(self.out_b), A.ptr(out), H * W * self.nout, 0,
                 B, H, W, last["cout"], self.nout, o.dt, _stream(A))
        self.acts = acts
        return A.view_f32(out, (B, H * W, self.nout))

    def _weight_grad(self, i, x, dz):
        return self.ops.weight_grad(x, dz, tag=i)

    def backward(self, d_out, n_off=0, out_batch_stride=None):
        """d_out: the float32 gradient of the head output, the level at pixel offset n_off of each frame's run -- RpnLoss's flat d_logit
        (B, N) / d_delta (B, N, 8) are read in place.  -> (the gradient of the tower input in the activation type, {reference parameter
        name: float32 gradient}).  Keeps each layer's dL/dy, dz and input gradient in self.gs, self.dzs, self.dxs (input side first)."""
        if self.acts is None:
            raise RuntimeError("backward before forward: the activations are kept by forward(x)")
        o, acts, n = self.ops, self.acts, len(self.layers)
        g, dw, db = o.head_out_bwd(d_out, acts[n], self.out_w, self.nout, n_off, out_batch_stride, **self._out_bwd_kwargs())
        grads = {self.out_names[0]: dw.reshape(self.nout, self.layers[-1]["cout"], 1, 1), self.out_names[1]: db}
        gs, dzs, dxs = [None] * n, [None] * n, [None] * n
        for i in range(n - 1, -1, -1):
            gs[i] = g
            dzs[i] = self._dz(i, g, grads)
            grads[self._stems[i] + "_weight"] = self._weight_grad(i, acts[i], dzs[i])
            g = dxs[i] = o.data_grad(dzs[i], self.layers[i]["bwd"], tag=i)
        self.gs, self.dzs, self.dxs = gs, dzs, dxs
        return g, grads


class HeadTowerTrain(_HeadTower):
    """One tower ('cls' or 'reg') of one pyramid level as the reference trains it: every layer is conv3x3 (no bias) + BatchNorm with the
    batch's own statistics + ReLU (normalizer_factory(type="localbn"), the BatchNorm named <conv name>_bn), then the 1x1 output conv.
      conv_weights                 (cout, cin, 3, 3) float32, input side first; index `first_conv` names the first of them
      gammas, betas                the BatchNorm parameters of each layer (cout values each)
      moving_means, moving_vars    its auxiliary states: copied to the device once, updated there by every forward()
    forward(x) -> the float32 head output (B, H * W, nout): per layer the unscaled conv, rd_bn_stats, rd_bn_fold, rd_affine_relu, then
    rd_head_out.  backward(d_out, n_off) -> (the gradient of the tower input, {reference parameter name: float32 gradient}): rd_head_out_bwd,
    then per layer rd_bn_relu_bwd, rd_conv3x3_bwd_weight and the data gradient.  aux() -> {name: float32 device vector} of the moving
    statistics.  Nothing synchronises with the host.  Keeps x and every activation in self.acts, every conv output in self.zs, and after
    backward() each layer's dL/dy, dz and input gradient in self.gs, self.dzs, self.dxs (input side first)."""

    def __init__(self, conv_weights, gammas, betas, moving_means, moving_vars, out_weight, out_bias, kind="cls", level=0, first_conv=0,
                 eps=BN_EPS, momentum=BN_MOMENTUM, dtype=rdlib.RD_BF16, lib=None, alloc=None):
        super().__init__(conv_weights, (gammas, betas, moving_means, moving_vars), "gamma, beta, moving mean and moving variance",
                         out_weight, out_bias, kind, level, first_conv, dtype, lib, alloc)
        self.names = self._stems
        self.eps, self.momentum = float(eps), float(momentum)
        self.zs = self.saved = None

    def _layer(self, w, name, gamma, beta, mmean, mvar):
        o, cout = self.ops, w.shape[0]
        return dict(fwd=o.pack_unscaled(w), gamma=_vec(o, gamma, cout, name + "_bn_gamma"), beta=_vec(o, beta, cout, name + "_bn_beta"),
                    mmean=_vec(o, mmean, cout, name + "_bn_moving_mean"), mvar=_vec(o, mvar, cout, name + "_bn_moving_var"))

    def _fwd_image(self, ly):
        return dict(fwd=ly["fwd"][0])

    def _norm_entries(self, i, stem, ly):
        o, C = self.ops, ly["cout"]
        for key, grad in (("gamma", "bn_dgamma"), ("beta", "bn_dbeta")):
            yield dict(name="%s_bn_%s" % (stem, key), weight=o.A.view_f32(ly[key], (C,)), grad=o.A.view_f32(o.buf((grad, i), C * 4), (C,)))

    def aux(self):
        A, out = self.ops.A, {}
        for name, ly in zip(self.names, self.layers):
            out[name + "_bn_moving_mean"] = A.view_f32(ly["mmean"], (ly["cout"],))
            out[name + "_bn_moving_var"] = A.view_f32(ly["mvar"], (ly["cout"],))
        return out

    def forward(self, x, unbiased=True):
        self._unbiased, self.zs, self.saved = unbiased, [], []
        return super().forward(x)

    def _layer_forward(self, i, x):
        o, ly = self.ops, self.layers[i]
        z = o.conv_unscaled(x, ly["fwd"], ly["cin"], ly["cout"], tag=i)
        mean, var = o.bn_stats(z, tag=i)
        rstd, a, b = o.bn_fold(mean, var, ly["gamma"], ly["beta"], ly["mmean"], ly["mvar"], int(np.prod(z.shape[:3])), ly["cout"], self.eps,
                               self.momentum, self._unbiased, tag=i)
        self.zs.append(z)
        self.saved.append(dict(a=a, b=b, mean=mean, var=var, rstd=rstd))
        return o.affine_relu(z, a, b, tag=i)

    def _out_bwd_kwargs(self):
        return {}

    def _dz(self, i, g, grads):
        name = self.names[i]
        dz, grads[name + "_bn_gamma"], grads[name + "_bn_beta"] = self.ops.bn_relu_bwd(g, self.zs[i], self.saved[i], self.layers[i]["gamma"], tag=i)
        return dz


class HeadTowerBackward(_HeadTower):
    """One tower ('cls' or 'reg') of one pyramid level with inference-mode normalisation.
      conv_weights   the tower's (cout, cin, 3, 3) float32 conv weights, input side first; index `first_conv` names the first of them
      scales, shifts the folded normalisation of each layer (cout values each)
      out_weight     (nout, cin[, 1, 1]) and out_bias (nout): rpn_cls_logit (nout 1) / rpn_reg_delta (nout 8)
    forward(x) -> the float32 head output (B, H * W, nout) through the unfused launches (rd_conv3x3_bn_act_ex per layer, then rd_head_out:
    the shipped fused last-conv + output-conv launch never writes the activation the backward needs).  backward(d_out, n_off) -> (the
    gradient of the tower input in the activation type, {reference parameter name: float32 gradient})."""

    def __init__(self, conv_weights, scales, shifts, out_weight, out_bias, kind="cls", level=0, first_conv=0, dtype=rdlib.RD_BF16,
                 lib=None, alloc=None):
        super().__init__(conv_weights, (scales, shifts), "scale and one shift", out_weight, out_bias, kind, level, first_conv, dtype, lib, alloc)
        self.names = [s + "_weight" for s in self._stems]

    def _layer(self, w, name, s, t):
        o, (cout, cin) = self.ops, w.shape[:2]
        s, t = np.ascontiguousarray(s, dtype=np.float32), np.ascontiguousarray(t, dtype=np.float32)
        if s.shape != (cout,) or t.shape != (cout,):
            raise ValueError("%s: scale / shift of %d values" % (name, cout))
        return dict(fwd=o.A.upload(o.L.pack_conv3x3_ex(w, 1, cin, fold_scale=s, dtype=o.dt)), shift=o.A.upload(t), scale=o.A.upload(s))

    def _fwd_image(self, ly):
        return dict(fwd=ly["fwd"], fold_scale=ly["scale"])

    def _norm_entries(self, i, stem, ly):
        return ()                      # the folded scale and shift are fixed: inference-mode normalisation has nothing to train

    def _layer_forward(self, i, x):
        ly = self.layers[i]
        return self.ops.conv3x3(x, ly["fwd"], ly["shift"], ly["cin"], ly["cout"], rdlib.RD_SCALE_FOLDED | rdlib.RD_RELU_PRE, ("act", i))

    def _out_bwd_kwargs(self):
        """the output conv's backward applies the last layer's mask and scale itself: its dx is that layer's dz"""
        return dict(scale=self.layers[-1]["scale"], relu_mask=True)

    def _dz(self, i, g, grads):
        if i == len(self.layers) - 1:
            return g
        return self.ops.relu_affine_bwd(g, self.acts[i + 1], self.layers[i]["scale"], tag=i)


class Level0TowerTrain(HeadTowerTrain):
    """The level-0 tower as the reference trains it: a HeadTowerTrain whose first layer is the concat conv rpn_{cls,reg}_conv_0_lvl_0 on
    [agg3 | range image] (dla_backbone.py:153-154), the concat never written: conv_weights[0] is (cout, 64 + c, 3, 3) with c the range
    image's channels (8 for Waymo, 5 for KITTI; 1 .. 16), the other layers 128 -> 128.
      forward(x, data) -> the head output; x (B, H, W, 64) the agg3 feature map, data (B, H, W, 16) the range-image slot
                          conv3x3_cat (rd_conv3x3_bn_act_cat, unscaled), then as the tower
      backward(d_out, n_off) -> (the gradient of x, grads): layer 0's weight gradient is weight_grad_cat in the reference's shape
                          (cout, 64 + c, 3, 3), its data gradient towards x the persistent launch on the flipped image of w[:, :64]; the
                          range image takes no gradient
    The concat forward reads a multiple of 8 range-image channels, so the device master is kept at that width, (cout, 64 + c8, 3, 3) with
    c8 = c rounded up to 8 and the columns from 64 + c on zero.  They stay exactly zero through any number of steps: the gradient buffer
    has the master's layout, is zeroed once when it is made, and rd_conv3x3_bwd_weight_cat_padded never writes those columns, so their
    update is momentum * 0 - lr wd * 0 - lr * 0.  With c a multiple of 8 there is no padding.  Slot channels c .. c8 - 1 of `data` meet
    only those zero weights.  The returned gradient is the (cout, 64 + c, 3, 3) view of that buffer.
    optimizer_entries() names the concat weight with pack=dict(cat=(64, c8), ...): SGD.step() re-packs both images from the master."""

    def __init__(self, conv_weights, gammas, betas, moving_means, moving_vars, out_weight, out_bias, kind="cls", level=0, first_conv=0,
                 eps=BN_EPS, momentum=BN_MOMENTUM, dtype=rdlib.RD_BF16, lib=None, alloc=None):
        super().__init__(conv_weights, gammas, betas, moving_means, moving_vars, out_weight, out_bias, kind, level, first_conv, eps, momentum,
                         dtype, lib, alloc)
        self.data = None

    def _layer_channels(self, i, w, name):
        if i:
            return super()._layer_channels(i, w, name)
        if w.shape[0] not in (64, 128) or not 64 < w.shape[1] <= 80:
            raise NotImplementedError("%s: %r -- the concat conv is a (cout, 64 + c, 3, 3) weight, c 1 .. 16" % (name, w.shape))
        self.c = int(w.shape[1]) - 64
        self.c8 = (self.c + 7) // 8 * 8
        return int(w.shape[0]), 64              # the tower's input x is the 64-channel half

    def _layer(self, w, name, gamma, beta, mmean, mvar):
        if self.layers:
            return super()._layer(w, name, gamma, beta, mmean, mvar)
        return self._layer0(w, name, gamma, beta, mmean, mvar)

    def _layer0(self, w, name, gamma, beta, mmean, mvar):
        o, cout = self.ops, w.shape[0]
        return dict(fwd=o.pack_cat(self._padded(w), self.c8), gamma=_vec(o, gamma, cout, name + "_bn_gamma"), beta=_vec(o, beta, cout, name + "_bn_beta"),
                    mmean=_vec(o, mmean, cout, name + "_bn_moving_mean"), mvar=_vec(o, mvar, cout, name + "_bn_moving_var"))

    def _padded(self, w):
        wp = np.zeros((w.shape[0], 64 + self.c8, 3, 3), np.float32)
        wp[:, :64 + self.c] = w
        return wp

    def _weight_images(self, i, w):
        if i:
            return super()._weight_images(i, w)
        o = self.ops
        return dict(bwd=o.pack_data_grad(np.ascontiguousarray(w[:, :64])), master=o.A.upload(self._padded(w)))

    def _weight_entry(self, i, stem, ly):
        if i:
            return super()._weight_entry(i, stem, ly)
        o = self.ops
        shape = (ly["cout"], 64 + self.c8, 3, 3)
        return dict(name=stem + "_weight", weight=o.A.view_f32(ly["master"], shape),
                    grad=o.A.view_f32(o.buf(("dWc", 0), ly["cout"] * (64 + self.c8) * 36, zero=True), shape),
                    pack=dict(cat=(64, self.c8), fwd=ly["fwd"][0], bwd=ly["bwd"][0], dtype=o.dt))

    def forward(self, x, data, unbiased=True):
        if _check16(data, "data") != tuple(int(v) for v in x.shape[:3]) + (16,):
            raise ValueError("forward: data %r with x %r -- the (B, H, W, 16) range-image slot" % (tuple(data.shape), tuple(x.shape)))
        self.data = data
        return super().forward(x, unbiased)

    def _layer_forward(self, i, x):
        if i:
            return super()._layer_forward(i, x)
        o, ly = self.ops, self.layers[0]
        z = o.conv3x3_cat(x, self.data, self.c8, ly["fwd"], ly["cout"], tag=0)
        mean, var = o.bn_stats(z, tag=0)
        rstd, a, b = o.bn_fold(mean, var, ly["gamma"], ly["beta"], ly["mmean"], ly["mvar"], int(np.prod(z.shape[:3])), ly["cout"], self.eps,
                               self.momentum, self._unbiased, tag=0)
        self.zs.append(z)
        self.saved.append(dict(a=a, b=b, mean=mean, var=var, rstd=rstd))
        return o.affine_relu(z, a, b, tag=0)

    def _weight_grad(self, i, x, dz):
        if i:
            return super()._weight_grad(i, x, dz)
        return self.ops.weight_grad_cat(x, self.data, self.c, dz, tag=0, cin_stride=64 + self.c8)[:, :64 + self.c]

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
so a result is valid until the next such call.  Inference-mode normalisation only (no batch statistics, no gradients of s and t); the
level-0 conv_0 (input: the un-materialised 64 + 8 channel concat) and strided / transposed convs are refused.
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


class _Ops:
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

    def buf(self, key, nbytes):
        k = (key, nbytes)
        if k not in self._bufs:
            self._bufs[k] = self.A.alloc(nbytes)
        return self._bufs[k]

    def pack_data_grad(self, w_oihw):
        """the forward launch's weight image of the data gradient: axes swapped, taps flipped, no scale"""
        w = np.asarray(w_oihw, np.float32)
        cout, cin = w.shape[:2]
        wf = np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])
        return self.A.upload(self.L.pack_conv3x3_ex(wf, 1, cout, fold_scale=None, dtype=self.dt)), self.A.upload(np.zeros(cin, np.float32)), cin

    def data_grad(self, dz, packed, tag=0):
        """dz (B, H, W, cout) -> dx (B, H, W, cin); packed = pack_data_grad(W)"""
        A, L = self.A, self.L
        img, zero_shift, cin = packed
        B, H, W, cout = _check16(dz, "dz")
        out = self.buf(("dx", tag), B * H * W * cin * 2)
        L.call("rd_conv3x3_bn_act_ex", rdlib.ptr(dz), cout, 0, A.ptr(img), None, A.ptr(zero_shift), None, 0, 0, None, 0, 0, 0, None,
               A.ptr(out), cin, 0, B, H, W, cout, cin, 1, rdlib.RD_SCALE_FOLDED, self.dt, _stream(A))
        return _view16(A, out, (B, H, W, cin), self.dt)

    def weight_grad(self, x, dz, tag=0, split=0):
        """x (B, H, W, cin), dz (B, H, W, cout) -> dW (cout, cin, 3, 3) float32"""
        A, L = self.A, self.L
        B, H, W, cin = _check16(x, "x")
        if _check16(dz, "dz")[:3] != (B, H, W):
            raise ValueError("weight_grad: x %r and dz %r differ in B, H or W" % (tuple(x.shape), tuple(dz.shape)))
        cout = int(dz.shape[3])
        if cin not in (64, 128) or cout not in (64, 128):
            raise NotImplementedError("weight_grad: %d -> %d channels; the kernel runs 64 or 128 on either side" % (cin, cout))
        nws = L.raw("rd_conv3x3_bwd_weight_workspace_bytes")(B, H, W, cin, cout, split)
        ws, out = self.buf(("bww_ws", 0), nws), self.buf(("dW", tag), cout * cin * 36)
        L.call("rd_conv3x3_bwd_weight", rdlib.ptr(x), cin, 0, rdlib.ptr(dz), cout, 0, A.ptr(out), B, H, W, cin, cout, split, self.dt, A.ptr(ws),
               nws, _stream(A))
        return A.view_f32(out, (cout, cin, 3, 3))

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


_OPS = {}


def _ops(dtype, lib, alloc):
    if lib is not None or alloc is not None:
        return _Ops(dtype, lib, alloc)
    if dtype not in _OPS:
        _OPS[dtype] = _Ops(dtype)
    return _OPS[dtype]


def conv3x3_data_grad(dz, w_oihw, dtype=rdlib.RD_BF16, lib=None, alloc=None):
    """dL/dx of a stride-1, pad-1 3x3 conv: dz (B, H, W, cout) device tensor of the activation type, w the (cout, cin, 3, 3) float32 weight
    on the host (packed on every call: keep a HeadTowerBackward, or _Ops.pack_data_grad, for repeated use)"""
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


class HeadTowerBackward:
    """One tower ('cls' or 'reg') of one pyramid level.
      conv_weights   the tower's (cout, cin, 3, 3) float32 conv weights, input side first; index `first_conv` names the first of them
      scales, shifts the folded normalisation of each layer (cout values each)
      out_weight     (nout, cin[, 1, 1]) and out_bias (nout): rpn_cls_logit (nout 1) / rpn_reg_delta (nout 8)
    forward(x) -> the float32 head output (B, H * W, nout) through the unfused launches (rd_conv3x3_bn_act_ex per layer, then rd_head_out:
    the shipped fused last-conv + output-conv launch never writes the activation the backward needs).  backward(d_out, n_off) -> (the
    gradient of the tower input in the activation type, {reference parameter name: float32 gradient})."""

    def __init__(self, conv_weights, scales, shifts, out_weight, out_bias, kind="cls", level=0, first_conv=0, dtype=rdlib.RD_BF16,
                 lib=None, alloc=None):
        if kind not in ("cls", "reg"):
            raise ValueError("kind: 'cls' or 'reg', got %r" % (kind,))
        self.ops = o = _Ops(dtype, lib, alloc)
        A, L = o.A, o.L
        if not (len(conv_weights) == len(scales) == len(shifts)) or not conv_weights:
            raise ValueError("one scale and one shift per conv weight, at least one layer")
        self.names, self.layers = [], []
        chans = None
        for i, (w, s, t) in enumerate(zip(conv_weights, scales, shifts)):
            w = np.asarray(w, np.float32)
            name = "rpn_%s_conv_%d_lvl_%d" % (kind, first_conv + i, level)
            if w.ndim != 4 or w.shape[2:] != (3, 3):
                raise NotImplementedError("%s: kernel %r -- 3x3, stride 1, pad 1 only (no strided or transposed conv)" % (name, w.shape[2:]))
            cout, cin = w.shape[:2]
            if cin not in (64, 128) or cout not in (64, 128):
                why = " (the level-0 conv_0 reads the un-materialised concat of 64 + 8 channels: the concat conv has no backward here)" \
                    if cin == 72 else ""
                raise NotImplementedError("%s: %d -> %d channels; the backward kernels run 64 or 128 on either side%s" % (name, cin, cout, why))
            if chans is not None and cin != chans:
                raise ValueError("%s: %d input channels after a layer with %d outputs" % (name, cin, chans))
            chans = cout
            s, t = np.ascontiguousarray(s, dtype=np.float32), np.ascontiguousarray(t, dtype=np.float32)
            if s.shape != (cout,) or t.shape != (cout,):
                raise ValueError("%s: scale / shift of %d values" % (name, cout))
            self.names.append(name + "_weight")
            self.layers.append(dict(cin=cin, cout=cout, fwd=A.upload(L.pack_conv3x3_ex(w, 1, cin, fold_scale=s, dtype=dtype)), shift=A.upload(t),
                                    scale=A.upload(s), bwd=o.pack_data_grad(w)))
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
        self.out_w, self.out_b = A.upload(ow), A.upload(ob)
        self.acts = None

    def forward(self, x):
        o = self.ops
        A, L = o.A, o.L
        B, H, W, C = _check16(x, "x")
        if C != self.layers[0]["cin"]:
            raise ValueError("forward: %d input channels, the first conv takes %d" % (C, self.layers[0]["cin"]))
        st, acts = _stream(A), [x]
        for i, ly in enumerate(self.layers):
            y = o.buf(("act", i), B * H * W * ly["cout"] * 2)
            L.call("rd_conv3x3_bn_act_ex", rdlib.ptr(acts[-1]), ly["cin"], 0, A.ptr(ly["fwd"]), None, A.ptr(ly["shift"]), None, 0, 0, None, 0, 0, 0,
                   None, A.ptr(y), ly["cout"], 0, B, H, W, ly["cin"], ly["cout"], 1, rdlib.RD_SCALE_FOLDED | rdlib.RD_RELU_PRE, o.dt, st)
            acts.append(_view16(A, y, (B, H, W, ly["cout"]), o.dt))
        out = o.buf(("out", 0), B * H * W * self.nout * 4)
        L.call("rd_head_out", rdlib.ptr(acts[-1]), self.layers[-1]["cout"], 0, A.ptr(self.out_w), A.ptr(self.out_b), A.ptr(out), H * W * self.nout, 0,
               B, H, W, self.layers[-1]["cout"], self.nout, o.dt, st)
        self.acts = acts
        return A.view_f32(out, (B, H * W, self.nout))

    def backward(self, d_out, n_off=0, out_batch_stride=None):
        """d_out: the float32 gradient of the head output, the level at pixel offset n_off of each frame's run -- RpnLoss's flat d_logit
        (B, N) / d_delta (B, N, 8) are read in place.  Also keeps every layer's dz and input gradient in self.dzs / self.dxs (input side first)."""
        if self.acts is None:
            raise RuntimeError("backward before forward: the activations are kept by forward(x)")
        o, acts, n = self.ops, self.acts, len(self.layers)
        last = self.layers[-1]
        dz, dw, db = o.head_out_bwd(d_out, acts[n], self.out_w, self.nout, n_off, out_batch_stride, scale=last["scale"], relu_mask=True)
        grads = {self.out_names[0]: dw.reshape(self.nout, last["cout"], 1, 1), self.out_names[1]: db}
        dzs, dxs = [None] * n, [None] * n
        dx = None
        for i in range(n - 1, -1, -1):
            ly = self.layers[i]
            dzs[i] = dz
            grads[self.names[i]] = o.weight_grad(acts[i], dz, tag=i)
            dx = dxs[i] = o.data_grad(dz, ly["bwd"], tag=i)
            if i > 0:
                dz = o.relu_affine_bwd(dx, acts[i], self.layers[i - 1]["scale"], tag=i - 1)
        self.dzs, self.dxs = dzs, dxs
        return dx, grads

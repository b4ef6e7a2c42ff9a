"""Executor: binds a lowered Plan (rangedet_amd.lower) to device buffers and parameters and replays it as C-ABI calls
into librangedet_hip.so on one HIP stream.  PyTorch is used only as the device allocator / stream provider.

Binding happens ONCE, in the constructor: one binder per step kind (Executor._BINDERS) turns a plan step into its library calls, each an
entry-point name with its complete argument tuple, counted against lib.SIGNATURES there and then.  What stays open until forward() is
the stream (read per call of forward, always the entry's last argument) and the caller's input tensors (Input slots).  forward()
resolves those and replays the calls; it knows no step kind.

This is the build's counterpart of the reference's DetModule.bind/set_params/forward/get_outputs
(utils/detection_module.py:419-510,627-679,783-805) for the test symbol: ``Executor(plan, params).forward(inputs)``
returns the Group outputs [rec_id, fg_cls_score, decoded_bbox, zeros, gt_bbox_imu, gt_class] (builder.py:77).
"""
from collections import namedtuple

import numpy as np

from . import lib as rdlib
from .lower import step_refs


class TorchAllocator:
    """Device memory + stream through torch (ROCm).  Fails loudly without a GPU -- there is no CPU path."""

    def __init__(self, device="cuda:0", stream=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("rangedet_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.torch = torch
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self._stream = stream

    @property
    def stream(self):
        st = self._stream or self.torch.cuda.current_stream(self.device)
        return st.cuda_stream

    def alloc(self, nbytes, zero=False):
        f = self.torch.zeros if zero else self.torch.empty
        return f(max(int(nbytes), 16), dtype=self.torch.uint8, device=self.device)

    def upload(self, arr):
        a = np.ascontiguousarray(arr)
        t = self.torch.from_numpy(a.view(np.uint8).reshape(-1)).to(self.device)
        return t

    def ptr(self, buf):
        return buf.data_ptr()

    def view_f32(self, buf, shape):
        n = int(np.prod(shape))
        return buf[: n * 4].view(self.torch.float32).view(*shape)

    def view_i32(self, buf, shape):
        n = int(np.prod(shape))
        return buf[: n * 4].view(self.torch.int32).view(*shape)

    def to_numpy(self, t):
        return t.detach().cpu().numpy()

    def as_device_f32(self, x):
        """numpy / torch input -> contiguous float32 device tensor (no copy if it already is one)."""
        t = self.torch
        if isinstance(x, np.ndarray):
            return t.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)
        return x.to(device=self.device, dtype=t.float32).contiguous()

    def assign(self, dst_view, src):
        dst_view.copy_(src.reshape(dst_view.shape))

    # ---- streams / events (the post-processing of frame i overlaps the forward of frame i+1) ----------------
    def new_stream(self, priority=0):
        """priority: 0 = normal, -1 = high (torch's convention; the HIP runtime maps it onto the hardware queue's priority)."""
        return self.torch.cuda.Stream(device=self.device, priority=priority)

    def stream_ptr(self, stream):
        return stream.cuda_stream if stream is not None else self.stream

    def record_event(self, stream=None):
        ev = self.torch.cuda.Event()
        ev.record(stream if stream is not None else self.torch.cuda.current_stream(self.device))
        return ev

    def wait_event(self, ev, stream=None):
        (stream if stream is not None else self.torch.cuda.current_stream(self.device)).wait_event(ev)

    def sync(self):
        self.torch.cuda.synchronize(self.device)


def bn_affine(P, name, eps, pad_to=None):
    """inference BatchNorm as scale / shift; pad_to: zero-padded output channels of a layer that runs on a wider kernel (scale 1, shift 0)"""
    g, b, m, v = (np.asarray(P[name + s], np.float64) for s in ("_gamma", "_beta", "_moving_mean", "_moving_var"))
    s = g / np.sqrt(v + eps)
    s, t = s.astype(np.float32), (b - m * s).astype(np.float32)
    if pad_to is not None and pad_to > len(s):
        s = np.concatenate([s, np.ones(pad_to - len(s), np.float32)])
        t = np.concatenate([t, np.zeros(pad_to - len(t), np.float32)])
    return s, t


def pad_rows(w, n, axis=0):
    """weights with zero rows appended along `axis` up to n (a layer whose logical width runs zero-padded on a 64 / 128-channel kernel)"""
    if w.shape[axis] >= n:
        return w
    shp = list(w.shape)
    shp[axis] = n - w.shape[axis]
    return np.concatenate([w, np.zeros(shp, w.dtype)], axis)


def cmap_cols(w, cmap):
    """weights (cout, logical cin, ...) -> (cout, physical cin, ...): the input buffer carries alignment padding (lower.TRef.cmap, physical ->
    logical channel or -1), zero weight columns there"""
    if not cmap:
        return w
    wp = np.zeros((w.shape[0], len(cmap)) + w.shape[2:], np.float32)
    for pc, lc in enumerate(cmap):
        if lc >= 0:
            wp[:, pc] = w[:, lc]
    return wp


# An argument the caller supplies per forward(): the float32 device copy of inputs[name]; shape = what its leading dimensions must be
# (all of them when exact)
Input = namedtuple("Input", "name shape exact")


class Executor:
    def __init__(self, plan, params, lib=None, alloc=None, reuse_buffers=True, keep_sorted_idx=False):
        """keep_sorted_idx: also keep get_sorted_foreground's (B,k) flat indices (parity tests read them with sorted_idx())."""
        self.keep_sorted_idx = keep_sorted_idx
        self.plan = plan
        self.lib = lib or rdlib.get_lib()
        self.alloc = alloc or TorchAllocator()
        self.dtype = plan.dtype
        self.B = plan.batch
        self._phys = {}
        self._held = []            # uploaded images and workspaces: the bound calls carry their addresses only
        self._sorted_idx = []      # per sorted_fg step: (index buffer, k)
        self._assign_buffers(reuse_buffers)
        self._bound = [self._bind(st, params) for st in plan.steps]   # per step: [(entry, arguments without the stream, input slots)]

    # ---- memory ------------------------------------------------------------------------------------------------
    def _assign_buffers(self, reuse):
        """One allocation per logical buffer; two non-persistent buffers of one size share it when their live ranges -- first to last step
        holding a reference at any depth (lower.step_refs) -- do not overlap.  A reference to a buffer the plan no longer has (the
        intermediate tensor inside a fused block) is not a use."""
        plan = self.plan
        last_use, first_def = {}, {}
        for i, st in enumerate(plan.steps):
            for _, v in step_refs(st):
                if v.buf in plan.buffers:
                    last_use[v.buf] = i
                    first_def.setdefault(v.buf, i)
        for _, v in step_refs(plan.outputs):
            last_use[v.buf] = len(plan.steps) + 1
        free = {}
        release = {}
        for b, i in last_use.items():
            release.setdefault(i, []).append(b)
        order = sorted(plan.buffers, key=lambda b: first_def.get(b, 0))
        by_def = {}
        for b in order:
            by_def.setdefault(first_def.get(b, 0), []).append(b)
        for i in range(len(plan.steps) + 2):
            for b in by_def.get(i, []):
                info = plan.buffers[b]
                if reuse and not info["persistent"] and free.get(info["nbytes"]):
                    self._phys[b] = free[info["nbytes"]].pop()
                else:
                    self._phys[b] = self.alloc.alloc(info["nbytes"], zero=info["zero"])
            for b in release.get(i, []):
                info = plan.buffers[b]
                if reuse and not info["persistent"] and last_use[b] <= len(plan.steps):
                    free.setdefault(info["nbytes"], []).append(self._phys[b])
        self.device_bytes = sum(int(t.numel()) if hasattr(t, "numel") else len(t) for t in {id(v): v for v in self._phys.values()}.values())

    def p(self, ref):
        return self.alloc.ptr(self._phys[ref.buf])

    def _up(self, arr):
        """address of a device copy of `arr` that lives as long as the executor (None stays None)"""
        if arr is None:
            return None
        self._held.append(self.alloc.upload(arr))
        return self.alloc.ptr(self._held[-1])

    def _ws(self, nbytes):
        self._held.append(self.alloc.alloc(nbytes))
        return self._held[-1]

    def _at(self, ref):
        """(address, channel stride, channel offset) of an activation; (None, 0, 0) for an operand that is not there"""
        return (self.p(ref), ref.cs, ref.co) if ref is not None else (None, 0, 0)

    # ---- binding: plan step -> library calls -------------------------------------------------------------------------
    def _bind(self, st, P):
        binder = self._BINDERS.get(st["kind"])
        if binder is None:
            raise RuntimeError("unknown plan step %r" % st["kind"])
        calls = []
        for name, *args in binder(self, st, P):
            want = len(rdlib.SIGNATURES[name][1]) - 1          # (the stream, every entry's last argument, is added per forward)
            if len(args) != want:
                raise TypeError("step %r (%s): %s bound with %d arguments before the stream, the library takes %d" %
                                (st.get("name", ""), st["kind"], name, len(args), want))
            calls.append((name, tuple(args), tuple((j, a) for j, a in enumerate(args) if isinstance(a, Input))))
        return calls

    def _bind_nchw_in(self, st, P):
        o, B = st["out"], self.B
        yield ("rd_nchw_to_nhwc", Input(st["name"], (B, o.C, o.H, o.W), True), self.p(o), B, o.C, o.H, o.W, o.cs, o.co, st["zero_pad"], self.dtype)

    def _bind_block(self, st, P):
        """a fused BasicBlock (lower._fuse_blocks): both 3x3 weights in one image, the shortcut's as for the unfused conv2"""
        L, dt = self.lib, self.dtype
        ca, cb, x, o = st["a"], st["b"], st["x"], st["out"]
        w1, w2 = (np.asarray(P[c["name"] + "_weight"], np.float32) for c in (ca, cb))
        w1 = cmap_cols(w1, ca.get("cmap"))      # (the first block's input buffer carries alignment padding)
        (s1, t1), (s2, t2) = bn_affine(P, ca["bn"], ca["eps"]), bn_affine(P, cb["bn"], cb["eps"])
        cin = w1.shape[1]
        m16 = bool(st.get("m16")) and cin == 64      # the 16 x 16 x 32 MFMA form (lower._mark_mfma16): its own weight images
        sc_w = None
        if cb.get("sc"):
            sc = cb["sc"]
            wsc = cmap_cols(np.asarray(P[sc["name"] + "_weight"], np.float32).reshape(64, -1), sc.get("cmap"))
            ss, ts = bn_affine(P, sc["bn"], sc["eps"])
            sc_w = L.pack_conv1x1_sc_m16(wsc, ss, dtype=dt) if m16 else L.pack_conv1x1_sc(wsc, fold_scale=ss, dtype=dt)
            t2 = (t2.astype(np.float64) + ts).astype(np.float32)
        tail = (self._up(L.pack_block64(w1, s1, w2, s2, dtype=dt, m16=m16)), self._up(t1), self._up(t2), self._up(sc_w),
                *self._at(o), self.B, x.H, x.W, dt)
        if m16:
            yield ("rd_block64_m16_bn_act", *self._at(x), *tail)
        else:
            yield ("rd_block64_bn_act", *self._at(x), cin, *tail)

    def _conv_form(self, st, cin):
        """How a conv step is launched, decided here and nowhere else.  Returns (form, m16): form = "plain" (the tap kernel), "ex" (the
        persistent 3x3 kernel), "ex_fold" (BatchNorm scale folded into the weights), "ex_sc" (fused projection shortcut), "cat" (two-tensor
        input) or "head" (fused output conv); m16 = the 16 x 16 x 32 MFMA form of "ex_fold" / "head", when the lowering asked for it
        (lower._mark_mfma16) and the library has it for this shape.  cin: physical input channels."""
        head, sc, cat = bool(st.get("head")), bool(st.get("sc")), st.get("x2") is not None
        fold = bool(st.get("ex") and st.get("fold"))
        if head + sc + cat > 1 or ((head or sc) and not st.get("ex")):
            raise NotImplementedError("conv step %r: no launch form for head=%s sc=%s x2=%s ex=%s" % (st["name"], head, sc, cat, st.get("ex")))
        if sc or cat:
            return ("ex_sc" if sc else "cat"), False
        m16 = fold and bool(st.get("m16")) and \
            self.lib.raw("rd_conv3x3_mfma16_ok")(cin, st["cout"], 1, st["x"].W, 1 if head else 0) == 1
        return ("head" if head else "ex_fold" if fold else "ex" if st.get("ex") else "plain"), m16

    def _bind_conv(self, st, P):
        L, dt, B = self.lib, self.dtype, self.B
        x, o, r, cout, sw = st["x"], st.get("out"), st.get("res"), st["cout"], st["stride_w"]
        w = cmap_cols(pad_rows(np.asarray(P[st["name"] + "_weight"], np.float32), cout), st.get("cmap"))
        s, t = bn_affine(P, st["bn"], st["eps"], pad_to=cout)
        form, m16 = self._conv_form(st, w.shape[1])
        folded = form in ("cat", "ex_fold") or (form == "head" and st.get("fold"))
        flags = st["flags"] | (rdlib.RD_SCALE_FOLDED if folded else 0) | (rdlib.RD_MFMA16 if m16 else 0)
        scale = None if folded or form == "ex_sc" else self._up(s)
        if form == "plain":
            yield ("rd_conv2d_bn_act", *self._at(x), self._up(L.pack_conv_weight(w, dt)), scale, self._up(t), *self._at(r), *self._at(o),
                   B, x.H, x.W, st["cin"], cout, st["k"][0], st["k"][1], sw, flags, dt)
            return
        if form == "cat":       # conv over the virtual concat [x | x2] (lower._concat): neither a shared buffer nor a copy exists
            x2 = st["x2"]
            yield ("rd_conv3x3_bn_act_cat", *self._at(x), x.C, *self._at(x2), x2.cs, self._up(L.pack_conv3x3_cat(w, x.C, x2.cs, fold_scale=s, dtype=dt)),
                   self._up(t), *self._at(o), B, x.H, x.W, cout, flags, dt)
            return
        # the persistent 3x3 kernel: scale folded into the weights (the shift then enters through the accumulators) or passed beside them
        wimg = self._up(L.pack_conv3x3_m16(w, s, dtype=dt) if m16 else
                        L.pack_conv3x3_ex(w, sw, x.cs, fold_scale=None if scale is not None else s, dtype=dt))
        if form == "head":      # fused 1x1 output conv (lower._fuse_head_out): the tower output is never written
            h = st["head"]
            r0, r1 = h["rows"]
            hw = np.asarray(P[h["name"] + "_weight"], np.float32).reshape(-1, cout)[r0:r1]
            yield ("rd_conv2d_bn_act_head_out", *self._at(x), wimg, scale, self._up(t), B, x.H, x.W, st["cin"], flags,
                   self._up(L.pack_head_weight(hw, dtype=dt, m16=m16)), self._up(np.asarray(P[h["name"] + "_bias"], np.float32)[r0:r1]),
                   self.p(h["out"]), h["N"] * h["nout"], h["n_off"], h["nout"], dt)
            return
        sc_x, sc_cin, sc_w = None, 0, None
        if form == "ex_sc":     # fused projection shortcut: both BN scales folded into the weights, one shift for the sum
            sc, sc_x = st["sc"], st["sc_x"]
            wsc = np.asarray(P[sc["name"] + "_weight"], np.float32)
            wsc = cmap_cols(pad_rows(wsc.reshape(wsc.shape[0], -1), cout), sc.get("cmap"))
            ss, ts = bn_affine(P, sc["bn"], sc["eps"], pad_to=cout)
            sc_cin, sc_w = len(sc["cmap"]) if sc.get("cmap") else sc["cin"], self._up(L.pack_conv1x1_sc(wsc, fold_scale=ss, dtype=dt))
            t = (t.astype(np.float64) + ts).astype(np.float32)
        yield ("rd_conv3x3_bn_act_ex", *self._at(x), wimg, scale, self._up(t), *self._at(r), *self._at(sc_x), sc_cin, sc_w, *self._at(o),
               B, x.H, x.W, len(st["cmap"]) if st.get("cmap") else st["cin"], cout, sw, flags, dt)

    def _bind_deconv(self, st, P):
        """per-phase launches, or -- where the lowering asked (one_launch) and the library has the form for this layer -- all phases in ONE
        launch (the phase images back to back), or phases 2p | 2p+1 as one 128-channel problem where its tensors are dense besides (agg1:
        128 -> 64, stride 4).  Only the images of the form that is launched are uploaded."""
        L, dt = self.lib, self.dtype
        x, o, r, cout, sw, pw, (kh, kw) = st["x"], st["out"], st["res"], st["cout"], st["stride_w"], st["pad_w"], st["k"]
        w = pad_rows(np.asarray(P[st["name"] + "_weight"], np.float32), cout, axis=1)      # (cin, cout, kh, kw)
        s, t = bn_affine(P, st["bn"], st["eps"], pad_to=cout)
        fold = bool(st.get("fold"))
        imgs = [L.pack_deconv_weight(w, sw, pw, ph, dt, fold_scale=s if fold else None) for ph in range(sw)]
        flags = st["flags"] | (rdlib.RD_SCALE_FOLDED if fold else 0)
        geom = (*self._at(r), *self._at(o), self.B, x.H, x.W, st["cin"], cout, kh, kw, sw, pw)
        dense = all(v.cs == cout and v.co == 0 for v in (o, r) if v is not None)
        all_phases = bool(st.get("one_launch")) and len({len(i) for i in imgs}) == 1 and \
            L.raw("rd_deconv2d_all_phases_ok")(kh, kw, sw, pw, cout, dt) == 1
        if all_phases and dense and L.raw("rd_deconv2d_phase_pairs_ok")(kh, kw, sw, pw, cout, dt) == 1:
            pimgs = [L.pack_deconv_phase_pair(imgs[p], imgs[p + 1], st["cin"], dt) for p in range(0, sw, 2)]
            yield ("rd_deconv2d_bn_act_pairs", *self._at(x), self._up(np.concatenate(pimgs)), len(pimgs[0]), self._up(np.concatenate([t, t])),
                   *geom, flags, dt)
        elif all_phases:
            yield ("rd_deconv2d_bn_act_all", *self._at(x), self._up(np.concatenate(imgs)), len(imgs[0]), self._up(t), *geom, flags, dt)
        else:
            scale, shift = (None if fold else self._up(s)), self._up(t)
            for ph in range(sw):
                yield ("rd_deconv2d_bn_act", *self._at(x), self._up(imgs[ph]), scale, shift, *geom, ph, flags, dt)

    def _bind_meta(self, st, P):
        x, o, B = st["x"], st["out"], self.B
        s1, t1 = bn_affine(P, st["bn1"], st["eps1"])
        s2, t2 = bn_affine(P, st["bn2"], st["eps2"])
        pk = self.lib.pack_meta(P[st["mlp0"] + "_weight"].reshape(32, 3), P[st["mlp0"] + "_bias"],
                                P[st["mlp1"] + "_weight"].reshape(64, 32), P[st["mlp1"] + "_bias"], s1, t1,
                                P[st["agg"] + "_weight"].reshape(64, 576), s2, t2, self.dtype)
        yield ("rd_meta_kernel_fwd", *self._at(x), Input(st["coord"], (B, 3, x.H, x.W), True), self._up(pk), *self._at(o), B, x.H, x.W, self.dtype)

    def _bind_head_out(self, st, P):
        x = st["x"]
        r0, r1 = st["rows"]
        w = np.asarray(P[st["name"] + "_weight"], np.float32).reshape(-1, x.C)[r0:r1]
        yield ("rd_head_out", *self._at(x), self._up(w), self._up(np.asarray(P[st["name"] + "_bias"], np.float32)[r0:r1]), self.p(st["out"]),
               st["N"] * st["nout"], st["n_off"], self.B, x.H, x.W, x.C, st["nout"], self.dtype)

    def _bind_concat_in(self, st, P):
        row = st["N"] * st["last"] * 4                      # bytes of one frame's concatenated row
        off = 0
        for name, n in st["names"]:
            yield ("rd_copy_rows", Input(name, (self.B, n), False), n * st["last"] * 4, self.p(st["out"]), row, off * st["last"] * 4,
                   n * st["last"] * 4, self.B)
            off += n

    def _bind_sorted_fg(self, st, P):
        A, B = self.alloc, self.B
        nb = self.lib.raw("rd_sorted_foreground_workspace_bytes")(st["N"], st["k"]) * B
        idx = self._ws(B * st["k"] * 4) if self.keep_sorted_idx else None
        self._sorted_idx.append((idx, st["k"]))
        yield ("rd_sorted_foreground", self.p(st["score"]), self.p(st["delta"]), self.p(st["pc"]), self.p(st["mask"]), B, st["N"], st["k"],
               st["D"], st["apply_sigmoid"], self.p(st["out_score"]), self.p(st["out_delta"]), self.p(st["out_pc"]),
               A.ptr(idx) if idx is not None else None, A.ptr(self._ws(nb)), nb)

    def _bind_decode(self, st, P):
        yield ("rd_decode3d_bbox", self.p(st["delta"]), self.p(st["pc"]), self.p(st["out"]), self.B, st["k"], st["box_type"], st["is_bin"])

    def _bind_batch_riou(self, st, P):
        three_d = st.get("iou_type", "bev") == "3d"
        yield ("rd_batch_rotated_iou_3d" if three_d else "rd_batch_rotated_iou", self.p(st["boxes"]), 10,
               Input(st["gt"], (self.B, st["n_gt"], 7 if three_d else 8), True), self.p(st["out"]), None, self.B, st["N"], st["n_gt"])

    def _bind_nms3d(self, st, P):
        nb = self.lib.raw("rd_nms3d_workspace_bytes")(st["N"], self.B)
        yield ("rd_nms3d", self.p(st["boxes"]), self.B, st["N"], st["thr"], st["max_keep"], st["normal_iou"], self.p(st["keep"]),
               self.p(st["out"]), self.alloc.ptr(self._ws(nb)), nb)

    _BINDERS = {"nchw_in": _bind_nchw_in, "block": _bind_block, "conv": _bind_conv, "deconv": _bind_deconv, "meta": _bind_meta,
                "head_out": _bind_head_out, "concat_in": _bind_concat_in, "sorted_fg": _bind_sorted_fg, "decode": _bind_decode,
                "batch_riou": _bind_batch_riou, "nms3d": _bind_nms3d}

    # ---- execution ------------------------------------------------------------------------------------------------------
    def forward(self, inputs, only=None, dev=None):
        """inputs: name -> float32 array/tensor WITH batch dim (the reference's data_name list, config:400-404).
        `only` (profiling aid): run just that plan step index.  `dev`: a dict that keeps the inputs' device copies between calls."""
        A, B = self.alloc, self.B
        call, stream = self.lib.call, A.stream
        dev = {} if dev is None else dev
        for calls in (self._bound if only is None else [self._bound[only]]):
            for name, args, slots in calls:
                if slots:
                    args = list(args)
                    for j, slot in slots:
                        if slot.name not in dev:
                            dev[slot.name] = A.as_device_f32(inputs[slot.name])
                        src = dev[slot.name]
                        shape = tuple(src.shape)
                        assert (shape if slot.exact else shape[:len(slot.shape)]) == slot.shape, (slot.name, shape, slot.shape)
                        args[j] = A.ptr(src)
                call(name, *args, stream)
        if only is not None:
            return None
        outs = []
        for kind, v in self.plan.outputs:
            if kind == "flat":
                outs.append(A.view_f32(self._phys[v.buf], (B,) + tuple(v.shape)))
            elif kind == "flat_i32":
                outs.append(A.view_i32(self._phys[v.buf], (B,) + tuple(v.shape)))
            elif kind == "input":
                outs.append(inputs.get(v))
            else:
                outs.append(np.zeros(v, np.float32))
        return outs

    def read_flat(self, ref):
        """numpy copy of a flat float32 plan tensor (B, *shape), e.g. the pre-sort logits/deltas (tests only)."""
        self.alloc.sync()
        return np.array(self.alloc.to_numpy(self.alloc.view_f32(self._phys[ref.buf], (self.B,) + tuple(ref.shape))))

    def sorted_idx(self, which=0):
        """(B,k) int32 flat indices chosen by the which-th get_sorted_foreground step (needs keep_sorted_idx=True)."""
        idx, k = self._sorted_idx[which]
        self.alloc.sync()
        return np.array(self.alloc.to_numpy(self.alloc.view_i32(idx, (self.B, k))))

    def debug_tensor(self, ref):
        """NCHW float32 numpy copy of an activation (tests only)."""
        A, L = self.alloc, self.lib
        out = A.alloc(self.B * ref.C * ref.H * ref.W * 4)
        L.call("rd_nhwc_to_nchw", self.p(ref), A.ptr(out), self.B, ref.C, ref.H, ref.W, ref.cs, ref.co, self.dtype, A.stream)
        A.sync()
        return A.to_numpy(A.view_f32(out, (self.B, ref.C, ref.H, ref.W)))

"""The parameter update on the device: the step after rangedet_amd.backward's towers, which hand back float32 gradients keyed by the
reference's parameter names.  The reference trains with mx.optimizer `sgd` (tools/train.py:306-365: momentum, wd, rescale_grad,
clip_gradient, and multi_precision under fp16; config/rangedet/*.py OptimizeParam.optimizer: momentum 0.9, wd 1e-5, clip_gradient 35) and
takes the learning rate from a scheduler (tools/train.py:268-291, utils/lr_scheduler.py), restated here as plain host functions.

    opt = SGD(lr=0.01, lr_scheduler=WarmupCosine(0.01, 0.0, warmup_iters, total_iters))
    opt.attach(tower)                        # every parameter of a HeadTowerTrain / HeadTowerBackward, with its weight images
    out = tower.forward(x); dx, grads = tower.backward(d_out); opt.step()      # the next forward() runs on the new weights

A step is rd_sgd_mom_update on a table of all registered tensors (csrc/k_optim.h): one launch updates the float32 master weights and
momenta, a second rewrites the 16-bit conv weight images the persistent conv reads from the updated masters.  The images of a transposed
conv (an `agg` stage's Deconvolution) are not in the table: step() re-packs them with one rd_pack_deconv_dev launch each, behind the
update.  Nothing goes through the
host and nothing synchronises; the table is built and uploaded on the first step and again only when a registered buffer has moved.
Per element, float32, one rounding per operation (MXNet's mp_sgd_mom_update as documented; not pinned by a run of the reference):
    g = rescale_grad * grad;  g = clip(g, -clip_gradient, clip_gradient) if clip_gradient >= 0
    mom = momentum * mom - (lr_t * wd_t) * w - lr_t * g;  w = w + mom            lr_t = lr * lr_mult, wd_t = wd * wd_mult
"""
import math

import numpy as np

from . import lib as rdlib


def default_wd_mult(name):
    """MXNet's rule (Optimizer.set_wd_mult): weight decay on names ending in _weight or _gamma, none on biases, betas and the rest"""
    return 1.0 if name.endswith("_weight") or name.endswith("_gamma") else 0.0


# ---- learning-rate schedules (host, pure Python) ---------------------------------------------------------------------------------------------
class WarmupCosine:
    """lr_mode = 'cosine' of tools/train.py:268-282: a linear scheduler from warmup_lr to base_lr over warmup_iters updates, then a cosine
    one from base_lr to 0 over the remaining total_iters - warmup_iters, composed as the reference's LRSequential composes them: the update
    is clamped to total_iters - 1, each part runs on T = clamp(update - its offset, 0, N) with N = its iterations - 1 (so the last warm-up
    update already gives base_lr, and the last update gives 0).
        warm-up   base_lr + (warmup_lr - base_lr) * (1 - T / N)
        cosine    base_lr * (1 + cos(pi * T / N)) / 2"""

    def __init__(self, base_lr, warmup_lr, warmup_iters, total_iters):
        self.base_lr, self.warmup_lr = float(base_lr), float(warmup_lr)
        self.warmup_iters, self.total_iters = int(warmup_iters), int(total_iters)
        if self.warmup_iters < 0 or self.warmup_iters == 1 or self.total_iters - self.warmup_iters < 2:
            raise ValueError("WarmupCosine: %d warm-up updates (0, or at least 2) of %d (at least 2 after the warm-up): a part of one update "
                             "divides by N = 0" % (self.warmup_iters, self.total_iters))

    def __call__(self, num_update):
        u = min(int(num_update), self.total_iters - 1)
        if u < self.warmup_iters:
            N = self.warmup_iters - 1
            T = min(max(0, u), N)
            return self.base_lr + (self.warmup_lr - self.base_lr) * (1 - T / N)
        N = self.total_iters - self.warmup_iters - 1
        T = min(max(0, u - self.warmup_iters), N)
        return 0 + (self.base_lr - 0) * ((1 + math.cos(math.pi * T / N)) / 2)


class WarmupMultiFactor:
    """utils/lr_scheduler.py WarmupMultiFactorScheduler (the 'step' mode of tools/train.py:284-291): during update <= warmup_step either
    warmup_lr ('constant') or (base_lr - warmup_lr) / warmup_step * update + warmup_lr ('gradual'); afterwards base_lr times `factor`
    once for every entry of `step` that the update has passed (update > step[i]), multiplied one at a time as the reference does."""

    def __init__(self, base_lr, step, factor=0.1, warmup_type="gradual", warmup_lr=0.0, warmup_step=0):
        step = [int(s) for s in step]
        if any(b <= a for a, b in zip(step, step[1:])):
            raise ValueError("WarmupMultiFactor: step must be an increasing list")
        if factor > 1.0:
            raise ValueError("WarmupMultiFactor: factor %r must be no more than 1" % (factor,))
        if warmup_type not in ("constant", "gradual"):
            raise ValueError("WarmupMultiFactor: warmup_type 'constant' or 'gradual', got %r" % (warmup_type,))
        if warmup_step and step and warmup_step >= step[0]:
            raise ValueError("WarmupMultiFactor: warmup_step %d must be smaller than the first step %d" % (warmup_step, step[0]))
        self.base_lr, self.step, self.factor = float(base_lr), step, float(factor)
        self.warmup_type, self.warmup_lr, self.warmup_step = warmup_type, float(warmup_lr), int(warmup_step)

    def __call__(self, num_update):
        if self.warmup_step > 0 and num_update <= self.warmup_step:
            if self.warmup_type == "constant":
                return self.warmup_lr
            return (self.base_lr - self.warmup_lr) / self.warmup_step * num_update + self.warmup_lr
        lr = self.base_lr
        for s in self.step:
            if num_update > s:
                lr *= self.factor
        return lr


# ---- the optimizer ------------------------------------------------------------------------------------------------------------------------------
def _numel(x):
    return int(np.prod(tuple(x.shape))) if len(x.shape) else 1


def _check_f32(x, what):
    item = x.itemsize if isinstance(x, np.ndarray) else x.element_size()
    is_f = (x.dtype == np.float32) if isinstance(x, np.ndarray) else x.dtype.is_floating_point
    if item != 4 or not is_f:
        raise ValueError("%s: a float32 device tensor, got %r" % (what, x.dtype))
    if hasattr(x, "is_contiguous") and not x.is_contiguous() or isinstance(x, np.ndarray) and not x.flags["C_CONTIGUOUS"]:
        raise ValueError("%s: not contiguous" % what)


class SGD:
    """SGD with momentum over float32 device tensors, one library call per step.
      lr, momentum, wd, rescale_grad, clip_gradient   as mx.optimizer.SGD takes them (clip_gradient None or negative: no clipping)
      lr_scheduler    a callable update number -> lr (WarmupCosine, WarmupMultiFactor); None: the fixed lr
    add(name, weight, grad, pack, lr_mult, wd_mult) registers a tensor, attach(tower) every parameter of a head tower; step() advances
    num_update, takes the learning rate and issues the update on the allocator's current stream; state() -> {name: momentum}."""

    def __init__(self, lr, momentum=0.9, wd=1e-5, rescale_grad=1.0, clip_gradient=35, lr_scheduler=None, lib=None, alloc=None):
        self.lr, self.momentum, self.wd, self.rescale_grad = float(lr), float(momentum), float(wd), float(rescale_grad)
        self.clip_gradient = -1.0 if clip_gradient is None else float(clip_gradient)
        self.lr_scheduler = lr_scheduler
        self.L = lib or rdlib.get_lib()
        if alloc is None:
            from .runtime import TorchAllocator
            alloc = TorchAllocator()
        self.A = alloc
        self.num_update = 0
        self.table_builds = 0           # how often step() has built and uploaded the table
        self._entries = {}              # name -> dict, in registration order
        self._dtype = None
        self._key = self._host = self._dev = None

    def add(self, name, weight, grad, pack=None, lr_mult=1.0, wd_mult=None):
        """weight, grad: float32 device tensors of one shape, 16-byte aligned.  pack, for a (cout, cin, 3, 3) or (cout, cin, 1, 1) conv weight
        with 64 or 128 channels on either side: dict(fwd=, bwd=, fold_scale=, dtype=) -- the device buffers of the forward image (with an optional
        device vector of cout scales folded in) and of the data-gradient image, either may be None; both are rewritten by every step.  With
        stride_w=2 in the dict (a (C, C, 3, 3) weight) they are the images of the stride-(1,2) launches (rd_sgd_tensor_t.stride_w).  wd_mult
        None: 1 for names ending in _weight or _gamma, else 0.  Registering a name again replaces its buffers and keeps its momentum.
        pack = dict(deconv=(KW, stride, pad), fwd=, bwd=, dtype=[, phase_bytes=]) on a (Cin, Cout, 3, KW) transposed-conv weight: the table
        updates the master as a plain tensor without images, and step() then issues one rd_pack_deconv_dev launch per named image on the
        same stream -- fwd, the `stride` phase images rd_deconv2d_bn_act_all reads (phase_bytes apart; default: packed back to back), and
        bwd, the image of the data gradient.  Nothing synchronises.
        The convs that read the range image follow the same precedent -- a plain tensor of the table, then one packer launch per image:
        pack = dict(narrow=ksize, fwd=, dtype=[, fold_scale=]) on a (cout, cin, k, k) weight with cin <= 16 (rd_pack_conv_narrow_dev; the 1x1
        image takes no fold scale), and pack = dict(cat=(cin1, cin2), fwd=, bwd=, dtype=[, fold_scale=]) on the (cout, 64 + cin2, 3, 3)
        concat weight (rd_pack_conv3x3_cat_dev: fwd the concat forward image, bwd the data-gradient image towards x1).
        The Meta-Kernel unit likewise: pack = dict(meta=dict(w0=, b0=, w1=, b1=, agg=), fwd=, bwd=, dtype=) on ONE of its five masters (each
        of them a plain tensor of the table, registered on its own) -- step() issues one rd_pack_meta_dev from the five updated masters into
        the unit's forward and backward blocks."""
        _check_f32(weight, name)
        _check_f32(grad, name + " gradient")
        n = _numel(weight)
        if n <= 0 or _numel(grad) != n:
            raise ValueError("%s: %d weight and %d gradient elements (equal, at least one)" % (name, n, _numel(grad)))
        e = dict(weight=weight, grad=grad, n=n, shape=tuple(int(v) for v in weight.shape), lr_mult=float(lr_mult),
                 wd_mult=default_wd_mult(name) if wd_mult is None else float(wd_mult), cout=0, cin=0, fwd=None, bwd=None, fold=None, stride_w=0)
        if pack is not None and pack.get("deconv") is not None:
            # a transposed-conv master (Cin, Cout, 3, KW): a plain n-element tensor of the table; step() re-packs its images afterwards
            shp = e["shape"]
            kw, s, p = (int(v) for v in pack["deconv"])
            if len(shp) != 4 or shp[2:] != (3, kw) or (kw, s, p) not in ((4, 2, 1), (8, 4, 2)):
                raise NotImplementedError("%s: deconv=%r images of a %r weight -- a (Cin, Cout, 3, KW) transposed-conv weight of the forms "
                                          "(KW, stride, pad) = (4, 2, 1) or (8, 4, 2)" % (name, tuple(pack["deconv"]), shp))
            dt = pack.get("dtype", rdlib.RD_BF16)
            if dt not in rdlib.H16 or self._dtype not in (None, dt):
                raise ValueError("%s: image type %r; one 16-bit type (RD_BF16 / RD_F16) per optimizer" % (name, dt))
            phase_bytes = int(pack.get("phase_bytes") or self.L.cdll.rd_conv_packed_bytes(6, shp[0], shp[1], dt))
            e["deconv"] = dict(form=(shp[0], shp[1], kw, s, p), fwd=pack.get("fwd"), bwd=pack.get("bwd"), phase_bytes=phase_bytes, dtype=dt)
            for k in ("fwd", "bwd"):
                if e["deconv"][k] is not None and rdlib.ptr(e["deconv"][k]) % 16:
                    raise ValueError("%s: %s buffer at %#x is not 16-byte aligned" % (name, k, rdlib.ptr(e["deconv"][k])))
        elif pack is not None and pack.get("meta") is not None:
            # the Meta-Kernel unit: its five masters are plain tensors of the table; the entry that carries this request (one of the five)
            # names them all, and step() re-packs the unit's two blocks from them with one rd_pack_meta_dev launch
            m = pack["meta"]
            dt = pack.get("dtype", rdlib.RD_BF16)
            if dt not in rdlib.H16 or self._dtype not in (None, dt):
                raise ValueError("%s: image type %r; one 16-bit type (RD_BF16 / RD_F16) per optimizer" % (name, dt))
            want = dict(w0=32 * 3, b0=32, w1=64 * 32, b1=64, agg=64 * 576)
            if set(m) != set(want) or any(_numel(m[k]) != n_k for k, n_k in want.items()):
                raise ValueError("%s: meta= names the five float32 masters w0 (32, 3), b0 (32), w1 (64, 32), b1 (64), agg (64, 576)" % name)
            if pack.get("fwd") is None or pack.get("bwd") is None:
                raise ValueError("%s: the Meta-Kernel unit's re-pack writes both blocks: fwd= and bwd=" % name)
            for k, v in m.items():
                _check_f32(v, "%s: master %s" % (name, k))
            e["repack"] = dict(kind="meta", masters=dict(m), fwd=pack["fwd"], bwd=pack["bwd"], fold=None, dtype=dt)
            for k in ("fwd", "bwd"):
                if rdlib.ptr(e["repack"][k]) % 16:
                    raise ValueError("%s: %s buffer at %#x is not aligned" % (name, k, rdlib.ptr(e["repack"][k])))
        elif pack is not None and (pack.get("narrow") is not None or pack.get("cat") is not None):
            # the convs that read the range image: plain n-element tensors of the table; step() re-packs their images afterwards
            shp = e["shape"]
            dt = pack.get("dtype", rdlib.RD_BF16)
            if dt not in rdlib.H16 or self._dtype not in (None, dt):
                raise ValueError("%s: image type %r; one 16-bit type (RD_BF16 / RD_F16) per optimizer" % (name, dt))
            if pack.get("narrow") is not None:
                k = int(pack["narrow"])
                if k not in (1, 3) or len(shp) != 4 or shp[2:] != (k, k) or shp[0] not in (64, 128) or not 1 <= shp[1] <= 16:
                    raise NotImplementedError("%s: narrow=%r images of a %r weight -- a (cout, cin, k, k) weight with k 1 or 3, cin 1 .. 16, cout "
                                              "64 or 128" % (name, pack["narrow"], shp))
                if pack.get("bwd") is not None or (k == 1 and pack.get("fold_scale") is not None):
                    raise ValueError("%s: a narrow conv has no data-gradient image, and its 1x1 image takes no fold scale" % name)
                e["repack"] = dict(kind="narrow", form=(shp[0], shp[1], k), fwd=pack.get("fwd"), bwd=None, fold=pack.get("fold_scale"), dtype=dt)
            else:
                cin1, cin2 = (int(v) for v in pack["cat"])
                if len(shp) != 4 or shp[2:] != (3, 3) or shp[0] not in (64, 128) or cin1 != 64 or cin2 not in (8, 16) or shp[1] != cin1 + cin2:
                    raise NotImplementedError("%s: cat=%r images of a %r weight -- a (cout, 64 + cin2, 3, 3) weight with cin2 8 or 16, cout 64 or "
                                              "128" % (name, tuple(pack["cat"]), shp))
                e["repack"] = dict(kind="cat", form=(shp[0], cin1, cin2), fwd=pack.get("fwd"), bwd=pack.get("bwd"), fold=pack.get("fold_scale"), dtype=dt)
            for k in ("fwd", "bwd", "fold"):
                if e["repack"][k] is not None and rdlib.ptr(e["repack"][k]) % (4 if k == "fold" else 16):
                    raise ValueError("%s: %s buffer at %#x is not aligned" % (name, k, rdlib.ptr(e["repack"][k])))
        elif pack is not None:
            shp = e["shape"]
            if len(shp) != 4 or shp[2:] not in ((3, 3), (1, 1)) or shp[0] not in (64, 128) or shp[1] not in (64, 128):
                raise NotImplementedError("%s: weight images of shape %r -- a (cout, cin, 3, 3) or (cout, cin, 1, 1) conv weight with 64 or 128 "
                                          "channels on either side (not the <= 16-channel body form, the stride-2 pair view, M16 images or the "
                                          "72-channel concat)" % (name, shp))
            dt = pack.get("dtype", rdlib.RD_BF16)
            if dt not in rdlib.H16 or self._dtype not in (None, dt):
                raise ValueError("%s: image type %r; one 16-bit type (RD_BF16 / RD_F16) per optimizer" % (name, dt))
            e.update(cout=shp[0], cin=shp[1], fwd=pack.get("fwd"), bwd=pack.get("bwd"), fold=pack.get("fold_scale"), stride_w=int(pack.get("stride_w", 0)))
            if e["stride_w"] not in (0, 1, 2) or (e["stride_w"] == 2 and (shp[2:] != (3, 3) or shp[0] != shp[1])):
                raise NotImplementedError("%s: stride_w %r images of a %r weight -- 0 / 1, or 2 for a (C, C, 3, 3) weight" % (name, pack.get("stride_w"), shp))
            if e["fold"] is not None and e["fwd"] is None:
                raise ValueError("%s: a fold scale without a forward image" % name)
        for k in ("weight", "grad", "fwd", "bwd"):
            if e[k] is not None and rdlib.ptr(e[k]) % 16:
                raise ValueError("%s: %s buffer at %#x is not 16-byte aligned" % (name, k, rdlib.ptr(e[k])))
        old = self._entries.get(name)
        if old is not None and old["n"] != n:
            raise ValueError("%s: registered with %d elements before, now %d" % (name, old["n"], n))
        e["mom"] = old["mom"] if old is not None else self.A.alloc(n * 4, zero=True)
        if pack is not None:
            self._dtype = pack.get("dtype", rdlib.RD_BF16)
        self._entries[name] = e

    def attach(self, tower):
        """every parameter tower.optimizer_entries() yields (rangedet_amd.backward.HeadTowerTrain / HeadTowerBackward)"""
        for kw in tower.optimizer_entries():
            self.add(**kw)

    def state(self):
        return {name: self.A.view_f32(e["mom"], e["shape"]) for name, e in self._entries.items()}

    def _pointers(self):
        return tuple(tuple(None if e[k] is None else rdlib.ptr(e[k]) for k in ("weight", "grad", "mom", "fwd", "bwd", "fold"))
                     for e in self._entries.values())

    def _build(self, key):
        ts = [rdlib.SgdTensor(p[0], p[1], p[2], e["n"], e["lr_mult"], e["wd_mult"], e["cout"], e["cin"], p[3], p[4], p[5], e["stride_w"])
              for e, p in zip(self._entries.values(), key)]
        self._host = self.L.sgd_table(ts, rdlib.RD_BF16 if self._dtype is None else self._dtype)
        self._dev = self.A.upload(self._host)
        self._key = key
        self.table_builds += 1

    def step(self):
        if not self._entries:
            raise RuntimeError("step: no tensor registered")
        key = self._pointers()
        if key != self._key:
            self._build(key)
        self.num_update += 1
        lr = self.lr if self.lr_scheduler is None else float(self.lr_scheduler(self.num_update))
        A = self.A
        stream = A.stream_ptr(None) if hasattr(A, "stream_ptr") else A.stream
        self.L.call("rd_sgd_mom_update", A.ptr(self._dev), self._host.ctypes.data, lr, self.momentum, self.wd, self.rescale_grad,
                    self.clip_gradient, stream)
        for e in self._entries.values():          # the transposed-conv images: one launch each, behind the update on the same stream
            d = e.get("deconv")
            if d is None:
                continue
            for key, data_grad in (("fwd", 0), ("bwd", 1)):
                if d[key] is not None:
                    self.L.call("rd_pack_deconv_dev", rdlib.ptr(e["weight"]), *d["form"], data_grad, d["phase_bytes"], d["dtype"],
                                rdlib.ptr(d[key]), stream)
        for e in self._entries.values():          # the narrow and the concat conv's images: one launch each, likewise
            r = e.get("repack")
            if r is None:
                continue
            fold = None if r["fold"] is None else rdlib.ptr(r["fold"])
            if r["kind"] == "meta":
                self.L.call("rd_pack_meta_dev", *[rdlib.ptr(r["masters"][k]) for k in ("w0", "b0", "w1", "b1", "agg")], rdlib.ptr(r["fwd"]),
                            rdlib.ptr(r["bwd"]), r["dtype"], stream)
                continue
            if r["kind"] == "narrow" and r["fwd"] is not None:
                self.L.call("rd_pack_conv_narrow_dev", rdlib.ptr(e["weight"]), fold, *r["form"], r["dtype"], rdlib.ptr(r["fwd"]), stream)
            if r["kind"] == "cat":
                for key, data_grad in (("fwd", 0), ("bwd", 1)):
                    if r[key] is not None:
                        self.L.call("rd_pack_conv3x3_cat_dev", rdlib.ptr(e["weight"]), None if data_grad else fold, *r["form"], data_grad,
                                    r["dtype"], rdlib.ptr(r[key]), stream)
        return lr

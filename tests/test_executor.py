"""The executor's host logic (rangedet_amd.runtime): which tensors a plan step holds and how long their buffers live, the library calls a
plan is bound to (entry points, argument counts), what stays open until forward() -- on host memory with the calls recorded instead of
launched (emu_util.RecordingLib) -- and, in both tiers, that replaying a plan step by step gives what the whole forward gives."""
import ctypes
from collections import Counter

import numpy as np
import pytest

from conftest import BOTH
from emu_util import NumpyAllocator, RecordingLib, emu_lib, small_shapes
from oracle import graph_ref as G
from oracle import input_ref as IR
from rangedet_amd import lib as R
from rangedet_amd import synth
from rangedet_amd.config import rangedet_veh_wo_aug_4_18e as cfgmod
from rangedet_amd.lower import FlatRef, TRef, lower, step_refs
from rangedet_amd.runtime import Executor

H, W = 8, 32          # the full-depth graph at the smallest field the three strides allow
DTYPES = {"bf16": R.RD_BF16, "f16": R.RD_F16, "f32": R.RD_F32}
_BOUND = {}


class _Alloc(NumpyAllocator):
    def __init__(self):
        self.stream = None


def _bound(variant, dn):
    """(plan, executor, recording library) of the full-depth graph at 8 x 32, B = 1, bound once per session on host memory"""
    if (variant, dn) not in _BOUND:
        shapes = small_shapes(H, W)
        if variant == "kitti":
            cfg = cfgmod.get_config(False, variant="kitti", feat_size=(H, W), pad_field=(H, W), pre_nms_top_n={'veh': 120, 'ped': 40})
            shapes['input_data'] = (cfgmod.KITTI_INPUT_CHANNELS, H, W)
            P = synth.make_weights(seed=5, width=W, in_ch=cfgmod.KITTI_INPUT_CHANNELS, num_classes=2)
        else:
            cfg = cfgmod.get_config(False, feat_size=(H, W - 2), pad_field=(H, W), pre_nms_top_n={'veh': 150})
            P = synth.make_weights(seed=18, width=W)
        plan = lower(cfg[6].test_symbol, shapes, DTYPES[dn], 1)
        lib = RecordingLib(emu_lib())
        _BOUND[variant, dn] = (plan, Executor(plan, P, lib=lib, alloc=_Alloc()), lib)
    return _BOUND[variant, dn]


def _zero_inputs(plan):
    return {n: np.zeros((plan.batch,) + tuple(s), np.float32) for n, s in plan.input_vars.items() if s is not None}


def _scan(v, out):
    """brute force: every reference inside v, whatever holds it"""
    if isinstance(v, (TRef, FlatRef)):
        out.append(v)
        if isinstance(v, TRef) and v.tail is not None:
            _scan(v.tail, out)
    elif isinstance(v, dict):
        for x in v.values():
            _scan(x, out)
    elif isinstance(v, (list, tuple)):
        for x in v:
            _scan(x, out)


@pytest.mark.parametrize("variant,dn", [("veh", "bf16"), ("veh", "f32"), ("kitti", "bf16")])
def test_step_refs_finds_every_reference_and_shared_buffers_never_overlap(variant, dn):
    """lower.step_refs against a recursive scan written here, and the outcome of Executor._assign_buffers: two logical buffers on one
    allocation are never live at the same step.  Live = from the first to the last step that holds a reference to the buffer at any depth
    (a graph output: to the end); a buffer the plan no longer has (the tensor inside a fused block) is nobody's."""
    plan, ex, _ = _bound(variant, dn)
    first, last = {}, {}
    nested = 0
    for i, st in enumerate(plan.steps):
        want = []
        _scan(st, want)
        got = list(step_refs(st))
        assert sorted(map(id, want)) == sorted(id(v) for _, v in got), (i, st["kind"])
        assert len({p for p, _ in got}) == len(got), "key paths are unique within a step"
        for p, v in got:
            q = st
            for k in p.split("."):
                q = getattr(q, k) if isinstance(q, TRef) else q[int(k) if isinstance(q, (list, tuple)) else k]
            assert q is v, (i, p)
        nested += sum("." in p for p, _ in got)
        for v in want:
            if v.buf in plan.buffers:
                first.setdefault(v.buf, i)
                last[v.buf] = i
    assert nested > 0 or dn == "f32", "the 16-bit graphs have references below the top level of a step (blocks, fused output convs, x.tail)"
    for kind, v in plan.outputs:
        if kind in ("flat", "flat_i32"):
            last[v.buf] = len(plan.steps) + 1
    assert set(ex._phys) == set(plan.buffers)
    share = {}
    for b, t in ex._phys.items():
        share.setdefault(id(t), []).append(b)
    groups = [bs for bs in share.values() if len(bs) > 1]
    assert groups, "no buffer is reused: the test would pass vacuously"
    for bs in groups:
        for a in bs:
            for b in bs:
                if a < b and a in first and b in first:
                    assert last[a] < first[b] or last[b] < first[a], (a, (first[a], last[a]), b, (first[b], last[b]))


_CALLS_16 = {"rd_conv3x3_bn_act_ex": 49, "rd_block64_m16_bn_act": 7, "rd_block64_bn_act": 1, "rd_conv2d_bn_act_head_out": 6, "rd_conv3x3_bn_act_cat": 2,
             "rd_deconv2d_bn_act_all": 3, "rd_deconv2d_bn_act_pairs": 1, "rd_meta_kernel_fwd": 1, "rd_nchw_to_nhwc": 1, "rd_copy_rows": 6,
             "rd_sorted_foreground": 1, "rd_decode3d_bbox": 1}
_CALLS_32 = {"rd_conv2d_bn_act": 82, "rd_deconv2d_bn_act": 12, "rd_head_out": 6, "rd_nchw_to_nhwc": 2, "rd_meta_kernel_fwd": 1, "rd_copy_rows": 6,
             "rd_sorted_foreground": 1, "rd_decode3d_bbox": 1}
# two classes: the tower outputs are read by two output convs each, so those stay separate launches
_KITTI_16 = {"rd_conv3x3_bn_act_ex": 55, "rd_block64_m16_bn_act": 7, "rd_block64_bn_act": 1, "rd_head_out": 12, "rd_conv3x3_bn_act_cat": 2,
             "rd_deconv2d_bn_act_all": 3, "rd_deconv2d_bn_act_pairs": 1, "rd_meta_kernel_fwd": 1, "rd_nchw_to_nhwc": 1, "rd_copy_rows": 12,
             "rd_sorted_foreground": 2, "rd_decode3d_bbox": 2}
_KITTI_32 = {"rd_conv2d_bn_act": 82, "rd_deconv2d_bn_act": 12, "rd_head_out": 12, "rd_nchw_to_nhwc": 2, "rd_meta_kernel_fwd": 1, "rd_copy_rows": 12,
             "rd_sorted_foreground": 2, "rd_decode3d_bbox": 2}
_EXPECTED = {("veh", "bf16"): (75, _CALLS_16), ("veh", "f16"): (75, _CALLS_16), ("veh", "f32"): (99, _CALLS_32),
             ("kitti", "bf16"): (91, _KITTI_16), ("kitti", "f16"): (91, _KITTI_16), ("kitti", "f32"): (109, _KITTI_32)}


@pytest.mark.parametrize("variant,dn", sorted(_EXPECTED))
def test_bound_calls_arity_and_entry_points(variant, dn):
    """Every call of one forward carries as many arguments as lib.SIGNATURES declares for its entry, and the entries are those the plan's
    launch forms stand for (79 calls in 75 steps in the 16-bit types, 111 in 99 in fp32; the two-class graph: 99 in 91, 125 in 109)."""
    plan, ex, lib = _bound(variant, dn)
    del lib.calls[:]
    ex.forward(_zero_inputs(plan))
    for name, args in lib.calls:
        assert len(args) == len(R.SIGNATURES[name][1]), (name, len(args))
    nsteps, want = _EXPECTED[variant, dn]
    assert len(plan.steps) == nsteps
    assert Counter(name for name, _ in lib.calls) == Counter(want)


def test_malformed_call_fails_in_the_constructor():
    """a binder that yields a call with an argument missing: the executor refuses it when it is built, without a device"""
    plan, ex, lib = _bound("veh", "f32")

    class Broken(Executor):
        _BINDERS = dict(Executor._BINDERS, decode=lambda self, st, P: [("rd_decode3d_bbox", 0, 0, 0)])
    with pytest.raises(TypeError, match="rd_decode3d_bbox bound with 3 arguments before the stream, the library takes 7"):
        Broken(plan, synth.make_weights(seed=18, width=W), lib=lib, alloc=_Alloc())
    with pytest.raises(RuntimeError, match="unknown plan step 'nope'"):
        ex._bind(dict(kind="nope"), {})


def test_stream_is_read_at_every_forward():
    """Pipelines run forward() under another current stream and graph capture on a capture stream: the stream is no part of the binding."""
    plan, ex, lib = _bound("veh", "bf16")
    fr = _zero_inputs(plan)
    try:
        for stream in (0x1111, 0x2222):
            ex.alloc.stream = stream
            del lib.calls[:]
            ex.forward(fr)
            assert len(lib.calls) == 79
            for name, args in lib.calls:
                assert R.SIGNATURES[name][1][-1] is ctypes.c_void_p and args[-1] == stream, (name, args[-1])
                assert stream not in args[:-1]
        del lib.calls[:]
        ex.forward(fr, only=3, dev={})
        assert lib.calls and all(args[-1] == 0x2222 for _, args in lib.calls)
    finally:
        ex.alloc.stream = None


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_stepwise_replay_equals_whole_forward(be):
    """forward(fr), then forward(fr, only=i, dev=dev) for every step in order on the same executor (every plan buffer cleared in between, so
    a step that did not run leaves a hole): the inputs and outputs of get_sorted_foreground and the graph outputs, bit for bit.  bf16; emu:
    the depth-reduced graph of test_e2e_small_f32 at 8 x 30 (pad 32), k = 150, B = 1; hip: the full graph at 16 x 250 (pad 256), k = 2000,
    B = 2 (the batch strides of rd_copy_rows and of the flat head outputs count from the second frame on)."""
    emu = be.name == "emu"
    Hh, Wr, Wp, k, B = (8, 30, 32, 150, 1) if emu else (16, 250, 256, 2000, 2)
    cfg = cfgmod.get_config(False, feat_size=(Hh, Wr), pad_field=(Hh, Wp), pre_nms_top_n={'veh': k}, batch_image=B)
    sym = cfg[6].test_symbol
    if emu:     # the reduced depth through the same builders
        from rangedet_amd.symbol.backbone.dla_backbone import DLABackbone
        from rangedet_amd.symbol.head.builder import RangeRCNN, RangeRpnHead
        RP = cfg[2]
        mk = dict(stride=1, meta_func_param='meta_baseline_bias', data_channels=64, coord_channels=3, channel_list=[32, 64], kernel_size=3)
        bp = type("BackboneParam", (), dict(fp16=True, normalizer=RP.normalizer, fpn_strides=(1, 2, 4), batch_image=1, range_image_shape_hw=(Hh, Wp),
                                            add_data_sc=True, num_block=dict({kk: 1 for kk in G.Cfg.num_block}, res1=2),
                                            num_filter=G.Cfg.num_filter, meta_kernel_units={'res1_unit2': mk}))
        RP.head.cls_conv_layers = RP.head.reg_conv_layers = 1
        dp = type("DetParam", (), dict(fpn_strides=(1, 2, 4), class_names=('veh',)))
        sym = RangeRCNN(dp).get_test_symbol(DLABackbone(bp), RangeRpnHead(RP))
    plan = lower(sym, small_shapes(Hh, Wp), R.RD_BF16, B)
    P = synth.make_weights(seed=18, width=Wp, cls_bias=-0.5)
    fr = IR.make_frame(0, W=Wr, pad_W=Wp, H=Hh) if B == 1 else IR.make_batch([0, 1], W=Wr, pad_W=Wp, H=Hh)
    ex = Executor(plan, P, lib=be.lib, alloc=be.alloc)
    sfg = [s for s in plan.steps if s["kind"] == "sorted_fg"][0]
    keys = ("score", "delta", "pc", "mask", "out_score", "out_delta", "out_pc")
    flat = [v for kind, v in plan.outputs if kind == "flat"]
    assert len(flat) == 2

    def snapshot():
        return [ex.read_flat(sfg[n]).view(np.uint32) for n in keys] + [ex.read_flat(v).view(np.uint32) for v in flat]
    outs = ex.forward(fr)
    whole = snapshot()
    assert np.array_equal(np.array(be.alloc.to_numpy(outs[1])).view(np.uint32), whole[-2])
    for t in {id(t): t for t in ex._phys.values()}.values():
        t[...] = 0
    assert not snapshot()[4].any()
    dev = {}
    for i in range(len(plan.steps)):
        assert ex.forward(fr, only=i, dev=dev) is None
    assert sorted(dev) == sorted(n for n, s in plan.input_vars.items() if s is not None)
    for n, a, b in zip(keys + ("fg_cls_score", "decoded_bbox"), whole, snapshot()):
        assert a.any() and np.array_equal(a, b), n
    if B > 1:
        assert not np.array_equal(whole[4][0], whole[4][1]), "the two frames differ"

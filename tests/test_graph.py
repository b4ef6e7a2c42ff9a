"""Host logic: the mirrored symbol API, lowering of the reference's test graph, and end-to-end parity of the lowered
plan against the graph oracle (oracle/graph_ref.py: PyTorch-CPU fp32 restatement, parity unpinned for MXNet op semantics)."""
import inspect
from collections import Counter

import numpy as np
import pytest

from conftest import BOTH, HIP_ONLY
from emu_util import small_shapes
from oracle import cpu_ops as O
from oracle import graph_ref as G
from oracle import input_ref as IR
from rangedet_amd import lib as R
from rangedet_amd import mx, synth
from rangedet_amd.config import rangedet_veh_wo_aug_4_18e as cfgmod
from rangedet_amd.lower import conv_steps, lower
from rangedet_amd.runtime import Executor


def test_config_and_full_graph_lowering(monkeypatch):
    cfg = cfgmod.get_config(False)
    assert len(cfg) == 14
    General, _, RpnParam, _, _, _, ModelParam, _, TestParam = cfg[:9]
    assert General.pad_field == (64, 2656) and RpnParam.all_proposal.rpn_pre_nms_top_n['veh'] == 50000
    assert TestParam.nms.thr_lo == 0.1 and TestParam.nms.thr_hi == 0.5 and TestParam.min_score['veh'] == 0.5
    sym = ModelParam.test_symbol
    args = sym.list_arguments()
    for n in ("input_data", "coord_s1", "res1_unit2_2656_mlp0_weight", "res1_unit2point_wise_mlp_bn1_gamma",
              "res1_unit2aggregation_conv1_weight", "agg2_deconv_weight", "rpn_cls_conv_3_lvl_2_weight",
              "rpn_reg_delta_lvl_0_bias", "pc_vehicle_frame_s4", "range_image_mask_s1"):
        assert n in args, n
    P = synth.make_weights()
    missing = [a for a in args if a not in P and not a.startswith(("input_data", "coord_", "pc_", "range_", "rec_id", "gt_"))]
    assert not missing, missing[:5]
    plan = lower(sym, small_shapes(64, 2656), R.RD_BF16, 1)
    kinds = Counter(s["kind"] for s in plan.steps)
    # 63 backbone conv/deconv - 4 deconv - 1 aggregation conv (inside the fused Meta unit) + 24 head tower convs
    # bf16: the six 1x1 output convs ride in the epilogue of their tower's last conv (lower._fuse_head_out) and the nine
    # 1x1 projection shortcuts in the epilogue of their block's second conv (lower._fusable_projection)
    # round 5: the seven 64-channel stride-1 BasicBlocks whose intermediate tensor has one reader are ONE launch each (lower._fuse_blocks,
    # rd_block64_bn_act), the network's first block (8 -> 64 -> 64) included: 73 convs = 57 launches + 8 blocks of two
    assert kinds["conv"] == 57 and kinds["block"] == 8 and kinds["deconv"] == 4 and kinds["meta"] == 1 and kinds["head_out"] == 0
    assert [s["name"] for s in plan.steps if s["kind"] == "block"] == [n + "_conv1 + " + n + "_conv2" for n in (
        "res1_unit1", "res2a_unit2", "res2a_unit3", "agg2a_res_unit1", "agg1_res_unit1", "agg1_res_unit2", "agg3_res_unit1", "agg3_res_unit2")]
    assert [bool(s["b"].get("sc")) for s in plan.steps if s["kind"] == "block"] == [True, False, False, True, True, False, True, False]
    inter = {s["a"]["out"].buf for s in plan.steps if s["kind"] == "block"}
    assert not inter & set(plan.buffers), "the intermediate tensor of a fused block has no buffer"
    monkeypatch.setenv("RD_DEV_SWITCHES", "1")      # (lowering A/B switches are honoured only with this set, rangedet_amd/devswitch.py)
    monkeypatch.setenv("RD_NO_FUSE_BLOCK", "1")
    assert Counter(s["kind"] for s in lower(sym, small_shapes(64, 2656), R.RD_BF16, 1).steps)["conv"] == 73
    monkeypatch.delenv("RD_NO_FUSE_BLOCK")
    convs = [s for s, _ in conv_steps(plan.steps) if s["kind"] == "conv"]
    assert len(convs) == 73
    # (launch counts: a transposed conv is ONE launch -- all its phases, rd_deconv2d_bn_act_all)
    assert sum(n for _, n in conv_steps(plan.steps)) == 57 + 8 + 4
    assert all(s["one_launch"] for s in plan.steps if s["kind"] == "deconv")
    scs = [s for s, _ in conv_steps(plan.steps) if s.get("sc")]
    assert sorted(s["sc"]["name"] for s in scs) == sorted(n + "_unit1_sc" for n in (
        "res1", "res2a", "res2", "res3a", "res3", "agg2_res", "agg2a_res", "agg1_res", "agg3_res"))
    assert sorted(s["name"] for s, _ in conv_steps(plan.steps) if s["kind"] == "conv" and s["stride_w"] == 2) == \
        ["res2_unit1_conv2", "res2a_unit1_conv2", "res3_unit1_conv2", "res3a_unit1_conv2"]
    assert all(s["ex"] for s in plan.steps if s["kind"] == "conv" and s["stride_w"] == 2)
    f32_kinds = Counter(s["kind"] for s in lower(sym, small_shapes(64, 2656), R.RD_F32, 1).steps)
    assert f32_kinds["conv"] == 82                                  # fp32 parity mode: every conv is its own launch
    fused = [s for s in convs if s.get("head")]
    assert sorted(s["name"] for s in fused) == sorted("rpn_%s_conv_3_lvl_%d" % (t, l) for t in ("cls", "reg") for l in range(3))
    assert sorted(s["head"]["nout"] for s in fused) == [1, 1, 1, 8, 8, 8]
    assert Counter(s["kind"] for s in lower(sym, small_shapes(64, 2656), R.RD_F32, 1).steps)["head_out"] == 6   # fp32: separate
    assert kinds["sorted_fg"] == 1 and kinds["decode"] == 1
    assert [o[0] for o in plan.outputs] == ["input", "flat", "flat", "zeros", "input", "input"]
    assert plan.outputs[1][1].shape == (50000,) and plan.outputs[2][1].shape == (50000, 10)
    macs = 0
    for s in convs:
        if s["kind"] == "conv":
            macs += s["out"].H * s["out"].W * s["cin"] * s["cout"] * s["k"][0] * s["k"][1]
            if s.get("sc"):
                macs += s["out"].H * s["out"].W * s["sc"]["cin"] * s["cout"]
    assert abs(macs / 1e9 - (557.07 - 9.64 - 20.89 - 0.35)) < 1.0  # SURVEY appendix A minus meta unit, deconvs, head 1x1


def test_unsupported_widths_fail_at_lowering_with_the_supported_set():
    """The reference's config surface lets BackboneParam.num_filter / meta_kernel_units vary (dla_backbone.py:59-103,130-161).  The symbol
    mirror builds any of them; the HIP lowering is welded to the shipped widths and must say which ones instead of mis-computing."""
    # (widths up to 128 that are not 64 / 128 run zero-padded: test_e2e_other_stage_widths; beyond 128 there is no kernel)
    sym = cfgmod.get_config(False, backbone={'num_filter': {'res3a': 160}})[6].test_symbol
    with pytest.raises(NotImplementedError, match=r"160 output channels.*64 and 128"):
        lower(sym, small_shapes(64, 2656), R.RD_BF16, 1)
    mk = dict(stride=1, meta_func_param='meta_baseline_bias', data_channels=64, coord_channels=3, channel_list=[16, 64], kernel_size=3)
    sym = cfgmod.get_config(False, backbone={'meta_kernel_units': {'res1_unit2': mk}})[6].test_symbol
    with pytest.raises(NotImplementedError, match=r"MLP 16 -> 64.*3 -> 32 -> 64"):
        lower(sym, small_shapes(64, 2656), R.RD_BF16, 1)
    # a virtual concat ([agg3 | range image], never written) handed to anything but a 3x3 stride-1 conv is refused, not half-read
    from rangedet_amd.lower import TRef, Lowering
    lw = Lowering.__new__(Lowering)
    from rangedet_amd.lower import Plan
    lw.plan = Plan(R.RD_BF16, 1)
    v = TRef(1, 64, 8, 32, 64, 0, None, TRef(2, 8, 8, 32, 16))
    with pytest.raises(NotImplementedError, match="virtual concat"):
        lw.step("deconv", name="d", x=v, out=TRef(3, 64, 8, 64, 64))
    with pytest.raises(NotImplementedError, match="virtual concat"):
        lw.step("conv", name="c", x=TRef(4, 64, 8, 32, 64), res=v, k=(3, 3), out=TRef(3, 64, 8, 32, 64))
    lw.step("conv", name="c", x=v, x2=v.tail, k=(3, 3), out=TRef(3, 128, 8, 32, 128))


def test_api_surface_matches_reference():
    from rangedet_amd.symbol.backbone.meta_kernel import MetaKernel
    from rangedet_amd.symbol.backbone.dla_backbone import DLABackbone, DLABackboneBuilder
    from rangedet_amd.symbol.head.builder import RangeRCNN, RangeRpnHead
    assert list(inspect.signature(MetaKernel.__init__).parameters) == ["self", "num_batch", "feat_height", "feat_width", "fp16", "num_frame"]
    assert list(inspect.signature(MetaKernel.meta_baseline_bias).parameters)[:9] == [
        "self", "name", "data", "coord_data", "data_channels", "coord_channels", "channel_list", "norm", "conv1_filter"]
    for m in ("sampler_im2col", "sample_data", "sample_coord", "relative_coord", "mlp"):
        assert hasattr(MetaKernel, m)
    for m in ("basicblock", "meta_kernel_conv", "res_stage", "agg_stage", "backbone_factory", "get_backbone"):
        assert hasattr(DLABackboneBuilder, m)
    assert hasattr(DLABackbone, "get_rpn_feature") and hasattr(RangeRCNN, "get_test_symbol")
    for m in ("get_fpn_output", "sep_level_type", "get_fpn_prediction", "get_prediction_of_one_type"):
        assert hasattr(RangeRpnHead, m)
    assert list(inspect.signature(RangeRpnHead.get_prediction_of_one_type).parameters) == [
        "self", "cls_score", "bbox_delta", "pc_vehicle_frame", "mask", "nms_thr", "pre_nms_top_n", "post_nms_top_n"]
    keep_inds, final = mx.contrib.NMS3D(mx.var("b"), 0.2, 200)        # nms_3d.cc:22-68: (idx, bbox_after_nms)
    assert keep_inds.op == "NMS3D" and (keep_inds.index, final.index) == (0, 1) and final.attrs["max_keep"] == 200
    with pytest.raises(NotImplementedError):
        mx.sym.ROIAlign
    from rangedet_amd import compat
    names = compat.install_aliases()
    import mxnext.complicate
    import rangedet.symbol.head.builder as b2
    assert b2.RangeRCNN is RangeRCNN and callable(mxnext.complicate.normalizer_factory) and "processing_cxx" in names


@pytest.mark.parametrize("be", BOTH, indirect=True)
@pytest.mark.parametrize("dt", [R.RD_F32, R.RD_BF16], ids=["f32", "bf16"])
def test_e2e_other_stage_widths(be, dt):
    """BackboneParam.num_filter other than the shipped 64 / 128 (the reference's config surface lets it vary, dla_backbone.py:59-103,
    130-161): a stage of 96 or 48 channels runs zero-padded on the 128- / 64-channel kernels (lower._conv_bn, runtime.pad_rows) and the
    consumers read its logical channels.  Widths consistent the way the reference graph needs them (a skip connection adds the stages
    agg2 = res2, agg2a = res2a): res2 = agg2 = 96, res3a = 96, res3 = 112, res2a = agg2a = 48 -- so every kind of consumer meets a padded
    tensor: 3x3 convs stride 1 / 2, projection shortcuts, residual adds, transposed convs (input AND output), head tower convs.
    fp32: against the graph oracle at the parity tolerance; bf16: the same graph within the 16-bit error model."""
    emu = be.name == "emu"
    H, Wr, W, k = (8, 30, 32, 150) if emu else (16, 250, 256, 2000)
    nf = dict(G.Cfg.num_filter, res2a=48, agg2a=48, res2=96, agg2=96, res3a=96, res3=112)

    class Cfg(G.Cfg):
        num_filter = nf
        num_block = dict({kk: 1 for kk in G.Cfg.num_block}, res1=2, res2=2, res2a=2)
        head_layers = 1
    cfg = cfgmod.get_config(False, feat_size=(H, Wr), pad_field=(H, W), pre_nms_top_n={'veh': k})
    from rangedet_amd.symbol.backbone.dla_backbone import DLABackbone
    from rangedet_amd.symbol.head.builder import RangeRCNN, RangeRpnHead
    RP = cfg[2]
    bp = type("BackboneParam", (), dict(fp16=True, normalizer=RP.normalizer, fpn_strides=(1, 2, 4), batch_image=1, range_image_shape_hw=(H, W),
                                        add_data_sc=True, num_block=Cfg.num_block, num_filter=nf,
                                        meta_kernel_units={'res1_unit2': dict(stride=1, meta_func_param='meta_baseline_bias', data_channels=64,
                                                                              coord_channels=3, channel_list=[32, 64], kernel_size=3)}))
    RP.head.cls_conv_layers = RP.head.reg_conv_layers = 1
    dp = type("DetParam", (), dict(fpn_strides=(1, 2, 4), class_names=('veh',)))
    sym = RangeRCNN(dp).get_test_symbol(DLABackbone(bp), RangeRpnHead(RP))
    plan = lower(sym, small_shapes(H, W), dt, 1)
    padded = [s for s, _ in conv_steps(plan.steps) if s.get("cout_logical") not in (None, s["cout"])]
    assert {s["cout_logical"] for s in padded} == {48, 96, 112} and all(s["cout"] in (64, 128) and s["out"].cs == s["cout"] for s in padded)
    assert any(s["kind"] == "deconv" for s in padded) and any(s.get("sc") or tuple(s["k"]) == (1, 1) for s in padded) and \
        any(s["stride_w"] == 2 for s in padded if s["kind"] == "conv")
    P = synth.make_weights(seed=18, width=W, cls_bias=-0.5, num_filter=nf)
    fr = IR.make_frame(0, W=Wr, pad_W=W, H=H)
    ex = Executor(plan, P, lib=be.lib, alloc=be.alloc)
    ex.forward(fr)
    ref = G.forward(fr, P, cfg=Cfg, num_fgs=k)
    sfg = [s for s in plan.steps if s["kind"] == "sorted_fg"][0]
    logit, delta = ex.read_flat(sfg["score"]), ex.read_flat(sfg["delta"])
    if dt == R.RD_F32:
        assert np.abs(logit - ref["logit"]).max() < 1e-4, np.abs(logit - ref["logit"]).max()
        assert np.abs(delta - ref["delta"]).max() < 1e-4, np.abs(delta - ref["delta"]).max()
    else:
        for got, want in ((logit, ref["logit"]), (delta, ref["delta"])):
            err = (got - want)
            assert np.sqrt((err ** 2).mean()) < 0.03 * want.std() + 1e-3 and np.abs(err).max() < 0.25 * want.std() + 1e-2, (np.sqrt((err ** 2).mean()), want.std())


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_e2e_small_f32(be):
    """Lowered plan vs graph oracle in fp32 on a small frame: emu runs a depth-reduced graph (CPU emulation is slow),
    hip runs the full-depth graph."""
    emu = be.name == "emu"
    H, Wr, W, k = (8, 30, 32, 150) if emu else (16, 250, 256, 2000)

    class Cfg(G.Cfg):
        pass
    if emu:
        Cfg.num_block = dict({kk: 1 for kk in G.Cfg.num_block}, res1=2)
        Cfg.head_layers = 1
    cfg = cfgmod.get_config(False, feat_size=(H, Wr), pad_field=(H, W), pre_nms_top_n={'veh': k})
    if emu:
        # rebuild the symbol with the reduced depth through the same builders
        from rangedet_amd.symbol.backbone.dla_backbone import DLABackbone
        from rangedet_amd.symbol.head.builder import RangeRCNN, RangeRpnHead
        RP = cfg[2]
        bp = type("BackboneParam", (), dict(fp16=True, normalizer=RP.normalizer, fpn_strides=(1, 2, 4), batch_image=1,
                                            range_image_shape_hw=(H, W), add_data_sc=True, num_block=Cfg.num_block,
                                            num_filter=G.Cfg.num_filter,
                                            meta_kernel_units={'res1_unit2': dict(stride=1, meta_func_param='meta_baseline_bias',
                                                                                  data_channels=64, coord_channels=3,
                                                                                  channel_list=[32, 64], kernel_size=3)}))
        RP.head.cls_conv_layers = RP.head.reg_conv_layers = 1
        dp = type("DetParam", (), dict(fpn_strides=(1, 2, 4), class_names=('veh',)))
        sym = RangeRCNN(dp).get_test_symbol(DLABackbone(bp), RangeRpnHead(RP))
    else:
        sym = cfg[6].test_symbol
    plan = lower(sym, small_shapes(H, W), R.RD_F32, 1)
    P = synth.make_weights(seed=18, width=W, cls_bias=-0.5)
    fr = IR.make_frame(0, W=Wr, pad_W=W, H=H)
    ex = Executor(plan, P, lib=be.lib, alloc=be.alloc)
    outs = ex.forward(fr)
    ref = G.forward(fr, P, cfg=Cfg, num_fgs=k)
    sfg = [s for s in plan.steps if s["kind"] == "sorted_fg"][0]
    logit, delta = ex.read_flat(sfg["score"]), ex.read_flat(sfg["delta"])
    assert np.abs(logit - ref["logit"]).max() < 1e-4, np.abs(logit - ref["logit"]).max()
    assert np.abs(delta - ref["delta"]).max() < 1e-4, np.abs(delta - ref["delta"]).max()   # box regressions <= 1e-4 (fp32)
    be.alloc.sync()
    sc = np.array(be.alloc.to_numpy(outs[1]))
    bx = np.array(be.alloc.to_numpy(outs[2]))
    assert np.all(np.diff(sc[0]) <= 0)
    assert np.abs(sc - ref["fg_cls_score"]).max() < 1e-5
    gap = np.abs(np.diff(ref["fg_cls_score"][0]))
    ok = np.ones(k, bool)
    ok[1:] &= gap > 1e-5
    ok[:-1] &= gap > 1e-5
    ok &= ref["fg_cls_score"][0] > 1e-6
    assert ok.sum() > k // 10
    assert np.abs(bx[0][ok] - ref["decoded_bbox"][0][ok]).max() < 1e-3
    assert outs[0] is None and outs[3].shape == (1,)


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_e2e_nms3d_branch_f32(be):
    """RpnParam.wnms = False: get_prediction_of_one_type ends in contrib.NMS3D (builder.py:530-534) and the test symbol
    returns (score, bbox_after_nms, keep_inds) per class.  The lowered plan runs rd_nms3d on the decoded boxes; its outputs
    must equal the oracle's NMS3D applied to those same boxes, bit for bit."""
    emu = be.name == "emu"
    H, Wr, W, k = (8, 30, 32, 150) if emu else (16, 250, 256, 2000)
    cfg = cfgmod.get_config(False, feat_size=(H, Wr), pad_field=(H, W), pre_nms_top_n={'veh': k})
    from rangedet_amd.symbol.backbone.dla_backbone import DLABackbone
    from rangedet_amd.symbol.head.builder import RangeRCNN, RangeRpnHead
    RP = cfg[2]
    nb = dict({kk: 1 for kk in G.Cfg.num_block}, res1=2) if emu else G.Cfg.num_block
    bp = type("BackboneParam", (), dict(fp16=True, normalizer=RP.normalizer, fpn_strides=(1, 2, 4), batch_image=1,
                                        range_image_shape_hw=(H, W), add_data_sc=True, num_block=nb,
                                        num_filter=G.Cfg.num_filter,
                                        meta_kernel_units={'res1_unit2': dict(stride=1, meta_func_param='meta_baseline_bias',
                                                                              data_channels=64, coord_channels=3,
                                                                              channel_list=[32, 64], kernel_size=3)}))
    if emu:
        RP.head.cls_conv_layers = RP.head.reg_conv_layers = 1
    RP.wnms = False
    thr, mk = RP.all_proposal.nms_thr['veh'], RP.all_proposal.rpn_post_nms_top_n['veh']
    dp = type("DetParam", (), dict(fpn_strides=(1, 2, 4), class_names=('veh',)))
    sym = RangeRCNN(dp).get_test_symbol(DLABackbone(bp), RangeRpnHead(RP))
    plan = lower(sym, small_shapes(H, W), R.RD_F32, 1)
    st = [s for s in plan.steps if s["kind"] == "nms3d"]
    assert len(st) == 1 and st[0]["N"] == k and st[0]["max_keep"] == mk and abs(st[0]["thr"] - thr) < 1e-7
    P = synth.make_weights(seed=18, width=W, cls_bias=-0.5)
    fr = IR.make_frame(0, W=Wr, pad_W=W, H=H)
    ex = Executor(plan, P, lib=be.lib, alloc=be.alloc)
    outs = ex.forward(fr)
    be.alloc.sync()
    final, keep = np.array(be.alloc.to_numpy(outs[2])), np.array(be.alloc.to_numpy(outs[3]))
    assert final.shape == (1, mk, 10) and keep.shape == (1, mk) and keep.dtype == np.int32
    boxes = ex.read_flat(st[0]["boxes"])
    rk, ro = O.nms3d(boxes, thr, mk, False)
    assert np.array_equal(keep, rk)
    assert np.array_equal(final.view(np.uint32), ro.view(np.uint32))
    nk = int((keep[0] >= 0).sum())
    assert 0 < nk <= mk and np.all(np.diff(keep[0, :nk]) > 0)


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_e2e_kitti_two_class_f32(be):
    """BASELINE config 5 shape: 5-channel KITTI range image (range, x, y, z, intensity), mixed veh + ped head.  The same
    lowering serves it (per-class weight rows of the 1x1 output convs, per-class top-k); logits / deltas / sorted scores /
    boxes of BOTH classes against the graph oracle.  emu: depth-reduced graph, hip: full depth at 16 x 256."""
    emu = be.name == "emu"
    H, W = (8, 32) if emu else (16, 256)
    ks = {'veh': 120, 'ped': 40} if emu else {'veh': 1500, 'ped': 300}

    class Cfg(G.Cfg):
        num_classes = 2
        class_names = ('veh', 'ped')
    cfg = cfgmod.get_config(False, variant="kitti", feat_size=(H, W), pad_field=(H, W), pre_nms_top_n=ks)
    assert cfg[0].num_classes == 2 and cfg[0].class_names == ('veh', 'ped')
    if emu:
        Cfg.num_block = dict({kk: 1 for kk in G.Cfg.num_block}, res1=2)
        Cfg.head_layers = 1
        from rangedet_amd.symbol.backbone.dla_backbone import DLABackbone
        from rangedet_amd.symbol.head.builder import RangeRCNN, RangeRpnHead
        RP = cfg[2]
        bp = type("BackboneParam", (), dict(fp16=True, normalizer=RP.normalizer, fpn_strides=(1, 2, 4), batch_image=1,
                                            range_image_shape_hw=(H, W), add_data_sc=True, num_block=Cfg.num_block,
                                            num_filter=G.Cfg.num_filter,
                                            meta_kernel_units={'res1_unit2': dict(stride=1, meta_func_param='meta_baseline_bias',
                                                                                  data_channels=64, coord_channels=3,
                                                                                  channel_list=[32, 64], kernel_size=3)}))
        RP.head.cls_conv_layers = RP.head.reg_conv_layers = 1
        dp = type("DetParam", (), dict(fpn_strides=(1, 2, 4), class_names=('veh', 'ped')))
        sym = RangeRCNN(dp).get_test_symbol(DLABackbone(bp), RangeRpnHead(RP))
    else:
        sym = cfg[6].test_symbol
    shapes = small_shapes(H, W)
    shapes['input_data'] = (cfgmod.KITTI_INPUT_CHANNELS, H, W)
    plan = lower(sym, shapes, R.RD_F32, 1)
    P = synth.make_weights(seed=5, width=W, in_ch=cfgmod.KITTI_INPUT_CHANNELS, cls_bias=-0.5, num_classes=2)
    fr = IR.make_frame(1, W=W, pad_W=W, H=H)
    fr['input_data'] = np.ascontiguousarray(fr['input_data'][:, [0, 3, 4, 5, 1]])     # range, x, y, z, intensity
    ex = Executor(plan, P, lib=be.lib, alloc=be.alloc)
    outs = ex.forward(fr)
    ref = G.forward(fr, P, cfg=Cfg, num_fgs=ks)
    be.alloc.sync()
    sfgs = [s for s in plan.steps if s["kind"] == "sorted_fg"]
    assert len(sfgs) == 2 and [s["k"] for s in sfgs] == [ks['veh'], ks['ped']]
    assert len(outs) == 9   # rec_id + (score, boxes, zeros) per class + gt_bbox_imu, gt_class  (builder.py:54-77)
    for ci, cname in enumerate(('veh', 'ped')):
        rc = ref["classes"][cname]
        logit, delta = ex.read_flat(sfgs[ci]["score"]), ex.read_flat(sfgs[ci]["delta"])
        assert np.abs(logit - rc["logit"]).max() < 1e-4
        assert np.abs(delta - rc["delta"]).max() < 1e-4
        sc = np.array(be.alloc.to_numpy(outs[1 + 3 * ci]))
        bx = np.array(be.alloc.to_numpy(outs[2 + 3 * ci]))
        assert sc.shape == (1, ks[cname]) and bx.shape == (1, ks[cname], 10)
        assert np.abs(sc - rc["fg_cls_score"]).max() < 1e-5
        gap = np.abs(np.diff(rc["fg_cls_score"][0]))
        ok = np.ones(ks[cname], bool)
        ok[1:] &= gap > 1e-5
        ok[:-1] &= gap > 1e-5
        ok &= rc["fg_cls_score"][0] > 1e-6
        assert ok.sum() > ks[cname] // 10
        assert np.abs(bx[0][ok] - rc["decoded_bbox"][0][ok]).max() < 1e-3
    # the two classes really are different heads
    assert np.abs(ref["classes"]['veh']["logit"] - ref["classes"]['ped']["logit"]).max() > 1e-2


@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
def test_full_size_bf16_properties(be):
    """BASELINE config 2 + 3 at full size (64 x 2650 pad 2656, 8 ch, bf16, top-50000, weighted NMS), batch of 3 with frame 0
    repeated: size-independent properties.  Sorted scores in [0, 1]; the repeated frame gives bit-identical graph outputs
    and detections (the persistent kernels, the LDS-DMA pipeline and the batched NMS are deterministic and frames do not
    leak into each other); a second run reproduces the first bit for bit; kept rows are a subset of the candidates with
    scores above min_score; the (M, 8) boxes have positive extents."""
    from rangedet_amd.pipeline import RangeDetPipeline
    P = synth.make_weights(seed=18)
    pipe = RangeDetPipeline(P, dtype=R.RD_BF16, wnms_cap=4096, batch=3, lib=be.lib, alloc=be.alloc)
    fr = IR.make_batch([0, 1, 0])
    r1 = pipe.run(fr)
    sc1 = np.array(be.alloc.to_numpy(r1["fg_cls_score"]))
    bx1 = np.array(be.alloc.to_numpy(r1["decoded_bbox"]))
    assert sc1.shape == (3, 50000) and bx1.shape == (3, 50000, 10)
    assert np.all(np.diff(sc1, axis=1) <= 0) and sc1.max() <= 1 and sc1.min() >= 0
    assert np.array_equal(sc1[0], sc1[2]) and np.array_equal(bx1[0], bx1[2]) and not np.array_equal(sc1[0], sc1[1])
    f1 = r1["frames"]
    assert f1[0]["keep_inds"].tolist() == f1[2]["keep_inds"].tolist()
    assert np.array_equal(f1[0]["wnms_rows"], f1[2]["wnms_rows"])
    r2 = pipe.run(fr)
    assert np.array_equal(sc1, np.array(be.alloc.to_numpy(r2["fg_cls_score"])))
    for a, b in zip(f1, r2["frames"]):
        assert a["keep_inds"].tolist() == b["keep_inds"].tolist() and np.array_equal(a["wnms_rows"], b["wnms_rows"])
    for b_, f in enumerate(f1):
        K, keep = f["num_candidates"], f["keep_inds"]
        assert K == int((sc1[b_] > 0.5).sum()) and 0 < len(keep) <= K
        assert np.all(keep >= 0) and np.all(keep < K) and len(set(keep.tolist())) == len(keep)
        d8 = f["det_xyzlwhyaws"]
        assert np.isfinite(d8).all() and np.all(d8[:, 3:6] > 0) and np.all(d8[:, 7] > 0.5)


_FULL = {}


def _full_size_oracle():
    """graph_ref.forward on frames 0 and 1 at 64 x 2650 (pad 2656), all 50 000 candidates -- ~13 s per frame on the GPU box's
    host cores; computed once per session and shared by the fp32 and bf16 full-size tests."""
    if not _FULL:
        P = synth.make_weights(seed=18)
        fr = IR.make_batch([0, 1])
        _FULL.update(P=P, fr=fr, ref=G.forward(fr, P, num_fgs=50000))
    return _FULL["P"], _FULL["fr"], _FULL["ref"]


@pytest.mark.slow
@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
def test_full_size_f32_parity_vs_oracle(be):
    """BASELINE configs 2 + 3 at the PRODUCTION shape -- rangedet_veh_wo_aug_4_18e, 64 x 2650 padded to 2656 (43 x 8 conv
    tiles per frame, the W = 166 / 332 tails, the 2650 -> 2656 pad), batch 2, all 297 472 points, top-50 000 -- fp32 HIP path
    against the graph oracle on identical inputs:
      * logits and box regressions (deltas) of EVERY pixel within 1e-4 (north_star's fp32 bound);
      * get_sorted_foreground picks the same flat indices wherever the oracle's neighbouring scores differ by more than
        8x the measured score error (two rows whose scores are closer than the fp32 noise of two different conv
        implementations may legitimately swap);
      * Decode3DBbox of the path's own sorted deltas within 1e-4 of the oracle's decode of those same deltas (device libm);
      * end to end, boxes within 1e-4 + the propagated delta error (printed);
      * weighted NMS of the path's own (score, box) rows: survivor indices equal, rows bit-equal, to the oracle (== reference)."""
    from rangedet_amd.pipeline import RangeDetPipeline
    P, fr, ref = _full_size_oracle()
    B, k = 2, 50000
    pipe = RangeDetPipeline(P, dtype=R.RD_F32, batch=B, wnms_cap=8192, lib=be.lib, alloc=be.alloc)
    pipe.exe = Executor(pipe.plan, P, lib=be.lib, alloc=be.alloc, keep_sorted_idx=True)
    res = pipe.run(fr)
    ex = pipe.exe
    sfg = [s for s in pipe.plan.steps if s["kind"] == "sorted_fg"][0]
    logit, delta = ex.read_flat(sfg["score"]), ex.read_flat(sfg["delta"])
    e_l, e_d = np.abs(logit - ref["logit"]).max(), np.abs(delta - ref["delta"]).max()
    print("full size fp32: logit maxerr %.2e, delta maxerr %.2e" % (e_l, e_d))
    assert logit.shape == (B, 297472) and e_l < 1e-4 and e_d < 1e-4
    sc = np.array(be.alloc.to_numpy(res["fg_cls_score"]))
    bx = np.array(be.alloc.to_numpy(res["decoded_bbox"]))
    idx = ex.sorted_idx()
    assert np.abs(sc - ref["fg_cls_score"]).max() < 1e-5 and np.all(np.diff(sc, axis=1) <= 0)
    sdelta, spc = ex.read_flat(sfg["out_delta"]), ex.read_flat(sfg["out_pc"])
    assert np.abs(bx - O.decode3d(sdelta, spc, False)).max() < 1e-4           # decode alone: device libm vs glibc
    e_s = np.abs(sc - ref["fg_cls_score"]).max()
    sep = max(8 * e_s, 1e-6)
    for b in range(B):
        rs = ref["fg_cls_score"][b]
        gap = np.abs(np.diff(rs))
        ok = np.ones(k, bool)
        ok[1:] &= gap > sep
        ok[:-1] &= gap > sep
        ok &= rs > 1e-6
        same = idx[b] == ref["sorted_idx"][b]
        print("frame %d: score maxerr %.2e; %d of %d rows separated by > %.1e; %d of %d sorted indices equal overall" %
              (b, e_s, ok.sum(), k, sep, same.sum(), k))
        assert ok.sum() > 500 and same.mean() > 0.8
        assert np.array_equal(idx[b][ok], ref["sorted_idx"][b][ok])             # same points, same order
        # ... and EVERY row picked by the HIP path is a legitimate pick: its oracle score equals the oracle's score at that
        # sorted position up to the fp32 noise (rows that differ are swaps inside groups of numerically tied scores)
        mask = np.concatenate([fr["range_image_mask_s%d" % s_] for s_ in (1, 2, 4)], 1)[b]
        full = (1.0 / (1.0 + np.exp(-ref["logit"][b].astype(np.float64)))) * mask
        assert np.abs(full[idx[b]] - rs).max() < 4 * e_s + 1e-7
        e_b = np.abs(bx[b][ok] - ref["decoded_bbox"][b][ok]).max()
        # corners are centre +- exp(log l)/2 * cos/sin: d corner / d delta <= ~3 m for a car-sized box, so the bound is
        # 1e-4 (libm) + 3 * (measured delta error)
        print("frame %d: %d of %d rows with separated scores, box maxerr %.2e (delta err %.2e)" % (b, ok.sum(), k, e_b, e_d))
        assert e_b < 1e-4 + 3.0 * e_d
        got = res["frames"][b]
        dets, rows, keep, d8 = G.postprocess(sc[b], bx[b])
        assert got["num_candidates"] == dets.shape[0] and dets.shape[0] > 200
        assert got["keep_inds"].tolist() == list(keep)                          # WNMS survivor indices bit-exact
        assert np.abs(got["wnms_rows"] - rows).max() < 1e-5 and np.abs(got["det_xyzlwhyaws"] - d8).max() < 1e-4
        # and against the oracle's own end-to-end result (inputs differ by the <=1e-4 box error): same survivors
        dets_r, rows_r, keep_r, d8_r = G.postprocess(ref["fg_cls_score"][b], ref["decoded_bbox"][b])
        print("frame %d: %d candidates, %d kept (oracle end to end: %d, %d)" % (b, dets.shape[0], len(keep), dets_r.shape[0], len(keep_r)))
        # (row numbers refer to each run's own candidate list, in which rows with numerically tied scores may be swapped:
        # compare the surviving BOXES -- a one-to-one match within the box tolerance)
        assert dets.shape[0] == dets_r.shape[0] and len(keep) == len(keep_r)
        dist = np.abs(got["det_xyzlwhyaws"][:, None, :] - d8_r[None, :, :]).max(axis=2)
        match = dist.argmin(axis=1)
        assert dist.min(axis=1).max() < 2e-3 and len(set(match.tolist())) == len(keep_r)
        assert (np.asarray(keep) != np.asarray(keep_r)).sum() <= 4               # identical but for a few swapped neighbours


# bf16 error model for the tolerance below: every conv layer rounds its output activation to bf16 (relative 2^-9, uniform ->
# rms 2^-9/sqrt(3)) and uses weights rounded the same way; errors of independent layers add in quadrature, so along the
# deepest path of the graph (res1 4 + res2a 6 + res2 6 + res3a 10 + res3 10 + agg2 5 + agg2a 3 + agg3 5 + tower 4 = 53
# conv layers) the relative rms error of a pre-output activation is ~ 2^-9 * sqrt(2 * 53 / 3) = 1.2 %.  The 1x1 output conv
# is exact in fp32 on those activations, so logits / deltas inherit that fraction of the SPREAD of their value; residual adds
# re-inject un-rounded signal (lower), ReLU clipping correlates errors (higher): the test allows 2.5x the model for the rms
# and 6 rms (Gaussian tail over 6e5 samples, x safety) for the maximum.
BF16_REL_RMS = 2.0 ** -9 * np.sqrt(2 * 53 / 3.0)
F16_REL_RMS = 2.0 ** -12 * np.sqrt(2 * 53 / 3.0)    # fp16: the same model with its rounding unit (0.15 %)


@pytest.mark.slow
@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
@pytest.mark.parametrize("dt", [R.RD_BF16, R.RD_F16], ids=["bf16", "f16"])
def test_full_size_bf16_vs_f32_oracle(be, dt):
    """The throughput mode (bf16 persistent kernels, fused Meta-Kernel, fused tower outputs) at the production shape against
    the SAME fp32 oracle output, with a tolerance derived from bf16 rounding depth (see BF16_REL_RMS) instead of a smoke
    threshold: rms and max error of logits / deltas relative to their spread, and the agreement of the final detections."""
    from rangedet_amd.pipeline import RangeDetPipeline
    P, fr, ref = _full_size_oracle()
    BF16_REL_RMS = globals()["BF16_REL_RMS"] if dt == R.RD_BF16 else F16_REL_RMS     # (the body reads "BF16_REL_RMS")
    pipe = RangeDetPipeline(P, dtype=dt, batch=2, wnms_cap=8192, lib=be.lib, alloc=be.alloc)
    res = pipe.run(fr)
    sfg = [s for s in pipe.plan.steps if s["kind"] == "sorted_fg"][0]
    logit, delta = pipe.exe.read_flat(sfg["score"]), pipe.exe.read_flat(sfg["delta"])
    for name, got, want in (("logit", logit, ref["logit"]), ("delta", delta, ref["delta"])):
        err = got - want
        axes = (0, 1) if want.ndim == 3 else None
        spread = want.std(axis=axes)                  # per regression channel for the deltas
        rms = np.sqrt((err ** 2).mean(axis=axes)) / spread
        mx = np.abs(err).max(axis=axes) / spread
        print("full size " + ("bf16" if dt == R.RD_BF16 else "fp16") + " vs fp32 oracle, %s: rms/std %s  max/std %s  (model rms %.4f)" %
              (name, np.round(rms, 4), np.round(mx, 4), BF16_REL_RMS))
        assert np.all(rms < 2.5 * BF16_REL_RMS) and np.all(mx < 6 * 2.5 * BF16_REL_RMS)
    sc = np.array(be.alloc.to_numpy(res["fg_cls_score"]))
    assert np.abs(sc - ref["fg_cls_score"]).max() < 6 * 2.5 * BF16_REL_RMS * ref["logit"].std() * 0.25   # sigmoid' <= 1/4
    for b in range(2):
        dets_r, rows_r, keep_r, d8_r = G.postprocess(ref["fg_cls_score"][b], ref["decoded_bbox"][b])
        got = res["frames"][b]
        # detections: the bf16 path finds the same objects -- every oracle detection has a bf16 detection whose centre is
        # within 0.3 m (and vice versa for all but the few boxes that sit on the score threshold)
        d8 = got["det_xyzlwhyaws"]
        dist = np.linalg.norm(d8[:, None, :2] - d8_r[None, :, :2], axis=2)
        print("frame %d: bf16 %d detections, oracle %d; unmatched oracle %d, unmatched bf16 %d" %
              (b, len(d8), len(d8_r), int((dist.min(0) > 0.3).sum()), int((dist.min(1) > 0.3).sum())))
        assert abs(len(d8) - len(d8_r)) <= max(3, len(d8_r) // 20)
        # the unmatched ones are marginal detections (random-init weights put many boxes right at min_score 0.5: a logit
        # error of 0.04 std moves them across it), not different boxes: few, and low-scoring
        um_r, um_b = dist.min(0) > 0.3, dist.min(1) > 0.3
        assert um_r.mean() < 0.10 and um_b.mean() < 0.10
        assert not um_r.any() or np.median(d8_r[um_r, 7]) < 0.6
        assert not um_b.any() or np.median(d8[um_b, 7]) < 0.6


@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
def test_interleaved_pipelines_match_single(be):
    """Two batches in flight on two launch streams (pipeline.InterleavedPipelines, what bench.py runs) give, batch by batch,
    bit-identical detections to one pipeline run serially -- four batches, so each stream is reused while the other is busy."""
    from rangedet_amd.pipeline import InterleavedPipelines, RangeDetPipeline
    H, Wr, W, k = 16, 250, 256, 2000
    P = synth.make_weights(seed=18, width=W, cls_bias=-1.0)
    kw = dict(dtype=R.RD_BF16, feat_size=(H, Wr), pad_field=(H, W), pre_nms_top_n=k, wnms_cap=2048, batch=2)
    batches = [IR.make_batch([2 * i, 2 * i + 1], W=Wr, pad_W=W, H=H) for i in range(4)]
    single = RangeDetPipeline(P, lib=be.lib, alloc=be.alloc, **kw)
    want = [single.run(b_)["frames"] for b_ in batches]
    multi = InterleavedPipelines(P, n=2, lib=be.lib, alloc=be.alloc, **kw)
    got = [None] * 4
    for i in (0, 1):
        multi.enqueue(batches[i])
    for i in (0, 1):                      # collect batch i (pipeline i), then reuse its pipeline for batch i + 2
        got[i] = multi.collect(i)
        j, _ = multi.enqueue(batches[i + 2])
        assert j == i
    for i in (2, 3):
        got[i] = multi.collect(i - 2)
    for w_, g_ in zip(want, got):
        for fw, fg in zip(w_, g_):
            assert fw["num_candidates"] == fg["num_candidates"] and fw["keep_inds"].tolist() == fg["keep_inds"].tolist()
            assert np.array_equal(fw["wnms_rows"], fg["wnms_rows"])


@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
def test_kitti_full_size_bf16_properties(be):
    """BASELINE config 5 at its full size (64 x 2048 x 5, veh + ped heads, bf16): size-independent properties of the graph
    outputs -- per-class scores sorted and inside (0, 1), exactly k rows per class, finite boxes with positive extent,
    and the fp32 plan on the same frame agrees on the logits within the bf16 tolerance of test_e2e_bf16_tolerance."""
    H, W = 64, 2048
    ks = {'veh': 50000, 'ped': 5000}
    cfg = cfgmod.get_config(False, variant="kitti", feat_size=(H, W), pad_field=(H, W))
    shapes = small_shapes(H, W)
    shapes['input_data'] = (cfgmod.KITTI_INPUT_CHANNELS, H, W)
    P = synth.make_weights(seed=5, width=W, in_ch=cfgmod.KITTI_INPUT_CHANNELS, num_classes=2)
    fr = IR.make_frame(2, W=W, pad_W=W, H=H)
    fr['input_data'] = np.ascontiguousarray(fr['input_data'][:, [0, 3, 4, 5, 1]])
    logits = {}
    for dt in (R.RD_BF16, R.RD_F32):
        plan = lower(cfg[6].test_symbol, shapes, dt, 1)
        ex = Executor(plan, P, lib=be.lib, alloc=be.alloc)
        outs = ex.forward(fr)
        be.alloc.sync()
        sfgs = [s for s in plan.steps if s["kind"] == "sorted_fg"]
        logits[dt] = [ex.read_flat(s["score"]).copy() for s in sfgs]
        if dt == R.RD_BF16:
            for ci, cname in enumerate(('veh', 'ped')):
                sc = np.array(be.alloc.to_numpy(outs[1 + 3 * ci]))[0]
                bx = np.array(be.alloc.to_numpy(outs[2 + 3 * ci]))[0]
                assert sc.shape == (ks[cname],) and bx.shape == (ks[cname], 10)
                assert np.all(np.diff(sc) <= 0) and sc[0] < 1 and sc[-1] >= 0
                assert np.isfinite(bx).all() and np.all(bx[:, 9] > bx[:, 8])
        del ex
    for a, b in zip(logits[R.RD_BF16], logits[R.RD_F32]):
        el = np.abs(a - b).max() / b.std()
        print("kitti bf16 vs fp32 plan: logit maxerr/std %.3f" % el)
        assert el < 0.25


@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
def test_kitti_pipeline_two_class_fp16(be):
    """BASELINE config 5 through the PRODUCT harness at its full size, in the reference's own arithmetic type:
    RangeDetPipeline(variant="kitti", dtype=RD_F16), 64 x 2048 x 5 input, batch 2 -- per class (vehicle top-50000 / min_score 0.5,
    pedestrian top-5000 / 0.4, builder.py:467-478) the device's score filter + weighted NMS + 12->8 equal the oracle's harness
    restatement (tools/test.py:184-224) on the pipeline's own stage outputs: survivor indices bit-exact."""
    from rangedet_amd.pipeline import RangeDetPipeline
    H, W = 64, 2048
    P = synth.make_weights(seed=5, width=W, in_ch=cfgmod.KITTI_INPUT_CHANNELS, num_classes=2)
    fr = IR.make_batch([2, 3], W=W, pad_W=W, H=H)
    fr['input_data'] = np.ascontiguousarray(fr['input_data'][:, [0, 3, 4, 5, 1]])
    pipe = RangeDetPipeline(P, dtype=R.RD_F16, variant="kitti", feat_size=(H, W), pad_field=(H, W), batch=2,
                            pre_nms_top_n={'veh': 50000, 'ped': 5000}, wnms_cap=8192)
    assert pipe.class_names == ('veh', 'ped') and pipe.ks == {'veh': 50000, 'ped': 5000}
    outs = pipe.enqueue(fr)
    frames = pipe.collect()
    assert len(frames) == 2
    seen = 0
    for ci, c in enumerate(pipe.class_names):
        sc = np.array(be.alloc.to_numpy(outs[1 + 3 * ci]))
        bx = np.array(be.alloc.to_numpy(outs[2 + 3 * ci]))
        assert sc.shape == (2, pipe.ks[c]) and np.all(np.diff(sc, axis=1) <= 0)
        for b in range(2):
            got = frames[b]["per_class"][c]
            dets, rows, keep, d8 = G.postprocess(sc[b], bx[b], cls=c)
            assert got["num_candidates"] == dets.shape[0]
            assert got["keep_inds"].tolist() == list(keep), (c, b)
            if len(keep):
                # merged rows: a kept box's voter set depends on IoUs whose clip compares edge angles from atan2f with |da| < 1e-5
                # (nms.h:120-123).  Round 4: the device's own atan2f differed from glibc's by an ulp and flipped about one vote in a few
                # thousand rows (0.5 % of the rows were exempt).  Round 5: the edge angles are the C library's algorithm restated on the
                # device (rd_common.h fdlibm_atan2f) -- every row agrees; the tolerance left is the yaw column's atan2f in the score
                # filter (numpy's arctan2 in the reference, tools/test.py:56-81: an SVML routine, neither glibc's nor the device's)
                rowerr = np.abs(got["wnms_rows"] - rows).max(axis=1)
                assert (rowerr < 1e-5).all(), (c, b, int((rowerr >= 1e-5).sum()), len(rowerr))
                assert np.abs(got["det_xyzlwhyaws"] - d8).max() < 1e-4
            seen += dets.shape[0]
    assert seen > 100, "the synthetic weights must produce candidates in at least one class"
    # the first class's result is also what single-class callers read
    assert frames[0]["keep_inds"].tolist() == frames[0]["per_class"]["veh"]["keep_inds"].tolist()


@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
def test_pipeline_postprocess_matches_oracle(be):
    """forward + score filter + WNMS + 12->8 on the device == tools/test.py:184-224 restated on the same stage inputs."""
    from rangedet_amd.pipeline import RangeDetPipeline
    H, Wr, W, k = 16, 250, 256, 2000
    P = synth.make_weights(seed=18, width=W, cls_bias=-0.8)
    fr = IR.make_frame(1, W=Wr, pad_W=W, H=H)
    pipe = RangeDetPipeline(P, dtype=R.RD_F32, feat_size=(H, Wr), pad_field=(H, W), pre_nms_top_n=k, wnms_cap=2048)
    res = pipe.run(fr)
    sc, bx = res["fg_cls_score"].cpu().numpy()[0], res["decoded_bbox"].cpu().numpy()[0]
    dets, rows, keep, d8 = G.postprocess(sc, bx)   # oracle on the GPU's own stage outputs (identical stage inputs)
    assert res["num_candidates"] == dets.shape[0] and dets.shape[0] > 50
    assert res["keep_inds"].tolist() == list(keep)                      # WNMS survivor indices bit-exact
    assert np.abs(res["wnms_rows"] - rows).max() < 1e-5                   # yaw column goes through device atan2f
    assert np.abs(res["det_xyzlwhyaws"] - d8).max() < 1e-4


@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
def test_pipeline_nms3d_branch_matches_harness(be):
    """RangeDetPipeline(wnms=False): graph with contrib.NMS3D + the `not pTest.nms.wnms` harness branch on the device ==
    tools/test.py:193-224 restated in numpy on the graph's own outputs (two frames in one batch)."""
    from rangedet_amd.pipeline import RangeDetPipeline
    H, Wr, W, k = 16, 250, 256, 2000
    P = synth.make_weights(seed=18, width=W, cls_bias=-0.8)
    frs = [IR.make_frame(i, W=Wr, pad_W=W, H=H) for i in (1, 2)]
    fr = {n: np.concatenate([f[n] for f in frs]) for n in frs[0] if isinstance(frs[0][n], np.ndarray)}
    pipe = RangeDetPipeline(P, dtype=R.RD_F32, feat_size=(H, Wr), pad_field=(H, W), pre_nms_top_n=k, batch=2, wnms=False)
    assert any(s["kind"] == "nms3d" for s in pipe.plan.steps)
    res = pipe.run(fr)
    outs = pipe.forward(fr)
    be.alloc.sync()
    sc, final, keep = (np.array(o.cpu().numpy()) for o in outs[1:4])
    assert final.shape == (2, 200, 10) and keep.dtype == np.int32
    for b in range(2):
        kb = keep[b][keep[b] != -1]                                    # tools/test.py:194-196
        b4, s_ = final[b][keep[b] != -1], sc[b][kb]
        fg = s_ > 0.5
        assert fg.sum() > 5
        d11 = O.bbox3d_10dim_to_11dim(b4[fg])
        rows = np.concatenate([d11, s_[fg][:, None]], axis=1)
        got = res["frames"][b]
        assert got["num_candidates"] == rows.shape[0]
        assert np.abs(got["wnms_rows"] - rows).max() < 1e-5           # yaw column goes through device atan2f
        assert np.abs(got["det_xyzlwhyaws"] - O.bbox3d_12dim_to_8dim(rows)).max() < 1e-4
        assert got["keep_inds"].tolist() == kb[fg].tolist()


@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
def test_evaluate_loop_and_export(be, tmp_path):
    """rangedet_amd.evaluate (tools/test.py's loop on the HIP path): raw records -> device transform -> pipeline -> the
    output_dict pickle -> prediction bin; per frame the same detections as running that frame through the pipeline with
    the host-side transform."""
    from rangedet_amd import evaluate, export
    from rangedet_amd.pipeline import RangeDetPipeline
    H, W, Wp = 16, 250, 256
    P = synth.make_weights(seed=18, width=Wp, cls_bias=-0.8)
    roidb = [dict(synth.raw_record(i, H=H, W=W), rec_id=i) for i in range(3)]
    # record 1 goes through the pc_url path: an npz with the schema datasets/create_range_image_roidb.py writes
    seg = tmp_path / "segment-123_with_camera_labels"
    seg.mkdir()
    r1 = roidb[1]
    np.savez(seg / "1550083467346370.npz", range_image=r1['range_image'].astype(np.float64), pc_vehicle_frame=r1['pc_vehicle_frame'],
             inclination=r1['inclination'], azimuth=r1['azimuth'])
    roidb[1] = dict(pc_url=str(seg / "1550083467346370.npz"), rec_id=1, gt_bbox_imu=np.zeros((0, 8), np.float32))
    ann, out = evaluate.run(roidb, P, batch=2, pre_nms_top_n=2000)
    assert sorted(out) == [0, 1, 2] and set(ann) == set(out)
    pipe = RangeDetPipeline(P, feat_size=(H, W), pad_field=(H, Wp), batch=1, pre_nms_top_n=2000)
    for i in range(3):
        ref = pipe.run(IR.make_frame(i, W=W, pad_W=Wp, H=H))["det_xyzlwhyaws"]
        got = out[i]['det_xyzlwhyaws']['TYPE_VEHICLE']
        assert got.shape == ref.shape and got.shape[0] > 0 and np.abs(got - ref).max() < 1e-3   # bf16 graph both ways
        assert out[i]['meta_info'] == ({'name': 'synthetic', 'timestamp_micros': i} if i != 1 else
                                       {'name': '123', 'timestamp_micros': 1550083467346370})
    # a weighted-NMS capacity far below the number of candidates: the frames overflow, are re-run alone with a capacity that
    # fits, and give the same detections -- nothing is truncated (the reference has no capacity, nms.h:452-577)
    ann2, out2 = evaluate.run(roidb, P, batch=2, pre_nms_top_n=2000, wnms_cap=64)
    assert sorted(out2) == sorted(out)
    for i in out:
        assert np.array_equal(out2[i]['det_xyzlwhyaws']['TYPE_VEHICLE'], out[i]['det_xyzlwhyaws']['TYPE_VEHICLE'])
    pk = tmp_path / "checkpoint_output_dict_18e.pkl"
    with open(pk, "wb") as f:
        import pickle
        pickle.dump(ann, f)
        pickle.dump(out, f)
    export.main(str(pk), "cfg", str(tmp_path))
    objs = export.parse_objects((tmp_path / "cfg.bin").read_bytes())
    assert len(objs) == sum(v['det_xyzlwhyaws']['TYPE_VEHICLE'].shape[0] for v in out.values())
    assert objs[0]["type"] == 1 and abs(objs[0]["score"] - float(out[0]['det_xyzlwhyaws']['TYPE_VEHICLE'][0, 7])) < 1e-7


def _reduced_symbol(cfg, H, W):
    """The test symbol with one block per stage (two in res1, so the Meta-Kernel unit stays) and one-layer head towers, built
    through the same builders: what the CPU emulation can run in seconds."""
    from rangedet_amd.symbol.backbone.dla_backbone import DLABackbone
    from rangedet_amd.symbol.head.builder import RangeRCNN, RangeRpnHead

    class Cfg(G.Cfg):
        num_block = dict({kk: 1 for kk in G.Cfg.num_block}, res1=2)
        head_layers = 1
    RP = cfg[2]
    bp = type("BackboneParam", (), dict(fp16=True, normalizer=RP.normalizer, fpn_strides=(1, 2, 4), batch_image=1,
                                        range_image_shape_hw=(H, W), add_data_sc=True, num_block=Cfg.num_block,
                                        num_filter=G.Cfg.num_filter,
                                        meta_kernel_units={'res1_unit2': dict(stride=1, meta_func_param='meta_baseline_bias',
                                                                              data_channels=64, coord_channels=3,
                                                                              channel_list=[32, 64], kernel_size=3)}))
    RP.head.cls_conv_layers = RP.head.reg_conv_layers = 1
    dp = type("DetParam", (), dict(fpn_strides=(1, 2, 4), class_names=('veh',)))
    return RangeRCNN(dp).get_test_symbol(DLABackbone(bp), RangeRpnHead(RP)), Cfg


@pytest.mark.parametrize("be", BOTH, indirect=True)
@pytest.mark.parametrize("dt", [R.RD_BF16, R.RD_F16], ids=["bf16", "f16"])
def test_e2e_bf16_tolerance(be, dt, monkeypatch):
    """16-bit runs of the lowered plan: bf16 (BASELINE config 2) and fp16 (the reference's own mixed-precision type, config:35;
    rounding unit 2^-12 instead of 2^-9, the same error model).
    bf16 run of the lowered plan -- persistent 3x3 kernel incl. the stride-2 pixel-pair view and the
    fused projection shortcuts, fused Meta-Kernel, fused tower outputs -- against the fp32 oracle with the tolerance derived
    from bf16 rounding depth (BF16_REL_RMS, scaled to this graph's depth).  emu: depth-reduced graph, hip: full depth."""
    emu = be.name == "emu"
    H, Wr, W, k = (8, 62, 64, 300) if emu else (16, 250, 256, 2000)
    cfg = cfgmod.get_config(False, feat_size=(H, Wr), pad_field=(H, W), pre_nms_top_n={'veh': k})
    sym, Cfg = _reduced_symbol(cfg, H, W) if emu else (cfg[6].test_symbol, G.Cfg)
    plan = lower(sym, small_shapes(H, W), dt, 1)
    # (the reduced graph's one-layer towers read the never-materialised concat [agg3 | range image] directly at level 0: that two-tensor
    #  launch has no fused output conv, the level's two 1x1 output convs stay separate launches there)
    assert sum(1 for s, _ in conv_steps(plan.steps) if s.get("sc")) == 9 and sum(1 for s, _ in conv_steps(plan.steps) if s.get("head")) == (4 if emu else 6)
    assert sum(1 for s in plan.steps if s["kind"] == "block") == (4 if emu else 8)      # fused BasicBlocks (lower._fuse_blocks) run in both graphs
    assert sum(1 for s in plan.steps if s.get("x2") is not None) == 2 and sum(1 for s in plan.steps if s["kind"] == "nchw_in") == 1
    P = synth.make_weights(seed=18, width=W, cls_bias=-0.5)
    fr = IR.make_frame(0, W=Wr, pad_W=W, H=H)
    ex = Executor(plan, P, lib=be.lib, alloc=be.alloc)
    ex.forward(fr)
    ref = G.forward(fr, P, cfg=Cfg, num_fgs=k)
    sfg = [s for s in plan.steps if s["kind"] == "sorted_fg"][0]
    logit, delta = ex.read_flat(sfg["score"]), ex.read_flat(sfg["delta"])
    depth = 19 if emu else 53
    model = (2.0 ** -9 if dt == R.RD_BF16 else 2.0 ** -12) * np.sqrt(2 * depth / 3.0)
    for name, got, want in (("logit", logit, ref["logit"]), ("delta", delta, ref["delta"])):
        err = got - want
        axes = (0, 1) if want.ndim == 3 else None
        spread = want.std(axis=axes)
        rms, mx = np.sqrt((err ** 2).mean(axis=axes)) / spread, np.abs(err).max(axis=axes) / spread
        print(("bf16" if dt == R.RD_BF16 else "fp16") + " vs fp32 oracle (%s), %s: rms/std %s max/std %s (model rms %.4f)" % (be.name, name, np.round(rms, 4), np.round(mx, 4), model))
        assert np.all(rms < 2.5 * model) and np.all(mx < 6 * 2.5 * model)
    # batch 2, on the shared concat buffer and on the default plan
    if emu and dt != R.RD_BF16:
        return                                                  # (CPU tier: once, in bf16)
    monkeypatch.setenv("RD_DEV_SWITCHES", "1")
    fr2 = {kk: np.concatenate([v, IR.make_frame(1, W=Wr, pad_W=W, H=H)[kk]], 0) for kk, v in fr.items()}
    # (RD_CONCAT_BUFFER=1: the concat in one shared buffer; the default plan reads it from two tensors)
    monkeypatch.setenv("RD_CONCAT_BUFFER", "1")
    bplan = lower(sym, small_shapes(H, W), dt, 2)
    monkeypatch.delenv("RD_CONCAT_BUFFER")
    assert sum(1 for s in bplan.steps if s["kind"] == "nchw_in") == 2 and not any(s.get("x2") is not None for s in bplan.steps)
    outs = []
    for pl in (bplan, lower(sym, small_shapes(H, W), dt, 2)):
        e2 = Executor(pl, P, lib=be.lib, alloc=be.alloc)
        e2.forward(fr2)
        sf = [s for s in pl.steps if s["kind"] == "sorted_fg"][0]
        outs.append((e2.read_flat(sf["score"]).copy(), e2.read_flat(sf["delta"]).copy()))
    assert np.array_equal(outs[1][0][0], logit[0])            # (and frame 0 of the batch equals the single-frame run)
    # the never-materialised concat against the shared buffer: the same numbers in another channel order ([agg3 | range image]
    # instead of [range image | agg3]), i.e. another fp32 summation order in the level-0 tower convs -- a 128-channel activation
    # that sits on a rounding boundary may round the other way, and in the full graph that unit travels through three more tower
    # convs: differences of the size of the 16-bit error model itself (`model` above), nothing systematic; the reduced graph's
    # level 0 also applies its 1x1 output convs in a separate launch
    for i_ in (0, 1):
        d_ = np.abs(outs[1][i_] - outs[0][i_])
        assert d_.max() < 6 * model * outs[0][i_].std() and d_.mean() < 0.1 * model * outs[0][i_].std(), (d_.max(), d_.mean())


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_batch_rotated_iou_through_the_symbol_api(be):
    """mx.sym.Custom(op_type='batch_rotated_iou') on the graph's decoded boxes (builder.py:176-182 attaches it to every level's
    decoded boxes in training) is recorded, lowered to rd_batch_rotated_iou and equals the oracle on the graph's own boxes."""
    emu = be.name == "emu"
    H, Wr, W, k = (8, 30, 32, 150) if emu else (16, 250, 256, 2000)
    cfg = cfgmod.get_config(False, feat_size=(H, Wr), pad_field=(H, W), pre_nms_top_n={'veh': k})
    sym, Cfg = _reduced_symbol(cfg, H, W) if emu else (cfg[6].test_symbol, G.Cfg)
    boxes_sym = sym.inputs[2]                                    # decoded_bbox of the Group (builder.py:77)
    iou = mx.sym.Custom(proposal=boxes_sym, gt_bbox=mx.var("gt_bbox_veh_for_iou_pred"), op_type="batch_rotated_iou", iou_type="bev",
                        name="batch_rotated_iou_veh")
    # iou_type '3d' (batch_rotated_iou.py:17-18,36-39): gt_bbox is (200, 7), the proposals are converted on the device.  Both ops hang on
    # the same decoded boxes of ONE graph (one forward: the emulator needs a minute per forward)
    iou3 = mx.sym.Custom(proposal=boxes_sym, gt_bbox=mx.var("gt7"), op_type="batch_rotated_iou", iou_type="3d", name="batch_rotated_iou_3d_veh")
    grp = mx.sym.Group(list(sym.inputs) + [iou, iou3])
    shapes = dict(small_shapes(H, W), gt_bbox_veh_for_iou_pred=(200, 8), gt7=(200, 7))
    plan = lower(grp, shapes, R.RD_F32, 1)
    assert [s["kind"] for s in plan.steps][-2:] == ["batch_riou", "batch_riou"] and plan.outputs[-1][1].shape == (k,) and plan.outputs[-2][1].shape == (k,)
    assert plan.steps[-1]["iou_type"] == "3d" and plan.steps[-2].get("iou_type", "bev") == "bev"
    P = synth.make_weights(seed=18, width=W, cls_bias=-0.5)
    fr = IR.make_frame(0, W=Wr, pad_W=W, H=H)
    ex = Executor(plan, P, lib=be.lib, alloc=be.alloc)
    rb = G.forward(fr, P, cfg=Cfg, num_fgs=k)["decoded_bbox"][0]  # where the boxes will be (the oracle's, within 1e-3)
    gt = np.tile(np.array([0, 0, 0, 1e-3, 1e-3, 1e-3, 1e-3, 0], np.float32), (200, 1))
    gt[:20] = rb[::k // 20][:20, :8] + 0.2                        # GT boxes = shifted copies of some predictions
    gt7 = np.zeros((200, 7), np.float32)
    gt7[:, 3:6] = 1e-3
    p10 = rb[::k // 20][:20].copy()
    p10[:, :8] += 0.2
    gt7[:20] = O.to_box_type_7(p10)
    outs = ex.forward(dict(fr, gt_bbox_veh_for_iou_pred=gt[None], gt7=gt7[None]))
    be.alloc.sync()
    bx = np.array(be.alloc.to_numpy(outs[2]))[0]
    got = np.array(be.alloc.to_numpy(outs[-2]))[0]
    ref = O.batch_max_iou(bx[:, :8], gt)
    assert got.shape == (k,) and np.abs(got - ref).max() < 1e-5 and (ref > 0.3).sum() >= 20
    got3 = np.array(be.alloc.to_numpy(outs[-1]))[0]
    ref3 = O.batch_max_iou_3d(bx, gt7)[0]
    assert got3.shape == (k,) and np.abs(got3 - ref3).max() < 1e-5 and (ref3 > 0.2).sum() >= 20
    with pytest.raises(ValueError):
        lower(mx.sym.Group([mx.sym.Custom(proposal=boxes_sym, gt_bbox=mx.var("g"), op_type="batch_rotated_iou", iou_type="3d")]),
              dict(shapes, g=(200, 8)), R.RD_F32, 1)                     # the '3d' op takes 7-dim ground truth (batch_rotated_iou.py:88-89)
    with pytest.raises(ValueError):
        lower(mx.sym.Group([mx.sym.Custom(proposal=boxes_sym, gt_bbox=mx.var("g"), op_type="batch_rotated_iou", iou_type="giou")]),
              dict(shapes, g=(200, 8)), R.RD_F32, 1)

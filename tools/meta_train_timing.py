"""Training-mode Meta-Kernel unit timing (dev tool): every launch of rangedet_amd.backward.MetaUnitTrain -- the statistics of q
(rd_meta_kernel_stats), the training forward (rd_meta_kernel_fwd_train), pass A (rd_meta_kernel_bwd_sums), pass B
(rd_meta_kernel_bwd_params_train), the data gradient (rd_meta_kernel_bwd_data_train), the re-pack (rd_pack_meta_dev) -- and a whole unit
forward + backward (with both BatchNorms' statistics, folds and the second norm's launches), at res1_unit2's shape: B frames of 64 x 2656, 64
channels, in bf16 and fp16.

    python tools/meta_train_timing.py [--batch 8] [--iters 3] [--repeats 3] [--out profiles/meta_train_timing.json]

Baseline for the whole unit, on the very same inputs: torch autograd of the UN-FUSED formulation tools/meta_backward_timing.py times, with
F.batch_norm(training=True) on both norms, in the same 16-bit type on the same GPU.  The frozen-statistics unit (MetaUnitBackward) is timed
in the same process as the second yardstick.  If a baseline cannot run, the error is recorded and no number is invented.  Each figure is the
median over `repeats` windows of `iters` calls between device events, after a warm-up of every side; the windows alternate and the series is
run in both orders, all in this one process (tools/timing_util.py).  Not profiled: end-to-end launch windows only."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rangedet_amd import build, lib as rdlib, synth  # noqa: E402
from rangedet_amd.backward import BN_EPS, MetaUnitBackward, MetaUnitTrain  # noqa: E402
from rangedet_amd.runtime import TorchAllocator  # noqa: E402
from tools.timing_util import series  # noqa: E402

H, W, NAME = 64, 2656, "res1_unit2"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meta_train_timing.json"))
    a = ap.parse_args()
    A, L = TorchAllocator(), rdlib.get_lib()
    dev, B = A.device, a.batch
    P = dict(synth.make_weights(seed=18, width=0))
    for k in [k for k in P if k.startswith(NAME + "_0_")]:
        P[NAME + "_%d_" % W + k[len(NAME) + 3:]] = P[k]
    gen = torch.Generator(device="cpu").manual_seed(23)
    npix = B * H * W
    rows = []
    for dname, dt, tdt in (("bf16", rdlib.RD_BF16, torch.bfloat16), ("f16", rdlib.RD_F16, torch.float16)):
        data = torch.relu(torch.randn(npix, 64, generator=gen)).to(dev, tdt).view(B, H, W, 64)
        coord = torch.randn(B, 3, H, W, generator=gen).to(dev)
        g = torch.randn(npix, 64, generator=gen).to(dev, tdt).view(B, H, W, 64)
        unit, frozen = MetaUnitTrain(NAME, P, W, dtype=dt, lib=L, alloc=A), MetaUnitBackward(NAME, P, W, dtype=dt, lib=L, alloc=A)
        o = unit.ops
        unit.forward(data, coord)
        unit.backward(g)
        dz, tabs = unit.dz, dict(unit.saved["tabs"])
        sums = o.meta_bwd_sums(dz, data, coord, unit.packed_bwd, tabs)
        tabs.update(c1=sums["c1"], c2=sums["c2"])
        row = dict(dtype=dname, B=B, H=H, W=W, stats_workspace_bytes=int(L.raw("rd_meta_kernel_stats_workspace_bytes")(B, H, W, 0)),
                   bwd_workspace_bytes=int(L.raw("rd_meta_kernel_bwd_train_workspace_bytes")(B, H, W, 0)))

        def ours_unit():
            unit.forward(data, coord)
            return unit.backward(g)

        def frozen_unit():
            frozen.forward(data, coord)
            return frozen.backward(g)
        cases = dict(stats=dict(ours=lambda: o.meta_stats(data, coord, unit.packed_bwd)),
                     fwd_train=dict(ours=lambda: o.meta_forward_train(data, coord, unit.packed_fwd, unit.packed_bwd, tabs["a1"], tabs["bb1"])),
                     sums=dict(ours=lambda: o.meta_bwd_sums(dz, data, coord, unit.packed_bwd, tabs)),
                     params=dict(ours=lambda: o.meta_bwd_params_train(dz, data, coord, unit.packed_bwd, tabs)),
                     data=dict(ours=lambda: o.meta_bwd_data_train(dz, data, coord, unit.packed_bwd, tabs)),
                     pack=dict(ours=lambda: o.pack_meta_dev(unit.masters, unit.packed_fwd, unit.packed_bwd)),
                     unit=dict(ours=ours_unit, frozen=frozen_unit))
        try:
            f32 = lambda k, shape: np.ascontiguousarray(P[k], dtype=np.float32).reshape(shape)
            pre = "%s_%d" % (NAME, W)
            host = dict(w0=f32(pre + "_mlp0_weight", (32, 3)), b0=f32(pre + "_mlp0_bias", (32,)), w1=f32(pre + "_mlp1_weight", (64, 32)),
                        b1=f32(pre + "_mlp1_bias", (64,)), agg=f32(NAME + "aggregation_conv1_weight", (64, 576)),
                        g1=f32(NAME + "point_wise_mlp_bn1_gamma", (576,)), be1=f32(NAME + "point_wise_mlp_bn1_beta", (576,)),
                        g2=f32(NAME + "aggregation_bn1_gamma", (64,)), be2=f32(NAME + "aggregation_bn1_beta", (64,)))
            tp = {k: torch.from_numpy(v).to(dev, tdt).requires_grad_(True) for k, v in host.items()}
            xt = data.permute(0, 3, 1, 2).detach().requires_grad_(True)
            gt = g.permute(0, 3, 1, 2)

            def t_y():
                cs = F.unfold(coord, 3, padding=1).view(B, 3, 9, H, W)
                rel = (cs - coord.unsqueeze(2)).to(tdt).reshape(B, 3, 9 * H, W)
                h = torch.relu(F.conv2d(rel, tp["w0"].view(32, 3, 1, 1), tp["b0"]))
                w = F.conv2d(h, tp["w1"].view(64, 32, 1, 1), tp["b1"]).view(B, 64, 9, H, W)
                ds = F.unfold(xt, 3, padding=1).view(B, 64, 9, H, W)
                act = torch.relu(F.batch_norm((ds * w).reshape(B, 576, H, W), None, None, tp["g1"], tp["be1"], training=True, eps=BN_EPS))
                z = F.conv2d(act, tp["agg"].view(64, 576, 1, 1))
                return torch.relu(F.batch_norm(z, None, None, tp["g2"], tp["be2"], training=True, eps=BN_EPS))
            plist = list(tp.values())
            cases["unit"]["torch"] = lambda: torch.autograd.grad(t_y(), [xt] + plist, gt)
            od, td = ours_unit()[0].float(), cases["unit"]["torch"]()[0].permute(0, 2, 3, 1).float()
            torch.cuda.synchronize()
            row["data_grad_max_rel_diff_vs_torch"] = float(((od - td).abs().max() / td.abs().max()).cpu())
        except Exception as e:                                                     # recorded, not replaced by a guess
            row["torch_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
            cases["unit"].pop("torch", None)
        for what, fns in cases.items():
            print("warm-up", dname, what, sorted(fns), flush=True)
            try:
                for f in fns.values():
                    f()
                torch.cuda.synchronize()
                med, raw = series(fns, a.iters, a.repeats)
            except Exception as e:
                row[what + "_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
                continue
            row[what + "_ms"] = med["ours"]
            for other in ("torch", "frozen"):
                if other in med:
                    row["%s_%s_ms" % (what, other)], row["%s_%s_over_ours" % (what, other)] = med[other], med[other] / med["ours"]
            row[what + "_series"] = raw
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_series")}), flush=True)
        rows.append(row)
        del cases, unit, frozen, data, g, dz, tabs, sums
        xt = gt = tp = plist = None
        torch.cuda.empty_cache()
    out = dict(tool="tools/meta_train_timing.py", source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               iters=a.iters, repeats=a.repeats, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()

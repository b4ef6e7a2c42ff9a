"""Aggregation-stage timing (dev tool): the transposed conv's weight gradient (rd_deconv_bwd_weight), its data gradient (one persistent 3x3
launch on the s-pixel view of dz), the stage's join (rd_bn_stats + rd_bn_fold + rd_affine_relu_add), a whole
rangedet_amd.backbone_train.AggStageTrain forward + backward (with a one-block res stage) and the SGD step with and without the deconv
re-pack launches, at the four transposed convs of the network, B frames of 64 rows, W = 2656 at stride 1:

    agg2    128 @ 166 -> 128 @ 664    (3,8) / 4 / 2          agg1    128 @ 664 -> 64 @ 2656    (3,8) / 4 / 2
    agg2a   128 @ 664 -> 64 @ 1328    (3,4) / 2 / 1          agg3    64 @ 1328 -> 64 @ 2656    (3,4) / 2 / 1

    python tools/agg_stage_timing.py [--batch 8] [--iters 5] [--repeats 3] [--out profiles/agg_train_timing.json]

Baselines, on the very same buffers:
  torch     torch's own conv_transpose2d weight / input gradient, batch_norm(training=True) + relu + add for the join and, for the stage,
            conv_transpose2d / batch_norm / relu / add and one projection BasicBlock forward with autograd backward, in the same 16-bit type on
            channels-last views
  norepack  (SGD step only) the step over the same parameters with the deconv weight registered without images
The data gradient's cost model is a 3x3 conv of the view's shape, 9 B H Win (s Cout) Cin multiply-adds, of which one third meet structural
zeros of the view weight; data_grad_tflops counts all of them, data_grad_useful_tflops the two thirds that are the transposed conv's.
If a baseline cannot run, the error is recorded and no number is invented.  Each figure is the median over `repeats` windows of `iters`
calls between device events, after a warm-up of every side; the windows alternate and the series is run in both orders, all in this one
process (tools/timing_util.py).  Not profiled: no hardware counters, no per-kernel split; the times are end-to-end launch windows only."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rangedet_amd import build, lib as rdlib  # noqa: E402
from rangedet_amd.backbone_train import AggStageTrain, BasicBlockTrain, ResStageTrain  # noqa: E402
from rangedet_amd.backward import BN_EPS, BN_MOMENTUM, TowerOps  # noqa: E402
from rangedet_amd.optim import SGD  # noqa: E402
from rangedet_amd.runtime import TorchAllocator  # noqa: E402
from tools.timing_util import series  # noqa: E402

H = 64
# (stage, Win, cin, cout, KW, s, p)
SHAPES = (("agg2", 166, 128, 128, 8, 4, 2), ("agg1", 664, 128, 64, 8, 4, 2), ("agg2a", 664, 128, 64, 4, 2, 1), ("agg3", 1328, 64, 64, 4, 2, 1))


def bn_params(C, rng):
    return (rng.uniform(0.5, 1.5, C).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32), np.zeros(C, np.float32),
            np.ones(C, np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dtype", choices=("bf16", "f16"), default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agg_train_timing.json"))
    a = ap.parse_args()
    A, L = TorchAllocator(), rdlib.get_lib()
    dev, B = A.device, a.batch
    dt, tdt = (rdlib.RD_BF16, torch.bfloat16) if a.dtype == "bf16" else (rdlib.RD_F16, torch.float16)
    gen = torch.Generator(device="cpu").manual_seed(17)
    rng = np.random.default_rng(7)
    ops = TowerOps(dt, L, A)
    rows = []
    for stage, Win, cin, cout, KW, s, p in SHAPES:
        Wout = s * Win
        up = torch.relu(torch.randn(B * H * Win, cin, generator=gen)).to(dev, tdt).view(B, H, Win, cin)
        skip = torch.relu(torch.randn(B * H * Wout, cout, generator=gen)).to(dev, tdt).view(B, H, Wout, cout)
        g = torch.randn(B * H * Wout, cout, generator=gen).to(dev, tdt).view(B, H, Wout, cout)
        w = (rng.standard_normal((cin, cout, 3, KW)) / np.sqrt(3 * KW * cout / 4)).astype(np.float32)
        bw = [(rng.standard_normal((cout, cout, 3, 3)) / np.sqrt(9 * cout / 2)).astype(np.float32) for _ in range(2)]
        bsc = (rng.standard_normal((cout, cout, 1, 1)) / np.sqrt(cout)).astype(np.float32)
        bns = [bn_params(cout, rng) for _ in range(4)]
        macs = 3 * KW * B * H * Win * cin * cout                        # the transposed conv's multiply-adds (edges included)
        view_macs = 9 * B * H * Win * s * cout * cin
        row = dict(stage=stage, dtype=a.dtype, B=B, H=H, Win=Win, Wout=Wout, cin=cin, cout=cout, kernel_w=KW, stride_w=s, pad_w=p,
                   deconv_gmacs=macs / 1e9, view_conv_gmacs=view_macs / 1e9, view_cin=s * cout,
                   wgrad_partials=int(L.raw("rd_deconv_bwd_weight_workspace_bytes")(B, H, Win, cin, cout, KW, s, p, 0) // (12 * KW * cin * cout)))
        cases = {}
        cases["wgrad"] = dict(ours=lambda: ops.deconv_weight_grad(up, g, KW, s, p, tag="t"))
        image = ops.pack_deconv_data_grad(w, s, p)
        cases["data_grad"] = dict(ours=lambda: ops.deconv_data_grad(g, image, tag="t"))
        fwd = ops.pack_deconv_unscaled(w, s, p)
        z = ops.deconv_unscaled(up, fwd, tag="t")
        gamma, beta, mm, mv = (A.upload(v) for v in bns[0])

        def ours_join():
            mean, var = ops.bn_stats(z, tag="t")
            _, a_, b_ = ops.bn_fold(mean, var, gamma, beta, mm, mv, B * H * Wout, cout, BN_EPS, BN_MOMENTUM, tag="t")
            return ops.affine_relu_add(z, a_, b_, skip, tag="t")
        cases["join"] = dict(ours=ours_join)
        res = ResStageTrain([BasicBlockTrain(stage + "_res_unit1", bw[0], bw[1], bns[1], bns[2], bsc, bns[3], dtype=dt, lib=L, alloc=A)])
        st = AggStageTrain(stage, w, bns[0], res, (3, KW), (1, s), (1, p), dtype=dt, lib=L, alloc=A)

        def ours_stage():
            st.forward(skip, up)
            return st.backward(g)
        cases["stage"] = dict(ours=ours_stage)
        opts = {}
        for key, strip in (("ours", False), ("norepack", True)):
            opts[key] = SGD(lr=0.0, wd=0.0, lib=L, alloc=A)          # lr 0: the weights stay as they are over the repeats
            for kw in st.optimizer_entries():
                if strip and kw["name"].endswith("_deconv_weight"):
                    kw = dict(kw, pack=None)
                opts[key].add(**kw)
        cases["sgd_step"] = {k: o.step for k, o in opts.items()}
        try:
            nc = lambda v: v.permute(0, 3, 1, 2)
            upt, skt, zt0 = (nc(v).detach().requires_grad_(True) for v in (up, skip, z))
            gt = nc(g)
            cl = lambda v: torch.from_numpy(v).to(dev, tdt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            tw, tbw, tsc = cl(w), [cl(v) for v in bw], cl(bsc)
            tb = [torch.from_numpy(v).to(dev).requires_grad_(True) for b_ in bns for v in b_[:2]]
            tz = F.conv_transpose2d(upt, tw, stride=(1, s), padding=(1, p))
            cases["wgrad"]["torch"] = lambda: torch.autograd.grad(tz, tw, gt, retain_graph=True)
            cases["data_grad"]["torch"] = lambda: torch.autograd.grad(tz, upt, gt, retain_graph=True)
            bnf = lambda v, ga, be: F.batch_norm(v, None, None, ga, be, training=True, momentum=1 - BN_MOMENTUM, eps=BN_EPS)
            cases["join"]["torch"] = lambda: torch.relu(bnf(zt0, tb[0], tb[1])) + skt      # (timed under no_grad: the forward alone)

            def t_stage():
                t = torch.relu(bnf(F.conv_transpose2d(upt, tw, stride=(1, s), padding=(1, p)), tb[0], tb[1])) + skt
                y1 = torch.relu(bnf(F.conv2d(t, tbw[0], padding=1), tb[2], tb[3]))
                y = torch.relu(bnf(F.conv2d(y1, tbw[1], padding=1), tb[4], tb[5]) + bnf(F.conv2d(t, tsc), tb[6], tb[7]))
                return torch.autograd.grad(y, [upt, skt, tw, tsc] + tbw + tb, gt)
            cases["stage"]["torch"] = t_stage
            odW, tdW = cases["wgrad"]["ours"]().clone(), cases["wgrad"]["torch"]()[0].float()
            odx, tdx = cases["data_grad"]["ours"]().float(), cases["data_grad"]["torch"]()[0].permute(0, 2, 3, 1).float()
            torch.cuda.synchronize()
            row["wgrad_max_rel_diff_vs_torch"] = float(((odW - tdW).abs().max() / tdW.abs().max()).cpu())
            row["data_grad_max_rel_diff_vs_torch"] = float(((odx - tdx).abs().max() / tdx.abs().max()).cpu())
        except Exception as e:                                                     # recorded, not replaced by a guess
            row["torch_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
        for what, fns in cases.items():
            print("warm-up", a.dtype, stage, what, sorted(fns), flush=True)
            try:
                with torch.no_grad() if what == "join" else torch.enable_grad():
                    for _ in range(2):
                        for f in fns.values():
                            f()
                    torch.cuda.synchronize()
                    med, raw = series(fns, a.iters, a.repeats)
            except Exception as e:
                row[what + "_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
                continue
            row[what + "_ms"] = med["ours"]
            for k in ("torch", "norepack"):
                if k in med:
                    row["%s_%s_ms" % (what, k)], row["%s_%s_over_ours" % (what, k)] = med[k], med[k] / med["ours"]
            if what == "wgrad":
                row["wgrad_tflops"] = 2 * macs / med["ours"] / 1e9
            if what == "data_grad":
                row["data_grad_tflops"], row["data_grad_useful_tflops"] = 2 * view_macs / med["ours"] / 1e9, 2 * view_macs * 2 / 3 / med["ours"] / 1e9
            row[what + "_series"] = raw
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_series")}), flush=True)
        rows.append(row)
        del up, skip, g, z, cases, st, res, opts
        upt = skt = zt0 = gt = tz = tw = tbw = tsc = None
        torch.cuda.empty_cache()
    out = dict(tool="tools/agg_stage_timing.py", source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               iters=a.iters, repeats=a.repeats, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()

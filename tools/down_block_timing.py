"""Down-sampling BasicBlock timing (dev tool): the stride-(1,2) weight gradient (rd_conv3x3_bwd_weight_ex), the strided conv's data gradient
(TowerOps.data_grad_s2), a whole rangedet_amd.backbone_train.DownBlockTrain forward + backward and the SGD step with the strided images, at
the four strided units of the network, B frames of 64 x Win: 2656 at 64 -> 64 (res2a), 1328 at 64 -> 128 (res2), 664 and 332 at 128 -> 128
(res3a, res3); bf16 unless --dtype f16.

    python tools/down_block_timing.py [--batch 8] [--iters 5] [--repeats 3] [--out profiles/down_block_timing.json]

Baselines, on the very same buffers:
  torch     torch's own conv2d (stride (1, 2)) weight / input gradient and, for the block, conv2d / batch_norm(training=True) / add / relu
            forward and autograd backward, in the same 16-bit type on channels-last views
  compose   (weight gradient only) what the library could do before the entry point: rd_conv3x3_bwd_weight at full width on y1 and a dz with
            zeros interleaved on the odd pixels -- twice the multiply-adds of the strided form; the interleaved dz is made once, outside the
            timed window
  stride1   (SGD step only) the step over the same parameters with the stride-1 images of conv2
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
from rangedet_amd.backbone_train import BasicBlockTrain, DownBlockTrain  # noqa: E402
from rangedet_amd.backward import BN_EPS, BN_MOMENTUM, TowerOps  # noqa: E402
from rangedet_amd.optim import SGD  # noqa: E402
from rangedet_amd.runtime import TorchAllocator  # noqa: E402
from tools.timing_util import series  # noqa: E402

H, SHAPES = 64, ((2656, 64, 64), (1328, 64, 128), (664, 128, 128), (332, 128, 128))


def block_params(cin, cout, rng):
    def bn():
        return (rng.uniform(0.5, 1.5, cout).astype(np.float32), (0.1 * rng.standard_normal(cout)).astype(np.float32), np.zeros(cout, np.float32),
                np.ones(cout, np.float32))
    w = [(rng.standard_normal((cout, c, 3, 3)) / np.sqrt(9 * c / 2)).astype(np.float32) for c in (cin, cout)]
    return w, [bn(), bn(), bn()], (rng.standard_normal((cout, cin, 1, 1)) / np.sqrt(cin)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dtype", choices=("bf16", "f16"), default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "down_block_timing.json"))
    a = ap.parse_args()
    A, L = TorchAllocator(), rdlib.get_lib()
    dev, B = A.device, a.batch
    dt, tdt = (rdlib.RD_BF16, torch.bfloat16) if a.dtype == "bf16" else (rdlib.RD_F16, torch.float16)
    gen = torch.Generator(device="cpu").manual_seed(13)
    rng = np.random.default_rng(5)
    ops = TowerOps(dt, L, A)
    rows = []
    for Win, cin, cout in SHAPES:
        Wo = Win // 2
        x = torch.relu(torch.randn(B * H * Win, cin, generator=gen)).to(dev, tdt).view(B, H, Win, cin)
        y1 = torch.relu(torch.randn(B * H * Win, cout, generator=gen)).to(dev, tdt).view(B, H, Win, cout)
        g = torch.randn(B * H * Wo, cout, generator=gen).to(dev, tdt).view(B, H, Wo, cout)
        w, bns, ws = block_params(cin, cout, rng)
        macs = 9 * B * H * Wo * cout * cout
        row = dict(dtype=a.dtype, B=B, H=H, Win=Win, Wo=Wo, cin=cin, cout=cout, conv2_gmacs=macs / 1e9,
                   wgrad_partials=int(L.raw("rd_conv3x3_bwd_weight_ex_workspace_bytes")(B, H, Win, cout, cout, 2, 0) // (36 * cout * cout)))
        cases = {}
        # (i) the strided weight gradient of conv2 (cout -> cout), against the full-width call on a zero-interleaved dz
        gz = torch.zeros(B, H, Win, cout, device=dev, dtype=tdt)
        gz[:, :, 0::2] = g
        # full width: out[w] pairs with x[w + kx - 1]; the strided conv pairs out[wo] with x[2 wo + kx - 1]: dz on the even pixels
        cases["wgrad_s2"] = dict(ours=lambda: ops.weight_grad(y1, g, tag="t", stride_w=2), compose=lambda: ops.weight_grad(y1, gz, tag="c"))
        # (ii) the data gradient
        packed = ops.pack_data_grad_s2(w[1])
        cases["data_grad_s2"] = dict(ours=lambda: ops.data_grad_s2(g, packed, tag="t"))
        # (iii) the whole block
        blk = DownBlockTrain("timing", w[0], w[1], bns[0], bns[1], ws, bns[2], dtype=dt, lib=L, alloc=A)

        def ours_block():
            blk.forward(x)
            return blk.backward(g)
        cases["block"] = dict(ours=ours_block)
        # (iv) the SGD step: this block's parameters, and a stride-1 projection block of the same parameter count
        flat = BasicBlockTrain("flat", w[0], w[1], bns[0], bns[1], ws, bns[2], dtype=dt, lib=L, alloc=A)
        opts = {}
        for key, b_ in (("ours", blk), ("stride1", flat)):
            opts[key] = SGD(lr=0.0, wd=0.0, lib=L, alloc=A)          # lr 0: the weights stay as they are over the repeats
            opts[key].attach(b_)
        cases["sgd_step"] = {k: o.step for k, o in opts.items()}
        try:
            nc = lambda v: v.permute(0, 3, 1, 2)
            xt, y1t = (nc(v).detach().requires_grad_(True) for v in (x, y1))
            gt = nc(g)
            tw = [torch.from_numpy(v).to(dev, tdt).contiguous(memory_format=torch.channels_last).requires_grad_(True) for v in (w[0], w[1], ws)]
            tb = [torch.from_numpy(v).to(dev).requires_grad_(True) for b_ in bns for v in b_[:2]]
            tz2 = F.conv2d(y1t, tw[1], padding=1, stride=(1, 2))
            cases["wgrad_s2"]["torch"] = lambda: torch.autograd.grad(tz2, tw[1], gt, retain_graph=True)
            cases["data_grad_s2"]["torch"] = lambda: torch.autograd.grad(tz2, y1t, gt, retain_graph=True)
            bnf = lambda v, ga, be: F.batch_norm(v, None, None, ga, be, training=True, momentum=1 - BN_MOMENTUM, eps=BN_EPS)

            def t_block():
                t1 = torch.relu(bnf(F.conv2d(xt, tw[0], padding=1), tb[0], tb[1]))
                main = bnf(F.conv2d(t1, tw[1], padding=1, stride=(1, 2)), tb[2], tb[3])
                short = bnf(F.conv2d(xt, tw[2], stride=(1, 2)), tb[4], tb[5])
                return torch.autograd.grad(torch.relu(main + short), [xt] + tw + tb, gt)
            cases["block"]["torch"] = t_block
            odW, cdW, tdW = cases["wgrad_s2"]["ours"]().clone(), cases["wgrad_s2"]["compose"]().clone(), cases["wgrad_s2"]["torch"]()[0].float()
            og1, tg1 = cases["data_grad_s2"]["ours"]().float(), cases["data_grad_s2"]["torch"]()[0].permute(0, 2, 3, 1).float()
            torch.cuda.synchronize()
            row["wgrad_s2_max_rel_diff_vs_torch"] = float(((odW - tdW).abs().max() / tdW.abs().max()).cpu())
            row["wgrad_s2_max_rel_diff_vs_compose"] = float(((odW - cdW).abs().max() / cdW.abs().max()).cpu())
            row["data_grad_s2_max_rel_diff_vs_torch"] = float(((og1 - tg1).abs().max() / tg1.abs().max()).cpu())
        except Exception as e:                                                     # recorded, not replaced by a guess
            row["torch_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
        for what, fns in cases.items():
            print("warm-up", a.dtype, Win, cin, cout, what, sorted(fns), flush=True)
            try:
                for _ in range(2):
                    for f in fns.values():
                        f()
                torch.cuda.synchronize()
                med, raw = series(fns, a.iters, a.repeats)
            except Exception as e:
                row[what + "_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
                continue
            row[what + "_ms"] = med["ours"]
            for k in ("torch", "compose", "stride1"):
                if k in med:
                    row["%s_%s_ms" % (what, k)], row["%s_%s_over_ours" % (what, k)] = med[k], med[k] / med["ours"]
            if what in ("wgrad_s2", "data_grad_s2"):
                row[what + "_tflops"] = 2 * macs / med["ours"] / 1e9
            row[what + "_series"] = raw
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_series")}), flush=True)
        rows.append(row)
        del x, y1, g, gz, cases, blk, flat, opts
        xt = y1t = gt = tz2 = tw = None
        torch.cuda.empty_cache()
    res = dict(tool="tools/down_block_timing.py", source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               iters=a.iters, repeats=a.repeats, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()

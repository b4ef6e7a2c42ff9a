"""Meta-Kernel backward timing (dev tool): the data-gradient kernel (rd_meta_kernel_bwd_data), the parameter-gradient kernel with its
reduction (rd_meta_kernel_bwd_params), a whole rangedet_amd.backward.MetaUnitBackward forward + backward, and rd_meta_kernel_fwd alone, at
res1_unit2's shape: B frames of 64 x 2656, 64 channels, in bf16 and fp16.

    python tools/meta_backward_timing.py [--batch 8] [--iters 3] [--repeats 3] [--out profiles/meta_bwd_timing.json]

Baseline, on the very same inputs: torch autograd of the UN-FUSED formulation (unfold, two 1x1 convs, the 576-channel product, affine, ReLU,
the 576 -> 64 conv) in the same 16-bit type on the same GPU -- it keeps several (B, 576, H, W) tensors alive.  `torch_data` / `torch_params`
are autograd.grad of z w.r.t. the data / the parameters on a retained graph (backward only), `torch_unit` is forward + backward of everything.
Algorithmic multiply-adds per pixel (8 MLP taps, 9 product taps):
    mlp    = 8 (32 * 3 + 64 * 32)                     the 3 -> 32 -> 64 MLP, recomputed by both backward kernels
    fwd    = mlp + 576 + 64 * 576                     rd_meta_kernel_fwd
    data   = mlp + 64 * 576 + 2 * 576                 A_k^T dz and the element-wise products
    params = mlp + 2 * 64 * 576 + 8 * 2 * 64 * 32     A_k^T dz, dz (x) a, e (x) h and (s1 W1)^T e
achieved FLOP/s = 2 * multiply-adds / time.  If the baseline cannot run, the error is recorded and no number is invented.  Each figure is
the median over `repeats` windows of `iters` calls between device events, after a warm-up of every side; the windows alternate and the series
is run in both orders, all in this one process (tools/timing_util.py).  Not profiled: no hardware counters; end-to-end launch windows only."""
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
from rangedet_amd.backward import MetaUnitBackward  # noqa: E402
from rangedet_amd.runtime import TorchAllocator  # noqa: E402
from tools.timing_util import series  # noqa: E402

H, W, NAME = 64, 2656, "res1_unit2"
MLP = 8 * (32 * 3 + 64 * 32)
MACS = dict(fwd=MLP + 576 + 64 * 576, data=MLP + 64 * 576 + 2 * 576, params=MLP + 2 * 64 * 576 + 8 * 2 * 64 * 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meta_bwd_timing.json"))
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
        unit = MetaUnitBackward(NAME, P, W, dtype=dt, lib=L, alloc=A)
        o = unit.ops
        unit.forward(data, coord)
        unit.backward(g)
        dz = unit.dz
        row = dict(dtype=dname, B=B, H=H, W=W, macs_per_pixel=MACS, workspace_bytes=int(L.raw("rd_meta_kernel_bwd_workspace_bytes")(B, H, W, 0)))

        def ours_unit():
            unit.forward(data, coord)
            return unit.backward(g)
        cases = dict(fwd=dict(ours=lambda: o.meta_forward(data, coord, unit.packed_fwd)),
                     data=dict(ours=lambda: o.meta_data_grad(dz, data, coord, unit.packed_bwd)),
                     params=dict(ours=lambda: o.meta_param_grads(dz, data, coord, unit.packed_bwd)), unit=dict(ours=ours_unit))
        try:
            prm = unit.prm
            tp = {k: torch.from_numpy(np.ascontiguousarray(prm[k])).to(dev, tdt).requires_grad_(True) for k in ("w0", "b0", "w1", "b1", "s1", "t1", "agg")}
            xt = data.permute(0, 3, 1, 2).detach().requires_grad_(True)
            s2 = torch.from_numpy(prm["s2"]).to(dev, tdt).view(1, 64, 1, 1)
            t2 = torch.from_numpy(prm["t2"]).to(dev, tdt).view(1, 64, 1, 1)
            dzt, gt = dz.permute(0, 3, 1, 2), g.permute(0, 3, 1, 2)

            def t_z():
                cs = F.unfold(coord, 3, padding=1).view(B, 3, 9, H, W)
                rel = (cs - coord.unsqueeze(2)).to(tdt).reshape(B, 3, 9 * H, W)
                h = torch.relu(F.conv2d(rel, tp["w0"].view(32, 3, 1, 1), tp["b0"]))
                w = F.conv2d(h, tp["w1"].view(64, 32, 1, 1), tp["b1"]).view(B, 64, 9, H, W)
                ds = F.unfold(xt, 3, padding=1).view(B, 64, 9, H, W)
                act = torch.relu((ds * w).reshape(B, 576, H, W) * tp["s1"].view(1, 576, 1, 1) + tp["t1"].view(1, 576, 1, 1))
                return F.conv2d(act, tp["agg"].view(64, 576, 1, 1))
            z = t_z()
            plist = list(tp.values())
            cases["data"]["torch"] = lambda: torch.autograd.grad(z, xt, dzt, retain_graph=True)
            cases["params"]["torch"] = lambda: torch.autograd.grad(z, plist, dzt, retain_graph=True)
            cases["unit"]["torch"] = lambda: torch.autograd.grad(torch.relu(t_z() * s2 + t2), [xt] + plist, gt)
            cases["fwd"]["torch"] = lambda: torch.relu(t_z() * s2 + t2)            # (timed under no_grad: the forward alone)
            od, td = cases["data"]["ours"]().float(), cases["data"]["torch"]()[0].permute(0, 2, 3, 1).float()
            torch.cuda.synchronize()
            row["data_grad_max_rel_diff_vs_torch"] = float(((od - td).abs().max() / td.abs().max()).cpu())
        except Exception as e:                                                     # recorded, not replaced by a guess
            row["torch_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
            for c in cases.values():
                c.pop("torch", None)
        for what, fns in cases.items():
            print("warm-up", dname, what, sorted(fns), flush=True)
            try:
                with torch.no_grad() if what == "fwd" else torch.enable_grad():
                    for f in fns.values():
                        f()
                    torch.cuda.synchronize()
                    med, raw = series(fns, a.iters, a.repeats)
            except Exception as e:
                row[what + "_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
                continue
            row[what + "_ms"] = med["ours"]
            if "torch" in med:
                row[what + "_torch_ms"], row[what + "_torch_over_ours"] = med["torch"], med["torch"] / med["ours"]
            if what in MACS:
                row[what + "_tflops"] = 2 * MACS[what] * npix / med["ours"] / 1e9
            row[what + "_series"] = raw
        if "unit_ms" in row and "fwd_ms" in row:
            row["unit_over_fwd"] = row["unit_ms"] / row["fwd_ms"]
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_series")}), flush=True)
        rows.append(row)
        del cases, unit, data, g, dz
        z = xt = dzt = gt = tp = plist = None
        torch.cuda.empty_cache()
    out = dict(tool="tools/meta_backward_timing.py", source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               iters=a.iters, repeats=a.repeats, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()

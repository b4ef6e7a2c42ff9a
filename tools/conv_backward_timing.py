"""Head-tower backward timing (dev tool): the weight-gradient launch (rd_conv3x3_bwd_weight) and the output-conv backward
(rd_head_out_bwd, nout 8, fused mask and scale) at the three tower shapes, B frames of 64 x {2656, 1328, 664}, 128 -> 128, in both
16-bit types.  Baseline of the weight gradient: torch's own conv backward on the same device, shape and type, channels-last
(torch.nn.grad.conv2d_weight on views of the very same buffers).  If that cannot run, the error is recorded and no number is invented.

    python tools/conv_backward_timing.py [--batch 8] [--iters 10] [--repeats 5] [--out profiles/conv_backward_timing.json]

Each figure is the median over `repeats` windows of `iters` calls between device events, after a warm-up of both sides; the windows
alternate ours / torch and the series is run in both orders, all in this one process.  TFLOP/s = 2 B H W 9 cin cout / time, against the
2.5 PFLOP/s dense 16-bit peak bench.py uses; the output-conv backward is reported in GB/s of the bytes it has to move (x and dx in the
activation type, d_out in float32)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rangedet_amd import build, lib as rdlib  # noqa: E402
from rangedet_amd.backward import TowerOps  # noqa: E402
from rangedet_amd.runtime import TorchAllocator  # noqa: E402
from tools.timing_util import series  # noqa: E402

H, WIDTHS, C, NOUT, PEAK = 64, (2656, 1328, 664), 128, 8, 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_backward_timing.json"))
    a = ap.parse_args()
    A, L = TorchAllocator(), rdlib.get_lib()
    dev, B = A.device, a.batch
    g = torch.Generator(device="cpu").manual_seed(7)
    rows = []
    for dt, tdt, name in ((rdlib.RD_BF16, torch.bfloat16, "bf16"), (rdlib.RD_F16, torch.float16, "f16")):
        ops = TowerOps(dt, L, A)
        for W in WIDTHS:
            n = B * H * W
            x = torch.relu(torch.randn(n, C, generator=g)).to(dev, tdt).view(B, H, W, C)          # post-ReLU activations: half zeros
            dz = torch.randn(n, C, generator=g).to(dev, tdt).view(B, H, W, C)
            d_out = torch.randn(B, H * W * NOUT, generator=g).to(dev)
            w_out = A.upload((np.random.default_rng(1).standard_normal((NOUT, C)) / np.sqrt(C)).astype(np.float32))
            scale = A.upload(np.random.default_rng(2).uniform(0.5, 1.5, C).astype(np.float32))
            row = dict(dtype=name, B=B, H=H, W=W, cin=C, cout=C, flop=2.0 * n * 9 * C * C,
                       split=int(L.raw("rd_conv3x3_bwd_weight_workspace_bytes")(B, H, W, C, C, 0) // (36 * C * C)))
            ours = lambda: ops.weight_grad(x, dz)                                                  # noqa: E731
            hob = lambda: ops.head_out_bwd(d_out, x, w_out, NOUT, scale=scale, relu_mask=True)     # noqa: E731
            fns = {"ours": ours}
            xt, gt = x.permute(0, 3, 1, 2), dz.permute(0, 3, 1, 2)                                 # NCHW views, channels-last memory
            ref = lambda: torch.nn.grad.conv2d_weight(xt, (C, C, 3, 3), gt, stride=1, padding=1)   # noqa: E731
            try:
                want = ref().float()
                got = ours()
                torch.cuda.synchronize()
                row["max_abs_diff_vs_torch"] = float((got - want).abs().max().cpu())
                row["max_abs_torch"] = float(want.abs().max().cpu())
                fns["torch"] = ref
            except Exception as e:                                                                 # recorded, not replaced by a guess
                row["torch_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
            print("warm-up", name, W, sorted(fns), flush=True)
            for _ in range(3):
                for f in list(fns.values()) + [hob]:
                    f()
            torch.cuda.synchronize()
            med, raw = series(fns, a.iters, a.repeats)
            row["weight_grad_ms"], row["weight_grad_tflops"] = med["ours"], row["flop"] / med["ours"] / 1e9
            row["weight_grad_fraction_of_peak"] = row["flop"] / (med["ours"] * 1e-3) / PEAK
            if "torch" in med:
                row["torch_weight_grad_ms"], row["torch_weight_grad_tflops"] = med["torch"], row["flop"] / med["torch"] / 1e9
                row["torch_over_ours"] = med["torch"] / med["ours"]
            row["weight_grad_series"] = raw
            hmed, hraw = series({"head_out_bwd": hob}, a.iters, a.repeats)
            nbytes = n * (2 * C * 2 + NOUT * 4)
            row["head_out_bwd_ms"], row["head_out_bwd_gbps"], row["head_out_bwd_series"] = hmed["head_out_bwd"], nbytes / hmed["head_out_bwd"] / 1e6, hraw
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_series")}), flush=True)
            rows.append(row)
            del x, dz, d_out, xt, gt
            torch.cuda.empty_cache()
    res = dict(tool="tools/conv_backward_timing.py", source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               iters=a.iters, repeats=a.repeats, peak_flops=PEAK, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()

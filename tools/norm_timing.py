"""Training-mode batch-norm timing (dev tool): the forward (rd_bn_stats + rd_bn_fold + rd_affine_relu) and the backward (rd_bn_relu_bwd) of one
head-tower layer at the three tower shapes, B frames of 64 x {2656, 1328, 664}, 128 channels, in both 16-bit types.  Baseline: torch's own
batch_norm(training=True) + relu, forward and backward, on channels-last views of the very same buffers.  If that cannot run, the error is
recorded and no number is invented.

    python tools/norm_timing.py [--batch 8] [--iters 10] [--repeats 5] [--out profiles/norm_timing.json]

Each figure is the median over `repeats` windows of `iters` calls between device events, after a warm-up of both sides; the windows
alternate ours / torch and the series is run in both orders, all in this one process.  GB/s are those of the compulsory bytes -- forward:
read z for the statistics, read z and write y (3 tensor passes); backward: read g and z for the sums, read g and z and write dz (5 passes) --
against the 8 TB/s HBM peak bench.py uses.  torch's figures are given over the same byte counts."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rangedet_amd import build, lib as rdlib  # noqa: E402
from rangedet_amd.backward import BN_EPS, BN_MOMENTUM, TowerOps  # noqa: E402
from rangedet_amd.runtime import TorchAllocator  # noqa: E402
from tools.timing_util import series  # noqa: E402

H, WIDTHS, C, PEAK_HBM_GBPS = 64, (2656, 1328, 664), 128, 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "norm_timing.json"))
    a = ap.parse_args()
    A, L = TorchAllocator(), rdlib.get_lib()
    dev, B = A.device, a.batch
    gen = torch.Generator(device="cpu").manual_seed(7)
    rng = np.random.default_rng(1)
    gamma_h, beta_h = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.normal(0, 0.1, C).astype(np.float32)
    rows = []
    for dt, tdt, name in ((rdlib.RD_BF16, torch.bfloat16, "bf16"), (rdlib.RD_F16, torch.float16, "f16")):
        ops = TowerOps(dt, L, A)
        gamma, beta = A.upload(gamma_h), A.upload(beta_h)
        mm, mv = A.upload(np.zeros(C, np.float32)), A.upload(np.ones(C, np.float32))
        for W in WIDTHS:
            n = B * H * W
            z = (0.3 + torch.randn(n, C, generator=gen)).to(dev, tdt).view(B, H, W, C)
            g = torch.randn(n, C, generator=gen).to(dev, tdt).view(B, H, W, C)
            tensor_bytes = n * C * 2
            row = dict(dtype=name, B=B, H=H, W=W, C=C, tensor_mb=tensor_bytes / 1e6, forward_bytes=3 * tensor_bytes, backward_bytes=5 * tensor_bytes,
                       partials=int(L.raw("rd_bn_stats_workspace_bytes")(B, H, W, C, 0) // (12 * C)))
            saved = {}

            def fwd():
                mean, var = ops.bn_stats(z)
                rstd, sa, sb = ops.bn_fold(mean, var, gamma, beta, mm, mv, n, C, BN_EPS, BN_MOMENTUM)
                saved.update(a=sa, b=sb, mean=mean, var=var, rstd=rstd)
                return ops.affine_relu(z, sa, sb)

            def bwd():
                return ops.bn_relu_bwd(g, z, saved, gamma)
            ffn, bfn = {"ours": fwd}, {"ours": bwd}
            try:
                zt = z.permute(0, 3, 1, 2).detach().requires_grad_(True)              # NCHW view, channels-last memory
                gt = g.permute(0, 3, 1, 2)
                tg, tb = (torch.from_numpy(v).to(dev).requires_grad_(True) for v in (gamma_h, beta_h))
                rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)

                def tfwd():
                    return torch.relu(torch.nn.functional.batch_norm(zt, rm, rv, tg, tb, training=True, momentum=1 - BN_MOMENTUM, eps=BN_EPS))
                with torch.no_grad():
                    want = tfwd().permute(0, 2, 3, 1).float()
                    got = fwd().float()
                    torch.cuda.synchronize()
                    row["forward_max_abs_diff_vs_torch"] = float((got - want).abs().max().cpu())
                    del want, got
                ty = tfwd()

                def tbwd():
                    return torch.autograd.grad(ty, (zt, tg, tb), gt, retain_graph=True)
                wdz, wdg, wdb = tbwd()
                odz, odg, odb = bwd()
                torch.cuda.synchronize()
                row["dz_max_abs_diff_vs_torch"] = float((odz.float() - wdz.permute(0, 2, 3, 1).float()).abs().max().cpu())
                row["dgamma_max_rel_diff_vs_torch"] = float(((odg - wdg).abs().max() / wdg.abs().max()).cpu())
                row["dbeta_max_rel_diff_vs_torch"] = float(((odb - wdb).abs().max() / wdb.abs().max()).cpu())
                del wdz, odz

                def tfwd_nograd():
                    with torch.no_grad():
                        return tfwd()
                ffn["torch"], bfn["torch"] = tfwd_nograd, tbwd
            except Exception as e:                                                     # recorded, not replaced by a guess
                row["torch_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
            print("warm-up", name, W, sorted(ffn), flush=True)
            for _ in range(3):
                for f in list(ffn.values()) + list(bfn.values()):
                    f()
            torch.cuda.synchronize()
            for what, fns, nbytes in (("forward", ffn, 3 * tensor_bytes), ("backward", bfn, 5 * tensor_bytes)):
                med, raw = series(fns, a.iters, a.repeats)
                row[what + "_ms"], row[what + "_gbps"] = med["ours"], nbytes / med["ours"] / 1e6
                row[what + "_fraction_of_hbm_peak"] = row[what + "_gbps"] / PEAK_HBM_GBPS
                if "torch" in med:
                    row["torch_" + what + "_ms"], row["torch_" + what + "_gbps"] = med["torch"], nbytes / med["torch"] / 1e6
                    row[what + "_torch_over_ours"] = med["torch"] / med["ours"]
                row[what + "_series"] = raw
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_series")}), flush=True)
            rows.append(row)
            del z, g
            zt = gt = ty = None
            torch.cuda.empty_cache()
    res = dict(tool="tools/norm_timing.py", source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               iters=a.iters, repeats=a.repeats, peak_hbm_gbps=PEAK_HBM_GBPS, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()

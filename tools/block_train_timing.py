"""Training-mode BasicBlock timing (dev tool): the residual batch norm forward (rd_affine_add_relu) and backward (rd_bn_add_relu_bwd, identity
and projection shortcut), the 1x1 weight gradient (rd_conv1x1_bwd_weight) and a whole rangedet_amd.backbone_train.BasicBlockTrain forward +
backward at the five backbone shapes, B frames of 64 x {2656, 1328} at 64 channels and 64 x {664, 332, 166} at 128, in both 16-bit types.

    python tools/block_train_timing.py [--batch 8] [--iters 5] [--repeats 3] [--out profiles/block_train_timing.json]

Two baselines, on the very same buffers:
  torch     torch's own conv2d / batch_norm(training=True) / add / relu, forward and autograd backward, in the same 16-bit type on
            channels-last views
  compose   what the library could do before these entry points: rd_affine_relu(relu=0) and rd_bn_relu_bwd(relu=0), with torch for the add,
            the ReLU, the mask ((y > 0) * g) and -- for a projection -- a second rd_bn_relu_bwd(relu=0) on the shortcut; the whole block the
            same way, with torch's matmul for the 1x1 weight gradient and a torch add for dx.  (The 1x1 weight gradient alone has no such
            composition: there was no library call for it.)
If a baseline cannot run, the error is recorded and no number is invented.  Each figure is the median over `repeats` windows of `iters`
calls between device events, after a warm-up of every side; the windows alternate and the series is run in both orders, all in this one
process (tools/timing_util.py).  TB/s are those of the compulsory tensor passes -- forward: read z, read r, write y (3); backward: two reads
each of g, z and r and the writes of dz and dr (8) -- against the 8 TB/s HBM peak bench.py uses.  Not profiled: no hardware counters, no
per-kernel split of the three launches of the backward, no occupancy or cache figures; the times are end-to-end launch windows only."""
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
from rangedet_amd.backbone_train import BasicBlockTrain  # noqa: E402
from rangedet_amd.backward import BN_EPS, BN_MOMENTUM, TowerOps  # noqa: E402
from rangedet_amd.runtime import TorchAllocator  # noqa: E402
from tools.timing_util import series  # noqa: E402

H, SHAPES, PEAK_HBM_GBPS = 64, ((2656, 64), (1328, 64), (664, 128), (332, 128), (166, 128)), 8000.0


def fold(ops, A, z, gamma, beta, C, n, tag):
    mean, var = ops.bn_stats(z, tag=tag)
    rstd, a, b = ops.bn_fold(mean, var, gamma, beta, None, None, n, C, BN_EPS, BN_MOMENTUM, tag=tag)
    return dict(a=a, b=b, mean=mean, var=var, rstd=rstd)


def block_params(C, proj, rng):
    def bn():
        return (rng.uniform(0.5, 1.5, C).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32), np.zeros(C, np.float32), np.ones(C, np.float32))
    w = [(rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C / 2)).astype(np.float32) for _ in range(2)]
    ws = (rng.standard_normal((C, C, 1, 1)) / np.sqrt(C)).astype(np.float32) if proj else None
    return w, [bn(), bn(), bn()], ws


def composed_step(blk, x, g):
    """BasicBlockTrain.forward + backward with the residual steps composed from the older calls and torch"""
    o, cv, bn, C = blk.ops, blk.convs, blk.bns, blk.cout
    n = int(np.prod(x.shape[:3]))
    z1 = o.conv_unscaled(x, cv["conv1"]["fwd"], blk.cin, C, tag=1)
    s1 = fold(o, o.A, z1, bn["bn1"]["gamma"], bn["bn1"]["beta"], C, n, 1)
    y1 = o.affine_relu(z1, s1["a"], s1["b"], tag=1)
    z2 = o.conv_unscaled(y1, cv["conv2"]["fwd"], C, C, tag=2)
    s2 = fold(o, o.A, z2, bn["bn2"]["gamma"], bn["bn2"]["beta"], C, n, 2)
    t = o.affine_relu(z2, s2["a"], s2["b"], relu=False, tag=2)
    if blk.proj:
        zs = o.conv1x1(x, cv["sc"]["fwd"], blk.cin, C, ("zs", 0))
        ss = fold(o, o.A, zs, bn["sc_bn"]["gamma"], bn["sc_bn"]["beta"], C, n, "s")
        u = o.affine_relu(zs, ss["a"], ss["b"], relu=False, tag="s")
    else:
        u = x
    y = torch.relu(t + u)
    gy = g * (y > 0)
    dz2, dg2, db2 = o.bn_relu_bwd(gy, z2, s2, bn["bn2"]["gamma"], relu=False, tag=2)
    dW2 = o.weight_grad(y1, dz2, tag=2)
    g1 = o.data_grad(dz2, cv["conv2"]["bwd"], tag=2)
    dz1, dg1, db1 = o.bn_relu_bwd(g1, z1, s1, bn["bn1"]["gamma"], tag=1)
    dW1 = o.weight_grad(x, dz1, tag=1)
    if blk.proj:
        dr, dgs, dbs = o.bn_relu_bwd(gy, zs, ss, bn["sc_bn"]["gamma"], relu=False, tag="s")
        dWs = torch.matmul(dr.reshape(n, C).t(), x.reshape(n, blk.cin)).float()
        short = o.conv1x1(dr, cv["sc"]["bwd"], C, blk.cin, ("ds", 0))
    else:
        short = gy
    return o.data_grad(dz1, cv["conv1"]["bwd"], tag=1) + short


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_train_timing.json"))
    a = ap.parse_args()
    A, L = TorchAllocator(), rdlib.get_lib()
    dev, B = A.device, a.batch
    gen = torch.Generator(device="cpu").manual_seed(11)
    rng = np.random.default_rng(3)
    rows = []
    for dt, tdt, name in ((rdlib.RD_BF16, torch.bfloat16, "bf16"), (rdlib.RD_F16, torch.float16, "f16")):
        ops = TowerOps(dt, L, A)
        for W, C in SHAPES:
            n = B * H * W
            z, r, g = ((s + torch.randn(n, C, generator=gen)).to(dev, tdt).view(B, H, W, C) for s in (0.3, 0.0, 0.0))
            x = torch.relu(torch.randn(n, C, generator=gen)).to(dev, tdt).view(B, H, W, C)
            gam = [rng.uniform(0.5, 1.5, C).astype(np.float32) for _ in range(2)]
            bet = [rng.normal(0, 0.1, C).astype(np.float32) for _ in range(2)]
            gamma, beta, gamma_r, beta_r = A.upload(gam[0]), A.upload(bet[0]), A.upload(gam[1]), A.upload(bet[1])
            sv, svr = fold(ops, A, z, gamma, beta, C, n, 0), fold(ops, A, r, gamma_r, beta_r, C, n, "r")
            tensor_bytes = n * C * 2
            row = dict(dtype=name, B=B, H=H, W=W, C=C, tensor_mb=tensor_bytes / 1e6, forward_bytes=3 * tensor_bytes, backward_bytes=8 * tensor_bytes,
                       bn_partials=int(L.raw("rd_bn_add_relu_bwd_workspace_bytes")(B, H, W, C, 0, 0) // (8 * C)),
                       wgrad1x1_partials=int(L.raw("rd_conv1x1_bwd_weight_workspace_bytes")(B, H, W, C, C, 0) // (4 * C * C)))
            cases = {}
            # ---- kernels: ours and the composition
            cases["add_relu_identity"] = dict(ours=lambda: ops.affine_add_relu(z, sv["a"], sv["b"], r),
                                              compose=lambda: torch.relu(ops.affine_relu(z, sv["a"], sv["b"], relu=False) + r))
            cases["add_relu_projection"] = dict(ours=lambda: ops.affine_add_relu(z, sv["a"], sv["b"], r, svr["a"], svr["b"]),
                                                compose=lambda: torch.relu(ops.affine_relu(z, sv["a"], sv["b"], relu=False)
                                                                           + ops.affine_relu(r, svr["a"], svr["b"], relu=False, tag="r")))
            y_id, y_pr = cases["add_relu_identity"]["ours"]().clone(), cases["add_relu_projection"]["ours"]().clone()

            def comp_bwd(y, proj):
                gy = g * (y > 0)
                out = ops.bn_relu_bwd(gy, z, sv, gamma, relu=False)
                return (out, ops.bn_relu_bwd(gy, r, svr, gamma_r, relu=False, tag="r")) if proj else (out, gy)
            cases["add_bwd_identity"] = dict(ours=lambda: ops.bn_add_relu_bwd(g, z, r, sv, gamma), compose=lambda: comp_bwd(y_id, False))
            cases["add_bwd_projection"] = dict(ours=lambda: ops.bn_add_relu_bwd(g, z, r, sv, gamma, svr, gamma_r), compose=lambda: comp_bwd(y_pr, True))
            cases["wgrad1x1"] = dict(ours=lambda: ops.weight_grad1x1(x, g))
            blocks = {}
            for proj in (False, True):
                w, bns, ws = block_params(C, proj, rng)
                blk = BasicBlockTrain("timing", w[0], w[1], bns[0], bns[1], ws, bns[2] if proj else None, dtype=dt, lib=L, alloc=A)
                blocks[proj] = (blk, w, bns, ws)

                def ours_block(blk=blk):
                    blk.forward(x)
                    return blk.backward(g)
                cases["block_" + ("projection" if proj else "identity")] = dict(ours=ours_block, compose=lambda blk=blk: composed_step(blk, x, g))
            # ---- torch on channels-last views of the same buffers
            try:
                nc = lambda v: v.permute(0, 3, 1, 2)
                zt, rt, xt = (nc(v).detach().requires_grad_(True) for v in (z, r, x))
                gt = nc(g)
                tp = [torch.from_numpy(v).to(dev).requires_grad_(True) for v in (gam[0], bet[0], gam[1], bet[1])]
                bnf = lambda v, ga, be: F.batch_norm(v, None, None, ga, be, training=True, momentum=1 - BN_MOMENTUM, eps=BN_EPS)

                def t_id():
                    return torch.relu(bnf(zt, tp[0], tp[1]) + rt)

                def t_pr():
                    return torch.relu(bnf(zt, tp[0], tp[1]) + bnf(rt, tp[2], tp[3]))
                with torch.no_grad():
                    row["add_relu_identity_max_abs_diff_vs_torch"] = float((y_id.float() - t_id().permute(0, 2, 3, 1).float()).abs().max().cpu())
                    row["add_relu_projection_max_abs_diff_vs_torch"] = float((y_pr.float() - t_pr().permute(0, 2, 3, 1).float()).abs().max().cpu())
                ty_id, ty_pr = t_id(), t_pr()
                nog = lambda f: (lambda: _nograd(f))
                cases["add_relu_identity"]["torch"], cases["add_relu_projection"]["torch"] = nog(t_id), nog(t_pr)
                cases["add_bwd_identity"]["torch"] = lambda: torch.autograd.grad(ty_id, (zt, tp[0], tp[1], rt), gt, retain_graph=True)
                cases["add_bwd_projection"]["torch"] = lambda: torch.autograd.grad(ty_pr, (zt, tp[0], tp[1], rt, tp[2], tp[3]), gt, retain_graph=True)
                tw1 = torch.randn(C, C, 1, 1, generator=gen).to(dev, tdt).requires_grad_(True)
                tzs = F.conv2d(xt, tw1)
                cases["wgrad1x1"]["torch"] = lambda: torch.autograd.grad(tzs, tw1, gt, retain_graph=True)
                odW = cases["wgrad1x1"]["ours"]()
                wdW = cases["wgrad1x1"]["torch"]()[0]
                torch.cuda.synchronize()
                row["wgrad1x1_max_rel_diff_vs_torch"] = float(((odW - wdW.float()).abs().max() / wdW.float().abs().max()).cpu())
                for proj in (False, True):
                    blk, w, bns, ws = blocks[proj]
                    tw = [torch.from_numpy(v).to(dev, tdt).contiguous(memory_format=torch.channels_last).requires_grad_(True) for v in w + ([ws] if proj else [])]
                    tb = [torch.from_numpy(v).to(dev).requires_grad_(True) for b_ in bns[:3 if proj else 2] for v in b_[:2]]

                    def t_block(tw=tw, tb=tb, proj=proj):
                        y1 = torch.relu(bnf(F.conv2d(xt, tw[0], padding=1), tb[0], tb[1]))
                        main = bnf(F.conv2d(y1, tw[1], padding=1), tb[2], tb[3])
                        short = bnf(F.conv2d(xt, tw[2]), tb[4], tb[5]) if proj else xt
                        return torch.autograd.grad(torch.relu(main + short), [xt] + tw + tb, gt)
                    cases["block_" + ("projection" if proj else "identity")]["torch"] = t_block
            except Exception as e:                                                     # recorded, not replaced by a guess
                row["torch_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
            for what, fns in cases.items():
                print("warm-up", name, W, C, what, sorted(fns), flush=True)
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
                for k in ("torch", "compose"):
                    if k in med:
                        row["%s_%s_ms" % (what, k)], row["%s_%s_over_ours" % (what, k)] = med[k], med[k] / med["ours"]
                nbytes = 3 * tensor_bytes if what.startswith("add_relu") else 8 * tensor_bytes if what.startswith("add_bwd") else None
                if nbytes:
                    row[what + "_tbps"] = nbytes / med["ours"] / 1e9
                    row[what + "_fraction_of_hbm_peak"] = nbytes / med["ours"] / 1e6 / PEAK_HBM_GBPS
                row[what + "_series"] = raw
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_series")}), flush=True)
            rows.append(row)
            del z, r, g, x, cases, blocks
            zt = rt = xt = gt = ty_id = ty_pr = tzs = None
            torch.cuda.empty_cache()
    res = dict(tool="tools/block_train_timing.py", source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               iters=a.iters, repeats=a.repeats, peak_hbm_gbps=PEAK_HBM_GBPS, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("written", a.out)


def _nograd(f):
    with torch.no_grad():
        return f()


if __name__ == "__main__":
    main()

"""Timing of the training path of the convs that read the range image (dev tool): the narrow weight gradient (rd_conv_bwd_weight_narrow)
8 -> 64 at ksize 3 and 1 and 8 -> 128 at ksize 3, the concat weight gradient 64 + 8 -> 128 (rd_conv3x3_bwd_weight_cat), a whole
rangedet_amd.backbone_train.StemBlockTrain and a whole rangedet_amd.backward.Level0TowerTrain forward + backward, and the SGD step with and
without the new re-pack launches, at B frames of 64 x 2656 in both 16-bit types:

    python tools/narrow_conv_timing.py [--batch 8] [--iters 5] [--repeats 3] [--out profiles/narrow_train_timing.json]

Baselines, on the very same buffers:
  torch     torch's own conv weight gradient in the same 16-bit type on channels-last views (for the two classes: the forward with autograd
            backward of conv / batch_norm / relu)
  padded    the only route the library had before: x zero-padded to 64 channels, then rd_conv3x3_bwd_weight or rd_conv1x1_bwd_weight (the
            padding copy is made once, outside the timed window); for the concat: the 64-channel call on x1 plus the padded call on x2
  norepack  (SGD step only) the step over the same parameters with the narrow / concat weights registered without images
For every kernel figure: the achieved bytes/s of the compulsory traffic (x slot + dz, each read once), the TFLOP/s of the padded-slot
arithmetic the kernel actually issues (16 slot channels per tap), and which of the two roofs -- 6.29 TB/s measured HBM copy rate, 2.5 PFLOP/s
dense 16-bit MFMA -- gives the longer time for that case, i.e. bounds it.  The HBM roof is the measured copy rate, not the 8 TB/s peak.  The
concat's bound is nominal: its flops count 64 + 16 channels once, while its wide half is rd_conv3x3_bwd_weight's kernel, one launch of three
tap-column workgroups that reads dz three times.  If a baseline cannot run, the error is recorded and no number is
invented.  Each figure is the median over `repeats` windows of `iters` calls between device events, after a warm-up of every side; the
windows alternate and the series is run in both orders, all in this one process (tools/timing_util.py).  Not profiled: no hardware
counters; the times are end-to-end launch windows (kernel + reduce)."""
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
from rangedet_amd.backbone_train import StemBlockTrain  # noqa: E402
from rangedet_amd.backward import BN_EPS, BN_MOMENTUM, Level0TowerTrain, TowerOps  # noqa: E402
from rangedet_amd.optim import SGD  # noqa: E402
from rangedet_amd.runtime import TorchAllocator  # noqa: E402
from tools.timing_util import series  # noqa: E402

H, W, C, SLOT = 64, 2656, 8, 16
HBM_BPS, MFMA_FLOPS = 6.29e12, 2.5e15          # MI355X: measured HBM copy rate, dense 16-bit MFMA peak


def bn_params(n, rng):
    return (rng.uniform(0.5, 1.5, n).astype(np.float32), (0.1 * rng.standard_normal(n)).astype(np.float32), np.zeros(n, np.float32),
            np.ones(n, np.float32))


def roofs(row, what, ms, nbytes, flops):
    t_b, t_f = nbytes / HBM_BPS * 1e3, flops / MFMA_FLOPS * 1e3
    row[what + "_compulsory_bytes"], row[what + "_issued_flops"] = nbytes, flops
    row[what + "_tbytes_per_s"], row[what + "_tflops"] = nbytes / ms / 1e9, flops / ms / 1e9
    row[what + "_roof_ms"] = dict(bytes=t_b, mfma=t_f)
    row[what + "_bound"] = "bytes" if t_b >= t_f else "mfma"
    row[what + "_fraction_of_bound"] = max(t_b, t_f) / ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "narrow_train_timing.json"))
    a = ap.parse_args()
    A, L = TorchAllocator(), rdlib.get_lib()
    dev, B = A.device, a.batch
    npix = B * H * W
    rows = []
    for dname, dt, tdt in (("bf16", rdlib.RD_BF16, torch.bfloat16), ("f16", rdlib.RD_F16, torch.float16)):
        gen = torch.Generator(device="cpu").manual_seed(23)
        rng = np.random.default_rng(29)
        ops = TowerOps(dt, L, A)
        slot = torch.zeros(npix, SLOT)
        slot[:, :C] = torch.randn(npix, C, generator=gen)
        slot = slot.to(dev, tdt).view(B, H, W, SLOT)
        pad64 = torch.zeros(B, H, W, 64, device=dev, dtype=tdt)
        pad64[..., :C] = slot[..., :C]
        x1 = torch.relu(torch.randn(npix, 64, generator=gen)).to(dev, tdt).view(B, H, W, 64)
        dz = {co: torch.randn(npix, co, generator=gen).to(dev, tdt).view(B, H, W, co) for co in (64, 128)}
        row = dict(dtype=dname, B=B, H=H, W=W, c=C, slot=SLOT)
        cases = {}
        nc = lambda v: v.permute(0, 3, 1, 2)
        for key, cout, ks in (("narrow_8_64_k3", 64, 3), ("narrow_8_64_k1", 64, 1), ("narrow_8_128_k3", 128, 3)):
            fns = dict(ours=lambda cout=cout, ks=ks: ops.weight_grad_narrow(slot, dz[cout], C, ks, tag="t"))
            if ks == 3:
                fns["padded"] = lambda cout=cout: ops.weight_grad(pad64, dz[cout], tag="tp")
            else:
                fns["padded"] = lambda cout=cout: ops.weight_grad1x1(pad64, dz[cout], tag="tp")
            try:
                xt = nc(slot[..., :C]).contiguous(memory_format=torch.channels_last)
                zt = nc(dz[cout])
                fns["torch"] = lambda xt=xt, zt=zt, cout=cout, ks=ks: torch.ops.aten.convolution_backward(
                    zt, xt, torch.empty(cout, C, ks, ks, device=dev, dtype=tdt).contiguous(memory_format=torch.channels_last), None, (1, 1), (ks // 2, ks // 2),
                    (1, 1), False, (0, 0), 1, (False, True, False))
                ours, ref = fns["ours"]().clone(), fns["torch"]()[1].float()
                torch.cuda.synchronize()
                row[key + "_max_rel_diff_vs_torch"] = float(((ours - ref).abs().max() / ref.abs().max()).cpu())
            except Exception as e:                                                     # recorded, not replaced by a guess
                row[key + "_torch_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
                fns.pop("torch", None)
            cases[key] = (fns, npix * 2 * (SLOT + cout), 2 * npix * ks * ks * SLOT * cout)
        fns = dict(ours=lambda: ops.weight_grad_cat(x1, slot, C, dz[128], tag="t"))

        def padded_cat():
            ops.weight_grad(x1, dz[128], tag="tq")
            return ops.weight_grad(pad64, dz[128], tag="tp")
        fns["padded"] = padded_cat
        try:
            xt = torch.cat([nc(x1), nc(slot[..., :C])], 1).contiguous(memory_format=torch.channels_last)
            zt = nc(dz[128])
            fns["torch"] = lambda: torch.ops.aten.convolution_backward(
                zt, xt, torch.empty(128, 64 + C, 3, 3, device=dev, dtype=tdt).contiguous(memory_format=torch.channels_last), None, (1, 1), (1, 1), (1, 1),
                False, (0, 0), 1, (False, True, False))
            ours, ref = fns["ours"]().clone(), fns["torch"]()[1].float()
            torch.cuda.synchronize()
            row["cat_64_8_128_max_rel_diff_vs_torch"] = float(((ours - ref).abs().max() / ref.abs().max()).cpu())
        except Exception as e:
            row["cat_64_8_128_torch_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
            fns.pop("torch", None)
        cases["cat_64_8_128"] = (fns, npix * 2 * (64 + SLOT + 128), 2 * npix * 9 * (64 + SLOT) * 128)
        # ---- the two classes
        w1 = (rng.standard_normal((64, C, 3, 3)) / 6).astype(np.float32)
        w2 = (rng.standard_normal((64, 64, 3, 3)) / 17).astype(np.float32)
        wsc = (rng.standard_normal((64, C, 1, 1)) / 3).astype(np.float32)
        sbn = [bn_params(64, rng) for _ in range(3)]
        stem = StemBlockTrain("res1_unit1", w1, w2, sbn[0], sbn[1], wsc, sbn[2], dtype=dt, lib=L, alloc=A)
        g64 = dz[64]

        def ours_stem():
            stem.forward(slot)
            return stem.backward(g64)
        fns_stem = dict(ours=ours_stem)
        tw = [(rng.standard_normal((128, 64 + C, 3, 3)) / 18).astype(np.float32)] + [(rng.standard_normal((128, 128, 3, 3)) / 24).astype(np.float32) for _ in range(3)]
        tbn = [bn_params(128, rng) for _ in range(4)]
        ow, ob = (rng.standard_normal((8, 128, 1, 1)) / 11).astype(np.float32), np.zeros(8, np.float32)
        tower = Level0TowerTrain(tw, [b[0] for b in tbn], [b[1] for b in tbn], [b[2] for b in tbn], [b[3] for b in tbn], ow, ob, kind="reg", level=0,
                                 dtype=dt, lib=L, alloc=A)
        d_out = torch.randn(B, H * W, 8, generator=gen).to(dev)

        def ours_tower():
            tower.forward(x1, slot)
            return tower.backward(d_out)
        fns_tower = dict(ours=ours_tower)
        try:
            cl = lambda v: torch.from_numpy(v).to(dev, tdt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            bnf = lambda v, ga, be: F.batch_norm(v, None, None, ga, be, training=True, momentum=1 - BN_MOMENTUM, eps=BN_EPS)
            vec = lambda bns: [torch.from_numpy(v).to(dev).requires_grad_(True) for b_ in bns for v in b_[:2]]
            xs = nc(slot[..., :C]).contiguous(memory_format=torch.channels_last)
            sw, sb = [cl(w1), cl(w2), cl(wsc)], vec(sbn)

            def t_stem():
                y1 = torch.relu(bnf(F.conv2d(xs, sw[0], padding=1), sb[0], sb[1]))
                y = torch.relu(bnf(F.conv2d(y1, sw[1], padding=1), sb[2], sb[3]) + bnf(F.conv2d(xs, sw[2]), sb[4], sb[5]))
                return torch.autograd.grad(y, sw + sb, nc(g64))
            fns_stem["torch"] = t_stem
            x1t = nc(x1).detach().requires_grad_(True)
            ww, wb, wo = [cl(v) for v in tw], vec(tbn), cl(ow)
            wob = torch.from_numpy(ob).to(dev, tdt).requires_grad_(True)
            dot = d_out.view(B, H, W, 8).permute(0, 3, 1, 2).to(tdt)

            def t_tower():
                y = torch.cat([x1t, xs], 1)
                for i in range(4):
                    y = torch.relu(bnf(F.conv2d(y, ww[i], padding=1), wb[2 * i], wb[2 * i + 1]))
                return torch.autograd.grad(F.conv2d(y, wo, wob), [x1t] + ww + wb + [wo, wob], dot)
            fns_tower["torch"] = t_tower
        except Exception as e:
            row["class_torch_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
        cases["stem_block"] = (fns_stem, None, None)
        cases["level0_tower"] = (fns_tower, None, None)
        opts = {}
        for key, strip in (("ours", False), ("norepack", True)):
            opts[key] = SGD(lr=0.0, wd=0.0, lib=L, alloc=A)          # lr 0: the weights stay as they are over the repeats
            for kw in list(stem.optimizer_entries()) + list(tower.optimizer_entries()):
                if strip and kw.get("pack") and (kw["pack"].get("narrow") or kw["pack"].get("cat")):
                    kw = dict(kw, pack=None)
                opts[key].add(**kw)
        cases["sgd_step"] = ({k: o.step for k, o in opts.items()}, None, None)
        for what, (fns, nbytes, flops) in cases.items():
            print("warm-up", dname, what, sorted(fns), flush=True)
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
            for k in ("torch", "padded", "norepack"):
                if k in med:
                    row["%s_%s_ms" % (what, k)], row["%s_%s_over_ours" % (what, k)] = med[k], med[k] / med["ours"]
            if nbytes:
                roofs(row, what, med["ours"], nbytes, flops)
            row[what + "_series"] = raw
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_series")}), flush=True)
        rows.append(row)
        del cases, stem, tower, opts, fns, fns_stem, fns_tower
        torch.cuda.empty_cache()
    out = dict(tool="tools/narrow_conv_timing.py", source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               iters=a.iters, repeats=a.repeats, roofs=dict(hbm_bytes_per_s=HBM_BPS, mfma_flops=MFMA_FLOPS), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()

"""Optimizer-step timing (dev tool): one rangedet_amd.optim.SGD step over the table of a realistic head -- the cls and the reg tower of the
three pyramid levels as HeadTowerTrain accepts them (128 channels; four convs per tower, three at level 0 whose conv_0 reads the 72-channel
concat and is refused), every conv weight with its two 16-bit images, every gamma, beta, output weight and bias -- against what the code
had to do before the step existed:

  (a) torch_foreach   the same arithmetic as torch._foreach_* operations on float32 device tensors of the same sizes
  (b) host_repack     (a), then for every conv weight the download, Lib.pack_conv3x3_ex, TowerOps.pack_data_grad, upload round trip

    python tools/optimizer_timing.py [--iters 200] [--repeats 5] [--out profiles/optimizer_timing.json]

Each figure is the median over `repeats` windows of `iters` calls between device events, after a warm-up of all sides; the windows alternate
and the series is run in both orders, all in this one process (tools/timing_util.py).  (b) ends every call in host copies, so its windows
are short: --host-iters.  Bytes: 20 per parameter (read w, grad, mom; write w, mom) plus, per conv weight, 4 read and 2 x 2 written for the
images; GB/s over those bytes against the 8 TB/s HBM peak bench.py uses.  If a baseline cannot run, the error is recorded and no number
is invented."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rangedet_amd import build, lib as rdlib  # noqa: E402
from rangedet_amd.backward import HeadTowerTrain  # noqa: E402
from rangedet_amd.optim import SGD, default_wd_mult  # noqa: E402
from rangedet_amd.runtime import TorchAllocator  # noqa: E402
from tools.timing_util import series  # noqa: E402

C, PEAK_HBM_GBPS = 128, 8000.0
LR, MOMENTUM, WD, RESCALE, CLIP = 0.01, 0.9, 1e-5, 1.0 / 128, 35.0


def head(L, A, dt, rng):
    towers = []
    for level in range(3):
        first = 1 if level == 0 else 0
        nconv = 4 - first
        for kind, nout in (("cls", 1), ("reg", 8)):
            ws = [(rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C / 2)).astype(np.float32) for _ in range(nconv)]
            one, zero = [np.ones(C, np.float32)] * nconv, [np.zeros(C, np.float32)] * nconv
            ow, ob = (rng.standard_normal((nout, C, 1, 1)) / np.sqrt(C)).astype(np.float32), np.zeros(nout, np.float32)
            towers.append(HeadTowerTrain(ws, one, zero, zero, one, ow, ob, kind=kind, level=level, first_conv=first, dtype=dt, lib=L, alloc=A))
    return towers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_timing.json"))
    a = ap.parse_args()
    A, L = TorchAllocator(), rdlib.get_lib()
    rows = []
    for dt, name in ((rdlib.RD_BF16, "bf16"), (rdlib.RD_F16, "f16")):
        rng = np.random.default_rng(11)
        gen = torch.Generator(device="cpu").manual_seed(12)
        towers = head(L, A, dt, rng)
        opt = SGD(LR, MOMENTUM, WD, RESCALE, CLIP, lib=L, alloc=A)
        entries = []
        for t in towers:
            opt.attach(t)
            entries += list(t.optimizer_entries())
        for e in entries:
            e["grad"].copy_((100.0 * torch.randn(e["grad"].shape, generator=gen)).to(A.device))
        convs = [e for e in entries if e.get("pack")]
        nparam, nconvparam = sum(e["weight"].numel() for e in entries), sum(e["weight"].numel() for e in convs)
        nbytes = 20 * nparam + 8 * nconvparam
        row = dict(dtype=name, tensors=len(entries), conv_weights=len(convs), parameters=nparam, step_bytes=nbytes, launches_per_step=2,
                   table_bytes=0)
        # the baselines run on their own copies of the state: timing must not depend on whose weights moved
        tw = [e["weight"].clone() for e in entries]
        tg = [e["grad"] for e in entries]
        tm = [torch.zeros_like(w) for w in tw]
        dec = [i for i, e in enumerate(entries) if default_wd_mult(e["name"]) > 0]
        images = [(torch.empty_like(e["pack"]["fwd"]), torch.empty_like(e["pack"]["bwd"])) for e in convs]
        conv_idx = [i for i, e in enumerate(entries) if e.get("pack")]

        def foreach():
            g = torch._foreach_mul(tg, RESCALE)
            torch._foreach_clamp_min_(g, -CLIP)
            torch._foreach_clamp_max_(g, CLIP)
            torch._foreach_mul_(tm, MOMENTUM)
            torch._foreach_add_([tm[i] for i in dec], [tw[i] for i in dec], alpha=-LR * WD)
            torch._foreach_add_(tm, g, alpha=-LR)
            torch._foreach_add_(tw, tm)

        def host_repack():
            foreach()
            for (fwd, bwd), i in zip(images, conv_idx):
                w = tw[i].cpu().numpy()                                          # one synchronisation per tensor
                fwd.copy_(torch.from_numpy(L.pack_conv3x3_ex(w, 1, C, fold_scale=None, dtype=dt)))
                wf = np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])
                bwd.copy_(torch.from_numpy(L.pack_conv3x3_ex(wf, 1, C, fold_scale=None, dtype=dt)))
        # one step of both from the same state: the same update up to the rounding order, the same images
        try:
            foreach()
            opt.step()
            torch.cuda.synchronize()
            row["table_bytes"] = int(opt._host.size)
            row["max_abs_weight_diff_vs_torch"] = max(float((e["weight"] - w).abs().max().cpu()) for e, w in zip(entries, tw))
            host_repack()
            opt.step()
            torch.cuda.synchronize()
            want = L.pack_conv3x3_ex(convs[0]["weight"].cpu().numpy(), 1, C, fold_scale=None, dtype=dt)
            row["image_bytes_that_differ_from_host_packer"] = int((convs[0]["pack"]["fwd"][:want.size].cpu().numpy() != want).sum())
            fns = {"ours": opt.step, "torch_foreach": foreach}
        except Exception as e:                                                     # recorded, not replaced by a guess
            row["torch_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
            fns = {"ours": opt.step}
        print("warm-up", name, sorted(fns), flush=True)
        for _ in range(5):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        med, raw = series(fns, a.iters, a.repeats)
        row["step_ms"], row["step_gbps"] = med["ours"], nbytes / med["ours"] / 1e6
        row["step_fraction_of_hbm_peak"] = row["step_gbps"] / PEAK_HBM_GBPS
        row["device_series"] = raw
        if "torch_foreach" in med:
            row["torch_foreach_ms"] = med["torch_foreach"]
            row["torch_foreach_over_ours"] = med["torch_foreach"] / med["ours"]
            med2, raw2 = series({"ours": opt.step, "host_repack": host_repack}, a.host_iters, a.repeats)
            row["host_repack_ms"], row["host_repack_over_ours"] = med2["host_repack"], med2["host_repack"] / med2["ours"]
            row["ours_ms_in_short_windows"] = med2["ours"]
            row["host_series"] = raw2
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_series")}), flush=True)
        rows.append(row)
    res = dict(tool="tools/optimizer_timing.py", source_hash=build.source_hash(), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               iters=a.iters, host_iters=a.host_iters, repeats=a.repeats, peak_hbm_gbps=PEAK_HBM_GBPS,
               step=dict(lr=LR, momentum=MOMENTUM, wd=WD, rescale_grad=RESCALE, clip_gradient=CLIP), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()

"""What the timing tools share: a window of calls between device events, and a series of alternating windows run in both orders."""
import numpy as np
import torch


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def series(fns, iters, repeats):
    """fns: {name: callable}; -> {name: median over both orders of the per-order medians}, and the raw per-order summary"""
    names, out = list(fns), {}
    for order in (names, names[::-1]):
        ms = {k: [] for k in names}
        for _ in range(repeats):
            for k in order:
                ms[k].append(window(fns[k], iters))
        out["%s_first" % order[0]] = {k: dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v))) for k, v in ms.items()}
    return {k: float(np.median([o[k]["median_ms"] for o in out.values()])) for k in names}, out

"""The chain from the last tower conv to the weighted NMS -- rd_head_out, rd_sorted_foreground, rd_decode3d_bbox, rd_gather_keep_scores,
rd_score_filter_dets_batched, rd_dets12_to_8_batched -- per element or bit for bit at the sizes where the kernels change path: the sort
tile (2048) and the 64-lane round, both sides of the full-sort / pre-selection switch, the 256-thread block of the filters, the scan's
carry loop, the 32-pixel tile and the grid-stride iterations of the head kernels.  Every output buffer is a few words longer than needed
and pre-filled with a sentinel that must survive.  References and bounds: oracle/cpu_ops.py and post_model.py.
Each case runs on 'emu' (CPU tier) and on 'hip' (-m gpu)."""
import os

import numpy as np
import pytest

from conftest import BOTH, HIP_ONLY
from emu_util import f32_to_bf16_bits, f32_to_f16_bits
import post_model as PM
from oracle import cpu_ops as O
from rangedet_amd import lib as R

F32, BF16, F16 = R.RD_F32, R.RD_BF16, R.RD_F16
SENT = 0xDEADBEEF            # as float32: -6.3e18, finite, never a result here
PAD = 4                      # words behind every output


def _sent(be, nwords):
    return be.up(np.full(int(nwords), SENT, np.uint32))


def _u32(be, buf, nwords):
    return be.down(buf, np.uint32, (int(nwords),))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _name():
    return os.environ.get("PYTEST_CURRENT_TEST", "").rsplit(" ", 1)[0].split("::")[-1]


def _pe(got, ref, tol, what=""):
    nover, worst = PM.ratio(got, ref, tol)
    print("post-pe %s %s: %d over, worst err / tol %.3f" % (_name(), what, nover, worst))
    assert nover == 0, ("per-element", what, nover, worst)


# ---- 1. sort grid ------------------------------------------------------------------------------------------------------------------------
SORT_N = (1, 64, 65, 2047, 2048, 2049, 4097)


def _sort_ks(N):
    return sorted({k for k in (1, N // 2, N // 2 + 1, N) if 1 <= k <= N})


def _sort_grid():
    """(N, k, D, with_mask, with_idx, wide) -- every (N, k) once, the multi-tile N (> 2048) and the tile edge a second time with all four
    options flipped, so that each option value meets the full sort and the pre-selection at a multi-tile N"""
    grid, i = [], 0
    for N in SORT_N:
        for k in _sort_ks(N):
            c = (i * 7 + 3) % 16
            for cc in ((c, c ^ 15) if N >= 2047 else (c,)):
                grid.append((N, k, 8 if cc & 1 else 7, bool(cc & 2), bool(cc & 4), bool(cc & 8)))
            i += 1
    return grid


SORT_GRID = _sort_grid()


def test_sort_grid_covers_every_option_on_both_paths():
    assert len(SORT_GRID) <= 48
    for opt in range(2, 6):
        for val in set(g[opt] for g in SORT_GRID):
            for full in (False, True):
                assert any(g[opt] == val and (2 * g[1] > g[0]) == full and g[0] > 2048 for g in SORT_GRID), (opt, val, full)


def _sort_inputs(N, B=3, seed=0):
    rng = np.random.default_rng(100 + seed)
    score = rng.uniform(0.0, 1.0, (B, N)).astype(np.float32)
    score[:, ::5] = score[:, :1]                                   # exact ties
    mask = (rng.uniform(size=(B, N)) > 0.3).astype(np.float32)
    delta8 = rng.standard_normal((B, N, 8)).astype(np.float32)
    pc = rng.standard_normal((B, N, 3)).astype(np.float32)
    return score, mask, delta8, pc


def _run_sort(be, score, delta, pc, mask, k, sigmoid, with_idx=True, wide=True, ws=None, ws_bytes=None):
    """-> (scores, deltas, points, indices or None) with the sentinels behind each output checked"""
    B, N = score.shape
    D = delta.shape[2]
    L = be.lib
    per = L.raw("rd_sorted_foreground_workspace_bytes")(N, k)
    nb = ws_bytes if ws_bytes is not None else per * (B if wide else 1)
    if ws is None:
        ws = be.empty(nb)
    o_s, o_d, o_p = _sent(be, B * k + PAD), _sent(be, B * k * D + PAD), _sent(be, B * k * 3 + PAD)
    o_i = _sent(be, B * k + PAD) if with_idx else None
    L.call("rd_sorted_foreground", be.ptr(be.up(score)), be.ptr(be.up(delta)), be.ptr(be.up(pc)), None if mask is None else be.ptr(be.up(mask)),
           B, N, k, D, sigmoid, be.ptr(o_s), be.ptr(o_d), be.ptr(o_p), be.ptr(o_i), be.ptr(ws), nb, be.stream)
    out = []
    for buf, n in ((o_s, B * k), (o_d, B * k * D), (o_p, B * k * 3), (o_i, B * k)):
        if buf is None:
            out.append(None)
            continue
        w = _u32(be, buf, n + PAD)
        assert (w[n:] == SENT).all(), ("written past the end", N, k, D)
        out.append(w[:n])
    return out[0].reshape(B, k), out[1].reshape(B, k, D), out[2].reshape(B, k, 3), None if out[3] is None else out[3].view(np.int32).reshape(B, k)


def _assert_sorted_bits(got, ref, what):
    gs, gd, gp, gi = got
    rs, rd, rp, ri = ref
    if gi is not None:
        assert np.array_equal(gi, ri.astype(np.int32)), ("indices", what)
    assert np.array_equal(gs, _bits(rs)), ("scores", what)
    assert np.array_equal(gd, _bits(rd)), ("deltas", what)
    assert np.array_equal(gp, _bits(rp)), ("points", what)


@pytest.mark.parametrize("be", BOTH, indirect=True)
@pytest.mark.parametrize("N", SORT_N)
def test_sorted_foreground_grid(be, N):
    """rd_sorted_foreground bit for bit against O.get_sorted_foreground at N around the sort tile and the 64-lane round, k on both sides of
    the 2 k > N switch and at 1 and N, D 7 and 8, with and without mask / out_idx, side by side and one problem at a time."""
    score, mask, delta8, pc = _sort_inputs(N)
    ones = np.ones_like(mask)
    for (n, k, D, with_mask, with_idx, wide) in SORT_GRID:
        if n != N:
            continue
        delta = np.ascontiguousarray(delta8[:, :, :D])
        ref = O.get_sorted_foreground(score, delta, pc, mask if with_mask else ones, k)
        got = _run_sort(be, score, delta, pc, mask if with_mask else None, k, 0, with_idx, wide)
        _assert_sorted_bits(got, ref, (N, k, D, with_mask, with_idx, wide))


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_sorted_foreground_reused_workspace(be):
    """the Executor hands the sort a pool that other steps have written: a workspace of 0xA5 bytes, used twice (pre-selection at
    (4097, 1000), then the full sort at (2049, 2049) over what the first call left), must give the same bits as a zeroed one"""
    B = 3
    L = be.lib
    nb = max(L.raw("rd_sorted_foreground_workspace_bytes")(N, k) for N, k in ((4097, 1000), (2049, 2049))) * B
    ws = be.up(np.full(nb + 256, 0xA5, np.uint8))
    for N, k in ((4097, 1000), (2049, 2049)):
        score, mask, delta8, pc = _sort_inputs(N, B, seed=1)
        ref = O.get_sorted_foreground(score, delta8, pc, mask, k)
        got = _run_sort(be, score, delta8, pc, mask, k, 0, ws=ws, ws_bytes=L.raw("rd_sorted_foreground_workspace_bytes")(N, k) * B)
        _assert_sorted_bits(got, ref, (N, k))


# ---- 2. the shipped sigmoid path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", BOTH, indirect=True)
@pytest.mark.parametrize("N,k", [(5000, 1200), (2049, 2049)])
def test_sorted_foreground_sigmoid(be, N, k):
    """apply_sigmoid = 1, as lower.py emits it, without leaning on any libm for the order: logits on a grid of 1/8 in [-8, 8] (neighbouring
    sigmoids differ by >= 4e-5 relative, equal logits give equal scores) and two saturated groups at 25 and 30, which both give exactly
    1.0f and so tie in index order (PM.sigmoid_order).  Indices, deltas and points bit-exact; each score within
    PM.SIGMOID_REL = 4 * 2^-24 = 2.4e-7 relative of the float64 sigmoid: expf 1 ulp (2 * 2^-24, ROCm HIP math API reference), the add and
    the correctly rounded division 2^-24 each (glibc's expf on the emulator tier: 7.7e-8).  Frame 0 masks 30 % of the points out; frame 1
    masks more than N - k out, so its cut falls inside the tie of exact zeros.  (2049, 2049) takes the full sort, (5000, 1200) the
    pre-selection."""
    rng = np.random.default_rng(21)
    B, D = 2, 8
    logit = (rng.integers(-64, 65, (B, N)) / 8.0).astype(np.float32)
    logit[:, 10:400:6] = 25.0
    logit[:, 13:400:6] = 30.0
    mask = np.stack([rng.uniform(size=N) > 0.3, rng.uniform(size=N) > 0.8]).astype(np.float32)
    assert int((mask[1] == 0).sum()) > N - k
    delta = rng.standard_normal((B, N, D)).astype(np.float32)
    pc = rng.standard_normal((B, N, 3)).astype(np.float32)
    idx = np.stack([PM.sigmoid_order(logit[b], mask[b], k) for b in range(B)])
    gs, gd, gp, gi = _run_sort(be, logit, delta, pc, mask, k, 1)
    assert np.array_equal(gi, idx.astype(np.int32))
    for b in range(B):
        assert np.array_equal(gd[b], _bits(delta[b][idx[b]])) and np.array_equal(gp[b], _bits(pc[b][idx[b]]))
    rows = np.arange(B)[:, None]
    want = PM.sigmoid64(logit[rows, idx]) * mask[rows, idx]
    got = gs.view(np.float32)
    sat = (logit[rows, idx] >= 25.0) & (mask[rows, idx] > 0)
    assert sat.sum() >= 40 and (got[sat] == 1.0).all()
    _pe(got, want, PM.SIGMOID_REL * np.abs(want), "sigmoid")


# ---- 3. signed zero in the sort key -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", BOTH, indirect=True)
@pytest.mark.parametrize("N,k,zeros", [(300, 300, 0.5), (5000, 1200, 0.8)])
def test_sorted_foreground_signed_zero(be, N, k, zeros):
    """a negative score times a zero mask is -0.0; the reference compares values, so it ties with +0.0 and index order decides.  Raw
    standard-normal scores; at (5000, 1200) more than N - k points are masked out, so the cut falls inside the tie of zeros."""
    rng = np.random.default_rng(31)
    B, D = 2, 8
    score = rng.standard_normal((B, N)).astype(np.float32)
    mask = (rng.uniform(size=(B, N)) > zeros).astype(np.float32)
    assert ((mask == 0).sum(1) > N - k).all() and (np.signbit(score * mask) & (score * mask == 0)).any()
    delta = rng.standard_normal((B, N, D)).astype(np.float32)
    pc = rng.standard_normal((B, N, 3)).astype(np.float32)
    rs, rd, rp, ri = O.get_sorted_foreground(score, delta, pc, mask, k)
    gs, gd, gp, gi = _run_sort(be, score, delta, pc, mask, k, 0)
    assert np.array_equal(gi, ri.astype(np.int32))
    assert np.array_equal(gs.view(np.float32), rs)                                   # by value: the zeros' sign is not part of the contract
    assert np.array_equal(gd, _bits(rd)) and np.array_equal(gp, _bits(rp))


# ---- 4. rd_gather_keep_scores -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", BOTH, indirect=True)
@pytest.mark.parametrize("mk", [1, 255, 256, 257])
def test_gather_keep_scores(be, mk):
    rng = np.random.default_rng(41)
    B, k = 3, 300
    bs = k + 7
    score = np.full((B, bs), np.nan, np.float32)
    score[:, :k] = rng.uniform(0, 1, (B, k)).astype(np.float32)
    pool = np.concatenate([[0, -1, k, k - 1, 7, 7, k + 5, -1, 123], rng.integers(0, k, 300)]).astype(np.int32)
    keep = np.stack([np.roll(pool, -b)[:mk] for b in range(B)]).astype(np.int32)       # mk = 1: 0, -1 and k
    out = _sent(be, B * mk + PAD)
    be.lib.call("rd_gather_keep_scores", be.ptr(be.up(score)), bs, k, be.ptr(be.up(keep)), mk, be.ptr(out), B, be.stream)
    got = _u32(be, out, B * mk + PAD)
    assert (got[B * mk:] == SENT).all()
    ok = (keep >= 0) & (keep < k)
    want = np.where(ok, _bits(score)[np.arange(B)[:, None], np.clip(keep, 0, k - 1)], np.uint32(0xFF800000))
    assert np.array_equal(got[:B * mk].reshape(B, mk), want)


# ---- 5. score filter, batched -------------------------------------------------------------------------------------------------------------
def _filter_case(be, n, B, seed):
    rng = np.random.default_rng(50 + seed)
    L = be.lib
    thr = np.float32(0.3)
    s_bs, b_bs, d_bs = n + 3, (n + 2) * 10, (n + 1) * 12
    sc = rng.uniform(0, 1, (B, n)).astype(np.float32)
    kind = rng.integers(0, 12, (B, n))
    sc[kind < 4] = thr                                             # a third exactly at the threshold: the compare is a strict >
    sc[kind == 4] = np.nan
    sc[kind == 5] = np.inf
    sc[kind == 6] = -np.inf
    if B > 1:
        sc[0] = rng.uniform(0.5, 1, n).astype(np.float32)         # passes everything
        sc[1] = np.where(rng.integers(0, 3, n) == 0, thr, np.where(rng.integers(0, 2, n) == 0, np.float32(np.nan), np.float32(-np.inf)))   # passes nothing
    boxes = (rng.standard_normal((B, n, 10)) * 10).astype(np.float32)
    scores = np.full((B, s_bs), np.nan, np.float32)
    scores[:, :n] = sc
    bx = np.full((B, b_bs), np.nan, np.float32)
    bx[:, :n * 10] = boxes.reshape(B, -1)
    nb = L.raw("rd_score_filter_workspace_bytes")(n) * B
    ws = be.up(np.full(nb + 256, 0xA5, np.uint8))
    dets, cnt = _sent(be, B * d_bs + PAD), _sent(be, B + PAD)
    L.call("rd_score_filter_dets_batched", be.ptr(be.up(scores)), s_bs, be.ptr(be.up(bx)), b_bs, n, float(thr), be.ptr(dets), d_bs,
           be.ptr(cnt), be.ptr(ws), nb, B, be.stream)
    c = _u32(be, cnt, B + PAD)
    assert (c[B:] == SENT).all()
    refs = [O.score_filter_to_dets(sc[b], boxes[b], thr) for b in range(B)]
    assert list(c[:B]) == [r.shape[0] for r in refs]
    if B > 1:
        assert c[0] == n and c[1] == 0
    got = _u32(be, dets, B * d_bs + PAD)
    assert (got[B * d_bs:] == SENT).all()
    got = got[:B * d_bs].reshape(B, n + 1, 12)
    # column 8 = the device's own edge atan2f (pinned to the C library's by test_edge_atan2f_equals_the_c_library) on the same differences
    ys, xs = [], []
    for b in range(B):
        fg = sc[b] > thr
        ys.append(boxes[b][fg, 1] - boxes[b][fg, 3])
        xs.append(boxes[b][fg, 0] - boxes[b][fg, 2])
    y, x = np.concatenate(ys).astype(np.float32), np.concatenate(xs).astype(np.float32)
    yaw = np.zeros(0, np.uint32)
    if len(y):
        o = be.empty(len(y) * 4)
        L.call("rd_edge_atan2f", be.ptr(be.up(y)), be.ptr(be.up(x)), len(y), be.ptr(o), be.stream)
        yaw = be.down(o, np.uint32, (len(y),))
    at = 0
    for b in range(B):
        K = refs[b].shape[0]
        assert (got[b, K:] == SENT).all(), ("rows at and beyond the count", n, b)
        r = _bits(refs[b]).reshape(K, 12)
        assert np.array_equal(got[b, :K, :8], r[:, :8]) and np.array_equal(got[b, :K, 9:], r[:, 9:]), (n, b)
        assert np.array_equal(got[b, :K, 8], yaw[at:at + K]), (n, b)
        at += K


@pytest.mark.parametrize("be", BOTH, indirect=True)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_score_filter_batched_edges(be, n):
    """rd_score_filter_dets_batched at the wave and block edges, 8 frames, every batch stride wider than its natural value with NaN in
    the gaps, a third of the scores exactly at the threshold, NaN and both infinities among them (rd_gather_keep_scores feeds -inf), one
    frame that passes everything and one that passes nothing, a workspace that is not zero."""
    _filter_case(be, n, 8, n)


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_score_filter_scan_carry(be):
    """n = 65537: 257 blocks, so filter_scan_kernel's carry goes round its loop a second time"""
    _filter_case(be, 65537, 1, 0)


# ---- 6. rd_dets12_to_8_batched ------------------------------------------------------------------------------------------------------------
def _check_8(got_words, d12, n, cap8_rows, what):
    """got_words (rows, 8) uint32 of one frame; the first n rows against PM.dets8_ref64, the rest untouched"""
    assert (got_words[n:] == SENT).all(), ("rows at and beyond the count", what)
    g = got_words[:n].view(np.float32)
    ref, tol = PM.dets8_ref64(d12[:n])
    for col, src in ((5, 10), (6, 8), (7, 11)):
        assert np.array_equal(got_words[:n, col], _bits(d12[:n, src])), ("copied column", col, what)
    if n:
        for cols, name in ((slice(0, 2), "centre"), (slice(2, 3), "cz"), (slice(3, 5), "lengths")):
            _pe(g[:, cols], ref[:, cols], tol[:, cols], "%s %s" % (what, name))


@pytest.mark.parametrize("be", BOTH, indirect=True)
@pytest.mark.parametrize("cap", [1, 255, 256, 257])
def test_dets12_to_8_batched(be, cap):
    """three frames in strided buffers with the count below, at and above cap (the kernel clamps), then the single-frame entry with
    d_count = NULL.  Copied columns bit-equal; computed ones per element within PM.dets8_ref64's bound: (3, 1, 4) * 2^-24 = (1.5, 0.5, 2)
    eps32 times the sum of the operands' magnitudes for the centre, cz and the two lengths."""
    rng = np.random.default_rng(60 + cap)
    B = 3
    L = be.lib
    in_bs, out_bs = (cap + 2) * 12, (cap + 3) * 8
    d12 = (rng.standard_normal((B, cap + 2, 12)) * 20).astype(np.float32)
    d12[:, :, 0:8:2] += rng.uniform(-70, 70, (B, cap + 2, 1)).astype(np.float32)     # corners of one box share a far centre: the lengths cancel
    d12[:, :, 1:8:2] += rng.uniform(-70, 70, (B, cap + 2, 1)).astype(np.float32)
    counts = np.array([max(cap - 1, 0) if cap > 1 else 0, cap, cap + 2], np.int32)
    out = _sent(be, B * out_bs + PAD)
    L.call("rd_dets12_to_8_batched", be.ptr(be.up(d12)), in_bs, cap, be.ptr(be.up(counts)), be.ptr(out), out_bs, B, be.stream)
    got = _u32(be, out, B * out_bs + PAD)
    assert (got[B * out_bs:] == SENT).all()
    got = got[:B * out_bs].reshape(B, cap + 3, 8)
    for b in range(B):
        _check_8(got[b], d12[b], min(int(counts[b]), cap), cap, (cap, b))
    out1 = _sent(be, cap * 8 + PAD)
    L.call("rd_dets12_to_8", be.ptr(be.up(d12[0])), cap, None, be.ptr(out1), be.stream)
    got1 = _u32(be, out1, cap * 8 + PAD)
    assert (got1[cap * 8:] == SENT).all()
    _check_8(got1[:cap * 8].reshape(cap, 8), d12[0], cap, cap, (cap, "no count"))


# ---- 7. rd_decode3d_bbox ------------------------------------------------------------------------------------------------------------------
def _decode_inputs(box_type):
    rng = np.random.default_rng(70 + box_type)
    B, N = 2, 777                                                  # 1554 points: six full blocks and 18 threads of a seventh
    d = rng.normal(0, 0.7, (B, N, box_type)).astype(np.float32)
    pc = rng.uniform(-70, 70, (B, N, 3)).astype(np.float32)
    pc[0, :60] = rng.uniform(-0.55, 0.55, (60, 3)).astype(np.float32)                # next to the sensor: |pc| < 1
    assert int((np.linalg.norm(pc[0, :60], axis=1) < 1).sum()) >= 50
    pc[0, 60:70, 0] = -rng.uniform(0.5, 60, 10).astype(np.float32)                   # the negative x axis, y = +0 / -0: atan2's branch cut
    pc[0, 60:70, 1] = np.where(np.arange(10) % 2 == 0, np.float32(0.0), np.float32(-0.0))
    pc[0, 70:75] = 0.0                                                               # missing returns
    pc[1, -3:] = 0.0                                                                 # ... in the last, partial block too
    sz = (2, 3, 7) if box_type == 8 else (3, 4, 5)
    for j, c in enumerate(sz):
        d[1, 10 + j:40:3, c] = rng.uniform(2.0, 3.0, len(range(10 + j, 40, 3))).astype(np.float32)    # log sizes up to 3
    d[1, 40, list(sz)] = 3.0
    d[0, 80, :2] = 0.0
    return d, pc


@pytest.mark.parametrize("be", BOTH, indirect=True)
@pytest.mark.parametrize("box_type", [8, 7])
def test_decode3d_bbox_per_element(be, box_type):
    """rd_decode3d_bbox against its float64 restatement (PM.decode3d_ref64), regular (8) and bin (7) type, every output within
    7 * 2^-24 (|x| + |y| + |dx| + |dy| + l/2 + w/2) (1 + |az| + |yaw_r|) for the corners and 5 * 2^-24 (|z terms| + h) for z -- constants
    derived in post_model.py from 1 ulp each for the device's atan2f, sinf, cosf and expf plus the float32 roundings.  Next to the sensor
    that is 1e-6, a hundred times tighter than the whole-tensor 1e-4.  The regular type copies d[6] to o[8]."""
    d, pc = _decode_inputs(box_type)
    B, N = d.shape[:2]
    out = _sent(be, B * N * 10 + PAD)
    be.lib.call("rd_decode3d_bbox", be.ptr(be.up(d)), be.ptr(be.up(pc)), be.ptr(out), B, N, box_type, int(box_type == 7), be.stream)
    w = _u32(be, out, B * N * 10 + PAD)
    assert (w[B * N * 10:] == SENT).all()
    w = w[:B * N * 10].reshape(B, N, 10)
    got = w.view(np.float32)
    ref, tol = PM.decode3d_ref64(d, pc, box_type == 7)
    if box_type == 8:
        assert np.array_equal(w[..., 8], _bits(d[..., 6]))
    _pe(got[..., :8], ref[..., :8], tol[..., :8], "corners")
    _pe(got[..., 8:], ref[..., 8:], tol[..., 8:], "z")
    near = slice(0, 60)
    _pe(got[0, near, :8], ref[0, near, :8], tol[0, near, :8], "corners, |pc| < 1")


# ---- 8. rd_head_out -----------------------------------------------------------------------------------------------------------------------
HEAD_LAYOUTS = [(128, 128, 0), (64, 80, 16), (16, 16, 0), (8, 24, 8), (72, 80, 0), (24, 32, 8)]      # (cin, cstride, coff)
HEAD_HW = (1, 31, 32, 33, 127, 128, 129, 300)
HEAD_PAD = {F32: np.float32(1.0e7), BF16: 0x4B4B, F16: 0x4B4B}      # channels outside [coff, coff + cin): never read; 1.3e7 / 14.6 as 16-bit


def _head_image(x, dt, cstride, coff):
    """x (B, HW, cin) rounded to dt -> the (B, HW, cstride) device image with the foreign channels set to HEAD_PAD"""
    B, HW, cin = x.shape
    if dt == F32:
        img = np.full((B, HW, cstride), HEAD_PAD[F32], np.float32)
        img[..., coff:coff + cin] = x
    else:
        img = np.full((B, HW, cstride), HEAD_PAD[dt], np.uint16)
        img[..., coff:coff + cin] = f32_to_bf16_bits(x) if dt == BF16 else f32_to_f16_bits(x)
    return img


def _head_case(be, dt, nout, cin, cstride, coff, x, w, b, n_off=5):
    B, HW, _ = x.shape
    obs = (n_off + HW) * nout + 3
    out = _sent(be, B * obs + PAD)
    # NaN behind the nout * cin weights: a k-step past cin (the matrix-core kernel always runs 8) must load zeros, never what lies there
    wbuf = np.concatenate([w.ravel(), np.full(128, np.nan, np.float32)])
    be.lib.call("rd_head_out", be.ptr(be.up(_head_image(x, dt, cstride, coff))), cstride, coff, be.ptr(be.up(wbuf)), be.ptr(be.up(b)), be.ptr(out),
                obs, n_off, B, 1, HW, cin, nout, dt, be.stream)
    g = _u32(be, out, B * obs + PAD)
    assert (g[B * obs:] == SENT).all()
    g = g[:B * obs].reshape(B, obs)
    assert (g[:, :n_off * nout] == SENT).all() and (g[:, (n_off + HW) * nout:] == SENT).all(), ("sentinel", dt, nout, cin, HW)
    got = g[:, n_off * nout:(n_off + HW) * nout].view(np.float32).reshape(B, HW, nout)
    ref, tol = PM.head_ref64(x, w, b, dt, PM.head_uses_matrix_cores(dt, nout, cin, cstride, coff))
    return PM.ratio(got, ref, tol)


@pytest.mark.parametrize("be", BOTH, indirect=True)
@pytest.mark.parametrize("layout", HEAD_LAYOUTS, ids=lambda l: "cin%d-cs%d-off%d" % l)
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_head_out_per_element(be, dt, layout):
    """rd_head_out per element against the float64 product on the type-rounded input (PM.head_ref64): nout 1 / 7 / 8, HW around the
    32-pixel tile (generic kernel) and the 128-pixel block (matrix cores), two images, a pixel offset in the output, input channels at an
    offset inside a wider buffer whose other channels hold garbage.  cin 128 / 64 / 16 with aligned strides run on the matrix cores for
    nout 7 / 8 (nks = 8 / 4 / 1 k-steps), cin 72 and 24 fall back to the generic kernel, cin 8 and 72 take its scalar loads.  Tolerance:
    (cin + 2) 2^-24 (sum |x w| + |b|) + 2^-24 |ref|, plus the hi + lo weight pair's residual on the matrix cores."""
    cin, cstride, coff = layout
    rng = np.random.default_rng(800 + cin + coff)
    xa = PM.head_input(rng, 2, max(HEAD_HW), cin, dt)
    nover_all, worst_all = 0, 0.0
    for nout in (1, 7, 8):
        w = (rng.standard_normal((nout, cin)) / np.sqrt(cin)).astype(np.float32)
        b = rng.standard_normal(nout).astype(np.float32)
        for HW in HEAD_HW:
            nover, worst = _head_case(be, dt, nout, cin, cstride, coff, np.ascontiguousarray(xa[:, -HW:]), w, b)
            nover_all, worst_all = nover_all + nover, max(worst_all, worst)
    print("post-pe %s: %d over, worst err / tol %.3f" % (_name(), nover_all, worst_all))
    assert nover_all == 0, ("per-element", nover_all, worst_all)


@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
@pytest.mark.parametrize("nout,HW", [(1, 131072 + 33), (8, 262144 + 33)], ids=["generic-grid-stride", "matrix-core-prefetch"])
def test_head_out_grid_stride(be, nout, HW):
    """more pixels than one sweep of the grid: the generic kernel's grid-stride loop (4096 blocks of 32 pixels) and the matrix-core
    kernel's prefetch of its next tile (2048 blocks of 128) run their second iteration; bf16, cin 16, one image, same per-element check.

    The matrix-core case is also the one that sees the whole weight residual: with a quarter of a million pixels against one 8 x 16 weight
    matrix some pixel meets the worst weight row.  Two round-to-nearest bf16 terms miss w by up to 2^-17 |w| (here 1.84 * 2^-18 |w| in
    output channel 0), more than the 2^-18 sum |x w| of the tolerance: with hi + lo alone three of the 2 097 416 elements were at up to
    1.075 of it, on the GPU and under the emulator alike.  The kernel carries a third bf16 term, which makes the sum the fp32 weight."""
    rng = np.random.default_rng(900 + nout)
    cin = 16
    x = PM.head_input(rng, 1, HW, cin, BF16)
    w = (rng.standard_normal((nout, cin)) / np.sqrt(cin)).astype(np.float32)
    b = rng.standard_normal(nout).astype(np.float32)
    assert PM.head_uses_matrix_cores(BF16, nout, cin, cin, 0) == (nout == 8)
    nover, worst = _head_case(be, BF16, nout, cin, cin, 0, x, w, b)
    print("post-pe %s: %d over, worst err / tol %.3f" % (_name(), nover, worst))
    assert nover == 0, ("per-element", nover, worst)

"""Range image from a raw point cloud on the device (rd_range_image_from_points, csrc/k_rangeimg.h; rangedet_amd.range_image) against

  * tests/golden/range_image_kitti_{0,1}.npz -- what the reference's OWN get_range_image (datasets/create_range_image_in_kitti.py:107-137)
    returns for two small clouds, with the beam tables they were made with (tests/golden/make_range_image_golden.py), and
  * tests/range_image_model.py -- the NumPy restatement pinned by those files (stable argsort: the higher index wins a tie), for the
    shapes and inputs without a golden file.

Everything is compared bit for bit on every cell.  That is sound because every cloud meets two margin conditions (range_image_model.py):
the float64 row errors of the best and the second-best beam differ by >= 1e-9 rad (a last-ulp difference between two double atan2
implementations is ~1e-16), and the float64 column value is >= 0.01 away from a rounding boundary (the float32 chain is within ~3e-4 of
it at W = 2048); the column's float32 atan2f is the C library's bit for bit (rd_common.h fdlibm_atan2f), the points with y = +-0, x < 0
sit exactly ON the boundaries -0.5 and W - 0.5 and exercise both clamps."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import range_image_model as M
from conftest import BOTH, HIP_ONLY
from rangedet_amd import lib as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W = 2048
_CACHE = {}


def _gold():
    if "gold" not in _CACHE:
        gs = []
        for i in (0, 1):
            g = dict(np.load(os.path.join(GOLD, "range_image_kitti_%d.npz" % i)))
            img = np.full((64 * W, 5), -1, np.float32)
            img[g["cells"]] = g["values"]
            g["image"] = img.reshape(64, W, 5)
            g["image"].setflags(write=False)
            gs.append(g)
        _CACHE["gold"] = gs
    return _CACHE["gold"]


def _same(a, b):
    """bit for bit (-0.0 and 0.0 differ)"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _abi(be, clouds, incl, height, width, ws_fill=None, index=True):
    """rd_range_image_from_points on a list of (N,4) clouds -> (range_image (B,H,W,5), mask (B,H,W) uint8, point_index (B,H,W) or None)."""
    L, B, H = be.lib, len(clouds), len(incl)
    off = (ctypes.c_longlong * (B + 1))(*np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).tolist())
    incl, height = np.ascontiguousarray(incl, np.float64), np.ascontiguousarray(height, np.float64)
    pts = be.up(np.concatenate(clouds).astype(np.float32)) if off[B] else None
    n = B * H * width
    nws = L.raw("rd_range_image_workspace_bytes")(B, H, width)
    assert nws == n * 8
    ws = be.empty(nws) if ws_fill is None else be.up(np.full(nws, ws_fill, np.uint8))
    img, mask, idx = be.empty(n * 20), be.empty(n), be.empty(n * 4) if index else None
    L.call("rd_range_image_from_points", be.ptr(pts), ctypes.addressof(off), B, incl.ctypes.data, height.ctypes.data, H, width,
           be.ptr(img), be.ptr(mask), be.ptr(idx), be.ptr(ws), nws, be.stream)
    return (be.down(img, np.float32, (B, H, width, 5)), be.down(mask, np.uint8, (B, H, width)),
            be.down(idx, np.int32, (B, H, width)) if index else None)


def _check(got, clouds, want_imgs, want_idx, what):
    """got = _abi(...); want_imgs / want_idx per scan.  mask and point_index follow from the image, the points under point_index are the
    image's values."""
    img, mask, idx = got
    for b, (pc, wi, wx) in enumerate(zip(clouds, want_imgs, want_idx)):
        assert _same(img[b], wi), (what, b, "range_image", int((img[b] != wi).any(-1).sum()))
        assert np.array_equal(mask[b], (wi[..., 0] > -1).astype(np.uint8)), (what, b, "mask")
        assert np.array_equal(idx[b], wx), (what, b, "point_index")
        f = idx[b] >= 0
        assert np.array_equal(f, mask[b] == 1) and _same(img[b][f][:, 1:], np.ascontiguousarray(pc[idx[b][f]])), (what, b, "points")


# ---- 1, 2: the fixtures and the restatement (CPU) ----------------------------------------------------------------------------------
def test_fixture_conditions_hold_on_the_committed_data():
    """Margins, unique ranges per cell, both clamps, and for scan 0: >= 100 cells hit twice, one hit >= 8 times, a collision won by the
    lowest and one won by the highest index, every row and the columns 0 and 2047 filled -- the generator's own conditions()."""
    spec = importlib.util.spec_from_file_location("make_range_image_golden", os.path.join(GOLD, "make_range_image_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gs = _gold()
    assert [len(g["pc"]) for g in gs] == [5947, 37]
    for g, full in zip(gs, (True, False)):
        assert g["pc"].dtype == np.float32 and g["incl"].dtype == g["height"].dtype == np.float64 and len(g["incl"]) == len(g["height"]) == 64
        gen.conditions(g["pc"], g["incl"], g["height"], g["cells"], g["values"], full)


def test_restatement_equals_reference_python():
    for g in _gold():
        img, idx = M.get_range_image(g["pc"], g["incl"], g["height"], W, with_index=True)
        assert _same(img, g["image"])
        assert np.array_equal(idx >= 0, img[..., 0] > -1) and _same(img[idx >= 0][:, 1:], np.ascontiguousarray(g["pc"][idx[idx >= 0]]))


def _gold_idx():
    if "gold_idx" not in _CACHE:
        _CACHE["gold_idx"] = [M.get_range_image(g["pc"], g["incl"], g["height"], W, with_index=True)[1] for g in _gold()]
    return _CACHE["gold_idx"]


# ---- 3, 4, 7: the golden scans through the ABI -------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_golden_through_the_abi(be):
    """Each golden scan alone (B = 1) against the reference's output: every cell of range_image, mask and point_index."""
    for i, (g, wx) in enumerate(zip(_gold(), _gold_idx())):
        got = _abi(be, [g["pc"]], g["incl"], g["height"], W)
        _check(got, [g["pc"]], [g["image"]], [wx], "golden %d (%s)" % (i, be.name))
        noidx = _abi(be, [g["pc"]], g["incl"], g["height"], W, index=False)           # point_index may be NULL
        assert _same(noidx[0], got[0]) and _same(noidx[1], got[1])


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_batch_of_three_and_dirty_workspace(be):
    """One call with scan 0, an empty scan and scan 1 equals the three single-scan results; a workspace pre-filled with 0x5A gives the same
    bytes (the library sets the keys on the stream in every call)."""
    g0, g1 = _gold()
    clouds = [g0["pc"], np.zeros((0, 4), np.float32), g1["pc"]]
    singles = [_abi(be, [c], g0["incl"], g0["height"], W) for c in clouds]
    assert (singles[1][0] == -1).all() and not singles[1][1].any() and (singles[1][2] == -1).all()
    got = _abi(be, clouds, g0["incl"], g0["height"], W)
    dirty = _abi(be, clouds, g0["incl"], g0["height"], W, ws_fill=0x5A)
    for k in range(3):
        assert _same(got[k], np.concatenate([s[k] for s in singles])), k
        assert _same(dirty[k], got[k]), k
    empty = np.full((64, W, 5), -1, np.float32)
    _check(got, clouds, [g0["image"], empty, g1["image"]], [_gold_idx()[0], np.full((64, W), -1, np.int32), _gold_idx()[1]], "B = 3")


@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_deterministic(be):
    """The scatter goes through atomics (an integer minimum: order-independent): three runs give identical bytes."""
    g = _gold()[0]
    runs = [_abi(be, [g["pc"]], g["incl"], g["height"], W) for _ in range(3)]
    assert all(_same(r[k], runs[0][k]) for r in runs[1:] for k in range(3))


# ---- 5: ties and non-finite points ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_ties_and_non_finite_points(be):
    """Duplicated points (same coordinates, another intensity: same cell, same range) -- the higher index wins, as in the restatement's
    stable argsort; points with a NaN / +-Inf coordinate interleaved -- the output is that of the cloud without them."""
    g0, g1 = _gold()
    rs = np.random.RandomState(3)
    base = np.concatenate([g1["pc"], g0["pc"][:300]])
    dup = base[rs.choice(len(base), 80, replace=False)].copy()
    dup[:, 3] += 1.0
    pc = np.concatenate([base, dup, dup[:20] + np.float32([0, 0, 0, 1])])          # some cells with three equal ranges
    pc = pc[rs.permutation(len(pc))]
    bad = pc[rs.choice(len(pc), 45, replace=True)].copy()
    for j, v in enumerate([np.nan, np.inf, -np.inf] * 15):
        bad[j, j % 3] = v
    bad[40:, 3] = np.nan                                                            # (and an intensity, which does not disqualify ...)
    slots = np.sort(rs.choice(len(pc) + 45, 45, replace=False))
    full = np.empty((len(pc) + 45, 4), np.float32)
    isbad = np.zeros(len(full), bool)
    isbad[slots] = True
    full[isbad], full[~isbad] = bad, pc
    kept = np.nonzero(~isbad)[0]
    full[kept[-1], 3] = np.nan                                                      # ... a finite point with a NaN intensity stays
    assert np.isfinite(full[kept, :3]).all() and not np.isfinite(full[isbad, :3]).all(axis=1).any()
    img, idx = M.get_range_image(full[kept], g0["incl"], g0["height"], W, with_index=True)
    rows, cols, rng = M.rows_cols_range(full[kept], g0["incl"], g0["height"], W)
    key = np.stack([rows * W + cols, rng.view(np.int32)])
    assert len(full[kept]) - len(np.unique(key, axis=1).T) >= 100                    # the ties are there
    want_idx = np.where(idx >= 0, kept[np.maximum(idx, 0)], -1).astype(np.int32)
    got = _abi(be, [full], g0["incl"], g0["height"], W)
    assert got[0].tobytes() == img.tobytes() and np.array_equal(got[2][0], want_idx)
    assert np.array_equal(got[1][0], (img[..., 0] > -1).astype(np.uint8))
    f = want_idx >= 0
    assert got[0][0][f][:, 1:].tobytes() == full[want_idx[f]].tobytes()


# ---- 6: other shapes against the restatement -------------------------------------------------------------------------------------------
def _second(H, width):
    """Made-up tables, three clouds of different lengths (none a multiple of 64) that meet the margin conditions; computed once."""
    k = ("second", H, width)
    if k not in _CACHE:
        incl = np.linspace(-0.04, 0.42, H) + 0.003 * np.sin(np.arange(H))
        height = 0.21 - 0.09 * np.arange(H) / H
        clouds = [M.synth_cloud(20 + i, n, incl, height, width, cluster=c) for i, (n, c) in enumerate(((700, 9), (130, 0), (300, 3)))]
        assert all(len(c) % 64 and M.keep_by_margin(c, incl, height, width).all() for c in clouds)
        ref = [M.get_range_image(c, incl, height, width, with_index=True) for c in clouds]
        assert all((r[0][..., 0] > -1).sum() < len(c) for r, c in zip(ref, clouds))        # collisions
        _CACHE[k] = (incl, height, clouds, [r[0] for r in ref], [r[1] for r in ref])
    return _CACHE[k]


@pytest.mark.parametrize("shape", [(16, 96), (3, 37)], ids=["16x96", "3x37"])
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_second_shape_against_the_restatement(be, shape):
    """16 x 96: W no power of two, six workgroups of cells per scan.  3 x 37: 111 cells, less than one workgroup, and 555 floats per scan, so
    scans 1 and 2 start off a 16-byte boundary (the resolve pass's ragged ends)."""
    incl, height, clouds, imgs, idxs = _second(*shape)
    _check(_abi(be, clouds, incl, height, shape[1]), clouds, imgs, idxs, "%dx%d (%s)" % (shape + (be.name,)))


# ---- 8: Python surface ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_python_surface(be, tmp_path):
    from rangedet_amd import range_image as RI
    g0, g1 = _gold()
    img = RI.get_range_image(g1["pc"], g1["incl"], g1["height"], lib=be.lib, alloc=be.alloc)       # the reference's call shape
    assert isinstance(img, np.ndarray) and _same(img, g1["image"])
    incl, height, clouds, imgs, idxs = _second(16, 96)
    assert _same(RI.get_range_image(clouds[1], incl, height, 96, lib=be.lib, alloc=be.alloc), imgs[1])
    # the class: a batch of host arrays, then resident device tensors; the buffers are reused
    t = RI.PointCloudToRangeImage(g0["incl"], g0["height"], lib=be.lib, alloc=be.alloc)
    out = t([g0["pc"], g1["pc"]])
    be.alloc.sync()
    assert sorted(out) == ["point_index", "range_image", "range_image_mask"]
    host = {k: np.array(be.alloc.to_numpy(v)) for k, v in out.items()}
    assert host["range_image"].shape == (2, 64, W, 5) and host["range_image_mask"].dtype == np.bool_ and host["point_index"].dtype == np.int32
    assert _same(host["range_image"][0], g0["image"]) and _same(host["range_image"][1], g1["image"])
    assert np.array_equal(host["range_image_mask"], host["range_image"][..., 0] > -1)
    assert np.array_equal(host["point_index"][1], _gold_idx()[1])
    dev = [be.alloc.as_device_f32(g1["pc"]), be.alloc.as_device_f32(g0["pc"])]
    out2 = t(dev)
    be.alloc.sync()
    assert be.alloc.ptr(out2["range_image"]) == be.alloc.ptr(out["range_image"])
    host2 = np.array(be.alloc.to_numpy(out2["range_image"]))
    assert _same(host2[0], g1["image"]) and _same(host2[1], g0["image"])
    one = t(dev[1:])                                                                               # a single resident tensor is used in place
    be.alloc.sync()
    assert _same(np.array(be.alloc.to_numpy(one["range_image"]))[0], g0["image"])
    with pytest.raises(ValueError):
        t([g0["pc"][:, :3]])
    with pytest.raises(ValueError):
        RI.PointCloudToRangeImage(g0["incl"], g0["height"][:63], lib=be.lib, alloc=be.alloc)
    # the command line: .bin in, the two arrays of the reference's tool out
    g1["pc"].tofile(str(tmp_path / "scan.bin"))
    np.savez(str(tmp_path / "beams.npz"), inclination=g1["incl"], height=g1["height"])
    RI.main(["--bin", str(tmp_path / "scan.bin"), "--beams", str(tmp_path / "beams.npz"), "--out", str(tmp_path / "scan.npz")],
            lib=be.lib, alloc=be.alloc)
    z = np.load(str(tmp_path / "scan.npz"))
    assert sorted(z.files) == ["range_image", "range_image_mask"]
    assert _same(z["range_image"], g1["image"]) and np.array_equal(z["range_image_mask"], g1["image"][..., 0] > -1)


# ---- 9: status codes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", BOTH, indirect=True)
def test_status_codes(be):
    """RD_ESHAPE / RD_EWORKSPACE / RD_EINVAL instead of a launch; the thread-local message is set.  (Every check precedes the first launch, so
    one zeroed buffer stands for all device pointers; the valid forms -- a NULL point_index, NULL points when there is no point at all --
    run with buffers of their own in the tests above.)"""
    L = be.lib
    p = be.ptr(be.empty(1 << 16))
    tab = np.linspace(0.0, 0.4, 129)
    wsb = L.raw("rd_range_image_workspace_bytes")
    assert wsb(3, 64, 2048) == 3 * 64 * 2048 * 8 and wsb(1, 1, 1) == 8

    def call(B=2, H=4, W_=8, off=(0, 5, 9), ws_bytes=None, **null):
        o = (ctypes.c_longlong * len(off))(*off)
        a = dict(points=p, offsets=ctypes.addressof(o), incl=tab.ctypes.data, height=tab.ctypes.data, image=p, mask=p, index=p, ws=p)
        a.update(null)
        nb = wsb(B, H, W_) if ws_bytes is None else ws_bytes
        return L.raw("rd_range_image_from_points")(a["points"], a["offsets"], B, a["incl"], a["height"], H, W_, a["image"], a["mask"],
                                                   a["index"], a["ws"], nb, be.stream)
    for kw in (dict(B=0), dict(B=-1), dict(H=0), dict(H=129), dict(W_=0), dict(W_=-3), dict(off=(1, 5, 9)), dict(off=(0, 5, 4)),
               dict(off=(0, -1, 4)), dict(off=(0, 1 << 31, 1 << 31)), dict(B=1, off=(0, 1 << 31))):
        assert call(**kw) == R.RD_ESHAPE, kw
        assert L.rd_last_error_string().decode() != ""
    assert call(ws_bytes=2 * 4 * 8 * 8 - 1) == R.RD_EWORKSPACE and "workspace" in L.rd_last_error_string().decode()
    assert call(ws_bytes=0) == R.RD_EWORKSPACE
    for name in ("points", "offsets", "incl", "height", "image", "mask", "ws"):
        assert call(**{name: None}) == R.RD_EINVAL, name
    assert call(points=p + 4) == R.RD_EINVAL and call(image=p + 8) == R.RD_EINVAL      # 16-byte alignment


# ---- 10: one full-size scan (GPU only) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("be", HIP_ONLY, indirect=True)
def test_full_size_scan(be):
    """120 000 points at 64 x 2048 with the fixture's beam tables, filtered to the margin conditions, against the restatement: every cell."""
    g = _gold()[0]
    pc = M.synth_cloud(11, 120000, g["incl"], g["height"], W, cluster=40)
    assert len(pc) > 119000
    img, idx = M.get_range_image(pc, g["incl"], g["height"], W, with_index=True)
    assert (idx >= 0).sum() < 0.7 * len(pc)                                          # two thirds of the cells' worth of points: many collisions
    _check(_abi(be, [pc], g["incl"], g["height"], W), [pc], [img], [idx], "120k")

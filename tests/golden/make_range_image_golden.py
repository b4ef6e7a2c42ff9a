"""Writes tests/golden/range_image_kitti_{0,1}.npz: small point clouds, the beam tables they were made with, and what the REFERENCE's own
get_range_image (datasets/create_range_image_in_kitti.py:107-137) returns for them -- the filled cells only (flat cell index + the five
values), every other cell of the 64 x 2048 image is -1.

Build container only: needs the reference checkout (RANGEDET_REFERENCE, default /root/reference).  The function and the two beam tables are
compiled from the reference file's syntax tree at generation time; none of its text is stored here or in the fixtures (the tables are
recorded as data: the arrays the outputs were computed with).

  scan 0   about 6000 points: every beam, a sector with many two-point cells, one cell hit by 12 points, the +-pi azimuth points
  scan 1   37 points

conditions() is asserted here and again by tests/test_range_image.py on the committed files."""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import range_image_model as M  # noqa: E402

W = 2048


def load_reference():
    path = os.path.join(os.environ.get("RANGEDET_REFERENCE", "/root/reference"), "datasets", "create_range_image_in_kitti.py")
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_range_image"]
    main = [n for n in tree.body if isinstance(n, ast.If)][-1]
    keep += [n for n in main.body if isinstance(n, ast.Assign) and n.targets[0].id in ("height", "zenith", "incl")]
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns["get_range_image"], np.asarray(ns["incl"], np.float64), np.asarray(ns["height"], np.float64)


def conditions(pc, incl, height, cells, values, full):
    """The fixture conditions.  full: scan 0's collision and coverage conditions as well."""
    H = len(incl)
    row_m, col_m = M.margins(pc, incl, height, W)
    assert len(pc) % 64 != 0 and np.isfinite(pc).all()
    assert row_m.min() >= M.ROW_MARGIN, row_m.min()
    assert col_m.min() >= M.COL_MARGIN, col_m.min()
    rows, cols, rng = M.rows_cols_range(pc, incl, height, W)
    neg = (pc[:, 0] < 0) & (pc[:, 1] == 0)
    minus, plus = neg & np.signbit(pc[:, 1]), neg & ~np.signbit(pc[:, 1])
    assert minus.any() and plus.any() and (cols[minus] == W - 1).all() and (cols[plus] == 0).all()       # both clamps
    cell = rows * W + cols
    assert len(np.unique(np.stack([cell, rng.view(np.int32)]), axis=1).T) == len(pc)                     # unique ranges within a cell
    u, cnt = np.unique(cell, return_counts=True)
    assert np.array_equal(u, cells) and values.shape == (len(cells), 5) and (values[:, 0] > -1).all()
    if not full:
        return
    assert (cnt >= 2).sum() >= 100 and cnt.max() >= 8, ((cnt >= 2).sum(), cnt.max())
    lower = higher = 0                                       # collisions whose nearest point has the lowest / the highest index
    for c in u[cnt >= 2]:
        i = np.nonzero(cell == c)[0]
        k = i[np.argmin(rng[i])]
        lower += k == i[0]
        higher += k == i[-1]
    assert lower >= 1 and higher >= 1, (lower, higher)
    assert set(cells // W) == set(range(H)) and (cells % W == 0).any() and (cells % W == W - 1).any()


def special_points(rs, incl, height):
    """y = -0 / +0 with x < 0: azimuth exactly -pi / +pi, columns 2047.5 -> 2048 -> 2047 and -0.5 -> -0 -> 0."""
    out = []
    for y in (-0.0, 0.0, -0.0, 0.0):
        b, d = rs.randint(0, len(incl)), rs.uniform(5, 60)
        out.append([-d, y, height[b] - d * np.tan(incl[b]), rs.uniform(0, 1)])
    return np.asarray(out, np.float32)


def make_scan(seed, n, incl, height, full):
    rs = np.random.RandomState(seed)
    parts = [M.synth_cloud(seed, n, incl, height, W, cluster=12 if full else 3), special_points(rs, incl, height)]
    if full:                                                 # a 40-column sector with ~600 points: many cells hit twice
        s = M.synth_cloud(seed + 100, 4000, incl, height, W)
        az = np.arctan2(s[:, 1], s[:, 0])
        parts.append(s[(az > 1.0) & (az < 1.0 + 40 * 2 * np.pi / W)][:600])
    pc = np.concatenate(parts)
    pc = pc[rs.permutation(len(pc))]
    pc = pc[M.keep_by_margin(pc, incl, height, W)]
    rows, cols, rng = M.rows_cols_range(pc, incl, height, W)     # drop points that share cell AND range with an earlier one
    _, first = np.unique(np.stack([rows * W + cols, rng.view(np.int32)]), axis=1, return_index=True)
    pc = pc[np.sort(first)]
    if len(pc) % 64 == 0:
        pc = pc[:-1]
    return np.ascontiguousarray(pc)


def main():
    ref, incl, height = load_reference()
    for i, (n, full) in enumerate(((5850, True), (30, False))):
        pc = make_scan(7 + i, n, incl, height, full)
        img = ref(pc.copy(), incl, height)
        assert img.shape == (64, W, 5) and img.dtype == np.float32
        cells = np.nonzero(img[..., 0].reshape(-1) > -1)[0]
        values = img.reshape(-1, 5)[cells]
        assert (img.reshape(-1, 5)[np.setdiff1d(np.arange(64 * W), cells)] == -1).all()
        conditions(pc, incl, height, cells, values, full)
        out = os.path.join(HERE, "range_image_kitti_%d.npz" % i)
        np.savez_compressed(out, pc=pc, incl=incl, height=height, cells=cells.astype(np.int32), values=values)
        print(out, len(pc), "points", len(cells), "cells", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

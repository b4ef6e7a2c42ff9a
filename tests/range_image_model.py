"""NumPy restatement of the reference's get_range_image (datasets/create_range_image_in_kitti.py:107-137) with the build's two additions:
the width is a parameter and the argsort is STABLE (of two points of one cell with the same range the higher index wins; the
reference's argsort leaves that open).  tests/golden/range_image_kitti_*.npz pin it to the reference's own function bit for bit.
TEST INFRASTRUCTURE ONLY: also the source of the margin conditions the fixtures and the synthetic clouds have to meet."""
import numpy as np

ROW_MARGIN = 1e-9      # rad: best and second-best beam differ by at least this (a last-ulp difference of a double atan2 is ~1e-16)
COL_MARGIN = 0.01      # columns: distance of the float64 column value from a rounding boundary (float32 error of the chain ~3e-4 at W = 2048)


def rows_cols_range(pc, incl, height, width):
    """Per point: row (int64), column (int32), range (float32), in the reference's arithmetic."""
    pc = np.asarray(pc, np.float32)
    incl, height = np.asarray(incl, np.float64), np.asarray(height, np.float64)
    xy_norm = np.sqrt(pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1])                                   # float32 (:110)
    err = np.stack([np.abs(incl[i] - np.arctan2(height[i] - pc[:, 2], xy_norm)) for i in range(len(incl))], axis=-1)   # float64 (:112-117)
    rows = np.argmin(err, axis=-1) if len(pc) else np.zeros(0, np.int64)
    azi = np.arctan2(pc[:, 1], pc[:, 0])                                                            # float32 (:120)
    col = np.float32(width - 1.0 + 0.5) - (azi + np.float32(np.pi)) / np.float32(2.0 * np.pi) * np.float32(width)
    assert col.dtype == np.float32 and xy_norm.dtype == np.float32 and err.dtype == np.float64
    col = np.round(col).astype(np.int32)
    col[col == width] = width - 1
    col[col < 0] = 0
    rng = np.sqrt((pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1]) + pc[:, 2] * pc[:, 2])               # float32 (:127)
    return rows, col, rng


def get_range_image(pc, incl, height, width=2048, with_index=False):
    """(H, width, 5) float32, -1 in empty cells; with_index: also (H, width) int32, the winning point's index (-1 = empty)."""
    pc = np.asarray(pc, np.float32).reshape(-1, 4)
    rows, cols, rng = rows_cols_range(pc, incl, height, width)
    order = np.argsort(-rng, kind='stable')
    img = np.full((len(incl), width, 5), -1, np.float32)
    idx = np.full((len(incl), width), -1, np.int32)
    img[rows[order], cols[order]] = np.concatenate([rng[order, None], pc[order]], axis=1)
    idx[rows[order], cols[order]] = order.astype(np.int32)
    return (img, idx) if with_index else img


def margins(pc, incl, height, width):
    """(row margin per point [rad], column margin per point [columns]): what ROW_MARGIN / COL_MARGIN are compared with.  The points with
    y = +-0 and x < 0 (azimuth exactly +-pi in any library) get an infinite column margin."""
    pc = np.asarray(pc, np.float32)
    incl, height = np.asarray(incl, np.float64), np.asarray(height, np.float64)
    xy_norm = np.sqrt(pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1])
    err = np.stack([np.abs(incl[i] - np.arctan2(height[i] - pc[:, 2], xy_norm)) for i in range(len(incl))], axis=-1)
    if err.shape[1] > 1:
        two = np.partition(err, 1, axis=-1)[:, :2]
        row_m = two[:, 1] - two[:, 0]
    else:
        row_m = np.full(len(pc), np.inf)
    c = (width - 0.5) - (np.arctan2(pc[:, 1].astype(np.float64), pc[:, 0].astype(np.float64)) + np.pi) / (2 * np.pi) * width
    col_m = np.abs(c - np.floor(c) - 0.5)
    col_m[(pc[:, 1] == 0) & (pc[:, 0] < 0)] = np.inf
    return row_m, col_m


def keep_by_margin(pc, incl, height, width):
    row_m, col_m = margins(pc, incl, height, width)
    return (row_m >= ROW_MARGIN) & (col_m >= COL_MARGIN)


def synth_cloud(seed, n, incl, height, width, jitter=8e-4, cluster=0):
    """A spinning-LiDAR-like cloud of about n points that meets the margin conditions: every beam, azimuths over the full circle, ranges
    2 - 80 m, beam jitter `jitter` rad; `cluster` extra points packed into one cell's solid angle at different ranges."""
    rs = np.random.RandomState(seed)
    incl, height = np.asarray(incl, np.float64), np.asarray(height, np.float64)
    H = len(incl)
    m = int(n * 1.1) + 8
    beam = rs.randint(0, H, m)
    beam[:min(H, m)] = np.arange(min(H, m))
    az = rs.uniform(-np.pi, np.pi, m)
    d = rs.uniform(2.0, 80.0, m)                                  # horizontal distance
    th = incl[beam] + rs.normal(0, jitter, m)
    if cluster:
        k = rs.randint(0, m)
        beam = np.concatenate([beam, np.full(cluster, beam[k])])
        centre = (width - 0.5 - np.round((width - 0.5) - (az[k] + np.pi) / (2 * np.pi) * width)) / width * 2 * np.pi - np.pi
        az = np.concatenate([az, centre + rs.uniform(-0.2, 0.2, cluster) * 2 * np.pi / width])
        d = np.concatenate([d, rs.uniform(2.0, 80.0, cluster)])
        th = np.concatenate([th, np.full(cluster, incl[beam[k]])])
    z = height[beam] - d * np.tan(th)
    pc = np.stack([d * np.cos(az), d * np.sin(az), z, rs.uniform(0, 1, len(d))], axis=1).astype(np.float32)
    pc = pc[rs.permutation(len(pc))]
    pc = pc[keep_by_margin(pc, incl, height, width)]
    return np.ascontiguousarray(pc[:n + cluster])

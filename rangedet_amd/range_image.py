"""Range image from a raw spinning-LiDAR point cloud on the device: the build's counterpart of the reference's get_range_image
(datasets/create_range_image_in_kitti.py:107-137, mask :178), which builds the KITTI range image from a Velodyne scan on the host with a
loop over the beams, an argsort and a fancy-index scatter.  One rd_range_image_from_points call (csrc/k_rangeimg.h) per batch of scans.

The beam tables (one inclination and one sensor height per beam, float64) are arguments: the package ships none.  The reference's KITTI
tables stand as literals in its tool (:211-240, "obtained from Hough transformation"; inclination = -zenith); for another sensor take the
calibrated beam angles and the height of each beam's origin above the sensor frame.

Tie rule: of two points of one cell with the same range the one with the HIGHER index wins (a stable argsort; the reference's is not
stable and leaves it open).  Points with a non-finite x, y or z are skipped.

  python -m rangedet_amd.range_image --bin scan.bin --beams beams.npz --out scan.npz
writes range_image and range_image_mask like the reference's tool (:187-191); beams.npz holds `inclination` and `height`.
"""
import ctypes

import numpy as np

from . import lib as rdlib


class PointCloudToRangeImage:
    """clouds -> {'range_image' (B,H,W,5) float32, 'range_image_mask' (B,H,W) bool, 'point_index' (B,H,W) int32} as device tensors on the
    current stream, without a host synchronisation.  The output buffers and the workspace are reused between calls with the same number
    of scans: a result is valid until the next such call."""

    def __init__(self, inclination, height, width=2048, lib=None, alloc=None):
        self.incl = np.ascontiguousarray(inclination, dtype=np.float64).reshape(-1)
        self.height = np.ascontiguousarray(height, dtype=np.float64).reshape(-1)
        if self.incl.shape != self.height.shape or not 1 <= len(self.incl) <= 128:
            raise ValueError("inclination and height: one value per beam each, 1..128 beams, got %d and %d" % (len(self.incl), len(self.height)))
        self.H, self.W = len(self.incl), int(width)
        self.L = lib or rdlib.get_lib()
        if alloc is None:
            from .runtime import TorchAllocator
            alloc = TorchAllocator()
        self.A = alloc
        self._bufs = {}

    def _points(self, clouds):
        """One (sum N, 4) float32 buffer, 16-byte aligned, from host arrays (one upload) or resident tensors (no host copy)."""
        A = self.A
        for c in clouds:
            if len(c.shape) != 2 or c.shape[1] != 4:
                raise ValueError("a cloud is (N, 4) x, y, z, intensity, got %r" % (tuple(c.shape),))
        if all(isinstance(c, np.ndarray) for c in clouds):
            return A.upload(np.concatenate([np.asarray(c, np.float32) for c in clouds]))
        dev = [A.as_device_f32(c) for c in clouds]
        if len(dev) == 1 and A.ptr(dev[0]) % 16 == 0:
            return dev[0]
        return A.torch.cat(dev)

    def __call__(self, clouds):
        A, L, H, W = self.A, self.L, self.H, self.W
        clouds = list(clouds)
        B = len(clouds)
        if B < 1:
            raise ValueError("no cloud")
        offsets = (ctypes.c_longlong * (B + 1))(*np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).tolist())
        pts = self._points(clouds)
        if B not in self._bufs:
            nws = L.raw("rd_range_image_workspace_bytes")(B, H, W)
            self._bufs[B] = (A.alloc(B * H * W * 20), A.alloc(B * H * W), A.alloc(B * H * W * 4), A.alloc(nws), nws)
        img, mask, idx, ws, nws = self._bufs[B]
        st = A.stream_ptr(None) if hasattr(A, "stream_ptr") else A.stream
        L.call("rd_range_image_from_points", A.ptr(pts) if offsets[B] else None, ctypes.addressof(offsets), B, self.incl.ctypes.data,
               self.height.ctypes.data, H, W, A.ptr(img), A.ptr(mask), A.ptr(idx), A.ptr(ws), nws, st)
        m = mask[:B * H * W]
        m = m.view(np.bool_).reshape(B, H, W) if isinstance(m, np.ndarray) else m.view(A.torch.bool).view(B, H, W)
        return {"range_image": A.view_f32(img, (B, H, W, 5)), "range_image_mask": m, "point_index": A.view_i32(idx, (B, H, W))}


def get_range_image(pc, incl, height, width=2048, lib=None, alloc=None):
    """The reference's call shape (:107): pc (N,4) float32, incl / height per beam -> (H, width, 5) float32 NumPy array, -1 in empty
    cells.  (The reference hard-codes width = 2048 and 64 rows.)"""
    t = PointCloudToRangeImage(incl, height, width, lib=lib, alloc=alloc)
    out = t([np.ascontiguousarray(pc, dtype=np.float32).reshape(-1, 4)])["range_image"]
    t.A.sync()
    return np.array(t.A.to_numpy(out))[0]


def main(argv=None, lib=None, alloc=None):
    import argparse
    ap = argparse.ArgumentParser(description="Velodyne scan (.bin: float32 x, y, z, intensity) -> range image (.npz)")
    ap.add_argument("--bin", required=True, help="the scan")
    ap.add_argument("--beams", required=True, help=".npz with `inclination` and `height`, one float64 per beam")
    ap.add_argument("--out", required=True, help=".npz to write: range_image (H,W,5) float32, range_image_mask (H,W) bool")
    ap.add_argument("--width", type=int, default=2048)
    a = ap.parse_args(argv)
    beams = np.load(a.beams)
    pc = np.fromfile(a.bin, dtype=np.float32).reshape(-1, 4)
    img = get_range_image(pc, beams["inclination"], beams["height"], a.width, lib=lib, alloc=alloc)
    np.savez(a.out, range_image=img, range_image_mask=img[..., 0] > -1)


if __name__ == "__main__":
    main()

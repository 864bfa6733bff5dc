"""The drive of the ray-clearing tests: the synthetic room with a seventh box that moves between frames, eight 6 400-ray scans, and which
map voxels are the box's trail.   *** TEST INFRASTRUCTURE ONLY ***   Not collected by pytest (no test_ prefix)."""
from __future__ import annotations

import functools

import numpy as np

import _vgicp_ray_model as ray
from _vgicp_rolling_model import transform_pcl_f32
from direct_lidar_odometry_amd import clouds

FRAMES = 8
COLS = 400


def _scene(f):
    sc = clouds.make_scene()
    cx, cy = -4.0 + 1.2 * f, 5.0
    lo = np.array([[cx - 0.5, cy - 0.5, clouds.FLOOR_Z]])
    hi = np.array([[cx + 0.5, cy + 0.5, clouds.FLOOR_Z + 1.6]])
    return sc, clouds.Scene(np.vstack([sc.boxes_lo, lo]), np.vstack([sc.boxes_hi, hi]))


@functools.lru_cache(maxsize=None)
def frames():
    """-> [(pose float32 (4, 4), points float32 (6400, 3) in the sensor frame, on_box (6400,) bool)] for f = 0 .. 7"""
    out = []
    for f in range(FRAMES):
        pose = clouds.make_pose((0.3 * f, 0.1 * f, 0.0), (0.0, 0.0, 2.0 * f))
        static, moving = _scene(f)
        pts = clouds.vlp16(moving, pose, noise_seed=100 + f, cols=COLS)
        dirs = clouds._ray_dirs(16, COLS, -15.0, 15.0) @ pose[:3, :3].T
        on_box = clouds._raycast(moving, pose[:3, 3], dirs) < clouds._raycast(static, pose[:3, 3], dirs)
        assert len(pts) == 16 * COLS == len(on_box)
        out.append((pose.astype(np.float32), pts, on_box))
    return out


def trail_mask(ijk, res):
    """(V,) bool: every point of frames 0 .. 6 that fell into the voxel lay on the moving box."""
    box_only = {}
    for pose, pts, on_box in frames()[:FRAMES - 1]:
        cells, ok = ray.cells_of(transform_pcl_f32(pose, pts), res)
        assert ok.all()
        for key, b in zip(ray.pack(cells).tolist(), on_box.tolist()):
            box_only[key] = box_only.get(key, True) and b
    return np.array([box_only[k] for k in ray.pack(ijk).tolist()], bool)


def numpy_map(res):
    """The map frames 0 .. 6 leave, without the engine: (ijk, mean, stamp) in the numbering of the definition, each voxel's S summed per
    scan in ascending original index and added to the map scan by scan (the covariances play no part in the clearing)."""
    acc, order = {}, []
    for stamp, (pose, pts, _) in enumerate(frames()[:FRAMES - 1], start=1):
        q = transform_pcl_f32(pose, pts)
        cells, _ = ray.cells_of(q, res)
        q64, sums = q.astype(np.float64), {}
        for j, key in enumerate(map(tuple, cells.tolist())):
            s = sums.setdefault(key, [np.zeros(3), 0])
            s[0] = s[0] + q64[j]
            s[1] += 1
        for key in sorted(sums, key=lambda k: (k[2], k[1], k[0])):
            if key in acc:
                a = acc[key]
                a[0], a[1], a[2] = a[0] + sums[key][0], a[1] + sums[key][1], stamp
            else:
                acc[key] = [sums[key][0], sums[key][1], stamp]
                order.append(key)
    ijk = np.array(order, np.int64)
    mean = np.array([acc[k][0] / float(acc[k][1]) for k in order])
    return ijk, mean, np.array([acc[k][2] for k in order], np.int64)


def report(label, out, trail):
    """the removed trail / static voxels of a clear's model result, printed; -> (trail removed, trail, static removed, static)"""
    gone = ~out["keep"]
    t = (int((gone & trail).sum()), int(trail.sum()), int((gone & ~trail).sum()), int((~trail).sum()))
    print(f"{label}: {t[0]} of {t[1]} trail voxels removed, {t[2]} of {t[3]} static voxels removed; "
          f"{out['steps']} counted steps, {out['occupied']} in occupied cells, {out['misses']} misses")
    return t

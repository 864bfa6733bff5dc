"""A plain numpy statement of removeNaN, CropBox (negative, inclusive bounds) and VoxelGrid, written from the rules in the header
comment of csrc/ngicp_filters.hip and NOT from the oracle's code (oracle/ngicp_oracle.cpp "filters"), so that the two can be proved
against each other (test_filter_cases_cpu.py) before either judges the GPU kernels (test_gpu_filters.py).

  removeNaN   keeps the rows whose x, y, z are all finite, in order.
  CropBox     negative, no pose: drops the rows with -crop <= x, y, z <= crop (a NaN coordinate is not inside), keeps the rest in order.
  VoxelGrid   skips non-finite rows; inverse leaf = float32(1) / float32(leaf); ijk = floor(p * inv_leaf) with a float32 product;
              lattice and voxel index in int64; stable sort by index; per voxel the float32 sums of x, y, z, intensity are
              accumulated one point after the other in input order and divided by the float32 count; ascending index.
  Overflow    VoxelGrid returns ITS input (what removeNaN / CropBox left, non-finite rows included when remove_nan is off) when
              (1) inv_leaf is not finite, or on an axis ext = (max - min) * inv_leaf is not finite or >= 2^31, or the product of
                  int64(ext) + 1 over the axes exceeds INT_MAX (PCL's extent test), or
              (2) floor(min * inv_leaf) or floor(max * inv_leaf) does not fit an int32 on an axis, or
              (3) the product of div = max_b - min_b + 1 exceeds INT_MAX.
"""
import numpy as np

INT_MAX = 2**31 - 1
_F = np.float32


def unpack(cloud, intensity_col) -> np.ndarray:
    """(n, >= 3) rows -> (n, 4) float32 {x, y, z, intensity}; intensity 0 without a column."""
    c = np.asarray(cloud, dtype=_F)
    out = np.zeros((c.shape[0], 4), _F)
    out[:, :3] = c[:, :3]
    if intensity_col is not None and intensity_col >= 0:
        out[:, 3] = c[:, intensity_col]
    return out


def overflows(mn, mx, inv) -> bool:
    """The overflow rule on a float32 bounding box (mn, mx: 3 float32 each) and a float32 inverse leaf."""
    with np.errstate(all="ignore"):
        if not np.isfinite(inv):
            return True
        cells = 1
        for d in range(3):
            ext = _F(_F(mx[d] - mn[d]) * inv)
            if not np.isfinite(ext) or not ext < _F(2**31):
                return True
            cells *= int(ext) + 1  # python ints: no overflow of its own
        if cells > INT_MAX:
            return True
        cells = 1
        for d in range(3):
            flo, fhi = np.floor(_F(mn[d] * inv)), np.floor(_F(mx[d] * inv))
            if not (flo >= _F(-2**31) and fhi < _F(2**31)):  # (both powers of two are exact in float32; false for an infinite product too)
                return True
            cells *= int(fhi) - int(flo) + 1
        return cells > INT_MAX


def filter_cloud(cloud, remove_nan=True, crop=0.0, leaf=0.0, intensity_col=None) -> np.ndarray:
    p = unpack(cloud, intensity_col)
    finite = np.isfinite(p[:, :3]).all(axis=1)
    keep = np.ones(len(p), bool)
    if remove_nan:
        keep &= finite
    if crop > 0:
        c = _F(crop)
        with np.errstate(invalid="ignore"):
            keep &= ~((p[:, :3] >= -c) & (p[:, :3] <= c)).all(axis=1)
    stage_in = p[keep]
    if not leaf > 0:
        return stage_in
    pts = stage_in[np.isfinite(stage_in[:, :3]).all(axis=1)]
    if len(pts) == 0:
        return pts
    with np.errstate(all="ignore"):
        inv = _F(1) / _F(leaf)
    mn, mx = pts[:, :3].min(axis=0), pts[:, :3].max(axis=0)
    if overflows(mn, mx, inv):
        return stage_in
    ijk = np.floor(pts[:, :3] * inv).astype(np.int64)  # float32 product, float32 floor
    min_b = np.floor(mn * inv).astype(np.int64)
    div = np.floor(mx * inv).astype(np.int64) - min_b + 1
    idx = (ijk[:, 0] - min_b[0]) + (ijk[:, 1] - min_b[1]) * div[0] + (ijk[:, 2] - min_b[2]) * div[0] * div[1]
    order = np.argsort(idx, kind="stable")
    sidx = idx[order]
    start = np.flatnonzero(np.r_[True, sidx[1:] != sidx[:-1]])
    count = np.diff(np.r_[start, len(sidx)])
    sums = np.zeros((len(start), 4), _F)
    active = np.arange(len(start))
    j = 0
    with np.errstate(all="ignore"):
        while len(active):  # the j-th member of every voxel that has one: sequential float32 sums in input order
            sums[active] = sums[active] + pts[order[start[active] + j]]
            j += 1
            active = active[count[active] > j]
        return sums / count.astype(_F)[:, None]

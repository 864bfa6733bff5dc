"""The shared case table of the filter tests (test_filter_cases_cpu.py, test_gpu_filters.py): named clouds with the stages to run
on them, built deterministically from seeds.  Every case is valid input; what is expected comes from tests/_filter_model.py.

A case is (name, cloud, intensity_col, remove_nan, crop, leaf); `cloud` is a C-contiguous float32 array, 32 bytes per row
(x y z 1 | intensity 0 0 0, pcl::PointXYZI) unless a case says otherwise."""
import functools
from collections import namedtuple

import numpy as np

import _filter_model as model

Case = namedtuple("Case", "name cloud icol remove_nan crop leaf")

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193)  # wave, block, radix tile, 4-wave block = scan tile
# the stage combinations of tests/test_gpu_submap.py::test_preprocess_scan_matches_oracle_restatement
STAGES = (("nan", True, 0.0, 0.0), ("nan_crop", True, 1.0, 0.0), ("nan_crop_leaf", True, 1.0, 0.25), ("raw_leaf", False, 0.0, 0.5),
          ("nan_fineleaf", True, 0.0, 0.05))
ORDER_INTENSITIES = np.array([1e8, 1.0, -1e8, 1.0], np.float32)  # ((1e8 + 1) - 1e8) + 1 = 1 in float32, reversed ((1 - 1e8) + 1) + 1e8 = 0


def xyzi32(xyz, intensity=None) -> np.ndarray:
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    c = np.zeros((len(xyz), 8), np.float32)
    c[:, :3] = xyz
    c[:, 3] = 1.0
    if intensity is not None:
        c[:, 4] = intensity
    return c


def scan_cloud(n, seed) -> np.ndarray:
    """n rows in a 40 x 40 x 5 m box, about 1 % of them with a NaN / +-Inf coordinate and about 1 % inside the +-1 m crop box."""
    rng = np.random.default_rng(seed)
    xyz = (rng.uniform(-1, 1, (n, 3)) * (20.0, 20.0, 2.5)).astype(np.float32)
    c = xyzi32(xyz, rng.uniform(0, 255, n).astype(np.float32))
    k = max(1, n // 100)
    if n >= 3:
        rows = rng.choice(n, k, replace=False)
        c[rows, :3] = rng.uniform(-0.9, 0.9, (k, 3)).astype(np.float32)
    if n >= 2:
        rows = rng.choice(n, k, replace=False)
        c[rows, rng.integers(0, 3, k)] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), k)
    return c


def keybits_cloud(E, n, seed) -> np.ndarray:
    """Leaf 1.0: n points in [0.6, E - 0.6]^3 of which two are the corner sentinels (0.5, 0.5, 0.5) and (E - 0.5, ...), both off the
    voxel faces, so that the lattice is exactly E^3 cells by PCL's extent rule and by the div product alike.  E = 8, 100, 1000 need
    <= 11, 12-22 and 23-31 key bits (1, 2 and 3 passes of the 11-bit radix sort); 1290^3 = 2 146 689 000 still fits an int, 1291^3
    does not.  The intensities make the float32 sums depend on the order of addition."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0.6, E - 0.6, (n, 3)).astype(np.float32)
    if n >= 3:
        xyz[n // 3] = 0.5
        xyz[2 * n // 3] = E - 0.5
    return xyzi32(xyz, ORDER_INTENSITIES[np.arange(n) % 4])


KEYBIT_E = {"bits11": 8, "bits22": 100, "bits31": 1000, "fits_int": 1290, "overflow": 1291}


def _order_sensitive(n, seed, reverse=False) -> np.ndarray:
    """About ten points per voxel (8^3 voxels of 1 m): intensities cycle through 1e8, 1, -1e8, 1 and the coordinates mix 0.3 with
    0.3 + m * 2^-20 for m up to 2^12, so that an unstable sort, a reversed rank or a tree reduction changes the sums."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 8, (n, 3)).astype(np.float32)
    frac = np.where(rng.random((n, 3)) < 0.5, np.float32(0.3), (np.float32(0.3) + rng.integers(1, 4096, (n, 3)).astype(np.float32) * np.float32(2.0**-20)))
    c = xyzi32(base + frac.astype(np.float32), ORDER_INTENSITIES[np.arange(n) % 4])
    return np.ascontiguousarray(c[::-1]) if reverse else c


def _heavy_voxel(n=20_000, seed=21) -> np.ndarray:
    """One voxel (leaf 64: [64, 128)^3) holds the rows i % 997 == 0, spread over many waves, tiles and blocks; the others lie elsewhere."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-640, 0, (n, 3)).astype(np.float32)
    heavy = np.arange(0, n, 997)
    xyz[heavy] = (64.0 + rng.uniform(0, 1, (len(heavy), 3)) * 2.0 ** -(np.arange(len(heavy)) % 20)[:, None] * 63.0).astype(np.float32)
    it = rng.uniform(0, 255, n).astype(np.float32)
    it[heavy] = ORDER_INTENSITIES[np.arange(len(heavy)) % 4]
    return xyzi32(xyz, it)


def _boundaries(crop) -> np.ndarray:
    f = np.float32
    ks = np.arange(-9, 10, dtype=np.float32)
    rows = []
    for step in (f(0.25), f(0.5), f(0.1)):  # exactly on k * leaf (0.1: the multiples of float32(0.1), which is not 1/10)
        for k in ks:
            rows += [(k * step, f(3.0), f(-3.0)), (f(3.0), k * step, k * step), (k * step, k * step, k * step)]
    rows += [(f(-0.0), f(-0.0), f(-0.0)), (f(-0.0), f(2.0), f(0.0)), (f(0.0), f(-2.0), f(-0.0))]
    c = f(crop)
    out_p, out_m = np.nextafter(c, f(np.inf)), np.nextafter(-c, f(-np.inf))
    in_p, in_m = np.nextafter(c, f(0)), np.nextafter(-c, f(0))
    for a in (c, -c, in_p, in_m, out_p, out_m):  # exactly on / just inside (removed), just outside (kept) the box, per axis
        rows += [(a, f(0.5), f(-0.5)), (f(0.5), a, f(-0.5)), (f(-0.5), f(0.5), a), (a, a, a), (a, -a, a)]
    rows += [(f(-7.3), f(-0.2), f(-11.9)), (f(-1.5), f(-1.5), f(-1.5)), (f(-1e-30), f(-1e-30), f(-2.0))]  # negative in all coordinates
    xyz = np.array(rows, np.float32)
    return xyzi32(xyz, np.arange(len(xyz), dtype=np.float32))


def _unusual(seed=31) -> np.ndarray:
    rng = np.random.default_rng(seed)
    n = 700
    c = xyzi32((rng.uniform(-1, 1, (n, 3)) * 6.0).astype(np.float32), rng.uniform(0, 255, n).astype(np.float32))
    c[5, 0], c[70, 1], c[300, 2] = np.inf, -np.inf, np.inf
    c[130, :3] = (np.inf, -np.inf, np.nan)
    c[64, 0], c[65, 2], c[699, 1] = np.nan, np.nan, np.nan
    c[200, :3] = (0.3, np.nan, -0.4)        # the finite coordinates inside the crop box
    c[201, :3] = (np.inf, 0.2, 0.2)
    c[10, 4] = np.nan                        # NaN intensity on a finite point: kept, and its voxel's intensity is NaN
    c[400, :3] = c[10, :3] + np.float32(0.001)
    c[401, 4] = np.inf
    return c


def _far_cluster() -> np.ndarray:
    rng = np.random.default_rng(41)
    return xyzi32((3e9 + rng.uniform(0, 4096, (500, 3))).astype(np.float32), rng.uniform(0, 255, 500).astype(np.float32))


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = []

    def add(name, cloud, remove_nan, crop, leaf, icol=4):
        cloud = np.ascontiguousarray(cloud, dtype=np.float32)
        cloud.setflags(write=False)
        out.append(Case(name, cloud, icol, remove_nan, crop, leaf))

    for i, n in enumerate(SIZES):
        c = scan_cloud(n, 100 + i)
        for tag, rn, crop, leaf in STAGES:
            add(f"n{n}-{tag}", c, rn, crop, leaf)
    rng = np.random.default_rng(7)
    add("large-600001", scan_cloud(600_001, 8), True, 1.0, 0.25)
    for tag, E in KEYBIT_E.items():
        add(f"keybits-{tag}-E{E}", keybits_cloud(E, 5002, 50 + E), True, 0.0, 1.0)
    pts5000 = (rng.uniform(-1, 1, (5000, 3)) * 50.0).astype(np.float32)
    add("one-voxel-leaf1e6", xyzi32(pts5000 + np.float32(51.0), ORDER_INTENSITIES[np.arange(5000) % 4]), True, 0.0, 1e6)
    grid = np.stack(np.meshgrid(np.arange(-8, 9), np.arange(-8, 9), np.arange(-8, 9), indexing="ij"), -1).reshape(-1, 3)
    add("own-voxel-each", xyzi32(grid[rng.permutation(len(grid))], rng.uniform(0, 255, len(grid)).astype(np.float32)), True, 0.0, 0.5)
    add("heavy-voxel-spread", _heavy_voxel(), True, 0.0, 64.0)
    add("order-sensitive", _order_sensitive(5000, 61), True, 0.0, 1.0)
    add("order-sensitive-9000", _order_sensitive(9000, 62), False, 0.0, 1.0)
    b = _boundaries(1.0)
    for tag, rn, crop, leaf in (("crop", True, 1.0, 0.0), ("crop-leaf025", True, 1.0, 0.25), ("leaf025", True, 0.0, 0.25), ("leaf05", False, 0.0, 0.5),
                                ("leaf01", True, 0.0, 0.1)):
        add(f"boundaries-{tag}", b, rn, crop, leaf)
    nan_rows = scan_cloud(300, 71).copy()
    nan_rows[np.arange(300), rng.integers(0, 3, 300)] = np.nan
    nan_rows[::3, :3] = np.nan
    inside = xyzi32(rng.uniform(-0.99, 0.99, (300, 3)).astype(np.float32), rng.uniform(0, 255, 300).astype(np.float32))
    inside[0, :3], inside[299, :3] = 1.0, (-1.0, 1.0, -1.0)
    for tag, leaf in (("", 0.0), ("-leaf", 0.25)):
        add(f"nothing-survives-all-nan{tag}", nan_rows, True, 0.0, leaf)
        add(f"nothing-survives-all-inside{tag}", inside, True, 1.0, leaf)
    add("nothing-survives-all-nan-raw-leaf", nan_rows, False, 0.0, 0.25)
    u = _unusual()
    for tag, rn, crop, leaf in (("raw", False, 0.0, 0.0), ("raw-crop", False, 1.0, 0.0), ("nan", True, 0.0, 0.0), ("nan-crop-leaf", True, 1.0, 0.25),
                                ("raw-leaf", False, 0.0, 0.5)):
        add(f"unusual-{tag}", u, rn, crop, leaf)
    # ---- the overflow rule ----
    pts2000 = xyzi32(pts5000[:2000], rng.uniform(0, 255, 2000).astype(np.float32))
    for leaf in (1e-6, 1e-8, 1e-9, 1e-12, 1e-42):
        add(f"overflow-leaf{leaf:g}", pts2000, True, 0.0, leaf)
    stray = pts2000.copy()
    stray[1234, :3] = (3e9, 1.0, -2.0)
    add("overflow-stray-3e9", stray, True, 0.0, 1.0)
    add("overflow-single-3e9", xyzi32([(3e9, 0.0, 0.0)], [7.0]), True, 0.0, 1.0)
    add("overflow-far-cluster", _far_cluster(), True, 0.0, 1.0)
    with_nan = scan_cloud(2000, 81)
    add("overflow-raw-nan-rows-leaf1e-9", with_nan, False, 0.0, 1e-9)
    add("overflow-raw-nan-rows-crop-leaf1e-9", with_nan, False, 1.0, 1e-9)
    add("overflow-nan-removed-leaf1e-9", with_nan, True, 1.0, 1e-9)
    return tuple(out)


def names() -> list:
    return [c.name for c in cases()]


def by_name(name) -> Case:
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name) -> np.ndarray:
    """The model's answer, computed once per process and shared (read-only)."""
    c = by_name(name)
    r = model.filter_cloud(c.cloud, c.remove_nan, c.crop, c.leaf, c.icol)
    r.setflags(write=False)
    return r


def same_bits(a, b, nan_equal=False) -> bool:
    """Bit for bit as uint32 views (so -0.0 is not 0.0); with nan_equal any NaN equals any NaN (centroids of a voxel that holds a NaN
    intensity: a NaN's payload after arithmetic is not part of the rules)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    eq = a.view(np.uint32) == b.view(np.uint32)
    if nan_equal:
        eq |= np.isnan(a) & np.isnan(b)
    return bool(eq.all())


def same(case, a, b) -> bool:
    """Survivors without a leaf are copies: raw bits.  Centroids: bits, NaN equal to NaN."""
    return same_bits(a, b, nan_equal=case.leaf > 0)

"""The yardstick of the filter tests, without a GPU: on every case of tests/_filter_cases.py the oracle's C++ restatement of
removeNaN / CropBox / VoxelGrid (oracle/ngicp_oracle.cpp "filters") and the independent numpy model (tests/_filter_model.py) agree bit
for bit - so test_gpu_filters.py judges the kernels by two statements of the rules that were proved against each other first - and the
table really holds what it is meant to hold: the key-bit classes, the order-sensitive sums, the overflow cases that return their input."""
import numpy as np
import pytest

import _filter_cases as fc
import _filter_model as model


@pytest.mark.parametrize("name", fc.names())
def test_oracle_equals_model(oracle_mod, name):
    c = fc.by_name(name)
    ref = oracle_mod.filter_cloud(c.cloud, c.remove_nan, c.crop, c.leaf, intensity_col=c.icol)
    exp = fc.expected(name)
    print(f"{name}: {len(c.cloud)} rows -> oracle {len(ref)}, model {len(exp)}")
    assert ref.shape == exp.shape
    assert fc.same(c, ref, exp)


def _lattice_bits(c):
    p = fc.expected(c.name)
    pts = model.filter_cloud(c.cloud, True, c.crop, 0.0, c.icol)[:, :3]  # (the lattice is recomputed here from the rules)
    inv = np.float32(1) / np.float32(c.leaf)
    div = np.floor(pts.max(axis=0) * inv).astype(np.int64) - np.floor(pts.min(axis=0) * inv).astype(np.int64) + 1
    return int(div[0]) * int(div[1]) * int(div[2]), len(p), fc.same_bits(p, model.unpack(c.cloud, c.icol))


def test_keybit_classes_are_what_they_claim():
    cells = {tag: _lattice_bits(fc.by_name(f"keybits-{tag}-E{E}")) for tag, E in fc.KEYBIT_E.items()}
    print("lattice cells, output rows, output is the input:", cells)
    assert cells["bits11"][0] == 8**3 and cells["bits11"][0] <= 2**11
    assert 2**11 < cells["bits22"][0] == 100**3 <= 2**22
    assert 2**22 < cells["bits31"][0] == 1000**3 <= 2**31 - 1
    assert cells["fits_int"][0] == 2_146_689_000 <= 2**31 - 1 < cells["overflow"][0] == 1291**3
    assert not cells["fits_int"][2] and cells["overflow"][2]  # filtered (in voxel order) / returned as it is
    assert 400 < cells["bits11"][1] <= 512  # about ten points per voxel


@pytest.mark.parametrize("name", [n for n in fc.names() if n.startswith("overflow-") or n == "keybits-overflow-E1291"])
def test_overflow_cases_return_the_voxel_stage_input(name):
    c = fc.by_name(name)
    stage_in = model.filter_cloud(c.cloud, c.remove_nan, c.crop, 0.0, c.icol)
    assert len(stage_in) > 0 and fc.same_bits(fc.expected(name), stage_in)
    if not c.remove_nan:
        assert not np.isfinite(stage_in[:, :3]).all()  # the non-finite rows are part of that input


def test_leaf_1e6_is_not_an_overflow_but_1e8_is():
    """The table of the defect as it was found: 2000 points in +-50 m came back as 1651, 229 and 1 points at leaves 1e-8, 1e-9, 1e-12."""
    assert [len(fc.expected(f"overflow-leaf{leaf:g}")) for leaf in (1e-6, 1e-8, 1e-9, 1e-12)] == [2000] * 4


@pytest.mark.parametrize("name", ["order-sensitive", "order-sensitive-9000", "heavy-voxel-spread", "keybits-bits11-E8", "one-voxel-leaf1e6"])
def test_order_sensitive_cases_depend_on_the_order_of_addition(name):
    """The same points added in reverse order inside every voxel must give other sums: else a stable and an unstable sort, or a
    forward and a backward sum, could not be told apart by this case."""
    c = fc.by_name(name)
    fwd = fc.expected(name)
    rev = model.filter_cloud(c.cloud[::-1], c.remove_nan, c.crop, c.leaf, c.icol)
    assert fwd.shape == rev.shape
    differs = (fwd.view(np.uint32) != rev.view(np.uint32))
    print(f"{name}: voxels whose x / y / z / intensity sums depend on the order:", differs.sum(axis=0), "of", len(fwd))
    assert differs[:, 3].any() and differs[:, :3].any()


def test_intensity_cycle_sums_to_quarter_forward_and_zero_reversed():
    pts = fc.xyzi32(np.full((4, 3), 0.3, np.float32), fc.ORDER_INTENSITIES)
    assert model.filter_cloud(pts, True, 0.0, 1.0, 4)[0, 3] == np.float32(0.25)
    assert model.filter_cloud(pts[::-1], True, 0.0, 1.0, 4)[0, 3] == np.float32(0.0)


def test_occupancy_extremes():
    assert len(fc.expected("one-voxel-leaf1e6")) == 1
    assert len(fc.expected("own-voxel-each")) == 17**3
    c = fc.by_name("heavy-voxel-spread")
    idx = np.flatnonzero((c.cloud[:, :3] >= 64).all(axis=1))
    assert np.array_equal(idx, np.arange(0, 20_000, 997)) and len(fc.expected("heavy-voxel-spread")) > 500
    for n in fc.names():
        if n.startswith("nothing-survives"):
            assert len(fc.expected(n)) == 0


def test_boundary_and_unusual_cases_hold_what_they_claim():
    b = fc.by_name("boundaries-crop")
    kept = fc.expected("boundaries-crop")
    one, out = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    assert (np.abs(b.cloud[:, :3]) == one).any() and not ((np.abs(kept[:, :3]) <= one).all(axis=1)).any()
    assert (np.abs(kept[:, :3]).max(axis=1) == out).sum() >= 10            # just outside: kept
    assert np.signbit(b.cloud[:, :3]).all(axis=1).sum() >= 10               # negative in all coordinates (and -0.0)
    u = fc.by_name("unusual-raw")
    raw = fc.expected("unusual-raw")
    assert fc.same_bits(raw, model.unpack(u.cloud, 4)) and np.isinf(raw[:, :3]).any() and np.isnan(raw[:, :3]).any()
    assert len(fc.expected("unusual-raw-crop")) < len(raw) and np.isnan(fc.expected("unusual-raw-crop")[:, 1]).sum() == np.isnan(raw[:, 1]).sum()
    vox = fc.expected("unusual-raw-leaf")
    assert np.isfinite(vox[:, :3]).all() and np.isnan(vox[:, 3]).sum() == 1 and np.isinf(vox[:, 3]).sum() == 1

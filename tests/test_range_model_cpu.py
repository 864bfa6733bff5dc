"""The numpy model of the range select and its case generators (tests/_range_model.py), checked without a GPU: the model against a
plain full sort, the generators against what they claim, the engine's rounding rule (restated) against numpy's correctly rounded
sqrt, and the declared ABI."""
import os
import re

import numpy as np
import pytest

import _range_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    out = {f"random_{n}": rm.random_cloud(n) for n in rm.EDGE_SIZES}
    out.update(all_equal=rm.all_equal(), low_bits=rm.low_bits_only(), top_bits=rm.top_bits_only(), two_values=rm.two_values(),
               big_bin=rm.big_bin(), ties=rm.rounding_ties(), nonfinite=rm.with_nonfinite_rows()[0])
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_equals_a_full_sort(name):
    c = CASES[name]
    d = np.sort(rm.ranges(c))  # numpy sorts NaN last
    for r in rm.ranks_for(len(c)):
        assert rm.same_bits(rm.select(c, r), d[r]), r
    assert rm.same_bits(rm.median(c), d[len(c) // 2])


def test_ranks_cover_every_rank_of_small_clouds_and_the_ends_of_large_ones():
    assert rm.ranks_for(257) == list(range(257))
    r = rm.ranks_for(2049)
    assert {0, 1, 1024, 2047, 2048} <= set(r) and len(r) >= 16 and max(r) < 2049


def test_generators_produce_what_they_claim():
    assert len(np.unique(rm.ranges(rm.all_equal()))) == 1
    d = rm.ranges(rm.low_bits_only(700))
    k = rm.keys(d)
    assert len(np.unique(k)) == 700 and len(np.unique(k >> 10)) == 1 and np.array_equal(np.sort(k), k.min() + np.arange(700, dtype=np.uint32))
    assert (rm.digit_counts(d, 0) > 0).sum() == 1 and (rm.digit_counts(d, 1, int(k[0])) > 0).sum() == 1 and (rm.digit_counts(d, 2, int(k[0])) == 1).sum() == 700
    d = rm.ranges(rm.top_bits_only())
    k = rm.keys(d)
    assert np.array_equal(np.sort(d), np.ldexp(np.float32(1), np.arange(-20, 21)).astype(np.float32))
    assert not (k & np.uint32((1 << 21) - 1)).any() and (rm.digit_counts(d, 0) == 1).sum() == 41
    c = rm.two_values(301, 212)
    d = np.sort(rm.ranges(c))
    assert np.array_equal(np.unique(d), np.array([5, 13], np.float32)) and d[300] == 5 and d[301] == 13
    c = rm.big_bin()
    d = rm.ranges(c)
    assert len(c) == 70_050 and d[d == 7].size >= 70_000
    top = int(rm.keys(np.float32(7))[()])
    assert max(rm.digit_counts(d, 0).max(), rm.digit_counts(d, 1, top).max(), rm.digit_counts(d, 2, top).max()) > 65_535
    c, n_nan, n_inf = rm.with_nonfinite_rows()
    d = rm.ranges(c)
    assert np.isnan(d).sum() == n_nan and np.isposinf(d).sum() == n_inf
    s = np.sort(d)
    assert np.isnan(s[-n_nan:]).all() and np.isposinf(s[-n_nan - n_inf:-n_nan]).all() and np.isfinite(s[:-n_nan - n_inf]).all()
    assert rm.same_bits(rm.select(c, len(c) - 1), np.nan) and rm.select(c, len(c) - n_nan - 1) == np.inf


def test_rounding_ties_are_ties():
    c = rm.rounding_ties()
    assert c.shape == (4096, 3)
    u = rm.tie_distance_ulps(c[:-4])
    assert (u <= 1.0).all()  # within one double ulp of a tie of the root
    assert (u == 0).any() and (u > 0).any()
    d = rm.ranges(c)
    assert d[-4] == 0 and d[-3] == np.float32(1e-40) and d[-3] > 0 and d[-2] == np.float32(3e38) and d[-1] == np.inf
    # the double rounding matters here: rounding the (nearly exact) long double root straight to float gives other bits on some rows
    if np.finfo(np.longdouble).nmant > 52:
        x, y, z = (c[:-4, k].astype(np.float64) for k in range(3))
        s = x * x + y * y + z * z
        direct = np.sqrt(s.astype(np.longdouble)).astype(np.float32)
        assert (direct.view(np.uint32) != d[:-4].view(np.uint32)).any()


@pytest.mark.parametrize("offset", [0, 1, -1])
def test_midpoint_rule_reproduces_the_correctly_rounded_root(offset):
    """The correction the kernel applies (csrc/ngicp_range.h range_key) reaches numpy's float(sqrt_double(s)) bit for bit from a
    candidate one float step off on either side: on the ties, the extremes, non-finite rows and ordinary points."""
    c = np.concatenate([rm.rounding_ties(600, seed=11), rm.with_nonfinite_rows(400)[0], rm.random_cloud(200, 9), rm.top_bits_only()])
    assert np.array_equal(rm.key_by_midpoint_rule(c, offset), rm.keys(rm.ranges(c)))


def test_lowpass_restatement():
    out = rm.lowpass_f32([10.0, 20.0, 20.0])
    assert out[0] == np.float32(10.0)
    assert out[1] == np.float32(0.95 * 10.0 + 0.05 * 20.0) and out[2] == np.float32(0.95 * float(out[1]) + 0.05 * 20.0)
    assert all(isinstance(v, np.float32) for v in out)


def test_abi_declares_the_range_entries():
    from direct_lidar_odometry_amd import nano_gicp
    with open(os.path.join(ROOT, "include", "ngicp.h")) as f:
        declared = set(re.findall(r"\b(ngicp_range_\w+)\s*\(", f.read()))
    assert declared == {"ngicp_range_select", "ngicp_range_median"} <= set(nano_gicp.EXPORTS)
    assert hasattr(nano_gicp.NanoGICP, "rangeSelect") and hasattr(nano_gicp.NanoGICP, "medianRange")

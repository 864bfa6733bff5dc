"""numpy model of the engine's range select (include/ngicp.h "range select") and the clouds its tests run on.

The range of a point is what src/dlo/odom.cc:996 of the reference computes: the squares and their left-to-right sum in double,
std::sqrt in double (correctly rounded, as numpy's), narrowed to float.  Ranges are ordered ascending with NaN after +inf, which is
numpy's sort order.  The CPU tests (test_range_model_cpu.py) check the model and the generators; the GPU tests
(test_gpu_range.py) run the engine on the same clouds and compare bit for bit."""
import numpy as np

F4, F8 = np.float32, np.float64


def ranges(cloud) -> np.ndarray:
    c = np.asarray(cloud, F4)
    x, y, z = c[:, 0].astype(F8), c[:, 1].astype(F8), c[:, 2].astype(F8)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt(x ** 2 + y ** 2 + z ** 2).astype(F4)


def select(cloud, r: int) -> np.float32:
    d = ranges(cloud)
    return np.partition(d, r)[r]


def median(cloud) -> np.float32:
    return select(cloud, len(cloud) // 2)


def same_bits(a, b) -> bool:
    """Bit equality of two float32 values; every NaN equals every NaN (the engine returns the quiet NaN 0x7fc00000)."""
    a, b = F4(a), F4(b)
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    return a.view(np.uint32) == b.view(np.uint32)


def keys(d) -> np.ndarray:
    """The engine's 32-bit sort key of a range: the float's bit pattern, 0xffffffff for NaN."""
    d = np.asarray(d, F4)
    return np.where(np.isnan(d), np.uint32(0xFFFFFFFF), d.view(np.uint32))


def digit_counts(d, round_: int, prefix: int = 0) -> np.ndarray:
    """Points per bin of round 0 / 1 / 2 of the 11 + 11 + 10 bit radix select, among the keys that share `prefix`'s higher bits."""
    k = keys(d).astype(np.uint64)
    keep_shift, digit_shift, bins = ((32, 21, 2048), (21, 10, 2048), (10, 0, 1024))[round_]
    if keep_shift < 32:
        k = k[(k >> np.uint64(keep_shift)) == np.uint64(prefix >> keep_shift)]
    return np.bincount(((k >> np.uint64(digit_shift)) & np.uint64(bins - 1)).astype(np.int64), minlength=bins)


# ---------------------------------------------------------------------------------------------------------------- the rounding rule
def key_by_midpoint_rule(cloud, candidate_offset: int = 0) -> np.ndarray:
    """The engine's range_key (csrc/ngicp_range.h) restated: start from a float candidate `candidate_offset` steps away from
    (float)sqrt(s) and correct it against the float rounding boundaries in exact double arithmetic - no reliance on a correctly
    rounded sqrt.  For a boundary m between the floats g < g', u = ulp_double(m), t = m u, e = s - m^2: e > t above, e <= -t below,
    otherwise the correctly rounded double root IS m and the tie goes to the even float."""
    c = np.asarray(cloud, F4)
    x, y, z = c[:, 0].astype(F8), c[:, 1].astype(F8), c[:, 2].astype(F8)
    with np.errstate(over="ignore", invalid="ignore"):
        s = x * x + y * y + z * z
        cand = np.sqrt(s).astype(F4)
    out = np.empty(len(c), np.uint32)
    for i in range(len(c)):
        si = s[i]
        if np.isnan(si):
            out[i] = 0xFFFFFFFF
            continue
        if np.isinf(si):
            out[i] = 0x7F800000
            continue
        f = min(max(int(cand[i].view(np.uint32)) + candidate_offset, 0), 0x7F800000)
        for _ in range(4):
            if f < 0x7F800000:
                side = _side(si, f)
                if side > 0 or (side == 0 and f & 1):
                    f += 1
                    continue
            if f > 0:
                side = _side(si, f - 1)
                if side < 0 or (side == 0 and f & 1):
                    f -= 1
                    continue
            break
        out[i] = f
    return out


def _side(s: float, g: int) -> int:
    ef = max(g >> 23, 1)
    m = F8(np.uint32(g).view(F4)) + F8(2.0) ** (ef - 151)  # g + half a float step
    u = np.spacing(m)
    e, t = F8(s) - m * m, m * u
    return 1 if e > t else (-1 if e <= -t else 0)


# ------------------------------------------------------------------------------------------------------------------------- clouds
EDGE_SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 2049)


def random_cloud(n: int, seed: int = 0) -> np.ndarray:
    """A LiDAR-like spread of ranges (a fraction of a metre to about a hundred), every direction."""
    rng = np.random.default_rng(1000 + seed + n)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.exp(rng.uniform(np.log(0.3), np.log(120.0), size=(n, 1)))
    return (d * r).astype(F4)


def ranks_for(n: int, seed: int = 0):
    """Every rank up to n = 257; above, the ends, the median and 16 random ranks."""
    if n <= 257:
        return list(range(n))
    rng = np.random.default_rng(7 + seed + n)
    return sorted({0, 1, n // 2, n - 2, n - 1, *rng.integers(0, n, 16).tolist()})


def all_equal(n: int = 300) -> np.ndarray:
    return np.tile(np.array([[1.5, -2.25, 7.0]], F4), (n, 1))


def low_bits_only(n: int = 700, seed: int = 1) -> np.ndarray:
    """Ranges that are n consecutive floats (they differ in the low 10 bits only: n <= 1024 and the first one's are zero), shuffled;
    points on the x axis, where the range is |x| exactly."""
    assert n <= 1024
    bits = np.uint32(np.float32(10.0).view(np.uint32) & ~np.uint32(1023)) + np.arange(n, dtype=np.uint32)
    x = bits.view(F4)
    c = np.zeros((n, 3), F4)
    c[:, 0] = np.random.default_rng(seed).permutation(x)
    c[::2, 0] *= -1
    return c


def top_bits_only(seed: int = 2) -> np.ndarray:
    """Ranges 2^-20 .. 2^20: they differ in the exponent, inside the top 11 bits of the key, and in nothing below."""
    x = np.ldexp(F4(1.0), np.arange(-20, 21)).astype(F4)
    c = np.zeros((len(x), 3), F4)
    c[:, 1] = np.random.default_rng(seed).permutation(x)
    return c


def two_values(n_low: int = 301, n_high: int = 212, seed: int = 3) -> np.ndarray:
    """n_low points of range 5 and n_high of range 13, shuffled: ranks n_low - 1 and n_low straddle the boundary."""
    c = np.concatenate([np.tile(np.array([[3.0, 4.0, 0.0]], F4), (n_low, 1)), np.tile(np.array([[0.0, 5.0, -12.0]], F4), (n_high, 1))])
    return c[np.random.default_rng(seed).permutation(len(c))]


def big_bin(copies: int = 70_000, others: int = 50, seed: int = 4) -> np.ndarray:
    """One point repeated more than 65 535 times plus a few others: one bin of every round overflows a 16-bit counter."""
    c = np.concatenate([np.tile(np.array([[2.0, -3.0, 6.0]], F4), (copies, 1)), random_cloud(others, seed)])
    return c[np.random.default_rng(seed).permutation(len(c))]


def rounding_ties(n: int = 4096, seed: int = 5, extremes: bool = True) -> np.ndarray:
    """Points whose double sum s lies within one double ulp of m^2, m a boundary between two neighbouring floats (a rounding tie of
    the root): x is the float below m, y and z are searched so that x^2 + y^2 + z^2 lands near (x + half a float step)^2.  There the
    float range depends on the double rounding of the root: sqrt(s) rounds to m itself in double, and the tie then goes to the even
    float, where the exact root would have gone to the nearer one.  With `extremes` the last rows are the zero point, a denormal
    coordinate, 3e38 on one axis (the double sum stays finite, a float sum would not) and 3e38 on all three (the range is +inf)."""
    rng = np.random.default_rng(seed)
    tail = np.array([[0.0, 0.0, 0.0], [1e-40, 0.0, 0.0], [0.0, -3e38, 0.0], [3e38, 3e38, -3e38]], F4) if extremes else np.zeros((0, 3), F4)
    want = n - len(tail)
    got = []
    f = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), 2 * want)).astype(F4)
    half = (np.spacing(f) / 2).astype(F8)
    m = f.astype(F8) + half
    m2 = m * m  # 25 significant bits squared: exact
    r = m2 - f.astype(F8) ** 2  # = half * (2 f + half): exact
    y = np.sqrt(r).astype(F4)
    y = np.where(y.astype(F8) ** 2 > r, np.nextafter(y, F4(0)), y)
    res = r - y.astype(F8) ** 2
    for k in (0, 1, -1):  # aim at m^2 itself and at its two double neighbours: both sides of the tie come up
        z = np.sqrt(np.maximum(res + k * np.spacing(m2), 0.0)).astype(F4)
        c = np.stack([f, y, z], axis=1)
        x8, y8, z8 = (c[:, j].astype(F8) for j in range(3))
        s = x8 * x8 + y8 * y8 + z8 * z8
        near = np.abs(s - m2) <= np.spacing(m2)
        got.append(c[near][:(want + 2) // 3])
    assert sum(len(g) for g in got) >= want
    c = np.concatenate(got)[:want]
    signs = rng.choice(np.array([-1.0, 1.0], F4), size=c.shape)
    return np.concatenate([c * signs, tail]).astype(F4)


def tie_distance_ulps(cloud) -> np.ndarray:
    """|s - m^2| in ulps of m^2 for the float boundary m nearest to sqrt(s) (finite, positive s only; NaN elsewhere)."""
    c = np.asarray(cloud, F4)
    x, y, z = (c[:, k].astype(F8) for k in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        s = x * x + y * y + z * z
        root = np.sqrt(s)
        f = root.astype(F4)
        out = np.full(len(c), np.nan)
        ok = np.isfinite(f) & (f > 0)
        best = np.full(len(c), np.inf)
        for g in (np.nextafter(f, F4(0)), f):  # the boundary above g
            m = g.astype(F8) + (np.spacing(g) / 2).astype(F8)
            m2 = m * m
            best = np.minimum(best, np.abs(s - m2) / np.spacing(m2))
        out[ok] = best[ok]
    return out


def with_nonfinite_rows(n: int = 500, seed: int = 6):
    """A random cloud with NaN and inf rows mixed in -> (cloud, number of NaN ranges, number of +inf ranges)."""
    c = random_cloud(n, seed)
    c[5, 0] = np.nan
    c[77, 2] = np.nan
    c[200] = (np.inf, np.nan, 0.0)  # NaN wins
    c[123, 1] = np.inf
    c[300, 0] = -np.inf
    c[301] = (np.inf, -np.inf, 1.0)  # inf + inf = inf, not NaN
    return c, 3, 3


def lowpass_f32(medians):
    """computeSpaciousness's low-pass (odom.cc:1003-1005): a float state seeded with the first median, the update evaluated in
    double (the literals 0.95 and 0.05 are doubles) and narrowed to float."""
    out, prev = [], None
    for m in medians:
        m = F4(m)
        if prev is None:
            prev = m
        prev = F4(0.95 * float(prev) + 0.05 * float(m))
        out.append(prev)
    return out

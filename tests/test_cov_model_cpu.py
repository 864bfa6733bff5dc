"""CPU check of tests/_cov_model.py: the oracle's covariances against the numpy definition model on every input family, every k
and every regularisation, and the caps that keep tests/test_gpu_covariances_edges.py honest (how many rows it may leave out).

MEASURED (seed _cov_model.SEED; `PYTHONPATH=. python tests/test_cov_model_cpu.py` prints the table):
  max |oracle - model| on the rows compared by value, over all families and k (tolerance 1e-9, every family must stay below 5e-10):
    NONE                0         (both sum the same float64 products in the same order)
    MIN_EIG             1.8e-14   (lidar, k = 32)
    NORMALIZED_MIN_EIG  2.2e-15   (far_utm, k = 20)
    PLANE               8.8e-11   (lidar, k = 3)
    FROBENIUS           2.2e-10   (dups4, k = 10)
  FROBENIUS is what sets the families' extents.  Its two 3x3 inverses are cofactor inverses (as the reference's are); on a
  neighbourhood of rank <= 2 with largest eigenvalue L the cofactors of C + 1e-3 I cancel from L^2 down to 1e-3 L, and the
  difference to numpy's LU inverse grew faster than L^2: 5.5e-6 at L = 15 (Gaussian, sigma 5 m, k = 2), 1.8e-8 at L = 1.3
  (line_diag over +-10 m, k = 32), 2.2e-9 (tilted plane over +-5 m, k = 32).  So the planes span +-2 m, line_diag +-3 m, the tiny
  clouds have sigma 0.3 m, `far` sigma 0.5 m, and `far_utm` sigma 0.75 m instead of 5 m (at 0.5 m its y quantum of 0.25 m
  stacked 2.2 % of the k = 3 neighbourhoods on exact vertical lines, over the 2 % cap; at 0.75 m it is 0.5 %).
  Ambiguous rows (cap 1 %): 0 in every family and every k.
  PLANE rows without a separated normal where the cap of 2 % applies (rank >= 2 by construction, k >= 3):
    plane_z 0.33 % (k = 3), far_utm 0.50 % (k = 3), every other family 0.
  `lidar` carries an isotropic jitter of 1 cm: a 2000-point 16-ring scan has 125 columns, the three nearest points are the point
  and its ring neighbours in the same column, and range noise alone keeps them in the column's vertical plane, where 2.4 to 3.3 %
  of them (noise seeds 0 to 3) were collinear to 1e-3 of their length; with the jitter it is 0.
"""
import numpy as np
import pytest

import _cov_model as cm


ORACLE_SYM_TOL = 1e-15  # the oracle forms all nine entries of V f V^T: symmetric to rounding only (_cov_model.check_case)


def _skip_cap_applies(name, k):
    from_k = cm.RANK2_FROM_K.get(name, 3)
    return from_k is not None and k >= max(3, from_k)


def test_families_are_what_they_claim():
    fam = cm.families()
    assert set(fam) >= {"plane_x", "plane_y", "plane_z", "plane_tilted", "line_x", "line_y", "line_z", "line_diag", "dups4", "dups_k", "far",
                        "lidar"} | {f"tiny_n{n}" for n in (1, 2, 3, 10, 11, 20, 21, 32, 33)}
    for name, p in fam.items():
        assert p.dtype == np.float32 and p.ndim == 2 and p.shape[1] == 3 and p.flags.c_contiguous and np.all(np.isfinite(p))
        if not name.startswith("tiny"):
            assert 500 <= len(p) <= 2000, name
    assert len(fam["lidar"]) == 2000  # not divisible by 3: the emulated three-rank split is uneven
    for axis, name in enumerate("xyz"):
        assert np.all(fam["plane_" + name][:, axis] == np.float32(1.25))
        others = [a for a in range(3) if a != axis]
        assert np.all(fam["line_" + name][:, others] == fam["line_" + name][0, others])
        assert len(np.unique(fam["line_" + name][:, axis])) > 490
    d = fam["line_diag"]
    assert np.all(d[:, 0] == d[:, 1]) and np.all(d[:, 0] == d[:, 2])
    for name, copies, sites in (("dups4", 4, 300), ("dups_k", 32, 30)):
        u, c = np.unique(fam[name], axis=0, return_counts=True)
        assert len(u) == sites and np.all(c == copies)
    assert np.abs(fam["far"].mean(axis=0) - [4000, -2500, 30]).max() < 0.2
    if "far_utm" in fam:  # quantised by float32: x in steps of 1/32 m, y in steps of 1/4 m
        assert np.all(fam["far_utm"][:, 1].astype(np.float64) % 0.25 == 0)


def test_ambiguity_mask_separates_real_ties_from_coincident_copies(oracle_mod):
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    nbr, amb = cm.neighbour_sets(oracle_mod, g, 3)  # a lattice: six neighbours at distance 1, k = 3 cuts through them
    assert nbr.shape == (216, 3) and amb.all()
    _, amb = cm.neighbour_sets(oracle_mod, g, 1)  # the point itself, strictly nearest
    assert not amb.any()
    rng = np.random.default_rng(0)
    sites = rng.normal(size=(12, 3)).astype(np.float32)
    copies = np.repeat(sites, 40, axis=0)  # 40 coincident copies: the tie run at k = 3 is longer than k + 8 and must be re-queried
    nbr, amb = cm.neighbour_sets(oracle_mod, copies, 3)
    assert not amb.any() and np.all(copies[nbr] == copies[:, None, :])
    _, amb = cm.neighbour_sets(oracle_mod, copies, 40)  # the 40 copies exactly, then a strictly farther site
    assert not amb.any()
    # two DIFFERENT points at the same distance behind a run of copies: ambiguous, and only for the rows that see them
    p = np.array([[0, 0, 0]] * 3 + [[1, 0, 0], [-1, 0, 0], [0, 7, 0]], np.float32)
    _, amb = cm.neighbour_sets(oracle_mod, p, 4)
    assert amb[:3].all() and not amb[3:].any()
    _, amb = cm.neighbour_sets(oracle_mod, p, 6)  # n == k: nothing to choose
    assert not amb.any()


def test_model_agrees_with_a_direct_loop():
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(40, 3)).astype(np.float32)
    nbr = np.stack([rng.permutation(40)[:7] for _ in range(40)])
    full, absw = cm.model_covariances(pts, nbr, cm.REGS["NONE"])
    for i in (0, 17, 39):
        x = pts[nbr[i]].astype(np.float64)
        x = x - x.mean(axis=0)
        assert np.abs(full[i, :3, :3] - x.T @ x / 7).max() < 1e-15
        assert np.abs(absw[i] - np.sort(np.abs(np.linalg.eigvalsh(x.T @ x / 7)))).max() < 1e-15
    plane, _ = cm.model_covariances(pts, nbr, cm.REGS["PLANE"])
    w = np.linalg.eigvalsh(plane[:, :3, :3])
    assert np.abs(w - [1e-3, 1, 1]).max() < 1e-14
    zero, absw = cm.model_covariances(pts, np.repeat(np.arange(40)[:, None], 5, axis=1), cm.REGS["NORMALIZED_MIN_EIG"])  # rank 0
    assert np.all(absw == 0) and np.array_equal(zero[:, :3, :3], np.broadcast_to(1e-3 * np.eye(3), (40, 3, 3)))


@pytest.mark.parametrize("name,k", cm.cases())
def test_caps_hold_on_the_reference(oracle_mod, name, k):
    """The GPU test leaves out ambiguous rows and, under PLANE, rows without a separated smallest eigenvalue.  Both shares are
    capped here, on the reference alone, so a family cannot quietly stop testing anything."""
    _, ambiguous, _, absw = cm.reference(name, k)
    skipped = (~cm.plane_separated(absw))[~ambiguous]
    print(f"{name} k={k}: n={len(ambiguous)} ambiguous={ambiguous.mean():.4f} plane_skipped={skipped.mean() if len(skipped) else 0.0:.4f}")
    assert ambiguous.mean() <= cm.AMBIGUOUS_CAP
    if _skip_cap_applies(name, k):
        assert skipped.mean() <= cm.PLANE_SKIP_CAP
    elif name in cm.RANK2_FROM_K and k >= 3 and cm.RANK2_FROM_K[name] is None:
        assert skipped.all()  # a family of rank <= 1 is judged by the PLANE properties on every row


@pytest.mark.parametrize("reg", list(cm.REGS))
@pytest.mark.parametrize("name,k", cm.cases())
def test_oracle_matches_model(oracle_mod, name, k, reg):
    """orc.covariances against model_covariances at 1e-9 on the well-defined rows, the PLANE properties on the oracle's own output
    elsewhere: the judgement (`check_case`) is proven on the CPU before it judges the kernel."""
    r = cm.REGS[reg]
    nbr, _, _, _ = cm.reference(name, k)
    model, _ = cm.model_covariances(cm.families()[name], nbr, r)
    fig = cm.check_case(cm.oracle_covariances(name, k, r), model, name, k, r, sym_tol=ORACLE_SYM_TOL)
    print(f"{name} k={k} {reg}: {fig}")
    assert fig["max_diff"] < 0.5 * cm.TOL  # a family closer than a factor of 2 to the tolerance must shrink its extent


def test_k_larger_than_the_cloud_is_an_error(oracle_mod):
    with pytest.raises(RuntimeError):
        oracle_mod.covariances(cm.families()["tiny_n10"], 11, 3)


def _table():
    from oracle import oracle as orc
    orc.build(ref=False)
    worst = {reg: (0.0, None) for reg in cm.REGS}
    shares = {}
    for name, k in cm.cases():
        nbr, ambiguous, _, absw = cm.reference(name, k)
        skipped = (~cm.plane_separated(absw))[~ambiguous]
        fam = "tiny" if name.startswith("tiny") else name
        a, s = shares.get(fam, (0.0, 0.0))
        shares[fam] = (max(a, float(ambiguous.mean())), max(s, float(skipped.mean()) if _skip_cap_applies(name, k) and len(skipped) else 0.0))
        for reg, r in cm.REGS.items():
            model, _ = cm.model_covariances(cm.families()[name], nbr, r)
            fig = cm.check_case(cm.oracle_covariances(name, k, r), model, name, k, r, sym_tol=ORACLE_SYM_TOL)
            if fig["max_diff"] > worst[reg][0]:
                worst[reg] = (fig["max_diff"], f"{name}, k = {k}")
    for reg, (v, where) in worst.items():
        print(f"  {reg:<19} max |oracle - model| = {v:.2e}  ({where})")
    for fam, (a, s) in shares.items():
        print(f"  {fam:<13} ambiguous rows <= {100 * a:.2f} %   PLANE rows without a separated normal (where capped) <= {100 * s:.2f} %")


if __name__ == "__main__":
    _table()

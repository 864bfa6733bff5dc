"""Generate tests/golden/ref_kdtree.npz.   Run where the reference is present:  python tests/golden/make_ref_kdtree.py

The REAL reference kd-tree (the reference's vendored nanoflann, compiled by oracle/Makefile into oracle/_ref/; the reference
source is never copied) queried on the inputs of tests/test_oracle_cpu.py's kd-tree cases:
  * n<N>_k<K>_{pts,q,idx,d2}  — seeded normal clouds of N points, queries inside and far outside, K neighbours
  * ties_{pts,q,idx,d2}       — a lattice with duplicates: many exactly equal distances, traversal order decides
Inputs and outputs are stored, so that the tests need neither the reference nor oracle/_ref.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import oracle as orc  # noqa: E402

CASES = [(1, 1), (7, 3), (101, 20), (100, 20), (5000, 1), (5000, 20), (20000, 32)]


def live_case(n: int, k: int):
    rng = np.random.default_rng(n * 31 + k)
    pts = (rng.normal(size=(n, 3)) * [10, 8, 1.5]).astype(np.float32)
    q = np.concatenate([pts[: min(n, 200)], (rng.normal(size=(200, 3)) * 30).astype(np.float32)])  # inside + far outside
    return pts, q, min(k, n)


def ties_case():
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(6), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    pts = np.concatenate([g, g[:100]])  # lattice (many equal distances) + duplicates
    q = g[::7] + np.float32(0.5)
    return pts, q, 8


def main():
    orc.build(ref=True)
    assert orc.ref_available(), "needs the reference to build oracle/_ref"
    arrays = {}
    for key, (pts, q, k) in [(f"n{n}_k{k}", live_case(n, k)) for n, k in CASES] + [("ties", ties_case())]:
        idx, d2 = orc.RefTree(pts).knn(q, k)
        arrays.update({f"{key}_pts": pts, f"{key}_q": q, f"{key}_idx": idx, f"{key}_d2": d2})
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_kdtree.npz")
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

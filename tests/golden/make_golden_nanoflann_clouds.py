"""Regenerates tests/golden/golden_nanoflann_clouds.npz: what the REFERENCE's k-d tree (src/util/nanoflann.h behind oracle/ref_nanoflann.cpp, built by
`make -C oracle` into oracle/_ref/libref_nanoflann.so) answers on the point clouds of tests/test_initializer_cpu.py's two k-d tree tests. Inputs (the seeded
clouds and queries) and expected outputs (indices incl. the order of equidistant neighbours, fp32 squared distances) are stored; no reference text is.
With the fixture those tests pin the oracle's restatement wherever they run, with or without the reference; where the library is built they also check
that it still answers what the fixture holds.
Needs the reference (oracle/Makefile, REF). Run:  python tests/golden/make_golden_nanoflann_clouds.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc  # noqa: E402

OUT = os.path.join(HERE, "golden_nanoflann_clouds.npz")
GRID_CASES = [(80, 60, 0.3), (306, 92, 0.05), (40, 30, 1.0), (13, 11, 0.5), (612, 184, 0.03)]
RANDOM_K = (1, 7, 10)


def grid_key(W, H, dens):
    return "grid_%d_%d_%g" % (W, H, dens)


def _grid_cloud(rng, W, H, dens):
    ys, xs = np.nonzero(rng.rand(H, W) < dens)
    return (xs + 0.1).astype(np.float32), (ys + 0.1).astype(np.float32)


def grid_inputs(W, H, dens):
    """grid points + 0.1 (most 10-NN sets end in a tie) and the parent query of makeNN: (u/2 - 0.25, v/2 - 0.25) in a coarser cloud"""
    rng = np.random.RandomState(W * 7 + H)
    u, v = _grid_cloud(rng, W, H, dens)
    u2, v2 = _grid_cloud(rng, W // 2, H // 2, min(1.0, dens * 2))
    qu, qv = u * np.float32(0.5) - np.float32(0.25), v * np.float32(0.5) - np.float32(0.25)
    return u, v, u2, v2, qu, qv


def random_inputs():
    rng = np.random.RandomState(5)
    u, v = (rng.rand(5000) * 100).astype(np.float32), (rng.rand(5000) * 50).astype(np.float32)
    qu, qv = (rng.rand(3000) * 140 - 20).astype(np.float32), (rng.rand(3000) * 90 - 20).astype(np.float32)
    return u, v, qu, qv


def idx16(idx):
    """indices as int16 (every cloud holds fewer than 32768 points)"""
    assert idx.min() >= 0 and idx.max() < 32768
    return idx.astype(np.int16)


def main():
    assert orc.ref_nanoflann() is not None, "oracle/_ref/libref_nanoflann.so missing: make -C oracle (needs the reference, oracle/Makefile REF)"
    out = {}
    for W, H, dens in GRID_CASES:
        g = grid_key(W, H, dens)
        u, v, u2, v2, qu, qv = grid_inputs(W, H, dens)
        out[g + "_u"], out[g + "_v"], out[g + "_u2"], out[g + "_v2"] = u, v, u2, v2
        idx, out[g + "_nn_dist"] = orc.ref_nanoflann_knn(u, v, u, v, 10)
        out[g + "_nn_idx"] = idx16(idx)
        out[g + "_nn11_dist_9_10"] = orc.ref_nanoflann_knn(u, v, u, v, 11)[1][:, 9:11]     # the tie test reads the 10th and 11th distances only
        idx, out[g + "_parent_dist"] = orc.ref_nanoflann_knn(u2, v2, qu, qv, 1)
        out[g + "_parent_idx"] = idx16(idx)
    u, v, qu, qv = random_inputs()
    out["random_u"], out["random_v"], out["random_qu"], out["random_qv"] = u, v, qu, qv
    # one stored answer: the reference's k = 1 and k = 7 lists are the first columns of its k = 10 list (checked here)
    idx, dist = orc.ref_nanoflann_knn(u, v, qu, qv, max(RANDOM_K))
    for k in RANDOM_K:
        i_k, d_k = orc.ref_nanoflann_knn(u, v, qu, qv, k)
        assert np.array_equal(i_k, idx[:, :k]) and np.array_equal(d_k, dist[:, :k]), k
    out["random_idx"], out["random_dist"] = idx16(idx), dist
    np.savez_compressed(OUT, **out)
    print("%s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()

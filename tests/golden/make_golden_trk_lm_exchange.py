"""Regenerates tests/golden/golden_trk_lm_exchange.npz: what trk_lm_kernel computes on the clouds of tests/test_trk_lm_exchange_gpu.py (T, aff, lastResiduals,
the flow indicators, ok and the evaluations per level of one track per cloud), as "<level-0 points>_<name>" arrays.

The fixture pins the kernel's outputs as they were BEFORE the exchange loop's loads were batched, so it is only regenerated with a library built from a
commit whose exchange is known good (the committed file: the parent of the commit that added the test). Needs an MI355X and the built library. Run:
    python tests/golden/make_golden_trk_lm_exchange.py [OUT.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT):
    sys.path.insert(0, p)
import nalo_pkg  # noqa: E402

nalo_pkg.load()
import test_trk_lm_exchange_gpu as t  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    s = t.scene()
    out = {}
    for n0 in t.CLOUDS:
        g = s.track(n0)
        t.check_grid(s, n0, g)
        again = s.track(n0)
        for key in t.KEYS:
            out["%d_%s" % (n0, key)] = np.asarray(g[key])
            assert np.array_equal(out["%d_%s" % (n0, key)], np.asarray(again[key]), equal_nan=True), (n0, key)
        print("n0 = %d: workgroups %d, evals %s, ok %d" % (n0, g["cfg"]["nblocks"], list(g["ev"]), g["ok"]))
    s.ctx.close()
    np.savez_compressed(out_path, **out)
    print("%s: %d arrays, %d bytes" % (out_path, len(out), os.path.getsize(out_path)))


if __name__ == "__main__":
    main()

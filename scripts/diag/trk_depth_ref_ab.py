"""nalo_trk_set_ref_from_depth at the KITTI shape: the volume of tests/test_tsdf_gpu.py's chain (1224x368, W = 8, three keyframes fused into 256x64x256 voxels)
ray-cast from the last keyframe's pose into a 1224x368 depth image that stays on the device, and the tracking reference built from it. One process, the legs
alternating inside every repetition, for step = 1 and step = 4:

  (a) from_depth   nalo_trk_set_ref_from_depth on the ray-cast's view: one call, nothing crosses to the host but pc_n and n_seeded
  (b) round trip   what a caller does without it: download the depth image (1.8 MB), form the four arrays on the host (tests/trk_depth_ref_model.py's
                   vectorised numpy), nalo_trk_set_ref (pinned staging and one H2D copy of up to 7.2 MB); its three parts are also timed one by one

Both end on the same host poll for pc_n, so the wall clock of a call is the whole cost. The two references are compared once per step before anything is timed.

    timeout -k 10 600 python scripts/diag/trk_depth_ref_ab.py --log profiles/trk_depth_ref_ab.log

Prints a table and one JSON line; --log appends both to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests"))
from tsdf_ab import F, stats  # noqa: E402  (loads the package)
from tsdf_raycast_time import chain_context  # noqa: E402

import torch  # noqa: E402
import trk_depth_ref_model as dm  # noqa: E402

HDI = 1e-4


def reference(c):
    return [c.trk_get_pc(l) + list(c.trk_get_depth(l)) for l in range(c.levels)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    c, made, T, K, mn, mx = chain_context()
    w, h = c.w, c.h
    assert (w, h) == (1224, 368)
    st = (mx - mn) / 250.0
    cnt = c.tsdf_raycast(w, h, K, T, mn, mx, st, 1.0, download=False)
    view = c.tsdf_raycast_view()["depth"]
    t = torch.as_tensor(view, device="cuda")
    assert t.data_ptr() == view.ptr
    slot = 0
    c.frame_upload(slot, np.random.RandomState(0).uniform(5, 250, (h, w)).astype(F))
    out = {"part": "trk_depth_ref", "shape": [w, h], "levels": c.levels, "n_hit": cnt["n_hit"], "steps": {}}
    lines = ["trk_set_ref_from_depth %dx%d, %d levels, ray-cast of the chain's volume: %d of %d pixels hit" % (w, h, c.levels, cnt["n_hit"], w * h)]
    for step in (1, 4):
        # once, untimed: the same reference both ways
        n = c.trk_set_ref_from_depth(slot, view, mn, mx, HDI, step)
        got = reference(c)
        lists = dm.inputs(t.cpu().numpy(), None, mn, mx, HDI, step)
        c.trk_set_ref(slot, *lists)
        want = reference(c)
        assert n == len(lists[0]) and all(x.tobytes() == y.tobytes() for g, v in zip(got, want) for x, y in zip(g, v)), "the two routes disagree"
        legs = {k: [] for k in ("from_depth", "round_trip", "download", "numpy_list", "set_ref")}
        for k in range(a.warmup + a.reps):
            c.sync()
            t0 = time.perf_counter()
            c.trk_set_ref_from_depth(slot, view, mn, mx, HDI, step)
            t1 = time.perf_counter()
            depth = t.cpu().numpy()
            t2 = time.perf_counter()
            lists = dm.inputs(depth, None, mn, mx, HDI, step)
            t3 = time.perf_counter()
            c.trk_set_ref(slot, *lists)
            t4 = time.perf_counter()
            if k >= a.warmup:
                for name, dt in (("from_depth", t1 - t0), ("round_trip", t4 - t1), ("download", t2 - t1), ("numpy_list", t3 - t2), ("set_ref", t4 - t3)):
                    legs[name].append(dt * 1e6)
        s = {name: stats(v) for name, v in legs.items()}
        out["steps"][str(step)] = dict(n_seeded=n, pc_n=[len(g[0]) for g in got], **s)
        lines.append("  step %d: %d pixels seeded, pc_n %s" % (step, n, [len(g[0]) for g in got]))
        lines.append("    (a) from_depth  median %8.1f us (p95 %8.1f)" % (s["from_depth"]["median"], s["from_depth"]["p95"]))
        lines.append("    (b) round trip  median %8.1f us (p95 %8.1f) = download %.1f + numpy list %.1f + nalo_trk_set_ref %.1f (medians)" % (
            s["round_trip"]["median"], s["round_trip"]["p95"], s["download"]["median"], s["numpy_list"]["median"], s["set_ref"]["median"]))
    lines.append(json.dumps(out))
    print("\n".join(lines))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")
    c.close()


if __name__ == "__main__":
    main()

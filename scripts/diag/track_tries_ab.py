"""nalo_trk_track_tries against the loop over nalo_trk_track it replaces, at 1224x368 on the headline cloud (bench.py's kitti00_8kf inputs: 8750 residuals,
64 workgroups, two rounds on levels 0 and 1), one process, the legs alternating per repeat, wall clock of call + drain:

  (i)   n_tries = 1 against one nalo_trk_track: what the outer level costs a caller that never needs it
  (ii)  the reference's 31 hypotheses with lastCoarseRMSE[0] = 1e-6 (all 31 run) against the literal loop of 31 nalo_trk_track calls driven from Python with
        the same take-over rule (tests/track_tries_model.py) - and against the same loop with the Python model's bookkeeping stripped to the bare calls

Reports median and p95 per leg, the evaluations per try, and checks that both forms of (ii) give the same bits. Prints a table and one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import nalo_pkg  # noqa: E402

nalo_pkg.load()
import bench  # noqa: E402
import track_tries_model as model  # noqa: E402
from nalo_slam_amd import binding, synth  # noqa: E402


def stats(us):
    us = np.asarray(us, np.float64)
    return {"median": float(np.median(us)), "p95": float(np.percentile(us, 95)), "n": int(us.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    win, _, trk = bench.make_inputs("kitti00_8kf")
    W = win.W
    c = binding.Context(win.w, win.h, win.K, n_slots=2)
    c.frame_upload(0, win.images[W - 1]); c.frame_upload(1, win.images[W])
    c.trk_set_ref(0, *trk)
    top = c.levels - 1
    Ttrue = synth.se3_mul(win.world_to_cam[W], synth.se3_inv(win.world_to_cam[W - 1]))
    T0 = model.se3_exp(model.se3_log(Ttrue) * 0.95)
    tries = binding.trk_motion_tries(model.se3_inv(T0), np.hstack([np.eye(3), np.zeros((3, 1))]))
    aff, ref_aff, exp_ = (0.0, 0.0), (0.0, 0.0), (1.0, 1.0)
    nan5 = np.full(5, np.nan)

    def track(T, aff0, min_res):
        return c.trk_track(1, T, aff0, ref_aff, exp_, top, min_res=min_res)

    def one_track():
        return c.trk_track(1, T0, aff, ref_aff, exp_, top, min_res=nan5)

    def one_try():
        return c.trk_track_tries(1, tries[:1], aff, ref_aff, exp_, top, 1e-6)

    def all_tries():
        return c.trk_track_tries(1, tries, aff, ref_aff, exp_, top, 1e-6)

    def loop_model():
        return model.track_new_coarse(track, tries, aff, 1e-6)

    bounds = []

    def loop_bare():                                                 # the 31 calls with the bounds the model loop passed them, no bookkeeping in between
        for T, b in zip(tries, bounds):
            c.trk_track(1, T, aff, ref_aff, exp_, top, min_res=b)

    one, loop = all_tries(), loop_model()
    cfg = c.trk_launch_config()
    same = one["try_iterations"] == loop["try_iterations"] == len(tries) and one["winner"] == loop["winner"] and \
        all(np.array_equal(one[k], loop[k], equal_nan=True) for k in ("T", "aff", "flow", "achievedRes")) and \
        all(np.array_equal(q["lastResiduals"], r["lastResiduals"], equal_nan=True) and np.array_equal(q["T"].reshape(3, 4), r["T"]) and q["ok"] == r["ok"]
            for q, r in zip(one["records"], loop["records"]))
    ach = np.full(5, np.nan)
    have = False
    for r in loop["records"]:                                        # replay achievedRes to get each call's bound
        bounds.append(ach.copy())
        have = have or bool(r["taken"])
        if have:
            for l in range(5):
                if not model.finite_as_float(ach[l]) or ach[l] > r["lastResiduals"][l]:
                    ach[l] = r["lastResiduals"][l]
    legs = {"i_trk_track": one_track, "i_tries_1": one_try, "ii_tries_31": all_tries, "ii_loop_31_model": loop_model, "ii_loop_31_bare": loop_bare}
    wall = {k: [] for k in legs}
    for rep in range(a.warmup + a.reps):
        for name, leg in legs.items():
            c.sync()
            t0 = time.perf_counter()
            leg()
            c.sync()
            if rep >= a.warmup:
                wall[name].append((time.perf_counter() - t0) * 1e6)
    res = {k: stats(v) for k, v in wall.items()}
    ev = [int(q["n_evals"]) for q in one["records"]]
    out = {"shape": "%dx%d" % (win.w, win.h), "inputs": int(len(trk[0])), "pc_n": [int(x) for x in c.trk_last_evals()[1][:c.levels]], "workgroups": cfg["nblocks"], "rounds": cfg["rounds"],
           "driver": one["driver"], "same_bits_one_call_vs_loop": bool(same), "tries": len(tries), "winner": one["winner"], "evals_per_try": ev, "evals_total": int(sum(ev)),
           "abort_lvl_per_try": [int(q["abort_lvl"]) for q in one["records"]], "wall_us": res}
    print("%s, %d inputs, levels %s, %d workgroups, rounds %s, driver %d; one call and loop give the same bits: %s" %
          (out["shape"], out["inputs"], out["pc_n"], out["workgroups"], out["rounds"], out["driver"], same))
    print("evaluations per try (31 tries, winner %d): %s = %d" % (one["winner"], ev, sum(ev)))
    for k, v in res.items():
        print("  %-20s median %9.1f us  p95 %9.1f us  (n=%d)" % (k, v["median"], v["p95"], v["n"]))
    d = res["i_tries_1"]["median"] - res["i_trk_track"]["median"]
    print("(i)  one try costs %+.1f us over nalo_trk_track; that leg's p95 - median spread is %.1f us" % (d, res["i_trk_track"]["p95"] - res["i_trk_track"]["median"]))
    print("(ii) 31 tries: one call %.1f us, the loop of 31 calls %.1f us (bare calls %.1f us): x%.2f / x%.2f" %
          (res["ii_tries_31"]["median"], res["ii_loop_31_model"]["median"], res["ii_loop_31_bare"]["median"],
           res["ii_loop_31_model"]["median"] / res["ii_tries_31"]["median"], res["ii_loop_31_bare"]["median"] / res["ii_tries_31"]["median"]))
    print(json.dumps(out))
    c.close()


if __name__ == "__main__":
    main()

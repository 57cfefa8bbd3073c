"""The window panel of one keyframe (FullSystem::debugPlot -> displayImageStitch), two ways in one process, the legs alternating per call: wall time from the
first call to the result on the host

  device    nalo_map_window_plot(mode 1): scatter and resolve on the device, 3 B/px per window frame (+ 0.5 KB of counters) up behind one wait
  readback  the route a caller of the device chain has without it: nalo_frame_download(slot, 0) of the W window frames (16 B/px of {I, dx, dy, 0} on the bus; the
            binding also fetches absSquaredGrad), nalo_ba_get_points and nalo_map_get_frame of the W frames ...
  hostpaint ... + the base image and the rings, here as tests/window_plot_model.py's vectorised NumPy `fast` (a stand-in for the caller's C++ loops, which were
            NOT measured; reported apart from the transfers)

at 1224x368 and at 1920x1072 with W = 8 and about 2000 points, after one keyframe of the chain (nalo_ba_flag_points -> nalo_ba_marginalize_flagged, the archive on),
untimed, the stream drained before each leg. The script checks that both routes give the same bytes. A second pass of the device leg runs with the library's
profile brackets on and prints the scopes window_plot_scatter / window_plot_resolve (device events around each launch); wall times are taken with them off."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import nalo_pkg  # noqa: E402

nalo_pkg.load()
import lifecycle_model as lm  # noqa: E402
import lifecycle_scenes as sc  # noqa: E402
import window_plot_model as model  # noqa: E402
from nalo_slam_amd import binding, synth  # noqa: E402


def stats(name, a):
    a = np.asarray(a)
    print("  %-22s median %9.1f us   p95 %9.1f   (n = %d)" % (name, np.median(a), np.percentile(a, 95), len(a)), flush=True)
    return float(np.median(a))


def one_shape(w, h, calls):
    W, P = 8, 2000
    s = 3e-4
    win = synth.make_window(w=w, h=h, W=W, P=P, seed=sc.SEED, n_extra=0, step_z=0.8 * s, step_x=0.03 * s, full_graph=False)
    c = binding.Context(w, h, win.K, n_slots=W)
    for i in range(W):
        c.frame_upload(i, win.images[i])
    fids = [300 + i for i in range(W)]
    c.ba_set_window(list(range(W)), win.world_to_cam[:W], state6=synth.perturbed_poses(win, sigma_t=0.004, sigma_r=0.0004)[:W], frame_ids=fids)
    c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
    c.ba_set_residuals(win.exists)
    c.map_enable()
    c.ba_set_point_history(*sc.plant_history(len(win.host), W))
    c.ba_linearize(False)
    c.ba_linearize(True)
    dec, _, _ = c.ba_flag_points(sc.flag_sets(W)[1])
    c.ba_marginalize_flagged()
    valid = dec == lm.KEEP
    box = {}

    def device():
        box["dev"] = c.map_window_plot(1)

    def readback():
        idepth = c.ba_get_points()["idepth"]
        frames = []
        for i in range(W):
            rec = c.map_get_frame(fids[i])
            sel = valid & (win.host == i)
            f = dict(I=c.frame_download(i, 0)[0][:, 0], active=dict(u=win.u[sel], v=win.v[sel], idepth=idepth[sel]))
            for name, st in (("marg", 2), ("out", 3)):
                r = rec[rec["status"] == st]
                f[name] = dict(u=r["u"], v=r["v"], idepth=r["idepth"])
            frames.append(f)
        box["frames"] = frames

    legs = ["device", "readback", "hostpaint"]
    ts = {k: [] for k in legs}
    same = True
    for i in range(calls + 1):                                                 # call 0 is the warm-up (first-use allocations), not timed
        c.sync()
        t = {}
        for k in (("device", "readback") if i % 2 == 0 else ("readback", "device")):
            t0 = time.perf_counter()
            (device() if k == "device" else readback())
            t[k] = time.perf_counter() - t0
        if i % 10 == 0:                                                        # the NumPy stand-in is slow: every tenth call
            t0 = time.perf_counter(); mod = model.fast(box["frames"], w, h, 1); t["hostpaint"] = time.perf_counter() - t0
            same = same and np.array_equal(box["dev"]["bgr"], mod["bgr"]) and np.array_equal(box["dev"]["sources"], mod["sources"])
        if i > 0:
            for k in t:
                ts[k].append(t[k] * 1e6)
    n_src = int(box["dev"]["sources"].sum())
    n_rec = sum(len(c.map_get_frame(f)) for f in fids)
    print("window_plot_ab: %d x %d, W = %d, %d rings (%d valid points, %d archive records), %d calls per leg; both routes give the same bytes: %s" %
          (w, h, W, n_src, int(valid.sum()), n_rec, calls, same))
    print("  bytes up, device route:    %d (images) + 512 (counters)" % (3 * w * h * W))
    print("  bytes up, read-back route: %d (frames: {I, dx, dy, 0} + absSquaredGrad) + %d (points: 11 floats each) + %d (archive records)" %
          (20 * w * h * W, 44 * len(win.host), 64 * n_rec))
    print("  bytes down: a segment table of a few hundred bytes (device route), none (read-back route)")
    med = {k: stats(k, ts[k]) for k in legs}
    print("  read-back route, total  = readback + hostpaint (NumPy): %9.1f us" % (med["readback"] + med["hostpaint"]))
    c.profile_enable(True)
    c.profile_reset()
    for i in range(calls):
        c.map_window_plot(1)
    c.sync()
    for name in ("window_plot_scatter", "window_plot_resolve"):
        stats(name, c.profile_samples(name))
    c.profile_enable(False)
    c.close()
    return same


ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=120)
ap.add_argument("--shapes", default="1224x368,1920x1072", help="comma-separated WxH")
args = ap.parse_args()
ok = True
for shape in args.shapes.split(","):
    w, h = [int(v) for v in shape.split("x")]
    ok = one_shape(w, h, args.calls) and ok
sys.exit(0 if ok else 1)

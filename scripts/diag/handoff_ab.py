"""The hand-offs between a mapping and a tracking context, each against the route that exists without them, in one process, the legs alternating per repeat:

  (a) reference   nalo_trk_ref_export + nalo_trk_ref_import + a drain, against the host route: nalo_trk_get_pc + nalo_trk_get_depth per level, then
                  nalo_trk_set_pc + nalo_trk_set_depth (every one a blocking copy), at 1224x368 and 1920x1072
  (b) kernel      handoff_copy_kernel alone (the scope trk_ref_import, dispatch-attached timestamps), and its moved bytes (read + written) over the copy rate
                  nalo_hbm_calibrate reports in the same run
  (c) frame       nalo_frame_plane + nalo_frame_ingest_device (level 0 copied as words, the pyramid rebuilt) + a drain, against nalo_frame_download(0) +
                  nalo_frame_upload
  (d) threaded    keyframes per second of the keyframe loop on two threads (a mapper and a tracker context, the swap between two barriers) and on one thread.
                  Per keyframe the mapper restores the window, optimises, builds the reference from it and exports; the tracker tracks three frames against the
                  reference of the keyframe before, hands each to the mapper through its plane, then imports and releases. The window is restored from a snapshot
                  every keyframe (as bench.py's pipelined leg does): without point activation a carried window runs out of points within a few keyframes.

Prints a table and one JSON line per part. The script checks that both routes of (a) and (c) leave the same bits."""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import nalo_pkg  # noqa: E402

nalo_pkg.load()
from nalo_slam_amd import binding, synth  # noqa: E402

TRACKED_PER_KF = 3
WAIT = 120.0


def stats(us):
    us = np.asarray(us, np.float64)
    return {"median": float(np.median(us)), "p95": float(np.percentile(us, 95)), "n": int(us.size)}


def ref_inputs(win, n, seed=1):
    rng = np.random.RandomState(seed)
    Ku, Kv = rng.uniform(5, win.w - 6, n).astype(np.float32), rng.uniform(5, win.h - 6, n).astype(np.float32)
    d = win.depth[win.W - 1][(Kv + 0.5).astype(int), (Ku + 0.5).astype(int)]
    ok = np.isfinite(d)
    return Ku[ok], Kv[ok], (1.0 / d[ok]).astype(np.float32), (10.0 ** rng.uniform(-6, -3, int(ok.sum()))).astype(np.float32)


def same_ref(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for l in range(a.levels) for x, y in zip(a.trk_get_pc(l) + list(a.trk_get_depth(l)), b.trk_get_pc(l) + list(b.trk_get_depth(l))))


def timed(legs, reps, drain):
    wall = {k: [] for k in legs}
    for _ in range(reps):
        for name, leg in legs.items():
            drain()
            t0 = time.perf_counter()
            leg()
            drain()
            wall[name].append((time.perf_counter() - t0) * 1e6)
    return {k: stats(v) for k, v in wall.items()}


def hand_offs(w, h, reps, copy_GBs):
    win = synth.make_window(w=w, h=h, W=2, P=200, seed=7, n_extra=0)
    A, B = [binding.Context(w, h, win.K, n_slots=2) for _ in range(2)]
    for c in (A, B):
        c.frame_upload(0, win.images[1]); c.frame_upload(1, win.images[0])
    A.trk_set_ref(0, *ref_inputs(win, 8 * 2000))
    L = A.levels

    def host_route():
        for l in range(L):
            pc, dm = A.trk_get_pc(l), A.trk_get_depth(l)
            B.trk_set_pc(0, l, *pc)
            B.trk_set_depth(0, l, *dm)

    def device_route():
        B.trk_ref_import(0, A.trk_ref_export()["view"])
        B.trk_ref_release(A.stream)

    def drain():
        A.sync(); B.sync()
    for _ in range(5):
        host_route(); device_route()
    drain()
    ok_ref = same_ref(A, B)
    e = A.trk_ref_export()
    moved = 2 * 4 * sum(4 * e["n"][l] + 2 * (w >> l) * (h >> l) for l in range(L))          # read + written
    res = {"shape": "%dx%d" % (w, h), "levels": L, "pc_n": e["n"], "same_reference": bool(ok_ref), "kernel_bytes_read_and_written": moved}
    res["a_reference_wall_us"] = timed({"host_route": host_route, "import": device_route}, reps, drain)
    B.profile_enable(True); B.profile_reset()
    for _ in range(reps):
        device_route(); drain()
    res["b_kernel_us"] = stats(B.profile_samples("trk_ref_import"))
    B.profile_enable(False)
    res["b_bytes_over_copy_rate_us"] = moved / (copy_GBs * 1e3)

    def frame_host():
        B.frame_upload(1, A.frame_download(1, 0)[0][:, 0].reshape(h, w))

    def frame_device():
        B.frame_ingest(1, image=A.frame_plane(1, "irradiance"))
    for _ in range(5):
        frame_host(); frame_device()
    drain()
    res["same_frame"] = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for l in range(L) for x, y in zip(A.frame_download(1, l), B.frame_download(1, l)))
    res["c_frame_wall_us"] = timed({"download_upload": frame_host, "planes": frame_device}, reps, drain)
    A.close(); B.close()
    return res


class Loop:
    """(d): one mapper and one tracker context; the four bodies of a keyframe"""

    def __init__(self, win, st6):
        W = win.W
        self.win, self.W = win, W
        self.M = binding.Context(win.w, win.h, win.K, n_slots=W + TRACKED_PER_KF)
        self.T = binding.Context(win.w, win.h, win.K, n_slots=1 + TRACKED_PER_KF)
        M, T = self.M, self.T
        for i in range(W + TRACKED_PER_KF):
            M.frame_upload(i, win.images[i])
        M.ba_set_window(list(range(W)), win.world_to_cam[:W], state6=st6)
        M.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
        M.ba_set_residuals(win.exists)
        M.ba_snapshot()
        T.frame_upload(0, win.images[W - 1])
        for k in range(TRACKED_PER_KF):
            T.frame_upload(1 + k, win.images[W + k])
        self.T0 = [synth.se3_mul(win.world_to_cam[W + k], synth.se3_inv(win.world_to_cam[W - 1])) for k in range(TRACKED_PER_KF)]
        self.view, self.planes = None, []
        self.map_keyframe(); self.swap(); self.M.sync(); self.T.sync()      # the first reference

    def map_keyframe(self):
        M = self.M
        M.ba_restore()
        M.ba_optimize(3, never_break=True)
        M.trk_set_ref_from_window()
        self.view = M.trk_ref_export()["view"]

    def track(self):
        T = self.T
        self.planes = []
        for k in range(TRACKED_PER_KF):
            T.frame_rebuild(1 + k)
            T.trk_track(1 + k, self.T0[k], [0, 0], [0, 0], [1, 1], T.levels - 1)
            self.planes.append(T.frame_plane(1 + k, "irradiance"))

    def swap(self):                                                          # the tracker's side of the swap: import, then the back edge
        self.T.trk_ref_import(0, self.view)
        self.T.trk_ref_release(self.M.stream)

    def take_frames(self):                                                   # the mapper's side of deliverTrackedFrame
        for k, p in enumerate(self.planes):
            self.M.frame_ingest(self.W + k, image=p)

    def close(self):
        self.M.sync(); self.T.sync()
        self.T.close(); self.M.close()


def keyframe_loop(win, st6, steps, warmup, threaded):
    lp = Loop(win, st6)
    err, t = [], {}
    n_total = warmup + steps
    if not threaded:
        for s in range(n_total):
            if s == warmup:
                lp.M.sync(); lp.T.sync(); t["t0"] = time.perf_counter()
            lp.track(); lp.map_keyframe(); lp.swap(); lp.take_frames()
    else:
        bar = threading.Barrier(2, timeout=WAIT)

        def body(first, second):
            try:
                for s in range(n_total):
                    if s == warmup:
                        bar.wait()
                        if first == lp.track:
                            t["t0"] = time.perf_counter()
                    first()
                    bar.wait()                                               # the reference of this keyframe stands, the three frames are tracked
                    second()
                    bar.wait()                                               # imported and released; the frames are in the mapper
            except Exception as e:
                err.append(e); bar.abort()
        ths = [threading.Thread(target=body, args=(lp.track, lp.swap)), threading.Thread(target=body, args=(lp.map_keyframe, lp.take_frames))]
        [x.start() for x in ths]
        [x.join(WAIT + 600) for x in ths]
        if any(x.is_alive() for x in ths):
            raise RuntimeError("a thread of the keyframe loop did not finish")
    lp.M.sync(); lp.T.sync()
    dt = time.perf_counter() - t["t0"]
    driver = lp.T.trk_launch_config()["driver"]
    lp.close()
    if err:
        raise err[0]
    return {"keyframes_per_s": steps / dt, "keyframes": steps, "tracker_driver_at_the_end": driver}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--keyframes", type=int, default=200)
    a = ap.parse_args()
    c = binding.Context(64, 64, (50.0, 50.0, 31.5, 31.5), n_slots=1)
    copy_GBs, triad_GBs = c.hbm_calibrate()
    c.close()
    print("nalo_hbm_calibrate: copy %.0f GB/s, triad %.0f GB/s" % (copy_GBs, triad_GBs))
    for w, h in ((1224, 368), (1920, 1072)):
        r = hand_offs(w, h, a.reps, copy_GBs)
        print("%s  levels %d  pc_n %s  same reference: %s  same frame: %s" % (r["shape"], r["levels"], r["pc_n"], r["same_reference"], r["same_frame"]))
        for part, key in (("(a) reference, call + drain", "a_reference_wall_us"), ("(c) frame, call + drain", "c_frame_wall_us")):
            for k, v in r[key].items():
                print("  %-28s %-16s median %9.1f us  p95 %9.1f us  (n=%d)" % (part, k, v["median"], v["p95"], v["n"]))
        v = r["b_kernel_us"]
        print("  %-28s %-16s median %9.2f us  p95 %9.2f us  (n=%d); %d bytes read + written over the copy rate: %.2f us" %
              ("(b) kernel scope", "trk_ref_import", v["median"], v["p95"], v["n"], r["kernel_bytes_read_and_written"], r["b_bytes_over_copy_rate_us"]))
        print(json.dumps(r))
    s = 3e-4
    win = synth.make_window(w=1224, h=368, W=8, P=2000, seed=7, n_extra=TRACKED_PER_KF, step_z=0.8 * s, step_x=0.03 * s, full_graph=False)
    st6 = synth.perturbed_poses(win, sigma_t=0.004, sigma_r=0.0004)
    d = {}
    for rep in range(2):                                                     # the legs alternate; the second pair is reported beside the first
        for name, th in (("one_thread", False), ("threaded", True)):
            d.setdefault(name, []).append(keyframe_loop(win, st6, a.keyframes, 5, th))
    for name, runs in d.items():
        print("  (d) %-12s %s keyframes/s over %d keyframes (tracker driver at the end: %s)" %
              (name, " / ".join("%.0f" % r["keyframes_per_s"] for r in runs), a.keyframes, [r["tracker_driver_at_the_end"] for r in runs]))
    print(json.dumps({"d_keyframe_loop_1224x368_W8": d}))


if __name__ == "__main__":
    main()

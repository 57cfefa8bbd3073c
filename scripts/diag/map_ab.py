"""The map side of one keyframe, two ways in one process, the legs alternating per keyframe: wall time from the first call to the last result on the host

  plain     nalo_ba_flag_points (decisions resident) + nalo_ba_marginalize_flagged, map off: what the keyframe costs without a map
  archive   the same two calls with nalo_map_enable on: the difference to `plain` is the archive append (count / scan / write, the patch, 128 bytes of counts)
  clouds    the eight nalo_map_frame_cloud calls of publishKeyframes(frameHessians, false), display mode 1, with draws. The thresholds are taken from the data
            (the median of var * depth^4, the upper quartile of var, the lower quartile of maxRelBaseline over the records of statuses 1 and 2): the
            low-parallax scene leaves nothing under the viewer's defaults (0.001, 0.001, 0.1), and a cloud without a vertex is no measurement
  readback  what a caller of the device chain needs for the same map without nalo_map_*: nalo_ba_get_points + nalo_ba_flag_points(decision, idepth_hessian)
            BEFORE the marginalisation, nalo_ba_get_points after it (the re-accumulated Hdd of the marginalised points), nalo_imm_resident_get
  hostloops the caller's loops on those arrays: the push-backs, setFromKF and refreshPC of the eight frames, here as tests/map_model.py's vectorised NumPy
            (a stand-in for the caller's C++ loops, reported apart from the transfers)

on a KITTI-shaped window: 1224x368, W = 8, ~2000 active and ~1500 immature points per frame, the low-parallax scene of tests/lifecycle_scenes.py with two frames
flagged. Every keyframe starts from the same restored window (nalo_ba_restore, the two linearisations and the accumulation, untimed) and an emptied archive
(nalo_map_reset keeps the chunks: steady state). The script checks the device clouds against the model once. The kernels' own times: run this under
rocprofv3 --kernel-trace --stats (rows map_*)."""
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
import map_model as mm  # noqa: E402
from nalo_slam_amd import binding, synth  # noqa: E402

W, P_ACTIVE, N_IMM = 8, 16000, 12000
TH = dict(scaledTH=1e30, absTH=1e30, minRelBS=0.0)                        # replaced by the data's quantiles after the first (untimed) keyframe


def main(keyframes):
    s = sc.SCENES["kitti"]
    win = synth.make_window(w=s["w"], h=s["h"], W=W, P=P_ACTIVE, seed=sc.SEED, n_extra=0, step_z=0.8 * s["scale"], step_x=0.03 * s["scale"], full_graph=False)
    st6 = synth.perturbed_poses(win, sigma_t=0.004, sigma_r=0.0004)
    hp = (win.host == 0).astype(np.int32)
    fids = list(range(100, 100 + W))
    c = binding.Context(win.w, win.h, win.K, n_slots=W)
    for i in range(W):
        c.frame_upload(i, win.images[i])
    c.ba_set_window(list(range(W)), win.world_to_cam[:W], state6=st6, frame_ids=fids)
    c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights, has_prior=hp)
    c.ba_set_residuals(win.exists)
    c.ba_set_point_history(*sc.plant_history(len(win.host), W))
    rng = np.random.RandomState(11)
    f = lambda *sh: rng.rand(*sh).astype(np.float32)
    imm = dict(u=f(N_IMM) * 1000, v=f(N_IMM) * 300, color=f(N_IMM, 8) * 255, host=rng.randint(0, W, N_IMM).astype(np.int32), idmin=f(N_IMM), idmax=1 + f(N_IMM))
    c.imm_resident_set(imm["u"], imm["v"], imm["color"], f(N_IMM, 8), f(N_IMM, 3), f(N_IMM), imm["host"], imm["idmin"], imm["idmax"], np.zeros(N_IMM, np.int32), f(N_IMM))
    c.ba_snapshot()
    ff = sc.flag_sets(W)[2]
    draws = rng.randint(0, 2 ** 31 - 1, 8 * 8000).astype(np.int32)
    ci = mm.calib_inverse(c.ba_get_frames()[2])
    box = {}

    def prep(on):
        c.ba_restore()
        c.ba_linearize(False)
        c.ba_linearize(True)
        c.ba_get_points()
        c.map_reset()
        c.map_enable(on)
        c.sync()

    def removal():
        c.ba_flag_points(ff, outputs=False)
        c.ba_marginalize_flagged()

    def clouds():
        box["clouds"] = [c.map_frame_cloud(fid, 1, draws=draws, **TH) for fid in fids]

    def readback():
        pre = c.ba_get_points()
        dec, H, _ = c.ba_flag_points(ff)
        c.ba_marginalize_flagged()
        post = c.ba_get_points()
        box["rb"] = (pre, dec, H, post, c.imm_resident_get())

    def hostloops():
        pre, dec, H, post, (idmin, idmax, _, _, _, _) = box["rb"]
        exp = mm.flag_points_push(win.host, fids, win.u, win.v, pre["idepth"], win.color, dec, H, pre["maxRelBaseline"], post["Hdd"], post["HdiF"], hp)
        Ha = lm.idepth_hessian(post["Hdd"], post["HdiF"], hp)
        out = []
        for h, fid in enumerate(fids):
            sel = imm["host"] == h
            idx = np.nonzero((win.host == h) & (dec == lm.KEEP))[0]
            act = np.zeros(len(idx), mm.RECORD)
            act["u"], act["v"], act["idepth"], act["color"], act["idepth_hessian"], act["maxRelBaseline"] = win.u[idx], win.v[idx], post["idepth"][idx], win.color[idx], Ha[idx], pre["maxRelBaseline"][idx]
            rec = mm.set_from_kf(dict(u=imm["u"][sel], v=imm["v"][sel], idepth_min=idmin[sel], idepth_max=idmax[sel], color=imm["color"][sel]), act, *exp[fid])
            out.append(mm.refresh_pc(rec, TH["scaledTH"], TH["absTH"], 1, TH["minRelBS"], ci, draws))
        box["model"] = out

    # once, untimed: thresholds from the records, then the two routes publish the same clouds
    prep(False); readback(); hostloops()
    pre, dec, H, post, _ = box["rb"]
    shown = (dec == lm.KEEP) | (dec == lm.MARGINALIZE)
    ok = shown & (pre["idepth"] > 0)
    Hs = np.where(dec == lm.KEEP, lm.idepth_hessian(post["Hdd"], post["HdiF"], hp), mm.add_point_rewrite(H, pre["maxRelBaseline"], post["Hdd"], post["HdiF"], hp)[0])
    var = (1.0 / (Hs[ok].astype(np.float64) + 0.01)).astype(np.float32)
    d4 = (np.float32(1) / pre["idepth"][ok]) ** 4
    TH.update(scaledTH=float(np.median(var * d4)), absTH=float(np.percentile(var, 75)), minRelBS=float(np.percentile(pre["maxRelBaseline"][ok], 25)))
    print("thresholds from the data:", TH)
    prep(True); removal(); clouds()
    dev = box["clouds"]
    prep(False); readback(); hostloops()
    same = all(mm.bits_equal(d["xyz"], m[0]) and np.array_equal(d["rgb"], m[1]) for d, m in zip(dev, box["model"]))
    nrec = sum(int(d["records"].sum()) for d in dev)
    legs = ["plain", "archive", "clouds", "readback", "hostloops"]
    ts = {k: [] for k in legs}
    for i in range(keyframes):
        for j in range(3):
            k = ("plain", "archive", "readback")[(i + j) % 3]
            prep(k == "archive")
            t0 = time.perf_counter()
            (readback if k == "readback" else removal)()
            c.sync()
            ts[k].append(time.perf_counter() - t0)
            if k == "readback":
                t0 = time.perf_counter(); hostloops(); ts["hostloops"].append(time.perf_counter() - t0)
            if k == "archive":
                t0 = time.perf_counter(); clouds(); ts["clouds"].append(time.perf_counter() - t0)
    print("map_ab: W = %d, %d active + %d immature points, %d records and %d vertices over the eight clouds, %d keyframes per leg; device clouds equal the model: %s"
          % (W, len(win.host), N_IMM, nrec, sum(len(d["xyz"]) for d in dev), keyframes, same))
    med = {}
    for k in legs:
        t = np.array(ts[k]) * 1e6
        med[k] = np.median(t)
        print("  %-9s median %9.1f us   p10 %9.1f   p90 %9.1f" % (k, med[k], np.percentile(t, 10), np.percentile(t, 90)), flush=True)
    print("  archive append          = archive - plain        : %9.1f us" % (med["archive"] - med["plain"]))
    print("  device route            = append + clouds        : %9.1f us" % (med["archive"] - med["plain"] + med["clouds"]))
    print("  read-back route, bus    = readback - plain       : %9.1f us" % (med["readback"] - med["plain"]))
    print("  read-back route, total  = bus + hostloops (NumPy): %9.1f us" % (med["readback"] - med["plain"] + med["hostloops"]))
    c.close()
    return same


ap = argparse.ArgumentParser()
ap.add_argument("--keyframes", type=int, default=40)
args = ap.parse_args()
sys.exit(0 if main(args.keyframes) else 1)

"""The initialiser's depth panel (CoarseInitializer::debugPlot -> pushDepthImage) at 1224x368, level 0, two ways in one process: wall time from the call to the
image on the host, every call behind a tracked frame (so the host mirror of the Pnt arrays is stale, as it is in a running initialisation)

  device    nalo_init_depth_image: sum, scatter and resolve on the device, 3 B/px up behind one wait
  readback  the route a caller has without it: nalo_init_get_points (it refreshes the host mirror of every member of every level) ...
  hostpaint ... + the base image and the squares, here as tests/init_plot_model.py's vectorised NumPy `fast` (a stand-in for the caller's C++ loops, which were
            NOT measured; reported apart from the read-back)

28 calls per leg, the median of the last 24. The script checks that both routes give the same bytes."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import nalo_pkg  # noqa: E402

nalo_pkg.load()
import init_plot_model as ip  # noqa: E402
from nalo_slam_amd import binding, synth  # noqa: E402


def main():
    w, h, calls, warm = 1224, 368, 28, 4
    win = synth.make_window(w=w, h=h, W=2, P=20, seed=3, n_extra=1, step_z=0.15, yaw_deg=0.1)
    c = binding.Context(w, h, win.K, n_slots=4)
    for i in range(3):
        c.frame_upload(i, win.images[i])
    c.pixsel_set_random(np.random.RandomState(3).randint(0, 256, w * h).astype(np.uint8))
    num, _ = c.init_set_first(0)
    I = c.frame_download(0, 0)[0][:, 0].copy()
    dev, old, get = [], [], []
    for it in range(calls):
        c.init_track_frame(1 + it % 2)
        t0 = time.perf_counter()
        c.init_depth_image(0)
        dev.append(time.perf_counter() - t0)
    for it in range(calls):
        c.init_track_frame(1 + it % 2)
        t0 = time.perf_counter()
        p = c.init_points(0)
        t1 = time.perf_counter()
        want = ip.fast(I, w, h, p["u"], p["v"], p["iR"], p["isGood"])
        old.append(time.perf_counter() - t0)
        get.append(t1 - t0)
    assert np.array_equal(c.init_depth_image(0)["bgr"], want["bgr"])

    def med(x):
        return 1e3 * float(np.median(x[warm:]))
    print("init plot, %dx%d level 0, %d points: device %.3f ms | readback %.3f ms, readback + hostpaint %.3f ms" % (w, h, int(num[0]), med(dev), med(get), med(old)))
    c.close()


if __name__ == "__main__":
    main()

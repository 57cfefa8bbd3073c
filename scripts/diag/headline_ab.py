"""A/B driver: the headline step alone, ms per keyframe, timed on the library in the tree"""
import os, sys, time, gc
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import bench
gc.disable()
win, st6, trk = bench.make_inputs("kitti00_8kf")
job = bench.GpuJob(win, st6, trk, 0)
for _ in range(20): job.step(True)
for rep in range(3):
    job.ctx.sync(); t0 = time.perf_counter()
    for _ in range(300): job.step(True)
    job.ctx.sync(); print("headline ms/KF %.4f" % ((time.perf_counter() - t0) / 300 * 1e3), flush=True)

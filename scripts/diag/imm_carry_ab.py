"""The immature set across a keyframe, two ways in one process, the routes alternating per keyframe: wall time from the first call to a drained stream

  reissue  nalo_imm_resident_get, the caller's bookkeeping (here: one NumPy gather per array through the map the carry returned, the cheapest a caller can do),
           nalo_imm_create of the new keyframe's points, nalo_imm_resident_set + nalo_imm_resident_set_type: what a caller did before nalo_imm_resident_carry
  carry2   nalo_imm_resident_carry(A), then nalo_imm_resident_carry(C + B from the selector's map): the two calls of a keyframe
  carry1   the three parts in one call

on a 1224x368 frame with 8 hosts: the seam of a real keyframe (12 k points) and 160 k points; 30 % of the points leave with the activation, one host is dropped,
the selector's map of a noise image is appended. Every keyframe starts from the same set (nalo_imm_resident_set + _set_type, untimed). The script checks that the
routes leave the same set, bit for bit, in every word but lastTraceUV / lastTracePixelInterval, which the re-issue resets. The kernels' own times: run this under
rocprofv3 --kernel-trace --stats (rows immc_*)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import nalo_pkg  # noqa: E402

nalo_pkg.load()
from nalo_slam_amd import binding  # noqa: E402

W_IMG, H_IMG, HOSTS = 1224, 368, 8
SHAPES = {"seam12k": 12000, "set160k": 160000}


def u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run(name, keyframes):
    n = SHAPES[name]
    rng = np.random.RandomState(3)
    c = binding.Context(W_IMG, H_IMG, (700.0, 700.0, W_IMG / 2 - 0.5, H_IMG / 2 - 0.5), n_slots=2, levels=3)
    c.frame_upload(1, (100 + 50 * rng.rand(H_IMG, W_IMG)).astype(np.float32))
    c.pixsel_set_random(rng.randint(0, 256, W_IMG * H_IMG).astype(np.uint8))
    c.pixsel_make_maps(1, 1500.0, 3)
    idx, st = c.pixsel_get_selected()
    x, y = idx % W_IMG, idx // W_IMG
    inb = (x >= 3) & (x < W_IMG - 4) & (y >= 3) & (y < H_IMG - 4)
    ax, ay, ast = x[inb].astype(np.int32), y[inb].astype(np.int32), st[inb].astype(np.float32)
    f = lambda *s: rng.rand(*s).astype(np.float32)
    base = [f(n), f(n), f(n, 8), f(n, 8), f(n, 3), f(n)]
    host = rng.randint(0, HOSTS, n).astype(np.int32)
    state = [f(n), f(n), rng.randint(0, 6, n).astype(np.int32), f(n)]
    typ = rng.choice([1.0, 2.0, 4.0], n).astype(np.float32)
    fate = np.where(rng.rand(n) < 0.3, rng.choice([-1, -2, -3, 1], n), rng.choice([0, 2, 3], n)).astype(np.int32)
    sel = np.nonzero(fate == 1)[0].astype(np.int32)
    result = rng.choice([1, 0, -1], len(sel)).astype(np.int32)
    hm = np.int32([0, 1, 2, -1, 3, 4, 5, 6])
    app = dict(append_slot=1, append_host=HOSTS - 1)

    def prep():
        c.imm_resident_set(*base, host, *state)
        c.imm_resident_set_type(typ)
        c.sync()

    def carry1():
        c.imm_resident_carry(fate, sel, result, hm, **app)

    def carry2():
        c.imm_resident_carry(fate, sel, result)
        c.imm_resident_carry(host_map=hm, **app)
    prep(); carry1()
    src = c.imm_resident_carry_map()
    kept = src[src >= 0]
    new_host = np.concatenate([hm[host[kept]], np.full((src < 0).sum(), HOSTS - 1, np.int32)])

    def reissue():
        idmin, idmax, status, quality, _, _ = c.imm_resident_get()
        color, weights, gradH, eth = c.imm_create(1, ax, ay)
        ok = np.isfinite(eth)
        cat = lambda a, b: np.concatenate([a[kept], b[ok]])
        m = int(ok.sum())
        c.imm_resident_set(cat(base[0], ax.astype(np.float32)), cat(base[1], ay.astype(np.float32)), cat(base[2], color), cat(base[3], weights), cat(base[4], gradH),
                           cat(base[5], eth), new_host, cat(idmin, np.zeros(m, np.float32)), cat(idmax, np.full(m, np.nan, np.float32)),
                           cat(status, np.full(m, 5, np.int32)), cat(quality, np.full(m, 10000, np.float32)))
        c.imm_resident_set_type(cat(typ, ast))
    legs = {"reissue": reissue, "carry2": carry2, "carry1": carry1}
    names = list(legs)
    sets = {}
    for k in names:
        for _ in range(3):
            prep(); legs[k](); c.sync()
        p = c.imm_resident_get_points()
        sets[k] = [u32(p[q]) for q in sorted(p)] + [u32(a) for a in c.imm_resident_get()[:4]]
    same = all(all(np.array_equal(a, b) for a, b in zip(sets[k], sets["carry1"])) for k in names)
    ts = {k: [] for k in names}
    for i in range(keyframes):
        for j in range(len(names)):
            k = names[(i + j) % len(names)]
            prep()
            t0 = time.perf_counter()
            legs[k]()
            c.sync()
            ts[k].append(time.perf_counter() - t0)
    print("%s: %d points -> %d (%d appended), %d keyframes per route; the routes leave the same set: %s" % (name, n, len(src), (src < 0).sum(), keyframes, same))
    for k in names:
        t = np.array(ts[k]) * 1e6
        print("  %-7s median %9.1f us   p10 %9.1f   p90 %9.1f" % (k, np.median(t), np.percentile(t, 10), np.percentile(t, 90)), flush=True)
    c.close()
    return same


ap = argparse.ArgumentParser()
ap.add_argument("--keyframes", type=int, default=60)
ap.add_argument("--shapes", default="seam12k,set160k")
args = ap.parse_args()
ok = all([run(s, args.keyframes) for s in args.shapes.split(",")])
sys.exit(0 if ok else 1)

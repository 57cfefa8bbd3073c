"""activatePointsMT's steps 1-3 two ways in one process, the legs alternating per keyframe: wall time per keyframe, medians and spread

  parent   nalo_dist_make_map + nalo_imm_resident_get + the selection loop on the host + nalo_imm_resident_optimize(sel)
  device   one nalo_imm_resident_activate

The host loop is compiled code: a plain C++ restatement of FullSystem.cpp:805-876 with addIntoDistFinal's queue BFS, written for this script and built here
with hipcc -O2 as host code into a scratch directory. It is measurement scaffolding: the tests compare against tests/activation_model.py, not against it;
this script only checks that both legs select the same points.

  K      1224x368, W = 8, ~12 k immature points traced over two later frames of the synthetic sequence, 2000 active points
  scale  2560x1280, W = 8, 160 000 immature points with random states on flat images, 8000 active points

Then, with the library's event brackets on, the device time of the three stages (classify = classify + cell scan + scatter, resolve = the rounds,
emit = count + scan + list) and the rounds the selection ran. Kernel by kernel: run this under rocprofv3 --kernel-trace --stats."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import nalo_pkg  # noqa: E402

nalo_pkg.load()
from nalo_slam_amd import binding, synth  # noqa: E402
from imm_helpers import host_to_new, imm_points  # noqa: E402

HOST_LOOP = r"""
#include <cmath>
#include <vector>
extern "C" int host_select(int n, int W, int frame, int w1, int h1, float* D, const int* host, const float* u, const float* v, const float* idmin, const float* idmax,
                           const int* status, const float* quality, const float* interval, const float* type, const float* KRKi, const float* Kt, const int* flagged,
                           float minActDist, int* sel) {
    std::vector<std::vector<int>> by_host(W);
    for (int i = 0; i < n; ++i) by_host[host[i]].push_back(i);
    std::vector<int> a, b;
    int ns = 0;
    for (int h = 0; h < W; ++h) {
        if (h == frame) continue;
        const float* M = KRKi + 9 * h; const float* T = Kt + 3 * h;
        for (int i : by_host[h]) {
            if (!std::isfinite(idmax[i]) || status[i] == 2) continue;
            const bool can = (status[i] == 0 || status[i] == 3 || status[i] == 4 || status[i] == 1) && interval[i] < 8 && quality[i] > 3.0f && (idmax[i] + idmin[i]) > 0;
            if (!can) continue;
            const float z = 0.5f * (idmax[i] + idmin[i]);
            float p[3];
            for (int k = 0; k < 3; ++k) p[k] = M[3 * k] * u[i] + M[3 * k + 1] * v[i] + M[3 * k + 2] * 1 + T[k] * z;
            const float qu = p[0] / p[2] + 0.5f, qv = p[1] / p[2] + 0.5f;
            if (!(qu > -1e9f && qu < 1e9f && qv > -1e9f && qv < 1e9f)) continue;
            const int x = (int)qu, y = (int)qv;
            if (!(x > 0 && y > 0 && x < w1 && y < h1)) continue;
            if (!(D[x + w1 * y] + (p[0] - floorf(p[0])) >= minActDist * type[i])) continue;
            sel[ns++] = i;
            D[x + w1 * y] = 0;
            a.assign(1, x + w1 * y);
            for (int k = 1; k < 40 && !a.empty(); ++k) {
                b.clear();
                for (int idx : a) {
                    const int cx = idx % w1, cy = idx / w1;
                    if (cx == 0 || cy == 0 || cx == w1 - 1 || cy == h1 - 1) continue;
                    const int off[8] = {1, -1, w1, -w1, 1 + w1, -1 + w1, -1 - w1, 1 - w1};
                    for (int t = 0; t < ((k & 1) ? 8 : 4); ++t) if (D[idx + off[t]] > k) { D[idx + off[t]] = (float)k; b.push_back(idx + off[t]); }
                }
                a.swap(b);
            }
        }
    }
    return ns;
}
"""


def build_host_loop():
    d = tempfile.mkdtemp(prefix="nalo_activate_ab_")
    src, so = os.path.join(d, "host_select.cpp"), os.path.join(d, "libhost_select.so")
    open(src, "w").write(HOST_LOOP)
    subprocess.check_call(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-x", "c++", src, "-o", so])
    L = C.CDLL(so)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    L.host_select.argtypes = [C.c_int] * 5 + [fp, ip, fp, fp, fp, fp, ip, fp, fp, fp, fp, fp, ip, C.c_float, ip]
    return L


def level1_maps(win_K, world_to_cam, W, frame):
    fx, fy, cx, cy = [np.float32(x) for x in win_K]
    K1 = np.array([[fx * np.float32(0.5), 0, np.float32((cx + 0.5) / 2 - 0.5)], [0, fy * np.float32(0.5), np.float32((cy + 0.5) / 2 - 0.5)], [0, 0, 1]], np.float32)
    Ki0 = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]], np.float32)
    KRKi, Kt = np.zeros((W, 9), np.float32), np.zeros((W, 3), np.float32)
    for h in range(W):
        T = synth.se3_mul(world_to_cam[frame], synth.se3_inv(world_to_cam[h]))
        KRKi[h] = ((K1 @ T[:, :3].astype(np.float32)) @ Ki0).reshape(-1)
        Kt[h] = K1 @ T[:, 3].astype(np.float32)
    return KRKi, Kt


def setup_K():
    W = 8
    win = synth.make_window(w=1224, h=368, W=W, P=2000, seed=9, n_extra=2, step_z=0.25, yaw_deg=0.4)
    c = binding.Context(win.w, win.h, win.K, n_slots=W + 2)
    for i in range(W + 2):
        c.frame_upload(i, win.images[i])
    u, v, host = imm_points(win, per_host=1500, seed=4, margin=3)
    p = np.random.RandomState(11).permutation(len(u))
    u, v, host = u[p], v[p], host[p]
    n = len(u)
    color, weights, gradH, eth = [np.zeros((n, k), np.float32) for k in (8, 8, 3)] + [np.zeros(n, np.float32)]
    for h in range(W):
        m = host == h
        color[m], weights[m], gradH[m], eth[m] = c.imm_create(h, u[m], v[m])
    uf, vf = u.astype(np.float32), v.astype(np.float32)
    c.imm_resident_set(uf, vf, color, weights, gradH, eth, host, np.zeros(n, np.float32), np.full(n, np.nan, np.float32), np.full(n, 5, np.int32), np.full(n, 10000, np.float32))
    for new in (W, W + 1):
        c.imm_resident_trace(new, *host_to_new(win, new))
    my_type = np.random.RandomState(12).choice([1.0, 2.0, 4.0], n).astype(np.float32)
    c.imm_resident_set_type(my_type)
    c.ba_set_window(list(range(W)), win.world_to_cam[:W])
    c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
    KRKi, Kt = level1_maps(win.K, win.world_to_cam, W, W - 1)
    return c, W, uf, vf, host, my_type, KRKi, Kt


def setup_scale():
    w1, h1, W, n, na = 1280, 640, 8, 160000, 8000
    c = binding.Context(2 * w1, 2 * h1, (100.0, 100.0, w1 - 0.5, h1 - 0.5), n_slots=W)
    for s in range(W):
        c.frame_upload(s, np.full((2 * h1, 2 * w1), 100, np.float32))
    c.ba_set_window(list(range(W)), np.tile(np.eye(4)[:3], (W, 1, 1)))
    rng = np.random.RandomState(12)
    c.ba_set_points(np.zeros(na, np.int32), 2 * rng.randint(1, w1, na).astype(np.float32), 2 * rng.randint(1, h1, na).astype(np.float32), np.ones(na, np.float32),
                    np.zeros((na, 8), np.float32), np.ones((na, 8), np.float32))
    u = (2 * rng.randint(-2, w1 + 2, n) + 2 * rng.choice([0, 0.125, 0.25, 0.4375], n)).astype(np.float32)
    v = (2 * rng.randint(-2, h1 + 2, n)).astype(np.float32)
    host = rng.randint(0, W, n).astype(np.int32)
    status = rng.choice([0, 0, 0, 3, 4, 1, 2, 5], n).astype(np.int32)
    quality = rng.choice([10.0, 10.0, 10.0, 2.0], n).astype(np.float32)
    idmax = np.where(rng.rand(n) < 0.03, np.nan, 1.5).astype(np.float32)
    z = np.zeros((n, 8), np.float32)
    c.imm_resident_set(u, v, z, z, np.zeros((n, 3), np.float32), np.zeros(n, np.float32), host, np.full(n, 0.5, np.float32), idmax, status, quality)
    my_type = rng.choice([1.0, 2.0, 4.0], n).astype(np.float32)
    c.imm_resident_set_type(my_type)
    KRKi, Kt = np.tile(np.array([0.5, 0, 0, 0, 0.5, 0, 0, 0, 1], np.float32), (W, 1)), np.zeros((W, 3), np.float32)
    return c, W, u, v, host, my_type, KRKi, Kt


def run(name, setup, HL, keyframes, dist, min_obs):
    c, W, u, v, host, my_type, KRKi, Kt = setup()
    n, frame = len(u), W - 1
    flagged = np.zeros(W, np.int32); flagged[[1, W - 3]] = 1
    hi = np.ascontiguousarray(host, np.int32)
    selbuf = np.zeros(n, np.int32)
    F, I = binding._f, binding._i

    def parent():
        D = c.dist_make_map(frame, KRKi, Kt)
        idmin, idmax, status, quality, _, interval = c.imm_resident_get()
        ns = HL.host_select(n, W, frame, D.shape[1], D.shape[0], F(D), I(hi), F(u), F(v), F(idmin), F(idmax), I(status), F(quality), F(interval), F(my_type), F(KRKi), F(Kt),
                            I(flagged), dist, I(selbuf))
        sel = selbuf[:ns].copy()
        return sel, c.imm_resident_optimize(sel, min_obs) if ns else None

    def device():
        _, sel, opt = c.imm_resident_activate(frame, KRKi, Kt, flagged, dist, min_obs)
        return sel, opt
    legs = {"parent": parent, "device": device}
    names = list(legs)
    for k in names:                                                            # warm-up: allocations, code objects
        for _ in range(5):
            legs[k]()
    ts = {k: [] for k in names}
    for i in range(keyframes):
        for j in range(2):
            k = names[(i + j) % 2]
            c.sync()
            t0 = time.perf_counter()
            legs[k]()
            c.sync()
            ts[k].append(time.perf_counter() - t0)
    sp, op = parent()
    sd, od = device()
    same = np.array_equal(sp, sd) and (op is None or all(np.array_equal(a, b, equal_nan=True) for a, b in zip(op, od)))
    st = c.imm_activate_last()
    print("%s: %d resident points, minActDist %.1f, %d keyframes; survivors %d, selected %d, rejected by an earlier point %d, rounds %d; both legs agree: %s"
          % (name, n, dist, keyframes, st[0], st[1], st[2], st[3], same))
    for k in names:
        t = np.array(ts[k]) * 1e6
        print("  %-7s median %8.1f us   p10 %8.1f   p90 %8.1f" % (k, np.median(t), np.percentile(t, 10), np.percentile(t, 90)), flush=True)
    c.profile_enable(True)
    c.profile_reset()
    for _ in range(50):
        device()
    for s in ("dist_bfs", "act_classify", "act_resolve", "act_emit", "imm_optimize"):
        x = c.profile_samples(s)
        if len(x):
            print("  device stage %-13s median %7.1f us (%d samples; event brackets, so each includes ~10 us of bracket)" % (s, np.median(x), len(x)), flush=True)
    c.profile_enable(False)
    c.close()


ap = argparse.ArgumentParser()
ap.add_argument("--keyframes", type=int, default=200)
ap.add_argument("--shapes", default="K,scale")
ap.add_argument("--dist", type=float, default=1.0)
args = ap.parse_args()
HL = build_host_loop()
for s in args.shapes.split(","):
    run(s, {"K": setup_K, "scale": setup_scale}[s], HL, args.keyframes, args.dist, 3)

"""nalo_trk_set_ref_from_window: setCoarseTrackingRef (CoarseTracker.cpp:382-538, called at FullSystem.cpp:1404) fed from the BA window on the device.

The expected result is always nalo_trk_set_ref fed with the arrays the reference's loop would collect, extracted HERE in Python from nalo_ba_get_residuals /
nalo_ba_get_points: the IN residuals (state 0) that target the newest window frame, ordered by (host index, submission index), each with its centerProjectedTo
and its point's HdiF. Point clouds and depth / weight maps of every level must agree bit for bit.

Points are submitted shuffled and host-interleaved, so the reference order, the caller's order and the device order (host, then Hilbert cell:
nalo_ba_set_points) all differ. Pixels of the newest frame hit three or more times are summed in input order (trk_scatter_hot_kernel), so the order is
observable: test_order_sensitive_clusters plants such pixels and shows in numpy that the device order would change their sums."""
import numpy as np
import pytest

from nalo_slam_amd import binding, synth
from seq_helpers import GpuBackend, SequenceDriver, make_sequence

pytestmark = pytest.mark.gpu

ERR_STATE = -4
PRE_DIRECT_SLOTS = 32768          # ba_device.h kPreDirectSlots


# ------------------------------------------------------------------------------------------------ helpers
def expected_inputs(c, host_idx):
    """what makeCoarseDepthL0's loop collects, read back through the C-ABI: IN residuals to frame W-1, ordered by (host, submission index)"""
    st, _, _, _, cp = c.ba_get_residuals()
    hdi = c.ba_get_points()["HdiF"]
    W = st.shape[1]
    idx = np.nonzero(st[:, W - 1] == 0)[0]
    idx = idx[np.argsort(np.asarray(host_idx)[idx], kind="stable")]
    return idx, [np.ascontiguousarray(a, np.float32) for a in (cp[idx, W - 1, 0], cp[idx, W - 1, 1], cp[idx, W - 1, 2], hdi[idx])]


def tracker_ref(c):
    """every level's point cloud (u, v, idepth, colour) and idepth / weight maps"""
    return [c.trk_get_pc(l) + list(c.trk_get_depth(l)) for l in range(c.levels)]


def assert_same_ref(got, want):
    for l, (g, w) in enumerate(zip(got, want)):
        for k, (a, b) in enumerate(zip(g, w)):
            assert a.shape == b.shape, "level %d array %d: %s vs %s" % (l, k, a.shape, b.shape)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "level %d array %d: %d entries differ" % (l, k, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


def window_ctx(win, order, st6, n_slots=None):
    c = binding.Context(win.w, win.h, win.K, n_slots=n_slots or win.W)
    for i in range(win.W):
        c.frame_upload(i, win.images[i])
    c.ba_set_window(list(range(win.W)), win.world_to_cam[:win.W], state6=st6)
    c.ba_set_points(win.host[order], win.u[order], win.v[order], win.idepth[order], win.color[order], win.weights[order])
    c.ba_set_residuals(win.exists[order])
    return c


def check_against_host_arrays(c, host_idx):
    """the new call, then the host-array build on the extracted inputs in the same context: identical"""
    c.trk_set_ref_from_window()
    got = tracker_ref(c)
    idx, inp = expected_inputs(c, host_idx)
    c.trk_set_ref(c.W - 1, *inp)
    want = tracker_ref(c)
    assert_same_ref(got, want)
    return idx, inp, got


def hilbert_device_rank(host, u, v, w, h):
    """position of every submitted point in the device order of nalo_ba_set_points: stable sort by (host, Hilbert index of the 8x8 cell)"""
    hn = 1
    while hn * 8 < max(w, h):
        hn <<= 1
    x = np.minimum(hn - 1, np.maximum(0.0, u).astype(np.int64) >> 3)
    y = np.minimum(hn - 1, np.maximum(0.0, v).astype(np.int64) >> 3)
    d = np.zeros(len(u), np.int64)
    s = hn // 2
    while s > 0:
        rx, ry = ((x & s) > 0).astype(np.int64), ((y & s) > 0).astype(np.int64)
        d += s * s * ((3 * rx) ^ ry)
        flip = (ry == 0) & (rx == 1)
        x, y = np.where(flip, hn - 1 - x, x), np.where(flip, hn - 1 - y, y)
        x, y = np.where(ry == 0, y, x), np.where(ry == 0, x, y)
        s //= 2
    order = np.argsort((np.asarray(host, np.int64) << 40) | d, kind="stable")
    rank = np.empty(len(u), np.int64)
    rank[order] = np.arange(len(u))
    return rank


def hot_pixel_sums(Ku, Kv, nid, hdi, w, h, seq):
    """fp32 sums of the pixels with >= 3 hits, added in the order `seq` (indices into the input arrays): {pixel: (sum idepth*weight, sum weight)}"""
    u, v = np.trunc(Ku + np.float32(0.5)).astype(np.int64), np.trunc(Kv + np.float32(0.5)).astype(np.int64)
    ok = (u >= 0) & (v >= 0) & (u < w) & (v < h)
    pix = np.where(ok, u + w * v, -1)
    cnt = np.bincount(pix[ok], minlength=w * h)
    wgt = np.sqrt((1e-3 / (hdi.astype(np.float64) + 1e-12)).astype(np.float32))
    out = {}
    for i in seq:
        p = pix[i]
        if p < 0 or cnt[p] < 3:
            continue
        a, b = out.get(p, (np.float32(0), np.float32(0)))
        out[p] = (np.float32(a + np.float32(nid[i] * wgt[i])), np.float32(b + wgt[i]))
    return out


def _bilinear(img, x, y):
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    fx, fy = (x - x0).astype(np.float32), (y - y0).astype(np.float32)
    return ((1 - fx) * (1 - fy) * img[y0, x0] + fx * (1 - fy) * img[y0, x0 + 1] + (1 - fx) * fy * img[y0 + 1, x0] + fx * fy * img[y0 + 1, x0 + 1]).astype(np.float32)


def plant_clusters(win, n, seed):
    """n clusters on one pixel of the newest frame each: a world point X seen by host h2 < h1 at its exact projection, and two points of host h1 either side of
    an 8-pixel cell boundary (0.1 px apart, so they land with X): the device order (Hilbert cell) and the submission order of that pair can disagree, and
    with X added first the two orders give different fp32 sums. (Hits of one pixel from DIFFERENT hosts alone cannot show a device-order bug: the device
    order is host-major like the reference's, so their relative order is the same in both.) Returns the extended window (points appended, colours
    bilinear, true inverse depths)."""
    rng = np.random.RandomState(seed)
    W, w, h = win.W, win.w, win.h
    fx, fy, cx, cy = win.K
    N = 400000
    qx, qy = rng.randint(12, w - 12, N), rng.randint(12, h - 12, N)
    z = win.depth[W - 1][qy, qx].astype(np.float64)
    Xc = np.stack([(qx - cx) / fx * z, (qy - cy) / fy * z, z], 1)
    c2w = synth.se3_inv(win.world_to_cam[W - 1])
    Xw = Xc @ c2w[:, :3].T + c2w[:, 3]
    h1 = rng.randint(1, W - 1, N)
    h2 = (rng.rand(N) * h1).astype(np.int64)

    def proj(hh):
        T = win.world_to_cam[hh]
        Xh = np.einsum("nij,nj->ni", T[:, :, :3], Xw) + T[:, :, 3]
        return fx * Xh[:, 0] / Xh[:, 2] + cx, fy * Xh[:, 1] / Xh[:, 2] + cy, Xh[:, 2]

    u1, v1, z1 = proj(h1)
    u2, v2, z2 = proj(h2)
    ok = np.isfinite(z) & (z1 > 0) & (z2 > 0)
    for uu, vv in ((u1, v1), (u2, v2)):
        ok &= (uu > 6) & (uu < w - 7) & (vv > 6) & (vv < h - 7)
    B = 8 * np.round(u1 / 8)
    ok &= (np.abs(u1 - B) < 0.05) & (B >= 16)
    idx = np.nonzero(ok)[0]
    vis = np.ones(len(idx), bool)
    for hh, uu, vv, zz in ((h1, u1, v1, z1), (h2, u2, v2, z2)):
        dd = win.depth[hh[idx], np.round(vv[idx]).astype(int), np.round(uu[idx]).astype(int)]
        vis &= np.abs(dd - zz[idx]) < 0.01 * zz[idx]
    idx = idx[vis][:n]
    assert len(idx) == n, len(idx)
    # per cluster: [X on h2, h1 left of the boundary, h1 right of it]
    host = np.stack([h2[idx], h1[idx], h1[idx]], 1).reshape(-1)
    u = np.stack([u2[idx], B[idx] - 0.05, B[idx] + 0.05], 1).reshape(-1)
    v = np.stack([v2[idx], v1[idx], v1[idx]], 1).reshape(-1)
    idt = (1.0 / np.stack([z2[idx], z1[idx], z1[idx]], 1).reshape(-1)).astype(np.float32)
    gx = np.zeros_like(win.images); gy = np.zeros_like(win.images)
    gx[:, :, 1:-1] = 0.5 * (win.images[:, :, 2:] - win.images[:, :, :-2])
    gy[:, 1:-1, :] = 0.5 * (win.images[:, 2:, :] - win.images[:, :-2, :])
    col = np.zeros((len(u), 8), np.float32); wts = np.zeros((len(u), 8), np.float32)
    for k in range(8):
        xk, yk = u + synth.PATTERN[k, 0], v + synth.PATTERN[k, 1]
        col[:, k] = [_bilinear(win.images[hh], np.array([a]), np.array([b]))[0] for hh, a, b in zip(host, xk, yk)]
        g2 = gx[host, np.round(yk).astype(int), np.round(xk).astype(int)] ** 2 + gy[host, np.round(yk).astype(int), np.round(xk).astype(int)] ** 2
        wts[:, k] = np.sqrt(synth.OUTLIER_TH_SUMCOMP / (synth.OUTLIER_TH_SUMCOMP + g2))
    ex = np.ones((len(u), W), np.uint8)
    ex[np.arange(len(u)), host] = 0
    cat = lambda a, b: np.concatenate([a, b.astype(a.dtype)])
    import dataclasses
    return dataclasses.replace(win, host=cat(win.host, host), u=cat(win.u, u), v=cat(win.v, v), idepth=cat(win.idepth, idt), idepth_true=cat(win.idepth_true, idt),
                               color=cat(win.color, col), weights=cat(win.weights, wts), exists=cat(win.exists, ex))


# ------------------------------------------------------------------------------------------------ 1. after optimize(6)
@pytest.mark.parametrize("shape", ["kitti", "large"])
def test_after_optimize_matches_host_arrays(shape):
    if shape == "kitti":
        win = synth.make_window(w=1224, h=368, W=8, P=8000, seed=21, n_extra=0)
    else:
        win = synth.make_window(w=1224, h=368, W=8, P=250000, seed=22, n_extra=0)
    st6 = synth.perturbed_poses(win, sigma_t=0.003, sigma_r=0.0003)
    order = np.random.RandomState(1).permutation(len(win.host))          # shuffled, host-interleaved submission
    c = window_ctx(win, order, st6)
    cfg = c.ba_launch_config()
    if shape == "kitti":
        assert cfg["prelaunch_eligible"] == 1 and cfg["Ppad"] <= PRE_DIRECT_SLOTS       # the gated pre-launch path of optimize()
    else:
        assert cfg["Ppad"] > PRE_DIRECT_SLOTS and cfg["pull"] == 1
    c.ba_optimize(6)
    idx, inp, got = check_against_host_arrays(c, win.host[order])
    W = win.W
    assert len(idx) > 0.5 * np.count_nonzero(win.exists[:, W - 1])
    assert got[0][0].size > 1000
    if shape == "large":                      # many pixels with >= 3 hits: the ordered redo runs on the global list (> 4096 entries)
        u, v = np.trunc(inp[0] + np.float32(0.5)).astype(int), np.trunc(inp[1] + np.float32(0.5)).astype(int)
        ok = (u >= 0) & (v >= 0) & (u < win.w) & (v < win.h)
        cnt = np.bincount(u[ok] + win.w * v[ok])
        assert cnt[cnt >= 3].sum() > 4096
    # the call again, unchanged window: the same reference
    c.trk_set_ref_from_window()
    assert_same_ref(tracker_ref(c), got)
    c.close()


# ------------------------------------------------------------------------------------------------ 2. order sensitivity
def test_order_sensitive_clusters():
    base = synth.make_window(w=640, h=480, W=5, P=3000, seed=23, n_extra=0)
    win = plant_clusters(base, 300, seed=4)
    st6 = synth.perturbed_poses(win, sigma_t=0.002, sigma_r=0.0002)
    P = len(win.host)
    rng = np.random.RandomState(2)
    order = rng.permutation(P)
    # every pair of one host either side of a cell boundary is submitted against its device order half of the time
    c = window_ctx(win, order, st6)
    c.ba_optimize(6)
    idx, inp, got = check_against_host_arrays(c, win.host[order])
    host_s, u_s, v_s = win.host[order], win.u[order], win.v[order]
    rank = hilbert_device_rank(host_s, u_s, v_s, win.w, win.h)
    ref_seq = np.arange(len(idx))                                      # the inputs are in reference order already
    dev_seq = np.argsort(rank[idx], kind="stable")                     # the same inputs in device order
    assert not np.array_equal(ref_seq, dev_seq)
    s_ref = hot_pixel_sums(*inp, win.w, win.h, ref_seq)
    s_dev = hot_pixel_sums(*inp, win.w, win.h, dev_seq)
    assert len(s_ref) >= 20, len(s_ref)
    differ = [p for p in s_ref if s_ref[p][0] != s_dev[p][0] or s_ref[p][1] != s_dev[p][1]]
    assert len(differ) >= 1, "no hot pixel whose fp32 sums depend on the order: the test could not see an order bug"
    # and on the device: the host-array build in device order is a different reference
    c.trk_set_ref(win.W - 1, *[a[dev_seq] for a in inp])
    dev = tracker_ref(c)
    assert any(not np.array_equal(a.view(np.uint32), b.view(np.uint32)) for g, w in zip(dev, got) for a, b in zip(g, w) if a.shape == b.shape)
    c.close()


# ------------------------------------------------------------------------------------------------ 3. explicit linearize(fix=1)
def test_explicit_fix_linearization_accumulates_on_demand():
    win = synth.make_window(w=640, h=480, W=5, P=4000, seed=24, n_extra=0)
    st6 = synth.perturbed_poses(win, sigma_t=0.003, sigma_r=0.0003)
    order = np.random.RandomState(3).permutation(len(win.host))
    a, b = window_ctx(win, order, st6), window_ctx(win, order, st6)
    for c in (a, b):
        c.ba_linearize(False)
        c.ba_linearize(True)
    a.trk_set_ref_from_window()                                        # before any nalo_ba_get_points: HdiF comes from the on-demand accumulation
    got = tracker_ref(a)
    _, inp = expected_inputs(b, win.host[order])                      # nalo_ba_get_points runs the same accumulation on b
    assert np.all(inp[3] > 0)
    b.trk_set_ref(win.W - 1, *inp)
    assert_same_ref(got, tracker_ref(b))
    assert np.array_equal(a.ba_get_points()["HdiF"], b.ba_get_points()["HdiF"])
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 4. closed loop
class WindowRefBackend(GpuBackend):
    """GpuBackend whose tracking reference comes from nalo_trk_set_ref_from_window, checked at every keyframe against the host-array build"""
    name = "gpu-window-ref"

    def __init__(self, win):
        super().__init__(win)
        self.checked = 0

    def set_points(self, host_idx, u, v, idepth, color, weights, has_prior, exists):
        self.host_idx = np.array(host_idx)
        super().set_points(host_idx, u, v, idepth, color, weights, has_prior, exists)

    def set_tracking_ref(self, fid, calib, Ku, Kv, nid, hdi):
        c = self.c
        c._ck(c.L.nalo_trk_make_k(c.h_, *[float(x) for x in calib]))
        _, inp = expected_inputs(c, self.host_idx)
        c.trk_set_ref(fid, *inp)
        want = tracker_ref(c)
        c.trk_set_ref_from_window()                                    # this one stays: the tracking below runs on it
        assert_same_ref(tracker_ref(c), want)
        self.checked += 1


def test_closed_loop_sequence():
    win, kf = make_sequence(w=640, h=480, n_kf=10)
    B = [GpuBackend(win), WindowRefBackend(win)]
    drv = SequenceDriver(win, kf, B, teacher=False)
    drv.bootstrap()
    n_frames_marg, n_pts_marg, n_tracked = 0, 0, 0
    for k in range(2, len(kf)):
        rec = drv.add_keyframe(k)
        n_frames_marg += len(rec["flagged"]); n_pts_marg += rec["n_marg"]
        for (b, fid), (ok, T, aff) in rec["tracked"].items():
            if b == 1:
                ok0, T0, aff0 = rec["tracked"][(0, fid)]
                assert ok == ok0 and np.array_equal(T, T0) and np.array_equal(aff, aff0), "keyframe %d, frame %d" % (k, fid)
                n_tracked += 1
    assert B[1].checked == len(kf) - 1 and n_tracked >= len(kf) - 2
    assert n_frames_marg >= 1 and n_pts_marg > 0
    for be in B:
        be.close()


# ------------------------------------------------------------------------------------------------ 5. empty newest column, error paths
def test_empty_newest_column():
    win = synth.make_window(w=640, h=480, W=4, P=1500, seed=25, n_extra=0)
    win.exists[:, win.W - 1] = 0                                        # no residual targets the newest frame
    st6 = synth.perturbed_poses(win, sigma_t=0.003, sigma_r=0.0003)
    c = window_ctx(win, np.arange(len(win.host)), st6)
    c.ba_optimize(6)
    c.trk_set_ref_from_window()
    for l in range(c.levels):
        assert c.trk_get_pc(l)[0].size == 0
    e = np.zeros(0, np.float32)
    got = tracker_ref(c)
    c.trk_set_ref(win.W - 1, e, e, e, e)
    assert_same_ref(got, tracker_ref(c))
    c.close()


def test_error_paths_leave_the_resident_block_alone():
    win = synth.make_window(w=640, h=480, W=4, P=1500, seed=26, n_extra=0)
    st6 = synth.perturbed_poses(win, sigma_t=0.003, sigma_r=0.0003)
    order = np.random.RandomState(5).permutation(len(win.host))
    c = binding.Context(win.w, win.h, win.K, n_slots=win.W)
    call = lambda: c.L.nalo_trk_set_ref_from_window(c.h_)
    assert call() == ERR_STATE                                          # no window
    assert b"no window" in c.L.nalo_last_error(c.h_)
    for i in range(win.W):
        c.frame_upload(i, win.images[i])
    # a resident block of other inputs: replayed bit for bit after everything below
    rng = np.random.RandomState(6)
    n = 900
    res = [rng.uniform(5, win.w - 6, n), rng.uniform(5, win.h - 6, n), rng.uniform(0.05, 0.5, n), rng.uniform(1e-5, 1e-3, n)]
    c.trk_ref_upload(*res)
    c.trk_set_ref_resident(0)
    resident = tracker_ref(c)
    c.ba_set_window(list(range(win.W)), win.world_to_cam[:win.W], state6=st6)
    assert call() == ERR_STATE                                          # no points
    c.ba_set_points(win.host[order], win.u[order], win.v[order], win.idepth[order], win.color[order], win.weights[order])
    c.ba_set_residuals(win.exists[order])
    assert call() == ERR_STATE                                          # no linearisation yet
    c.ba_snapshot()
    c.ba_linearize(False)
    assert call() == ERR_STATE and b"linearizeAll(true)" in c.L.nalo_last_error(c.h_)      # fix = 0
    c.ba_optimize(6)
    c.trk_set_ref_from_window()
    good = tracker_ref(c)
    c.ba_set_allreduce(lambda ptr, k: None)                             # sharded: a one-rank hook is enough to refuse
    assert call() == ERR_STATE and b"nalo_trk_set_ref" in c.L.nalo_last_error(c.h_)
    c.ba_set_allreduce(None)
    c.trk_set_ref_from_window()
    assert_same_ref(tracker_ref(c), good)
    c.ba_restore()
    assert call() == ERR_STATE                                          # restored window: its last linearisation is gone
    c.ba_optimize(6)
    c.trk_set_ref_from_window()
    c.ba_marginalize_points(np.zeros(len(order), np.uint8))
    assert call() == ERR_STATE                                          # marginalisation relinearises
    c.ba_linearize(True)
    c.trk_set_ref_from_window()
    c.ba_set_residuals(win.exists[order])
    assert call() == ERR_STATE
    c.trk_set_ref_resident(0)
    assert_same_ref(tracker_ref(c), resident)
    c.close()

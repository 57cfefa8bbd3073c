"""nalo_tsdf_align_eval / _depth / _frame on the device (include/nalo_gpu.h, "The alignment") against tests/tsdf_align_model.py. The per-pixel records are
compared bit for bit - a NaN as a NaN - and the state counts exactly: the definition contains only correctly rounded float operations. Each of the 37 sums is
a sum of n exact products, so whatever the order the device adds them in, it lies within gamma_(n-1) * sum |term| (u = 2^-53) of the model's math.fsum: a
derived bound, not a tuned one. The loop is checked against its own rule from the traced numbers, and against the model's float64 loop."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

import tsdf_align_model as am
import tsdf_mesh_model as mm
import tsdf_model as tm
from nalo_slam_amd import binding
from test_tsdf_align_cpu import CH, CK, CORNER_START, CORNER_TRUE, CW, DEG, GRIDS, H0, K0, K86, LOOP, POSES, W0, compose, corner_model, corner_volume, fused_model, pose_error
from test_tsdf_cpu import EYE, pose, wavy_depth
from test_tsdf_gpu import bits_eq, ctx
from test_tsdf_raycast_cpu import plane_volume
from test_tsdf_raycast_gpu import dev, plant

pytestmark = pytest.mark.gpu
F = np.float32
ERR_ARG, ERR_STATE = -1, -4
SENT = 12345.0                                                                  # what the records hold where the kernel must not write
VIEW2 = (70, 33, (70.0, 68.0, 34.5, 16.0))                                      # partial tiles both ways


def vec(S):
    return np.concatenate([S["H"], S["b"], [S["E"], S["rr"]]])


def check_sums(got, rec, huber, step, tag=""):
    """the counts exactly, each of the 37 sums within the worst case of any summation order of the model's exact terms"""
    S = am.sums(rec, huber, step)
    assert got["count"] == S["count"], (tag, got["count"], S["count"])
    n = S["count"][0]
    bound = am.gamma(max(n - 1, 0)) * S["abs"]
    d = np.abs(vec(got) - vec(S))
    assert (d <= bound).all(), (tag, n, int(np.argmax(d - bound)), d.max(), bound.max())
    return S


def eval_both(c, vol, depth, K, c2w, s=1.0, mn=0.5, mx=3.5, mw=1.0, huber=0.02, step=1, dof=6, plane=None, with_sums=True, tag=""):
    """one evaluation on the device (from `plane`, or a fresh contiguous tensor of depth) with records, against the vectorised model"""
    h, w = depth.shape
    rec_t = torch.full((h, w, 10), SENT, device="cuda")
    got = c.tsdf_align_eval(dev(depth) if plane is None else plane, K, c2w, s, mn, mx, mw, huber, step, dof, records=rec_t)
    rec = rec_t.cpu().numpy()
    want = am.records(vol, depth, K, c2w, s, mn, mx, mw, huber, step, dof, fill=SENT)
    bad = ~((rec.view(np.uint32) == want.view(np.uint32)) | (np.isnan(rec) & np.isnan(want)))
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:4].tolist(), rec[bad][:4], want[bad][:4])
    if with_sums:
        check_sums(got, want, huber, step, tag)
    else:
        assert got["count"] == am.sums(want, huber, step)["count"], tag
    return got, rec


@pytest.fixture(scope="module")
def fused():
    """the two fused grids of tests/test_tsdf_gpu.py, planted from the model (tests/test_tsdf_align_cpu.py builds them once)"""
    out = []
    for gi in range(len(GRIDS)):
        c = ctx()
        out.append((c, plant(c, fused_model(gi))))
    yield out
    for c, _ in out:
        c.close()


@pytest.fixture(scope="module")
def corner():
    """the loop's scene: the three planes planted, and the depth plane ray-cast from the true pose with nalo_tsdf_raycast (it is the model's, bit for bit)"""
    c = ctx(CW, CH, CK)
    vol = plant(c, corner_volume())
    depth = c.tsdf_raycast(CW, CH, CK, CORNER_TRUE, 0.2, 4.0, 0.02, 1.0)["depth"]
    assert bits_eq(depth, corner_model(6)[1]) and (depth > 0).all()
    yield c, vol, depth
    c.close()


# ------------------------------------------------------------------------------------------------ records and sums on the fused volumes
@pytest.mark.parametrize("gi", [0, 1])
def test_records_and_sums_on_the_fused_volumes(fused, gi):
    """both plane sizes, the three poses, step 1, 2, 5 and one beyond w, both dof, s != 1"""
    c, vol = fused[gi]
    n_used = 0
    cases = [(1, 6, 1.0), (2, 7, 1.03), (5, 7, 0.98), (100, 6, 1.0), (1, 7, 1.02), (2, 6, 0.99)]
    for pi, c2w in enumerate(POSES):
        for vi, (w, h, K) in enumerate([(W0, H0, K0), VIEW2]):
            depth = wavy_depth(w, h, 10 * gi + pi, base=2.01)
            for step, dof, s in (cases if (pi, vi) == (0, 0) else [cases[(2 * pi + vi) % 6], cases[(2 * pi + vi + 3) % 6]]):
                got, _ = eval_both(c, vol, depth, K, c2w, s, step=step, dof=dof, tag=(gi, pi, vi, step, dof, s))
                n_used += got["count"][0]
                assert sum(got["count"]) == -(-w // step) * -(-h // step)
                if step == 100:
                    assert sum(got["count"]) == 1                                # pixel (0, 0) alone
    assert n_used > (3000, 100)[gi]


def test_records_against_the_literal_model(fused):
    c, vol = fused[0]
    w, h, K = VIEW2
    depth = wavy_depth(w, h, 3, base=2.01)
    _, rec = eval_both(c, vol, depth, K, POSES[1], 1.01, step=1, dof=7)
    px = [(int(u), int(v)) for u, v in np.random.RandomState(1).randint(0, (w, h), (250, 2))]
    lit = am.records_literal(vol, depth, K, POSES[1], 1.01, 0.5, 3.5, 1.0, 0.02, 1, 7, pixels=px)
    assert all(mm.same_floats(rec[v, u], lit[v, u]) for u, v in px) and sum(lit[v, u, 9] == 0 for u, v in px) > 30


# ------------------------------------------------------------------------------------------------ planted volumes, 8 x 6 planes, the literal model
def planted_eval(c, vol, depth, huber=0.125, dof=7, mn=0.5, mx=3.0, mw=1.0, c2w=EYE, s=1.0, K=K86):
    """the device's records of a small plane against the LITERAL model, every pixel; -> the states"""
    h, w = depth.shape
    rec_t = torch.full((h, w, 10), SENT, device="cuda")
    got = c.tsdf_align_eval(dev(depth), K, c2w, s, mn, mx, mw, huber, 1, dof, records=rec_t)
    rec = rec_t.cpu().numpy()
    lit = am.records_literal(vol, depth, K, c2w, s, mn, mx, mw, huber, 1, dof)
    assert mm.same_floats(rec, lit), (rec[~(rec == lit)][:8], lit[~(rec == lit)][:8])
    st = lit[..., 9].astype(int)
    assert got["count"] == tuple(int((st == k).sum()) for k in range(4))
    return st, lit


def test_planted_weights_nan_and_infinite_corners_under_every_sample():
    """pixel (0, 0) at D = 1.25 samples q = (3.8125, 4.4375, 3.0) of plane_volume: its cell starts at voxel (3, 4, 3). A corner that only the cell of q, of
    q + e_a or of q - e_a contains is made invalid in turn - a weight one ulp below min_weight (and, as the control, exactly at it), a NaN, and infinities"""
    c = ctx()
    base = plane_volume(1.3125)
    plant(c, base)
    depth = np.full((6, 8), 1.25, F)
    corners = {"q": (3, 4, 3), "+x": (5, 4, 3), "-x": (2, 4, 3), "+y": (3, 6, 3), "-y": (3, 3, 3), "+z": (3, 4, 5), "-z": (3, 4, 2)}
    seen = set()
    for name, (i, j, k) in corners.items():
        for kind, wv, tv in (("below", np.nextafter(F(1.0), F(0.0)), None), ("at", F(1.0), None), ("nan", None, F(np.nan)), ("+inf", None, F(np.inf)), ("-inf", None, F(-np.inf))):
            vol = dict(base, tsdf=base["tsdf"].copy(), weight=base["weight"].copy())
            if wv is not None:
                vol["weight"][k, j, i] = wv
            if tv is not None:
                vol["tsdf"][k, j, i] = tv
            c.tsdf_set((i, j, k), vol["tsdf"][k:k + 1, j:j + 1, i:i + 1], vol["weight"][k:k + 1, j:j + 1, i:i + 1])
            st, lit = planted_eval(c, vol, depth)
            want = 0 if kind == "at" else (2 if name == "q" else 3)
            if kind in ("below", "at", "nan"):
                assert st[0, 0] == want, (name, kind, st[0, 0])
            seen.add((kind, int(st[0, 0])))
            c.tsdf_set((i, j, k), base["tsdf"][k:k + 1, j:j + 1, i:i + 1], base["weight"][k:k + 1, j:j + 1, i:i + 1])
    assert {("below", 2), ("below", 3), ("at", 0), ("nan", 2), ("nan", 3)} <= seen
    st, _ = planted_eval(c, base, depth)
    assert (st[0, 0], st.min()) == (0, 0)                                       # everything was put back
    c.close()


def test_planted_grid_edges_depth_range_huber_and_a_zero_gradient():
    c = ctx()
    vol = plant(c, plane_volume(1.3125))
    up, dn = (lambda x: np.nextafter(F(x), F(np.inf))), (lambda x: np.nextafter(F(x), F(-np.inf)))
    # row 0: i_z exactly 0 (D = 0.5: q_z = 0) and exactly dim - 2 (D = 2.5: q_z = 8), for q itself and for its shifted samples (D = 0.75: q_z - 1 = 0; D = 2.25: q_z + 1 = 8)
    # row 1: both ends of [0.75, 2.25] and one ulp outside; row 2: 0, NaN, +inf, -inf, a negative depth; row 3: r exactly 0
    depth = np.full((6, 8), 1.25, F)
    depth[0, :4] = [0.5, 2.5, 0.75, 2.25]
    depth[1, :4] = [dn(0.75), up(0.75), dn(2.25), up(2.25)]
    depth[2, :5] = [0.0, np.nan, np.inf, -np.inf, -1.0]
    depth[3, :] = 1.3125
    st, lit = planted_eval(c, vol, depth)
    assert st[0, :4].tolist() == [3, 3, 0, 0] and (st[2, :5] == 1).all() and (lit[3, :, 0] == 0).all() and (st[3] == 0).all()
    st, _ = planted_eval(c, vol, depth, mn=0.75, mx=2.25)
    assert st[0, :4].tolist() == [1, 1, 0, 0] and st[1, :4].tolist() == [1, 0, 0, 1]
    # |r| just below, exactly at and just above huber: huber is the pixel's own |r| and its two neighbours
    r = lit[4, 0, 0]
    assert r == F(0.0625)
    for hb, hw in ((r, 1.0), (up(r), 1.0), (dn(r), float(dn(r) / r))):
        _, l2 = planted_eval(c, vol, depth, huber=float(hb))
        assert l2[4, 0, 1] == F(hw) and (hw == 1.0 or l2[4, 0, 1] < 1)
    # x at the grid's edges: a camera moved so that a pixel column lands on i_x = 0 (q_x = 0) or i_x = dim - 2 (q_x = 11) exactly, and one voxel further out
    for tx in (-0.953125, -1.203125, 0.703125, 0.953125):
        st, _ = planted_eval(c, vol, depth, c2w=pose(0, 0, 0, (tx, 0.0, 0.0)))
        assert len(set(st[4].tolist())) > 1                                     # the row crosses the edge: some pixels are used, some are not
    # a grid with a dimension of 1 has no cell: every usable pixel is state 2
    flat = tm.volume((-1.625, -1.625, 1.125), 0.25, (13, 13, 1), 0.5, 4.0)
    flat["weight"][:] = 1.0
    plant(c, flat)
    st, _ = planted_eval(c, flat, depth)
    assert set(st.ravel().tolist()) == {1, 2}
    # a zero gradient: a constant field. Every J is 0, the system is singular, and the loop says so
    const = plane_volume(1.3125)
    const["tsdf"][:] = 0.25
    plant(c, const)
    st, lit = planted_eval(c, const, np.full((6, 8), 1.25, F))
    assert (st == 0).all() and (lit[..., 0] == 0.25).all() and not lit[..., 2:9].any()
    r = c.tsdf_align_depth(dev(np.full((6, 8), 1.25, F)), K86, EYE, min_depth=0.5, max_depth=3.0, huber=0.125)
    assert (r["status"], r["iterations"], r["evaluations"]) == (binding.ALIGN_SOLVE_FAILED, 0, 1) and (r["cam_to_world"] == EYE).all()
    c.close()


# ------------------------------------------------------------------------------------------------ plane views, sums, determinism
def test_pitched_and_x_strided_views(fused):
    """the plane as a view inside a larger tensor whose other elements are usable depths: reading one of them would change records and sums"""
    c, vol = fused[0]
    w, h, K = VIEW2
    depth = wavy_depth(w, h, 5, base=2.01)
    ref, rec0 = eval_both(c, vol, depth, K, POSES[0], step=2, dof=7)
    big = torch.full((h + 7, 2 * w + 9), 2.2, device="cuda")
    for name, view in (("pitched", big[3:3 + h, 5:5 + w]), ("x-strided", big[2:2 + h, 1:1 + 2 * w:2]), ("both, shifted", big[4:4 + h, 3:3 + 2 * w:2])):
        view.copy_(dev(depth))
        got, rec = eval_both(c, vol, depth, K, POSES[0], step=2, dof=7, plane=view, tag=name)
        assert vec(got).tobytes() == vec(ref).tobytes() and rec.tobytes() == rec0.tobytes(), name
        view.fill_(2.2)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, CW * CH])
def test_each_of_the_37_sums_within_the_summation_bound(corner, n):
    """n used pixels of the corner scene's plane at a pose half way to the start (residuals and all seven Jacobian entries are far from 0); n = 1: exact"""
    c, vol, depth = corner
    keep = np.random.RandomState(n).permutation(CW * CH)[:n]
    d = np.zeros(CW * CH, F)
    d[keep] = depth.ravel()[keep]
    d = d.reshape(CH, CW)
    mid = compose([0.03, -0.025, 0.03, 0.3 * DEG, -0.32 * DEG, 0.24 * DEG], CORNER_TRUE)
    got, rec = eval_both(c, vol, d, CK, mid, 1.01, 0.2, 4.0, 1.0, 0.05, 1, 7, tag=n)
    assert got["count"] == (n, CW * CH - n, 0, 0)
    assert np.count_nonzero(vec(got)) >= 16 and ((rec[..., 1] < 1) & (rec[..., 9] == 0)).any()      # on an axis-aligned plane a pixel's g has zero entries
    if n == 1:
        S = am.sums(rec, 0.05)
        assert vec(got).tobytes() == vec(S).tobytes()


def test_two_runs_give_the_same_bytes(corner):
    c, vol, depth = corner
    runs = []
    for _ in range(2):
        rec_t = torch.full((CH, CW, 10), SENT, device="cuda")
        got = c.tsdf_align_eval(dev(depth), CK, CORNER_START, 1.03, 0.2, 4.0, 1.0, 0.25, 1, 7, records=rec_t)
        lp = c.tsdf_align_depth(dev(depth), CK, CORNER_START, 1.03, dof=7, max_iterations=4, min_used=100, **LOOP)
        runs.append((vec(got).tobytes(), got["count"], rec_t.cpu().numpy().tobytes(), result_bytes(lp)))
    assert runs[0] == runs[1]


def result_bytes(r):
    out = [r["cam_to_world"].tobytes(), np.float64([r["s"], r["E_first"], r["E_last"]]).tobytes(), (r["status"], r["iterations"], r["evaluations"], r["n_first"], r["n_last"]),
           vec(r["last"]).tobytes(), r["last"]["count"]]
    for t in r["trace"]:
        out += [t["cam_to_world"].tobytes(), np.float64([t["s"], t["lam"], t["E"]]).tobytes(), t["count"], t["accepted"]]
    return out


# ------------------------------------------------------------------------------------------------ the loop
def check_trace(c, vol, depth, K, r, dof, min_used, lambda0, eps, max_iterations, kw):
    """every traced evaluation against the model at the traced estimate; flags, lambdas, estimates and the status from the traced numbers by the header's rule"""
    need = max(min_used, 1)
    tr = r["trace"]
    assert len(tr) == r["evaluations"] == r["iterations"] + 1 and tr[0]["accepted"]
    lam = 0.01 if lambda0 == 0 else lambda0
    cur = tr[0]
    status = binding.ALIGN_ITERATION_LIMIT
    for k, t in enumerate(tr):
        rec = am.records(vol, depth, K, t["cam_to_world"], t["s"], kw["min_depth"], kw["max_depth"], kw["min_weight"], kw["huber"], kw["step"], dof)
        S = am.sums(rec, kw["huber"], kw["step"])
        n = S["count"][0]
        assert t["count"] == S["count"] and abs(t["E"] - S["E"]) <= am.gamma(max(n - 1, 0)) * S["abs"][35], (k, t["E"], S["E"])
        if k == 0:
            continue
        assert t["lam"] == lam, (k, t["lam"], lam)
        # the estimate is the host helper applied to the current estimate's system (the device's own sums: the same bytes on every run)
        sys_ = c.tsdf_align_eval(dev(depth), K, cur["cam_to_world"], cur["s"], kw["min_depth"], kw["max_depth"], kw["min_weight"], kw["huber"], kw["step"], dof)
        assert sys_["E"] == cur["E"] and sys_["count"] == cur["count"]
        inc, T, s = binding.tsdf_align_step(sys_["H"], sys_["b"], lam, dof, cur["cam_to_world"], cur["s"])
        assert T.tobytes() == t["cam_to_world"].tobytes() and s == t["s"], k
        ok = t["count"][0] >= need and t["E"] / t["count"][0] < cur["E"] / cur["count"][0]
        assert t["accepted"] == ok, (k, t, cur)
        if ok:
            cur, lam = t, lam * 0.5
        else:
            lam *= 4.0
        if math.sqrt(float(inc @ inc)) <= eps:
            status = binding.ALIGN_CONVERGED
            assert k == len(tr) - 1
    assert r["status"] == status and (status == binding.ALIGN_CONVERGED or r["iterations"] == max_iterations)
    assert r["cam_to_world"].tobytes() == cur["cam_to_world"].tobytes() and r["s"] == cur["s"] and (r["E_last"], r["n_last"]) == (cur["E"], cur["count"][0])
    assert (r["E_first"], r["n_first"]) == (tr[0]["E"], tr[0]["count"][0]) and r["last"]["E"] == cur["E"]


@pytest.mark.parametrize("dof", [6, 7])
def test_loop_on_the_three_planes(corner, dof):
    """From two voxels and one degree off (3 % off in scale for dof = 7), twelve iterations. The model's float64 loop from the same start, measured on the CPU
    (tests/test_tsdf_align_cpu.py): dof = 6 ends 2.54e-5 from the true camera centre and 0.00111 degrees from its rotation, which is the ray-cast's own
    interpolation error; with every sum of every evaluation moved by its worst-case summation error (gamma_(n-1) sum |term|, random signs, four seeds) the
    end moves by at most 3.1e-13 and 6.6e-10 degrees. The margin over the model's error is 1e-9 and 1e-7 degrees. dof = 7: three planes through one point are
    unchanged by a scaling about that point, so one direction of (t, s) is free; the model ends 0.0158 from the centre and 0.0083 off in scale after its twelve iterations (0.0423 and 0.0222 after twenty), the same
    perturbation moves its end by up to 3.5e-6, 1.2e-6 degrees and 1.9e-6 in scale, and the margin is 1e-4 for each. The residual per pixel must not rise."""
    c, vol, depth = corner
    s0 = 1.03 if dof == 7 else 1.0
    r = c.tsdf_align_depth(dev(depth), CK, CORNER_START, s0, dof=dof, max_iterations=12, min_used=100, lambda0=0.0, eps=1e-7, **LOOP)
    m = corner_model(dof)[2]
    check_trace(c, vol, depth, CK, r, dof, 100, 0.0, 1e-7, 12, LOOP)
    e, em = pose_error(r["cam_to_world"], r["s"]), pose_error(m["cam_to_world"], m["s"])
    print("align loop dof", dof, "device", e, "model", em, "status", r["status"], m["status"], "iterations", r["iterations"], m["iterations"])
    margin = (1e-9, 1e-7, 0.0) if dof == 6 else (1e-4, 1e-4, 1e-4)
    assert all(e[k] <= em[k] + margin[k] for k in range(3)), (e, em)
    per = [t["E"] / t["count"][0] for t in r["trace"] if t["accepted"]]
    assert all(b < a for a, b in zip(per, per[1:])) and r["E_last"] / r["n_last"] < 1e-4 * r["E_first"] / r["n_first"]
    if dof == 6:
        assert r["status"] == m["status"] == binding.ALIGN_CONVERGED and r["s"] == 1.0 and [t["accepted"] for t in r["trace"]] == [t["accepted"] for t in m["trace"]]


def test_loop_ends(corner):
    """a rejected first step, a start with too few pixels, the iteration limit, eps met at once, a capped trace"""
    c, vol, depth = corner
    d = dev(depth)
    done = c.tsdf_align_depth(d, CK, CORNER_START, dof=6, max_iterations=12, min_used=100, eps=1e-7, **LOOP)
    # from the converged estimate the next step makes the residual worse (model: E 0.0034357 -> 0.0034360): rejected, and the answer is est_in itself
    r = c.tsdf_align_depth(d, CK, done["cam_to_world"], dof=6, max_iterations=2, min_used=100, eps=0.0, **LOOP)
    check_trace(c, vol, depth, CK, r, 6, 100, 0.0, 0.0, 2, LOOP)
    assert [t["accepted"] for t in r["trace"]] == [True, False, False] and r["cam_to_world"].tobytes() == done["cam_to_world"].tobytes() and r["status"] == binding.ALIGN_ITERATION_LIMIT
    assert [t["lam"] for t in r["trace"]] == [0.01, 0.01, 0.04]
    # too few: a camera that looks at nothing, and a min_used above what there is
    away = np.array(CORNER_TRUE)
    away[:, 3] += 10.0
    for kw in (dict(cam_to_world=away, min_used=1), dict(cam_to_world=CORNER_START, min_used=CW * CH + 1)):
        r = c.tsdf_align_depth(d, CK, kw["cam_to_world"], dof=7, max_iterations=5, min_used=kw["min_used"], **LOOP)
        assert (r["status"], r["iterations"], r["evaluations"], len(r["trace"])) == (binding.ALIGN_TOO_FEW, 0, 1, 1) and r["cam_to_world"].tobytes() == np.asarray(kw["cam_to_world"]).tobytes()
        assert r["n_first"] == r["n_last"] == (0 if kw["min_used"] == 1 else CW * CH)
    # the iteration limit
    r = c.tsdf_align_depth(d, CK, CORNER_START, dof=6, max_iterations=2, min_used=100, eps=1e-7, **LOOP)
    check_trace(c, vol, depth, CK, r, 6, 100, 0.0, 1e-7, 2, LOOP)
    assert (r["status"], r["iterations"], r["evaluations"]) == (binding.ALIGN_ITERATION_LIMIT, 2, 3)
    # eps met at once: one step, taken and evaluated
    r = c.tsdf_align_depth(d, CK, CORNER_START, dof=6, max_iterations=9, min_used=100, eps=1e3, lambda0=0.5, **LOOP)
    check_trace(c, vol, depth, CK, r, 6, 100, 0.5, 1e3, 9, LOOP)
    assert (r["status"], r["iterations"], r["evaluations"]) == (binding.ALIGN_CONVERGED, 1, 2) and r["trace"][1]["accepted"] and r["trace"][1]["lam"] == 0.5
    # a trace cap below the evaluations, and none at all
    full = c.tsdf_align_depth(d, CK, CORNER_START, dof=6, max_iterations=4, min_used=100, **LOOP)
    for cap in (0, 2):
        r = c.tsdf_align_depth(d, CK, CORNER_START, dof=6, max_iterations=4, min_used=100, trace_cap=cap, **LOOP)
        assert len(r["trace"]) == cap and r["evaluations"] == 5 and result_bytes(dict(r, trace=[])) == result_bytes(dict(full, trace=[]))
        assert result_bytes(dict(r, trace=r["trace"]))[5:] == result_bytes(dict(full, trace=full["trace"][:cap]))[5:]


# ------------------------------------------------------------------------------------------------ nalo_tsdf_align_frame
def test_align_frame_equals_align_depth_of_the_models_plane():
    import plane_model as pm
    import test_dense_map_gpu as tdm
    from test_tsdf_gpu import FRAME_GRID, frame_scene, make
    w, h = 80, 48
    sc = frame_scene(w, h)
    c = tdm.context(sc)
    make(c, FRAME_GRID)
    # the volume holds ONE frame of a sparse plane: its weights have holes, and a 4 x 4 x 4 neighbourhood without one is rare. min_weight = 0 takes every voxel
    kw = dict(min_depth=0.5, max_depth=8.0, min_weight=0.0, huber=0.2, step=1, dof=6, max_iterations=3, min_used=10)
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
        c.tsdf_align_frame(tdm.FID, sc["K"], tdm.C2W, **kw)                       # the archive has not seen the frame yet
    assert c.tsdf_align_counts == (0, 0, 0, 0, 0)
    assert c.dense_update_map(0, pm.make_draws(w), tdm.C2W)[2] > 1000
    c.tsdf_integrate_frame(tdm.FID, tdm.C2W, sc["K"], 0.5, 8.0)
    with np.errstate(all="ignore"):
        D = tm.frame_plane(c.map_dense_get(tdm.FID), w, h)
    start = compose([0.02, -0.015, 0.03, 0.2 * DEG, -0.1 * DEG, 0.15 * DEG], tdm.C2W)
    before = [a.tobytes() for a in c.tsdf_get()]
    a = c.tsdf_align_frame(tdm.FID, sc["K"], start, **kw)
    b = c.tsdf_align_depth(dev(D), sc["K"], start, **kw)
    assert result_bytes(a) == result_bytes(b) and a["n_first"] > 100 and a["evaluations"] == a["iterations"] + 1 >= 2
    vol = dict(tm.volume(FRAME_GRID["origin"], FRAME_GRID["vs"], FRAME_GRID["dims"], FRAME_GRID["trunc"], FRAME_GRID["mw"]))
    vol["tsdf"], vol["weight"] = c.tsdf_get()
    check_sums(dict(a["last"]), am.records(vol, D, sc["K"], a["cam_to_world"], a["s"], 0.5, 8.0, 0.0, 0.2, 1, 6), 0.2, 1, "frame")
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
        c.tsdf_align_frame(tdm.FID + 7, sc["K"], start, **kw)                     # unknown frame_id
    c.ba_set_allreduce(lambda ptr, n: None)
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.tsdf_align_frame(tdm.FID, sc["K"], start, **kw)                         # a sharded window
    assert [x.tobytes() for x in c.tsdf_get()] == before
    c.close()


# ------------------------------------------------------------------------------------------------ stream order, side effects
def test_stream_order_without_a_host_wait_in_front(corner):
    """the plane is produced behind at least 0.2 s of matmuls on a torch stream. The call is made while they run (it does not wait for the producer before it
    queues its kernel), evaluates the right data, and with the release the tensor is overwritten on that stream right after"""
    c, vol, depth = corner
    wrong = (depth + F(0.3)).astype(F)
    d_right, d_wrong = dev(depth), dev(wrong)
    t = torch.empty_like(d_right)
    want = c.tsdf_align_eval(d_right, CK, CORNER_START, huber=0.25, min_depth=0.2, max_depth=4.0)
    assert vec(c.tsdf_align_eval(d_wrong, CK, CORNER_START, huber=0.25, min_depth=0.2, max_depth=4.0)).tobytes() != vec(want).tobytes()
    a = torch.randn(4096, 4096, device="cuda")
    out = torch.empty_like(a)
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        torch.mm(a, a, out=out)
        S.synchronize()
        t0 = time.perf_counter()
        torch.mm(a, a, out=out)
        S.synchronize()
        one = max(time.perf_counter() - t0, 1e-5)
        reps = min(int(math.ceil(0.25 / one)) + 1, 20000)
        for release in (False, True):
            t.copy_(d_wrong)
            for _ in range(reps):
                torch.mm(a, a, out=out)
            t.copy_(d_right)
            t_call = time.perf_counter()
            got = c.tsdf_align_eval(t, CK, CORNER_START, huber=0.25, min_depth=0.2, max_depth=4.0, release=release)      # stream=None: torch's current stream, S
            waited = time.perf_counter() - t_call
            if release:
                t.fill_(1.9)
            else:
                c.tsdf_release(S.cuda_stream)
                t.fill_(1.8)
            S.synchronize()
            assert vec(got).tobytes() == vec(want).tobytes() and got["count"] == want["count"], release
            assert waited > 0.1, "the producer's matmuls were not queued in front of the call (%.3f s)" % waited
            assert float(t[0, 0]) == F(1.9 if release else 1.8)
    torch.cuda.synchronize()


def test_a_twin_that_never_aligns_has_the_same_volume():
    vol = fused_model(0)
    out = []
    for align in (True, False):
        c = ctx()
        plant(c, vol)
        d = dev(wavy_depth(W0, H0, 1, base=2.01))
        c.tsdf_integrate_depth(d, K0, POSES[0], 0.5, 3.5)
        if align:
            rec_t = torch.zeros((H0, W0, 10), device="cuda")
            c.tsdf_align_eval(d, K0, POSES[1], 1.02, 0.5, 3.5, 1.0, 0.02, 2, 7, records=rec_t)
            c.tsdf_align_depth(d, K0, POSES[0], 1.0, 0.5, 3.5, 1.0, 0.05, 1, 7, max_iterations=3)
        c.tsdf_integrate_depth(d, K0, POSES[1], 0.5, 3.5)
        out.append([a.tobytes() for a in c.tsdf_get()] + [repr(c.tsdf_last()), d.cpu().numpy().tobytes()])
        c.close()
    assert out[0] == out[1]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_everything_and_the_next_call_works(corner):
    c, vol, depth = corner
    d = dev(depth)
    rec_t = torch.full((CH, CW, 10), SENT, device="cuda")
    trace = (binding.TsdfAlignTrace * 4)()

    def call(which, est=(CORNER_START, 1.0), plane=None, null=None, trace_cap=4, trace_ptr=True, **kw):
        args = dict(depth=d if plane is None else plane, K=CK, min_depth=0.2, max_depth=4.0, min_weight=1.0, huber=0.25, step=1, dof=7, stream=0, records=rec_t,
                    max_iterations=3, min_used=1, lambda0=0.0, eps=1e-7)
        args.update(kw)
        a, _ = c._align_args(**args)
        e = binding.tsdf_align_est(*est)
        S, R = binding.TsdfAlignSums(), binding.TsdfAlignResult()
        C.memset(C.byref(S), 0x5A, C.sizeof(S))
        C.memset(C.byref(R), 0x5A, C.sizeof(R))
        R.trace, R.trace_cap = (trace if trace_ptr else None), trace_cap
        C.memset(trace, 0x5A, C.sizeof(trace))
        pa, pe = (None if null == "args" else C.byref(a)), (None if null == "est" else C.byref(e))
        if which == "eval":
            rc = c.L.nalo_tsdf_align_eval(c.h_, pa, pe, C.byref(S))
            kept = bytes(S)[:37 * 8] == b"\x5a" * (37 * 8) and tuple(S.count) == (0, 0, 0, 0)
        else:
            rc = c.L.nalo_tsdf_align_depth(c.h_, pa, pe, C.byref(R))
            kept = (bytes(R.est) == b"\x5a" * C.sizeof(R.est) and bytes(R.last) == b"\x5a" * C.sizeof(R.last) and bytes(trace) == b"\x5a" * C.sizeof(trace) and
                    (R.iterations, R.evaluations, R.n_first, R.n_last, R.n_trace) == (0, 0, 0, 0, 0))
        return rc, kept

    before = [a.tobytes() for a in c.tsdf_get()]
    nan_pose, inf_pose = np.array(CORNER_START), np.array(CORNER_START)
    nan_pose[1, 2], inf_pose[0, 3] = np.nan, np.inf
    host = np.zeros((CH, CW), F)
    u8 = torch.zeros((CH, CW), dtype=torch.uint8, device="cuda")
    rgb = torch.zeros((CH, CW, 3), device="cuda")
    small = torch.zeros(CH * CW * 10 - 1, device="cuda")
    bad_planes = [binding.DevPlane(host.ctypes.data, binding.DT_F32, CW, CH, 1, 4 * CW, 4, 0), binding.dev_plane(u8), binding.dev_plane(rgb, "hwc"),
                  binding.DevPlane(None, binding.DT_F32, CW, CH, 1, 4 * CW, 4, 0), binding.DevPlane(d.data_ptr(), binding.DT_F32, CW, CH, 1, 4 * CW, 2, 0)]
    common = [dict(plane=p) for p in bad_planes] + [
        dict(step=0), dict(step=-3), dict(dof=5), dict(dof=8), dict(est=(nan_pose, 1.0)), dict(est=(inf_pose, 1.0)), dict(K=(np.nan, 80.0, 47.5, 35.5)), dict(K=(80.0, 80.0, 47.5, np.inf)),
        dict(est=(CORNER_START, np.nan)), dict(est=(CORNER_START, np.inf)), dict(est=(CORNER_START, 0.0)), dict(est=(CORNER_START, -1.0)), dict(huber=0.0), dict(huber=-0.1),
        dict(huber=np.nan), dict(huber=np.inf), dict(min_depth=2.0, max_depth=1.0), dict(min_depth=np.nan), dict(max_depth=np.inf), dict(min_weight=np.nan), dict(records=small),
        dict(null="args"), dict(null="est")]
    loop_only = [dict(max_iterations=0), dict(max_iterations=65), dict(trace_cap=-1), dict(trace_cap=2, trace_ptr=False), dict(lambda0=-1.0), dict(lambda0=np.nan), dict(eps=-1.0), dict(eps=np.nan)]
    for which, cases in (("eval", common), ("depth", common + loop_only)):
        for kw in cases:
            rc, kept = call(which, **kw)
            assert rc == ERR_ARG and kept, (which, kw, rc, kept)
        assert call(which) == (0, False)                                        # the next legal call works
    assert (rec_t.cpu().numpy()[..., 9] != SENT).all()                          # ... and wrote its records; no refused call did:
    rec_t.fill_(SENT)
    for kw in common[:8]:
        call("eval", **kw)
    torch.cuda.synchronize()
    assert (rec_t == SENT).all() and [a.tobytes() for a in c.tsdf_get()] == before
    assert c.L.nalo_tsdf_align_eval(c.h_, None, None, None) == ERR_ARG and c.L.nalo_tsdf_align_depth(c.h_, None, None, None) == ERR_ARG
    # no volume: NALO_ERR_STATE, for all three; no dense archive: the frame route's own
    c2 = ctx(CW, CH, CK)
    for fn in (lambda: c2.tsdf_align_eval(d, CK, CORNER_START), lambda: c2.tsdf_align_depth(d, CK, CORNER_START), lambda: c2.tsdf_align_frame(1, CK, CORNER_START)):
        with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
            fn()
    assert c2.tsdf_align_counts == (0, 0, 0, 0, 0)
    plant(c2, plane_volume(1.3125))
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c2.tsdf_align_frame(1, CK, CORNER_START)                                # the dense archive is not enabled
    c2.close()


# ------------------------------------------------------------------------------------------------ the device chain
def run_chain():
    """tests/test_tsdf_gpu.py's chain at 1224x368, W = 8, three keyframes into 256x64x256 voxels; every keyframe is aligned (nalo_tsdf_align_frame) before it is
    integrated. -> per keyframe (result, the frame's dense points, the volume as it was aligned against), and the pose and K used"""
    import lifecycle_model as lm
    import lifecycle_scenes as lsc
    import plane_cases as pc
    import plane_model as pm
    from nalo_slam_amd import synth
    WW, KF, w, h, s = 8, 3, 1224, 368, 3e-4
    win = synth.make_window(w=w, h=h, W=WW, P=8000, seed=lsc.SEED, n_extra=KF, step_z=0.8 * s, step_x=0.03 * s, full_graph=False)
    nF = WW + KF
    srng = np.random.RandomState(lsc.SEED + 3)
    st6 = np.zeros((nF, 6))
    st6[1:, :3] = 0.004 * srng.randn(nF - 1, 3) / 0.5
    st6[1:, 3:] = 0.0004 * srng.randn(nF - 1, 3)
    mask = pc.block_mask(w, h, 2, 1, [2.0, 0.0])
    mask[2 * h // 3:, :w // 2] = 6.0
    mask[2 * h // 3:, w // 2:] = 8.0
    bgr = np.random.RandomState(1).randint(0, 256, (h, w, 3)).astype(np.uint8)
    c = binding.Context(w, h, win.K, n_slots=nF)
    fids = [200 + i for i in range(WW)]
    for i in range(nF):
        c.frame_upload(i, win.images[i], mask=mask, bgr=bgr)
    c.ba_set_prior_carry(True)
    c.ba_set_window(list(range(WW)), win.world_to_cam[:WW], state6=st6[:WW], frame_ids=fids)
    c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
    c.ba_set_residuals(win.exists)
    ng0, lt0, ls0 = lm.default_history(win.exists)
    ls0[win.host == WW - 1, 0] = lm.IN
    c.ba_set_point_history(ng0, lt0, ls0)
    c.map_enable()
    c.map_dense_enable(True, 65536)
    cur, out = list(fids), []
    for kf in range(KF):
        if kf:
            c.ba_marginalize_frame(0)
            c.ba_carry_window(c.frame_state(WW - 1 + kf, win.world_to_cam[WW - 1 + kf], frame_id=200 + WW - 1 + kf, state6=st6[WW - 1 + kf]))
            cur = cur[1:] + [200 + WW - 1 + kf]
        c.ba_linearize(False)
        c.ba_linearize(True)
        hf, slot = WW - 3, WW - 3 + kf
        T = synth.se3_inv(win.world_to_cam[slot])
        c.dense_update_map(hf, pm.make_draws(60 + kf), T)
        pts = c.map_dense_get(cur[hf])
        if kf == 0:
            xyz = c.map_dense_world_points(cur[hf], T)
            ok = np.isfinite(xyz).all(1)
            lo, hi = np.percentile(xyz[ok], 2, axis=0), np.percentile(xyz[ok], 98, axis=0)
            vs = float(max((hi - lo) / np.array([256, 64, 256])) * 1.05)
            origin = 0.5 * (lo + hi) - 0.5 * vs * np.array([256, 64, 256])
            dep = 1.0 / pts["idepth"].astype(np.float64)
            dep = dep[np.isfinite(dep) & (dep > 0)]
            rng_d = (float(np.percentile(dep, 2)) * 0.5, float(np.percentile(dep, 98)) * 2.0)
            c.tsdf_create(origin, vs, (256, 64, 256), 4 * vs, 16.0)
            geo = (origin, vs)
        # the dense planes are sparse, so the fused weights have holes: min_weight = 0 takes every voxel (at min_weight = 1 no pixel of this chain has all seven samples)
        kw = dict(min_depth=rng_d[0], max_depth=rng_d[1], min_weight=0.0, huber=0.5, step=1, dof=7, max_iterations=2, min_used=50)
        r = c.tsdf_align_frame(cur[hf], win.K, T, **kw)
        out.append((r, pts, c.tsdf_get(), T, kw))
        c.tsdf_integrate_frame(cur[hf], T, win.K, rng_d[0], rng_d[1])
        ff = np.zeros(WW, np.uint8)
        ff[0] = 1
        c.ba_flag_points(ff)
        c.ba_marginalize_flagged()
    final = [a.tobytes() for a in c.tsdf_get()]
    c.close()
    return out, final, geo, win.K, (w, h)


def test_three_keyframes_are_aligned_before_they_are_integrated_at_1224x368():
    a, vol_a, geo, K, (w, h) = run_chain()
    b, vol_b, _, _, _ = run_chain()
    assert vol_a == vol_b and [result_bytes(x[0]) for x in a] == [result_bytes(x[0]) for x in b]
    # the first keyframe meets an empty volume: tsdf = 1 everywhere, every gradient 0, a singular system
    assert (a[0][0]["status"], a[0][0]["iterations"]) == (binding.ALIGN_SOLVE_FAILED, 0) and a[0][0]["n_first"] > 1000 and not a[0][0]["last"]["H"].any()
    used = []
    for kf, (r, pts, (t, wgt), T, kw) in enumerate(a):
        vol = tm.volume(geo[0], geo[1], (256, 64, 256), 4 * geo[1], 16.0)
        vol["tsdf"], vol["weight"] = t, wgt
        with np.errstate(all="ignore"):
            D = tm.frame_plane(pts, w, h)
        for tr in r["trace"]:                                                   # every evaluation of the loop against the vectorised model
            rec = am.records(vol, D, K, tr["cam_to_world"], tr["s"], kw["min_depth"], kw["max_depth"], 0.0, 0.5, 1, 7)
            S = am.sums(rec, 0.5)
            assert tr["count"] == S["count"] and abs(tr["E"] - S["E"]) <= am.gamma(max(S["count"][0] - 1, 0)) * S["abs"][35], (kf, tr["count"], S["count"])
        check_sums(dict(r["last"]), am.records(vol, D, K, r["cam_to_world"], r["s"], kw["min_depth"], kw["max_depth"], 0.0, 0.5, 1, 7), 0.5, 1, ("chain", kf))
        used.append(r["n_first"])
    print("align chain 1224x368 into 256x64x256: used pixels", used, "status", [x[0]["status"] for x in a], "E/n", [(x[0]["E_first"] / max(x[0]["n_first"], 1), x[0]["E_last"] / max(x[0]["n_last"], 1)) for x in a])
    assert used[1] > 1000 and used[2] > 1000                                    # not vacuous: the later keyframes land on fused surface

"""NumPy restatement of the reference's ground-plane scale correction, line by line (paths relative to the reference's src/):
  score            CoarseTracker::fitPlane            FullSystem/CoarseTracker.cpp:299-378
  choose, mark     CoarseTracker::makeCoarseDepthL0   FullSystem/CoarseTracker.cpp:563-625, 669-693
  Machine.update   the same function                  FullSystem/CoarseTracker.cpp:609-616, 696-816
  set_global_plane FullSystem::setglobalplane         FullSystem/FullSystem.cpp:1911-1976
  local_scale      FullSystem::planeOptimize          FullSystem/PlaneOptimize.cpp:203-211
It is built over tests/plane_model.py: a cluster is one of its dicts (members, xx, yy, mask_value, n, n_cloud, fitted, plane). The fitted plane is an INPUT of the
score: a test of the device passes the device's own records, because a refined plane is only held to a tolerance (test_plane_fit_gpu.py), and everything here is
compared bit for bit. All float arithmetic is float32 in the order the reference writes it."""
import numpy as np

import plane_model as pm

F = np.float32
FLT_MAX = np.finfo(F).max
SCORE_OUT = F(9999999)


def takes_part(c, min_points=20):
    """fitPlane returns true: no member failed the finite test (:320-324) and the cloud has min_points points (:336; 20 in the tracker)"""
    return bool(c["fitted"]) and c["n_cloud"] == c["n"] and c["n_cloud"] >= min_points


def mid_z(c, idepth, K):
    """:332 `mid_z += point.z / size_points` over the members in vector order: a chain of float adds"""
    _, _, Z = pm.back_project(c["xx"], c["yy"], np.asarray(idepth, F)[c["members"]], K)
    n = F(len(c["members"]))
    s = F(0)
    with np.errstate(all="ignore"):
        for z in Z:
            s = F(s + F(z / n))
    return s


def mid_z_fast(c, idepth, K):
    """mid_z() for large clusters: np.add.accumulate adds in index order, one float32 add per term. Held equal to mid_z() in the CPU tests."""
    _, _, Z = pm.back_project(c["xx"], c["yy"], np.asarray(idepth, F)[c["members"]], K)
    with np.errstate(all="ignore"):
        return np.add.accumulate((Z / F(len(Z))).astype(F), dtype=F)[-1]


def score(c, idepth, K, plane=None, min_points=20, fast=False):
    """-> (scored, mid_z, score) of one cluster; plane: the fitted (a, b, c, d), the cluster's own by default"""
    if not takes_part(c, min_points):
        return 0, F(0), F(0)
    a, b, cc, d = [F(x) for x in (c["plane"] if plane is None else plane)]
    n = len(c["members"])
    mz = (mid_z_fast if fast else mid_z)(c, idepth, K)
    if n < 100 or mz < 0 or F(c["mask_value"]) < 200:                  # :363-368
        return 1, mz, SCORE_OUT
    with np.errstate(all="ignore"):
        dot = F(a + cc)                                                # :370-371: x_axis . dir + z_axis . dir
        s = F(F(F(dot * F(1000)) + F(np.abs(d) * F(100))) + F(100 // n))       # :373: float abs, INTEGER 100 / size
    return 1, mz, s


def choose(clusters, idepth, K, planes=None, min_points=20, fast=False):
    """the loop of :582-625 without the append -> dict(ran, cluster, gp_raw, ground_height, scores [(scored, mid_z, score)], g_u, g_v)"""
    out = dict(ran=0, cluster=-1, gp_raw=np.zeros(4, F), ground_height=None, scores=[], g_u=[], g_v=[])
    if len(clusters) < 4:                                              # :563-567
        return out
    out["ran"] = 1
    min_score = FLT_MAX
    for i, c in enumerate(clusters):
        pl = np.asarray(c["plane"] if planes is None else planes[i], F)
        sc = score(c, idepth, K, pl, min_points, fast)
        out["scores"].append(sc)
        if not sc[0]:
            continue                                                   # :591
        if sc[2] < min_score:                                          # :609 (false for a NaN)
            out["gp_raw"] = (-pl if pl[1] > 0 else pl).astype(F).copy()         # :611-614
            out["ground_height"] = F(np.abs(pl[3]))
            min_score = sc[2]
            out["cluster"] = i
            out["g_u"] = [int(x) for x in c["xx"]]
            out["g_v"] = [int(y) for y in c["yy"]]
    return out


def c_int_round(x):
    """`int u = x + 0.5f` (:679): the float sum, then the conversion as the device defines it (saturating, NaN -> 0)"""
    with np.errstate(all="ignore"):
        return pm._c_int(F(F(x) + F(0.5)))


def mark(g_u, g_v, tested, cpt_u, cpt_v):
    """:669-693 as the double loop it is. tested[p]: lastResiduals[0] names an IN residual to the newest frame -> (onground bytes, temp_gp_num)"""
    on = np.zeros(len(tested), np.uint8)
    num = 0
    for p in range(len(tested)):
        if not tested[p]:
            continue
        u, v = c_int_round(cpt_u[p]), c_int_round(cpt_v[p])
        for gi in range(len(g_u)):
            if u == g_u[gi] and v == g_v[gi]:
                on[p] = 1
                num += 1
                break
    return on, num


def mark_fast(g_u, g_v, tested, cpt_u, cpt_v):
    """mark() for large inputs: membership in the set of (g_u, g_v) pairs. Held equal to mark() in the CPU tests."""
    pix = set(zip(g_u, g_v))
    on = np.array([1 if tested[p] and (c_int_round(cpt_u[p]), c_int_round(cpt_v[p])) in pix else 0 for p in range(len(tested))], np.uint8)
    return on, int(on.sum())


class Frame:
    def __init__(self):
        self.groundP = np.zeros(4, F)
        self.last_ground = np.zeros(4, F)                              # uninitialised in the reference (HessianBlocks.h:270): DEFINED as zeros
        self.haveground = 0
        self.scaleFixed = 0


class Tracker:
    """the members of one CoarseTracker object (CoarseTracker.cpp:104-106)"""
    def __init__(self):
        self.ground_height, self.last_height, self.suc_num = F(-1), F(-1), 0


class Globals:
    """util/settings.cpp:36-40"""
    def __init__(self):
        self.scale_fix = 0
        self.init_height = F(-1)
        self.last_ScaleRate = F(-1)
        self.last_gp = np.full(4, -1, F)
        self.old_rate = []


def update(pick, tr, g, frames):
    """pick: dict(ran, cluster, gp_raw, ground_height). CoarseTracker.cpp:609-616 and 696-816 as written."""
    if not pick["ran"]:
        return                                                         # :566
    gp_raw = np.zeros(4, F)                                            # :577
    if pick["cluster"] >= 0:
        gp_raw = np.asarray(pick["gp_raw"], F).copy()
        tr.ground_height = F(pick["ground_height"])                    # :615
    back = frames[-1]
    gh = F(tr.ground_height)
    with np.errstate(all="ignore"):
        if not g.scale_fix:                                            # :696
            if tr.last_height < 0:
                tr.last_height = gh
            else:
                diff = F(np.abs(F(tr.last_height - gh)))
                if float(diff) < 0.01:                                 # the float against the double literal
                    tr.suc_num += 1
                else:
                    tr.suc_num = 0
            if tr.suc_num > 3:
                g.init_height = F(F(gh + tr.last_height) / F(2))
                g.scale_fix = 1
            tr.last_height = gh
        else:
            scale_rate = F(gh / g.init_height)                         # :720
            if g.last_ScaleRate < 0:
                g.last_ScaleRate = scale_rate
                g.last_gp = gp_raw.copy()
                g.old_rate.append(g.last_ScaleRate)
            else:
                ave2 = ave3 = ave4 = ave5 = scale_rate
                o, size = g.old_rate, len(g.old_rate)
                a2 = lambda: F(np.abs(F(o[size - 1] + o[size - 2])) / F(2))
                a3 = lambda: F(np.abs(F(F(o[size - 1] + o[size - 2]) + o[size - 3])) / F(3))
                a4 = lambda: F(np.abs(F(F(F(o[size - 1] + o[size - 2]) + o[size - 3]) + o[size - 4])) / F(4))
                a5 = lambda: F(np.abs(F(F(F(F(o[size - 1] + o[size - 2]) + o[size - 3]) + o[size - 4]) + o[size - 5])) / F(5))
                if size > 5:                                           # :736-755
                    ave2, ave3, ave4, ave5 = a2(), a3(), a4(), a5()
                elif size > 4:
                    ave2, ave3, ave4 = a2(), a3(), a4()
                elif size > 3:
                    ave2, ave3 = a2(), a3()
                elif size > 2:
                    ave2 = a2()
                diff = F(np.abs(F(g.last_ScaleRate - scale_rate)) / g.last_ScaleRate)
                diffs = [diff] + [F(np.abs(F(a - scale_rate)) / a) for a in (ave2, ave3, ave4, ave5)]
                if all(float(d) > 0.25 for d in diffs):                # :762
                    scale_rate = g.last_ScaleRate
                    back.groundP = g.last_gp.copy()                    # :767; haveground stays (:768 is commented out)
                else:
                    g.last_ScaleRate = scale_rate
                    back.haveground = 1
                    back.groundP = gp_raw.copy()
                if len(g.old_rate) < 7:                                # :780-788
                    g.old_rate.append(g.last_ScaleRate)
                else:
                    g.old_rate.pop(0)
                    g.old_rate.append(g.last_ScaleRate)
    if g.scale_fix and len(frames) > 6:                                # :792
        for fhid in range(len(frames) - 2, 0, -1):
            p = frames[fhid].groundP
            if (p[0] == 0 and p[1] == 0 and p[2] == 0 and p[3] == 0) or p[3] == 0:
                continue
            back.last_ground = p.copy()
            break


def set_global_plane(frames, worldToCam1, max_frames=7):
    """-> (fixed, gplane float64[4], lgh float32) ; (False, None, None) when not fixed. worldToCam1: 3x4 [R|t] of window frame 1."""
    W = len(frames)
    if W < max_frames or W < 2:                                        # :1913
        return False, None, None
    sumnorm = 0.0
    lastpi = frames[W - 2].groundP.astype(np.float64)
    for i in range(W - 2, 0, -1):
        pi = lastpi
        lastpi = frames[i - 1].groundP.astype(np.float64)
        if pi[3] == 0 or np.isnan(pi).any() or abs(pi[1]) > 1:         # :1934
            return False, None, None
        d = pi - lastpi
        sq = 0.0
        with np.errstate(all="ignore"):
            for k in range(4):                                         # DEFINED: left to right in double
                sq = sq + d[k] * d[k]
            sumnorm += np.sqrt(sq)
    if not sumnorm < 0.2:                                              # :1944
        return False, None, None
    pih = frames[1].groundP.astype(np.float64)
    M = np.vstack([np.asarray(worldToCam1, np.float64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])
    piw = np.zeros(4)
    with np.errstate(all="ignore"):
        for j in range(4):                                             # piw = M^T pih, left to right
            s = M[0, j] * pih[0]
            s = s + M[1, j] * pih[1]
            s = s + M[2, j] * pih[2]
            s = s + M[3, j] * pih[3]
            piw[j] = s
    return True, piw, F(pih[3])                                        # :1970: float lgh = pih[3]


def local_scale(frame, lgh):
    """PlaneOptimize.cpp:203-211: float getlocalgh() / double local_plane[3]; None when !haveground"""
    if not frame.haveground:
        return None
    with np.errstate(all="ignore"):
        return float(np.float64(F(lgh)) / np.float64(frame.groundP[3]))

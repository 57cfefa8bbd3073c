"""Inputs of tests/test_ground_gpu.py, built without a device so that the cases can be checked against tests/ground_model.py on the CPU (test_ground_cpu.py)."""
import numpy as np

F = np.float32
COL = 32                                      # with cx = 32 every point of this pixel column back-projects to X = 0 exactly: fxi * 32 + cxi == 0 in float


def calib(w, h):
    return (0.6 * w, 0.6 * w, float(COL), 0.5 * h - 0.5)


def scene(w, h, specs, seed):
    """Mask clusters planted as vertical stripes over the legal columns [3, w - 2), column COL left out, in the order of `specs`; a spec with col = (y0, y1)
    is planted in column COL, rows [y0, y1). spec: n points, mask `value`, ny = the y component of the stripe's plane normal, sign of the
    inverse depths, zero = one zero inverse depth among them. A stripe's points lie on a plane of its own (+-2 mm along the normal), several may share a pixel. The input order is shuffled. -> dict(w, h, K, mask, u, v, idp)"""
    rng = np.random.RandomState(seed)
    K = calib(w, h)
    fx, fy, cx, cy = K
    mask = np.full((h, w), 1.0, F)
    stripes = [s for s in specs if "col" not in s]
    edges = np.linspace(3, w - 2, len(stripes) + 1).astype(int)
    U, V, ID = [], [], []
    k = 0
    for s in specs:
        n = s["n"]
        if "col" in s:
            y0, y1 = s["col"]
            x = np.full(n, COL)
            y = rng.randint(y0, y1, n)
            Z = rng.uniform(2.0, 4.0, n)
        else:
            x0, x1 = edges[k], edges[k + 1]
            mask[:, x0:x1] = s["value"]
            cols = np.array([c for c in range(x0, x1) if c != COL])
            x = cols[rng.randint(0, len(cols), n)]
            y = rng.randint(3, h - 2, n)
            nrm = np.array([0.1, s.get("ny", 0.2), 1.0]) / np.linalg.norm([0.1, 0.2, 1.0])
            ray = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones(n)], 1)
            Z = (3.0 + 0.3 * k + rng.uniform(-0.002, 0.002, n)) / (ray @ nrm)
            k += 1
        idp = s.get("sign", 1) / Z
        if s.get("zero"):
            idp[n // 2] = 0.0
        U.append(x + rng.uniform(0, 0.99, n)); V.append(y + rng.uniform(0, 0.99, n)); ID.append(idp)
    for s in specs:
        if "col" in s:
            mask[s["col"][0]:s["col"][1], COL] = s["value"]
    u, v, idp = np.concatenate(U).astype(F), np.concatenate(V).astype(F), np.concatenate(ID).astype(F)
    p = rng.permutation(len(u))
    return dict(w=w, h=h, K=K, mask=mask, u=u[p], v=v[p], idp=idp[p])


def S(n, value, **kw):
    return dict(n=n, value=float(value), **kw)


def score_scenes(w, h):
    """name -> (scene, draw seed, append)"""
    half = h // 2
    return {
        "sizes": (scene(w, h, [S(99, 255), S(100, 254), S(101, 253), S(130, 252)], 1), 1, 0),                  # n < 100, and the integer 100 / n: 1, 0
        "masks": (scene(w, h, [S(120, 199), S(121, 200), S(122, 255), S(123, 201)], 2), 2, 0),
        "negative": (scene(w, h, [S(110, 255, sign=-1), S(120, 254), S(130, 253), S(140, 252)], 3), 3, 0),     # mid_z < 0
        "zero_idepth": (scene(w, h, [S(150, 255, zero=True), S(120, 254), S(110, 253), S(105, 252)], 4), 4, 0),   # fitted, yet n_cloud != n
        "all_out": (scene(w, h, [S(50, 255), S(40, 254), S(30, 253), S(25, 252)], 5), 5, 0),                   # every score 9999999: the first wins
        "zero_mask_wins": (scene(w, h, [S(60, 0), S(50, 3), S(45, 5), S(40, 7)], 6), 6, 1),                    # chosen, and not appended (CoarseTracker.cpp:635)
        "three": (scene(w, h, [S(110, 255), S(120, 254), S(130, 253)], 7), 7, 0),                              # ran == 0
        "b_positive": (scene(w, h, [S(110, 255, ny=-0.2), S(120, 254, ny=-0.2), S(130, 253, ny=-0.2), S(140, 252, ny=-0.2)], 10), 0, 0),   # winners with b > 0
        "big": (scene(w, h, [S(1025, 255), S(120, 254), S(110, 253), S(105, 252)], 8), 8, 0),                  # the ordered sum over more than one 256-term round
        # two clusters in column COL: both planes are (+-1, +-0, +-0, +-0) exactly; when both normals come out as -1 the scores tie at -1000 and b == -0.0
        "column": (scene(w, h, [S(110, 250, col=(3, half)), S(105, 251, col=(half, h - 2)), S(120, 254), S(130, 253)], 9), 0, 0),
    }

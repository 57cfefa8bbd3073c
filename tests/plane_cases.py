"""Inputs of tests/test_plane_fit_gpu.py, built without a device so that the float64 floor of the model can be measured on them (test_plane_fit_cpu.py)."""
import numpy as np

F = np.float32
SIZES_SMALL = (1, 9, 10, 11, 63, 64, 65)
SIZES_ALL = (1, 9, 10, 11, 63, 64, 65, 255, 256, 257, 1025)


def calib(w, h):
    return (0.6 * w, 0.6 * w, 0.5 * w - 0.5, 0.5 * h - 0.5)


def stripe_scene(w, h, sizes, values, seed, extras=True, outlier_from=64):
    """len(sizes) vertical stripes, stripe k with mask value values[k] and sizes[k] points on a noisy plane of its own (+-2 mm along the normal, 30 % outliers
    from `outlier_from` points on), at random pixels of the stripe that pass the border test (several points may share a pixel). extras: points that fail the
    border test on every side, two points on a NaN mask pixel, and a zero inverse depth on the first member of every stripe with more than 11 points. The
    input order is shuffled. -> dict(w, h, K, mask, u, v, idp)"""
    rng = np.random.RandomState(seed)
    K = calib(w, h)
    fx, fy, cx, cy = K
    ns = len(sizes)
    sw = w // ns
    mask = np.zeros((h, w), F)
    nrm = np.array([0.1, 0.2, 1.0]) / np.linalg.norm([0.1, 0.2, 1.0])
    U, V, ID = [], [], []
    for k in range(ns):
        x0, x1 = k * sw, (w if k == ns - 1 else (k + 1) * sw)
        mask[:, x0:x1] = values[k]
        n = sizes[k]
        x = rng.randint(max(x0, 3), min(x1, w - 2), n)
        y = rng.randint(3, h - 2, n)
        ray = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones(n)], 1)
        Z = (3.0 + 0.3 * k + rng.uniform(-0.002, 0.002, n)) / (ray @ nrm)
        if n >= outlier_from:
            out = rng.rand(n) < 0.3
            Z[out] *= rng.uniform(0.5, 0.9, int(out.sum()))
        idp = 1.0 / Z
        if extras and n > 11:
            idp[0] = 0.0
        U.append(x + rng.uniform(0, 0.99, n)); V.append(y + rng.uniform(0, 0.99, n)); ID.append(idp)
    if extras:
        mask[5, 5] = np.nan
        U.append(np.array([5.3, 5.9, 2.9, 1.0, w - 2.0, w - 1.5, 10.0, 11.0, 12.0, 13.0, -4.0, 1e9]))
        V.append(np.array([5.6, 5.1, 10.0, 10.0, 10.0, 10.0, 2.5, h - 2.0, h - 1.2, 0.0, 10.0, 10.0]))
        ID.append(np.full(12, 0.3))
    u, v, idp = np.concatenate(U).astype(F), np.concatenate(V).astype(F), np.concatenate(ID).astype(F)
    p = rng.permutation(len(u))
    return dict(w=w, h=h, K=K, mask=mask, u=u[p], v=v[p], idp=idp[p])


def planted_scenes(w, h):
    """the cases of the planted-cloud test at one image size: name -> scene"""
    sizes = SIZES_SMALL if w < 100 else SIZES_ALL
    many = list(sizes) + [64, 10, 40, 40]                       # size ties: 64 and 10 twice, and the two halves of the zero region
    vals = [3.0 + k for k in range(len(sizes))] + [50.0, 51.0, 0.0, -0.0]
    s = {
        "one": stripe_scene(w, h, (300,), (5.0,), 1, extras=False),
        "three": stripe_scene(w, h, (40, 30, 20), (1.0, 2.0, 3.0), 2, extras=False),
        "many": stripe_scene(w, h, many, vals, 3),
        "four_ties": stripe_scene(w, h, (12, 12, 12, 12), (4.0, 1.0, 3.0, 2.0), 4),
    }
    out = stripe_scene(w, h, (30,), (7.0,), 5, extras=False)
    out["u"] = np.where(np.arange(30) % 2 == 0, F(1.5), F(w - 1.5)).astype(F)
    s["all_outside"] = out
    return s


def block_mask(w, h, nx, ny, values):
    """nx x ny rectangular regions"""
    mask = np.zeros((h, w), F)
    for j in range(ny):
        for i in range(nx):
            mask[j * h // ny:(j + 1) * h // ny, i * w // nx:(i + 1) * w // nx] = values[j * nx + i]
    return mask


def large_scene(w=1920, h=1072, n=160000, seed=11):
    """a 160 k-point cloud over 40 mask values (8 x 5 regions): region r on the plane n . P = 3 + 0.1 r, +-2 mm, 30 % outliers"""
    rng = np.random.RandomState(seed)
    K = calib(w, h)
    fx, fy, cx, cy = K
    values = [float(1 + 3 * r) for r in range(40)]
    mask = block_mask(w, h, 8, 5, values)
    x = rng.randint(0, w, n)
    y = rng.randint(0, h, n)
    reg = (y * 5 // h) * 8 + (x * 8 // w)
    nrm = np.array([0.1, 0.2, 1.0]) / np.linalg.norm([0.1, 0.2, 1.0])
    ray = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones(n)], 1)
    Z = (3.0 + 0.1 * reg + rng.uniform(-0.002, 0.002, n)) / (ray @ nrm)
    out = rng.rand(n) < 0.3
    Z[out] *= rng.uniform(0.5, 0.9, int(out.sum()))
    u = (x + rng.uniform(0, 0.99, n)).astype(F)
    v = (y + rng.uniform(0, 0.99, n)).astype(F)
    return dict(w=w, h=h, K=K, mask=mask, u=u, v=v, idp=(1.0 / Z).astype(F))


def six_region_mask(w, h):
    """six regions with colour 0 among them; the first touches the image border"""
    return block_mask(w, h, 3, 2, [0.0, 7.0, 3.0, 12.0, 5.0, 9.0])

"""The literal model of "The window replacement" in the TSDF section of include/nalo_gpu.h: the chain as a loop over tests/tsdf_replace_model.py's single
replacement (imported, not copied), with the per-pair counts and written_total, the voxels where any pair fired, each counted once. A pair is a dict(remove=,
add=, box=) of tests/tsdf_replace_model.py's sides. No device."""
import numpy as np

import tsdf_replace_model as rm

KEYS = ("removed", "reset", "added", "written")


def replace_n(vol, pairs, literal=False):
    """the pairs applied to vol one after the other, in order. Returns dict(pairs=[dict(removed, reset, added, written), ...], written_total, fired): fired
    the mask of the voxels some pair fired at (None with literal=True, the one-voxel-at-a-time form, which keeps no masks)"""
    nx, ny, nz = vol["dims"]
    fired = None if literal else np.zeros((nz, ny, nx), bool)
    rows = []
    for p in pairs:
        n = (rm.replace_literal if literal else rm.replace)(vol, p.get("remove"), p.get("add"), p.get("box"))
        rows.append({k: int(n[k]) for k in KEYS})
        if not literal:
            fired |= n["rem"] | n["add"]
    return dict(pairs=rows, written_total=None if literal else int(fired.sum()), fired=fired)


def order_case():
    """the planted case in which the ORDER of the list shows, on tests/test_tsdf_gpu.py's 33x17x5 grid with max_weight = 4: six coloured planes fused (weights up
    to 4, saturated in the middle, 1 at the rims), then pair 0 removes the fourth of them and pair 1 adds a seventh. At a voxel of weight 1 pair 0 resets and pair
    1 adds into the initial values, the other way round the add comes first and the removal leaves a mean; at a saturated voxel the list ends at weight 4, its
    reverse at 3. Returns (grid, fused, pairs): the grid as a dict, the six sides as side() argument tuples (depth, K, c2w, s, mn, mx, bgr), and the two pairs as
    dict(remove=tuple or None, add=tuple or None)"""
    from test_tsdf_cpu import pose, wavy_depth
    from test_tsdf_replace_cpu import H0, K0, POSES, W0
    grid = dict(origin=(-0.7, -0.5, 1.85), vs=0.055, dims=(33, 17, 5), trunc=0.2, mw=4.0)
    bgr = lambda seed: np.random.RandomState(seed).randint(0, 256, (H0, W0, 3)).astype(np.uint8)
    fused = [(wavy_depth(W0, H0, 10 + pi, base=2.0 + 0.02 * rnd), K0, POSES[pi], 1.0, 0.5, 3.5, bgr(60 + 3 * rnd + pi)) for rnd in range(2) for pi in range(3)]
    seventh = (wavy_depth(W0, H0, 19, base=2.03), K0, pose(0.05, -0.1, 0.05, (0.05, -0.02, 0.05)), 1.0, 0.5, 3.5, bgr(77))
    return grid, fused, [dict(remove=fused[3], add=None), dict(remove=None, add=seventh)]


def hull_n(vol, pairs):
    """what nalo_tsdf_last reports after nalo_tsdf_replace_depth_n: (lo, hi, visited) of the hull of every side's box, each pair's remove side cut by its box"""
    boxes = []
    for p in pairs:
        for sd, cut in ((p.get("remove"), p.get("box")), (p.get("add"), None)):
            if sd is None:
                continue
            lo, hi, v = rm.hull(vol, remove=sd, box=cut) if cut is not None else rm.hull(vol, add=sd)
            if v:
                boxes.append((lo, hi))
    if not boxes:
        return (0, 0, 0), (0, 0, 0), 0
    lo = tuple(min(b[0][a] for b in boxes) for a in range(3))
    hi = tuple(max(b[1][a] for b in boxes) for a in range(3))
    return lo, hi, (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])

"""tests/imm_carry_model.py (the literal loops of FullSystem.cpp:893-931 and :1677-1687, the frame drop as an erase) on hand-built vectors, with the expected
results written out by hand. No GPU."""
import numpy as np

import imm_carry_model as cm

OOB, GOOD = cm.OOB, cm.GOOD


def compact(vec):
    """:920-931 on one vector of names with None holes"""
    frames = [list(vec)]
    cm.activation_end(frames, [], [], [], [], [], [])
    return frames[0]


def test_swap_with_back_by_hand():
    a, b, c, d, e = "abcde"
    assert compact([a, None, c, d, None]) == [a, d, c]                        # b and e gone: the back e is null and is consumed by re-examining slot 1
    assert compact([a, None, c, None, None]) == [a, c]
    assert compact([None, None, None]) == []                                  # everything gone
    assert compact([a, b, c]) == [a, b, c]                                    # nothing gone
    assert compact([a]) == [a] and compact([None]) == [] and compact([]) == []
    assert compact([None, b, c, d, e]) == [e, b, c, d]
    assert compact([None, None, c, d, e]) == [e, d, c]
    assert compact([a, None, None, None, e, None, None]) == [a, e]            # a chain of null backs
    assert compact([None, b, None, d, None, "f"]) == ["f", b, d]


def test_fates_and_results_decide_who_leaves():
    # one host, seven points: fate -1, -2, -3 leave; 0, 2, 3 stay; the selected one follows its result
    host = [0] * 7
    status = [GOOD] * 7
    fate = [0, -1, 2, -2, 3, -3, 1]
    for res, want in ((1, [0, 4, 2]), (-1, [0, 4, 2]), (0, [0, 6, 2, 4])):
        src, nh = cm.carry(host, status, fate, [6], [res])
        assert src.tolist() == want and nh.tolist() == [0] * len(want)
    # result == 0: only a point the trace left OOB is deleted (:908)
    status[6] = OOB
    src, _ = cm.carry(host, status, fate, [6], [0])
    assert src.tolist() == [0, 4, 2]
    # OOB does not matter for a point that was not selected (fate 0 / 2 stay whatever their status)
    status = [OOB] * 7
    src, _ = cm.carry(host, status, [0, 2, 0, 2, 3, 0, 0], [], [])
    assert src.tolist() == list(range(7))


def test_hosts_interleaved_in_storage():
    # storage: h1 h0 h1 h0 h1 h0 h0; vectors: host 0 = [1, 3, 5, 6], host 1 = [0, 2, 4]
    host = [1, 0, 1, 0, 1, 0, 0]
    status = [GOOD] * 7
    src, nh = cm.carry(host, status, [0, -1, -1, 0, 0, 0, 0], [], [])
    assert src.tolist() == [6, 3, 5, 0, 4] and nh.tolist() == [0, 0, 0, 1, 1]   # host 0: [x, 3, 5, 6] -> [6, 3, 5]; host 1: [0, x, 4] -> [0, 4]
    # a host emptied, a host untouched
    src, nh = cm.carry(host, status, [-1, 0, -2, 0, -3, 0, 0], [], [])
    assert src.tolist() == [1, 3, 5, 6] and nh.tolist() == [0] * 4
    # a single point, kept and deleted
    assert cm.carry([0], [GOOD], [0], [], [])[0].tolist() == [0]
    assert cm.carry([0], [GOOD], [-1], [], [])[0].tolist() == []
    assert cm.carry([], [], [], [], [])[0].tolist() == []


def test_dropped_middle_host():
    host = [2, 0, 1, 2, 1, 0, 2]
    status = [GOOD] * 7
    src, nh = cm.carry(host, status, host_map=[0, -1, 1])
    assert src.tolist() == [1, 5, 0, 3, 6] and nh.tolist() == [0, 0, 1, 1, 1]
    # deletion first, then the drop: host 2 = [0, 3, 6] loses 0 -> [6, 3]
    src, nh = cm.carry(host, status, [-1, 0, 0, 0, 0, 0, 0], [], [], host_map=[0, -1, 1])
    assert src.tolist() == [1, 5, 6, 3] and nh.tolist() == [0, 0, 1, 1]
    # the first and the last host leave; a host without points is renumbered too
    src, nh = cm.carry(host, status, host_map=[-1, 0, -1, 1])
    assert src.tolist() == [2, 4] and nh.tolist() == [0, 0]


def test_append_bounds_and_nan():
    w, h = 12, 10
    # makeNewTraces walks 3 <= x < w - 4 = 8 and 3 <= y < h - 4 = 6
    px = [(2, 3), (3, 3), (7, 3), (8, 3), (5, 2), (5, 5), (5, 6), (3, 5), (7, 5)]
    idx = sorted(x + y * w for x, y in px)
    xy = [(i % w, i // w) for i in idx]
    status = [1 + (k % 3 == 0) + 2 * (k % 3 == 1) for k in range(len(idx))]
    app = dict(host=1, w=w, h=h, idx=idx, status=status, energy_finite=lambda k: True)
    src, nh = cm.carry([0, 0], [GOOD, GOOD], append=app)
    inside = [k for k, (x, y) in enumerate(xy) if 3 <= x < 8 and 3 <= y < 6]
    assert [xy[k] for k in inside] == [(3, 3), (7, 3), (3, 5), (5, 5), (7, 5)]
    assert src.tolist() == [0, 1] + [-(k + 2) for k in inside] and nh.tolist() == [0, 0] + [1] * 5
    # a point whose energyTH is not finite is deleted; the ones behind it keep their order
    app["energy_finite"] = lambda k: xy[k] != (7, 3)
    src, _ = cm.carry([0, 0], [GOOD, GOOD], append=app)
    assert src.tolist() == [0, 1] + [-(k + 2) for k in inside if xy[k] != (7, 3)]
    # appended behind the carried points of the same host, hosts after it move back; all three parts in one call
    app["host"], app["energy_finite"] = 0, lambda k: True
    src, nh = cm.carry([1, 2, 1, 0], [GOOD] * 4, [0, 0, -1, 0], [], [], host_map=[-1, 0, 1], append=app)
    assert src.tolist() == [0] + [-(k + 2) for k in inside] + [1] and nh.tolist() == [0] * 6 + [1]
    # status 0 entries are not selected
    app["status"] = [0] * len(idx)
    assert cm.carry([], [], append=app)[0].tolist() == []


def test_apply_builds_the_new_arrays():
    old = {f: np.arange(3, dtype=np.float32) for f in cm.FIELDS}
    old["host_idx"] = np.int32([0, 1, 1]); old["status"] = np.int32([0, 1, 2])
    old["color"] = old["weights"] = np.arange(24, dtype=np.float32).reshape(3, 8)
    old["gradH"] = np.arange(9, dtype=np.float32).reshape(3, 3); old["lastUV"] = np.arange(6, dtype=np.float32).reshape(3, 2)
    z8 = np.zeros(8, np.float32)
    out = cm.apply([2, -2], [0, 1], old, lambda k: cm.fresh_record(5, 6, 1, 4, z8, z8, np.zeros(3, np.float32), np.float32(7)))
    assert out["u"].tolist() == [2, 5] and out["host_idx"].tolist() == [0, 1] and out["status"].tolist() == [2, cm.UNINITIALIZED]
    assert out["color"][0].tolist() == list(range(16, 24)) and np.isnan(out["idmax"][1]) and out["my_type"].tolist() == [2, 4]
    assert out["lastUV"].tolist() == [[4, 5], [-1, -1]] and out["quality"].tolist() == [2, 10000]


def test_closed_form_of_the_kernels_equals_the_loop():
    """kernels_imm_carry.hip does not run the loop: with p a point's rank in its host's vector, kb the kept points before it and m the host's kept points, a kept
    point below m stays, the kept point at p >= m goes to the hole of index m - 1 - kb, and the hole at q has index q - kb(q). Restated here in NumPy and
    compared with the literal loop on random vectors (dropped hosts included)."""
    rng = np.random.RandomState(0)
    for trial in range(1500):
        n, H = rng.randint(0, 60), rng.randint(1, 5)
        host = rng.randint(0, H, n)
        keep = rng.rand(n) < rng.rand()
        hm = None
        if trial % 2:
            drop = rng.rand(H) < 0.3
            hm = np.full(H, -1)
            hm[~drop] = np.arange((~drop).sum())
        src, _ = cm.carry(host, np.zeros(n, int), np.where(keep, 0, -1), [], [], hm)
        kept = keep & ((np.arange(H) if hm is None else hm)[host] >= 0)
        want = []
        for h in range(H):
            idx = np.nonzero(host == h)[0]
            k = kept[idx]
            m, kb = int(k.sum()), np.cumsum(k) - k
            slot, mover = [None] * m, {}
            for p, i in enumerate(idx):
                if k[p] and p < m:
                    slot[p] = i
                elif k[p]:
                    mover[m - 1 - kb[p]] = i
            for p in range(min(m, len(idx))):
                if not k[p]:
                    slot[p] = mover[p - kb[p]]
            want += slot
        assert src.tolist() == want, trial

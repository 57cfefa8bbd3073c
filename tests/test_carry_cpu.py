"""tests/carry_model.py on hand-built windows: the semantics nalo_ba_carry_window is held to (tests/test_ba_carry_gpu.py), worked out by hand from the reference
lines the model cites. No device."""
import numpy as np

import carry_model as cm
import lifecycle_model as lm

N = -1            # no residual


def window():
    """five frames, six points; frame 1 hosts only an invalid point, frame 2 hosts none"""
    host = np.array([0, 0, 1, 3, 3, 4], np.int32)
    valid = np.array([1, 1, 0, 1, 1, 1], bool)
    st = np.array([[N, 0, 0, N, 2],       # p0: residuals to 1, 2, 4
                   [N, 0, N, N, N],       # p1: its only residual targets frame 1
                   [0, N, 0, 0, 0],       # p2: removed earlier
                   [0, N, N, N, 1],       # p3
                   [N, N, 0, N, N],       # p4: its only residual targets frame 2
                   [0, 0, 0, 0, N]], np.int8)
    ng = np.array([7, 0, 9, 3, 1, 20], np.int32)
    lt = np.array([[4, 2], [1, -1], [4, 3], [-1, 0], [2, -1], [3, 2]], np.int8)
    ls = np.array([[2, 0], [0, 1], [0, 0], [1, 0], [0, 1], [0, 0]], np.int8)
    return host, valid, st, (ng, lt, ls)


def test_frames_leave_and_one_enters():
    host, valid, st, (ng, lt, ls) = window()
    # frames 1 and 2 leave, one after the other: the history's targets are remapped by each marginalizeFrame, before the carry sees them
    lt = lm.remap_at_frame_marginalization(lt, 1)
    lt = lm.remap_at_frame_marginalization(lt, 1)            # old frame 2 is index 1 once frame 1 has gone
    m = cm.carry(host, valid, st, (ng, lt, ls), rows=[0, 3, 4], entering=True)
    assert m["old_p"].tolist() == [0, 1, 3, 4, 5]            # old order, dense
    assert m["host"].tolist() == [0, 0, 1, 1, 2]
    assert m["exists"].tolist() == [[0, 0, 1, 1],            # p0 keeps the residual to old frame 4, gets the new one
                                    [0, 0, 0, 1],            # p1 and p4: only residuals to leaving frames: all that is left is the new one
                                    [1, 0, 1, 1],
                                    [0, 0, 0, 1],
                                    [1, 1, 0, 1]]
    g, t, s = m["hist"]
    assert g.tolist() == [7, 0, 3, 1, 20]
    assert t.tolist() == [[3, 2], [3, -1], [3, -1], [3, -1], [3, 1]]     # [1] = the old [0] in the NEW indices (4 -> 2, 1 and 2 -> null, 3 -> 1), [0] = the new frame
    assert s.tolist() == [[0, 2], [0, 0], [0, 1], [0, 0], [0, 0]]        # [1] takes the old [0]'s state whatever its pointer was; [0] is IN


def test_last_target_null_before_the_shift():
    host, valid, st, hist = window()
    assert hist[1][3, 0] == -1 and hist[2][3, 0] == lm.OOB
    m = cm.carry(host, valid, st, hist, rows=[0, 1, 2, 3, 4], entering=True)
    i = m["old_p"].tolist().index(3)
    assert m["hist"][1][i].tolist() == [5, -1] and m["hist"][2][i].tolist() == [lm.IN, lm.OOB]      # the null pointer and its state move to [1]
    assert (m["exists"][:, 5] == 1).all() and m["exists"].shape == (5, 6)
    assert np.array_equal(m["exists"][:, :5], (st[valid] >= 0).astype(np.uint8))


def test_no_frame_enters():
    host, valid, st, (ng, lt, ls) = window()
    lt1 = lm.remap_at_frame_marginalization(lt, 2)
    m = cm.carry(host, valid, st, (ng, lt1, ls), rows=[0, 1, 3, 4], entering=False)
    assert m["exists"].shape == (5, 4) and m["host"].tolist() == [0, 0, 2, 2, 3]
    assert m["exists"][3].sum() == 0                           # p4 has no residual left; it stays a point until somebody flags it
    assert np.array_equal(m["hist"][1], lt1[valid]) and np.array_equal(m["hist"][2], ls[valid]) and np.array_equal(m["hist"][0], ng[valid])
    n = cm.carry(host, valid, st, None, rows=[0, 1, 3, 4], entering=False)
    assert n["hist"] is None and np.array_equal(n["exists"], m["exists"])


def test_insertion_takes_result_one_only_and_builds_the_default_history():
    host, valid, st, hist = window()
    win = cm.carry(host, valid, st, hist, rows=[0, 1, 2, 3, 4], entering=False)
    W = 5
    imm_host = np.array([4, 0, 2, 2, 1, 3, 0], np.int32)
    sel = np.array([6, 1, 4, 2, 5], np.int32)                  # toOptimize order
    result = np.array([1, 0, 1, -1, 1], np.int32)
    res_in = np.array([[0, 1, 1, 1, 1],                        # both newest frames
                       [1, 1, 1, 1, 1],                        # result 0: not inserted, whatever its rows say
                       [1, 0, 1, 0, 1],                        # without the second-newest frame
                       [1, 1, 1, 1, 1],                        # result -1
                       [1, 1, 1, 0, 0]], np.uint8)             # without both
    m = cm.insert(win, result, res_in, imm_host, sel)
    assert m["old_p"].tolist() == win["old_p"].tolist() + [-1, -3, -5]
    assert m["from_k"].tolist() == [-1] * 5 + [0, 2, 4]
    assert m["host"].tolist() == win["host"].tolist() + [0, 1, 3]
    assert np.array_equal(m["exists"][:5], win["exists"]) and np.array_equal(m["exists"][5:], res_in[[0, 2, 4]])
    g, t, s = m["hist"]
    assert np.array_equal(g[:5], win["hist"][0]) and np.array_equal(t[:5], win["hist"][1]) and np.array_equal(s[:5], win["hist"][2])
    assert g[5:].tolist() == [0, 0, 0]
    assert t[5:].tolist() == [[W - 1, W - 2], [W - 1, -1], [-1, -1]]
    assert s[5:].tolist() == [[lm.IN, lm.IN], [lm.IN, lm.OOB], [lm.OOB, lm.OOB]]
    # the same defaults as the model of nalo_ba_set_point_history's NULL form
    d = lm.default_history(res_in[[0, 2, 4]])
    assert np.array_equal(d[1], t[5:]) and np.array_equal(d[2], s[5:])
    # a window without a history stays without one
    assert cm.insert(cm.carry(host, valid, st, None, rows=[0, 1, 2, 3, 4], entering=False), result, res_in, imm_host, sel)["hist"] is None


def test_prior_extension_is_a_zero_block():
    H, b = np.arange(144.0).reshape(12, 12), np.arange(12.0)
    H2, b2 = cm.extend_prior(H, b)
    assert H2.shape == (20, 20) and np.array_equal(H2[:12, :12], H) and not H2[12:].any() and not H2[:, 12:].any() and np.array_equal(b2[:12], b) and not b2[12:].any()

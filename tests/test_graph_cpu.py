"""tests/graph_model.py - the model tests/test_graph_gpu.py holds nalo_map_graph / nalo_map_graph_connections against - on a hand-built session. Every
entry and every connection below is worked out by hand from the four events of EnergyFunctional::connectivityMap and from publishGraph's walk.

The session (frame ids chosen out of order, so that window order and key order differ):
  frames 5 and 3 enter; points a, b, c of host 5 get a residual to 3, points d, e of host 3 one to 5; a fix pass removes c -> 3
  frame 7 enters; a, b, d, e get a residual to it
  a is marginalised with a -> 3 active and a -> 7 inactive, then removed
  frame 3 leaves from the middle of [5, 3, 7]: d is marginalised (both residuals active) and removed, e is dropped, b -> 3 is dropped with the frame
  frame 8 enters; b gets a residual to it, a new point f of host 7 one to 5 and one to 8"""
import numpy as np

import graph_model as gm


def session(upto):
    g = gm.Graph()
    g.insert_frame(5)
    g.insert_frame(3)
    if upto == "two frames":
        return g
    for _ in "abc":
        g.insert_residual(5, 3)
    for _ in "de":
        g.insert_residual(3, 5)
    g.drop_residual(5, 3)                                   # c -> 3, linearizeAll(true)
    if upto == "residuals":
        return g
    g.insert_frame(7)
    for h in (5, 5, 3, 3):
        g.insert_residual(h, 7)
    g.marginalize(5, 3)                                     # a -> 3 is active, a -> 7 is not
    g.drop_residual(5, 3); g.drop_residual(5, 7)            # removePoint(a)
    if upto == "a point marginalised":
        return g
    g.marginalize(3, 5); g.marginalize(3, 7)                # d
    g.drop_residual(3, 5); g.drop_residual(3, 7)            # removePoint(d)
    g.drop_residual(3, 5); g.drop_residual(3, 7)            # e: dropped, not marginalised
    g.drop_residual(5, 3)                                   # b -> 3: FullSystem::marginalizeFrame
    g.frame_leaves(3)
    if upto == "a frame left":
        return g
    g.insert_frame(8)
    g.insert_residual(5, 8)                                 # b
    g.insert_residual(7, 5); g.insert_residual(7, 8)        # f
    return g


def test_two_frames_enter():
    g = session("two frames")
    assert g.entries() == [(3, 3, 0, 0), (3, 5, 0, 0), (5, 3, 0, 0), (5, 5, 0, 0)]
    assert g.connections() == [(3, 5, 0, 0, 0, 0)]


def test_residuals_are_inserted_and_dropped():
    g = session("residuals")
    assert g.entries() == [(3, 3, 0, 0), (3, 5, 2, 0), (5, 3, 2, 0), (5, 5, 0, 0)]
    assert g.connections() == [(3, 5, 2, 2, 0, 0)]


def test_a_point_is_marginalised_with_one_inactive_residual():
    g = session("a point marginalised")
    assert g.entries() == [(3, 3, 0, 0), (3, 5, 2, 0), (3, 7, 2, 0), (5, 3, 1, 1), (5, 5, 0, 0), (5, 7, 1, 0), (7, 3, 0, 0), (7, 5, 0, 0), (7, 7, 0, 0)]
    # (from, to, fwdAct, bwdAct, fwdMarg, bwdMarg): the one marginalised residual is 5 -> 3, the BACKWARD direction of connection 3 - 5
    assert g.connections() == [(3, 5, 2, 1, 0, 1), (3, 7, 2, 0, 0, 0), (5, 7, 1, 0, 0, 0)]


def test_a_frame_leaves_from_the_middle():
    g = session("a frame left")
    assert g.window == [5, 7]
    e = g.entries()
    assert len(e) == 9                                      # nothing is erased
    assert e == [(3, 3, 0, 0), (3, 5, 0, 1), (3, 7, 0, 1), (5, 3, 0, 1), (5, 5, 0, 0), (5, 7, 1, 0), (7, 3, 0, 0), (7, 5, 0, 0), (7, 7, 0, 0)]
    assert all(x[2] == 0 for x in e if 3 in x[:2])          # every pair with the departed frame holds no residual, and keeps its marg
    assert g.connections() == [(3, 5, 0, 0, 1, 1), (3, 7, 0, 0, 1, 0), (5, 7, 1, 0, 0, 0)]


def test_a_third_frame_enters():
    g = session("all")
    assert g.window == [5, 7, 8]
    assert g.entries() == [(3, 3, 0, 0), (3, 5, 0, 1), (3, 7, 0, 1), (5, 3, 0, 1), (5, 5, 0, 0), (5, 7, 1, 0), (5, 8, 1, 0), (7, 3, 0, 0), (7, 5, 1, 0), (7, 7, 0, 0),
                           (7, 8, 1, 0), (8, 5, 0, 0), (8, 7, 0, 0), (8, 8, 0, 0)]      # 9 + 5: the new frame pairs with the window's frames only, not with 3
    assert g.connections() == [(3, 5, 0, 0, 1, 1), (3, 7, 0, 0, 1, 0), (5, 7, 1, 1, 0, 0), (5, 8, 1, 0, 0, 0), (7, 8, 1, 0, 0, 0)]


def test_the_read_back_helpers():
    g = session("residuals")
    g.set_live(5, 3, 7); g.set_live(3, 5, 0); g.set_live(5, 5, 0)
    assert g.entries() == [(3, 3, 0, 0), (3, 5, 0, 0), (5, 3, 7, 0), (5, 5, 0, 0)]
    state = np.array([[-1, 0, 2], [-1, -1, 1], [0, -1, -1], [-1, -1, -1]], np.int8)       # IN 0, OOB 1, OUTLIER 2 all exist
    assert gm.live_counts([0, 0, 1, 2], state, 3).tolist() == [[0, 1, 2], [1, 0, 0], [0, 0, 0]]
    assert gm.key(3, 5) == 3 * 2 ** 32 + 5 and gm.key(0, 0) == 0

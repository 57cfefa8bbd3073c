"""A literal model of EnergyFunctional::connectivityMap (the argument of Output3DWrapper::publishGraph) and of the walk PangolinDSOViewer::publishGraph makes
over it. The map is a dict keyed like the reference's, (host frameID << 32) + target frameID, with the value [act, marg] = Eigen::Vector2i [0], [1].

Four events touch the map (OptimizationBackend/EnergyFunctional.cpp):
  insert_frame      insertFrame, :453-458     (new, f2) and (f2, new) = {0, 0} for every frame f2 then in the window, the new one included
  insert_residual   insertResidual, :423      [0]++
  drop_residual     dropResidual, :493        [0]--
  marginalize       marginalizePointsF, :633  [1]++ for an active residual of a PS_MARGINALIZE point
Entries are never erased."""
import numpy as np


def key(host_id, target_id):
    assert host_id >= 0 and target_id >= 0
    return (int(host_id) << 32) + int(target_id)


class Graph:
    def __init__(self):
        self.m = {}
        self.window = []                                   # frame ids of EnergyFunctional::frames

    # ---- the four events
    def insert_frame(self, new_id):
        self.window.append(new_id)
        for f2 in self.window:
            self.m[key(new_id, f2)] = [0, 0]
            if f2 != new_id:
                self.m[key(f2, new_id)] = [0, 0]

    def insert_residual(self, host_id, target_id, n=1):
        self.m[key(host_id, target_id)][0] += n

    def drop_residual(self, host_id, target_id, n=1):
        self.m[key(host_id, target_id)][0] -= n

    def marginalize(self, host_id, target_id, n=1):
        self.m[key(host_id, target_id)][1] += n

    # ---- what is not an event of the map itself
    def frame_leaves(self, frame_id):
        """EnergyFunctional::marginalizeFrame: the frame leaves `frames`; the map keeps its entries (FullSystem::marginalizeFrame has dropped every residual
        that targets it, and its own points were removed before: the caller issues those drops)"""
        self.window.remove(frame_id)

    def set_live(self, host_id, target_id, n):
        """insert_residual / drop_residual until the pair holds n residuals (a model driven by read-backs sees counts, not objects)"""
        d = n - self.m[key(host_id, target_id)][0]
        if d > 0:
            self.insert_residual(host_id, target_id, d)
        elif d < 0:
            self.drop_residual(host_id, target_id, -d)

    # ---- the two output forms
    def entries(self):
        """every entry in std::map's iteration order -> [(host_id, target_id, act, marg)]"""
        return [(k >> 32, k & 0xFFFFFFFF, v[0], v[1]) for k, v in sorted(self.m.items())]

    def connections(self):
        """PangolinDSOViewer::publishGraph (IOWrapper/Pangolin/PangolinDSOViewer.cpp:528-571) -> [(from, to, fwdAct, bwdAct, fwdMarg, bwdMarg)], runningID = len"""
        out = []
        for k, v in sorted(self.m.items()):
            host, target = k >> 32, k & 0xFFFFFFFF
            if host == target:
                assert v == [0, 0]
                continue
            if host > target:
                continue
            st = self.m[key(target, host)]                 # connectivity.at(inverseKey)
            out.append((host, target, v[0], st[0], v[1], st[1]))
        return out


def live_counts(host, state, W):
    """residual objects per (host index, target index) of a window from the read-backs: state [P][W] with -1 = no residual -> [W][W]"""
    out = np.zeros((W, W), np.int64)
    ex = np.asarray(state) >= 0
    for h in range(W):
        out[h] = ex[np.asarray(host) == h].sum(0)
    return out

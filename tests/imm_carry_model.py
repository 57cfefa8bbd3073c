"""Literal model of what happens to the immature points of a window across one keyframe (reference paths relative to src/FullSystem/):

  (A) activatePointsMT, FullSystem.cpp:805-876 as it ends for the immature set (a deleted point leaves a null in its host's vector), step 4 :893-917 and
      the compaction :920-931, the loops written as the reference writes them;
  (C) a frame leaves the window: it is erased from frameHessians and its ImmaturePoints go with it (HessianBlocks.cpp:117);
  (B) makeNewTraces, FullSystem.cpp:1677-1687: the raster walk over the selection map inside the pattern padding.

Every frame is a Python list (FrameHessian::immaturePoints) of point ids with None for a null pointer. A carried point's id is its index in the old resident
set, an appended point's id is -(k + 2) for entry k of the append list: exactly what nalo_imm_resident_carry_map returns. No closed form is used anywhere."""
import numpy as np

GOOD, OOB, OUTLIER, SKIPPED, BADCONDITION, UNINITIALIZED = range(6)
PATTERN_PADDING = 2                                                            # util/settings.h: patternPadding
FIELDS = ("u", "v", "color", "weights", "gradH", "energyTH", "host_idx", "idmin", "idmax", "status", "quality", "lastUV", "interval", "my_type")


def vectors(host_idx, n_hosts):
    """frameHessians[h]->immaturePoints: a host's points in ascending resident index; idx_in[i] = ImmaturePoint::idxInImmaturePoints"""
    frames = [[] for _ in range(n_hosts)]
    idx_in = []
    for i, h in enumerate(host_idx):
        idx_in.append(len(frames[h]))
        frames[h].append(i)
    return frames, idx_in


def activation_end(frames, idx_in, host_idx, status, fate, sel, result):
    """what activatePointsMT leaves of the immature vectors, given the selection loop's fates and optimizeImmaturePoint's verdicts"""
    for i, f in enumerate(fate):                                              # :820-826, :840-851, :870-874: delete ph; host->immaturePoints[i] = 0
        if f in (-1, -2, -3):
            frames[host_idx[i]][idx_in[i]] = None
    for k in range(len(sel)):                                                  # :893-917
        ph = sel[k]
        newpoint = result[k]                                                   # 1: a PointHessian, -1: (PointHessian*)((long)(-1)), 0: null
        if newpoint != 0 and newpoint != -1:
            frames[host_idx[ph]][idx_in[ph]] = None                            # :900 (the point lives on as a PointHessian)
        elif newpoint == -1 or status[ph] == OOB:
            frames[host_idx[ph]][idx_in[ph]] = None                            # :910
        else:
            assert newpoint == 0 or newpoint == -1                             # :915
    for host in frames:                                                        # :920-931
        i = 0
        while i < len(host):
            if host[i] is None:
                host[i] = host[-1]
                host.pop()
                i -= 1
            i += 1


def drop_frames(frames, host_map):
    """frames with host_map[h] == -1 are erased; the survivors' positions must be what host_map names"""
    for h in reversed(range(len(host_map))):
        if host_map[h] == -1:
            del frames[h]
    kept = [m for m in host_map if m != -1]
    assert kept == list(range(len(frames))), "host_map's kept entries must be 0 .. W_new-1 in increasing order"


def make_new_traces(frames, append_host, selection_map, entry_of, energy_finite, w, h):
    """:1677-1687. selection_map [h, w] (0: not selected), entry_of[y, x] = the list entry of that pixel, energy_finite(k) = std::isfinite(impt->energyTH)"""
    while len(frames) <= append_host:
        frames.append([])
    new_frame = frames[append_host]
    for y in range(PATTERN_PADDING + 1, h - PATTERN_PADDING - 2):
        for x in range(PATTERN_PADDING + 1, w - PATTERN_PADDING - 2):
            if selection_map[y, x] == 0:
                continue
            k = int(entry_of[y, x])
            if not energy_finite(k):
                continue                                                       # delete impt
            new_frame.append(-(k + 2))


def carry(host_idx, status, fate=None, sel=None, result=None, host_map=None, append=None):
    """-> (src, new_host): per point of the new set its id and its new host index, frames in order, every frame's vector front to back.
    append = dict(host, w, h, idx, status, energy_finite): the append list (idx = x + y*w; raster order, as the selector gives it)"""
    host_idx = [int(x) for x in host_idx]
    n_hosts = len(host_map) if host_map is not None else (max(host_idx) + 1 if host_idx else 0)
    frames, idx_in = vectors(host_idx, n_hosts)
    if fate is not None:
        activation_end(frames, idx_in, host_idx, status, fate, [] if sel is None else sel, result)
    if host_map is not None:
        drop_frames(frames, [int(m) for m in host_map])
    if append is not None:
        w, h = append["w"], append["h"]
        smap, entry = np.zeros((h, w), np.uint8), np.full((h, w), -1, np.int64)
        idx = np.asarray(append["idx"], np.int64)
        assert len(set(idx.tolist())) == len(idx)
        smap.reshape(-1)[idx] = append["status"]
        entry.reshape(-1)[idx] = np.arange(len(idx))
        make_new_traces(frames, append["host"], smap, entry, append["energy_finite"], w, h)
    src = [p for f in frames for p in f]
    new_host = [hn for hn, f in enumerate(frames) for _ in f]
    return np.asarray(src, np.int64), np.asarray(new_host, np.int32)


def fresh_record(x, y, host, my_type, color, weights, gradH, energyTH):
    """the ImmaturePoint constructor's members (ImmaturePoint.cpp:32-60) around the pattern values"""
    return dict(u=np.float32(x), v=np.float32(y), color=color, weights=weights, gradH=gradH, energyTH=energyTH, host_idx=np.int32(host), idmin=np.float32(0),
                idmax=np.float32(np.nan), status=np.int32(UNINITIALIZED), quality=np.float32(10000), lastUV=np.full(2, -1, np.float32), interval=np.float32(0),
                my_type=np.float32(my_type))


def apply(src, new_host, old, fresh):
    """the new set's arrays: old = {field: array} of the old set, fresh(k) = fresh_record of append entry k"""
    src = np.asarray(src, np.int64)
    n = len(src)
    out = {f: np.zeros((n,) + np.asarray(old[f]).shape[1:], np.asarray(old[f]).dtype) for f in FIELDS}
    carried = src >= 0
    for f in FIELDS:
        out[f][carried] = np.asarray(old[f])[src[carried]]
    out["host_idx"][carried] = np.asarray(new_host)[carried]
    for j in np.nonzero(~carried)[0]:
        rec = fresh(-(int(src[j]) + 2))
        assert rec["host_idx"] == new_host[j]
        for f in FIELDS:
            out[f][j] = rec[f]
    return out

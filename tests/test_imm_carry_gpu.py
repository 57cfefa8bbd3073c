"""nalo_imm_resident_carry - the resident immature set across a keyframe, on the device - against the literal model of tests/imm_carry_model.py.

The comparison is the same everywhere (carry_and_compare): the full state before (nalo_imm_resident_get_points + nalo_imm_resident_get), the model on it, the
call, the full state after. All 31 words of every point must be equal BIT FOR BIT (floats are compared as uint32, NaNs included), and so must
nalo_imm_resident_carry_map, the counts of nalo_imm_resident_carry_last and the largest host index as nalo_imm_resident_trace sees it. What the inputs reach is
asserted on the MODEL's output before the device is asked.

  planted       noise images, hand-built fates, hosts interleaved in storage: n = 1, 255, 256, 257, 513 with 4 and 16 hosts; a host emptied; a host whose last
                points are all holes (the null-back chain); every host untouched; n_new = 0; every combination of the parts A, B, C in one call
  real shape    test_imm_large_gpu.Case("K"), 1224x368, W = 8: the whole seam of a keyframe, then the next activation and insertion on the carried set
  NaN           an explicit append list on a frame with one +inf texel: the constructor's `delete impt` branch, checked on the CPU with the oracle first
  scale         160 000 points over 8 hosts, 30 % removed at random, one host dropped
  repeat        two keyframes in a row on one context. (The context does not expose its buffer capacities, so that the second call allocates nothing is not
                asserted here; the call sizes its buffers with half as much again as the first set needs.)
  refusals      every refusal of the header; the set is unchanged after each and the context stays usable

The host copies the call rebuilds (u | v and host_idx of every point, which give an inserted point its host and its slot key in nalo_ba_carry_window) are not
readable, so the real shape runs two contexts: A carries its set through two keyframes, B makes the same window calls and is GIVEN A's read-back set where A
carries. After the next trace both hold the same 31 words per point, and the same activation and insertion must leave the same window bit for bit - launch
configuration, points, residual states, history, the linearised and solved system, every residual's centre projection - once for carried points whose index and
host both carries changed, once for points the carry appended."""
import types

import numpy as np
import pytest

import activation_model as am
import imm_carry_model as cm
import orc
from imm_helpers import host_to_new
from nalo_slam_amd import binding, synth

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -4
OOB = cm.OOB


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def full_state(c):
    """{field: array} of the resident set: all 31 words of every point"""
    p = c.imm_resident_get_points()
    idmin, idmax, status, quality, uv, li = c.imm_resident_get() if len(p["u"]) else (np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32),
                                                                                       np.zeros(0, np.float32), np.zeros((0, 2), np.float32), np.zeros(0, np.float32))
    p.update(idmin=idmin, idmax=idmax, status=status, quality=quality, lastUV=uv, interval=li)
    assert set(p) == set(cm.FIELDS)
    return p


def assert_same_state(got, want, what):
    for f in cm.FIELDS:
        assert got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
        assert np.array_equal(bits(got[f]), bits(want[f])), (what, f, int((bits(got[f]) != bits(want[f])).sum()))


def fresh_from_create(c, slot, w, host, idx, status):
    """fresh(k) for the model + energy_finite(k), from nalo_imm_create on the entries makeNewTraces' bounds admit (it refuses the others)"""
    idx, status = np.asarray(idx, np.int64), np.asarray(status)
    x, y = idx % w, idx // w
    ok = (x >= 3) & (x < w - 4) & (y >= 3) & (y < c.h - 4) & (status != 0)
    pos = np.full(len(idx), -1)
    pos[ok] = np.arange(ok.sum())
    color, weights, gradH, eth = c.imm_create(slot, x[ok].astype(np.int32), y[ok].astype(np.int32))

    def fresh(k):
        q = pos[k]
        assert q >= 0
        return cm.fresh_record(x[k], y[k], host, status[k], color[q], weights[q], gradH[q], eth[q])
    return fresh, (lambda k: bool(np.isfinite(eth[pos[k]]))), (color, weights, gradH, eth, ok)


def carry_and_compare(c, what, fate=None, sel=None, result=None, host_map=None, append=None, expect=None, probe_trace=True):
    """append = dict(slot, host, idx, status[, explicit]): explicit=False takes the selector's last map on the device (idx / status = nalo_pixsel_get_selected).
    expect(src, new_host, before): assertions on the model's output, run before the device is asked. -> (src, new_host, before, after)"""
    before = full_state(c)
    n = len(before["u"])
    app_m, fresh = None, None
    if append is not None:
        fresh, finite, _ = fresh_from_create(c, append["slot"], c.w, append["host"], append["idx"], append["status"])
        app_m = dict(host=append["host"], w=c.w, h=c.h, idx=append["idx"], status=append["status"], energy_finite=finite)
    src, new_host = cm.carry(before["host_idx"], before["status"], fate, sel, result, host_map, app_m)
    want = cm.apply(src, new_host, before, fresh)
    if expect is not None:
        expect(src, new_host, before)
    kw = dict(fate=fate, sel=sel, result=result, host_map=host_map)
    if append is not None:
        kw.update(append_slot=append["slot"], append_host=append["host"])
        if append.get("explicit", True):
            kw.update(append_idx=append["idx"], append_status=append["status"])
    st = c.imm_resident_carry(**kw)
    after = full_state(c)
    assert_same_state(after, want, what)
    assert np.array_equal(c.imm_resident_carry_map(), src), what
    n_new = len(src)
    dropped = 0 if host_map is None else int((np.asarray(host_map)[before["host_idx"][deleted_by_a(before, fate, sel, result) == 0]] < 0).sum())
    n_del = int(deleted_by_a(before, fate, sel, result).sum())
    assert st[:4] == (n_new, n_del, dropped, int((src < 0).sum())), (what, st[:4])
    assert n_new == n - n_del - dropped + int((src < 0).sum())
    assert st[4].tolist() == np.bincount(new_host, minlength=16).tolist(), what
    if n_new and probe_trace:
        # the largest host index, as the trace's range check sees it: max rows are refused, max + 1 accepted. (The accepted trace runs, with zero matrices: it
        # changes the state behind `after`. The real shape traces with real matrices instead.)
        mx = int(new_host.max())
        if mx >= 1:
            z = np.zeros((mx, 9), np.float32)
            with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_ARG):
                c.imm_resident_trace(0, z, z[:, :3], z[:, :2])
        z = np.zeros((mx + 1, 9), np.float32)
        c.imm_resident_trace(0, z, z[:, :3], z[:, :2])
        c.sync()
    return src, new_host, before, after


def deleted_by_a(before, fate, sel, result):
    """1 for every point part (A) removes (the rule of the header, for the counts only; the order comes from the model)"""
    n = len(before["u"])
    d = np.zeros(n, np.int32)
    if fate is None:
        return d
    d[np.asarray(fate) < 0] = 1
    for k, i in enumerate(sel):
        d[i] = 1 if (result[k] != 0 or before["status"][i] == OOB) else 0
    return d


# ---------------------------------------------------------------------------------------------------------------- planted sets
PW, PH = 96, 64


class Planted:
    def __init__(self):
        self.c = binding.Context(PW, PH, (80.0, 80.0, PW / 2 - 0.5, PH / 2 - 0.5), n_slots=3, levels=3)      # three levels: the selector's
        rng = np.random.RandomState(5)
        self.img = (100 + 50 * rng.rand(PH, PW)).astype(np.float32)
        for s in range(2):                                                     # slot 2 never gets a pyramid
            self.c.frame_upload(s, self.img if s else np.full((PH, PW), 100, np.float32))

    def resident(self, n, W, seed, host=None):
        """n points with random words (NaNs and arbitrary statuses among them), hosts interleaved in storage. lastTraceUV / lastTracePixelInterval are the
        constructor's here; the real shape carries traced ones"""
        rng = np.random.RandomState(seed)
        f = lambda *s: rng.randn(*s).astype(np.float32)
        host = rng.randint(0, W, n).astype(np.int32) if host is None else np.asarray(host, np.int32)
        idmax = f(n); idmax[rng.rand(n) < 0.2] = np.nan
        status = rng.randint(0, 6, n).astype(np.int32)
        self.c.imm_resident_set(f(n), f(n), f(n, 8), f(n, 8), f(n, 3), f(n), host, f(n), idmax, status, f(n))
        self.c.imm_resident_set_type(rng.choice([1.0, 2.0, 4.0], n).astype(np.float32))
        return host, status

    def fates(self, n, seed, status=None, p_gone=0.4):
        rng = np.random.RandomState(seed)
        fate = rng.choice([0, 2, 3, -1, -2, -3, 1], n, p=[(1 - p_gone) / 3] * 3 + [p_gone / 6] * 3 + [p_gone / 2]).astype(np.int32)
        sel = rng.permutation(np.nonzero(fate == 1)[0]).astype(np.int32)
        result = rng.choice([1, 0, -1], len(sel)).astype(np.int32)
        return fate, sel, result

    def append_list(self, seed, m=40):
        """a raster-ordered list over the whole image, the border included (entries outside makeNewTraces' bounds are skipped), some with status 0"""
        rng = np.random.RandomState(seed)
        idx = np.sort(rng.choice(PW * PH, m, replace=False)).astype(np.int32)
        edge = np.int32([0, 2, 3 + 2 * PW, 3 + 3 * PW, PW - 5 + 3 * PW, PW - 4 + 3 * PW, 3 + (PH - 5) * PW, 3 + (PH - 4) * PW, PW * PH - 1])
        idx = np.unique(np.concatenate([idx, edge])).astype(np.int32)
        status = rng.choice([0, 1, 2, 4], len(idx), p=[0.1, 0.3, 0.3, 0.3]).astype(np.uint8)
        return idx, status


@pytest.fixture(scope="module")
def planted():
    p = Planted()
    yield p
    p.c.close()


@pytest.mark.parametrize("W", [4, 16])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_planted_sizes(planted, n, W):
    P = planted
    host, status = P.resident(n, W, seed=n + W)
    fate, sel, result = P.fates(n, seed=n)
    idx, st = P.append_list(seed=n)
    hm = np.arange(W, dtype=np.int32)
    hm[1] = -1; hm[2:] -= 1                                                   # the second frame leaves, the new one is hosted behind the others

    def expect(src, new_host, before):
        if n >= 255:
            carried = src[src >= 0]
            assert (np.diff(carried) < 0).any()                               # somebody moved forward into a hole
            assert (src < 0).sum() >= 10 and (new_host[src < 0] == W - 1).all()
    carry_and_compare(P.c, "n=%d W=%d" % (n, W), fate, sel, result, hm, dict(slot=1, host=W - 1, idx=idx, status=st), expect)


def test_planted_shapes_of_holes(planted):
    P = planted
    W, n = 4, 600
    host, status = P.resident(n, W, seed=77)
    mine = [np.nonzero(host == h)[0] for h in range(W)]
    fate = np.zeros(n, np.int32)
    fate[mine[0]] = -1                                                        # host 0 emptied
    fate[mine[1][-40:]] = -2                                                  # host 1: the last 40 are holes, and 10 more before them: a chain of null backs
    fate[mine[1][5:50:5]] = -3
    fate[mine[2]] = np.random.RandomState(1).choice([0, 2, 3], len(mine[2]))  # host 2 untouched
    fate[mine[3][::2]] = 1                                                    # host 3: every other point selected; result 0 keeps the ones that are not OOB
    sel = mine[3][::2][::-1].astype(np.int32)
    result = np.zeros(len(sel), np.int32)

    def expect(src, new_host, before):
        cnt = np.bincount(new_host, minlength=W)
        assert cnt[0] == 0 and cnt[1] == len(mine[1]) - 49 and cnt[2] == len(mine[2])
        assert np.array_equal(src[new_host == 2], mine[2])
        v1 = src[new_host == 1]
        assert np.array_equal(v1[:5], mine[1][:5]) and v1[5] == mine[1][-41]   # the first hole takes the last kept point: 40 null backs were consumed
        oob = before["status"][sel] == OOB
        assert oob.any() and (~oob).any() and cnt[3] == len(mine[3]) - oob.sum()
    carry_and_compare(P.c, "holes", fate, sel, result, expect=expect)
    # every host untouched: the identity
    host, status = P.resident(300, W, seed=78)
    src, _, before, after = carry_and_compare(P.c, "untouched", np.random.RandomState(2).choice([0, 2, 3], 300).astype(np.int32), np.zeros(0, np.int32), None)
    order = np.argsort(host, kind="stable")
    assert np.array_equal(src, order)
    # n_new = 0, by deletion and by dropping every frame; the empty set carries too, and takes an append
    P.resident(300, W, seed=79)
    carry_and_compare(P.c, "all deleted", np.full(300, -1, np.int32), np.zeros(0, np.int32), None)
    assert P.c.imm_resident_get_points()["u"].shape == (0,)
    carry_and_compare(P.c, "empty")
    P.resident(300, W, seed=80)
    carry_and_compare(P.c, "all dropped", host_map=np.full(W, -1, np.int32))
    idx, st = P.append_list(seed=3)
    src, new_host, _, _ = carry_and_compare(P.c, "append to the empty set", append=dict(slot=1, host=2, idx=idx, status=st))
    assert len(src) >= 10 and (new_host == 2).all()


@pytest.mark.parametrize("parts", ["A", "B", "C", "AB", "AC", "BC", "ABC"])
def test_planted_every_combination(planted, parts):
    P = planted
    W, n = 5, 513
    host, status = P.resident(n, W, seed=11)
    fate, sel, result = P.fates(n, seed=12) if "A" in parts else (None, None, None)
    hm = np.int32([0, 1, -1, 2, 3]) if "C" in parts else None
    idx, st = P.append_list(seed=13)
    # appended behind the carried points of an existing host (the hosts after it move back) or to a new last host
    app = dict(slot=1, host=1 if parts != "B" else W, idx=idx, status=st) if "B" in parts else None

    def expect(src, new_host, before):
        if "B" in parts and parts != "B":
            at = np.nonzero(src < 0)[0]
            assert (new_host[:at[0]] <= 1).all() and (new_host[at[-1] + 1:] >= 2).all() and new_host[at[0] - 1] == 1 and len(at) >= 10
    carry_and_compare(P.c, parts, fate, sel, result, hm, app, expect)


# ---------------------------------------------------------------------------------------------------------------- NaN rejection
def test_constructor_rejects_non_finite_energy(planted):
    P = planted
    c = P.c
    img = P.img.copy()
    img[30, 40] = np.inf
    c.frame_upload(1, img)
    try:
        ys, xs = np.mgrid[24:37, 32:49]
        idx = (xs + ys * PW).reshape(-1).astype(np.int32)                      # raster order
        st = np.random.RandomState(4).choice([1, 2, 4], len(idx)).astype(np.uint8)
        eth = orc.imm_create(orc.make_images(img, 1)[0], PW, PH, (idx % PW).astype(np.int32), (idx // PW).astype(np.int32))[3]
        bad = ~np.isfinite(eth)
        assert 8 <= bad.sum() < len(idx) and np.isfinite(eth[np.nonzero(bad)[0].max() + 1:]).all() and not bad[0] and not bad[-1]     # the branch is reached
        P.resident(100, 3, seed=21)

        def expect(src, new_host, before):
            k = -(src[src < 0] + 2)
            assert np.array_equal(k, np.nonzero(~bad)[0])                     # the map skips the rejected entries, the others keep their order
        carry_and_compare(c, "NaN", append=dict(slot=1, host=3, idx=idx, status=st), expect=expect)
    finally:
        c.frame_upload(1, P.img)


# ---------------------------------------------------------------------------------------------------------------- scale
def test_scale_160k(planted):
    P = planted
    n, W = 160000, 8
    rng = np.random.RandomState(33)
    host, status = P.resident(n, W, seed=31)
    fate = np.where(rng.rand(n) < 0.3, rng.choice([-1, -2, -3, 1], n), rng.choice([0, 2, 3], n)).astype(np.int32)
    sel = np.nonzero(fate == 1)[0].astype(np.int32)
    result = rng.choice([1, 0, -1], len(sel)).astype(np.int32)
    hm = np.int32([0, 1, 2, -1, 3, 4, 5, 6])

    def expect(src, new_host, before):
        assert 0.55 * n < len(src) < 0.7 * n and (np.bincount(new_host, minlength=7) > 10000).all()
    carry_and_compare(P.c, "scale", fate, sel, result, hm, expect=expect)


# ---------------------------------------------------------------------------------------------------------------- two keyframes in a row
def test_two_keyframes_in_a_row(planted):
    P = planted
    W = 6
    P.resident(2000, W, seed=41)
    for kf in range(2):
        n = P.c._imm_n
        fate, sel, result = P.fates(n, seed=42 + kf, p_gone=0.3)
        idx, st = P.append_list(seed=44 + kf, m=300)
        carry_and_compare(P.c, "keyframe %d: A" % kf, fate, sel, result)
        carry_and_compare(P.c, "keyframe %d: C + B" % kf, host_map=np.int32([-1, 0, 1, 2, 3, 4]), append=dict(slot=1, host=W - 1, idx=idx, status=st))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_set_as_it_was(planted):
    P = planted
    c = P.c
    W, n = 4, 300
    host, status = P.resident(n, W, seed=51)
    fate, sel, result = P.fates(n, seed=52)
    idx, st = P.append_list(seed=53)
    before = full_state(c)

    def refused(code, **kw):
        with pytest.raises(binding.NaloError, match="nalo error %d:" % code):
            c.imm_resident_carry(**kw)
        assert_same_state(full_state(c), before, str(kw.keys()))
        assert c._imm_n == n
    assert len(sel) >= 3
    refused(ERR_ARG, fate=fate, sel=sel[:-1], result=result[:-1])                             # a selected point is missing
    extra = np.nonzero(fate == 0)[0][:1].astype(np.int32)
    refused(ERR_ARG, fate=fate, sel=np.concatenate([sel, extra]), result=np.concatenate([result, [1]]))      # one too many
    dup = sel.copy(); dup[1] = dup[0]
    refused(ERR_ARG, fate=fate, sel=dup, result=result)                                       # the right number, one of them twice
    wrong = sel.copy(); wrong[0] = extra[0]
    refused(ERR_ARG, fate=fate, sel=wrong, result=result)                                     # a point whose fate is not 1
    outside = sel.copy(); outside[0] = n
    refused(ERR_ARG, fate=fate, sel=outside, result=result)
    refused(ERR_ARG, fate=fate, sel=sel, result=None)                                         # result is required with n_sel > 0
    f2 = fate.copy(); f2[extra[0]] = 4
    refused(ERR_ARG, fate=f2, sel=sel, result=result)
    r2 = result.copy(); r2[0] = 2
    refused(ERR_ARG, fate=fate, sel=sel, result=r2)
    for hm in ([1, 0, 2, 3], [0, 2, 3, 4], [0, 0, 1, 2], [0, 1, 2, -2], [0, 1, 2]):           # not 0 .. W_new-1 increasing; a resident host outside the map
        refused(ERR_ARG, host_map=np.int32(hm))
    refused(ERR_ARG, host_map=np.full(17, -1, np.int32))
    refused(ERR_ARG, append_slot=1, append_host=16, append_idx=idx, append_status=st)
    refused(ERR_ARG, append_slot=1, append_host=-1, append_idx=idx, append_status=st)
    refused(ERR_ARG, append_slot=1, append_host=W, append_idx=np.int32([PW * PH]), append_status=np.uint8([1]))
    refused(ERR_ARG, append_slot=1, append_host=W, append_idx=np.int32([-1]), append_status=np.uint8([1]))
    refused(ERR_ARG, append_slot=1, append_host=W, append_idx=np.int32([500]), append_status=np.uint8([16]))
    swapped = idx.copy(); swapped[[3, 4]] = swapped[[4, 3]]
    refused(ERR_ARG, append_slot=1, append_host=W, append_idx=swapped, append_status=st)      # not in raster order
    twice = idx.copy(); twice[4] = twice[3]
    refused(ERR_ARG, append_slot=1, append_host=W, append_idx=twice, append_status=st)        # a pixel twice
    refused(ERR_STATE, append_slot=2, append_host=W, append_idx=idx, append_status=st)        # a slot without a pyramid
    refused(ERR_STATE, append_slot=3, append_host=W, append_idx=idx, append_status=st)        # no such slot
    refused(ERR_STATE, append_slot=1, append_host=W)                                          # no selection map at all
    c.pixsel_set_random(np.random.RandomState(6).randint(0, 256, PW * PH).astype(np.uint8))
    c.pixsel_make_maps(1, 300.0, 3)
    refused(ERR_STATE, append_slot=0, append_host=W)                                          # the map was made on another slot
    c.frame_upload(1, P.img)
    refused(ERR_STATE, append_slot=1, append_host=W)                                          # the slot was uploaded to since
    c.pixsel_make_maps(1, 300.0, 3)
    c.pixsel_make_hists(0)
    refused(ERR_STATE, append_slot=1, append_host=W)                                          # the thresholds' read-back went through the block that held the list
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.imm_resident_carry_map()                                                            # the set comes from nalo_imm_resident_set
    # the context is usable: the selector's list on the device, all three parts
    c.pixsel_make_maps(1, 300.0, 3)
    sidx, sst = c.pixsel_get_selected()
    assert len(sidx) >= 20
    hm = np.int32([0, -1, 1, 2])
    carry_and_compare(c, "after the refusals", fate, sel, result, hm, dict(slot=1, host=W - 1, idx=sidx, status=sst, explicit=False))
    # a set without types takes no append (its points would have none, the appended ones theirs); it carries without one
    z = np.zeros((5, 8), np.float32)
    c.imm_resident_set(np.zeros(5, np.float32), np.zeros(5, np.float32), z, z, z[:, :3], z[:, 0], np.int32([0, 1, 0, 1, 0]), z[:, 0], z[:, 0], np.zeros(5, np.int32), z[:, 0])
    with pytest.raises(binding.NaloError, match="nalo error %d:" % ERR_STATE):
        c.imm_resident_carry(append_slot=1, append_host=2, append_idx=idx, append_status=st)
    assert c.imm_resident_get_points(with_type=False)["host_idx"].tolist() == [0, 1, 0, 1, 0]
    assert c.imm_resident_carry(fate=np.int32([0, 0, -1, 0, 0]), sel=np.zeros(0, np.int32))[:4] == (4, 1, 0, 0)
    assert c.imm_resident_get_points(with_type=False)["host_idx"].tolist() == [0, 0, 1, 1]


# ---------------------------------------------------------------------------------------------------------------- the real shape
def reissue(b, st):
    """the route the carry replaces: the whole set given to a context (lastTraceUV / lastTracePixelInterval reset, as nalo_imm_resident_set does)"""
    b.imm_resident_set(st["u"], st["v"], st["color"], st["weights"], st["gradH"], st["energyTH"], st["host_idx"], st["idmin"], st["idmax"], st["status"], st["quality"])
    b.imm_resident_set_type(st["my_type"])


def assert_same_traced_state(a, b, what):
    """after one trace the re-issued set equals the carried one in all 31 words: every path of traceOn that does not return at once writes lastTraceUV and the
    interval, and it returns at once only for an OOB point, which holds the constructor's values wherever it became OOB"""
    sa, sb = full_state(a), full_state(b)
    assert_same_state(sa, sb, what)
    return sa


def assert_same_insertion(a, b, what):
    """the window after nalo_ba_carry_window(insert_activated): A took host and slot key of every inserted point from the host copies the carry rebuilt, B from
    the arrays it was given. Launch configuration, frames, prior, points, residual states, history and the linearised, accumulated and solved system bit for bit
    (test_ba_carry_gpu.assert_equal_windows), then every residual's Jacobian products, energy and centre projection (which holds u, v of its point)"""
    from test_ba_carry_gpu import assert_equal_windows
    assert_equal_windows(a, b, what)
    for x, y, name in zip(a.ba_get_residuals(), b.ba_get_residuals(), ("state", "active", "JpJdF", "energy", "centre projection")):
        assert np.array_equal(bits(x), bits(y)), (what, name)


def test_real_shape_keyframe_seam():
    """Context A carries its set through two keyframes; context B runs the same window calls and is GIVEN the set (A's read-back, after it was compared with the
    model) where A carries. After the next trace both hold the same set; the same activation and insertion must then leave the same window, bit for bit."""
    from test_imm_activate_gpu import level1_maps
    from test_imm_large_gpu import CASES, Case, fresh_state
    cs = Case("K")
    c, W, F, s = cs.c, cs.W, cs.F, CASES["K"]
    wp = synth.make_window(w=s["w"], h=s["h"], W=W, P=W * 250, seed=9, n_extra=2, step_z=s["step_z"], yaw_deg=s["yaw"])
    b = binding.Context(cs.w, cs.h, wp.K, n_slots=F)
    both = (c, b)
    try:
        for i in range(F):
            b.frame_upload(int(cs.slot[i]), cs.win.images[i])
        # the window's own points, 250 per host, residuals, history
        st6 = synth.perturbed_poses(wp, sigma_t=0.002, sigma_r=0.0002)
        for x in both:
            x.ba_set_window([int(k) for k in cs.slot[:W]], wp.world_to_cam[:W], aff=cs.aff[:W], exposure=cs.exposure[:W], state6=st6[:W])
            x.ba_set_points(wp.host, wp.u, wp.v, wp.idepth, wp.color, wp.weights)
            x.ba_set_residuals(wp.exists[:, :W])
            x.ba_set_point_history()
        # 1: the resident set, shuffled, traced over the two later frames. The OOB points and every 37th point then lose their pattern weights
        # (optimizeImmaturePoint returns the null pointer for them: result 0), and the set is traced once more so that lastTraceUV / the interval are real
        uu, vv, hh = cs.points(s["per_host"], seed=4, margin=3)
        color, weights, gradH, eth = cs.create(uu, vv, hh)
        p = np.random.RandomState(4 + 7).permutation(len(uu))
        u, v, host, color, weights, gradH, eth = [x[p] for x in (uu.astype(np.float32), vv.astype(np.float32), hh, color, weights, gradH, eth)]
        n = len(u)
        fs = fresh_state(n)
        c.imm_resident_set(u, v, color, weights, gradH, eth, host, fs["idmin"], fs["idmax"], fs["status"], fs["quality"])
        for new in (W, W + 1):
            c.imm_resident_trace(int(cs.slot[new]), *host_to_new(cs.win, new, cs.aff, cs.exposure))
        idmin, idmax, status, quality = c.imm_resident_get()[:4]
        weights = weights.copy()
        weights[::37] = 0
        weights[status == OOB] = 0
        my_type = np.random.RandomState(4 + 8).choice([1.0, 2.0, 4.0], n).astype(np.float32)
        for x in both:
            x.imm_resident_set(u, v, color, weights, gradH, eth, host, idmin, idmax, status, quality)
            x.imm_resident_set_type(my_type)
            x.imm_resident_trace(int(cs.slot[W + 1]), *host_to_new(cs.win, W + 1, cs.aff, cs.exposure))
        # 2, 3: activation with its outputs, insertion
        KRKi, Kt = level1_maps(cs.win, W - 1, yaw_deg=2.5)
        gone = 1
        flagged = np.zeros(W, np.int32); flagged[gone] = 1
        fate, sel, (result, idp, rin) = c.imm_resident_activate(W - 1, KRKi, Kt, flagged, 0.3, 3)
        fate_b, sel_b, (result_b, _, _) = b.imm_resident_activate(W - 1, KRKi, Kt, flagged, 0.3, 3)
        assert np.array_equal(fate, fate_b) and np.array_equal(sel, sel_b) and np.array_equal(result, result_b)
        status_now = c.imm_resident_get()[2]
        for x in both:
            x.ba_carry_window(None, insert_activated=True)
        # 4: carry(A); every removal class occurs, and so does the selected point that stays
        sel_oob = status_now[sel] == OOB
        classes = dict(f1=(fate == -1).sum(), f2=(fate == -2).sum(), f3=(fate == -3).sum(), r1=(result == 1).sum(), rm1=(result == -1).sum(),
                       r0_oob=((result == 0) & sel_oob).sum(), r0_stays=((result == 0) & ~sel_oob).sum())
        print("IMM-CARRY K n=%d classes %s" % (n, {k: int(x) for k, x in classes.items()}))
        assert all(x >= 1 for x in classes.values()), classes

        def expect_a(src, new_host, before):
            assert (np.diff(src) < 0).sum() > W and len(src) < n
            li = before["interval"][src]
            assert len(np.unique(li)) > 50 and (before["lastUV"][src] != -1).any()            # what nalo_imm_resident_set would have reset
        src_a, _, _, after_a = carry_and_compare(c, "K: A", fate, sel, result, expect=expect_a, probe_trace=False)
        assert np.array_equal(after_a["status"], status_now[src_a])
        reissue(b, after_a)
        # 6: the fix pass, flagPointsForRemoval, the removal
        ff = np.zeros(W, np.uint8); ff[gone] = 1
        for x in both:
            x.ba_linearize(False)
            x.ba_linearize(True)
            x.ba_flag_points(ff)
            x.ba_marginalize_flagged()
        # 5 / 7: the selector's map of the new keyframe (frame W of the case); 8: the flagged frame leaves; 9: carry(C + B) from the map on the device
        new_slot = int(cs.slot[W])
        c.pixsel_set_random(np.random.RandomState(3).randint(0, 256, cs.w * cs.h).astype(np.uint8))
        c.pixsel_make_maps(new_slot, 1500.0, 3)
        sidx, sst = c.pixsel_get_selected()
        for x in both:
            x.ba_marginalize_frame(gone)
        hm = np.arange(W, dtype=np.int32); hm[gone] = -1; hm[gone + 1:] -= 1
        px, py = sidx % cs.w, sidx // cs.w
        inb = (px >= 3) & (px < cs.w - 4) & (py >= 3) & (py < cs.h - 4)

        def expect_cb(src, new_host, before):
            # the frame that leaves was flagged at the activation, which deleted its points that were not ready (fate -2): what (C) drops is the rest, and the
            # case needs no more than that there is a rest
            left = int((before["host_idx"] == gone).sum())
            print("IMM-CARRY K: (C) drops %d points of host %d, (B) appends %d of %d selected" % (left, gone, int((src < 0).sum()), len(sidx)))
            assert left >= 1 and (src < 0).sum() == inb.sum() >= 1 and (new_host[src < 0] == W - 1).all()
            assert (new_host[src >= 0] < W - 1).all()
        src_b, host_b, _, after = carry_and_compare(c, "K: C + B", host_map=hm, append=dict(slot=new_slot, host=W - 1, idx=sidx, status=sst, explicit=False),
                                                    expect=expect_cb, probe_trace=False)
        reissue(b, after)
        # the appended records are nalo_imm_create's on the filtered list, bit for bit, and the oracle's
        app = src_b < 0
        got = c.imm_create(new_slot, px[inb].astype(np.int32), py[inb].astype(np.int32))
        ref = orc.imm_create(cs.dI[W], cs.w, cs.h, px[inb].astype(np.int32), py[inb].astype(np.int32))
        for f, g, r in zip(("color", "weights", "gradH", "energyTH"), got, ref):
            assert np.array_equal(bits(after[f][app]), bits(g)) and np.array_equal(bits(g), bits(np.ascontiguousarray(r, np.float32))), f
        assert np.array_equal(after["u"][app], px[inb].astype(np.float32)) and np.array_equal(after["my_type"][app], sst[inb].astype(np.float32))
        # the next keyframe on the carried set: the new frame enters the window, one more trace (with W rows: the largest host index is W - 1), the activation
        # is the model's on the read-back state, and the insertion leaves the window that the re-issued set leaves
        order = [i for i in range(W) if i != gone] + [W]                                    # the case's frames in the new window's order
        entering = c.frame_state(new_slot, wp.world_to_cam[W], frame_id=W, aff=cs.aff[W], exposure=cs.exposure[W])
        frames9 = np.concatenate([cs.win.world_to_cam[order], cs.win.world_to_cam[W + 1:W + 2]])
        nw = types.SimpleNamespace(W=W, K=cs.win.K, world_to_cam=frames9)
        aff2 = [cs.aff[i] for i in order] + [cs.aff[W + 1]]
        exp2 = np.concatenate([cs.exposure[order], cs.exposure[W + 1:W + 2]])
        for x in both:
            x.ba_carry_window(entering)
            x.imm_resident_trace(int(cs.slot[W + 1]), *host_to_new(nw, W, aff2, exp2))
        stt = assert_same_traced_state(c, b, "K: traced after C + B")
        assert np.array_equal(stt["host_idx"], host_b) and (stt["status"][app] != cm.UNINITIALIZED).any()      # the appended points were traced
        KRKi2, Kt2 = level1_maps(nw, W - 1, yaw_deg=2.5)
        D0 = c.dist_make_map(W - 1, KRKi2, Kt2)
        fl2 = np.zeros(W, np.int32)
        m_fate, m_sel, info = am.select(D0, W - 1, stt["host_idx"], stt["u"], stt["v"], stt["idmin"], stt["idmax"], stt["status"], stt["quality"], stt["interval"],
                                        stt["my_type"], KRKi2, Kt2, fl2, 0.3)
        print("IMM-CARRY K: the next activation selects %d of %d" % (len(m_sel), len(stt["u"])))
        assert len(m_sel) >= 1 and (m_fate[stt["host_idx"] == W - 1] == 3).all() and (src_b[m_sel] < 0).sum() == 0       # the appended points are hosted by the newest frame: not visited
        act = [x.imm_resident_activate(W - 1, KRKi2, Kt2, fl2, 0.3, 3) for x in both]
        g_fate, g_sel, (res2, idp2, rin2) = act[0]
        assert np.array_equal(g_fate, m_fate) and np.array_equal(g_sel, m_sel)
        assert np.array_equal(act[1][0], g_fate) and np.array_equal(act[1][1], g_sel) and all(np.array_equal(bits(p), bits(q)) for p, q in zip(act[0][2], act[1][2]))
        n_before = c.P
        for x in both:
            stats = x.ba_carry_window(None, insert_activated=True)
        assert stats[1] == int((res2 == 1).sum()) >= 1 and stats[2] == stats[0] + stats[1] and stats[0] <= n_before
        old_p = c.ba_carry_map()
        assert np.array_equal(-(old_p[old_p < 0] + 1), np.nonzero(res2 == 1)[0])
        ins = g_sel[res2 == 1]
        moved = src_a[src_b[ins]] != ins                                                    # inserted points whose index both carries changed ...
        assert moved.any() and (hm[host[src_a[src_b[ins]]]] != host[src_a[src_b[ins]]]).any()   # ... and whose host was renumbered
        assert_same_insertion(c, b, "K: insertion after A and C + B")
        # a second keyframe, so that the APPENDED points go through an insertion: carry(A), the last frame of the case enters, the set is traced against it
        # once more (nine rows), and the activation for that frame selects points of the keyframe before
        src_a2, _, _, after_a2 = carry_and_compare(c, "K: second A", g_fate, g_sel, res2, probe_trace=False)
        reissue(b, after_a2)
        entering2 = c.frame_state(int(cs.slot[W + 1]), wp.world_to_cam[W + 1], frame_id=W + 1, aff=cs.aff[W + 1], exposure=cs.exposure[W + 1])
        nw9 = types.SimpleNamespace(W=W + 1, K=cs.win.K, world_to_cam=frames9)
        for x in both:
            x.ba_carry_window(entering2)
            x.imm_resident_trace(int(cs.slot[W + 1]), *host_to_new(nw9, W, aff2, exp2))
        st3 = assert_same_traced_state(c, b, "K: traced after the second A")
        KRKi3, Kt3 = level1_maps(nw9, W, yaw_deg=2.5)
        fl3 = np.zeros(W + 1, np.int32)
        act = [x.imm_resident_activate(W, KRKi3, Kt3, fl3, 0.3, 3) for x in both]
        f3, s3, (r3, _, _) = act[0]
        assert np.array_equal(act[1][0], f3) and np.array_equal(act[1][1], s3) and all(np.array_equal(bits(p), bits(q)) for p, q in zip(act[0][2], act[1][2]))
        ins3 = s3[r3 == 1]
        from_app = st3["host_idx"][ins3] == W - 1                                            # hosted by the keyframe before: exactly the appended points
        print("IMM-CARRY K: the second activation inserts %d points, %d of them appended by the carry" % (len(ins3), int(from_app.sum())))
        assert from_app.sum() >= 1 and (src_a2[ins3[from_app]] != ins3[from_app]).any()
        for x in both:
            x.ba_carry_window(None, insert_activated=True)
        assert_same_insertion(c, b, "K: insertion of appended points")
    finally:
        c.close()
        b.close()

"""GPU parity of the candidate-pixel selection at its edges (kernels_pixsel.hip) against the scalar CPU oracle: exact equality of maps, counts and lists.
The cases (tests/pixsel_cases.py) are the ones test_pixsel_cpu.py shows to be non-vacuous: caller-owned random tables that force zero projections and
re-selection rounds, the potentials at which the lanes-per-cell split changes (4 and 8) and beyond 16, exact ties that span lanes, cells, and the four
waves of the 16-lane class, mask histograms at their edge bins and rand() draws that sit on the fuse kernel's comparisons, makeMaps' recursion across the
lane classes, the reuse of the pinned block that holds the last map's list, and a frame wide enough for select() to index past the reference's thresholds."""
import numpy as np
import pytest

import orc
import pixsel_cases as cases
from nalo_slam_amd import binding

pytestmark = pytest.mark.gpu

GROUPS = [(w, h, pot) for (w, h) in cases.SHAPES for pot in cases.POTS[(w, h)]]


@pytest.fixture(scope="module")
def contexts():
    """one context per shape, made on first use: slot 0 holds the scene (levels = 3)"""
    made = {}

    def get(w, h):
        if (w, h) not in made:
            c = binding.Context(w, h, (0.8 * w, 0.8 * w, 0.5 * w, 0.5 * h), n_slots=2, levels=3)
            c.frame_upload(0, cases.scene(w, h))
            made[(w, h)] = c
        return made[(w, h)]
    yield get
    for c in made.values():
        c.close()


def list_matches(c, m):
    idx, st = c.pixsel_get_selected()
    nz = np.flatnonzero(m)
    return np.array_equal(idx, nz) and np.array_equal(st, m.reshape(-1)[nz].astype(np.uint8))


def check_selects(c, w, h, pot):
    _, sm = c.pixsel_make_hists(0)
    assert np.array_equal(sm, cases.thresholds(w, h))
    mine = [k for k in cases.select_cases() if k[:3] == (w, h, pot)]
    assert mine
    for t in sorted(set(k[4] for k in mine)):
        c.pixsel_set_random(cases.table(t, w * h))
        for case in mine:
            if case[4] != t:
                continue
            got, n = c.pixsel_select(0, pot, case[3])
            ref, n_o = cases.oracle_select(*case)
            assert np.array_equal(n, n_o), (case, n, n_o)
            assert np.array_equal(got, ref), (case, int((got != ref).sum()))
            assert list_matches(c, got), case


@pytest.mark.parametrize("w,h,pot", GROUPS)
def test_select_exact(contexts, w, h, pot):
    check_selects(contexts(w, h), w, h, pot)


def test_wide_tail_select_exact(contexts):
    """3232x48: w/32 = 101 and h % 32 != 0, the rows below y = 32 index thresholds 101 .. 201 of a buffer that used to have 201"""
    w, h = cases.WIDE
    check_selects(contexts(w, h), w, h, 3)


@pytest.mark.parametrize("w,h", [(104, 72), (264, 168)])
def test_make_maps_exact(contexts, w, h):
    c = contexts(w, h)
    mine = [k for k in cases.make_maps_cases() if k[:2] == (w, h)]
    assert sorted(set(k[5] for k in mine)) == [0, 1, 2, 3]
    for (_, _, t, density, pot, rec, thf) in mine:
        c.pixsel_set_random(cases.table(t, w * h))
        got, num, pot_g = c.pixsel_make_maps(0, density, pot, recursionsLeft=rec, thFactor=thf)
        ref, num_o, pot_o = orc.pixsel_make_maps(*cases.images(w, h), w, h, cases.table(t, w * h), density, pot, rec, thf)
        assert (num, pot_g) == (num_o, pot_o), (t, density, pot, rec)
        assert np.array_equal(got, ref), (t, density, pot, rec, int((got != ref).sum()))
        assert num == (got != 0).sum() and list_matches(c, got)                    # the list after a sub-selection holds the kept pixels only


@pytest.mark.parametrize("w,h,pot,t", cases.FUSE_SELECTIONS)
def test_make_maps_lidar_exact(contexts, w, h, pot, t):
    c = contexts(w, h)
    mine = [k for k in cases.fuse_cases() if k[:4] == (w, h, pot, t)]
    plain = cases.oracle_select(w, h, pot, 1.0, t)[0]
    created = 0
    for mk in cases.MASKS:
        c.frame_upload(0, cases.scene(w, h), mask=cases.mask(mk, w, h))
        for dn in [k[5] for k in mine if k[4] == mk]:
            c.pixsel_set_random(cases.table(t, w * h), cases.draws(dn, w * h))
            got, num = c.pixsel_make_maps_lidar(0, pot, 1.0)
            ref, num_o = orc.pixsel_make_maps_lidar(*cases.images(w, h), w, h, cases.table(t, w * h), cases.mask(mk, w, h), cases.draws(dn, w * h), pot, 1.0)
            assert num == num_o and np.array_equal(got, ref), (mk, dn, num, num_o, int((got != ref).sum()))
            assert num == (got == 1).sum() + (got == 2).sum() and list_matches(c, got)
            made = np.flatnonzero((plain == 0) & (got == 1))
            assert np.isin(made, c.pixsel_get_selected()[0]).all()                  # pixels the fusion created are in the list
            created += len(made)
    assert created > 100
    c.frame_upload(0, cases.scene(w, h))                                            # the shared context goes back to the frame without a mask


def test_list_reuse(contexts):
    w, h = 104, 72
    c = contexts(w, h)
    c.pixsel_set_random(cases.table("libc", w * h))
    c.pixsel_make_hists(0)
    got, n = c.pixsel_select(0, 3, 1.0)
    assert n.sum() > 256 and list_matches(c, got)
    c.pixsel_make_hists(0)                                                          # the read-back goes through the pinned block that held the list
    with pytest.raises(binding.NaloError, match="nalo error -4"):
        c.pixsel_get_selected()
    got, n = c.pixsel_select(0, 3, 1.0)
    assert c.pixsel_make_hists(0, readback=False) is None                           # NULL, NULL: nothing is read back
    assert list_matches(c, got)
    c.frame_upload(1, cases.scene(w, h)[::-1].copy())                               # another slot: the list is untouched
    assert list_matches(c, got)
    got2, n2 = c.pixsel_select(0, 3, 1.0)
    assert np.array_equal(got2, got) and list_matches(c, got2)

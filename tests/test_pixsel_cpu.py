"""The pixel selection's edge cases on the CPU (no GPU): the model of the device scheme (tests/pixsel_model.py) reaches PixelSelector::select's result
(oracle/orc_pixsel.c) on every case test_pixsel_edges_gpu.py runs, and those cases are not vacuous: every lane class of pixsel_cells_kernel gets level-2 and
level-3 selections, repeated rounds and exact ties that span lanes, the fusion takes and declines every status change on both sides of its thresholds, and
makeMaps' recursion crosses the lane classes both ways. The non-vacuity conditions are conditions on the inputs: they are checked on the reference's results
and on the model of the scheme, never on what the kernels give."""
import functools

import numpy as np
import pytest

import orc
import pixsel_cases as cases
import pixsel_model as model

GROUPS = [(w, h, pot) for (w, h) in cases.SHAPES for pot in cases.POTS[(w, h)]] + [cases.WIDE + (3,)]


@functools.lru_cache(maxsize=None)
def modelled(case):
    w, h, pot, thf, t = case
    return model.run(cases.model_tables(w, h, pot, thf), cases.table(t, w * h))


@pytest.mark.parametrize("w,h,pot", GROUPS)
def test_model_reaches_the_oracles_selection(w, h, pot):
    for case in cases.select_cases():
        if case[:3] != (w, h, pot):
            continue
        ref, n = cases.oracle_select(*case)
        r = modelled(case)
        assert np.array_equal(r["n"], n), (case, r["n"], n)
        assert np.array_equal(r["map"], ref), case                # all three levels, not only level 1
        assert r["flags"].sum() == n[0] == (ref == 1).sum()


def test_select_cases_are_not_vacuous():
    by_class = {1: [], 4: [], 16: []}
    for case in cases.select_cases():
        by_class[model.lanes(case[2])].append((case, cases.oracle_select(*case)[1], modelled(case)))
    for L, rows in by_class.items():
        assert any(n[1] >= 3 and n[2] >= 2 for _, n, _ in rows), L                        # levels 2 and 3 of this lane class select (reference counts)
        assert any(r["rounds"] >= 5 for _, _, r in rows), L                                 # the count -> scan -> select scheme repeats
        assert all(r["rounds"] <= 2000 for _, _, r in rows), max(r["rounds"] for _, _, r in rows)   # every round is a stream wait on the device
        if L > 1:
            assert max(r["span_lanes"] for _, _, r in rows) >= 10, L                        # first strict maximum across two lanes' raster runs
        assert max(r["span_cells2"] for _, _, r in rows) >= 3 and max(r["span_cells3"] for _, _, r in rows) >= 2, L
    # the LDS merge of the 16-lane class: a level-3 maximum attained in two waves (2pot blocks) of a workgroup
    assert max(r["span_blocks3"] for _, _, r in by_class[16]) >= 2
    print("largest round count: %d" % max(r["rounds"] for rows in by_class.values() for _, _, r in rows))


def test_zero_table_is_the_control_that_directions_matter():
    """Direction (0,1) everywhere: the stripe cells (dy == 0) pass the threshold and select nothing, one correcting round, then the fixed point. A cell of
    potential > 16 is wider than half a band of the small scenes, holds pixels of two bands and selects under any direction: there one round may do."""
    for (w, h, pot, thf, t) in cases.select_cases():
        if t != "zero":
            continue
        r = modelled((w, h, pot, thf, t))
        if pot <= 16:
            assert r["rounds"] == 2, (w, h, pot, thf, r["rounds"])
            assert not np.array_equal(r["map"], modelled((w, h, pot, thf, "libc"))["map"])
            assert not np.array_equal(cases.oracle_select(w, h, pot, thf, "zero")[0], cases.oracle_select(w, h, pot, thf, "libc")[0])
        else:
            assert r["rounds"] in (1, 2)


def test_threshold_buffer_covers_every_index():
    for w in list(range(32, 400, 7)) + [1224, 3199, 3200, 3231, 3232, 3233, 6464]:
        for h in (32, 33, 36, 48, 63, 64, 100, 368):
            xs, ys = np.arange(4, w - 5), np.arange(4, h - 3)
            largest = (xs.max() >> 5) + (ys.max() >> 5) * (w // 32)
            assert largest < model.ths_len(w, h) == orc.pixsel_ths_len(w, h)
            if w // 32 < 100:
                assert model.ths_len(w, h) == (w // 32) * (h // 32) + 100                 # the reference's allocation wherever it is enough
    w, h = cases.WIDE
    assert (w // 32) * (h // 32) + 100 == 201 == (w - 6 >> 5) + (h - 4 >> 5) * (w // 32)   # the index the + 100 does not hold
    assert (cases.images(w, h)[1].reshape(h, w)[32:h - 3, 3200:w - 5] > 0).any()          # pixels that read it: candidates under the tail's 0 only


def _fuse_counts(st0, st1, m, dr, q, mm):
    r = dr.astype(np.int64) % 1000
    out = {}
    a, ok = st0 == 1, m < q // 3
    out.update({"1->2 taken": a & (st1 == 2), "1->2 declined by rs": a & ok & (st1 == 1), "1->2 declined at rs == 0.5": a & ok & (st1 == 1) & (r == 500),
                "1->2 declined by mask": a & ~ok & (r > 500)})
    a, ok = st0 == 2, m > q + int((mm - q) / 2)
    out.update({"2->1 taken": a & (st1 == 1), "2->1 declined by rs": a & ok & (st1 == 2), "2->1 declined at rs == 0.6f": a & ok & (st1 == 2) & (r == 600),
                "2->1 declined by mask": a & ~ok & (r < 600)})
    a, ok = st0 == 0, m > q
    out.update({"0->1 taken": a & (st1 == 1), "0->1 taken at rs == 0.01f": a & (st1 == 1) & (r == 10), "0->1 declined by rs": a & ok & (st1 == 0),
                "0->1 declined at rs == 0.011f": a & ok & (st1 == 0) & (r == 11), "0->1 declined by mask": a & ~ok & (r < 10)})
    return {k: int(v.sum()) for k, v in out.items()}


def test_fusion_takes_and_declines_every_transition():
    total, quantiles = {}, set()
    for (w, h, pot, t, mk, dn) in cases.fuse_cases():
        st0 = cases.oracle_select(w, h, pot, 1.0, t)[0]
        mask, dr = cases.mask(mk, w, h), cases.draws(dn, w * h)
        st1, n, qm = orc.pixsel_fuse_mask(mask, dr, st0)
        assert n[0] == (st1 == 1).sum() and n[1] == (st1 == 2).sum()
        quantiles.add((mk, int(qm[0]), int(qm[1])))
        if dn == "crafted":
            for k, v in _fuse_counts(st0.reshape(-1), st1.reshape(-1), mask.reshape(-1), dr, int(qm[0]), int(qm[1])).items():
                total[k] = total.get(k, 0) + v
    assert all(v >= 5 for v in total.values()) and len(total) == 13, total
    # the histogram's edges: no return at all / one return -> quantile 255; a constant mask; a mask whose top bin (255) is taken; (int)0.5 counted in bin 0
    q = {mk: (a, b) for mk, a, b in quantiles}
    assert q["zero"] == (255, 1) and q["single"] == (255, 90) and q["const37"] == (36, 37) and q["top_bins"][1] == 255 and q["fractions"][1] == 199
    for mk in cases.MASKS:
        m = cases.mask(mk, 104, 72)
        assert np.isfinite(m).all() and m.min() >= 0 and m.max() <= 256                      # the oracle indexes its 257-entry histogram with (int)mask
    assert (cases.mask("top_bins", 104, 72) == 256).sum() > 5 and (cases.mask("fractions", 104, 72) == 0.5).sum() > 5
    res = set(int(v) % 1000 for v in cases.draws("crafted", 104 * 72))
    assert res == set(cases.RESIDUES) and cases.draws("crafted", 104 * 72).min() >= 0


def test_make_maps_cases_cross_the_lane_classes():
    traces = {}
    for case in cases.make_maps_cases():
        w, h, t, density, pot, rec, thf = case
        visited, quotia, n = cases.make_maps_trace(*case)
        m, num, pot_o = orc.pixsel_make_maps(*cases.images(w, h), w, h, cases.table(t, w * h), density, pot, rec, thf)
        assert len(visited) <= rec + 1
        assert all(modelled((w, h, p, thf, t))["rounds"] <= 2000 for p in visited), case
        sel = cases.oracle_select(w, h, visited[-1], thf, t)[0]
        assert ((m != 0) <= (sel != 0)).all() and num == (m != 0).sum()               # the trace ends at the potential the oracle ended at
        if quotia < 0.95:                                                                 # the sub-selection: the rank-th pixel stays iff rp[rank] <= charTH
            charTH, rp = int(255 * np.float32(quotia)) & 255, cases.table(t, w * h)[:n]
            assert np.array_equal(m.reshape(-1)[np.flatnonzero(sel)] != 0, rp <= charTH)
            if t == "mod256" and rec == 0 and abs(quotia - 0.95) < 1e-6:                  # a long list: both sides of `> charTH` are visited
                assert n >= 256 and (rp == charTH).any() and (rp == charTH + 1).any(), (case, charTH)
        else:
            assert np.array_equal(m, sel)
        traces[case] = ([model.lanes(p) for p in visited], quotia)
    for (w, h) in [(104, 72), (264, 168)]:
        cl = [v[0] for k, v in traces.items() if k[:2] == (w, h)]
        assert any(c[0] == 1 and c[-1] == 16 for c in cl) and any(c[0] == 16 and c[-1] == 1 for c in cl)
        assert any(len(c) >= 3 for c in cl)                                               # more than one re-selection
        qs = sorted(v[1] for k, v in traces.items() if k[:2] == (w, h) and k[5] == 0 and abs(v[1] - 0.95) < 1e-6)
        assert len(qs) == 2 and qs[0] < 0.95 <= qs[1]                                     # quotia just below and just above makeMaps' 0.95

"""The inputs test_track_tries_cpu.py and test_track_tries_gpu.py share: the frame pair, the tracking reference and the lists of tries of every scenario, the
fp32 oracle's run of each (computed once per process) and the branch pattern it must show. The CPU file asserts the patterns on the oracle; the GPU file then
asserts the same patterns on the device, so it never asks for a branch the reference arithmetic does not take on these inputs.

Scene 640x480 (conftest's small_window: synth.make_window(w=640, h=480, W=4, P=400, seed=7)), 4 levels, reference = frame W-1 with tracker_inputs(win)
(3000 residuals; every level's cloud fits one round of the grid), new frame = frame W. T09 = exp(0.9 log(true motion)). LIST31 = the reference's 31 hypotheses with
T09 as the constant-motion entry (slast_2_sprelast = T09^-1, lastF_2_slast = identity).

  name        new frame   tries                                                lastCoarseRMSE[0]   what the reference arithmetic does
  accept      frame       LIST31                                               100                 try 0 is good and ends the loop (:653)
  all31       frame       LIST31                                               1e-6                all 31 run: try 0 wins, 1-2 stop at level 1, 3-30 at level 2
  affine      frame       [Ttrue rot_y(0.25), T09, Ttrue rot_y(0.25), I]        1e-6                try 0 finishes every level and fails the affine tail (:1249) with finite
                                                                                                   residuals, try 1 wins, tries 2-3 stop at level 2
  bright      4 x frame   [T09, I]                                             1e-6                both finish and fail the affine tail: none good
  nan         all NaN     [T09, I, T09]                                        1e-6                ok with NaN residuals (:633's isfinite): none good
  coarsest    frame       [T09, Ttrue rot_x(0.6), I]                           1e-6                try 1 is not good and stops at level 2, yet its coarsest-level residual
                                                                                                   (3.49: the gross rotation leaves few points in view) lowers achievedRes[3]
                                                                                                   (:643-650 run for every try once one was good); try 2 then stops AT the coarsest level
  takeover    frame       [exp(0.5 log Ttrue), T09]                            1e-6                try 0 is good (lastRes[0] 8.68), try 1 is good and better (4.48): it takes over
  repeat      frame + 45  [T09, Ttrue rot_x(0.6), I]                           1e-6                the brightness jump saturates the coarsest level: tries 0 and 1 re-run it
                                                                                                   (haveRepeated), try 2 stops on its first pass of it, before any re-run
The two branches the issue's probe had not reached (a stop at the coarsest level, a good try taking over from a good one) were found with the oracle at the
first attempt each that was tried for them; nothing is planted through the device.
"""
import functools

import numpy as np

import orc
import track_tries_model as model
from helpers import tracker_inputs, true_rel_pose
from nalo_slam_amd import synth

EXPOSURES = [1.0, 1.0]
IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])


def rot(axis, angle):
    w = np.zeros(6)
    w[3 + axis] = angle
    return model.se3_exp(w)


class Scene:
    def __init__(self, w=640, h=480):
        self.win = win = synth.make_window(w=w, h=h, W=4, P=400, seed=7)
        self.levels = win.levels
        self.ref_img, self.new_img = win.images[win.W - 1], win.images[win.W]
        self.inputs = tracker_inputs(win)
        self.Ttrue = true_rel_pose(win, win.W - 1, win.W)
        self.T09 = orc.se3_exp(orc.se3_log(self.Ttrue) * 0.9)
        self.list31 = model.motion_tries(model.se3_inv(self.T09), IDENTITY)
        self.dI_ref, _ = orc.make_images(self.ref_img, self.levels)

    def new_frame(self, kind):
        if kind == "frame":
            return self.new_img
        if kind == "plus45":
            return (self.new_img + 45.0).astype(np.float32)
        if kind == "bright":
            return (self.new_img * 4.0).astype(np.float32)
        assert kind == "nan"
        return np.full_like(self.new_img, np.nan)

    def scenario(self, name):
        """(kind of new frame, tries [n, 3, 4], lastCoarseRMSE[0])"""
        bad, gross = model.se3_mul(self.Ttrue, rot(1, 0.25)), model.se3_mul(self.Ttrue, rot(0, 0.6))
        return {
            "accept": ("frame", self.list31, 100.0),
            "all31": ("frame", self.list31, 1e-6),
            "affine": ("frame", np.array([bad, self.T09, bad, IDENTITY]), 1e-6),
            "bright": ("bright", np.array([self.T09, IDENTITY]), 1e-6),
            "nan": ("nan", np.array([self.T09, IDENTITY, self.T09]), 1e-6),
            "coarsest": ("frame", np.array([self.T09, gross, IDENTITY]), 1e-6),
            "takeover": ("frame", np.array([orc.se3_exp(orc.se3_log(self.Ttrue) * 0.5), self.T09]), 1e-6),
            "repeat": ("plus45", np.array([self.T09, gross, IDENTITY]), 1e-6),
        }[name]

    @functools.lru_cache(maxsize=None)
    def oracle_tracker(self):
        orc.lib("f32").orc_set_sum_mode(0)
        trk = orc.Tracker(self.win.w, self.win.h, self.levels, self.win.K)
        trk.set_ref(self.dI_ref, *self.inputs)
        return trk

    @functools.lru_cache(maxsize=None)
    def oracle(self, name):
        """the model loop over the fp32 oracle's trackNewestCoarse; a record's extra = (evaluations per level, haveRepeated)"""
        kind, tries, rmse0 = self.scenario(name)
        trk = self.oracle_tracker()
        dI_new, _ = orc.make_images(self.new_frame(kind), self.levels)

        def track(T0, aff0, min_res):
            orc.lib("f32").orc_set_sum_mode(0)
            r = trk.track(dI_new, T0, aff0, (0, 0), EXPOSURES, self.levels - 1, min_res=min_res)
            ev, rep = trk.last_evals()
            return r + (ev.copy(), int(rep))
        return model.track_new_coarse(track, tries, (0, 0), rmse0)


SCENARIOS = ("accept", "all31", "affine", "bright", "nan", "coarsest", "takeover", "repeat")


def pattern(res):
    """the decisions of a run, from the model's dict or from binding.Context.trk_track_tries': (tries run, winner, have_one_good, [(ok, taken, abort_lvl)])"""
    recs = res["records"]
    return (res["try_iterations"], res["winner"], res["have_one_good"], [(int(r["ok"]), int(r["taken"]), int(r["abort_lvl"])) for r in recs])


def expected_pattern(name, top):
    """what the header's table says, as pattern() returns it; top = the coarsest level"""
    good, win_, lvl1, lvl2, tail = (1, 0, -1), (1, 1, -1), (0, 0, 1), (0, 0, 2), (0, 0, -1)
    return {
        "accept": (1, 0, 1, [win_]),
        "all31": (31, 0, 1, [win_] + [lvl1] * 2 + [lvl2] * 28),
        "affine": (4, 1, 1, [tail, win_, lvl2, lvl2]),
        "bright": (2, -1, 0, [tail, tail]),
        "nan": (3, -1, 0, [good, good, good]),
        "coarsest": (3, 0, 1, [win_, lvl2, (0, 0, top)]),
        "takeover": (2, 1, 1, [win_, win_]),
        "repeat": (3, 0, 1, [win_, lvl2, (0, 0, top)]),
    }[name]


@functools.lru_cache(maxsize=None)
def scene():
    return Scene()

"""nalo_tsdf_shift at the chain's volume, 256x64x256 voxels, beside a device-to-device copy of the same bytes in the same run. The shift is a pure copy: what
the words are does not matter to it, so the volume holds its initial values; what matters is the shift, which decides how many groups load at all and how wide.

  legs        (4, 0, 0) and (-8, 4, -12): the 16-byte loads; (1, 0, 0) and (-7, 4, -10): four words a lane; each without and with colour
  shift       the scope tsdf_shift (the kernel, HIP events), median and p95, legs alternating inside every repetition
  copy        torch's copy_ of the same arrays (tsdf, weight, and the colour block with colour), device to device, between torch events, alternating with the legs
  bytes       read plus written: 16 B a voxel without colour, 40 B with; beside both, the copy rate of nalo_hbm_calibrate

Prints a table and one JSON line; --log appends both to a file."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from tsdf_ab import stats  # noqa: E402  (loads the package)

import torch  # noqa: E402

from nalo_slam_amd import binding  # noqa: E402

DIMS = (256, 64, 256)
SHIFTS = [(4, 0, 0), (1, 0, 0), (-8, 4, -12), (-7, 4, -10)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    c = binding.Context(64, 48, (70.0, 68.0, 31.5, 23.5), n_slots=1)
    n = DIMS[0] * DIMS[1] * DIMS[2]
    copy_GBs, _ = c.hbm_calibrate(1 << 28, 10)
    out = {"part": "tsdf_shift", "dims": list(DIMS), "copy_GBs": copy_GBs, "legs": {}}
    lines = ["tsdf_shift over %dx%dx%d voxels; nalo_hbm_calibrate copies at %.0f GB/s" % (DIMS + (copy_GBs,))]
    for colour in (False, True):
        c.tsdf_create((-12.8, -3.2, 0.0), 0.1, DIMS, 0.4, 16.0)
        if colour:
            c.tsdf_color_enable()
        c.tsdf_shift((1, 1, 1))                                                  # the spares exist from here on
        c.sync()
        words = (5 if colour else 2) * n
        src, dst = torch.zeros(words, device="cuda"), torch.empty(words, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        copy_us = []
        c.profile_enable(True)
        c.profile_select("tsdf_shift")
        scope = {s: [] for s in SHIFTS}
        for k in range(a.warmup + a.reps):
            for s in SHIFTS:
                c.profile_reset()
                c.tsdf_shift(s)
                c.tsdf_shift(tuple(-v for v in s))                               # base stays small; the way back is not counted
                c.sync()
                if k >= a.warmup:
                    scope[s].append(float(c.profile_samples("tsdf_shift")[0]))
            c.sync()
            ev[0].record()
            dst.copy_(src)
            ev[1].record()
            torch.cuda.synchronize()
            if k >= a.warmup:
                copy_us.append(ev[0].elapsed_time(ev[1]) * 1e3)
        c.profile_enable(False)
        cp = stats(copy_us)
        moved = 8.0 * words
        tag = "colour" if colour else "plain"
        out["legs"][tag] = {"bytes": moved, "copy_us": cp, "shift_us": {str(s): stats(np.asarray(v, np.float64)) for s, v in scope.items()}}
        lines.append("  %-6s %.1f MB read plus written; device-to-device copy median %.1f us (p95 %.1f) = %.0f GB/s" % (tag, moved * 1e-6, cp["median"], cp["p95"], moved / cp["median"] * 1e-3))
        for s in SHIFTS:
            st = out["legs"][tag]["shift_us"][str(s)]
            lines.append("         shift %-14s scope median %.1f us (p95 %.1f) = %.0f GB/s, %.2f x the copy" % (s, st["median"], st["p95"], moved / st["median"] * 1e-3, st["median"] / cp["median"]))
    lines.append(json.dumps(out))
    print("\n".join(lines))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")
    c.close()


if __name__ == "__main__":
    main()

"""the gate-cancel flow of tests/test_ba_gpu.py as a probe: N child processes per mode (plain / cancelled first optimize), the poses after restore + optimize hashed;
every line should be the same. usage: gate_probe.py [repeats]"""
import hashlib, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
script = r"""
import json, sys
root = sys.argv[1]
sys.path.insert(0, root)
import numpy as np
import nalo_pkg; nalo_pkg.load()
from nalo_slam_amd import binding, synth
win = synth.make_window(w=640, h=480, W=5, P=1200, seed=31)
st6 = synth.perturbed_poses(win, sigma_t=0.004, sigma_r=0.0004)
c = binding.Context(win.w, win.h, win.K, n_slots=win.W)
for i in range(win.W):
    c.frame_upload(i, win.images[i])
c.ba_set_window(list(range(win.W)), win.world_to_cam[:win.W], state6=st6)
c.ba_set_points(win.host, win.u, win.v, win.idepth, win.color, win.weights)
c.ba_set_residuals(win.exists)
c.ba_snapshot()
if sys.argv[2] == "cancel":
    c.test_inject(binding.INJECT_GATED_SOLVE, 2)      # the second gated solve fails between the pre-launch and its gates
out = {}
try:
    c.ba_optimize(6, never_break=True)
    out["first"] = "no error"
except RuntimeError as e:
    out["first"] = str(e)
c.sync()                                    # nothing is left spinning: the stream drains
c.ba_restore()
out["rmse_after"] = c.ba_optimize(6, never_break=True)
out["w2c_after"] = np.asarray(c.ba_get_frames()[1]).tolist()
c.close()
print("RESULT " + json.dumps(out))
"""
n = int(sys.argv[1]) if len(sys.argv) > 1 else 6
with tempfile.TemporaryDirectory() as td:
    p = os.path.join(td, "gc.py"); open(p, "w").write(script)
    seen = {}
    for rep in range(n):
        for name in ("plain", "cancel"):
            r = subprocess.run([sys.executable, p, ROOT, name], capture_output=True, text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if not line:
                print(name, "FAILED", r.stderr[-300:]); continue
            d = json.loads(line[-1][7:])
            h = hashlib.md5(json.dumps([d["rmse_after"], d["w2c_after"]]).encode()).hexdigest()[:10]
            seen.setdefault(h, []).append(name)
            print(rep, name, d["first"][:40], "rmse %.9g" % d["rmse_after"], h, flush=True)
    print("distinct results:", {k: len(v) for k, v in seen.items()})

"""Builds libnalo_gpu.so (HIP kernels + C-ABI) for gfx950 in-tree with hipcc. No torch involved."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = ["host_api.hip", "host_ba.hip", "kernels_pyramid.hip", "kernels_ingest_dev.hip", "kernels_handoff.hip", "kernels_tracker.hip", "kernels_trk_lm.hip", "kernels_ba.hip", "kernels_ba_lin.hip", "kernels_ba_carry.hip", "kernels_dense.hip", "kernels_plane.hip", "kernels_imm.hip", "kernels_imm_carry.hip", "kernels_map.hip", "kernels_map_render.hip", "kernels_map_render_mesh.hip", "host_map_render_mesh.cpp", "host_map.hip", "kernels_tsdf.hip", "kernels_tsdf_replace.hip", "kernels_tsdf_replace_n.hip", "kernels_tsdf_mesh.hip", "kernels_tsdf_raycast.hip", "kernels_tsdf_align.hip", "kernels_tsdf_archive.hip", "host_tsdf.hip", "host_tsdf.cpp", "kernels_init.hip", "kernels_init_window.hip", "kernels_pixsel.hip", "kernels_depth_image.hip", "kernels_window_plot.hip", "kernels_init_plot.hip", "kernels_residual_plot.hip", "host_io.cpp", "host_ground.cpp", "host_rccl.hip", "host_init.hip"]
OUT = os.path.join(HERE, "libnalo_gpu.so")
NO_CONTRACT = {"kernels_pyramid.hip", "kernels_ingest_dev.hip", "kernels_plane.hip", "kernels_imm.hip", "kernels_imm_carry.hip", "kernels_map.hip", "kernels_map_render.hip", "kernels_map_render_mesh.hip", "host_map_render_mesh.cpp", "kernels_init.hip", "kernels_init_window.hip", "kernels_pixsel.hip", "kernels_depth_image.hip", "kernels_window_plot.hip", "kernels_init_plot.hip", "kernels_residual_plot.hip", "host_init.hip", "host_ground.cpp", "kernels_tsdf.hip", "kernels_tsdf_replace.hip", "kernels_tsdf_replace_n.hip", "kernels_tsdf_mesh.hip", "kernels_tsdf_raycast.hip", "kernels_tsdf_align.hip", "host_tsdf.cpp"}   # a1 is bit-exact vs the reference's scalar fp32 code: no FMA contraction


def build(force=False, verbose=False):
    csrc = os.path.join(HERE, "csrc")
    srcs = [os.path.join(csrc, s) for s in SRC if os.path.exists(os.path.join(csrc, s))]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")] + [os.path.join(HERE, "..", "include", "nalo_gpu.h"), os.path.join(HERE, "..", "include", "nalo_io.h"), os.path.join(HERE, "..", "include", "nalo_io_mesh.h"), os.path.abspath(__file__)]
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    if not force and os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    objs = []
    procs = []
    for s in srcs:
        # the object name carries the contraction policy, so moving a file in/out of NO_CONTRACT rebuilds it
        tag = "nc" if os.path.basename(s) in NO_CONTRACT else "fc"
        o = os.path.join(HERE, "build", os.path.basename(s) + "." + tag + ".o")
        objs.append(o)
        if not force and os.path.exists(o) and all(os.path.getmtime(o) >= os.path.getmtime(d) for d in [s] + deps[len(srcs):]):
            continue
        cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", s, "-o", o, "-Wno-unused-result"]
        if os.path.basename(s) in NO_CONTRACT:
            cmd += ["-ffp-contract=off"]
        if verbose:
            cmd += ["-Rpass-analysis=kernel-resource-usage"]
        procs.append((s, subprocess.Popen(cmd)))
    for s, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed on " + s)
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs + ["-ldl", "-lz"])
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="--verbose" in sys.argv))

#!/usr/bin/env python3
"""Times the mesher (dvp_mesh_build) on cuda:0 at a real size and appends the lines to profiles/mesh.txt.  The data: a sphere of 500
voxels radius (the scene spans 1 000 voxels) seen by VIEWS cameras (default ten) of 3104 x 2064 pixels on a ring around it, every
pixel that sees it masked; voxel 0.01, truncation 4 voxels, min_weight 2.
  --device   dvp_mesh_build as shipped: allocation, integration and extraction (each ends with a wait), blocks, vertices, faces, the
             table's doublings and the job's device memory
  --host     the serial host text (tests/mesh_host) on the FIRST view alone - a tenth of the views, and of the blocks what that view
             allocates - labelled as such
usage: mesh_timing.py [--device] [--host] [VIEWS]"""
import importlib
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import np_mesh as M  # noqa: E402

W, H, S, RADIUS = 3104, 2064, 0.01, 5.0


def view(k, views):
    a = 2.0 * np.pi * k / views
    eye = np.array([14.0 * np.cos(a), 14.0 * np.sin(a), 3.0 * np.sin(3 * a)])
    cam = M.camera(eye, [0.0, 0.0, 0.0], 3300.0, 1)
    cam["K"][2], cam["K"][5] = (W - 1) / 2.0, (H - 1) / 2.0
    cam["width"], cam["height"] = W, H
    K, R, t = cam["K"].astype(np.float64).reshape(3, 3), cam["R"].astype(np.float64).reshape(3, 3), cam["t"].astype(np.float64)
    y, x = np.mgrid[0:H, 0:W]
    d = np.stack([(x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1], np.ones((H, W))], -1) @ R
    o = -R.T @ t
    a2, b, c = (d * d).sum(-1), 2 * (d @ o), o @ o - RADIUS * RADIUS
    disc = b * b - 4 * a2 * c
    z = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a2), 0.0)
    depth = np.where(z > 0, z, 0).astype(np.float32)
    bgr = np.stack([(x // 8) % 256, (y // 8) % 256, (x + y) // 16 % 256], -1).astype(np.uint8)
    return cam, depth, (depth > 0).astype(np.uint8), bgr


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    views = int(args[0]) if args else 10
    lines = []
    t = time.time()
    data = []
    for k in range(views):
        data.append(view(k, views))
        print("view %d rendered (%.1f s)" % (k, time.time() - t), flush=True)
    masked = sum(int(v[2].sum()) for v in data)
    head = "%d views of %d x %d, %d masked pixels, voxel %g, truncation %g, min_weight 2" % (views, W, H, masked, S, 4 * S)
    if "--device" in sys.argv:
        capi = importlib.import_module("dvp-mvs_amd").get_capi()
        capi.mesh_build(data[:1], 0.08, None, 1)      # (the first call pays for the module's load)
        for run in range(2):
            t = time.time()
            got = capi.mesh_build(data, S, 4 * S, 2, timings=True)
            wall = time.time() - t
            lines.append("device, run %d: %s: allocation %.1f ms, integration %.1f ms, extraction %.1f ms; %d blocks, %d vertices, %d faces, %d doublings, %.1f MB on the device; "
                         "the whole call with uploads and downloads %.2f s" % (run, head, got["ms"][0], got["ms"][1], got["ms"][2], got["blocks"], len(got["vertices"]),
                                                                               len(got["faces"]), got["regrows"], got["bytes"] / 1e6, wall))
            print(lines[-1], flush=True)
    if "--host" in sys.argv:
        M.build_program()
        with tempfile.TemporaryDirectory() as tmp:
            scene = os.path.join(tmp, "scene.bin")
            M.write_scene(data[:1], scene)
            t = time.time()
            out = M.run_program("build", scene, repr(S), repr(4 * S), 1, os.path.join(tmp, "out"))
            wall = time.time() - t
            assert out.returncode == 0, out.stderr
            lines.append("host, the serial text on view 0 alone (1 of %d views, min_weight 1; reading and writing its files included): %.2f s; %s"
                         % (views, wall, out.stdout.strip()))
            print(lines[-1], flush=True)
    path = os.path.join(ROOT, "profiles", "mesh.txt")
    fresh = not os.path.exists(path)
    with open(path, "a") as f:
        if fresh:
            f.write("# python tools/mesh_timing.py --device --host   (see the tool's docstring for the scene)\n"
                    "# The three device stages are wall-clock laps of dvp_mesh_build, each ending with a wait for the stream, and hold the stage's\n"
                    "# device-memory reservations: `allocation` the table, the claims of every view, the compaction and the host's sort of the keys;\n"
                    "# `integration` the slot-index and forward-neighbour launches as well as the integration launch; `extraction` both passes over\n"
                    "# cells and faces, the two scans and the count read-backs.  `the whole call` is what a caller of capi.mesh_build waits: the\n"
                    "# host's two passes over every view's pixels, the uploads, the build, the downloads.\n"
                    "# The host line is NOT the same work as the device lines: one view of the ten, the blocks that view allocates, min_weight 1,\n"
                    "# files read and written.  It says what the serial text costs on a tenth of the input, no more; no ratio is drawn from it.\n")
        for line in lines:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

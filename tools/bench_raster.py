#!/usr/bin/env python3
"""The exact z-buffer on the device: the 36-pair VGA ring (10k, 10k + 3 degrees, D = 128, ground-truth poses) fused into
[-0.13, 0.13]^3 at 128^3 and 256^3 grid points, the surface cleaned (default thresholds) and rendered as it is and simplified at 2
voxels, from the first ring camera at 640 x 480 and at 1920 x 1080.  Prints one JSON line and writes it to
profiles/raster_bench_line.json.

  raster_ms          HIP events from the first to the last launch of one sfmx_raster_run (sfmx_raster_last_us), mean over `calls`
                     after one warm-up call
  raycast_ms         sfmx_raycast_render of the same volume and camera in the same run (the yardstick of DESIGN.md 18)
  ratio              raster_ms / raycast_ms
  frags_per_face     fragments / faces; big_share = faces on the tiled path / faces
  --check            the 128^3 / VGA render of the cleaned surface compared byte for byte with tests/raster_ref.py (NumPy, the box
                     form: every face against every pixel of a VGA image is 10^11 tests)
Run on the GPU box."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "structure-from-motion-3d-reconstruction_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    capi = importlib.import_module(PKG + ".capi")
    pipeline = importlib.import_module(PKG + ".pipeline")
    synth = importlib.import_module(PKG + ".synth")
    angles = [x for k in range(36) for x in (10.0 * k, 10.0 * k + 3.0)]
    seq = synth.make_sequence(len(angles), 640, 480, angles=angles)
    poses = [(seq["R"][i].T, -seq["R"][i].T @ seq["t"][i]) for i in range(len(angles))]
    ctx = capi.Context(0)
    st = ctx.stereo(640, 480)
    views = []
    for k in range(36):
        i, j = 2 * k, 2 * k + 1
        r = pipeline.stereo_rectify(seq["K"], poses[i], poses[j], 640, 480)
        il, ir = (seq["images"][j], seq["images"][i]) if r["swapped"] else (seq["images"][i], seq["images"][j])
        views.append((r, st.disparity(il, ir, r["H_l"], r["H_r"])))
    st.close()
    K = np.asarray(seq["K"], np.float64).reshape(3, 3)
    R, c = poses[0]
    dist = float(np.linalg.norm(c))
    march = dict(z_min=max(dist - 0.23, 0.01), z_max=dist + 0.23)
    cams = {}
    for w, h in ((640, 480), (1920, 1080)):
        cams[f"{w}x{h}"] = dict(R_rw=np.asarray(R, np.float64).T.copy(), c_left=np.asarray(c, np.float64), f=float(K[0, 0]) * h / 480.0,
                                cx=(w - 1) / 2.0, cy=(h - 1) / 2.0, w=w, h=h)
    out = {"calls": a.calls, "pairs": 36}
    rc, rs, cl, sp = ctx.raycast(), ctx.raster(), ctx.clean(), ctx.simplify()
    ok = True
    for n in (128, 256):
        vol = dict(origin=(-0.13, -0.13, -0.13), voxel=0.26 / (n - 1), dims=(n, n, n))
        fu = ctx.fusion(**vol)
        for r, d in views:
            fu.add_view(r, d)
        fu.extract()
        cl.fusion(fu)
        cr = cl.read()
        sp.clean(cl, cell=2.0 * vol["voxel"], origin=vol["origin"])
        ns, pv, pf, ms = sp.device_mesh()
        meshes = {"cleaned": dict(verts=cr["verts"], faces=cr["faces"], n=None, m=None, faces_n=len(cr["faces"])),
                  "simplified": dict(verts=pv, faces=pf, n=ns, m=ms, faces_n=ms)}
        ctx.set_timing(True)
        for name, cam in cams.items():
            rc.render(fu, cam, **march, read=False)  # warm-up
            us = []
            for _ in range(a.calls):
                rc.render(fu, cam, **march, read=False)
                us.append(rc.last_us())
            ray = float(np.mean(us))
            for mname, mesh in meshes.items():
                args = (mesh["verts"], mesh["faces"], cam, march["z_min"])
                kw = dict(n=mesh["n"], m=mesh["m"], read=False)
                rs.render(*args, **kw)  # warm-up
                us = []
                for _ in range(a.calls):
                    rs.render(*args, **kw)
                    us.append(rs.last_us())
                t = float(np.mean(us))
                cnt = rs.counts()
                row = dict(raster_ms=round(t / 1e3, 4), raycast_ms=round(ray / 1e3, 4), ratio=round(t / ray, 3), faces=mesh["faces_n"],
                           fragments=cnt["fragments"], frags_per_face=round(cnt["fragments"] / max(mesh["faces_n"], 1), 3),
                           big_share=round(rs.last_big_faces() / max(mesh["faces_n"], 1), 5), hits=cnt["hits"],
                           back_pixels=cnt["back_pixels"], faces_drawn=cnt["faces_drawn"], faces_behind=cnt["faces_behind"],
                           faces_outside=cnt["faces_outside"])
                if a.check and n == 128 and name == "640x480" and mname == "cleaned":
                    import raster_ref as RR
                    got = rs.read()
                    ref = RR.render(cr["verts"], cr["faces"], cam, march["z_min"])
                    try:
                        RR.same(got, ref, "128^3 / VGA")
                        row["bit_equal"] = True
                    except AssertionError as e:
                        row["bit_equal"] = False
                        row["difference"] = str(e)[:200]
                        ok = False
                out[f"n{n}_{name}_{mname}"] = row
        ctx.set_timing(False)
        fu.close()
    for o in (rc, rs, cl, sp):
        o.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    with open(os.path.join(ROOT, "profiles", "raster_bench_line.json"), "w") as f:
        f.write(line + "\n")
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""TSDF ray casting on the device: the 36-pair VGA ring (10k, 10k + 3 degrees, D = 128, ground-truth poses) fused into
[-0.13, 0.13]^3 at 128^3 and 256^3 grid points, rendered from the first ring camera at 640 x 480 and at 1920 x 1080 with the
default step (voxel / 2).  Prints one JSON line and writes it to profiles/raycast_bench_line.json.

  render_ms          HIP events around k_rc_render (sfmx_raycast_last_us), mean over `calls` after one warm-up call
  samples            samples the kernel evaluated: inside the grid, up to each ray's hit (counted on the device)
  ns_per_ksample     render time per thousand of them
  bytes              algorithmic: the volume read once (12 B per grid point) plus the outputs written once (57 B per pixel)
  frac_hbm           bytes / render time / 6.3 TB/s
  --check            the 128^3 / VGA render compared bit for bit with tests/raycast_ref.py (NumPy, every sample of every ray)
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
HBM_BPS = 6.3e12


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
    rc = ctx.raycast()
    for n in (128, 256):
        vol = dict(origin=(-0.13, -0.13, -0.13), voxel=0.26 / (n - 1), dims=(n, n, n))
        fu = ctx.fusion(**vol)
        for r, d in views:
            fu.add_view(r, d)
        fu.integrate()
        ctx.set_timing(True)
        for name, cam in cams.items():
            rc.render(fu, cam, **march, read=False)  # warm-up
            us = []
            for _ in range(a.calls):
                rc.render(fu, cam, **march, read=False)
                us.append(rc.last_us())
            t = float(np.mean(us))
            res = rc.read()
            samples = rc.last_samples()
            nbytes = 12 * n ** 3 + 57 * cam["w"] * cam["h"]
            r = dict(render_ms=round(t / 1e3, 4), samples=samples, ns_per_ksample=round(t * 1e3 / (samples / 1e3), 3) if samples else None,
                     samples_per_ray=round(samples / (cam["w"] * cam["h"]), 1), hits=res["hits"], bytes=nbytes,
                     frac_hbm=round(nbytes / (t * 1e-6) / HBM_BPS, 4))
            if a.check and n == 128 and name == "640x480":
                import raycast_ref as RR
                s, cnt = fu.read()
                ref = RR.brute(s, cnt, vol["origin"], vol["voxel"], cam, cam["w"], cam["h"], **march)
                r["bit_equal"] = bool(RR.same(res, ref))
            out[f"n{n}_{name}"] = r
        ctx.set_timing(False)
        fu.close()
    rc.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    with open(os.path.join(ROOT, "profiles", "raycast_bench_line.json"), "w") as f:
        f.write(line + "\n")
    if a.check and not out["n128_640x480"]["bit_equal"]:
        sys.exit(1)


if __name__ == "__main__":
    main()

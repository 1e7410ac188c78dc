#!/usr/bin/env python3
"""Appearance of the fused surface on the device: the 36-pair VGA ring of tools/bench_fusion.py (10k, 10k + 3 degrees,
D = 128, ground-truth poses) fused into [-0.13, 0.13]^3 at 128^3 and 256^3 grid points, then normals and vertex grey.
Prints one JSON line.

  normals_us        HIP events around k_fu_emit_normals inside sfmx_fusion_extract_normals (sfmx_fusion_normals_us),
                    mean over `calls` after one warm-up call
  extract_us        the whole device extraction of that call without the normals kernel (the column of DESIGN.md 13)
  shade_us          HIP events around k_sh_shade inside sfmx_shade_fusion on the resident vertices, 36 views, depth_tol =
                    trunc, cull on (sfmx_shade_last_us), mean over `calls` after one warm-up call
  shade_call_ms     host clock around that call: the kernel and the two result copies
  normals_bytes     algorithmic: mask + offset of every grid point (8 B), the volume at most once (12 B per point),
                    24 B per vertex written
  shade_bytes       algorithmic: 48 B read and 5 B written per vertex, 3 B per accepted view lookup (disparity + pixel; the
                    rejected lookups read 2 B more each and are not counted)
  *_frac_hbm        bytes / time / 6.3 TB/s
  --check           the 128^3 normals, grey and view counts compared bit for bit with tests/appearance_ref.py (NumPy, device
                    disparity maps and rectified images)
Run on the GPU box."""
import argparse
import importlib
import json
import os
import sys
import time

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
    pairs = [(2 * k, 2 * k + 1) for k in range(36)]
    ctx = capi.Context(0)
    st = ctx.stereo(640, 480)
    views = []
    for i, j in pairs:
        r = pipeline.stereo_rectify(seq["K"], poses[i], poses[j], 640, 480)
        il, ir = (seq["images"][j], seq["images"][i]) if r["swapped"] else (seq["images"][i], seq["images"][j])
        d = st.disparity(il, ir, r["H_l"], r["H_r"], want_rect=True)
        views.append((r, d["disp16"], d["rect"][0].copy()))
    st.close()
    sh = ctx.shade()
    for r, d, im in views:
        sh.add_view(r, d, im)
    out = {"calls": a.calls, "pairs": 36}
    for n in (128, 256):
        vol = dict(origin=(-0.13, -0.13, -0.13), voxel=0.26 / (n - 1), dims=(n, n, n))
        tol = 4.0 * vol["voxel"]
        fu = ctx.fusion(**vol)
        for r, d, _ in views:
            fu.add_view(r, d)
        fu.integrate()
        ctx.set_timing(True)
        nrm_us, ext_us, shade_us, shade_wall = [], [], [], []
        for k in range(a.calls + 1):  # the first call allocates: not counted
            v, f, nr = fu.extract_normals()
            t0 = time.perf_counter()
            g, c = sh.shade_fusion(fu, len(v), tol)
            wall = (time.perf_counter() - t0) * 1e3
            if k:
                nrm_us.append(fu.normals_us())
                ext_us.append(fu.last_us() - fu.normals_us())
                shade_us.append(sh.last_us())
                shade_wall.append(wall)
        ctx.set_timing(False)
        fu.close()
        N, nv = n ** 3, len(v)
        nb, sb = 20 * N + 24 * nv, 53 * nv + 3 * int(c.sum())
        nus, sus = float(np.mean(nrm_us)), float(np.mean(shade_us))
        r = dict(verts=nv, faces=len(f), normals_us=round(nus, 2), extract_us=round(float(np.mean(ext_us)), 2), shade_us=round(sus, 2),
                 shade_call_ms=round(float(np.mean(shade_wall)), 3), normals_bytes=nb, shade_bytes=sb,
                 normals_frac_hbm=round(nb / (nus * 1e-6) / HBM_BPS, 4) if nus else None,
                 shade_frac_hbm=round(sb / (sus * 1e-6) / HBM_BPS, 4) if sus else None,
                 projections=nv * 36, seen=round(float((c >= 1).mean()), 4), views_mean=round(float(c.mean()), 2))
        if a.check and n == 128:
            import appearance_ref as AR
            ref = AR.fuse(vol["origin"], vol["voxel"], vol["dims"], views)
            r["bit_equal"] = bool(ref["verts"].tobytes() == v.tobytes() and ref["normals"].tobytes() == nr.tobytes()
                                  and ref["grey"].tobytes() == g.tobytes() and ref["vertex_views"].tobytes() == c.tobytes())
        out[f"n{n}"] = r
    sh.close()
    ctx.close()
    print(json.dumps(out))
    if a.check and not out["n128"]["bit_equal"]:
        sys.exit(1)


if __name__ == "__main__":
    main()

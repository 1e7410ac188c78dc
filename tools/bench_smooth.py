#!/usr/bin/env python3
"""Exact Taubin lambda|mu smoothing of the fused surface on the device: the 36-pair VGA ring of tools/bench_fusion.py (10k, 10k + 3
degrees, D = 128, ground-truth poses) fused into [-0.13, 0.13]^3 at 128^3 and 256^3 grid points, extracted with normals, cleaned
(sfmx_clean_fusion, defaults), then smoothed where the cleaning left it (sfmx_smooth_clean, --iters pairs, unit = the voxel, the
volume's origin).  Prints one JSON line and writes it to --out (default profiles/smooth_bench_line.json).

  smooth_us         HIP events from the first to the last launch of one sfmx_smooth_clean (sfmx_smooth_last_us), mean and min
                    over `calls` after one warm-up call.  The read-back of the flag and the edge counts lies between the table
                    kernels and the rest, so the host's round trip for it is inside the figure
  smooth_call_ms    host clock around the same call (the launches, the two read-backs and their synchronisations)
  clean_us, simplify_us  sfmx_clean_fusion and sfmx_simplify_clean (2 voxels) on the same surface in the same run: the yardsticks
  ratio_to_clean, ratio_to_simplify  smooth_us over each
  step_us           one k_sm_step launch: (smooth_us at iters + 1 minus smooth_us at iters) / 2
  step_bytes        what a step reads and writes: the Q array once (24 n), the CSR columns once (8 edges) and one 24-byte
                    gather per neighbour (48 edges)
  copy_us           a device-to-device copy of step_bytes bytes timed with events in the same run (mean of `calls`), and
  step_to_copy      step_us / copy_us
  --check           the 128^3 result (vertices, flags, the five counts) compared byte for byte with tests/smooth_ref.py (NumPy)
  --build-dir       load the libraries from another build directory of the package (a diagnostic build, e.g.
                    make -C <pkg>/csrc OUT=<pkg>/_build_diag HIPFLAGS_EXTRA=-DSFMX_SM_HASHED_ONLY hip host: the edge table with
                    hashed places only, the A/B of DESIGN.md 21)
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


def copy_us(nbytes, calls):
    import torch
    a = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda:0")
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    us = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return float(np.mean(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--build-dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_bench_line.json"))
    a = ap.parse_args()
    capi = importlib.import_module(PKG + ".capi")
    pipeline = importlib.import_module(PKG + ".pipeline")
    synth = importlib.import_module(PKG + ".synth")
    if a.build_dir:
        d = os.path.join(ROOT, PKG, a.build_dir)
        capi.LIB_PATH, pipeline.HOST_LIB_PATH = os.path.join(d, "libsfmx.so"), os.path.join(d, "libsfmx_host.so")
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
    cl, sp, sm = ctx.clean(), ctx.simplify(), ctx.smooth()
    out = {"calls": a.calls, "pairs": 36, "iters": a.iters, "build": a.build_dir or "_build"}

    def timed(fn, last_us):
        fn()  # warm-up: the work buffers grow here
        us, wall = [], []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            got = fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            us.append(last_us())
        return got, us, wall

    for n in (128, 256):
        vol = dict(origin=(-0.13, -0.13, -0.13), voxel=0.26 / (n - 1), dims=(n, n, n))
        fu = ctx.fusion(**vol)
        for r, d in views:
            fu.add_view(r, d)
        fu.integrate()
        ctx.set_timing(True)
        v, f, nr = fu.extract_normals()
        cgot, cus, _ = timed(lambda: cl.fusion(fu), cl.last_us)
        _, pus, _ = timed(lambda: sp.clean(cl, cell=2 * vol["voxel"], origin=vol["origin"]), sp.last_us)
        kw = dict(unit=vol["voxel"], origin=vol["origin"])
        _, us1, _ = timed(lambda: sm.clean(cl, iters=a.iters + 1, **kw), sm.last_us)
        got, us, wall = timed(lambda: sm.clean(cl, iters=a.iters, **kw), sm.last_us)
        ctx.set_timing(False)
        mus, clean_us, simp_us = float(np.mean(us)), float(np.mean(cus)), float(np.mean(pus))
        step_us = (float(np.mean(us1)) - mus) / 2.0
        step_bytes = 24 * cgot["n_verts"] + 56 * got["edges"]
        cp = copy_us(step_bytes, a.calls)
        row = dict(verts=len(v), faces=len(f), verts_in=cgot["n_verts"], faces_in=cgot["n_faces"], **got,
                   smooth_us=round(mus, 2), smooth_us_min=round(float(np.min(us)), 2), smooth_call_ms=round(float(np.mean(wall)), 3),
                   clean_us=round(clean_us, 2), simplify_us=round(simp_us, 2),
                   ratio_to_clean=round(mus / clean_us, 3) if clean_us else None,
                   ratio_to_simplify=round(mus / simp_us, 3) if simp_us else None,
                   step_us=round(step_us, 2), step_bytes=step_bytes, copy_us=round(cp, 2), step_to_copy=round(step_us / cp, 3) if cp else None)
        if a.check and n == 128:
            import clean_ref as LR
            import smooth_ref as MR
            lref = LR.clean(v, f, nr)
            ref = MR.smooth(lref["verts"], lref["faces"], iters=a.iters, **kw)
            res = sm.read()
            row["bit_equal"] = bool(got == MR.counts(ref) and res["verts"].tobytes() == ref["verts"].tobytes()
                                    and res["flags"].tobytes() == ref["flags"].tobytes())
        fu.close()
        out[f"n{n}"] = row
    for o in (cl, sp, sm):
        o.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    if a.check and not out["n128"]["bit_equal"]:
        sys.exit(1)


if __name__ == "__main__":
    main()

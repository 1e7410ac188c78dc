"""Fresh-process runner of the BA range suite (tests/test_gpu_ba_range.py): the switches SFMX_BA_EXPAND, SFMX_BA_CHUNK,
SFMX_BA_NO_FUSE, SFMX_BA_NO_POLL and SFMX_BA_NO_WAVE_PRIO are read once per process, so each set of them gets a process of its own.

    python tests/ba_child.py <case set> <out.npz>

The parent puts the switches into the environment.  This process builds the named cases of ba_inputs.child_cases, runs build
(damped and undamped) and step on each and writes S, b, dx and the status per case; the parent compares them with the oracle."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_inputs as B  # noqa: E402
import helpers as H  # noqa: E402


def main(which, out_path):
    capi = importlib.import_module(H.PKG_NAME + ".capi")
    ctx = capi.Context(0)
    out = {}
    names = []
    for i, (name, prob) in enumerate(B.child_cases(which).items()):
        names.append(name)
        q = ctx.ba_problem(prob.W, prob.X, prob.ptr, prob.li, prob.uv)
        a = prob.kargs() + (B.HUBER0, B.LAMBDA0)
        out[f"{i}:S1"], out[f"{i}:b1"] = q.build(prob.poses, *a, True)
        out[f"{i}:S0"], out[f"{i}:b0"] = q.build(prob.poses, *a, False)
        rc, dx = q.step(prob.poses, *a)
        out[f"{i}:rc"], out[f"{i}:dx"] = np.array(rc), dx
        rc, dx = q.step(prob.poses, *a)  # once more: the step after a step (ring slots, ticket and sequence words reused)
        out[f"{i}:rc2"], out[f"{i}:dx2"] = np.array(rc), dx
        q.close()
    out["names"] = np.array(names)
    np.savez(out_path, **out)
    ctx.close()
    print(f"ba_child {which}: {len(names)} cases")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])

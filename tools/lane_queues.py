#!/usr/bin/env python3
"""Which hardware queue every lane's stream landed on, and how busy each queue was.

    python tools/lane_queues.py KERNEL_TRACE.csv [--passes N]     # a rocprofv3 --kernel-trace CSV of bench.py (no counters)
    python tools/lane_queues.py --queue-log LOG [--plan "T+ B+ ..."]  # stderr of a run with AMD_LOG_LEVEL=3 AMD_LOG_MASK=16

Trace mode prints per hardware-queue id the streams on it (stream id where the trace has one, else the launching thread), the
lane each belongs to, its kernels (name, calls, total ms), and the share of the traced span during which a kernel was running
on the queue.  Lanes are told apart by their kernels: k_ba_* is lane B, k_shi_* / k_flag_row_* / k_row_scan a prefetch worker,
k_klt_track with ~46 calls per pass the tracker, k_downsample2 alone the tracker's copy stream (pyramids); streams that run
only the RANSAC kernels are lanes A, A2, E, E2 or the geometry lane and are listed with their calls per pass.  The trace mode
has only ever read the synthetic trace of tests/test_lane_queues_tool.py: no real kernel trace of the benchmark could be taken
where this was written (profiles/lane_plan_ab.txt), so its column names and lane rules are unproven against rocprofv3's output.

Queue-log mode needs no profiler.  The HIP runtime logs the hardware queue it opened or picked for every stream it creates
("acquireQueue refCount: <queue> (1)" for a new queue, "Selected queue refCount: <queue> (<streams on it>)" for an existing
one); the lines come in creation order, so with the creation plan (--plan, the
order= part of the line SFMX_LANE_PLAN_PRINT=1 prints; default: whole pairs T B P C A E P2 A2 E2) the n-th helper stream is
known by name.  It prints the queue of every stream and the compute streams grouped by queue.  No timing in this mode."""
import argparse
import collections
import csv
import re
import sys

PARENT = "T- T+ B- B+ P- P+ C- C+ A- A+ E- E+ P2- P2+ A2- A2+ E2- E2+"


def lane_of(kernels, passes):
    names = set(kernels)
    if any(k.startswith("k_ba_") or "k_ba_" in k for k in names):
        return "B"
    if any("k_shi_" in k or "k_flag_row" in k or "k_row_scan" in k for k in names):
        return "P (prefetch worker)"
    klt = sum(c for k, (c, _) in kernels.items() if "k_klt_track" in k)
    if klt and passes and klt / passes >= 30:
        return "T (tracker)"
    if names and all("k_downsample2" in k or "rocclr" in k for k in names):
        return "T- (tracker's copy stream: pyramids)" if any("k_downsample2" in k for k in names) else "copies only"
    r = sum(c for k, (c, _) in kernels.items() if "k_hypotheses" in k)
    if r:
        return f"RANSAC lane (A/A2/E/E2/G): {r / max(1, passes):.1f} k_hypotheses per pass" + (f", {klt / max(1, passes):.1f} k_klt_track" if klt else "")
    return "?"


def trace_table(path, passes):
    rows = list(csv.DictReader(open(path, newline="")))
    if not rows:
        sys.exit("empty trace")
    col = {c.lower(): c for c in rows[0]}
    need = [col.get(k) for k in ("queue_id", "kernel_name", "start_timestamp", "end_timestamp")]
    if None in need:
        sys.exit(f"not a kernel trace: columns {list(rows[0])}")
    qc, nc, sc, ec = need
    stc = col.get("stream_id") or col.get("thread_id")
    t0 = min(int(r[sc]) for r in rows)
    t1 = max(int(r[ec]) for r in rows)
    span = max(1, t1 - t0)
    queues = collections.defaultdict(lambda: collections.defaultdict(lambda: collections.defaultdict(lambda: [0, 0.0])))
    iv = collections.defaultdict(list)
    for r in rows:
        s, e = int(r[sc]), int(r[ec])
        k = queues[r[qc]][r[stc] if stc else "?"][r[nc].split("(")[0][:60]]
        k[0] += 1
        k[1] += (e - s) / 1e6
        iv[r[qc]].append((s, e))
    print(f"# {path}: {len(rows)} kernels, span {span / 1e6:.1f} ms, {passes} passes assumed; streams keyed by {stc}")
    for q in sorted(queues, key=lambda x: (len(x), x)):
        busy, end = 0, 0
        for s, e in sorted(iv[q]):
            if e > end:
                busy += e - max(s, end)
                end = e
        print(f"queue {q}: a kernel was running {100.0 * busy / span:.1f} % of the span; {sum(c for st in queues[q].values() for c, _ in st.values())} kernels")
        for st, ks in sorted(queues[q].items(), key=lambda kv: -sum(v[1] for v in kv[1].values())):
            print(f"  stream {st}: {lane_of({k: tuple(v) for k, v in ks.items()}, passes)}")
            for k, (c, ms) in sorted(ks.items(), key=lambda kv: -kv[1][1]):
                print(f"      {k:<60} {c:>7} {ms:>10.3f} ms")


def queue_log_table(path, plan, skip=None):
    sel = []
    for line in open(path, errors="replace"):
        m = re.search(r"(?:Selected queue|acquireQueue) refCount: (0x[0-9a-f]+) \((\d+)\)", line)  # an existing queue | a new one
        if m:
            sel.append((m.group(1), int(m.group(2))))
    if not sel:
        sys.exit("no queue selection lines: run with AMD_LOG_LEVEL=3 AMD_LOG_MASK=16")
    names = ["G-", "G+"] + plan.split()
    ids = {}
    for q, _ in sel:
        ids.setdefault(q, len(ids))  # queues numbered in the order the runtime opened them
    print(f"# {path}: {len(sel)} streams placed on {len(ids)} hardware queues; plan: G- G+ {plan}")
    # the named streams are the LAST len(names); whatever the process made before them (the default stream) is listed as such
    if skip is None:
        skip = max(0, len(sel) - len(names))
    by = collections.defaultdict(list)
    for i, (q, n) in enumerate(sel):
        name = names[i - skip] if 0 <= i - skip < len(names) else ("(before the pipeline)" if i < skip else "(later)")
        print(f"  stream {i:2d}  {name:<22} -> queue {ids[q]} ({q}), {n} streams on it now")
        by[ids[q]].append(name)
    for q in sorted(by):
        print(f"queue {q}: compute {{{', '.join(n[:-1] for n in by[q] if n.endswith('+'))}}}  copy {{{', '.join(n[:-1] for n in by[q] if n.endswith('-'))}}}"
              f"  other {sum(1 for n in by[q] if n.startswith('('))}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trace", nargs="?")
    ap.add_argument("--passes", type=int, default=23, help="pipeline passes in the trace (bench.py --steps 20 --warmup 3: 23)")
    ap.add_argument("--queue-log")
    ap.add_argument("--plan", default=PARENT)
    ap.add_argument("--skip", type=int, default=None, help="queue-log mode: selections before the caller's copy stream (default: all but the plan's)")
    a = ap.parse_args()
    if a.queue_log:
        queue_log_table(a.queue_log, a.plan, a.skip)
    elif a.trace:
        trace_table(a.trace, a.passes)
    else:
        ap.error("a trace CSV or --queue-log")


if __name__ == "__main__":
    main()

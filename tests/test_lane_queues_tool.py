"""CPU suite: tools/lane_queues.py on a synthetic kernel trace and a synthetic runtime queue log (no GPU, no profiler)."""
import os
import subprocess
import sys

import helpers as H

TOOL = os.path.join(H.ROOT, "tools", "lane_queues.py")


def run(*args):
    p = subprocess.run([sys.executable, TOOL, *args], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def test_trace_mode_groups_streams_by_queue_names_lanes_and_measures_busy_share(tmp_path):
    rows = ["Kind,Agent_Id,Queue_Id,Stream_Id,Thread_Id,Dispatch_Id,Kernel_Id,Kernel_Name,Correlation_Id,Start_Timestamp,End_Timestamp"]
    n = 0

    def k(queue, stream, name, start, end):
        nonlocal n
        n += 1
        rows.append(f'KERNEL_DISPATCH,1,{queue},{stream},100,{n},1,"{name}",{n},{start},{end}')  # names are quoted: they hold commas

    for i in range(40):                                     # one pass: queue 1 carries lane B and a RANSAC lane, queue 2 the tracker
        k(1, 11, "k_ba_reduce<32>(double*)", 1000 * i, 1000 * i + 100)
        k(2, 21, "void k_klt_track<5, false, true, true>(P)", 1000 * i, 1000 * i + 500)
    k(1, 12, "void k_hypotheses<true, false>(P)", 50, 150)   # overlaps the first BA kernel by 50 ns: the union counts it once
    k(3, 31, "k_shi_tile(P)", 0, 40000)
    k(3, 32, "k_downsample2(P)", 10, 20)
    path = tmp_path / "trace.csv"
    path.write_text("\n".join(rows) + "\n")
    out = run(str(path), "--passes", "1")
    blocks = {b.split(":")[0]: b for b in out.split("queue ")[1:]}
    assert set(blocks) == {"1", "2", "3"}
    span = 40000.0
    assert f"{100.0 * (40 * 100 + 50) / span:.1f} % of the span" in blocks["1"] and "stream 11: B" in blocks["1"]
    assert "stream 12: RANSAC lane" in blocks["1"] and "1.0 k_hypotheses per pass" in blocks["1"]
    assert f"{100.0 * 40 * 500 / span:.1f} % of the span" in blocks["2"] and "stream 21: T (tracker)" in blocks["2"]
    assert "100.0 % of the span" in blocks["3"] and "stream 31: P (prefetch worker)" in blocks["3"] and "stream 32: T- " in blocks["3"]
    assert "k_ba_reduce<32>" in blocks["1"] and "     40 " in blocks["1"]


def test_queue_log_mode_names_streams_by_creation_order(tmp_path):
    q = ["0xd00", "0xc00", "0xb00", "0xa00"]      # opened in this order; afterwards least loaded, ties to the lowest address
    lines = [f":3: : Created SWq=0x1 to map on HWq={a} with size 16384\n:3: : acquireQueue refCount: {a} (1)" for a in q]
    load = {a: 1 for a in q}
    for _ in range(5):                               # five more streams
        a = min(sorted(load), key=lambda x: load[x])
        load[a] += 1
        lines.append(f":3: : Number of allocated hardware queues\n:3: : Selected queue refCount: {a} ({load[a]})")
    path = tmp_path / "log.txt"
    path.write_text("\n".join(lines) + "\n")
    out = run("--queue-log", str(path), "--plan", "T+ B+ P+ T- B- P-")
    assert "9 streams placed on 4 hardware queues" in out
    assert "stream  0  (before the pipeline)  -> queue 0 (0xd00)" in out
    assert "G-                     -> queue 1" in out and "G+                     -> queue 2" in out
    assert "T+                     -> queue 3 (0xa00), 1 streams" in out and "B+                     -> queue 3 (0xa00), 2 streams" in out
    assert "queue 3: compute {T, B}  copy {P}  other 0" in out and "queue 2: compute {G, P}  copy {}  other 0" in out

"""CPU suite: csrc/host/lane_plan.hpp, the order in which the pipeline creates the streams of its helper contexts, driven through a
stand-alone program (tests/lane_plan_main.cpp) built with the host compiler -- once plainly, once with AddressSanitizer and
UBSan.  Every check runs on both builds.  No GPU, no library.  The queue groups are those of the driver's MODEL of the runtime's
placement (new queue first, then least loaded, ties to the queue opened last), which is what the runtime's queue log showed
(profiles/lane_plan_ab.txt); the table keeps the named orders and the groups their comments state consistent with that model."""
import os
import subprocess

import pytest

import helpers as H

HOST = os.path.join(H.ROOT, H.PKG_NAME, "csrc", "host")
ROLES = ("P", "T", "B", "C", "A", "E", "P2", "A2", "E2")
STREAMS = {r + k for r in ROLES for k in "+-"}
PARENT_ORDER = "T- T+ B- B+ P- P+ C- C+ A- A+ E- E+"
PARENT_FIRST_USE = ["P2", "A2", "E2"]
NAMED = ("parent", "b_own", "as8", "b_alone", "crit")
DEFAULT_AT_4 = "as8"
# Compute streams that share a hardware queue at four queues, G = the caller's (geometry) context, in a process that made one
# stream before the caller's (the default stream: the benchmark's case, checked against the runtime's queue log in
# profiles/lane_plan_ab.txt).  Second entry: the lane whose queue the tracker's copy stream (T-, the pyramid builds: the one busy
# copy stream) shares; None = a queue without compute streams.
GROUPS_AT_4 = {
    "b_own": ([{"B"}, {"T", "P", "P2", "C"}, {"G", "A", "A2", "E", "E2"}], None),
    "as8": ([{"G", "C", "A2"}, {"T", "A", "E2"}, {"B", "E"}, {"P", "P2"}], "T"),
    "b_alone": ([{"B"}, {"T", "G"}, {"P", "P2", "C"}, {"A", "A2", "E", "E2"}], "T"),
    "crit": ([{"B", "G"}, {"T"}, {"P", "P2", "C"}, {"A", "A2", "E", "E2"}], "T"),
    "parent": ([{"T", "P", "A", "P2", "E2"}, {"B", "C", "E", "A2"}, {"G"}], "T"),
}


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def prog(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lane_plan") / f"lane_plan_{request.param}")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if request.param != "plain" else []
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", HOST, "-o", out,
                    os.path.join(H.ROOT, "tests", "lane_plan_main.cpp")], check=True)
    return out


def run(prog, *args):
    p = subprocess.run([prog, *args], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not p.stderr, (args, p.returncode, p.stderr[-2000:])
    return p.stdout


def plan(prog, queues, override="NONE"):
    return dict(l.split("=", 1) for l in run(prog, "plan", str(queues), override).splitlines())


def groups(prog, queues, override="NONE", prior=1):
    cls = dict((a, int(b)) for a, b in (l.split() for l in run(prog, "classes", str(queues), override, str(prior)).splitlines()))
    assert set(cls) == STREAMS | {"G+", "G-"} and min(cls.values()) >= 0
    by = {}
    for s, c in cls.items():
        if s.endswith("+"):
            by.setdefault(c, set()).add(s[:-1])
    return cls, by


def test_named_plans_are_the_documented_ones(prog):
    assert tuple(run(prog, "names").split()) == NAMED


def test_every_stream_exactly_once_for_every_count_and_plan(prog):
    rows = run(prog, "sweep").splitlines()
    assert len(rows) == 32 * (1 + len(NAMED))
    for row in rows:
        head, order, first_use = [x.strip() for x in row.split("|")]
        queues, asked, name = head.split()
        warm = order.split()
        lazy = first_use.split()
        assert len(warm) == len(set(warm)) and set(warm) <= STREAMS, row          # no duplicate; the caller's G is not a role
        assert len(lazy) == len(set(lazy)) and set(lazy) <= set(ROLES), row
        assert sorted(warm + [r + k for r in lazy for k in "-+"]) == sorted(STREAMS), row   # warm-up + first use = each exactly once
        assert name == (asked if asked != "NONE" else (DEFAULT_AT_4 if queues == "4" else "parent")), row
        if name == "parent":   # whatever the count
            assert order == PARENT_ORDER and lazy == PARENT_FIRST_USE, row
        else:
            assert not lazy, row  # the plans for four queues leave nothing to first use


def test_every_count_but_four_keeps_the_parent_order(prog):
    for q in list(range(1, 4)) + list(range(5, 33)):
        p = plan(prog, q)
        assert (p["name"], p["default"], p["order"], p["first_use"].split(), p["message"]) == ("parent", "1", PARENT_ORDER, PARENT_FIRST_USE, ""), q
    p = plan(prog, 4, "parent")
    assert (p["name"], p["default"], p["order"], p["first_use"].split()) == ("parent", "0", PARENT_ORDER, PARENT_FIRST_USE)
    assert plan(prog, 4)["name"] == DEFAULT_AT_4 and plan(prog, 4)["default"] == "1"


@pytest.mark.parametrize("name", sorted(GROUPS_AT_4))
def test_classes_at_four_queues(prog, name):
    want, tcopy_with = GROUPS_AT_4[name]
    cls, by = groups(prog, 4, name)
    assert sorted(map(sorted, by.values())) == sorted(map(sorted, want))
    assert (cls["G-"], cls["G+"]) == (1, 2)  # after the one earlier stream
    if tcopy_with:
        assert cls["T-"] == cls[tcopy_with + "+"]
    else:
        assert cls["T-"] not in by
    if name == DEFAULT_AT_4:
        assert groups(prog, 4)[0] == cls
    if name == "b_own":
        assert {s for s, c in cls.items() if c == cls["B+"]} == {"B+", "B-", "G-", "A-", "A2-"}  # lane B beside idle copy streams only


def test_placement_rule_new_queue_first_then_least_loaded_ties_to_the_newest(prog):
    """the streams of the parent order at four queues, one earlier stream: the sequence read from the runtime's queue log"""
    cls, _ = groups(prog, 4, "parent")
    order = ["G-", "G+"] + (PARENT_ORDER + " P2- P2+ A2- A2+ E2- E2+").split()
    assert [cls[s] for s in order] == [1, 2, 3, 3, 2, 1, 0, 3, 2, 1, 0, 3, 2, 1, 0, 3, 2, 1, 0, 3]
    cls0, _ = groups(prog, 4, "parent", prior=0)   # no earlier stream: the caller's pair opens the first two queues
    assert [cls0[s] for s in order[:8]] == [0, 1, 2, 3, 3, 2, 1, 0]
    cls1, by1 = groups(prog, 1, "parent")
    assert set(cls1.values()) == {0} and len(by1) == 1
    _, by8 = groups(prog, 8)   # eight queues, the parent order: lane B has a queue without another compute stream there too
    assert sorted(map(sorted, by8.values())) == sorted(map(sorted, [{"P", "P2"}, {"B"}, {"C", "A2"}, {"T"}, {"A", "E2"}, {"G"}, {"E"}]))


def test_queue_count_from_the_environment_value(prog):
    assert run(prog, "queues").strip() == "4"          # unset: the runtime's default
    for v, want in (("4", 4), ("8", 8), ("32", 32), ("1", 1), ("", 4), ("0", 4), ("-3", 4), ("abc", 4), ("8x", 4)):
        assert int(run(prog, "queues", v)) == want, v


@pytest.mark.parametrize("order", [
    "T+ B+ P+ C+ A+ E+ P2+ A2+ E2+ T- B- P- C- A- E- P2- A2- E2-",
    "T+ P+ A+ B+ T- P2+ A2+ B- C- C+ E+ A- E- P- E2+ A2- E2- P2-",
    "E2- E2+ T- T+",
    "B+ T+ T- B- P2- P2+",
    PARENT_ORDER,
])
def test_spelled_override_round_trips(prog, order):
    p = plan(prog, 4, order)
    assert (p["name"], p["default"], p["order"], p["message"]) == ("custom", "0", order, "")
    again = plan(prog, 8, p["order"].replace(" ", ", "))   # commas and blanks both separate
    assert again["order"] == order and again["first_use"] == p["first_use"]
    warm = order.split()
    assert sorted(warm + [r + k for r in p["first_use"].split() for k in "-+"]) == sorted(STREAMS)
    assert f"order={order}" in p["describe"] and p["describe"].startswith("custom (override) queues=4 ")


@pytest.mark.parametrize("bad,why", [
    ("", "empty"), ("   ", "empty"), ("T+ X+ T- X-", "unknown role"), ("T+ T+ T-", "twice"), ("T+ B+ B-", "one of its two streams"),
    ("TB", "not ROLE+"), ("T", "not ROLE+"), ("as9", "not ROLE+"), ("G+ G-", "unknown role"), ("T+ t-", "unknown role"), ("+", "not ROLE+"),
])
def test_malformed_override_falls_back_with_a_message(prog, bad, why):
    for q in (4, 8):
        p = plan(prog, q, bad)
        d = plan(prog, q)
        assert why in p["message"] and "rejected" in p["message"] and "using the default" in p["message"], p["message"]
        assert (p["name"], p["default"], p["order"], p["first_use"]) == (d["name"], "1", d["order"], d["first_use"])

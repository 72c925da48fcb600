"""Kernel selection of the WaveNet layers on the host (csrc/wn_plan.h), without a GPU: a stand-alone program on the planner
header alone prints the plan of every case of tests/tools/wn_plan_cases.h, and the rows are compared with
tests/golden/wn_plan_expected.txt.

The expected table was printed by the selection code of the commit in front of the planner -- gate_shape_policy,
resskip_shape_policy, every launcher's fit expression and selection tail, and the try-and-fall-back cascades of the forward,
copied into a throw-away program that is not kept -- never by the code under test.  Rows: C in {64, 320, 340, 512} x 600 / 4 800 /
16 000 rows per item x batch 1 / 2 / 8 / 16 (full_blocks = 1024, the 5 040 blocks of the two-tile shape and the half_blocks
256 window are crossed), dilations 1 / 16 / 64 / 2048 (sub-sequences of at most 128 rows included), tune_gate_shape 0-4,
batch_invariant, cond_up 4 / 5 / 9 / 10 (the CR 28 / 56 / none edges), streamed and per-layer-span launches, causal padding,
the wave-tile bound at, below and above the tile count, np 10-13, an odd column-tile count under the two-tile shape, the
un-folded graph, and split half precision with and without planes and with each dynamic-LDS bit cleared.

The one intended difference: a split-precision handle whose gates do not take the planes at some layer (cond_up = 9, or the
device refused the LDS size of wn_gate_f16_kernel).  The earlier code decided "the planes are the hidden state" from weaker
conditions than its launchers checked and failed from the middle of the network (status 1); the plan is complete there,
keeps the float32 hidden state and runs the float32 gate kernels."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mbexwn_vocoder_amd", "csrc")
TOOLS = os.path.join(ROOT, "tests", "tools")
EXPECTED = os.path.join(ROOT, "tests", "golden", "wn_plan_expected.txt")
SPLIT_GATES = {"9", "10", "11"}       # MBX_GATE_K_SPLIT_F16, _WIDE, _F32H


def _table(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC, "-I", TOOLS,
                    os.path.join(TOOLS, "wn_plan_table.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    return _table(tmp_path_factory.mktemp("wn_plan"), "wn_plan_table", ["-O1"])


def _fields(line):
    parts = [pp.strip() for pp in line.split("|")]
    return parts[0], dict(pp.split("=", 1) for pp in parts[1:])


def _intended(name):
    """split gates asked for, and either cond_up = 9 (31 conditioning rows per 256-row block, the kernel holds 28) or the
    LDS bit of wn_gate_f16_kernel cleared (lds6 = all bits but WN_LDS_GATE_F16)"""
    return name.startswith("split-s2-") and (name.endswith("-up9") or "-lds6-" in name)


def test_plan_table_matches_the_selection_of_the_commit_before_the_planner(rows):
    want = open(EXPECTED).read().splitlines()
    assert len(rows) == len(want) > 900
    differ = []
    for got, exp in zip(rows, want):
        name, gf = _fields(got)
        ename, ef = _fields(exp)
        assert name == ename
        if got != exp:
            differ.append(name)
            # the intended difference, and nothing else: the earlier code refused, the plan is complete on float32 gates
            assert _intended(name), (got, exp)
            assert ef == {"st": "1"} and gf["st"] == "0" and gf["po"] == "0", (got, exp)
            gates = [gg.split("/")[0] for gg in gf["g"].split()]
            assert gates[0] == "8" and not set(gates[1:]) & SPLIT_GATES, got
            assert set(gf["r"].split()[:-1]) == {"11"}, got         # the res/skip layers stay in split precision
    # every row the description names as an intended difference that the earlier code could reach with the planes as the
    # hidden state differs (the others -- no split image on layer 0 -- ran without the planes before, and agree)
    assert differ and all(_intended(nn) for nn in differ)
    assert {nn for nn in differ} == {_fields(ll)[0] for ll in want if _intended(_fields(ll)[0]) and "-no00-" in ll}


def test_plan_table_covers_the_edges(rows):
    """The table reaches every gate, res/skip and tail kernel code and both refusals, so a row that stops
    exercising its edge shows here rather than as a silently weaker table."""
    gates, shapes, res, tails, status, planes = set(), set(), set(), set(), set(), set()
    for line in rows:
        _, ff = _fields(line)
        status.add(ff["st"])
        if ff["st"] != "0":
            continue
        for gg in ff["g"].split():
            parts = gg.split("/")
            gates.add(int(parts[0]))
            if len(parts) > 1:
                shapes.add((int(parts[1]), int(parts[2]), int(parts[3]), int(parts[4])))
        res |= {int(rr) for rr in ff["r"].split()}
        tails.add(ff["tail"])
        planes.add(ff["po"])
    assert gates == set(range(1, 12)) and res == set(range(0, 12))
    assert {ss[:2] for ss in shapes} == {(0, 32), (1, 32), (2, 16), (3, 64)}
    assert {ss[2] for ss in shapes} == {28, 56} and {ss[3] for ss in shapes} == {0, 1, 2}
    assert tails >= {"1/0", "2/1", "3/1", "4/1", "5/1", "6/1", "7/1", "5/0"}
    assert status == {"0", "1", "4"} and planes == {"0", "1"}


def test_plan_table_under_sanitizers(tmp_path, rows):
    """The same program built with the address and undefined-behaviour sanitizers (a stand-alone host binary) runs clean
    and prints the same table."""
    assert _table(tmp_path, "wn_plan_table_san", ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]) == rows

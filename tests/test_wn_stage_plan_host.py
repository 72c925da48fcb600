"""Which instantiation of the F(4,3) gate kernels every stage case launches, without a GPU.

The kernel report names a layer's kernel ("f43", "f43_psplit", ...), which carries neither the block shape (one or two column
tiles), the conditioning rows (CR 28 | 56), the sub-sequences per block (VS 1 | 2) nor the gate's template argument (0 gtu | -1
the others): test_gpu_wavenet_stages.test_gpu_cases_cover_every_gate_kernel cannot see an instantiation that no case
launches.  tests/tools/wn_plan_stage_cases.cpp, a stand-alone host program on csrc/wn_plan.h, prints each layer's kernel /
shape / block_channels / cr / vs_arg for the model, lengths and policy of every stage case; with the model's activation a row
names the instantiation launch_wn_gate_winograd4w launches, and the union over the cases must be every instantiation on
that launcher's hipLaunchKernelGGL lines -- a new instantiation without a case fails here.  On the GPU every stage case
asserts that the rows are what its forward reports."""
import pytest

import test_gpu_wavenet_stages as twn
import wn_stage_plan as wsp

Q, W, P, H = "wn_gate_winograd4q_kernel", "wn_gate_winograd4w_kernel", "wn_gate_winograd4p_kernel", "wn_gate_winograd4h_kernel"


@pytest.fixture(scope="module")
def cases():
    return wsp.stage_case_lines(twn)


@pytest.fixture(scope="module")
def rows(tmp_path_factory, cases):
    return wsp.run(wsp.build(tmp_path_factory.mktemp("wn_stage_plan")), cases[0])


def _launched(rows, model, cid):
    C, act = model[cid]
    return set().union(*(wsp.instantiations(row, C, act) for row in rows[cid]))


def test_stage_cases_launch_every_f43_instantiation(rows, cases):
    _, model = cases
    named = wsp.launcher_instantiations()
    assert len(named) == 16 and {nn.split("<")[0] for nn in named} == {Q, W, P, H}
    by_case = {case[0]: _launched(rows, model, case[0]) for case in twn.CASES}
    reached = set().union(*by_case.values())
    assert reached <= named, sorted(reached - named)
    assert reached == named, f"no stage case launches {sorted(named - reached)}"
    # the cases that are there for one instantiation reach it
    for cid, want in {"gfu-f43-256row": {f"{W}<28,-1>"}, "gfu-f43-hsplit": {f"{H}<-1>"}, "lin5-c64-gfu-f43": {f"{W}<56,-1>"},
                      "deep9-c64-gfu-f43": {f"{H}<-1>", f"{P}<-1,1>"},
                      "deep9-c64-gfu-invariant": {f"{W}<28,-1>", f"{P}<-1,1>", f"{W}<28,-1,1>", f"{W}<28,-1,2>"},
                      "gfu-two-tile": {f"{Q}<-1>"}, "gsu-two-tile": {f"{Q}<-1>"}, "glu-two-tile": {f"{Q}<-1>"},
                      "speech-two-tile": {f"{Q}<0>"}, "voice-two-tile": {f"{Q}<0>", f"{W}<28,0>"},
                      "c68-two-tile": {f"{Q}<0>", f"{W}<28,0>"}, "c36-two-tile": {f"{Q}<0>"},
                      "lin5-two-tile-refused": {f"{W}<56,0>"}, "large-f43": {f"{Q}<0>"}}.items():
        assert by_case[cid] == want, (cid, sorted(by_case[cid]))


def test_stage_case_rows_are_what_the_cases_declare(rows):
    """The rows agree with what the cases expect of the report: kernel names per case, and the block channels where a case
    declares them (the GPU run holds both to the forward itself)."""
    from mbexwn_vocoder_amd.engine import GATE_KERNEL_NAMES
    for cid, _, _, _, kernels in twn.CASES:
        assert {GATE_KERNEL_NAMES[row[0]] for row in rows[cid]} == kernels, (cid, rows[cid])
        if cid in twn.BLOCK_CHANNELS:
            assert [row[2] for row in rows[cid]] == twn.BLOCK_CHANNELS[cid], (cid, rows[cid])
    # the shape of every layer of a two-tile case behind a folded first one is 3; the refused one falls back to shape 0, CR 56
    for cid in twn.TWO_TILE:
        assert {row[1] for row in rows[cid] if row[2]} == {3} and {row[3] for row in rows[cid] if row[2]} == {28}, (cid, rows[cid])
    assert {row[1:4] for row in rows["lin5-two-tile-refused"]} == {(0, 32, 56)}


def test_stage_plan_program_under_sanitizers(tmp_path, rows, cases):
    """The same program built with the address and undefined-behaviour sanitizers (a stand-alone host binary) runs clean
    and prints the same rows."""
    exe = wsp.build(tmp_path, "wn_plan_stage_cases_san", ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert wsp.run(exe, cases[0]) == rows

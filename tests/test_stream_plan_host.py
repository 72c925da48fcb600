"""The streaming driver on the CPU, call by call: tests/tools/record_stream_calls.py drives StreamingSynthesizer with a
recording test double of the engine through eight scenarios; every argument of every engine call must equal
tests/golden/stream_calls.json (recorded before the tick was split into plan / upload / commit), the streamed audio
the closed form of the double, and stream_plan.plan_tick alone -- no synthesizer, no tensor, no engine -- must give
the recorded arguments from stream fields written out by hand."""
import importlib.util
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_recorder():
    spec = importlib.util.spec_from_file_location("record_stream_calls",
                                                  os.path.join(ROOT, "tests", "tools", "record_stream_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


recorder = _load_recorder()
STEADY = {"chunk8": True, "schedule_80ms": True, "chunk5": True, "chunk2": False, "force_causal": True, "pitch": True,
          "chunk8_graph": True, "no_layer_state": False}


@pytest.fixture(scope="module")
def golden():
    with open(recorder.FIXTURE) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def runs():
    """Every scenario, run once: name -> (record, streamed audio, closed-form audio)."""
    return {name: recorder.run_scenario(name) for name in recorder.SCENARIOS}


def test_fixture_holds_every_scenario(golden):
    assert sorted(golden) == sorted(recorder.SCENARIOS) == sorted(STEADY)
    assert os.path.getsize(recorder.FIXTURE) < 200 * 1024


def _differences(want, got, path):
    """Paths at which two JSON values differ (field by field, no tolerance)."""
    if isinstance(want, dict) and isinstance(got, dict):
        return [dd for kk in sorted(set(want) | set(got))
                for dd in (_differences(want[kk], got[kk], f"{path}.{kk}") if kk in want and kk in got else [f"{path}.{kk}"])]
    if isinstance(want, list) and isinstance(got, list) and len(want) == len(got):
        return [dd for ii, (ww, gg) in enumerate(zip(want, got)) for dd in _differences(ww, gg, f"{path}[{ii}]")]
    return [] if want == got and type(want) is type(got) else [f"{path}: {got!r} != recorded {want!r}"]


@pytest.mark.parametrize("name", sorted(recorder.SCENARIOS))
def test_engine_calls_equal_the_recording(name, golden, runs):
    got = json.loads(json.dumps(runs[name][0]))               # (tuples -> lists, as the fixture went through JSON)
    want = golden[name]
    assert len(got["ticks"]) == len(want["ticks"])
    diff = _differences(want, got, name)
    assert not diff, "\n".join(diff[:20])


@pytest.mark.parametrize("name", sorted(recorder.SCENARIOS))
def test_streamed_audio_is_the_closed_form(name, runs):
    """2e-5: the float32 sums of the double against numpy's (the bar of test_shared_input_rows_drop_and_grow)."""
    _, audio, want = runs[name]
    for sid in want:
        assert audio[sid].shape == want[sid].shape, (name, sid)
        np.testing.assert_allclose(audio[sid], want[sid], rtol=0, atol=2e-5, err_msg=f"{name} {sid}")


@pytest.mark.parametrize("name", sorted(STEADY))
def test_steady_ticks_where_they_belong(name, golden, runs):
    """A steady tick (layer_rows > 0: every WaveNet layer on the new rows only) needs the layer state and new rows of at
    least min_rows: chunk 2 (40 rows < 48) and a double without layer state have none, the other scenarios some."""
    for record in (golden[name], runs[name][0]):
        steady = [tt["layer_rows"] for tt in record["ticks"] if tt["layer_rows"] > 0]
        assert bool(steady) == STEADY[name], (name, steady)
        assert all(tt["call"]["layers"]["rows"] == tt["layer_rows"] for tt in record["ticks"] if tt["layer_rows"] > 0)


def test_control_keywords_appear_with_the_first_transposition(runs):
    """Stream "r" pushes 8 frames per tick and its transposition leaves 1 at frame 72: the push of tick 9 flips the sticky
    flag, inside a run of steady ticks; every call from there on carries the three keywords, none before."""
    ticks = runs["pitch"][0]["ticks"]
    flip = recorder.SCENARIOS["pitch"]["transposition_from"]["r"] // 8
    carried = [sorted(tt["call"]["pitch"]) for tt in ticks if tt["call"] is not None]
    assert all(tt["call"] is not None for tt in ticks[:flip + 1])
    assert carried[:flip] == [[]] * flip and carried[flip:] == [sorted(recorder.CONTROL)] * (len(carried) - flip)
    assert ticks[flip - 1]["layer_rows"] > 0 and ticks[flip]["layer_rows"] > 0
    # "p" (external F0 frames, mask 1) joins later, next to two streams that keep the F0-net
    masks = {tuple(tt["call"]["pitch"]["f0_item_mask"]) for tt in ticks[flip:]}
    assert (0, 0) in masks and (0, 0, 1) in masks


def test_failed_capture_falls_back_to_launches(runs, capfd):
    """use_graph left on, on a host whose capture fails: the first recorded phase that comes round again tries the capture,
    prints one line, turns use_graph off, and the tick runs launch by launch -- the same calls as without graphs."""
    capfd.readouterr()
    record, _, _ = recorder.run_scenario("chunk8_graph")
    err = capfd.readouterr().err
    assert err.count("hipGraph capture of the steady tick failed") == 1
    plain = runs["chunk8"][0]["ticks"]
    ticks = record["ticks"]
    off = [ii for ii, tt in enumerate(ticks) if not tt["use_graph"]]
    assert off and off == list(range(off[0], len(ticks))) and off[0] > 0
    assert ticks[off[0] - 1]["layer_rows"] > 0                  # the tick before was steady: it recorded the phase
    assert all(tt["graph_ticks"] == 0 and not tt["replayed"] for tt in ticks)
    assert [tt["call"] for tt in ticks] == [tt["call"] for tt in plain]
    assert [(tt["ids"], tt["lens"]) for tt in ticks] == [(tt["ids"], tt["lens"]) for tt in plain]


# ----------------------------------------------------------------------------------------------------------------------
# plan_tick on its own
# ----------------------------------------------------------------------------------------------------------------------
def _geometry(name):
    """The geometry of the canonical model (margins: test_canonical_margins) and of the small force_causal one (the table in
    streaming.stream_margins), at 8-frame ticks; min_rows and the ring (64 >= 10 + 8 + 11 + 32 frames) are the double's."""
    from mbexwn_vocoder_amd.stream_plan import StreamGeometry
    common = dict(align=8, steps_per_frame=20, pulse_per_frame=100, hop_size=300, carry=True, layer_carry=True,
                  layer_min_rows=recorder.LAYER_MIN_ROWS, fe_ring=64)
    if name == "chunk8":
        return StreamGeometry(left=10, right=11, lead=4, act_left=6, act_right=7, wn_left=2, wn_reach=2, sr_left=4, sr_right=5,
                              **common)
    return StreamGeometry(left=15, right=7, lead=7, act_left=8, act_right=6, wn_left=4, wn_reach=1, sr_left=6, sr_right=5,
                          **common)


def _fresh(slot, have, closed):
    return SimpleNamespace(slot=slot, emitted=0, have=have, closed=closed, carry_pos=None, carry_frames=0, layer_end=None,
                           state=(0.0, 0.0, 0), state_frame=0, f0_mode="net")


def _continuing(geo, slot, emitted, have, closed, state):
    """A stream whose last tick ended at `emitted` in the middle of its utterance: that tick stored the sub-band rows
    around `emitted`, the layer state of a region that reached act_right frames further, and captured the phase state
    left - lead frames in front (the double's: call number + item / 16, half the calls so far, the calls so far)."""
    return SimpleNamespace(slot=slot, emitted=emitted, have=have, closed=closed, carry_pos=emitted,
                           carry_frames=geo.sr_left + geo.sr_right, layer_end=emitted + geo.act_right, state=state,
                           state_frame=max(0, emitted - (geo.left - geo.lead)), f0_mode="net")


def _plan_cases():
    c8, fc = _geometry("chunk8"), _geometry("force_causal")
    return {
        # "a" alone, its 190 frames pushed and closed before the first tick
        ("chunk8", 0): [_fresh(0, 190, True)],
        # "d" joins "a", "b" (16 frames per tick) and the slowly fed "c": no common geometry
        ("chunk8", 4): [_continuing(c8, 0, 32, 190, True, (4.0, 2.0, 4)), _continuing(c8, 1, 24, 80, False, (4.0625, 1.5, 3)),
                        _continuing(c8, 2, 8, 31, False, (4.125, 0.5, 1)), _fresh(3, 24, False)],
        # all four in step, each at its own multiple of 8 frames: a steady tick
        ("chunk8", 10): [_continuing(c8, 0, 80, 190, True, (10.0, 5.0, 10)), _continuing(c8, 1, 72, 120, True, (10.0625, 4.5, 9)),
                         _continuing(c8, 2, 40, 60, False, (10.125, 2.5, 5)), _continuing(c8, 3, 48, 96, True, (10.1875, 3.0, 6))],
        ("force_causal", 0): [_fresh(0, 190, True), _fresh(1, 16, False)],
        # "d" after its first tick: its state still sits at frame 0
        ("force_causal", 5): [_continuing(fc, 0, 40, 190, True, (5.0, 2.5, 5)), _continuing(fc, 1, 40, 96, False, (5.0625, 2.5, 5)),
                              _continuing(fc, 2, 16, 39, False, (5.125, 1.0, 2)), _continuing(fc, 3, 8, 48, False, (5.1875, 0.5, 1))],
        # "c" sat out the tick before: its phase state is that of call 10
        ("force_causal", 11): [_continuing(fc, 0, 88, 190, True, (11.0, 5.5, 11)), _continuing(fc, 1, 88, 120, True, (11.0625, 5.5, 11)),
                               _continuing(fc, 2, 48, 67, False, (10.125, 3.0, 6)), _continuing(fc, 3, 56, 96, True, (11.125, 3.5, 7))],
    }


@pytest.mark.parametrize("name,tick", sorted(_plan_cases()))
def test_plan_tick_alone_gives_the_recorded_arguments(name, tick, golden):
    from mbexwn_vocoder_amd.stream_plan import plan_tick
    streams = _plan_cases()[(name, tick)]
    before = [dict(vars(st)) for st in streams]
    plan = plan_tick(_geometry(name), [(st, 8) for st in streams])
    assert [vars(st) for st in streams] == before             # a plan changes no stream
    record = golden[name]["ticks"][tick]
    call = record["call"]
    assert len(streams) == call["B"] and plan.tmax == call["T"]
    assert plan.nfr.tolist() == call["n_frames"] and plan.states.ravel().tolist() == call["stream_state"]
    assert [plan.a0, plan.act.tolist(), int(plan.act.max())] == call["active"]
    assert (None if plan.wn is None else [plan.wa, plan.wn.tolist(), int(plan.wn.max())]) == call["wavenet"]
    assert plan.desc.ravel().tolist() == call["carry"]["desc"] and plan.ldesc.ravel().tolist() == call["layers"]["desc"]
    assert plan.layer_rows == call["layers"]["rows"] == record["layer_rows"]
    assert plan.fpos.tolist() == call["frontend"]["pos"]
    assert plan.emit == [8] * len(streams) and [nn * 300 for nn in plan.emit] == record["lens"]
    for dtype_of in (plan.act, plan.nfr, plan.states, plan.desc, plan.ldesc, plan.fpos):
        assert dtype_of.dtype == np.int32


def test_plan_tick_successors_chain_into_the_next_tick(golden):
    """What a plan says the streams carry on is what the next tick's plan starts from: ticks 10 and 11 of the 8-frame
    scenario are both steady, and applying the successors of tick 10 by hand gives the recorded arguments of tick 11."""
    from mbexwn_vocoder_amd.stream_plan import plan_tick
    geo = _geometry("chunk8")
    streams = _plan_cases()[("chunk8", 10)]
    plan = plan_tick(geo, [(st, 8) for st in streams])
    assert plan.next_carry == [(st.emitted + 8, 9) for st in streams]
    assert plan.next_layer_end == [st.emitted + 8 + geo.act_right for st in streams]
    assert plan.next_state_frame == [st.emitted + 8 - (geo.left - geo.lead) for st in streams]
    call = golden["chunk8"]["ticks"][11]["call"]
    assert call["B"] == 4
    have = {0: 190, 1: 120, 2: 67, 3: 96}                    # "c" received PUSH_TABLE[(11 + 3 * 2) % 14] = 7 frames more
    for item, st in enumerate(streams):
        st.emitted += 8
        st.carry_pos, st.carry_frames = plan.next_carry[item]
        st.layer_end, st.state_frame = plan.next_layer_end[item], plan.next_state_frame[item]
        st.state = (11.0 + item / 16, st.state[1] + 0.5, st.state[2] + 1)
        st.have = have[item]
    nxt = plan_tick(geo, [(st, 8) for st in streams])
    assert nxt.states.ravel().tolist() == call["stream_state"] and nxt.ldesc.ravel().tolist() == call["layers"]["desc"]
    assert nxt.desc.ravel().tolist() == call["carry"]["desc"] and nxt.layer_rows == call["layers"]["rows"] == 160
    assert [nxt.wa, nxt.wn.tolist(), int(nxt.wn.max())] == call["wavenet"]


@pytest.mark.parametrize("name", ["chunk8", "force_causal"])
def test_hand_written_geometry_is_the_synthesizers(name):
    from mbexwn_vocoder_amd.config import canonical_config
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    cfg = canonical_config("SPEECH", **recorder.SCENARIOS[name].get("config", {}))
    assert StreamingSynthesizer(recorder.RecordingEngine(cfg), chunk_frames=8).geometry == _geometry(name)

"""What the analyzer's tick uploads and launches, planned on the host (mbexwn_vocoder_amd/live_plan.py::AnalysisPlan,
StreamingAnalyzer.plan / commit): the rows, the four descriptor tables of include/mbexwn_live.h and
include/mbexwn_live_resample.h, their place in the staging buffer, the launch groups and the ring lengths.  The expected
values are worked out by hand from the headers' layouts and the readiness rules.  No GPU."""
import subprocess
import sys

import numpy as np

from mbexwn_vocoder_amd import live
from test_live_host import TINY                # hop 4, win 16, 24 kHz

F48, F16 = (1, 2, 44, 89), (3, 2, 67, 135)     # (up, down, half, n_taps) of 48 kHz -> 24 kHz and of 16 kHz -> 24 kHz


def samples(tag, first, count):
    """Distinguishable values: sample i of stream `tag` is 1000 tag + i."""
    return (1000.0 * tag + np.arange(first, first + count)).astype(np.float32)


def worked_case():
    """a at the model rate with 11 samples; b at 48 kHz with 300 + 50; c at 16 kHz with 40, closed; d at 48 kHz with 3."""
    an = live.StreamingAnalyzer(TINY, slots=2)
    an.open("a")
    an.open("b", sample_rate=48000)
    an.open("c", sample_rate=16000)
    an.open("d", sample_rate=48000)
    an.push("a", samples(1, 0, 11))
    an.push("b", samples(2, 0, 300))
    an.push("b", samples(2, 300, 50))
    an.push("c", samples(3, 0, 40), last=True)
    an.push("d", samples(4, 0, 3))
    return an


def state(an):
    return {sid: {kk: (list(map(id, vv)) if kk == "queue" else vv) for kk, vv in vars(st).items()}
            for sid, st in an.streams.items()}


def test_first_plan_of_the_worked_case():
    an = worked_case()
    sts = an.streams
    assert [(st.slot, st.in_slot, st.filt) for st in sts.values()] == [(0, None, None), (1, 0, F48), (2, 1, F16), (3, 2, F48)]
    # b: outputs k with 2 k + 44 <= 350 - 1, so 153; c is closed: ceil(40 * 3 / 2) = 60; d: 3 - 1 - 44 < 0, none.
    # Frame t needs 4 t + 8 samples: 1 of 11, 37 of 153; the closed stream has 60 // 4 + 1 = 16
    assert [st.have for st in sts.values()] == [11, 153, 60, 0]
    assert [an._ready(st) for st in sts.values()] == [1, 37, 16, 0]
    plan = an.plan()
    assert plan.rows == [("a", 1), ("b", 37), ("c", 16), ("d", 0)] and (plan.S, plan.R) == (4, 3)
    assert plan.resampled == [2, 1, 3]                                   # c (16 kHz) in front of b and d (48 kHz), stable
    assert plan.counts == [11, 350, 40, 3] and plan.offsets == [0, 11, 361, 401]
    assert (plan.body, plan.samples) == (16 * 4 + 20 * 3, 404)
    for table in (plan.append, plan.frames, plan.in_append, plan.in_resample):
        assert table.dtype == np.int64
    # slot, abs_start, count, offset: a resampled stream appends nothing to its model-rate ring
    assert plan.append.tolist() == [[0, 0, 11, 0], [1, 0, 0, 11], [2, 0, 0, 361], [3, 0, 0, 401]]
    # slot, first_frame, n_frames, n_total: only c knows its length
    assert plan.frames.tolist() == [[0, 0, 1, -1], [1, 0, 37, -1], [2, 0, 16, 60], [3, 0, 0, -1]]
    # in_slot, abs_start, count, offset, in the order c, b, d
    assert plan.in_append.tolist() == [[1, 0, 40, 361], [0, 0, 350, 11], [2, 0, 3, 401]]
    # in_slot, out_slot, first_out, n_out_new, n_total_in, 0
    assert plan.in_resample.tolist() == [[1, 2, 0, 60, 40, 0], [0, 1, 0, 153, -1, 0], [2, 3, 0, 0, -1, 0]]
    assert plan.groups == [(16000, 0, 1, 60), (48000, 1, 3, 153)]
    assert (plan.max_model, plan.max_in, plan.max_new) == (11, 350, 37)
    # no frame has been handed out, so every ring holds its stream from sample 0: 153 samples at most, 350 at the input rate
    assert plan.ring_needed == 153 and an.ring_samples == 64 and live._pow2_at_least(153) == 256      # 64 -> 128 -> 256
    assert plan.in_ring_needed == 350 <= an.input_ring_samples == 4096
    assert plan.fresh == [0, 1, 2, 3]


def test_packed_bytes_of_the_worked_case():
    an = worked_case()
    plan = an.plan()
    stage = np.zeros(1024, dtype=np.float32)
    plan.pack(stage)
    S, R = 4, 3
    ints = stage.view(np.int64)                                          # word w of float32 is half of int64 w // 2
    assert ints[:4 * S].reshape(S, 4).tolist() == [[0, 0, 11, 0], [1, 0, 0, 11], [2, 0, 0, 361], [3, 0, 0, 401]]
    assert ints[4 * S:8 * S].reshape(S, 4).tolist() == [[0, 0, 1, -1], [1, 0, 37, -1], [2, 0, 16, 60], [3, 0, 0, -1]]
    at = 16 * S // 2
    assert ints[at:at + 4 * R].reshape(R, 4).tolist() == [[1, 0, 40, 361], [0, 0, 350, 11], [2, 0, 3, 401]]
    at = (16 * S + 8 * R) // 2
    assert ints[at:at + 6 * R].reshape(R, 6).tolist() == [[1, 2, 0, 60, 40, 0], [0, 1, 0, 153, -1, 0], [2, 3, 0, 0, -1, 0]]
    body = 16 * S + 20 * R
    want = np.concatenate([samples(1, 0, 11), samples(2, 0, 350), samples(3, 0, 40), samples(4, 0, 3)])
    assert np.array_equal(stage[body:body + 404], want) and not stage[body + 404:].any()


def test_commit_then_the_second_tick():
    an = worked_case()
    an.commit(an.plan())
    assert [(st.on_device, st.in_on_device, st.emitted, st.queue, st.fresh) for st in an.streams.values()] == [
        (11, 11, 1, [], False), (153, 350, 37, [], False), (60, 40, 16, [], False), (0, 3, 0, [], False)]
    assert an.finished("c") and not an.plan().rows                       # nothing queued, nothing new ready: no work
    an.push("a", samples(1, 11, 5))
    plan = an.plan()                                                     # 16 samples: frames 0 .. 2, frame 0 is out
    assert plan.rows == [("a", 2)] and (plan.S, plan.R, plan.groups, plan.fresh) == (1, 0, [], [])
    assert plan.append.tolist() == [[0, 11, 5, 0]] and plan.frames.tolist() == [[0, 1, 2, -1]]
    assert plan.in_append.shape == (0, 4) and plan.in_resample.shape == (0, 6) and plan.max_in == 0
    assert plan.ring_needed == 16                                        # frame 1 may read from 1 * 4 - 8 - 2 < 0 on
    stage = np.zeros(32, dtype=np.float32)
    plan.pack(stage)
    assert np.array_equal(stage[16:21], samples(1, 11, 5)) and not stage[21:].any()
    an.commit(plan)
    # d's samples are appended as they come, but its first output is final with 45 of them: 2 * 0 + 44 <= 45 - 1
    an.push("d", samples(4, 3, 41))
    plan = an.plan()
    assert plan.rows == [("d", 0)] and plan.in_append.tolist() == [[2, 3, 41, 0]]
    assert plan.in_resample.tolist() == [[2, 3, 0, 0, -1, 0]] and plan.groups == [(48000, 0, 1, 0)]
    an.commit(plan)
    assert not an.plan().rows
    an.push("d", samples(4, 44, 1))
    plan = an.plan()
    assert plan.in_append.tolist() == [[2, 44, 1, 0]] and plan.in_resample.tolist() == [[2, 3, 0, 1, -1, 0]]
    assert plan.append.tolist() == [[3, 0, 0, 0]] and plan.frames.tolist() == [[3, 0, 0, -1]]
    # the input ring holds d from the first sample output 0 reads, max(0, ceil((0 + 44 - 88) / 1)) = 0, to the newest
    assert plan.in_ring_needed == 45 and plan.ring_needed == 1


def test_a_released_slot_is_fresh_again():
    an = worked_case()
    an.commit(an.plan())
    an.close("c")
    an.open("e")
    assert (an.streams["e"].slot, an.streams["e"].fresh) == (2, True)
    an.push("e", samples(5, 0, 2))
    plan = an.plan()
    assert plan.rows == [("e", 0)] and plan.fresh == [2] and plan.append.tolist() == [[2, 0, 2, 0]]
    an.commit(plan)
    an.push("e", samples(5, 2, 2))
    assert an.plan().fresh == []


def test_no_work_is_no_device():
    an = live.StreamingAnalyzer(TINY)
    assert an.plan().rows == [] and an.tick() == {}
    an.open(0)
    plan = an.plan()
    assert plan.rows == [] and (plan.S, plan.R, plan.samples, plan.max_new, plan.ring_needed) == (0, 0, 0, 0, 0)
    assert an.tick() == {} and an.device is None and an.rings is None and an.input_rings is None
    assert an.device_allocations == 0 and an.ticks == 0


def test_planning_is_pure():
    an = worked_case()
    before = state(an)
    first, second = an.plan(), an.plan()
    assert state(an) == before and before["a"]["fresh"] is True
    for name, value in vars(first).items():
        other = getattr(second, name)
        assert np.array_equal(value, other) if isinstance(value, np.ndarray) else value == other, name
    stages = np.zeros((2, 600), dtype=np.float32)
    first.pack(stages[0])
    second.pack(stages[1])
    assert stages[0].tobytes() == stages[1].tobytes() and state(an) == before      # bytes: a -1 reads as a NaN
    # the module of the plans needs no torch
    code = "import sys; import mbexwn_vocoder_amd.live_plan; sys.exit(int('torch' in sys.modules))"
    assert subprocess.run([sys.executable, "-c", code], cwd=live.__file__.rsplit("/", 2)[0]).returncode == 0


def test_planned_frames_cover_every_frame_once():
    """Pushes of 1, 3, 7 and 40 samples, then the close: the planned (first_frame, n_frames) are contiguous and end at
    n // hop + 1 = 13, and no frame is planned before its window is there (4 t + 8 samples) while the stream is open."""
    an = live.StreamingAnalyzer(TINY)
    an.open("a")
    have, nxt = 0, 0
    for count in (1, 3, 7, 40, 0):
        an.push("a", samples(1, have, count), last=count == 0)
        have += count
        plan = an.plan()
        (slot, first, nn, n_total), = plan.frames.tolist()
        assert (slot, first, n_total) == (0, nxt, 51 if count == 0 else -1)
        assert count == 0 or nn == 0 or 4 * (first + nn - 1) + 8 <= have < 4 * (first + nn) + 8
        nxt += nn
        an.commit(plan)
    assert nxt == 51 // 4 + 1 == 13 and an.finished("a") and not an.plan().rows

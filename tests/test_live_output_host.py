"""Audio out at any rate, on the host (mbexwn_vocoder_amd/live.py, include/mbexwn_live_out.h): the header of the streaming
output resampler and its export, what the output stage plans tick by tick against the readiness rules, the look-ahead it
adds, and the refusals of the stage, the pipeline and the two tools.  No GPU."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from mbexwn_vocoder_amd import live

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")
MODEL_RATE = 24000
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 5}
OUT_RATES = (48000, 44100, 16000, 8000)
TINY = {"sample_rate": MODEL_RATE, "hop_size": 4, "win_size": 16, "fft_size": 16, "mel_channels": 4, "fmin": 0.0, "fmax": None,
        "lin_amp_off": 1e-5, "lin_amp_scale": 1, "mel_amp_scale": 1}


def geometry(rate):
    """(up, down, half, n_taps) of the reference's filter for the model rate -> rate."""
    from mbexwn_vocoder_amd.resample import reference_filter
    taps, up, down = reference_filter(MODEL_RATE, rate)
    return up, down, (taps.size - 1) // 2, int(taps.size)


def test_header_declares_the_output_resampler_and_the_library_exports_it(tmp_path):
    """(that the header declares exactly these names, no other header does and the library exports them: test_abi_headers.py)"""
    from mbexwn_vocoder_amd import abi
    from mbexwn_vocoder_amd.build import HEADERS, SOURCES
    text = open(os.path.join(ROOT, "include", "mbexwn_live_out.h")).read()
    assert "THE PROMISE" in text and "bits" in text and "out_offset" in text and "Refused" in text and "resample emit:" in text
    assert abi.symbols("mbexwn_live_out.h") == ["mbxo_resample_emit"]
    assert any(hh.endswith("mbexwn_live_out.h") for hh in HEADERS) and "resample_stream.hip" in SOURCES
    assert abi.MBX_ABI_VERSION == 11
    assert len(abi.TABLE["mbexwn_live_out.h"][0][2]) == 13
    # the header compiles as C
    src = tmp_path / "use.c"
    src.write_text('#include "mbexwn_live_out.h"\nint main(void){ (void)mbxo_resample_emit; return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_filter_sizes_of_a_24_khz_model():
    assert geometry(48000) == (2, 1, 44, 90)
    assert geometry(44100) == (147, 80, 3307, 6615)
    assert geometry(16000) == (2, 3, 66, 134)
    assert geometry(12345)[:2] == (823, 1600) and geometry(12345)[3] == 69955
    for rate in OUT_RATES + (12345,):
        assert live.output_filter(MODEL_RATE, rate) == geometry(rate)


def planned_ticks(stage, sid, cuts, source):
    """Push `cuts` one per tick, planning and committing on the host alone: the (first_out, n_out_new, n_total_in, have,
    ring_needed) of every tick that had work, and the index of the closing tick."""
    ticks, pos = [], 0
    for ii, cc in enumerate(cuts):
        stage.push(sid, source, pos, cc, last=ii == len(cuts) - 1)
        pos += cc
        plan = stage.plan()
        for row_sid, first, n_new, n_total in plan.rows:
            assert row_sid == sid
            ticks.append((first, n_new, n_total, stage.streams[sid].have, plan.ring_needed))
        stage.commit(plan)
    assert stage.plan().rows == []                               # nothing is left behind the close
    return ticks


@pytest.mark.parametrize("rate", OUT_RATES)
def test_planned_ticks_cover_every_output_once_and_none_early(rate):
    """Random push sizes: the (first_out, n_out_new) the stage plans are contiguous, cover [0, ceil(n * up / down)) exactly
    once, no output is planned before the newest sample it reads is there ((k * down + half) // up < have), and the ring
    the plan asks for holds everything from input_keep_from(first_out) to the newest sample."""
    import torch
    up, down, half, n_taps = geometry(rate)
    rng = np.random.default_rng(rate)
    for trial in range(4):
        n = int(rng.integers(half // up + 2, 3000))
        cuts = []
        while sum(cuts) < n:
            cuts.append(min(n - sum(cuts), int(rng.integers(1, 5)) if rng.integers(0, 2) else int(rng.integers(5, 700))))
        source = torch.zeros(n, dtype=torch.float32)
        stage = live.StreamingOutputResampler(MODEL_RATE)
        stage.open("s", rate)
        ticks = planned_ticks(stage, "s", cuts, source)
        nxt = 0
        for ii, (first, n_new, n_total, have, ring_needed) in enumerate(ticks):
            assert first == nxt and n_new >= 0
            closing = n_total >= 0
            assert closing == (have == n and ii == len(ticks) - 1) and (not closing or n_total == n)
            if n_new and not closing:
                assert ((first + n_new - 1) * down + half) // up < have          # the newest output reads nothing unseen
                assert ((first + n_new) * down + half) // up >= have             # ... and the next one would
            assert ring_needed >= have - live.input_keep_from(first, up, down, half, n_taps)
            assert ring_needed <= have
            nxt += n_new
        assert nxt == -(-n * up // down)
        assert stage.finished("s") and stage.rings is None                        # planning touches no device
        assert stage.device_allocations == 0


@pytest.mark.parametrize("rate", OUT_RATES)
def test_a_stream_shorter_than_half_the_filter_plans_nothing_before_its_close(rate):
    import torch
    up, down, half, _ = geometry(rate)
    short = half // up
    assert short >= 1
    stage = live.StreamingOutputResampler(MODEL_RATE)
    stage.open("s", rate)
    ticks = planned_ticks(stage, "s", [1] * short + [0], torch.zeros(short, dtype=torch.float32))
    assert [tt[1] for tt in ticks[:-1]] == [0] * short and not any(tt[2] >= 0 for tt in ticks[:-1])
    assert ticks[-1][:3] == (0, -(-short * up // down), short)
    assert stage.finished("s")


def test_seven_pushes_of_300_samples():
    """Seven 300-sample pushes to 48 kHz: 4156 outputs before the close, 4200 in all, and the ring never has to hold more
    than 344 samples -- 428 to 8 kHz, the longest filter span among the tested rates.  The chunks of the synthesizer's 80 ms
    schedule (6, 6, 7, 6, 7 frames of 300 samples, a chunk per push) fit the ring the stage starts with."""
    import torch
    source = torch.zeros(9600, dtype=torch.float32)
    for rate, span in ((48000, 344), (8000, 428)):
        stage = live.StreamingOutputResampler(MODEL_RATE)
        stage.open(0, rate)
        ticks = planned_ticks(stage, 0, [300] * 7 + [0], source)
        up, down, _, _ = geometry(rate)
        assert sum(tt[1] for tt in ticks) == -(-2100 * up // down)
        assert max(tt[4] for tt in ticks) == span
        if rate == 48000:
            assert sum(tt[1] for tt in ticks[:-1]) == 4156 and sum(tt[1] for tt in ticks) == 4200
        stage.open(1, rate)
        ticks = planned_ticks(stage, 1, [1800, 1800, 2100, 1800, 2100, 0], source)
        assert 2100 < max(tt[4] for tt in ticks) <= 2100 + span <= stage.ring_samples == 4096


def test_lookahead_ms_for():
    assert abs(live.output_lookahead_ms(MODEL_RATE, 48000) - 0.917) < 5e-4
    assert abs(live.output_lookahead_ms(MODEL_RATE, 44100) - 0.937) < 5e-4
    assert abs(live.output_lookahead_ms(MODEL_RATE, 16000) - 1.375) < 5e-4
    for rate in (48000, 44100, 16000):
        up, _, half, _ = geometry(rate)
        assert live.output_lookahead_ms(MODEL_RATE, rate) == 1000.0 * half / (up * MODEL_RATE)
    # the method of the pipeline, on a resynthesizer that has only what the look-ahead reads
    lr = object.__new__(live.LiveResynthesizer)
    lr.analyzer = live.StreamingAnalyzer(TINY)
    lr.synthesizer = types.SimpleNamespace(lookahead_ms=12.5)
    base = lr.lookahead_ms
    assert lr.lookahead_ms_for() == lr.lookahead_ms_for(None) == lr.lookahead_ms_for(24000) == base
    assert lr.lookahead_ms_for(None, 24000) == lr.lookahead_ms_for(None, "input") == base       # no stage, nothing added
    in44 = lr.lookahead_ms_for(44100)
    assert 0.9 < in44 - base < 0.95                                                              # as before this argument
    assert lr.lookahead_ms_for(None, 48000) == base + live.output_lookahead_ms(MODEL_RATE, 48000)
    assert lr.lookahead_ms_for(44100, "input") == in44 + live.output_lookahead_ms(MODEL_RATE, 44100)
    assert lr.lookahead_ms_for(44100, output_rate=16000) == in44 + live.output_lookahead_ms(MODEL_RATE, 16000)
    assert lr.lookahead_ms == base


def test_refusals():
    import torch
    stage = live.StreamingOutputResampler(MODEL_RATE)
    for bad in (0, -48000, 0.2, float("nan"), float("inf"), "48000", None):
        with pytest.raises(ValueError, match="output_rate"):
            stage.open("bad", bad)
        if bad != "48000":
            with pytest.raises(ValueError, match="output_rate"):
                live.resolve_output_rate(bad if bad is not None else float("nan"), None, MODEL_RATE)
    assert "bad" not in stage.streams
    with pytest.raises(ValueError, match="'input'"):
        live.resolve_output_rate("output", 44100, MODEL_RATE)
    # "input" on a stream without a rate of its own is the model rate, and the model rate needs no stage
    assert live.resolve_output_rate("input", None, MODEL_RATE) is None
    assert live.resolve_output_rate("input", 24000, MODEL_RATE) is None
    assert live.resolve_output_rate(24000, 44100, MODEL_RATE) is None
    assert live.resolve_output_rate(None, 44100, MODEL_RATE) is None
    assert live.resolve_output_rate("input", 44100, MODEL_RATE) == 44100
    assert live.resolve_output_rate(48000.0, None, MODEL_RATE) == 48000
    source = torch.zeros(64, dtype=torch.float32)
    stage.open("s", 48000)
    with pytest.raises(ValueError, match="open already"):
        stage.open("s", 16000)
    stage.push("s", source, 0, 10)
    for args in ((source, 60, 10), (source, -1, 4), (source, 0, -4), (source.double(), 0, 4), (source[::2], 0, 4), (None, 0, 4)):
        with pytest.raises(ValueError):
            stage.push("s", *args)
    assert stage.streams["s"].have == 10
    stage.push("s", source, 10, 5, last=True)
    with pytest.raises(ValueError, match="closed"):
        stage.push("s", source, 15, 5)
    assert stage.streams["s"].have == 15 and not stage.finished("s")
    # a released slot is the next one taken
    slot = stage.streams["s"].slot
    stage.open("t", 16000)
    stage.close("s")
    stage.open("u", 44100)
    assert stage.streams["u"].slot == slot != stage.streams["t"].slot


def run_tool(name, *argv):
    return subprocess.run([sys.executable, os.path.join(BIN, name), *argv], capture_output=True, text=True, timeout=300)


def test_tool_flags_parse_and_refuse(tmp_path):
    from scipy.io import wavfile
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    res = run_tool("resynth_mel.py", "SPEECH", "-i", "nothing.mell", "--out-rate", "0")
    assert res.returncode == 2 and "--out-rate" in res.stderr and "positive" in res.stderr
    res = run_tool("resynth_mel.py", "SPEECH", "-i", "nothing.mell", "--out-rate", "fast")
    assert res.returncode == 2 and "--out-rate" in res.stderr
    res = run_tool("resynth_mel.py", "--help")
    assert res.returncode == 0 and "--out-rate" in res.stdout and "mel_error" in res.stdout
    res = run_tool("stream_transpose.py", "in.wav", "-o", "out.wav", "--output-rate", "0")
    assert res.returncode == 2 and "--output-rate" in res.stderr
    res = run_tool("stream_transpose.py", "in.wav", "-o", "out.wav", "--output-rate", "source")
    assert res.returncode == 2 and "--output-rate" in res.stderr
    # "input" needs --resample when the file is not at the model rate: refused before anything touches a device
    model = create_synthetic_model_dir(str(tmp_path / "speech"), "SPEECH", **SMALL)
    src, dst = str(tmp_path / "in44.wav"), str(tmp_path / "out.wav")
    wavfile.write(src, 44100, np.zeros(4410, dtype=np.float32))
    res = run_tool("stream_transpose.py", src, "-o", dst, "--model_id", model, "--output-rate", "input")
    assert res.returncode == 1 and "--output-rate input" in res.stderr and "--resample" in res.stderr
    assert not os.path.exists(dst)


def test_a_worked_tick_packs_the_descriptor_words_of_the_headers():
    """Four streams, one tick, every word by hand from the row layouts of mbexwn_live.h (append: slot, abs_start, count,
    offset) and mbexwn_live_out.h (emit: in_slot, first_out, n_out_new, n_total_in or -1, out_offset, 0).  To 48 kHz (up 2,
    down 1, half 44) output k is final once 2 have - 45 >= k; to 16 kHz (up 2, down 3, half 66) once 2 have - 67 >= 3 k."""
    import torch
    one, two = torch.zeros(400, dtype=torch.float32), torch.zeros(128, dtype=torch.float32)
    stage = live.StreamingOutputResampler(MODEL_RATE)
    for sid, rate in (("a", 48000), ("b", 16000), ("c", 48000), ("d", 48000)):      # slots 0 .. 3
        stage.open(sid, rate)
    stage.push("a", one, 0, 40)                          # an earlier tick: 2 * 40 - 45 = 35, outputs 0 .. 35
    first = stage.plan()
    assert first.rows == [("a", 0, 36, -1)] and first.starts == [0, 36]
    stage.commit(first)
    stage.push("a", one, 40, 100)                        # two pushes from one tensor: two turns
    stage.push("a", one, 140, 50)                        # ... 190 samples: 2 * 190 - 45 = 335, outputs 36 .. 335
    stage.push("b", two, 10, 90)                         # a second tensor, another rate: 2 * 90 - 67 = 113 = 3 * 37 + 2, 38 outputs
    stage.push("c", one, 200, 30, last=True)             # closed at 30 samples: all ceil(30 * 2 / 1) = 60 outputs
    stage.push("d", one, 300, 20)                        # 2 * 20 - 45 < 0: appended, nothing final
    plan = stage.plan()
    assert plan.rows == [("b", 0, 38, -1), ("a", 36, 300, -1), ("c", 0, 60, 30), ("d", 0, 0, -1)]       # by rate, stable
    assert plan.groups == [(16000, 0, 1, 38), (48000, 1, 4, 300)]
    assert plan.starts == [0, 38, 338, 398, 398] and plan.ring_needed == 190     # output 36 still reads from sample 0 on
    # one call per (turn, tensor), no slot twice in a call: the second tensor, the first turn of the first, its second turn
    assert plan.calls == {(0, two.data_ptr(), 128): [(1, 0, 90, 10)],
                          (0, one.data_ptr(), 400): [(0, 40, 100, 40), (2, 0, 30, 200), (3, 0, 20, 300)],
                          (1, one.data_ptr(), 400): [(0, 140, 50, 140)]}
    assert list(plan.calls) == [(0, two.data_ptr(), 128), (0, one.data_ptr(), 400), (1, one.data_ptr(), 400)]
    assert (plan.n_app, plan.words) == (5, 4 * 5 + 6 * 4)
    desc = np.full(48, -7, dtype=np.int64)
    plan.pack(desc, stage._word5)
    assert desc.tolist() == [1, 0, 90, 10,
                             0, 40, 100, 40, 2, 0, 30, 200, 3, 0, 20, 300,
                             0, 140, 50, 140,
                             1, 0, 38, -1, 0, 0,
                             0, 36, 300, -1, 38, 0,
                             2, 0, 60, 30, 338, 0,
                             3, 0, 0, -1, 398, 0,
                             -7, -7, -7, -7]
    stage.commit(plan)
    assert [(st.emitted, st.on_device, st.queue) for st in stage.streams.values()] == [(336, 190, []), (38, 90, []), (60, 30, []),
                                                                                      (0, 20, [])]
    assert stage.finished("c") and not stage.finished("a") and stage.plan().rows == []
    assert stage.rings is None and stage.device_allocations == 0                 # planning and packing touch no device

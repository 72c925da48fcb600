"""Live streams on the host (mbexwn_vocoder_amd/live.py): the header of the streaming entry points, the readiness rule and
the transposition mapping as pure host logic, and the refusals.  No GPU."""
import os

import numpy as np
import pytest

from mbexwn_vocoder_amd import live

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = {"sample_rate": 24000, "hop_size": 4, "win_size": 16, "fft_size": 16, "mel_channels": 4, "fmin": 0.0, "fmax": None,
        "lin_amp_off": 1e-5, "lin_amp_scale": 1, "mel_amp_scale": 1}


def test_live_header_declares_the_live_symbols_and_the_library_exports_them():
    """(that the header declares exactly these names, no other header does and the library exports them: test_abi_headers.py)"""
    from mbexwn_vocoder_amd import abi
    from mbexwn_vocoder_amd.build import HEADERS
    text = open(os.path.join(ROOT, "include", "mbexwn_live.h")).read()
    assert "bits" in text and "desc" in text                       # the promise and the descriptor layouts are documented
    assert abi.symbols("mbexwn_live.h") == ["mbxl_ring_append", "mbxl_mel_frames"]
    assert any(hh.endswith("mbexwn_live.h") for hh in HEADERS)       # a change of the header rebuilds the library
    assert abi.MBX_ABI_VERSION == 11


def test_readiness_rule_in_closed_form():
    """hop 4, win 16: frame t needs 4 t + 8 samples.  Pushes of 1, 3, 7 and 40 samples: 1, 4, 11 and 51 samples have
    arrived, so 0, 0, 1 and 11 frames are ready; the closed stream has 51 // 4 + 1 = 13."""
    hop, win = 4, 16
    have, ready = 0, []
    for count in (1, 3, 7, 40):
        have += count
        ready.append(live.frames_ready(have, hop, win))
    assert ready == [0, 0, 1, 11]
    assert ready == [0 if hh < 8 else (hh - 8) // 4 + 1 for hh in (1, 4, 11, 51)]
    assert live.frames_ready(have, hop, win, closed=True) == have // hop + 1 == 13 == live.frames_total(have, hop)
    # the edge of the rule, and an odd window (the window of frame t ends at t hop - win // 2 + win)
    assert [live.frames_ready(hh, hop, win) for hh in (7, 8, 11, 12)] == [0, 1, 1, 2]
    assert [live.frames_ready(hh, 3, 7) for hh in (3, 4, 6, 7)] == [0, 1, 1, 2]
    # an open stream never has more frames than the closed one will
    assert all(live.frames_ready(hh, hop, win) <= live.frames_total(hh, hop) for hh in range(100))
    # the analyzer's streams follow the rule without a device
    an = live.StreamingAnalyzer(TINY)
    an.open("a")
    seen = []
    for count in (1, 3, 7, 40):
        an.push("a", np.zeros(count, dtype=np.float32))
        seen.append(an._ready(an.streams["a"]))
    an.push("a", np.zeros(0, dtype=np.float32), last=True)
    assert seen == [0, 0, 1, 11] and an._ready(an.streams["a"]) == 13 and not an.finished("a")


@pytest.mark.parametrize("pushes", [
    [(1, None), (3, 1.5), (7, 0.5), (40, 2.0)],          # 51 samples: the last frame (t = 12, centre 48) lies in a push
    [(4, 1.25), (0, 3.0), (8, None), (4, 0.75)],         # 16 = 4 hop: frame 4 is centred behind the end; an empty push
    [(3, 2.0)],                                          # shorter than a hop: one frame
    [(1, 1.5), (1, None), (1, 0.5), (1, 2.0), (1, 3.0)],  # one-sample pushes: frame 1 is centred in the fifth
])
def test_transposition_mapping_follows_the_frame_centres(pushes):
    hop = 4
    got = live.frame_factors(pushes, hop)
    n = sum(count for count, _ in pushes)
    want = np.ones(n // hop + 1, dtype=np.float32)
    last = 1.0
    for tt in range(n // hop + 1):
        start = 0
        for count, factor in pushes:
            if start <= tt * hop < start + count:
                want[tt] = 1.0 if factor is None else factor
            if count:
                last = 1.0 if factor is None else factor
            start += count
        if tt * hop == n:
            want[tt] = last                              # centred on the sample behind the end: the last non-empty push
    assert got.dtype == np.float32 and np.array_equal(got, want)
    # incrementally, a frame's factor is decided by the time the analysis can hand the frame out (win 16: 4 t + 8 samples)
    ff, have = live.FrameFactors(hop), 0
    for count, factor in pushes:
        ff.add(count, factor)
        have += count
        assert ff.frames >= live.frames_ready(have, hop, 16)
    ff.close()
    assert ff.frames == n // hop + 1 and np.array_equal(ff.take(0, ff.frames), want)


def test_refusals():
    an = live.StreamingAnalyzer(TINY)
    an.open(0)
    with pytest.raises(ValueError, match="generate_mel.py.*resample.resample_host"):
        an.push(0, np.zeros(10, dtype=np.float32), sample_rate=44100)
    an.push(0, np.zeros(10, dtype=np.float32), sample_rate=24000)
    with pytest.raises(ValueError, match="mono"):
        an.push(0, np.zeros((10, 2), dtype=np.float32))
    with pytest.raises(ValueError, match="open already"):
        an.open(0)
    # an empty closed stream, as generate_mels refuses an empty sound
    an.open(1)
    an.push(1, np.zeros(0, dtype=np.float32))
    with pytest.raises(ValueError, match="no samples"):
        an.push(1, [], last=True)
    an.push(0, [], last=True)                                      # closing a stream that has samples with an empty push
    with pytest.raises(ValueError, match="closed"):
        an.push(0, np.zeros(1, dtype=np.float32))

    class SplitEngine:
        def conv_form_info(self):
            return {"form": "f23", "split_f16_layers": 3, "split_f16_gate_layers": 0}

    class Inverter:
        model = SplitEngine()

    with pytest.raises(ValueError, match="float32 engine"):
        live.LiveResynthesizer(Inverter())

"""Live streams at any input rate, on the host (mbexwn_vocoder_amd/live.py): the header of the streaming resampler, its
readiness rule and the input ring's keep-from index against brute force over the definition of the resampler
(resample.py: output k is the chain over g[ph + i * up] x[jh - i]), the transposition mapping of resampled streams, and the
refusals.  No GPU."""
import os

import numpy as np
import pytest

from mbexwn_vocoder_amd import live

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_RATE = 24000
RATES = (44100, 48000, 16000, 22050, 32000, 8000, 11025, 96000)
TINY = {"sample_rate": MODEL_RATE, "hop_size": 4, "win_size": 16, "fft_size": 16, "mel_channels": 4, "fmin": 0.0, "fmax": None,
        "lin_amp_off": 1e-5, "lin_amp_scale": 1, "mel_amp_scale": 1}


def geometry(rate):
    """(up, down, half, n_taps) of the reference's filter for rate -> the model rate."""
    from mbexwn_vocoder_amd.resample import reference_filter
    taps, up, down = reference_filter(rate, MODEL_RATE)
    return up, down, (taps.size - 1) // 2, int(taps.size)


def reads(k, up, down, half, n_taps):
    """(first, last) input sample of the terms of output k of an endless sound, by enumeration of the tap indices."""
    c = k * down + half
    js = [j for j in range(max(0, c // up - n_taps // up - 2), c // up + 3) if 0 <= c - j * up < n_taps]
    return js[0], js[-1]


def test_header_declares_the_resampler_and_the_library_exports_it():
    """(that the header declares exactly these names, no other header does and the library exports them: test_abi_headers.py)"""
    from mbexwn_vocoder_amd import abi
    from mbexwn_vocoder_amd.build import HEADERS, SOURCES
    text = open(os.path.join(ROOT, "include", "mbexwn_live_resample.h")).read()
    assert "bits" in text and "desc" in text and "Refused" in text    # the promise, the descriptor layout, the refusals
    assert abi.symbols("mbexwn_live_resample.h") == ["mbxr_resample_rings"]
    assert any(hh.endswith("mbexwn_live_resample.h") for hh in HEADERS) and "resample_chain.h" in HEADERS
    assert "resample_stream.hip" in SOURCES
    assert abi.MBX_ABI_VERSION == 11


@pytest.mark.parametrize("rate", RATES)
def test_outputs_ready_against_the_definition(rate):
    """Every output below the count reads nothing behind the newest sample, the count itself does; a ready output exists in
    the final sound; a closed stream has ceil(n * up / down)."""
    up, down, half, n_taps = geometry(rate)
    for have in range(0, 401):
        count = live.outputs_ready(have, up, down, half)
        assert 0 <= count <= -(-have * up // down)
        if count:
            assert reads(count - 1, up, down, half, n_taps)[1] <= have - 1
            assert (count - 1) * down + half <= have * up - 1
        assert reads(count, up, down, half, n_taps)[1] > have - 1
        assert live.outputs_ready(have, up, down, half, closed=True) == int(np.ceil(have * up / down))
    # jh is monotone in k, so the two edges above cover every k: spelt out once, for the first 300 outputs
    last = [reads(k, up, down, half, n_taps)[1] for k in range(300)]
    assert last == sorted(last) and all(ll == (k * down + half) // up for k, ll in enumerate(last))


@pytest.mark.parametrize("rate", RATES)
def test_a_stream_shorter_than_half_the_filter_waits_for_its_end(rate):
    up, down, half, _ = geometry(rate)
    short = half // up
    assert short >= 1 and live.outputs_ready(short, up, down, half) == 0
    assert live.outputs_ready(short + 1, up, down, half) >= 1
    an = live.StreamingAnalyzer(TINY)
    an.open("s", sample_rate=rate)
    an.push("s", np.zeros(short, dtype=np.float32))
    st = an.streams["s"]
    assert st.have == 0 and st.in_have == short and an._ready(st) == 0
    an.push("s", [], last=True)
    assert st.have == -(-short * up // down) >= 1 and an._ready(st) == st.have // 4 + 1 and not an.finished("s")


@pytest.mark.parametrize("rate", RATES)
def test_input_keep_from_against_the_definition(rate):
    """The keep-from index is the smallest input sample any output from `nxt` on reads."""
    up, down, half, n_taps = geometry(rate)
    for nxt in list(range(0, 120)) + [1000, 1001, 77777]:
        want = min(reads(k, up, down, half, n_taps)[0] for k in range(nxt, nxt + 40))
        assert live.input_keep_from(nxt, up, down, half, n_taps) == want
    # what a ring of a resampled stream must hold while it is open: from there to the newest sample
    assert live.input_keep_from(0, up, down, half, n_taps) == 0


PUSHES = [
    [(1, None), (3, 1.5), (7, 0.5), (40, 2.0)],
    [(4, 1.25), (0, 3.0), (8, None), (4, 0.75)],
    [(3, 2.0)],
    [(1, 1.5), (1, None), (1, 0.5), (1, 2.0), (1, 3.0)],
]


@pytest.mark.parametrize("pushes", PUSHES)
def test_unit_ratio_is_the_present_mapping(pushes):
    """up = down = 1 (and the defaults) give what the function gave before it had them: the rule of test_live_host.py."""
    hop = 4
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
            want[tt] = last
    for got in (live.frame_factors(pushes, hop), live.frame_factors(pushes, hop, 1, 1), live.frame_factors(pushes, hop, up=1, down=1)):
        assert got.dtype == np.float32 and np.array_equal(got, want)


@pytest.mark.parametrize("rate,ratio", [(44100, (80, 147)), (48000, (1, 2)), (16000, (3, 2))])
def test_transposition_mapping_of_resampled_streams(rate, ratio):
    """A push's factor applies to the frames t whose centre, input sample (t * hop * down) // up, lies in the push; the
    frames up to ceil(n * up / down) // hop + 1 that no push decides (at most one) take the last push's factor; and a
    frame's factor is decided by the time the analysis can hand the frame out."""
    up, down, half, _ = geometry(rate)
    assert (up, down) == ratio
    hop, win = 4, 16
    rng = np.random.default_rng(rate)
    for trial in range(6):
        pushes = [(int(rng.integers(0, 30)) if trial else 1, [None, 0.5, 1.5, 2.0][int(rng.integers(0, 4))])
                  for _ in range(int(rng.integers(1, 12)))]
        if sum(count for count, _ in pushes) == 0:
            pushes.append((5, 1.75))
        n = sum(count for count, _ in pushes)
        total = -(-n * up // down) // hop + 1
        want = np.ones(total, dtype=np.float32)
        last = [1.0 if factor is None else factor for count, factor in pushes if count][-1]
        undecided = 0
        for tt in range(total):
            centre, start, found = (tt * hop * down) // up, 0, False
            for count, factor in pushes:
                if start <= centre < start + count:
                    want[tt], found = 1.0 if factor is None else factor, True
                start += count
            if not found:
                assert centre >= n
                want[tt], undecided = last, undecided + 1
        assert undecided <= 1
        got = live.frame_factors(pushes, hop, up, down)
        assert got.dtype == np.float32 and np.array_equal(got, want), (pushes, got, want)
        ff, have = live.FrameFactors(hop, up, down), 0
        for count, factor in pushes:
            ff.add(count, factor)
            have += count
            assert ff.frames == (0 if have == 0 else (have * up - 1) // (hop * down) + 1)
            assert ff.frames >= live.frames_ready(live.outputs_ready(have, up, down, half), hop, win)
        ff.close()
        assert ff.frames == total and np.array_equal(ff.take(0, total), want)


def test_refusals():
    an = live.StreamingAnalyzer(TINY)
    for bad in (0, -44100, 0.2, float("nan")):
        with pytest.raises(ValueError, match="sample_rate"):
            an.open("bad", sample_rate=bad)
    assert "bad" not in an.streams
    an.open("r", sample_rate=44100)
    an.push("r", np.zeros(10, dtype=np.float32), sample_rate=44100)
    an.push("r", np.zeros(10, dtype=np.float32))
    for other in (24000, 48000):
        with pytest.raises(ValueError, match="opened at 44100 Hz"):
            an.push("r", np.zeros(10, dtype=np.float32), sample_rate=other)
    assert an.streams["r"].in_have == 20
    # a stream without a rate of its own, or opened at the model rate: today's path and today's message
    an.open("m")
    an.open("m2", sample_rate=24000)
    for sid in ("m", "m2"):
        assert an.streams[sid].rate is None and an.streams[sid].in_slot is None
        with pytest.raises(ValueError, match="live streams take audio at the model rate 24000 Hz only; resample first "
                                             r"\(bin/generate_mel.py does it for files, resample.resample_host for arrays\)"):
            an.push(sid, np.zeros(10, dtype=np.float32), sample_rate=44100)
        an.push(sid, np.zeros(10, dtype=np.float32), sample_rate=24000)
        assert an.streams[sid].have == 10
    with pytest.raises(ValueError, match="open already"):
        an.open("r", sample_rate=48000)
    an.open("e", sample_rate=16000)
    with pytest.raises(ValueError, match="no samples"):
        an.push("e", [], last=True)
    # slots of both stores are reused
    slots = (an.streams["r"].slot, an.streams["r"].in_slot)
    an.close("r")
    an.open("again", sample_rate=8000)
    assert (an.streams["again"].slot, an.streams["again"].in_slot) == slots

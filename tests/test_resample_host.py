"""The reference's resampler on the host (mbexwn_vocoder_amd/resample.py) against the reference's own run
(tests/golden/reference_resample.npz) and the float64 evaluation of its definition (tests/resample_reference.py); the FLAC
reader and the sound-file reader of the analysis tool; the header of the audio-side entry points."""
import os
import re

import numpy as np
import pytest

import resample_reference as rr
from mbexwn_vocoder_amd import resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ulp_distance(aa, bb):
    ia, ib = (np.ascontiguousarray(vv, dtype=np.float32).view(np.int32).astype(np.int64) for vv in (aa, bb))
    ia, ib = (np.where(vv < 0, -(vv & 0x7FFFFFFF), vv) for vv in (ia, ib))
    return np.abs(ia - ib)


@pytest.mark.parametrize("in_sr", sorted({sr for sr, _ in rr.CASES}))
def test_reference_filter_gives_the_fixture_taps(in_sr):
    """Tap counts exactly; taps to at most 1 float32 ulp (bit-equal with one scipy build; the ulp allows another)."""
    taps, up, down = resample.reference_filter(in_sr, rr.OUT_SR)
    from math import gcd
    gg = gcd(in_sr, rr.OUT_SR)
    assert (up, down) == (rr.OUT_SR // gg, in_sr // gg) and isinstance(up, int) and isinstance(down, int)
    assert taps.dtype == np.float32 and taps.size % up == 0 and (taps.size // up) % 2 == 1
    if in_sr == 12345:
        assert taps.size == 72000 and (up, down) == (1600, 823)        # no taps stored: 288 KB
        return
    want = rr.fixture()[f"sr{in_sr}/taps"]
    assert taps.size == want.size
    assert int(ulp_distance(taps, want).max()) <= 1


def test_reference_filter_quirks():
    """float64 input keeps float64 taps; beta is fixed before the radius loop lowers stop_att (a ratio far enough down that
    the loop runs: the filter then is shorter than 70 dB would give, with the 70 dB window)."""
    from scipy.signal import firwin
    assert resample.reference_filter(48000, 24000, dtype=np.float64)[0].dtype == np.float64
    taps, up, down = resample.reference_filter(4_800_000, 24000, dtype=np.float64)       # tw = 2 pi * 0.005 * 0.1
    assert (up, down) == (1, 200) and 2 * ((taps.size - 1) // 2) <= 8000
    beta70 = 0.1102 * (70 - 8.7)
    assert np.array_equal(taps, firwin(taps.size, cutoff=0.9 / 200, window=("kaiser", beta70)))
    with pytest.raises(ValueError):
        resample.reference_filter(0, 24000)


def test_plan_gives_the_lengths_of_resample_poly():
    from scipy.signal import resample_poly
    for up, down, per_phase in ((1, 2, 89), (80, 147, 81), (3, 2, 45), (3, 1, 45), (1, 4, 175), (160, 147, 45), (7, 5, 3)):
        n_taps = per_phase * up
        win = np.ones(n_taps)
        for n in (0, 1, 2, 3, 10, 146, 147, 148, 1000, 1023):
            half, pre, rem, n_out = resample.plan(n_taps, up, down, n)
            assert half == (n_taps - 1) // 2 and (half + pre) % down == 0 and rem * down == half + pre
            assert n_out == -(-n * up // down)
            if n:                                              # scipy refuses an empty signal
                assert resample_poly(np.ones(n), up, down, window=win).size == n_out


@pytest.mark.parametrize("in_sr,n", rr.CASES)
def test_resample_host_against_the_definition_and_the_reference(in_sr, n):
    fx = rr.fixture()
    x, y_ref = fx[f"sr{in_sr}_n{n}/x"], fx[f"sr{in_sr}_n{n}/y"]
    taps, up, down = resample.reference_filter(in_sr, rr.OUT_SR)
    y64, bound = rr.evaluate_all(resample.scaled_taps(taps, up), up, down, x)
    got = resample.resample_host(x, in_sr, rr.OUT_SR)
    assert got.dtype == np.float32 and got.shape == y_ref.shape == y64.shape
    # one float32 rounding of the float64 value (the float64 sums differ by their order: 1e-3 of that rounding at most)
    assert np.all(np.abs(got - y64) <= rr.U32 * np.abs(y64) * 1.001 + 2.0 ** -150)
    assert np.all(np.abs(got - y_ref) <= bound)
    # the bar is not vacuous: the reference's own float32 run lies well inside it
    assert np.all(np.abs(y_ref - y64) <= bound)


def test_resample_host_edges():
    x = np.arange(5, dtype=np.float32)
    assert resample.resample_host(x, 24000, 24000) is x
    assert resample.resample_host(np.zeros(0, dtype=np.float32), 48000, 24000).shape == (0,)
    with pytest.raises(ValueError):
        resample.resample_host(np.zeros((2, 3), dtype=np.float32), 48000, 24000)


@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097])
def test_flac_decode_round_trips_encode(n):
    from mbexwn_vocoder_amd import flac
    pcm = np.random.default_rng(n).integers(-32768, 32768, size=n).astype(np.int16)
    stream = flac.encode(pcm, 24000)
    got, rate = flac.decode(stream)
    assert rate == 24000 and got.dtype == np.int16 and np.array_equal(got, pcm)


def test_flac_decode_checks_crc_md5_and_refuses_other_streams():
    from mbexwn_vocoder_amd import flac
    pcm = np.random.default_rng(5).integers(-32768, 32768, size=5000).astype(np.int16)
    stream = flac.encode(pcm, 44100)
    bad = bytearray(stream)
    bad[-1] ^= 0x01                                            # the CRC-16 of the last frame
    with pytest.raises(ValueError, match="CRC-16"):
        flac.decode(bad)
    bad = bytearray(stream)
    bad[flac.HEADER_BYTES + 2] ^= 0x01                         # inside the first frame's header
    with pytest.raises(ValueError, match="CRC-8"):
        flac.decode(bad)
    bad = bytearray(stream)
    bad[30] ^= 0xFF                                            # the MD5 of STREAMINFO
    with pytest.raises(ValueError, match="MD5"):
        flac.decode(bad)
    stereo = flac.encode(np.stack([pcm, pcm], axis=1), 44100)
    with pytest.raises(ValueError, match="soundfile"):
        flac.decode(stereo)
    with pytest.raises(ValueError, match="fLaC"):
        flac.decode(b"RIFF" + bytes(60))
    # a CONSTANT sub-frame (a silent block in other writers): one 2-sample frame of the value 7
    import hashlib
    frame = flac.frame_header(0, 2, 24000) + b"\x00" + (7).to_bytes(2, "big")
    frame += flac.crc16(frame).to_bytes(2, "big")
    md5 = hashlib.md5(np.array([7, 7], dtype="<i2").tobytes()).digest()
    got, _ = flac.decode(flac.stream_header(2, 24000, md5) + frame)
    assert np.array_equal(got, [7, 7])


def test_read_audio_scales_wav_like_libsndfile_and_refuses_channels(tmp_path):
    from scipy.io import wavfile
    from mbexwn_vocoder_amd import flac
    from mbexwn_vocoder_amd.audioio import read_audio
    try:
        import soundfile  # noqa: F401
        pytest.skip("soundfile installed: the built-in readers are not used")
    except ImportError:
        pass
    cases = {"i16": (np.array([-32768, -1, 0, 1, 32767], dtype=np.int16), 2.0 ** 15, 0),
             "i32": (np.array([-2 ** 31, -65536, 0, 65536, 2 ** 31 - 1], dtype=np.int32), 2.0 ** 31, 0),
             "u8": (np.array([0, 127, 128, 129, 255], dtype=np.uint8), 2.0 ** 7, 128)}
    for name, (data, scale, offset) in cases.items():
        path = str(tmp_path / f"{name}.wav")
        wavfile.write(path, 16000, data)
        got, rate = read_audio(path)
        assert rate == 16000 and got.dtype == np.float32 and got.ndim == 1
        assert np.array_equal(got, ((data.astype(np.float64) - offset) / scale).astype(np.float32)), name
    flt = np.array([-1.5, -0.25, 0.0, 1e-3, 1.0], dtype=np.float32)
    wavfile.write(str(tmp_path / "f32.wav"), 44100, flt)
    got, rate = read_audio(str(tmp_path / "f32.wav"))
    assert rate == 44100 and np.array_equal(got, flt)
    stereo = str(tmp_path / "stereo.wav")
    wavfile.write(stereo, 24000, np.zeros((10, 2), dtype=np.int16))
    with pytest.raises(ValueError, match="stereo.wav"):
        read_audio(stereo)
    # what resynth_mel.py writes by default can be analysed again
    audio = (0.5 * np.sin(np.arange(6000) / 20.0)).astype(np.float32)
    flac.write(str(tmp_path / "syn.flac"), audio, 24000)
    got, rate = read_audio(str(tmp_path / "syn.flac"))
    assert rate == 24000 and np.array_equal(got, flac.to_pcm16(audio).astype(np.float32) / np.float32(32768))
    (tmp_path / "x.ogg").write_bytes(b"OggS")
    with pytest.raises(RuntimeError, match="soundfile"):
        read_audio(str(tmp_path / "x.ogg"))


def test_audio_header_declares_the_audio_symbols_and_the_library_exports_them():
    """(that the header declares exactly these names, no other header does and the library exports them: test_abi_headers.py)"""
    from mbexwn_vocoder_amd import abi, engine
    text = open(os.path.join(ROOT, "include", "mbexwn_audio.h")).read()
    assert engine.AUDIO_SYMBOLS == abi.symbols("mbexwn_audio.h") == ["mbxa_resample_poly"]
    assert int(re.search(r"#define MBXA_RESAMPLE_TILE (\d+)", text).group(1)) == resample.DEVICE_TILE

"""The fixed-lag F0 decoder's host side (no GPU needed): the definition f0decode.viterbi_lag_host
against the prefix construction -- frame t of viterbi_host on the frames 0 .. t + lag --, on the adversarial sound of
test_f0decode_host.py and on hand-made tables; LagDecoder's cut invariance; the count rule and the refusals; the header
mbexwn_live_contour.h, its binding and the entry points' refusals on the host; the tools' flags.  Every comparison is on bits.

The two counts on the adversarial sound come from the table of the definition's measurement (161 frames, inner frames
[4:-4], more than 50 cents off): lag 8 has none and equals the whole decode, lag 0 has 21 -- "at least 10" is half of that."""
import ctypes
import importlib.util
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import c_headers
from mbexwn_vocoder_amd import abi, engine, f0decode, f0track, live

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")
SR, HOP = 24000, 300
f32 = np.float32
TINY = {"sample_rate": SR, "hop_size": 16, "win_size": 48, "fft_size": 64, "mel_channels": 8, "fmin": 0.0, "fmax": None,
        "lin_amp_off": 1e-5, "lin_amp_scale": 1, "mel_amp_scale": 1}


def bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float32).view(np.uint32)


def same(one, other):
    return all(np.array_equal(bits(aa), bits(bb)) for aa, bb in zip(one, other))


def cents(f0, true):
    return 1200.0 * np.log2(np.maximum(np.asarray(f0, np.float64), 1e-9) / true)


def load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(BIN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def adversarial(seed=1):
    """The sound of tests/test_f0decode_host.py: 110 Hz, strong even harmonics, the odd ones swelling and fading at 3 Hz."""
    n = 48000
    t = np.arange(n) / SR
    am = 0.3 + 0.2 * np.sin(2 * np.pi * 3 * t)
    x = 0.3 * sum(((1 if h % 2 == 0 else am) / h) * np.sin(2 * np.pi * h * 110 * t + h) for h in range(1, 13))
    return (x + 1e-3 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def random_tables(rng, frames):
    """The hand-made tables of tests/test_gpu_f0decode.py for one item: costs from {0, 0.25, 0.5, 1} and periods from {50,
    100, 200}, so that ties occur; 0 .. 7 used slots per frame -- frames without an available lag among them --; NaN, inf,
    negative and 1e7 entries sprinkled over both tables."""
    period = rng.choice(np.array([50, 100, 200], np.float32), size=(frames, 8))
    cost = rng.choice(np.array([0, 0.25, 0.5, 1], np.float32), size=(frames, 8))
    dprime = rng.random((frames, 8)).astype(np.float32)
    count = rng.integers(0, 8, size=frames)
    unused = np.arange(7)[None, :] >= count[:, None]
    period[:, :7][unused] = 0
    cost[:, :7][unused] = np.inf
    period[:, 7] = 0
    for tab in (period, cost):
        where = rng.random(tab.shape) < 0.03
        tab[where] = rng.choice(np.array([np.nan, np.inf, -0.5, 1e7], np.float32), size=int(where.sum()))
    return period, cost, dprime


@pytest.fixture(scope="module")
def adversarial_tables():
    """The candidate tables of the adversarial sound and its whole decode, computed once."""
    prm, dec = f0track.params(SR), f0decode.decode_params()
    tables = f0decode.candidates_host(*f0track.difference_host(adversarial(), np.arange(161) * HOP, prm), prm, dec)
    return dec, tables, f0decode.viterbi_host(*tables, SR, dec)


def prefix_construction(tables, dec, lag):
    """Frame t of viterbi_host on the frames 0 .. min(t + lag, T - 1): what "decided once frame t + lag is seen" means."""
    T = tables[0].shape[0]
    f0, per = np.zeros(T, f32), np.zeros(T, f32)
    for t in range(T):
        a, b = f0decode.viterbi_host(*(tt[:min(t + lag + 1, T)] for tt in tables), SR, dec)
        f0[t], per[t] = a[t], b[t]
    return f0, per


# ------------------------------------------------------------------------------------------------------------------------
# the definition
# ------------------------------------------------------------------------------------------------------------------------
def test_the_lag_does_the_work_on_the_adversarial_sound(adversarial_tables):
    dec, tables, whole = adversarial_tables
    wrong = {}
    for lag in (0, 8):
        f0, per = f0decode.viterbi_lag_host(*tables, SR, dec, lag)
        assert f0.dtype == per.dtype == np.float32 and f0.shape == per.shape == (161,)
        wrong[lag] = int(np.count_nonzero(np.abs(cents(f0[4:-4], 110.0)) > 50))
        print(f"lag {lag}: {wrong[lag]} of 153 inner frames more than 50 cents off")
        assert same((f0, per), prefix_construction(tables, dec, lag)), lag
        if lag == 8:
            assert same((f0, per), whole)                                # from lag 8 on: the whole-sound decode, bit for bit
    assert wrong[8] == 0 and wrong[0] >= 10


def test_hand_made_tables_equal_the_prefix_construction():
    rng = np.random.default_rng(41)
    voiced = 0
    for frames, w_jump, w_switch in ((37, 4.0, 0.5), (37, 0.0, 0.0), (60, 4.0, 0.0), (23, 0.0, 0.5)):
        tables = random_tables(rng, frames)
        assert np.any(np.all(~np.isfinite(tables[1][:, :7]) | (tables[0][:, :7] < 1), axis=1))      # frames without a lag
        dec = f0decode.decode_params(w_jump=w_jump, w_switch=w_switch)
        for lag in (0, 1, 2, 5, frames - 2, frames - 1, 128):
            got = f0decode.viterbi_lag_host(*tables, SR, dec, lag)
            assert same(got, prefix_construction(tables, dec, lag)), (frames, w_jump, w_switch, lag)
            assert np.all(np.isin(got[0], [0, SR / 50, SR / 100, SR / 200]))       # no sprinkled entry reaches f0
            voiced += int(np.count_nonzero(got[0]))
            if lag >= frames - 1:
                assert same(got, f0decode.viterbi_host(*tables, SR, dec)), (frames, lag)
    assert voiced > 0


def test_short_items_and_refusals():
    rng = np.random.default_rng(42)
    dec = f0decode.decode_params()
    for frames in (0, 1, 2):
        tables = tuple(tt[:frames] for tt in random_tables(rng, 2))
        for lag in (0, 1, 128):
            got = f0decode.viterbi_lag_host(*tables, SR, dec, lag)
            assert got[0].shape == got[1].shape == (frames,) and got[0].dtype == np.float32
            if lag >= frames - 1:
                assert same(got, f0decode.viterbi_host(*tables, SR, dec))
            assert same(got, prefix_construction(tables, dec, lag))
    tables = random_tables(rng, 4)
    with pytest.raises(ValueError, match="three tables"):
        f0decode.viterbi_lag_host(tables[0][:, :7], tables[1], tables[2], SR, dec, 2)
    with pytest.raises(ValueError, match="sample_rate"):
        f0decode.viterbi_lag_host(*tables, 0, dec, 2)
    with pytest.raises(ValueError, match="f0 decode"):
        f0decode.viterbi_lag_host(*tables, SR, {"n_cand": 3}, 2)
    with pytest.raises(ValueError, match="lag"):
        f0decode.viterbi_lag_host(*tables, SR, dec, 129)
    assert "lag" not in f0decode.DECODE_KEYS and sorted(dec) == sorted(f0decode.DECODE_KEYS)     # the lag is no key of dec


def test_check_lag_and_the_count_rule():
    for good in (0, 1, 8, 128, np.int64(5), np.int32(0)):
        assert f0decode.check_lag(good) == int(good) and type(f0decode.check_lag(good)) is int
    for bad in (True, False, np.bool_(True), -1, 129, 8.0, 2.5, "8", None, [8], np.float32(3)):
        with pytest.raises(ValueError, match="lag"):
            f0decode.check_lag(bad)
    rule = f0decode.lag_frames_decided
    assert [rule(done, 8) for done in (0, 1, 8, 9, 20)] == [0, 0, 0, 1, 12]
    assert [rule(done, 0) for done in (0, 1, 7)] == [0, 1, 7]
    assert [rule(done, 8, True) for done in (0, 1, 8, 20)] == [0, 1, 8, 20]
    assert rule(5, 128) == 0 and rule(5, 128, closed=True) == 5


def test_lag_decoder_is_cut_invariant(adversarial_tables):
    dec, adv, _ = adversarial_tables
    rng = np.random.default_rng(43)
    hand = random_tables(rng, 300)
    for name, tables in (("adversarial", adv), ("hand-made", hand)):
        T = tables[0].shape[0]
        for lag in (0, 1, 8, 63, 128):
            want = f0decode.viterbi_lag_host(*tables, SR, dec, lag)
            plans = [[int(rng.integers(0, 40)) for _ in range(60)], [1] * T, [150] * 2, [0, 0, T, 0]]
            for plan in plans:
                decoder = f0decode.LagDecoder(SR, dec, lag)
                parts, pos = [], 0
                for count in plan:
                    count = min(count, T - pos)
                    parts.append(decoder.push(*(tt[pos:pos + count] for tt in tables)))
                    pos += count
                    assert decoder.done == pos and decoder.decided == f0decode.lag_frames_decided(pos, lag)
                    assert parts[-1][0].shape == parts[-1][1].shape and parts[-1][0].dtype == np.float32
                    assert len(decoder.words) <= lag + 1 and len(decoder.periods) <= lag + 1        # the state is a ring
                parts.append(decoder.push(*(tt[pos:] for tt in tables)))
                parts.append(decoder.push(*(tt[:0] for tt in tables), last=True))      # `last` on an empty push
                assert decoder.decided == decoder.done == T
                got = tuple(np.concatenate([pp[kk] for pp in parts]) for kk in (0, 1))
                assert same(got, want), (name, lag, plan[:4])
    # `last` together with the frames, and a decoder that sees nothing
    decoder = f0decode.LagDecoder(SR, dec, 8)
    assert same(decoder.push(*adv, last=True), f0decode.viterbi_host(*adv, SR, dec))
    decoder = f0decode.LagDecoder(SR, dec, 8)
    assert decoder.push(*(tt[:0] for tt in adv), last=True)[0].shape == (0,)
    with pytest.raises(ValueError, match="lag"):
        f0decode.LagDecoder(SR, dec, -1)
    with pytest.raises(ValueError, match="sample_rate"):
        f0decode.LagDecoder(0, dec, 1)


# ------------------------------------------------------------------------------------------------------------------------
# the streams' refusals
# ------------------------------------------------------------------------------------------------------------------------
def prm_of(window, tau_min, tau_max):
    return {"sample_rate": SR, "window": window, "tau_min": tau_min, "tau_max": tau_max, "threshold": 0.15, "e_min": 0.0}


def test_open_refuses_what_it_cannot_decode():
    an = live.StreamingAnalyzer(TINY)
    prm, dec = prm_of(64, 2, 5), f0decode.decode_params()
    with pytest.raises(ValueError, match="whole sound"):                 # as before: a decoder without a lag
        an.open("x", f0_params=prm, f0_decode=dec)
    with pytest.raises(ValueError, match="f0_params"):
        an.open("x", f0_lag=8)
    with pytest.raises(ValueError, match="f0_params"):
        an.open("x", f0_lag=8, f0_decode=dec)
    for bad in (True, -1, 129, 2.0, "8"):
        with pytest.raises(ValueError, match="lag"):
            an.open("x", f0_params=prm, f0_lag=bad)
    with pytest.raises(ValueError, match="f0 decode"):
        an.open("x", f0_params=prm, f0_lag=8, f0_decode={"n_cand": 3})
    assert not an.streams and an.f0_lag is None
    an.open("x", f0_params=prm, f0_lag=8)                                 # None: the default decode_params
    assert an.f0_lag == 8 and live._same_decode(an.f0_decode, dec) and an.streams["x"].f0_decided == 0
    an.open("y", f0_params=prm, f0_lag=8, f0_decode=dec)
    an.open("r", sample_rate=44100, f0_params=prm, f0_lag=8)
    for other in (dict(f0_lag=7), dict(f0_lag=8, f0_decode=f0decode.decode_params(w_jump=2.0)), dict(),
                  dict(f0_lag=8, f0_decode=f0decode.decode_params(n_cand=3))):
        with pytest.raises(ValueError, match="share one"):                # one (f0_params, f0_decode, f0_lag) per analyzer
            an.open("z", f0_params=prm, **other)
    with pytest.raises(ValueError, match="share one"):
        an.open("z", f0_params=prm_of(64, 2, 7), f0_lag=8)
    an.open("plain")                                                      # a stream without a tracker is always welcome
    assert sorted(an.streams, key=str) == ["plain", "r", "x", "y"] and an.device is None
    # and the other way round: an analyzer whose tracking streams have no lag takes no decoding stream
    an = live.StreamingAnalyzer(TINY)
    an.open("x", f0_params=prm)
    with pytest.raises(ValueError, match="share one"):
        an.open("y", f0_params=prm, f0_lag=8)
    an.close("x")
    an.open("y", f0_params=prm, f0_lag=0)                                 # once they are gone, the next one sets the triple
    assert an.f0_lag == 0
    lr = object.__new__(live.LiveResynthesizer)
    lr.analyzer = an
    with pytest.raises(ValueError, match="whole sound"):
        lr.open("z", f0_source="audio", f0_decode=dec)
    with pytest.raises(ValueError, match="f0_source='audio'"):
        lr.open("z", f0_lag=8)
    with pytest.raises(ValueError, match="f0_source='audio'"):
        lr.open("z", f0_source="net", f0_lag=8, f0_decode=dec)


def test_lookahead_adds_the_lag():
    import types
    lr = object.__new__(live.LiveResynthesizer)
    lr.synthesizer = types.SimpleNamespace(lookahead_ms=12.5)
    lr.analyzer = live.StreamingAnalyzer(dict(TINY, hop_size=300, win_size=1200, fft_size=2048))
    base = lr.lookahead_ms_for(f0_source="audio")
    assert lr.lookahead_ms_for(f0_source="audio", f0_lag=None) == base
    assert lr.lookahead_ms_for(f0_source="audio", f0_lag=0) == base
    assert lr.lookahead_ms_for(f0_source="audio", f0_lag=8) == base + 100.0         # 8 frames at hop 300 / 24 kHz
    both = lr.lookahead_ms_for(44100, 48000, f0_source="audio", f0_lag=3)           # (the resamplers' parts are added behind it)
    assert abs(both - (lr.lookahead_ms_for(44100, 48000, f0_source="audio") + 37.5)) < 1e-9
    with pytest.raises(ValueError, match="lag"):
        lr.lookahead_ms_for(f0_source="audio", f0_lag=129)


def test_the_offline_calls_refuse_a_lag_without_a_decoder(tmp_path):
    from mbexwn_vocoder_amd import batched
    from mbexwn_vocoder_amd.analysis import generate_mels
    from mbexwn_vocoder_amd.mel_inverter import MELInverter, create_synthetic_model_dir
    for func, name in ((generate_mels, "f0_lag"), (batched.analyse_for_synthesis, "f0_lag"), (batched.run_audio_job, "f0_lag"),
                       (MELInverter.transform_audio, "f0_lag"), (MELInverter.track_f0, "f0_lag")):
        params = inspect.signature(func).parameters
        assert params[name].default is None
        assert [pp for pp in params if params[pp].kind is not inspect.Parameter.VAR_KEYWORD][-1] == name     # the trailing one
    from mbexwn_vocoder_amd.config import canonical_config
    cfg = canonical_config("SPEECH")["preprocess_config"]
    snd = adversarial()[:6000]
    with pytest.raises(ValueError, match="f0_lag"):
        generate_mels([snd], [SR], cfg, on_device=False, f0_out=[], f0_lag=8)
    with pytest.raises(ValueError, match="lag"):
        generate_mels([snd], [SR], cfg, on_device=False, f0_out=[], f0_decode=f0decode.decode_params(), f0_lag=129)
    inv = MELInverter.host_only(create_synthetic_model_dir(str(tmp_path / "model"), "SPEECH"))
    with pytest.raises(ValueError, match="f0_lag"):
        inv.transform_audio([snd], [SR], ["a.wav"], f0_source="audio", f0_lag=8)
    with pytest.raises(ValueError, match="f0_lag"):
        inv.track_f0(snd, SR, f0_lag=8)
    # the host path: the contour of a lagged call is viterbi_lag_host of the sound's candidates
    prm, dec = f0track.params(SR), f0decode.decode_params()
    tables = f0decode.candidates_host(*f0track.difference_host(snd, np.arange(21) * HOP, prm), prm, dec)
    for lag in (0, 8):
        _, f0, per = inv.track_f0(snd, SR, decode=dec, f0_lag=lag)
        assert same((f0, per), f0decode.viterbi_lag_host(*tables, SR, dec, lag)), lag
    _, f0, per = inv.track_f0(snd, SR, decode=dec)
    assert same((f0, per), f0decode.viterbi_host(*tables, SR, dec))


# ------------------------------------------------------------------------------------------------------------------------
# the header, the table, the entry points
# ------------------------------------------------------------------------------------------------------------------------
NAMES = ["mbxv_f0_candidate_frames", "mbxv_lag_state_words", "mbxv_decode_f0_frames"]


def test_the_header_and_its_binding(tmp_path):
    from mbexwn_vocoder_amd.build import HEADERS, SOURCES
    assert "mbexwn_live_contour.h" in c_headers.header_names() and abi.symbols("mbexwn_live_contour.h") == NAMES
    assert [pp[0] for pp in c_headers.prototypes(c_headers.read_code("mbexwn_live_contour.h"))] == NAMES
    assert any(hh.endswith("mbexwn_live_contour.h") for hh in HEADERS) and "f0_lag.hip" in SOURCES and "f0_viterbi.h" in HEADERS
    text = open(os.path.join(ROOT, "include", "mbexwn_live_contour.h")).read()
    assert all(word in text for word in ("THE PROMISE", "THE DEFINITION", "HOST pointers", "AT MOST ONE ROW", '"f0 candidate frames:"',
                                         '"decode f0 frames:"', "MBX_ERR_INVALID_ARGUMENT"))
    # the pinned export lists of the older headers did not move
    assert abi.symbols("mbexwn_contour.h") == ["mbxc_f0_candidates", "mbxc_decode_f0"]
    assert abi.symbols("mbexwn_live_pitch.h") == ["mbxt_f0_frames"] and abi.MBX_ABI_VERSION == 11
    table = {row[0]: row for row in abi.TABLE["mbexwn_live_contour.h"]}
    assert table["mbxv_f0_candidate_frames"][2][12] is table["mbxv_f0_candidate_frames"][2][13] is ctypes.POINTER(ctypes.c_float)
    assert table["mbxv_lag_state_words"][1] is ctypes.c_size_t
    src = tmp_path / "use.c"
    src.write_text('#include "mbexwn_live_contour.h"\nint main(void){ (void)mbxv_f0_candidate_frames; (void)mbxv_lag_state_words; '
                   '(void)mbxv_decode_f0_frames; return 0; }\n')
    res = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", c_headers.INCLUDE, "-c", str(src), "-o", str(tmp_path / "use.o")],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr                               # the header is plain C
    lib = engine.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.mbxv_lag_state_words() == 32 + 256 * 17                   # the head, then 256 frames of a word, 8 periods, 8 dprimes
    # the kernels share their code: one step, one candidates function, one ring fetch
    csrc = os.path.join(ROOT, "mbexwn_vocoder_amd", "csrc")
    lag, decode, stream = (open(os.path.join(csrc, name)).read() for name in ("f0_lag.hip", "f0_decode.hip", "f0_stream.hip"))
    shared, frame = open(os.path.join(csrc, "f0_viterbi.h")).read(), open(os.path.join(csrc, "f0_frame.h")).read()
    for text in (lag, shared):
        assert "#pragma clang fp contract(off)" in text and "fmaf" not in text and "getenv" not in text and "hipMalloc" not in text
    assert "f0_viterbi_step(" in shared and lag.count("f0_viterbi_step(") == decode.count("f0_viterbi_step(") == 1
    assert "f0_frame_candidates(" in frame and lag.count("f0_frame_candidates(") == decode.count("f0_frame_candidates(") == 1
    assert "F0RingFetch(" in frame and lag.count("F0RingFetch(") == stream.count("F0RingFetch(") == 1


def test_the_c_entry_points_refuse_on_the_host():
    """Both entry points check every argument before they touch the device: the refusals need no GPU."""
    lib = engine.load_library()
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    fpp = ctypes.POINTER(ctypes.c_float)

    def host(values):
        arr = np.asarray(values, np.float32)
        return arr, arr.ctypes.data_as(fpp)

    th, ww = host([0.1, 0.2]), host([0.5, 0.5])
    good = dict(rings=ptr, n_slots=1, ring_samples=2048, desc=ptr, n_streams=1, max_new_frames=1, hop=300, sample_rate=24000,
                window=1024, tau_min=24, tau_max=437, e_min=0.0, thresholds=th[1], weights=ww[1], n_thresholds=2, n_cand=7, period=ptr,
                cost=ptr, dprime=ptr)

    def call(**kw):
        aa = dict(good, **kw)
        return lib.mbxv_f0_candidate_frames(aa["rings"], aa["n_slots"], aa["ring_samples"], aa["desc"], aa["n_streams"],
                                            aa["max_new_frames"], aa["hop"], aa["sample_rate"], aa["window"], aa["tau_min"],
                                            aa["tau_max"], ctypes.c_float(aa["e_min"]), aa["thresholds"], aa["weights"],
                                            aa["n_thresholds"], aa["n_cand"], aa["period"], aa["cost"], aa["dprime"], None)

    broken = [host(vv) for vv in ([0.1, np.nan], [0.2, 0.1], [0.1, 0.1], [0.5, -1.0], [np.inf, 0.5])]
    cases = [{name: None} for name in ("rings", "desc", "thresholds", "weights", "period", "cost", "dprime")]
    # what check_f0_stream refuses ...
    cases += [{"n_streams": -1}, {"n_streams": 65536}, {"max_new_frames": -1}, {"n_slots": 0}, {"hop": 0}, {"window": 0}, {"window": 96},
              {"window": 2112}, {"tau_max": 1}, {"tau_min": 437}, {"window": 2048, "tau_max": 2049, "ring_samples": 8192},
              {"sample_rate": 0}, {"e_min": float("nan")}, {"ring_samples": 0}, {"ring_samples": 1000}, {"ring_samples": 1024}]
    # ... and what fill_f0_candidates refuses
    cases += [{"n_thresholds": 0}, {"n_thresholds": 17}, {"n_cand": 0}, {"n_cand": 8}]
    cases += [{"thresholds": bb[1]} for bb in broken[:3]] + [{"weights": bb[1]} for bb in broken[3:]]
    for kw in cases:
        assert call(**kw) == 1, kw                                       # MBX_ERR_INVALID_ARGUMENT
        message = lib.mbx_last_error().decode()
        assert message.startswith("f0 candidate frames:") and len(message) > 24, kw
    assert call(n_streams=0) == 0 and call(max_new_frames=0) == 0        # nothing to do

    good = dict(period=ptr, cost=ptr, dprime=ptr, desc=ptr, n_streams=1, max_new_frames=4, hop=300, state=ptr, n_slots=1, lag=8,
                sample_rate=24000, w_jump=4.0, w_switch=0.5, f0=ptr, periodicity=ptr, max_out=12)

    def decode(**kw):
        aa = dict(good, **kw)
        return lib.mbxv_decode_f0_frames(aa["period"], aa["cost"], aa["dprime"], aa["desc"], aa["n_streams"], aa["max_new_frames"],
                                         aa["hop"], aa["state"], aa["n_slots"], aa["lag"], aa["sample_rate"],
                                         ctypes.c_float(aa["w_jump"]), ctypes.c_float(aa["w_switch"]), aa["f0"], aa["periodicity"],
                                         aa["max_out"], None)

    cases = [{name: None} for name in ("period", "cost", "dprime", "desc", "state", "f0", "periodicity")]
    cases += [{"n_streams": -1}, {"n_streams": 65536}, {"max_new_frames": -1}, {"hop": 0}, {"n_slots": 0}, {"lag": -1}, {"lag": 129},
              {"max_out": 11}, {"max_out": 0}, {"lag": 128, "max_out": 131}, {"sample_rate": 0}]
    cases += [{key: vv} for key in ("w_jump", "w_switch") for vv in (float("nan"), -0.5, 1.5e6, float("inf"))]
    for kw in cases:
        assert decode(**kw) == 1, kw
        message = lib.mbx_last_error().decode()
        assert message.startswith("decode f0 frames:") and len(message) > 20, kw
    assert decode(n_streams=0) == 0


# ------------------------------------------------------------------------------------------------------------------------
# the tools
# ------------------------------------------------------------------------------------------------------------------------
def test_stream_transpose_flags(capsys):
    tool = load_script("stream_transpose")
    args = tool.make_parser().parse_args(["a.wav", "-o", "out.wav"])
    assert (args.pitch_decode, args.pitch_lag, args.pitch_jump, args.pitch_switch) == ("greedy", 8, 4.0, 0.5)
    args = tool.make_parser().parse_args(["a.wav", "-o", "out.wav", "--f0-source", "audio", "--pitch-decode", "viterbi", "--pitch-lag", "12",
                                          "--pitch-jump", "2.5", "--pitch-switch", "0"])
    assert (args.pitch_decode, args.pitch_lag, args.pitch_jump, args.pitch_switch) == ("viterbi", 12, 2.5, 0.0)
    assert set(vars(args)) == set(inspect.signature(tool.main).parameters)            # every parsed name is an argument of main
    for flag, value in (("--pitch-decode", "pyin"), ("--pitch-lag", "-1"), ("--pitch-lag", "129"), ("--pitch-lag", "2.5"),
                        ("--pitch-jump", "nan"), ("--pitch-switch", "2e6")):
        with pytest.raises(SystemExit) as exc:
            tool.make_parser().parse_args(["a.wav", "-o", "out.wav", flag, value])
        assert exc.value.code == 2 and flag in capsys.readouterr().err
    params = inspect.signature(tool.stream_file).parameters
    assert params["f0_lag"].default is None and params["f0_decode"].default is None


def test_stream_transpose_refuses_a_decoder_without_the_audio_source(tmp_path):
    from scipy.io import wavfile
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    model = create_synthetic_model_dir(str(tmp_path / "model"), "SPEECH")
    snd = tmp_path / "a.wav"
    wavfile.write(str(snd), SR, np.zeros(100, dtype=np.float32))
    res = subprocess.run([sys.executable, os.path.join(BIN, "stream_transpose.py"), str(snd), "-o", str(tmp_path / "no" / "out.wav"),
                          "--model_id", model, "--pitch-decode", "viterbi"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 1 and "--f0-source audio" in res.stderr and not os.path.exists(tmp_path / "no")


def test_file_tools_take_and_forward_the_lag(tmp_path, capsys, monkeypatch):
    from scipy.io import wavfile
    from mbexwn_vocoder_amd import batched
    from mbexwn_vocoder_amd.fileio import load_var
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    tool = load_script("transform_audio")
    assert tool.make_parser().parse_args(["a.wav", "-o", "out"]).pitch_lag is None
    args = tool.make_parser().parse_args(["a.wav", "-o", "out", "--pitch-decode", "viterbi", "--pitch-lag", "8"])
    assert args.pitch_lag == 8 and set(vars(args)) == set(inspect.signature(tool.main).parameters)
    for value in ("-1", "129", "x"):
        with pytest.raises(SystemExit) as exc:
            tool.make_parser().parse_args(["a.wav", "-o", "out", "--pitch-lag", value])
        assert exc.value.code == 2 and "--pitch-lag" in capsys.readouterr().err
    model = create_synthetic_model_dir(str(tmp_path / "model"), "SPEECH")
    snd = adversarial()[:12000]
    wav = str(tmp_path / "adv.wav")
    wavfile.write(wav, SR, snd)
    res = subprocess.run([sys.executable, os.path.join(BIN, "transform_audio.py"), wav, "-o", str(tmp_path / "no"), "--model_id", model,
                          "--f0-source", "audio", "--pitch-lag", "8"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 1 and "--pitch-decode viterbi" in res.stderr and not os.path.exists(tmp_path / "no")
    seen = []
    monkeypatch.setattr(batched, "run_ranks", lambda script, argv, *rest, **kw: seen.append(list(argv)) or 0)
    for extra, want in (({"f0_source": "audio", "pitch_decode": "viterbi"}, ["--pitch-decode", "viterbi"]),
                        ({"f0_source": "audio", "pitch_decode": "viterbi", "pitch_lag": 8}, ["--pitch-decode", "viterbi", "--pitch-lag", "8"]),
                        ({"write_f0": True, "pitch_decode": "viterbi", "pitch_lag": 0}, ["--pitch-decode", "viterbi", "--pitch-lag", "0"])):
        with pytest.raises(SystemExit) as exc:
            tool.main([wav], str(tmp_path / "out"), model_id=model, gpus=2, **extra)
        assert exc.value.code == 0
        argv = seen.pop()
        got = [aa for ii, aa in enumerate(argv) if "--pitch" in aa or (ii and "--pitch" in argv[ii - 1])]
        assert got == want
        assert tool.make_parser().parse_args(argv).pitch_lag == extra.get("pitch_lag")        # the rank's parser takes it
    # generate_mel.py writes the lagged contour
    gen = load_script("generate_mel")
    assert inspect.signature(gen.main).parameters["pitch_lag"].default is None
    prm, dec = f0track.params(SR), f0decode.decode_params()
    tables = f0decode.candidates_host(*f0track.difference_host(snd, np.arange(41) * HOP, prm), prm, dec)
    for lag in (0, 8):
        out = str(tmp_path / f"lag{lag}")
        res = subprocess.run([sys.executable, os.path.join(BIN, "generate_mel.py"), wav, "-o", out, "--model_id", model, "--host",
                              "--write-f0", "--pitch-decode", "viterbi", "--pitch-lag", str(lag), "-q"], capture_output=True, text=True,
                             timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        mell = load_var(os.path.join(out, "adv.mell"))["mell"]
        _, f0, per = f0track.read_f0(os.path.join(out, "adv.f0"), n_frames=mell.shape[1])
        assert mell.shape[1] == 41 and same((f0, per), f0decode.viterbi_lag_host(*tables, SR, dec, lag)), lag
    res = subprocess.run([sys.executable, os.path.join(BIN, "generate_mel.py"), wav, "-o", str(tmp_path / "no"), "--model_id", model,
                          "--host", "--write-f0", "--pitch-lag", "8"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 1 and "--pitch-decode viterbi" in res.stderr

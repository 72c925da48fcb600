"""The host side of the streaming F0 tracker, without a GPU: the readiness rule against the
definition ``f0track.track_f0_host``, the frame counts, the analyzer's plan with and without tracking streams, the causal
fill ``f0track.fill_hold``, the look-ahead and the new header.  Every comparison of values is on bits."""
import os
import subprocess
import types

import numpy as np
import pytest

import c_headers
from mbexwn_vocoder_amd import abi, f0track, live, live_plan
from test_live_host import TINY                # hop 4, win 16, 24 kHz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (window, tau_min, tau_max, hop): the smallest frame with an odd L = 69, and the defaults at 24 kHz, L = 1461
SETS = [(64, 2, 5, 16), (1024, 24, 437, 300)]


def bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float32).view(np.uint32)


def prm_of(window, tau_min, tau_max):
    return {"sample_rate": 24000, "window": window, "tau_min": tau_min, "tau_max": tau_max, "threshold": 0.15, "e_min": 0.0}


@pytest.mark.parametrize("window,tau_min,tau_max,hop", SETS)
def test_the_readiness_rule_is_exact(window, tau_min, tau_max, hop):
    """Frame t of seeded noise has its final bits as soon as the rule hands it out (m = t * hop - L // 2 + L samples), and
    not earlier: the rule waits for exactly what the frame reads.

    "Not earlier" needs a second fixture.  The frame's last sample, m - 1, is read by d[tau_max] alone, and the pick ends at
    tau_max - 1: while that sample is finite it cannot change f0 or periodicity (measured: no t of the noise differs in
    periodicity at m - 1, with either parameter set, and the definition says why).  It decides the frame all the same,
    through the rule for samples that are not finite: with an inf at m - 1 EVERY frame has other periodicity bits at m - 1
    than at m, which is what the kernel's promise includes."""
    n, L, prm = 3000, window + tau_max, prm_of(window, tau_min, tau_max)
    x = (0.1 * np.random.default_rng(11).standard_normal(n)).astype(np.float32)
    frames = [t for t in range(n // hop + 1) if t * hop - L // 2 + L <= n]      # the others wait for the close
    assert len(frames) >= 8
    want_f0, want_per = f0track.track_f0_host(x, np.asarray(frames) * hop, prm)
    for kk, t in enumerate(frames):
        m, centre = t * hop - L // 2 + L, np.asarray([t * hop])
        assert live_plan.f0_frames_ready(m, hop, L) == t + 1 and live_plan.f0_frames_ready(m - 1, hop, L) == t
        f0, per = f0track.track_f0_host(x[:m], centre, prm)
        assert bits(f0)[0] == bits(want_f0)[kk] and bits(per)[0] == bits(want_per)[kk], t
        _, per = f0track.track_f0_host(x[:m - 1], centre, prm)
        assert bits(per)[0] == bits(want_per)[kk], t                     # finite noise: sample m - 1 is read, and decides nothing
        spiked = x.copy()
        spiked[m - 1] = np.inf
        whole, ready, before = (f0track.track_f0_host(ss, centre, prm) for ss in (spiked, spiked[:m], spiked[:m - 1]))
        assert (whole[0][0], whole[1][0]) == (ready[0][0], ready[1][0]) == (0.0, 1.0), t
        assert bits(before[1])[0] == bits(want_per)[kk] != bits(whole[1])[0], t     # one sample early: not the frame's bits


def test_readiness_counts():
    ready, total = live_plan.f0_frames_ready, live_plan.frames_total
    for L, hop in ((69, 16), (1461, 300), (70, 16), (1460, 300)):         # odd and even L
        need = L - L // 2
        assert need == (L + 1) // 2
        assert ready(0, hop, L) == 0 and ready(need - 1, hop, L) == 0
        assert ready(need, hop, L) == 1 and ready(need + hop - 1, hop, L) == 1 and ready(need + hop, hop, L) == 2
        for have in (0, 1, need - 1, need, need + hop, 10 * hop + 3):
            assert ready(have, hop, L, closed=True) == total(have, hop) == have // hop + 1
            # frame t is ready exactly when t * hop - L // 2 + L <= have
            assert ready(have, hop, L) == sum(t * hop - L // 2 + L <= have for t in range(have // hop + 2))
    assert (ready(34, 16, 69), ready(35, 16, 69), ready(51, 16, 69)) == (0, 1, 2)
    assert (ready(730, 300, 1461), ready(731, 300, 1461), ready(1031, 300, 1461)) == (0, 1, 2)


def samples(count, seed=0):
    return np.random.default_rng(seed).standard_normal(count).astype(np.float32)


def plain_case(f0_for=()):
    an = live.StreamingAnalyzer(TINY, slots=2)
    prm = prm_of(64, 2, 5)
    for sid, rate in (("a", None), ("b", 48000), ("c", None)):
        an.open(sid, sample_rate=rate, **({"f0_params": prm} if sid in f0_for else {}))
    an.push("a", samples(100, 1))
    an.push("b", samples(350, 2))
    an.push("c", samples(40, 3), last=True)
    return an


def test_a_plan_without_tracking_streams_is_todays_plan():
    """Every field the plan had before the tracker, on a worked case with a resampled and a closed stream: the values follow
    from the rules of live_plan.py alone (hop 4, win 16: frame t needs 4 t + 8 samples)."""
    plan = plain_case().plan()
    assert plan.rows == [("a", 24), ("b", 37), ("c", 11)] and (plan.S, plan.R, plan.T) == (3, 1, 0)
    assert plan.resampled == [1] and plan.counts == [100, 350, 40] and plan.offsets == [0, 100, 450]
    assert (plan.body, plan.samples) == (16 * 3 + 20, 490)
    assert plan.append.tolist() == [[0, 0, 100, 0], [1, 0, 0, 100], [2, 0, 40, 450]]
    assert plan.frames.tolist() == [[0, 0, 24, -1], [1, 0, 37, -1], [2, 0, 11, 40]]
    assert plan.in_append.tolist() == [[0, 0, 350, 100]] and plan.in_resample.tolist() == [[0, 1, 0, 153, -1, 0]]
    assert plan.groups == [(48000, 0, 1, 153)] and (plan.max_new, plan.max_model, plan.max_in) == (37, 100, 350)
    assert plan.ring_needed == 153 and plan.in_ring_needed == 350 and plan.fresh == [0, 1, 2]
    assert sorted(vars(plan)) == sorted(["rows", "resampled", "S", "R", "T", "counts", "offsets", "queues", "body", "samples",
                                         "append", "frames", "in_append", "in_resample", "groups", "max_new", "max_model",
                                         "max_in", "ring_needed", "in_ring_needed", "fresh"])
    # and a tracking stream beside them changes nothing of theirs but the order of the rows: the tracking ones come first
    mixed = plain_case(f0_for=("c",)).plan()
    assert mixed.rows == [("c", 11), ("a", 24), ("b", 37)] and (mixed.S, mixed.R, mixed.T) == (3, 1, 1)
    assert mixed.frames.tolist() == [[2, 0, 11, 40], [0, 0, 24, -1], [1, 0, 37, -1]] and mixed.resampled == [2]


def test_a_tracking_stream_waits_for_both_frames_and_keeps_its_ring():
    """hop 4, win 16, L = 69: the mel needs 4 t + 8 samples, the F0 frame 4 t + 35 -- the later one decides, and both hand out
    the same frames."""
    an = live.StreamingAnalyzer(TINY, ring_samples=16)
    assert an.ring_samples == 16
    an.open("v", f0_params=prm_of(64, 2, 5))
    assert an.ring_samples == 128 and an.streams["v"].f0_len == 69      # the ring store starts at or above L
    an.open("w")
    for have, want_v, want_w in ((34, 0, 7), (35, 1, 7), (38, 1, 8), (39, 2, 8)):
        for sid in "vw":
            st = an.streams[sid]
            st.have = st.in_have = have
            st.queue = [samples(have)]
        plan = an.plan()
        assert plan.rows == [("v", want_v), ("w", want_w)] and plan.T == 1, have
        assert want_v == min(live_plan.frames_ready(have, 4, 16), live_plan.f0_frames_ready(have, 4, 69))
    # 39 samples, none handed out: everything is kept.  After 2 frames the next F0 frame starts at 2 * 4 - 34 < 0; after 20
    # frames at 20 * 4 - max(16 // 2 + 2, 69 // 2) = 46, where the mel window alone would keep from 70 on
    st = an.streams["v"]
    assert an.plan().ring_needed == 39
    st.emitted, st.have = 20, 200
    an.streams["w"].emitted, an.streams["w"].have = 20, 100
    assert an.plan().ring_needed == 200 - 46
    st.f0_len = None
    assert an.plan().ring_needed == 200 - 70
    # a closed stream hands out all its frames, whatever the tracker's reach
    an = live.StreamingAnalyzer(TINY)
    an.open("v", f0_params=prm_of(64, 2, 5))
    an.push("v", samples(9), last=True)
    assert an.plan().rows == [("v", 3)] and an.plan().frames.tolist() == [[0, 0, 3, 9]]


def test_open_refuses_what_a_stream_cannot_track():
    an = live.StreamingAnalyzer(TINY)
    with pytest.raises(ValueError, match="model-rate"):
        an.open("x", f0_params=dict(prm_of(64, 2, 5), sample_rate=16000))
    with pytest.raises(ValueError, match="window"):
        an.open("x", f0_params=prm_of(96, 2, 5))
    with pytest.raises(ValueError, match="whole sound"):
        an.open("x", f0_params=prm_of(64, 2, 5), f0_decode={"w_jump": 4.0})
    an.open("x", f0_params=prm_of(64, 2, 5))
    with pytest.raises(ValueError, match="share one set"):
        an.open("y", f0_params=prm_of(64, 2, 7))
    assert list(an.streams) == ["x"] and an.tick() == {} and an.last_f0 == {} and an.device is None
    lr = object.__new__(live.LiveResynthesizer)
    lr.analyzer = an
    with pytest.raises(ValueError, match="whole sound"):
        lr.open("z", f0_source="audio", f0_decode={"w_jump": 4.0})
    with pytest.raises(ValueError, match="f0_source"):
        lr.open("z", f0_source="file")
    with pytest.raises(ValueError, match="f0_initial"):
        lr.open("z", f0_source="audio", f0_initial=0.0)


def test_fill_hold():
    hold = f0track.fill_hold
    v = np.asarray([101.25, 0.1 + 200, 333.3], dtype=np.float32)
    cases = [([0, 0, v[0], 0, 0, v[1], v[2], 0], [150, 150, v[0], v[0], v[0], v[1], v[2], v[2]]),    # leading, gap, trailing
             ([0, 0, 0], [150, 150, 150]), (v, v), ([], []), ([v[0]], [v[0]]), ([0], [150])]
    for f0, want in cases:
        got = hold(np.asarray(f0, dtype=np.float32), 150.0)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (len(f0),)
        assert np.array_equal(bits(got), bits(np.asarray(want, dtype=np.float32))), f0
    assert bits(hold([0.0], 0.1))[0] == bits(np.float32(0.1))[0]         # float32(initial)
    assert np.array_equal(hold(np.asarray([0, 7], dtype=np.int64)), np.asarray([150, 7], dtype=np.float32))
    for bad in ([np.nan], [1.0, -1.0], [np.inf], [[1.0, 2.0]]):
        with pytest.raises(ValueError, match="fill_hold"):
            hold(np.asarray(bad, dtype=np.float32), 150.0)
    for bad in (0.0, -1.0, np.nan, np.inf, None, "x", [1.0, 2.0], 1e39):
        with pytest.raises(ValueError, match="initial"):
            hold(np.zeros(2, np.float32), bad)
    # chunk by chunk with the carried state: every cut of a 12-frame contour, and every pair of cuts
    contour = np.asarray([0, 0, 110.5, 0, 112.25, 0, 0, 0, 220.125, 221, 0, 0], dtype=np.float32)
    whole = hold(contour, 97.0)
    assert np.count_nonzero(whole == np.float32(97.0)) == 2
    for a in range(13):
        for b in range(a, 13):
            state, parts = np.float32(97.0), []
            for chunk in (contour[:a], contour[a:b], contour[b:], contour[:0]):
                parts.append(hold(chunk, state))
                state = parts[-1][-1] if parts[-1].size else state
            assert np.array_equal(bits(np.concatenate(parts)), bits(whole)), (a, b)
    # the two fills agree where there is nothing to fill, and "hold" needs the tracked contour
    assert np.array_equal(f0track.fill_tracked(v, "hold"), f0track.fill_tracked(v, "interpolate"))
    assert f0track.fill_tracked(np.zeros(3, np.float32)) is None
    assert np.array_equal(f0track.fill_tracked(np.zeros(3, np.float32), "hold", 99.0), np.full(3, 99.0, np.float32))
    f0track.check_fill("hold", "audio", "x")
    f0track.check_fill("interpolate", "net", "x")
    for fill, source in (("hold", "net"), ("linear", "audio")):
        with pytest.raises(ValueError, match="f0_fill"):
            f0track.check_fill(fill, source, "x")


def test_lookahead_ms_for_follows_its_formula():
    lr = object.__new__(live.LiveResynthesizer)
    lr.synthesizer = types.SimpleNamespace(lookahead_ms=12.5)
    # the defaults at 24 kHz on the model's grid (win 1200, hop 300): 3 frames instead of 2
    lr.analyzer = live.StreamingAnalyzer(dict(TINY, hop_size=300, win_size=1200, fft_size=2048))
    base = lr.lookahead_ms
    assert base == 1000.0 * 2 * 300 / 24000 + 12.5
    assert lr.lookahead_ms_for() == lr.lookahead_ms_for(f0_source="net") == base
    assert lr.lookahead_ms_for(f0_source="audio") == 1000.0 * 3 * 300 / 24000 + 12.5
    assert lr.lookahead_ms_for(f0_source="audio", f0_params=f0track.params(24000)) == lr.lookahead_ms_for(f0_source="audio")
    for prm in (prm_of(64, 2, 5), prm_of(2048, 24, 2047), prm_of(1024, 24, 437)):
        L = prm["window"] + prm["tau_max"]
        frames = -(-max(1200 - 600, L - L // 2) // 300)
        assert lr.lookahead_ms_for(f0_source="audio", f0_params=prm) == 1000.0 * frames * 300 / 24000 + 12.5, prm
        both = lr.lookahead_ms_for(44100, 48000, f0_source="audio", f0_params=prm)
        assert abs(both - (lr.lookahead_ms_for(44100, 48000) + 1000.0 * (frames - 2) * 300 / 24000)) < 1e-9
    with pytest.raises(ValueError, match="f0_source"):
        lr.lookahead_ms_for(f0_source="file")


def test_the_header_and_its_binding():
    from mbexwn_vocoder_amd.build import HEADERS, SOURCES
    assert "mbexwn_live_pitch.h" in c_headers.header_names() and abi.symbols("mbexwn_live_pitch.h") == ["mbxt_f0_frames"]
    assert any(hh.endswith("mbexwn_live_pitch.h") for hh in HEADERS) and "f0_stream.hip" in SOURCES and "f0_frame.h" in HEADERS
    text = open(os.path.join(ROOT, "include", "mbexwn_live_pitch.h")).read()
    assert "THE PROMISE" in text and "MBX_ERR_INVALID_ARGUMENT" in text
    # the pinned export lists of the older headers did not move
    assert abi.symbols("mbexwn_live.h") == ["mbxl_ring_append", "mbxl_mel_frames"] and abi.symbols("mbexwn_pitch.h") == ["mbxp_track_f0"]
    assert abi.MBX_ABI_VERSION == 11


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "mbexwn_live_pitch.h"\nint main(void){ (void)mbxt_f0_frames; return 0; }\n')
    res = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", c_headers.INCLUDE, "-c", str(src), "-o", str(tmp_path / "use.o")],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

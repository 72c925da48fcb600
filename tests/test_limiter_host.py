"""The look-ahead limiter's definition on the host (mbexwn_vocoder_amd/limiter.py): the window and
the weights, the ceiling and its bound, the shape of the gain around a peak, NaN and inf, the stream restatement against the
whole item, and the options of ``level.check_options``."""
import numpy as np
import pytest

from mbexwn_vocoder_amd import level, limiter

CEILING = np.float32(10.0 ** (-1.0 / 20.0))
RATES = {8000: (6, 160), 24000: (18, 480), 44100: (33, 882), 48000: (36, 960)}


def noisy(n, rate, seed):
    """A 110 Hz tone with slow amplitude modulation plus noise, peak about 0.8."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    x = 0.6 * np.sin(2 * np.pi * 110.0 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 1.3 * t)) + 0.05 * rng.standard_normal(n)
    return x.astype(np.float32)


@pytest.mark.parametrize("rate", sorted(RATES))
def test_window_and_weights(rate):
    h, H = limiter.window(rate)
    assert (h, H) == RATES[rate]
    w = limiter.weights(h)
    assert w.dtype == np.float32 and w.shape == (2 * h + 1,)
    assert np.all(w > 0) and np.array_equal(w, w[::-1])
    assert abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6
    want = np.sin(np.pi * (np.arange(2 * h + 1) + 1.0) / (2 * h + 2)) ** 2
    assert np.allclose(w, want / want.sum(), rtol=1e-6, atol=0)


def test_window_edges():
    assert limiter.window(100, 1.5, 20.0) == (1, 2)                      # h is at least 1
    assert limiter.window(48000, 5.0, 50.0) == (120, 2400)
    with pytest.raises(ValueError, match="hold"):
        limiter.window(24000, 10.0, 2.0)                                 # H = 48 < h = 120
    for bad in ((0, 1.5, 20.0), (24000, 0.0, 20.0), (24000, 1.5, float("nan")), (24000, -1.0, 20.0)):
        with pytest.raises(ValueError):
            limiter.window(*bad)
    limiter.check_window(36, 2400)
    with pytest.raises(ValueError, match="too long"):
        limiter.check_window(36, 6000)


def test_a_quiet_item_keeps_its_bits():
    h, H = limiter.window(24000)
    x = noisy(5000, 24000, 1)
    g0 = np.float32(0.9)
    assert np.max(np.abs(x * g0)) <= CEILING
    y, stats = limiter.limit_host(x, g0, CEILING, h, H)
    assert np.array_equal(y.view(np.uint32), (x * g0).view(np.uint32))
    assert stats == limiter.LimitStats(np.float32(1.0), 0, 0) and stats.reduction_db == 0.0
    assert list(stats.words()) == [limiter.ONE_BITS, 0, 0, 0]
    y, stats = limiter.limit_host(np.zeros(0, dtype=np.float32), g0, CEILING, h, H)
    assert y.size == 0 and stats.limited == 0


@pytest.mark.parametrize("g0", [2.0, 4.0])
@pytest.mark.parametrize("rate", [8000, 24000])
def test_noisy_items_stay_under_the_ceiling(rate, g0):
    h, H = limiter.window(rate)
    x = noisy(2 * rate, rate, 7)
    y, stats, u, need, g = limiter.limit_host(x, g0, CEILING, h, H, details=True)
    assert np.max(np.abs(y)) <= CEILING
    with np.errstate(over="ignore"):
        raw = np.abs(u * g)
    bound = np.float32((2 * h + 4) * 2.0 ** -24) * CEILING
    assert float(np.max(raw)) - float(CEILING) <= float(bound)
    assert stats.clamped == int(np.count_nonzero(raw > CEILING)) < x.size // 100
    assert stats.limited == int(np.count_nonzero(g < 1)) > 0 and stats.min_gain == g.min() < 1
    # g is exactly 1 wherever the window [i - h - H, i + 2 h] holds no over
    over = np.concatenate((np.zeros(h + H, bool), need < 1, np.zeros(2 * h, bool)))
    hit = np.convolve(over.astype(np.int64), np.ones(3 * h + H + 1, dtype=np.int64), mode="valid") > 0
    assert hit.size == x.size and np.any(~hit) and np.all(g[~hit] == 1.0)
    assert np.array_equal(y[~hit].view(np.uint32), u[~hit].view(np.uint32))
    assert np.all(g <= 1.0) and np.all(g > 0)


def test_the_gain_around_an_isolated_impulse():
    h, H = limiter.window(24000)
    n, p = 3000, 1200
    x = np.zeros(n, dtype=np.float32)
    x[p] = 3.0
    y, stats, u, need, g = limiter.limit_host(x, 1.0, CEILING, h, H, details=True)
    outside = np.ones(n, bool)
    outside[p - 2 * h:p + H + h + 1] = False
    assert np.all(g[outside] == 1.0)
    assert g[p - 2 * h] < 1.0 and g[p + H + h] < 1.0                     # the stated support is tight
    assert np.all(np.diff(g[p - 2 * h - 1:p + 1]) <= 0)                  # attack
    hold = g[p:p + H - h + 1]
    assert np.all(hold.view(np.uint32) == hold.view(np.uint32)[0])
    assert abs(float(hold[0]) - float(need[p])) <= (2 * h + 4) * 2.0 ** -24
    assert np.all(np.diff(g[p + H - h:p + H + h + 2]) >= 0)              # release
    assert abs(float(y[p])) <= CEILING and stats.limited == 3 * h + H + 1


def test_equal_peaks_within_the_hold_see_one_gain():
    h, H = limiter.window(24000)
    period = 240                                                         # 100 Hz, below H = 480
    x = np.zeros(6000, dtype=np.float32)
    peaks = np.arange(1000, 4000, period)
    x[peaks] = 2.5
    _, _, _, _, g = limiter.limit_host(x, 1.0, CEILING, h, H, details=True)
    between = g[peaks[0]:peaks[-1] + 1]
    assert between[0] < 1 and np.all(between.view(np.uint32) == between.view(np.uint32)[0])


def test_nan_and_inf_samples():
    h, H = limiter.window(8000)
    x = noisy(4000, 8000, 3) * np.float32(0.5)
    clean = x.copy()
    x[500], x[1500], x[2500] = np.nan, np.inf, -np.inf
    y, stats = limiter.limit_host(x, 1.0, CEILING, h, H)
    assert np.isnan(y[500]) and y[1500] == CEILING and y[2500] == -CEILING
    rest = np.ones(x.size, bool)
    rest[[500, 1500, 2500]] = False
    assert np.array_equal(y[rest].view(np.uint32), clean[rest].view(np.uint32))
    assert (stats.limited, stats.clamped, float(stats.min_gain)) == (0, 2, 1.0)


def test_true_peak_needs_take_the_neighbouring_outputs():
    u = np.asarray([0.1, 0.2, 0.3, 0.2], dtype=np.float32)
    v = np.zeros(16, dtype=np.float32)
    v[7], v[15] = -2.0, 4.0                                              # q = 7 is seen by k = 1 and k = 2, q = 15 by k = 3
    need = limiter.needs_host(u, 1.0, v)
    assert list(need) == [1.0, 0.5, 0.5, 0.25]
    v[0] = np.nan                                                        # a NaN is no finite peak: no need from it
    assert limiter.needs_host(u, 1.0, v)[0] == 1.0
    with pytest.raises(ValueError, match="4 n"):
        limiter.needs_host(u, 1.0, v[:15])


@pytest.mark.parametrize("rate,n", [(8000, 3000), (24000, 5000), (8000, 5), (8000, 0)])
def test_a_stream_in_random_cuts_equals_the_whole_item(rate, n):
    h, H = limiter.window(rate)
    rng = np.random.default_rng(rate + n)
    x = noisy(n, rate, 11)
    if n > 100:
        x[0], x[-1] = 2.0, -2.0
    whole, stats = limiter.limit_host(x, 2.0, CEILING, h, H)
    for trial in range(4):
        stream = limiter.StreamLimiterHost(2.0, CEILING, h, H)
        cuts = np.sort(rng.integers(0, n + 1, size=rng.integers(0, 12)))
        parts, at = [], 0
        for cut in list(cuts) + [n]:
            parts.append(stream.push(x[at:cut], last=False))
            assert stream.done == limiter.ready_outputs(cut, h) and stream.base == limiter.keep_from(stream.done, h, H)
            at = cut
        parts.append(stream.push(x[n:], last=True))
        got = np.concatenate(parts)
        assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))
        assert stream.stats == stats and stream.done == n


def test_readiness_and_keep_from_at_their_edges():
    h, H = 6, 160
    assert limiter.ready_outputs(0, h) == limiter.ready_outputs(2 * h, h) == 0
    assert limiter.ready_outputs(2 * h + 1, h) == 1                      # output i needs i + 2 h + 1 samples
    assert limiter.ready_outputs(5, h, final=5) == 5 and limiter.ready_outputs(5, h, final=-1) == 0
    assert limiter.keep_from(0, h, H) == limiter.keep_from(h + H, h, H) == 0
    assert limiter.keep_from(h + H + 1, h, H) == 1
    row = limiter.emit_row(3, 10, 20, None, 40, np.float32(2.0))
    assert row == [3, 10, 20, -1, 40, 0x40000000] and limiter.emit_row(0, 0, 1, 7, 0, 1.0)[3] == 7


def test_option_errors():
    assert level.check_options(-16.0, None, False) == (-16.0, level.DEFAULT_PEAK_LIMIT, False)     # as before
    assert level.check_options(None, None, False, limiter=True) == (None, level.DEFAULT_PEAK_LIMIT, False)
    assert level.check_options(-16.0, -3.0, True, limiter=True, lookahead_ms=5.0, hold_ms=50.0) == (-16.0, -3.0, True)
    for kwargs in ({"lookahead_ms": 3.0}, {"hold_ms": 10.0}, {"lookahead_ms": 1.5}, {"hold_ms": 20.0}):      # the defaults too
        with pytest.raises(ValueError, match="limiter"):
            level.check_options(-16.0, None, False, **kwargs)
    for kwargs in ({"lookahead_ms": 0.0}, {"hold_ms": float("inf")}, {"lookahead_ms": "x"}):
        with pytest.raises(ValueError):
            level.check_options(-16.0, None, False, limiter=True, **kwargs)
    control = level.level_control(limiter=True)
    assert control.limiter and control.peak_limit == level.DEFAULT_PEAK_LIMIT and control.target is None
    assert (control.lookahead_ms, control.hold_ms) == (None, None) and control.window(24000) == (18, 480)
    with pytest.raises(ValueError, match="limiter"):
        level.level_control(-16.0, hold_ms=20.0)
    with pytest.raises(ValueError, match="limiter"):
        level.LevelControl(-16.0, lookahead_ms=1.5)
    # the rates of a job, before anything runs: a hold under half the look-ahead, a window too long for the device
    level.level_control(-16.0).check_rates([24000])
    level.level_control(limiter=True, hold_ms=50.0).check_rates([8000, 24000, 48000])
    with pytest.raises(ValueError, match="too long"):
        level.level_control(limiter=True, hold_ms=125.0).check_rates([24000, 48000])
    with pytest.raises(ValueError, match="hold"):
        level.level_control(limiter=True, lookahead_ms=50.0).check_rates([24000])
    assert limiter.workspace_floats(2 * 2048 + 1, 3, 18, 480) == 3 * 3 * 534
    assert limiter.workspace_floats(2048, 1, 18, 480, 180) == 534 + 2 * 47
    assert level.level_control() is None and not level.level_control(-16.0).limiter
    with pytest.raises(ValueError, match="hold"):
        level.level_control(limiter=True, lookahead_ms=10.0, hold_ms=2.0).window(24000)


def test_the_streaming_plan_is_host_logic_alone():
    from mbexwn_vocoder_amd.live_plan import LimiterPlan, _DStream
    a = _DStream(0, 24000, 18, 480, np.float32(2.0), 0.89)
    b = _DStream(1, 8000, 6, 160, np.float32(1.0), 0.89)
    streams = {"a": a, "b": b}
    assert LimiterPlan(streams).rows == [] and LimiterPlan(streams).groups == []
    a.have, a.queue = 100, [(None, 0, 100)]
    plan = LimiterPlan(streams)
    assert plan.rows == [("a", 0, 100 - 36, -1)] and plan.ring_needed == 100
    assert plan.groups == [((18, 480, 0.89), 0, 1, 64)]
    b.have, b.queue, b.closed = 5, [(None, 0, 5)], True                  # shorter than 2 h and closed: every output is final
    plan = LimiterPlan(streams)
    assert plan.rows == [("b", 0, 5, 5), ("a", 0, 64, -1)]               # by window: one launch per group
    assert [gg[1:] for gg in plan.groups] == [(0, 1, 5), (1, 2, 64)]
    assert (a.emitted, a.on_device, b.emitted) == (0, 0, 0)              # planning changed nothing
    a.emitted, a.on_device, a.queue, a.have = 64, 100, [(None, 0, 2000)], 2100
    plan = LimiterPlan({"a": a})
    assert plan.rows == [("a", 64, 2000, -1)] and plan.ring_needed == 2100    # output 64 still reads sample 0: 64 - 18 - 480 < 0
    a.emitted = 600
    assert LimiterPlan({"a": a}).ring_needed == 2100 - min(600 - 498, 100)


def test_the_file_tools_refuse_a_window_before_a_model_is_loaded(tmp_path):
    """A window the written rate refuses is one error line of the tool, from the model's configuration alone."""
    import os
    import subprocess
    import sys
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mbexwn_vocoder_amd", "bin")
    model = create_synthetic_model_dir(str(tmp_path / "speech_small"), "SPEECH", **{"mbexwn_config:pp_mod_subnet:n_channels": 32,
                                                                                      "mbexwn_config:pp_mod_subnet:n_layers": 5})
    for tool, args, word in (("transform_audio.py", ["x.wav", "-o", str(tmp_path), "--model_id", model, "--limiter-hold", "300"], "too long"),
                             ("resynth_mel.py", [model, "-i", "x.mell", "-o", str(tmp_path), "--limiter-lookahead", "50"], "hold"),
                             ("transform_audio.py", ["x.wav", "-o", str(tmp_path), "--model_id", model, "--out-rate", "48000",
                                                     "--limiter-hold", "125"], "too long")):
        res = subprocess.run([sys.executable, os.path.join(tools, tool), *args, "--limiter"], capture_output=True, text=True,
                             timeout=120)
        assert res.returncode == 1 and f"{tool[:-3]}::error:: limiter:" in res.stderr and word in res.stderr, res.stderr[-2000:]
        assert "Traceback" not in res.stderr


def test_a_worked_tick_packs_the_descriptor_words_of_the_headers():
    """Four streams, one tick, every word by hand from the row layouts of mbexwn_live.h (append: slot, abs_start, count,
    offset) and mbexwn_limiter.h (emit: slot, first_out, n_new, n_total or -1, out_offset, the bits of g0).  Output i is
    final once sample i + 2 h is there: h = 18 at 24 kHz, 6 at 8 kHz."""
    import math
    import torch
    from mbexwn_vocoder_amd import live
    one, two = torch.zeros(1200, dtype=torch.float32), torch.zeros(64, dtype=torch.float32)
    stage = live.StreamingLimiter()
    double = 20.0 * math.log10(2.0)                      # 10 ** (double / 20) rounds to the float32 2.0
    for sid, rate, gain_db in (("a", 24000, double), ("b", 8000, 0.0), ("c", 24000, -double), ("d", 24000, 0.0)):    # slots 0 .. 3
        stage.open(sid, rate, gain_db=gain_db)
    ceiling = float(np.float32(10.0 ** (-1.0 / 20.0)))
    wide, narrow = (18, 480, ceiling), (6, 160, ceiling)
    assert [st.key for st in stage.streams.values()] == [wide, narrow, wide, wide]
    stage.push("a", one, 0, 100)                         # an earlier tick: outputs 0 .. 63
    first = stage.plan()
    assert first.rows == [("a", 0, 64, -1)] and first.starts == [0, 64]
    stage.commit(first)
    stage.push("a", one, 100, 500)                       # two pushes from one tensor: two turns
    stage.push("a", one, 600, 400)                       # ... 1000 samples: outputs 64 .. 963
    stage.push("b", two, 5, 50)                          # a second tensor, another window: 50 - 12 = 38 outputs
    stage.push("c", one, 1000, 20, last=True)            # closed at 20 samples: every output
    stage.push("d", one, 1100, 30)                       # 30 <= 2 h: appended, nothing final
    plan = stage.plan()
    assert plan.rows == [("b", 0, 38, -1), ("a", 64, 900, -1), ("c", 0, 20, 20), ("d", 0, 0, -1)]       # by window, stable
    assert plan.groups == [((6, 160, ceiling), 0, 1, 38), ((18, 480, ceiling), 1, 4, 900)]
    assert plan.starts == [0, 38, 938, 958, 958] and plan.ring_needed == 1000    # output 64 still reads sample 0: 64 - 18 - 480 < 0
    # one call per (turn, tensor), no slot twice in a call: the second tensor, the first turn of the first, its second turn
    assert plan.calls == {(0, two.data_ptr(), 64): [(1, 0, 50, 5)],
                          (0, one.data_ptr(), 1200): [(0, 100, 500, 100), (2, 0, 20, 1000), (3, 0, 30, 1100)],
                          (1, one.data_ptr(), 1200): [(0, 600, 400, 600)]}
    assert list(plan.calls) == [(0, two.data_ptr(), 64), (0, one.data_ptr(), 1200), (1, one.data_ptr(), 1200)]
    assert (plan.n_app, plan.words) == (5, 4 * 5 + 6 * 4)
    desc = np.full(48, -7, dtype=np.int64)
    plan.pack(desc, stage._word5)
    assert desc.tolist() == [1, 0, 50, 5,
                             0, 100, 500, 100, 2, 0, 20, 1000, 3, 0, 30, 1100,
                             0, 600, 400, 600,
                             1, 0, 38, -1, 0, 0x3F800000,
                             0, 64, 900, -1, 38, 0x40000000,
                             2, 0, 20, 20, 938, 0x3F000000,
                             3, 0, 0, -1, 958, 0x3F800000,
                             -7, -7, -7, -7]
    stage.commit(plan)
    assert [(st.emitted, st.on_device, st.queue) for st in stage.streams.values()] == [(964, 1000, []), (38, 50, []), (20, 20, []),
                                                                                      (0, 30, [])]
    assert stage.finished("c") and not stage.finished("a") and stage.plan().rows == []
    assert stage.rings is None and stage.device_allocations == 0                 # planning and packing touch no device

"""The look-ahead limiter on the GPU (csrc/limiter.hip) against its definition,
mbexwn_vocoder_amd/limiter.py, bit for bit, statistics included: every length around the window and the tile, every window
shape, the guard bands, batch invariance, the true-peak variant against the project's own resampler, the ring variant
against the whole item, and the option of synth_from_mels and of the file tools on the small test model."""
import ctypes

import numpy as np
import pytest

from guarded import GuardSet

pytestmark = pytest.mark.gpu
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 5}
SEED = 11
CEILING = np.float32(10.0 ** (-1.0 / 20.0))
T = 2048


def bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float32).view(np.int32)


def item(seed, n, scale=0.4):
    """Noise with a slow envelope: stretches under the ceiling (the fast path) and stretches over it."""
    rng = np.random.default_rng(seed)
    env = 0.25 + 0.75 * (np.sin(2 * np.pi * np.arange(n) / 1500.0 + seed) > 0.3)
    return (scale * env * rng.standard_normal(n)).astype(np.float32)


def stage(items, pad=37):
    import torch
    counts = [int(xx.size) for xx in items]
    host = np.full((len(items), max(counts) + pad), np.nan, dtype=np.float32)
    for bb, xx in enumerate(items):
        host[bb, :counts[bb]] = xx
    return torch.as_tensor(host).cuda(), counts


def run(items, gains, h, H, ceiling=CEILING, **kwargs):
    """(outputs per item, stats words per item, the whole output batch) of limit_device."""
    import torch
    from mbexwn_vocoder_amd import limiter
    audio, counts = stage(items)
    out = torch.full_like(audio, 77.0)
    g0 = torch.as_tensor(np.asarray(gains, dtype=np.float32)).cuda()
    got, stats = limiter.limit_device(audio, counts, g0, ceiling, h, H, out=out, **kwargs)
    assert got.data_ptr() == out.data_ptr()
    host, words = out.cpu().numpy(), stats.cpu().numpy()
    for bb, nn in enumerate(counts):
        assert np.all(host[bb, nn:] == 77.0), bb                       # nothing behind an item's end is written
    return [host[bb, :nn] for bb, nn in enumerate(counts)], words, host


def assert_definition(items, gains, h, H, outs, words, ceiling=CEILING, vs=None):
    from mbexwn_vocoder_amd import limiter
    for bb, xx in enumerate(items):
        want, stats = limiter.limit_host(xx, gains[bb], ceiling, h, H, v=None if vs is None else vs[bb])
        assert np.array_equal(bits(outs[bb]), bits(want)), (bb, xx.size)
        assert list(words[bb]) == list(stats.words()), (bb, xx.size, words[bb], stats)


def test_every_length_around_the_window_and_the_tile():
    """One mixed batch at 24 kHz (h = 18, H = 480, W = 499) with NaN behind every item's end: the lengths of the issue, an
    over at the first and at the last index, a run of overs longer than W, a gain per item, and 37 items (the lengths travel
    in the kernel arguments 32 at a time)."""
    from mbexwn_vocoder_amd import limiter
    h, H = limiter.window(24000)
    W = H + h + 1
    lengths = [0, 1, h, 2 * h + 1, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T + 13]
    items = [item(ii, nn) for ii, nn in enumerate(lengths)]
    for xx in items[1:]:
        xx[0], xx[-1] = 1.5, -1.25                                      # over at the first and at the last index
    items[-1][T - 300:T + 300] = 2.0 + 0.3 * np.sin(np.arange(600))     # a run of overs longer than W, across a tile edge
    items[-2][700:1100] = 0.01                                          # and a quiet stretch
    order = [bb % len(items) for bb in range(37)]
    batch = [items[kk] for kk in order]
    gains = [np.float32(0.7 + 0.05 * bb) for bb in range(37)]
    outs, words, _ = run(batch, gains, h, H)
    assert_definition(batch, gains, h, H, outs, words)
    assert all(np.max(np.abs(oo)) <= CEILING for oo in outs if oo.size)
    assert words[10][1] > W and words[0].tolist() == [limiter.ONE_BITS, 0, 0, 0]
    # an item alone equals the same item inside the batch
    alone, alone_words, _ = run([batch[21]], [gains[21]], h, H)
    assert np.array_equal(bits(alone[0]), bits(outs[21])) and np.array_equal(alone_words[0], words[21])
    # an item under the ceiling keeps the bits of x * g0
    quiet = item(50, T + 77, scale=0.05)
    outs, words, _ = run([quiet], [np.float32(1.7)], h, H)
    assert np.array_equal(bits(outs[0]), bits(quiet * np.float32(1.7))) and words[0].tolist() == [limiter.ONE_BITS, 0, 0, 0]


@pytest.mark.parametrize("rate,lookahead,hold", [(8000, 1.5, 20.0), (48000, 1.5, 50.0), (24000, 5.0, 20.0)])
def test_window_shapes(rate, lookahead, hold):
    """h = 6 at 8 kHz; a window of 2437 samples, longer than a tile, at 48 kHz with a 50 ms hold; h = 60 with a 5 ms
    look-ahead.  NaN, inf and huge samples inside the items."""
    from mbexwn_vocoder_amd import limiter
    h, H = limiter.window(rate, lookahead, hold)
    assert (h, H) == {8000: (6, 160), 48000: (36, 2400), 24000: (60, 480)}[rate]
    items = [item(60 + ii, nn) for ii, nn in enumerate((3 * T + 5, H + h, T, 5 * T + 1))]
    items[0][100], items[0][T + 9], items[0][2 * T - 1] = np.nan, np.inf, -np.inf
    items[0][2 * T + 500] = 1e38                                        # a need of 9e-39: a subnormal quotient
    items[0][2 * T + 900] = -3e38
    items[3][:] *= 0.01
    items[3][4 * T + 3] = 5.0                                           # one peak in a long quiet item: four tiles skip
    gains = [np.float32(gg) for gg in (1.0, 2.0, 4.0, 1.0)]
    outs, words, _ = run(items, gains, h, H)
    assert_definition(items, gains, h, H, outs, words)
    assert np.isnan(outs[0][100]) and outs[0][T + 9] == CEILING and outs[0][2 * T - 1] == -CEILING
    peak = 4 * T + 3
    assert words[3][1] == min(items[3].size - 1, peak + H + h) - (peak - 2 * h) + 1


def test_refusals_write_nothing():
    import torch
    from mbexwn_vocoder_amd import limiter
    from mbexwn_vocoder_amd.abi import load_library
    lib = load_library()
    audio, counts = stage([item(1, 500)])
    out = torch.full_like(audio, 77.0)
    stats = torch.full((1, 4), 5, dtype=torch.int32, device="cuda")
    gains = torch.ones(1, device="cuda")
    with pytest.raises(ValueError, match="too long"):
        limiter.limit_device(audio, counts, gains, CEILING, 36, 6000, out=out)
    w = limiter.device_weights(36, audio.device)
    counts_c = (ctypes.c_int64 * 1)(*counts)

    need = lib.mbxd_limit_workspace_floats(int(audio.shape[1]), 1, 36, 960, 0)
    assert need == limiter.workspace_floats(int(audio.shape[1]), 1, 36, 960) == 3 * 36 + 960
    assert lib.mbxd_limit_workspace_floats(100, 1, 0, 960, 0) == lib.mbxd_limit_workspace_floats(100, 1, 40, 39, 0) == 0
    space = torch.full((need,), 3.0, device="cuda")
    pair = torch.full((2 * int(audio.shape[1]),), 77.0, device="cuda")   # rows that overlap without being the same

    def call(ceiling=float(CEILING), h=36, hold=960, src=audio, dst=out, weights=w, n=counts_c, ws_ptr=None, ws_floats=0):
        status = lib.mbxd_limit(src.data_ptr(), int(src.shape[1]), 1, n, gains.data_ptr(), ceiling, h, hold,
                                weights.data_ptr(), None, 0, dst.data_ptr(), int(dst.shape[1]), stats.data_ptr(), ws_ptr, ws_floats,
                                None)
        return status, lib.mbx_last_error().decode()

    for kwargs, word in (({"hold": 6000}, "too long"), ({"h": 0}, "1 <= h <= hold"), ({"h": 40, "hold": 39}, "1 <= h <= hold"),
                         ({"ceiling": 0.0}, "ceiling"), ({"ceiling": float("nan")}, "ceiling"), ({"dst": audio}, "workspace"),
                         ({"dst": audio, "ws_ptr": space.data_ptr(), "ws_floats": need - 1}, "workspace"),
                         ({"dst": audio, "ws_ptr": audio.data_ptr() + 16, "ws_floats": need}, "overlap"),
                         ({"src": pair[:audio.shape[1]].view(1, -1), "dst": pair[8:8 + audio.shape[1]].view(1, -1)}, "overlap"),
                         ({"n": (ctypes.c_int64 * 1)(int(audio.shape[1]) + 1)}, "n_samples")):
        status, message = call(**kwargs)
        assert status == 1 and message.startswith("limit:") and word in message, (kwargs, message)
    torch.cuda.synchronize()
    assert torch.all(out == 77.0) and torch.all(stats == 5) and torch.all(space == 3.0) and torch.all(pair == 77.0)
    assert call()[0] == 0
    rings = torch.zeros((2, 1024), device="cuda")
    desc = torch.zeros((1, 6), dtype=torch.int64, device="cuda")
    for ring, hold in ((rings[:, :1000].contiguous(), 960), (rings, 6000)):
        with pytest.raises(ValueError, match="limit emit:|too long"):
            limiter.limit_emit_device(ring, desc, 1, 10, CEILING, 36, hold, out[0])


@pytest.mark.parametrize("fill", ["nan", "huge"])
def test_the_guard_bands_stay_untouched(fill):
    import torch
    from mbexwn_vocoder_amd import limiter
    from mbexwn_vocoder_amd.abi import _check, load_library
    h, H = limiter.window(8000)
    items = [item(70, 2 * T + 13), item(71, T), item(72, 1), item(73, 0)]
    for xx in items[:3]:
        xx[0], xx[-1] = 2.0, -2.0
    counts = [int(xx.size) for xx in items]
    stride = max(counts)                                                # the longest item ends where the guard begins
    host = np.zeros((len(items), stride), dtype=np.float32)
    for bb, xx in enumerate(items):
        host[bb, :xx.size] = xx
        host[bb, xx.size:] = np.nan
    gains = np.asarray([1.0, 2.0, 0.5, 1.0], dtype=np.float32)
    guards = GuardSet(fill, device="cuda")
    audio = guards.put("audio", host)
    g0 = guards.put("gains", gains)
    out = guards.new("out", host.nbytes)
    stats = guards.new("stats", len(items) * 16)
    w = limiter.device_weights(h, torch.device("cuda", torch.cuda.current_device()))
    _check(load_library().mbxd_limit(audio.ptr, stride, len(items), (ctypes.c_int64 * len(items))(*counts), g0.ptr,
                                     float(CEILING), h, H, w.data_ptr(), None, 0, out.ptr, stride, stats.ptr, None, 0, None))
    torch.cuda.synchronize()
    guards.check()
    got = out.view(torch.float32, len(items), stride).cpu().numpy()
    words = stats.view(torch.int32, len(items), 4).cpu().numpy()
    assert_definition(items, gains, h, H, [got[bb, :nn] for bb, nn in enumerate(counts)], words)
    assert np.array_equal(audio.view(torch.float32, len(items), stride).cpu().numpy().view(np.int32), host.view(np.int32))
    # in place, with a workspace of exactly the stated size between guards of its own
    floats = limiter.workspace_floats(stride, len(items), h, H)
    space = guards.new("workspace", 4 * floats)
    stats.refill()
    _check(load_library().mbxd_limit(audio.ptr, stride, len(items), (ctypes.c_int64 * len(items))(*counts), g0.ptr,
                                     float(CEILING), h, H, w.data_ptr(), None, 0, audio.ptr, stride, stats.ptr, space.ptr, floats,
                                     None))
    torch.cuda.synchronize()
    guards.check()
    here = audio.view(torch.float32, len(items), stride).cpu().numpy()
    for bb, nn in enumerate(counts):
        assert np.array_equal(bits(here[bb, :nn]), bits(got[bb, :nn])), bb
        assert np.all(np.isnan(here[bb, nn:])), bb                       # nothing behind an item's end is written
    assert np.array_equal(stats.view(torch.int32, len(items), 4).cpu().numpy(), words)


@pytest.mark.parametrize("rate,hold,true_peak", [(24000, 20.0, False), (48000, 50.0, False), (8000, 20.0, False),
                                                 (24000, 20.0, True)])
def test_in_place_equals_out_of_place(rate, hold, true_peak):
    """Every tile reads its neighbours' samples from the saved margins: the bits and the statistics of out of place, with a
    window shorter and longer than a tile, items of every length around both, 33 items, and the true-peak variant (whose
    chain reaches beyond the span of needs)."""
    import torch
    from mbexwn_vocoder_amd import limiter
    h, H = limiter.window(rate, 1.5, hold)
    W = H + h + 1
    lengths = [0, 1, h, 2 * h + 1, W - 1, W + 1, T - 1, T, T + 1, 2 * T + 13, 4 * T + 5]
    items = [item(200 + ii, nn) for ii, nn in enumerate(lengths)]
    for xx in items[1:]:
        xx[0], xx[-1] = 1.5, -1.25
    items[-1][2 * T - 300:2 * T + 300] = 2.0                            # a run of overs across a tile edge
    batch = [items[bb % len(items)] for bb in range(33)]
    gains = torch.as_tensor(np.linspace(0.8, 2.4, 33).astype(np.float32)).cuda()
    audio, counts = stage(batch)
    before = audio.clone()
    there, stats_there = limiter.limit_device(audio, counts, gains, CEILING, h, H, rate=rate, true_peak=true_peak)
    assert torch.equal(audio.view(torch.int32), before.view(torch.int32))             # out of place: the input is not touched
    here, stats_here = limiter.limit_device(audio, counts, gains, CEILING, h, H, rate=rate, true_peak=true_peak, out=audio)
    assert here.data_ptr() == audio.data_ptr()
    got, want = here.cpu().numpy(), there.cpu().numpy()
    for bb, nn in enumerate(counts):
        assert np.array_equal(bits(got[bb, :nn]), bits(want[bb, :nn])), (bb, nn)
        assert np.all(np.isnan(got[bb, nn:])), bb
    assert torch.equal(stats_here, stats_there) and int(stats_here[:, 1].sum()) > 0
    with pytest.raises(ValueError, match="workspace"):
        limiter.limit_device(audio, counts, gains, CEILING, h, H, out=audio, workspace=torch.zeros(5, device="cuda"))


def test_true_peak_variant_and_the_trim():
    """The needs from the 4x true peak, against the definition fed with resample_device's output; the static stage behind
    it -- measure with the true peak, a ceiling-only gain -- then holds the ceiling for the oversampled signal."""
    import torch
    from mbexwn_vocoder_amd import level, limiter
    from mbexwn_vocoder_amd.resample import resample_device
    rate = 24000
    h, H = limiter.window(rate)
    sine = (1.2 * np.sin(2 * np.pi * (rate / 4) * np.arange(T + 300) / rate + np.pi / 4)).astype(np.float32)
    items = [sine, item(80, 2 * T + 13, 0.5), item(81, 1), item(82, 0), item(83, 3)]
    gains = [np.float32(gg) for gg in (1.0, 1.5, 3.0, 1.0, 2.0)]
    audio, counts = stage(items)
    g0 = torch.as_tensor(np.asarray(gains)).cuda()
    scaled = audio * g0[:, None]                                        # u: one float32 product
    up, n_up = resample_device(scaled, torch.as_tensor(np.asarray(counts, dtype=np.int32)).cuda(), rate, 4 * rate)
    up = up.cpu().numpy()
    assert n_up.cpu().numpy().tolist() == [4 * nn for nn in counts]
    vs = [up[bb, :4 * nn] for bb, nn in enumerate(counts)]
    out, stats = limiter.limit_device(audio, counts, g0, CEILING, h, H, rate=rate, true_peak=True)
    host = out.cpu().numpy()
    assert_definition(items, gains, h, H, [host[bb, :nn] for bb, nn in enumerate(counts)], stats.cpu().numpy(), vs=vs)
    # the quarter-rate sine is under the ceiling sample by sample and over it between the samples
    assert np.max(np.abs(sine)) < CEILING < np.max(np.abs(vs[0])) and stats.cpu().numpy()[0, 1] > 0
    plain, _ = limiter.limit_device(audio, counts, g0, CEILING, h, H)
    assert np.array_equal(bits(plain.cpu().numpy()[0, :counts[0]]), bits(sine))
    # the trim
    measure = level.measure_device(out, counts, rate, true_peak=True)
    trim = level.gains_device(measure, None, ceiling=limiter.trim_ceiling(CEILING), true_peak=True)
    level.apply_device(out, counts, trim)
    after = level.measure_device(out, counts, rate, true_peak=True).host(details=False)
    assert all(mm.true_peak <= CEILING for mm in after)
    assert np.all(trim.cpu().numpy() <= 1.0) and np.all(trim.cpu().numpy() > 0.0)           # it only ever scales down


def test_streams_from_a_ring_equal_the_whole_item():
    """mbxd_limit_emit over a ring store: two streams of one window group in random cuts, tick by tick, with a gain each --
    one longer than the ring, one shorter than 2 h and closed at once -- and a second group at another window: every output
    and the statistics equal mbxd_limit on the whole item."""
    import torch
    from mbexwn_vocoder_amd import limiter
    rng = np.random.default_rng(5)
    for rate, ring_samples, lengths in ((8000, 2048, (3 * T + 7, 9)), (24000, 4096, (2 * T + 100, 1200))):
        h, H = limiter.window(rate)
        sounds = [item(90 + ii, nn) for ii, nn in enumerate(lengths)]
        for xx in sounds:
            xx[0], xx[-1] = 1.5, -1.5
        gains = [np.float32(1.25), np.float32(2.5)]
        whole, whole_words, _ = run(sounds, gains, h, H)
        rings = torch.full((3, ring_samples), float("nan"), device="cuda")
        stats = limiter.new_stats(3, "cuda")
        slots = [2, 0]
        have, done, got = [0, 0], [0, 0], [[], []]
        most = ring_samples - (3 * h + H)                              # what a tick may add without overwriting a sample still to be read
        while any(dd < xx.size for dd, xx in zip(done, sounds)):
            rows, offset = [], 0
            for ss, xx in enumerate(sounds):
                if done[ss] == xx.size:
                    continue
                room = most - (have[ss] - done[ss])
                add = min(int(rng.integers(0, 900)), room, xx.size - have[ss])
                index = (np.arange(have[ss], have[ss] + add) & (ring_samples - 1))
                rings[slots[ss], torch.as_tensor(index).cuda()] = torch.as_tensor(xx[have[ss]:have[ss] + add]).cuda()
                have[ss] += add
                last = have[ss] == xx.size
                ready = limiter.ready_outputs(have[ss], h, xx.size if last else None)
                assert limiter.keep_from(done[ss], h, H) > have[ss] - ring_samples - 1
                if ready > done[ss]:
                    rows.append((ss, limiter.emit_row(slots[ss], done[ss], ready - done[ss], xx.size if last else None, offset,
                                                      gains[ss])))
                    offset += ready - done[ss]
            if not rows:
                continue
            desc = torch.as_tensor(np.asarray([rr for _, rr in rows], dtype=np.int64)).cuda()
            out = torch.full((offset + 5,), 77.0, device="cuda")
            limiter.limit_emit_device(rings, desc, len(rows), max(rr[2] for _, rr in rows), CEILING, h, H, out, stats)
            host = out.cpu().numpy()
            assert np.all(host[offset:] == 77.0)
            for ss, rr in rows:
                got[ss].append(host[rr[4]:rr[4] + rr[2]])
                done[ss] += rr[2]
        words = stats.cpu().numpy()
        for ss, xx in enumerate(sounds):
            assert np.array_equal(bits(np.concatenate(got[ss])), bits(whole[ss])), (rate, ss)
            assert np.array_equal(words[slots[ss]], whole_words[ss]), (rate, ss)
        assert words[1].tolist() == [limiter.ONE_BITS, 0, 0, 0]          # the slot no row named


# ------------------------------------------------------------------------------------------------------------------------
# the streaming stage alone
# ------------------------------------------------------------------------------------------------------------------------
def offline(sound, rate, gain_db, peak_limit, lookahead_ms=1.5, hold_ms=20.0):
    """(limit_device on the whole sound, its LimitStats) with a stream's options."""
    import torch
    from mbexwn_vocoder_amd import limiter
    h, H = limiter.window(rate, lookahead_ms, hold_ms)
    audio = torch.as_tensor(np.ascontiguousarray(sound, dtype=np.float32)[np.newaxis]).cuda()
    out, stats = limiter.limit_device(audio, [sound.size], float(np.float32(10.0 ** (gain_db / 20.0))),
                                      np.float32(10.0 ** (peak_limit / 20.0)), h, H)
    return out.cpu().numpy()[0], limiter.LimitStats.from_words(stats.cpu().numpy()[0])


def test_streaming_limiter_equals_the_whole_item():
    """Random pushes from one device tensor, two rates (two window groups) in one tick, a stream shorter than 2 h that is
    closed at once, an item longer than the first ring: the streams equal mbxd_limit on the whole items, statistics
    included, and steady ticks allocate nothing on the device."""
    import torch
    from mbexwn_vocoder_amd.live import StreamingLimiter
    rng = np.random.default_rng(17)
    stage_ = StreamingLimiter(ring_samples=1024, slots=2)
    sounds = {"a": item(101, 9000), "b": item(102, 7000), "c": item(103, 10), "d": item(104, 1000)}
    for xx in sounds.values():
        xx[0], xx[-1] = 1.5, -1.5
    options = {"a": (24000, 6.0, -1.0), "b": (8000, 3.0, -3.0), "c": (8000, 3.0, -3.0), "d": (24000, 0.0, -1.0)}
    for sid, (rate, gain_db, peak) in options.items():
        stage_.open(sid, rate, gain_db=gain_db, peak_limit=peak)
    assert stage_.rings is None and stage_.plan().rows == []
    source = torch.as_tensor(np.concatenate([sounds[sid] for sid in "abcd"])).cuda()
    base = dict(zip("abcd", np.cumsum([0] + [sounds[sid].size for sid in "abc"]).tolist()))
    at, got = dict.fromkeys("abcd", 0), {sid: [] for sid in "abcd"}
    stage_.push("c", source, base["c"], 10, last=True)                   # shorter than 2 h = 12 and closed at once
    at["c"] = 10
    allocations = []
    for turn in range(200):
        for sid in "abd":
            left = sounds[sid].size - at[sid]
            if left:
                count = min(left, 700 if 3 <= turn < 9 else int(rng.integers(0, 1500)))
                stage_.push(sid, source, base[sid] + at[sid], count, last=count == left)
                at[sid] += count
        plan = stage_.plan()
        assert stage_.plan().rows == plan.rows                           # planning changes nothing
        for sid, chunk in stage_.tick().items():
            got[sid].append(chunk)
        allocations.append(stage_.device_allocations)
        if all(stage_.finished(sid) for sid in "abcd"):
            break
    assert all(stage_.finished(sid) for sid in "abcd") and stage_.ring_samples > 1024
    assert allocations[4] == allocations[8]                              # equal pushes of 700: steady ticks
    for sid, (rate, gain_db, peak) in options.items():
        want, stats = offline(sounds[sid], rate, gain_db, peak)
        assert np.array_equal(bits(np.concatenate(got[sid])), bits(want)), sid
        assert stage_.stats(sid) == stats, sid
    assert stage_.stats("d").limited > 0
    stage_.close("c")
    stage_.open("e", 8000, peak_limit=-1.0)                              # takes the released slot: its statistics start over
    assert stage_.streams["e"].slot == stage_.streams["d"].slot - 1 and stage_.stats("e").limited == 0
    quiet = torch.full((50,), 0.01, device="cuda")
    stage_.push("e", quiet, 0, 50, last=True)
    out = stage_.tick()["e"]
    assert np.array_equal(bits(out), bits(np.full(50, 0.01, dtype=np.float32))) and stage_.stats("e").limited == 0
    with pytest.raises(ValueError, match="hold"):
        stage_.open("f", 24000, lookahead_ms=50.0, hold_ms=20.0)
    with pytest.raises(ValueError, match="too long"):
        stage_.open("f", 48000, hold_ms=150.0)


# ------------------------------------------------------------------------------------------------------------------------
# the small test model
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    return create_synthetic_model_dir(str(tmp_path_factory.mktemp("model") / "speech_small"), "SPEECH", **SMALL)


@pytest.fixture(scope="module")
def inv(model_dir):
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    return MELInverter(model_dir, conv_form="f23")                       # the forward's kernels are pinned


def voiced(seed, n, rate, f0=150.0):
    rng = np.random.default_rng(seed)
    tt = np.arange(n) / float(rate)
    xx = sum(np.sin(2 * np.pi * f0 * kk * tt) / kk for kk in range(1, 12))
    return (0.2 * xx / np.max(np.abs(xx)) + 0.01 * rng.normal(size=n)).astype(np.float32)


def test_synth_from_mels_with_the_limiter(inv):
    """A loudness the static stage cannot reach under -1 dBFS: the limiter reaches further.  The limited audio is the host
    definition on the same call's unlevelled audio with the reported gain, bit for bit."""
    from mbexwn_vocoder_amd import level, limiter
    from mbexwn_vocoder_amd.analysis import generate_mels
    sounds = [voiced(70, 14400, 24000), voiced(71, 19200, 24000, 210.0)]
    mels = [inv.scale_mel(dd) for dd in generate_mels(sounds, [24000] * 2, inv.preprocess_config, on_device=True)]
    plain = inv.synth_from_mels(mels, noise_seed=SEED, max_batch=2)
    # 3 dB above the loudness at which the static gain would touch the ceiling
    loud = max(level.measure_host(raw, inv.srate).lufs - 20 * np.log10(np.max(np.abs(raw)) / CEILING) for raw in plain) + 3.0
    static, limited = [], []
    base = inv.synth_from_mels(mels, noise_seed=SEED, max_batch=2, loudness=loud, levels_out=static)
    same = inv.synth_from_mels(mels, noise_seed=SEED, max_batch=2, loudness=loud, limiter=False)
    assert all(rep["limited"] and "limiter" not in rep for rep in static)
    assert all(np.array_equal(bits(aa), bits(bb)) for aa, bb in zip(base, same))         # the option absent
    got = inv.synth_from_mels(mels, noise_seed=SEED, max_batch=2, loudness=loud, limiter=True, levels_out=limited)
    h, H = limiter.window(inv.srate)
    for out, raw, rep, before in zip(got, plain, limited, static):
        want, stats = limiter.limit_host(raw, np.float32(rep["gain"]), CEILING, h, H)
        assert np.array_equal(bits(out), bits(want))
        assert np.max(np.abs(out)) <= CEILING and rep["peak_out"] == np.max(np.abs(out))
        assert rep["loudness_out"] > before["loudness_out"] and not rep["limited"]
        assert abs(rep["loudness_out"] - level.measure_host(out, inv.srate).lufs) < 1e-9
        assert abs(rep["loudness_in"] + rep["gain_db"] - loud) < 1e-4                    # the loudness gain stands
        lim = rep["limiter"]
        assert (lim["limited"], lim["clamped"], lim["trim_db"]) == (stats.limited, stats.clamped, 0.0) and stats.limited > 0
        assert lim["reduction_db"] == stats.reduction_db > 0
    # the limiter alone brings the default ceiling; with the true peak the trim holds it for the oversampled signal
    reports = []
    alone = inv.synth_from_mels(mels[:1], noise_seed=SEED, limiter=True, levels_out=reports)
    want, stats = limiter.limit_host(plain[0], 1.0, CEILING, h, H)
    assert np.array_equal(bits(alone[0]), bits(want)) and reports[0]["limiter"]["limited"] == stats.limited
    assert reports[0]["gain"] == 1.0
    reports = []
    out = inv.synth_from_mels(mels[:1], noise_seed=SEED, loudness=loud, limiter=True, true_peak=True, levels_out=reports)
    assert reports[0]["limiter"]["trim_db"] <= 0.0 and reports[0]["peak_out"] <= CEILING
    import torch
    again = level.measure_device(torch.as_tensor(out[0][np.newaxis]).cuda(), [out[0].size], inv.srate, true_peak=True).host()[0]
    assert again.true_peak <= CEILING                                   # the promise, by the device's own meter
    assert level.measure_host(out[0], inv.srate, true_peak=True).true_peak <= CEILING * (1 + 1e-5)   # the host resampler rounds once
    with pytest.raises(ValueError, match="limiter"):
        inv.synth_from_mels(mels[:1], noise_seed=SEED, loudness=loud, hold_ms=30.0)
    with pytest.raises(ValueError, match="hold"):
        inv.synth_from_mels(mels[:1], noise_seed=SEED, limiter=True, lookahead_ms=50.0)


@pytest.mark.parametrize("output_rate", [None, 44100])
def test_live_streams_leave_through_the_limiter(inv, output_rate):
    """gain_db=12, peak_limit=-1: the stream equals the offline limiter on the output of a second stream with the same seed
    and no peak limit, bit for bit; the look-ahead grows by 2 h samples at the rate handed out."""
    from mbexwn_vocoder_amd import limiter
    from mbexwn_vocoder_amd.live import LiveResynthesizer
    live = LiveResynthesizer(inv)
    rate = inv.srate if output_rate is None else output_rate
    rates = {} if output_rate is None else {"output_rate": output_rate}
    h, _ = limiter.window(rate)
    grown = live.lookahead_ms_for(None, output_rate, peak_limit=-1.0) - live.lookahead_ms_for(None, output_rate)
    assert abs(grown - 1000.0 * 2 * h / rate) < 1e-9
    live.open("limited", seed=4, gain_db=12.0, peak_limit=-1.0, **rates)
    live.open("plain", seed=4, **rates)
    with pytest.raises(ValueError, match="peak_limit"):
        live.open("bad", seed=4, gain_db=12.0)
    snd = voiced(75, 12000 + 77, inv.srate)
    got = {"limited": [], "plain": []}
    for start in range(0, snd.size, 1920):
        for sid in got:
            live.push_audio(sid, snd[start:start + 1920], last=start + 1920 >= snd.size, transposition=1.2)
        for sid, chunk in live.tick().items():
            got[sid].append(chunk)
    rounds = 0
    while not (live.finished("limited") and live.finished("plain")):
        for sid, chunk in live.tick().items():
            got[sid].append(chunk)
        rounds += 1
        assert rounds < 1000
    plain = np.concatenate(got["plain"])
    want, stats = offline(plain, rate, 12.0, -1.0)
    audio = np.concatenate(got["limited"])
    assert audio.shape == plain.shape and np.array_equal(bits(audio), bits(want))
    assert np.max(np.abs(audio)) <= CEILING and live.limiter.stats("limited") == stats
    live.close("limited")
    live.close("plain")
    assert not live.limiter.streams


def test_the_tools_write_under_the_ceiling(model_dir, tmp_path):
    import os
    import subprocess
    import sys
    from scipy.io import wavfile
    from mbexwn_vocoder_amd.audioio import read_audio
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mbexwn_vocoder_amd", "bin")
    src = str(tmp_path / "voice.wav")
    wavfile.write(src, 24000, voiced(80, 14400, 24000))
    out = tmp_path / "out"
    res = subprocess.run([sys.executable, os.path.join(tools, "transform_audio.py"), src, "-o", str(out), "--model_id", model_dir,
                          "--loudness", "-16", "--limiter"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "level of " in res.stderr and "limiter: " in res.stderr and "samples limited" in res.stderr
    audio, rate = read_audio(str(out / "syn_voice.flac"))
    assert rate == 24000 and 0.1 < np.max(np.abs(audio)) <= CEILING + 2.0 ** -16         # 16-bit samples, rounded to nearest
    res = subprocess.run([sys.executable, os.path.join(tools, "transform_audio.py"), src, "-o", str(out), "--model_id", model_dir,
                          "--limiter-hold", "30"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 1 and "--limiter" in res.stderr
    # a window the written rate refuses is an error line of the tool, not a traceback, and nothing is written
    late = tmp_path / "late"
    res = subprocess.run([sys.executable, os.path.join(tools, "transform_audio.py"), src, "-o", str(late), "--model_id", model_dir,
                          "--limiter", "--limiter-hold", "300"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 1 and "transform_audio::error:: limiter:" in res.stderr and "too long" in res.stderr
    assert "Traceback" not in res.stderr and not list(late.glob("*.flac"))
    dst = str(tmp_path / "stream.wav")
    res = subprocess.run([sys.executable, os.path.join(tools, "stream_transpose.py"), src, "-o", dst, "--model_id", model_dir,
                          "--gain", "12", "--peak-limit", "-1"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    audio, rate = read_audio(dst)
    assert rate == 24000 and 0 < np.max(np.abs(audio)) <= CEILING

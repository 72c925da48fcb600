"""The level stage on the GPU (csrc/level.hip) against its definition, mbexwn_vocoder_amd/level.py:
hop energies, block powers, gates and the sample peak bit for bit, the true peak against the project's own resampler, the
gains to a float32 ulp, the product and its bounds, batch invariance, and the options of synth_from_mels / transform_audio on
the small test model."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 5}
SEED = 11


def f32_bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float32).view(np.int32)


def f64_bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float64).view(np.int64)


def noise_item(seed, n, scale=0.1, offset=0.05):
    return (scale * np.random.default_rng(seed).standard_normal(n) + offset).astype(np.float32)


def stage(items, pad=37):
    """(cuda batch (B, stride) with NaN behind every item's end, counts): stride longer than the longest item."""
    import torch
    counts = [int(xx.size) for xx in items]
    host = np.full((len(items), max(counts) + pad), np.nan, dtype=np.float32)
    for bb, xx in enumerate(items):
        host[bb, :counts[bb]] = xx
    return torch.as_tensor(host).cuda(), counts


def assert_equals_definition(got, want, what):
    assert np.array_equal(f64_bits(got.energies), f64_bits(want.energies)), what
    assert np.array_equal(f64_bits(got.blocks), f64_bits(want.blocks)), what
    assert f64_bits([got.power])[0] == f64_bits([want.power])[0], (what, got.power, want.power)
    assert (got.count, got.n_abs) == (want.count, want.n_abs), what
    assert f32_bits([got.sample_peak])[0] == f32_bits([want.sample_peak])[0], what
    assert np.isfinite(got.power) and np.isfinite(got.sample_peak), what          # no NaN from behind the item's end


def test_basic_shapes_equal_the_definition_bit_for_bit():
    from mbexwn_vocoder_amd import level
    rate, hop = 24000, 2400
    items = [noise_item(ii, nn) for ii, nn in enumerate((0, 4 * hop - 1, 4 * hop, 7 * hop + 13))]
    audio, counts = stage(items)
    got = level.measure_device(audio, counts, rate).host()
    for bb, xx in enumerate(items):
        assert_equals_definition(got[bb], level.measure_host(xx, rate), bb)
    assert [mm.count for mm in got[:2]] == [0, 0] and got[0].sample_peak == 0 and got[2].blocks.size == 1
    assert got[2].count == 1 and got[3].blocks.size == 4
    # a half-silent item: the gates do something (the second half is 30 dB down)
    xx = noise_item(9, 12 * hop + 5, offset=0.0)
    xx[xx.size // 2:] *= np.float32(10 ** (-30 / 20))
    audio, counts = stage([xx])
    one = level.measure_device(audio, counts, rate).host()[0]
    assert_equals_definition(one, level.measure_host(xx, rate), "gated")
    assert 0 < one.count < one.n_abs == one.blocks.size
    # any two biquads: the kernel leaves out the products by a numerator of (1, b1, 1), as the high-pass has it, and makes
    # them for every other one
    coefs = level.k_weighting(rate)
    coefs[5:8] = [0.75, -1.5, 0.75]
    other = level.measure_device(audio, counts, rate, coefs=coefs[np.newaxis]).host()[0]
    want = level.hop_energies_host(xx, rate, coefs=coefs)
    assert np.array_equal(f64_bits(other.energies), f64_bits(want)) and not np.array_equal(other.energies, one.energies)


def test_mixed_rates_more_than_one_block_and_more_than_one_launch():
    """Per-item coefficient rows and hops (11 025 Hz: the odd hop), an item of more than 64 hops (more than one block of the
    hop kernel), an item of more than 2048 blocks (more than one chunk of the gate kernel), and 33 items (the items travel in
    the kernel arguments 32 at a time)."""
    from mbexwn_vocoder_amd import level
    items = [noise_item(20, 7 * 1103 + 13), noise_item(21, 7 * 4800 + 13), noise_item(22, 66 * 1103 + 5)]
    rates = [11025, 48000, 11025]
    audio, counts = stage(items)
    got = level.measure_device(audio, counts, rates).host()
    for bb, (xx, rr) in enumerate(zip(items, rates)):
        assert_equals_definition(got[bb], level.measure_host(xx, rr), (bb, rr))
    assert got[2].energies.size == 66
    long_item = noise_item(23, 2100 * 800 + 7)
    audio, counts = stage([long_item])
    assert_equals_definition(level.measure_device(audio, counts, 8000).host()[0], level.measure_host(long_item, 8000), "long")
    kinds = [noise_item(24, 4 * 1103), noise_item(25, 5 * 1103 + 1), noise_item(26, 6 * 2400 + 2)]
    rates = [11025, 11025, 24000]
    want = [level.measure_host(xx, rr) for xx, rr in zip(kinds, rates)]
    order = [bb % 3 for bb in range(33)]
    audio, counts = stage([kinds[kk] for kk in order])
    got = level.measure_device(audio, counts, [rates[kk] for kk in order]).host()
    for bb, kk in enumerate(order):
        assert_equals_definition(got[bb], want[kk], bb)
    # ... the gains (the targets travel in the kernel arguments 32 at a time too) ...
    import torch
    measure = level.measure_device(audio, counts, [rates[kk] for kk in order])
    targets = [None if bb % 5 == 0 else level.target_power(-30.0 + bb) for bb in range(33)]
    some = level.gains_device(measure, targets, ceiling=0.3).cpu().numpy()
    for bb, kk in enumerate(order):
        assert one_ulp(some[bb], level.gain_host(want[kk].power, want[kk].count, want[kk].sample_peak, targets[bb], 0.3)[0]), bb
    # ... and the product over the same 33 items
    gains = torch.as_tensor(np.linspace(0.5, 1.5, 33).astype(np.float32)).cuda()
    out = level.apply_device(audio.clone(), counts, gains).cpu().numpy()
    for bb, kk in enumerate(order):
        assert np.array_equal(f32_bits(out[bb, :counts[bb]]), f32_bits(kinds[kk] * gains.cpu().numpy()[bb])), bb
        assert np.all(np.isnan(out[bb, counts[bb]:]))


def test_true_peak_equals_the_resampler():
    """max(sample peak, max |resample_device(audio, n, rate, 4 * rate)|) per item, bit for bit; the quarter-rate sine's true
    peak lies well above its sample peak."""
    import torch
    from mbexwn_vocoder_amd import level
    from mbexwn_vocoder_amd.resample import resample_device
    rate = 24000
    sine = (0.5 * np.sin(2 * np.pi * (rate / 4) * np.arange(5000) / rate + np.pi / 4)).astype(np.float32)
    items = [sine, noise_item(31, 3001, 0.3, 0.0), noise_item(32, 1), noise_item(33, 0), noise_item(34, 1024)]
    audio, counts = stage(items)
    got = level.measure_device(audio, counts, rate, true_peak=True).host()
    up, n_up = resample_device(audio, torch.as_tensor(np.asarray(counts, dtype=np.int32)).cuda(), rate, 4 * rate)
    up, n_up = up.cpu().numpy(), n_up.cpu().numpy()
    for bb, xx in enumerate(items):
        assert n_up[bb] == 4 * counts[bb]
        want = max(int(level.bits_peak(xx).view(np.uint32)), int(level.bits_peak(up[bb, :n_up[bb]]).view(np.uint32)))
        assert int(got[bb].true_peak.view(np.uint32)) == want, bb
        assert f32_bits([got[bb].sample_peak])[0] == f32_bits([level.bits_peak(xx)])[0]
    assert abs(float(got[0].sample_peak) - 0.35355) < 1e-4
    assert 1.35 * float(got[0].sample_peak) <= float(got[0].true_peak) <= 0.5 * 1.01
    # without taps the record's true peak is the sample peak; another rate takes the same taps
    plain = level.measure_device(audio, counts, rate).host()
    assert all(f32_bits([mm.true_peak])[0] == f32_bits([mm.sample_peak])[0] for mm in plain)
    other = level.measure_device(audio, counts, 11025, true_peak=True).host()
    assert all(f32_bits([aa.true_peak])[0] == f32_bits([bb.true_peak])[0] for aa, bb in zip(other, got))


def one_ulp(got, want):
    return abs(int(f32_bits([got])[0]) - int(f32_bits([want])[0])) <= 1


def test_gains_are_the_definitions_to_one_ulp():
    from mbexwn_vocoder_amd import level
    rate, hop = 24000, 2400
    items = [noise_item(40, 6 * hop, 0.1), noise_item(41, 5 * hop + 3, 0.02), noise_item(42, 4 * hop - 1, 0.1),
             noise_item(43, 0), np.zeros(5 * hop, dtype=np.float32)]
    audio, counts = stage(items)
    measure = level.measure_device(audio, counts, rate, true_peak=True)
    host = measure.host()
    other_items = [noise_item(50 + bb, 5 * hop, 0.05 * (bb + 1)) for bb in range(4)] + [noise_item(54, hop)]
    other_audio, other_counts = stage(other_items)
    other = level.measure_device(other_audio, other_counts, rate)
    other_host = other.host()
    assert other_host[4].count == 0 and host[2].count == 0 and host[4].sample_peak == 0
    cases = [(level.target_power(-23.0), None, False), (level.target_power(-23.0), 10.0, False),    # slack ceiling
             (level.target_power(-3.0), level.ceiling_linear(-1.0), False),                          # binding
             (level.target_power(-3.0), level.ceiling_linear(-1.0), True), (None, 0.05, False), (None, 10.0, True)]
    for target, ceiling, true_peak in cases:
        got = level.gains_device(measure, target, ceiling=ceiling, true_peak=true_peak).cpu().numpy()
        for bb, mm in enumerate(host):
            want, limited = level.gain_host(mm.power, mm.count, mm.peak(true_peak), target, ceiling)
            assert one_ulp(got[bb], want), (bb, target, ceiling, got[bb], want)
            if limited:
                assert float(got[bb]) * float(mm.peak(true_peak)) <= ceiling * (1 + 2.0 ** -22)
            if target is None:
                assert got[bb] <= 1.0                            # a ceiling alone never scales up
        assert got[2] <= 1.0 and got[3] == 1.0 and got[4] == 1.0  # not measurable: no loudness gain; no samples, silence: 1
    # per-item targets, and targets taken from other records on the device (a record that is not measurable: no target)
    per_item = [level.target_power(-20.0), None, level.target_power(-30.0), None, level.target_power(-20.0)]
    got = level.gains_device(measure, per_item).cpu().numpy()
    for bb, mm in enumerate(host):
        assert one_ulp(got[bb], level.gain_host(mm.power, mm.count, mm.sample_peak, per_item[bb])[0]), bb
    got = level.gains_device(measure, None, target_records=other, ceiling=2.0).cpu().numpy()
    for bb, (mm, oo) in enumerate(zip(host, other_host)):
        want = level.gain_host(mm.power, mm.count, mm.sample_peak, oo.power if oo.count else None, 2.0)[0]
        assert one_ulp(got[bb], want), bb
    assert got[0] != 1.0 and got[1] != 1.0
    # a NaN item: NaN peak, gain 1
    bad = noise_item(44, 5 * hop)
    bad[100] = np.nan
    audio, counts = stage([bad])
    measure = level.measure_device(audio, counts, rate)
    assert np.isnan(measure.host()[0].sample_peak)
    assert level.gains_device(measure, level.target_power(-23.0), ceiling=0.5).cpu().numpy()[0] == 1.0


def test_apply_is_one_product_and_stays_inside_the_items():
    import torch
    from mbexwn_vocoder_amd import level
    sentinel = np.float32(-123.25)
    counts, stride = [0, 1, 2049, 5000], 5003
    items = [noise_item(60 + bb, nn, 0.3) for bb, nn in enumerate(counts)]
    flat = np.full(len(items) * stride + 64, sentinel, dtype=np.float32)
    for bb, xx in enumerate(items):
        flat[bb * stride:bb * stride + xx.size] = xx
    gains = np.asarray([2.0, 0.3, 1.7, 0.123], dtype=np.float32)
    gains_dev = torch.as_tensor(gains).cuda()
    src = torch.as_tensor(flat).cuda()
    out_stride = stride + 9
    dst = torch.full((len(items) * out_stride + 64,), float(sentinel), dtype=torch.float32).cuda()
    out = level.apply_device(src[:len(items) * stride].view(len(items), stride), counts, gains_dev,
                             out=dst[:len(items) * out_stride].view(len(items), out_stride))
    assert out.data_ptr() == dst.data_ptr()
    assert np.array_equal(src.cpu().numpy(), flat)               # out of place: the input is not touched
    there = dst.cpu().numpy()
    level.apply_device(src[:len(items) * stride].view(len(items), stride), counts, gains_dev)
    here = src.cpu().numpy()
    for bb, xx in enumerate(items):
        want = f32_bits(xx * gains[bb])
        assert np.array_equal(f32_bits(here[bb * stride:bb * stride + xx.size]), want), bb
        assert np.array_equal(f32_bits(there[bb * out_stride:bb * out_stride + xx.size]), want), bb
        assert np.all(here[bb * stride + xx.size:(bb + 1) * stride] == sentinel)
        assert np.all(there[bb * out_stride + xx.size:(bb + 1) * out_stride] == sentinel)
    assert np.all(here[len(items) * stride:] == sentinel) and np.all(there[len(items) * out_stride:] == sentinel)


# ------------------------------------------------------------------------------------------------------------------------
# the small test model
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inv(tmp_path_factory):
    from mbexwn_vocoder_amd.mel_inverter import MELInverter, create_synthetic_model_dir
    path = create_synthetic_model_dir(str(tmp_path_factory.mktemp("model") / "speech_small"), "SPEECH", **SMALL)
    return MELInverter(path, conv_form="f23")                    # the forward's kernels are pinned


def voiced(seed, n, rate, f0=150.0):
    rng = np.random.default_rng(seed)
    tt = np.arange(n) / float(rate)
    xx = sum(np.sin(2 * np.pi * f0 * kk * tt) / kk for kk in range(1, 12))
    return (0.2 * xx / np.max(np.abs(xx)) + 0.01 * rng.normal(size=n)).astype(np.float32)


@pytest.fixture(scope="module")
def mels(inv):
    """Scaled mels of three voiced sounds of 0.6, 0.8 and 0.5 s."""
    from mbexwn_vocoder_amd.analysis import generate_mels
    sounds = [voiced(70, 14400, 24000), voiced(71, 19200, 24000, 210.0), voiced(72, 12000, 24000, 120.0)]
    return [inv.scale_mel(dd) for dd in generate_mels(sounds, [24000] * 3, inv.preprocess_config, on_device=True)]


@pytest.fixture(scope="module")
def plain(inv, mels):
    """The ungained audio of the three mels: the reference of the tests below, computed once."""
    return inv.synth_from_mels(mels, noise_seed=SEED, max_batch=3)


def test_synth_from_mels_comes_out_at_the_loudness(inv, mels, plain):
    from mbexwn_vocoder_amd import flac, level
    reports = []
    got = inv.synth_from_mels(mels, noise_seed=SEED, max_batch=3, loudness=-23.0, peak_limit=60.0, levels_out=reports)
    for ii, (out, raw, rep) in enumerate(zip(got, plain, reports)):
        before = level.measure_host(raw, inv.srate)
        assert before.count > 0 and not rep["limited"]
        assert abs(level.measure_host(out, inv.srate).lufs + 23.0) <= 0.01, ii
        assert abs(rep["loudness_in"] - before.lufs) < 1e-9 and abs(rep["loudness_out"] + 23.0) <= 0.01
        # one float32 product by the reported gain of the ungained audio
        assert np.array_equal(f32_bits(out), f32_bits(raw * np.float32(rep["gain"]))), ii
    # a binding ceiling: 0 LUFS is out of reach below -6 dBFS
    limit = 10 ** (-6 / 20)
    reports = []
    loud = inv.synth_from_mels(mels, noise_seed=SEED, max_batch=3, loudness=0.0, peak_limit=-6.0, levels_out=reports)
    for out, rep in zip(loud, reports):
        assert rep["limited"] and limit * (1 - 1e-6) <= np.max(np.abs(out)) <= limit * (1 + 1e-6)
        assert abs(rep["peak_out"] - np.max(np.abs(out))) == 0
    # a ceiling alone only scales down: slack it leaves the bits, binding it holds
    same = inv.synth_from_mels(mels, noise_seed=SEED, max_batch=3, peak_limit=60.0)
    assert all(np.array_equal(f32_bits(aa), f32_bits(bb)) for aa, bb in zip(same, plain))
    low = min(float(np.max(np.abs(raw))) for raw in plain) / 2
    held = inv.synth_from_mels(mels, noise_seed=SEED, max_batch=3, peak_limit=20 * np.log10(low))
    assert all(np.max(np.abs(out)) <= low * (1 + 1e-6) for out in held)
    # FLAC: the frames hold the gained audio, nothing is clipped
    for compression in ("verbatim", "fixed"):
        streams = inv.synth_from_mels(mels, noise_seed=SEED, max_batch=3, loudness=0.0, peak_limit=-6.0, flac=True,
                                      flac_compression=compression)
        for stream, out in zip(streams, loud):
            pcm, rate = flac.decode(stream)
            assert rate == inv.srate and np.array_equal(pcm, flac.to_pcm16(out)) and np.max(np.abs(pcm.astype(np.int32))) < 32767
    # with an output rate the measure is taken at that rate
    reports = []
    down = inv.synth_from_mels(mels, noise_seed=SEED, max_batch=3, out_rate=11025, loudness=-23.0, peak_limit=60.0,
                               levels_out=reports)
    ungained = inv.synth_from_mels(mels, noise_seed=SEED, max_batch=3, out_rate=11025)
    for out, raw, rep in zip(down, ungained, reports):
        assert out.shape == raw.shape and abs(level.measure_host(out, 11025).lufs + 23.0) <= 0.01
        assert abs(rep["loudness_in"] - level.measure_host(raw, 11025).lufs) < 1e-9
    # true peak: the ceiling holds for the oversampled signal
    reports = []
    inv.synth_from_mels(mels[:1], noise_seed=SEED, loudness=0.0, peak_limit=-6.0, true_peak=True, levels_out=reports)
    assert reports[0]["limited"] and reports[0]["peak_out"] <= limit * (1 + 1e-6)
    assert reports[0]["peak_in"] >= float(np.max(np.abs(plain[0])))
    assert inv.measure_loudness(plain[0], inv.srate).power == level.measure_host(plain[0], inv.srate).power
    # no samples: not measurable, nothing launched
    empty = inv.measure_loudness(np.zeros(0, dtype=np.float32), inv.srate, true_peak=True)
    assert (empty.count, empty.power, float(empty.sample_peak), float(empty.true_peak)) == (0, 0.0, 0.0, 0.0)
    import torch
    nothing = torch.zeros((2, 0), dtype=torch.float32, device="cuda")
    assert [mm.count for mm in level.measure_device(nothing, [0, 0], 24000).host()] == [0, 0]
    assert level.apply_device(nothing, [0, 0], torch.ones(2, device="cuda")).shape == (2, 0)


def test_an_items_level_does_not_depend_on_the_batch(inv, mels, plain):
    """Item 2 of a batch of 3 and the same item alone: the same measure, the same gain, the same samples."""
    from mbexwn_vocoder_amd import level
    together, alone = [], []
    batch = inv.synth_from_mels(mels, noise_seed=SEED, noise_keys=[0, 1, 2], max_batch=3, loudness=-20.0, levels_out=together)
    single = inv.synth_from_mels(mels[2:], noise_seed=SEED, noise_keys=[2], loudness=-20.0, levels_out=alone)
    assert np.array_equal(f32_bits(batch[2]), f32_bits(single[0])) and together[2] == alone[0]
    audio, counts = stage([plain[0], plain[1], plain[2]])
    own, own_counts = stage([plain[2]], pad=5)
    three = level.measure_device(audio, counts, inv.srate, true_peak=True)
    one = level.measure_device(own, own_counts, inv.srate, true_peak=True)
    assert np.array_equal(three.records.cpu().numpy()[2], one.records.cpu().numpy()[0])
    assert np.array_equal(f64_bits(three.host()[2].energies), f64_bits(one.host()[0].energies))


def test_transform_audio_keeps_the_loudness_of_its_input(inv):
    from mbexwn_vocoder_amd import level
    sounds = [voiced(80, 14400, 24000), voiced(81, 26460, 44100, 190.0), voiced(82, 2000, 24000)]
    rates, names = [24000, 44100, 24000], ["a.wav", "b.wav", "c.wav"]
    shift = [1.3, 1.3, 1.3]
    reports = []
    got = inv.transform_audio(sounds, rates, names, noise_seed=SEED, formant=shift, loudness="input", peak_limit=60.0,
                              levels_out=reports)
    raw = inv.transform_audio(sounds, rates, names, noise_seed=SEED, formant=shift)
    for ii in range(2):
        source = level.measure_host(sounds[ii], rates[ii]).lufs
        assert abs(level.measure_host(got[ii], inv.srate).lufs - source) <= 0.02, ii
        assert abs(level.measure_host(raw[ii], inv.srate).lufs - source) > 0.1, ii       # the feature does something
    # a source under 0.4 s is not measurable: its loudness gain stays 1
    assert level.measure_host(sounds[2], 24000).count == 0 and reports[2]["gain"] == 1.0
    assert np.array_equal(f32_bits(got[2]), f32_bits(raw[2]))
    # "input" brings the default ceiling of -1 dBFS along, on the true peak where that is asked for
    reports = []
    inv.transform_audio(sounds[:1], rates[:1], names[:1], noise_seed=SEED, formant=shift[:1], loudness="input", true_peak=True,
                        levels_out=reports)
    assert 0 < reports[0]["peak_out"] <= 10 ** (-1 / 20) * (1 + 1e-6)


def test_the_file_jobs_write_the_level_and_say_so(inv, tmp_path, capsys):
    """run_audio_job with the loudness of the input and run_job with a loudness: the files hold the gained audio, nothing is
    clipped, and the writer reports the level in place of the clipping note."""
    from scipy.io import wavfile
    from mbexwn_vocoder_amd import level
    from mbexwn_vocoder_amd.analysis import generate_mels
    from mbexwn_vocoder_amd.audioio import read_audio
    from mbexwn_vocoder_amd.batched import run_audio_job, run_job
    from mbexwn_vocoder_amd.fileio import save_var
    sounds = {"a.wav": (voiced(90, 14400, 24000), 24000), "b.wav": (voiced(91, 26460, 44100, 190.0), 44100)}
    files = []
    for name, (snd, rate) in sounds.items():
        files.append(str(tmp_path / name))
        wavfile.write(files[-1], rate, snd)
    out = tmp_path / "out"
    out.mkdir()
    assert run_audio_job(inv, files, str(out), "flac", noise_seed=SEED, formants=[1.3, 1.3], loudness="input", peak_limit=60.0) == []
    err = capsys.readouterr().err
    assert err.count("level of ") == 2 and "to prevent clipping" not in err and "LUFS, gain" in err
    for name, (snd, rate) in sounds.items():
        got, got_rate = read_audio(str(out / ("syn_" + name[:-4] + ".flac")))
        assert got_rate == inv.srate
        # 16-bit samples: the quantisation noise lies 60 dB and more below these signals
        assert abs(level.measure_host(got, got_rate).lufs - level.measure_host(snd, rate).lufs) <= 0.03, name
    # without the option: the note of before, no level line
    plain = tmp_path / "plain"
    plain.mkdir()
    run_audio_job(inv, files[:1], str(plain), "flac", noise_seed=SEED, formants=[1.3])
    assert "level of " not in capsys.readouterr().err
    # resynth_mel's job: a loudness out of reach under the ceiling, which then sets the gain
    mell = str(tmp_path / "a.mell")
    save_var(mell, generate_mels([sounds["a.wav"][0]], [24000], inv.preprocess_config, on_device=True)[0])
    run_job(inv, [mell], str(out), "flac", batch=1, level=level.level_control(0.0, -6.0))
    err = capsys.readouterr().err
    assert "level of " in err and "the peak limit" in err
    got, _ = read_audio(str(out / "syn_a.flac"))
    assert 0.49 <= np.max(np.abs(got)) <= 10 ** (-6 / 20) + 2.0 ** -15

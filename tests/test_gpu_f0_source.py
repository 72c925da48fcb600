"""The F0 tracker through the package: generate_mels(f0_out=) against the host definition, MELInverter.transform_audio with
f0_source="audio" against synth_from_mels(f0s=) of the host-tracked contours, the oscillator's contour against mbx_lin_interp
of the filled contour, the defaults against the calls without the new arguments -- all bit for bit, on the synthetic canonical
model with batch_invariant kernels -- and generate_mel.py --write-f0 followed by resynth_mel.py --f0-dir."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import build_case
from mbexwn_vocoder_amd import analysis, f0track, timemap

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")
SEED = 11
SR = 24000


def bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float32).view(np.uint32)


def run_script(name, args):
    return subprocess.run([sys.executable, os.path.join(BIN, name + ".py"), *args], capture_output=True, text=True, timeout=600)


def harmonic(freq, rate):
    """Eight harmonics at 0.5 / h on the instantaneous frequency ``freq`` (one value per sample)."""
    ph = 2 * np.pi * np.cumsum(freq) / rate
    return sum((0.5 / h) * np.sin(h * ph) for h in range(1, 9) if h * freq.max() < 0.45 * rate).astype(np.float32)


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    """helpers.build_case's canonical model, as a directory MELInverter and the tools load."""
    from mbexwn_vocoder_amd.config import dump_config
    from mbexwn_vocoder_amd.weights import save_weights
    cfg, raw, _ = build_case("SPEECH", {})
    path = str(tmp_path_factory.mktemp("model") / "speech")
    os.makedirs(path)
    dump_config(os.path.join(path, "config.yaml"), cfg)
    save_weights(os.path.join(path, "weights.npz"), raw)
    return path


@pytest.fixture(scope="module")
def inv(model_dir):
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    return MELInverter(model_dir, batch_invariant=True)


@pytest.fixture(scope="module")
def sounds():
    """(names, sounds, rates): a 150 Hz tone of 0.4 s, the vibrato glide, silence, and a 200 Hz tone at 16 kHz."""
    n = int(0.4 * SR)
    tt = np.arange(12000) / SR
    glide = 200 * 2 ** (0.5 * np.sin(2 * np.pi * 5.5 * tt) / 12) * (1 + 0.2 * tt)
    return (["tone.wav", "glide.wav", "silence.wav", "tone16.wav"],
            [harmonic(np.full(n, 150.0), SR), harmonic(glide, SR), np.zeros(7000, np.float32), harmonic(np.full(6400, 200.0), 16000)],
            [SR, SR, SR, 16000])


@pytest.fixture(scope="module")
def host_tracks(inv, sounds):
    """The definition on every sound at the model rate (the 16 kHz one through the device resampler, as generate_mels does)."""
    import torch
    from mbexwn_vocoder_amd import resample
    _, snds, rates = sounds
    prm = f0track.params(SR)
    out = []
    for snd, rate in zip(snds, rates):
        if rate != SR:
            dev, n_dev = resample.resample_device(torch.as_tensor(snd[None]).cuda(), torch.as_tensor(np.asarray([snd.size], np.int32)).cuda(),
                                                  rate, SR)
            snd = dev[0, :int(n_dev[0])].cpu().numpy()
            assert snd.size == analysis.resampled_length(6400, 16000, SR)
        out.append(f0track.track_f0_host(snd, timemap.centres(snd.size, inv.hop_size, SR, None), prm))
    return out


@pytest.fixture(scope="module")
def runs(inv, sounds, host_tracks):
    """The batch once per source, and the route through synth_from_mels with the host-tracked contours."""
    from mbexwn_vocoder_amd.noise import item_key
    names, snds, rates = sounds
    factors = [1.0, 1.25, 1.0, 0.8]
    plain = inv.transform_audio(snds, rates, names, transposition=factors, noise_seed=SEED)
    net = inv.transform_audio(snds, rates, names, transposition=factors, noise_seed=SEED, f0_source="net")
    audio = inv.transform_audio(snds, rates, names, transposition=factors, noise_seed=SEED, f0_source="audio")
    scaled = [inv.scale_mel(dd) for dd in analysis.generate_mels(snds, rates, inv.preprocess_config)]
    rows = [np.full(int(mm.shape[1]), ff, dtype=np.float32) for mm, ff in zip(scaled, factors)]
    keys = [item_key(nn) for nn in names]
    contours = [f0track.fill_unvoiced(ff) for ff, _ in host_tracks]
    routed = inv.synth_from_mels(scaled, noise_seed=SEED, noise_keys=keys, transpositions=rows, f0s=contours)
    without = inv.synth_from_mels(scaled, noise_seed=SEED, noise_keys=keys, transpositions=rows)
    none = inv.synth_from_mels(scaled, noise_seed=SEED, noise_keys=keys, transpositions=rows, f0s=[None] * 4)
    return {"plain": plain, "net": net, "audio": audio, "routed": routed, "without": without, "none": none, "scaled": scaled,
            "contours": contours, "keys": keys}


def test_generate_mels_tracks_what_the_host_tracks(inv, sounds, host_tracks):
    _, snds, rates = sounds
    plain = analysis.generate_mels(snds, rates, inv.preprocess_config, batch=3)
    tracked = []
    dicts = analysis.generate_mels(snds, rates, inv.preprocess_config, batch=3, f0_out=tracked)
    assert len(tracked) == 4
    for ii, (got, want) in enumerate(zip(tracked, host_tracks)):
        assert sorted(dicts[ii]) == sorted(plain[ii]) and np.array_equal(bits(dicts[ii]["mell"]), bits(plain[ii]["mell"]))
        assert got[0].shape == got[1].shape == (dicts[ii]["mell"].shape[1],)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), ii
    assert np.all(tracked[2][0] == 0) and np.all(tracked[2][1] == 1)     # silence
    for ii, freq in ((0, 150.0), (3, 200.0)):                            # and the tones are found
        mid = tracked[ii][0][3:-3]
        assert np.all(mid > 0) and np.max(np.abs(1200 * np.log2(mid / freq))) < 5.0
    # MELInverter.track_f0: the single-sound call, on the device and on the host
    times, f0, per = inv.track_f0(snds[0], SR, on_device=True)
    assert np.array_equal(bits(f0), bits(host_tracks[0][0])) and np.array_equal(bits(per), bits(host_tracks[0][1]))
    assert times.shape == f0.shape and times[1] == inv.hop_size / SR
    _, f0_host, _ = inv.track_f0(snds[0], SR)
    assert np.array_equal(bits(f0_host), bits(f0))
    # MBExWNEngine.track_f0: device tensors in and out, the parameters by keyword
    import torch
    cc = timemap.centres(snds[0].size, inv.hop_size, SR, None)
    f0_dev, per_dev = inv.model.track_f0(torch.as_tensor(snds[0][None]).cuda(), torch.as_tensor(np.asarray([snds[0].size], np.int32)).cuda(),
                                         torch.as_tensor(cc[None]).cuda(), torch.as_tensor(np.asarray([cc.size], np.int32)).cuda(),
                                         f0_min=55.0, f0_max=1000.0)
    assert np.array_equal(bits(f0_dev[0].cpu().numpy()), bits(f0)) and np.array_equal(bits(per_dev[0].cpu().numpy()), bits(per))


def test_audio_source_equals_the_route_through_synth_from_mels(runs):
    assert runs["contours"][2] is None and all(runs["contours"][ii] is not None for ii in (0, 1, 3))
    for ii in range(4):
        assert runs["audio"][ii].shape == runs["routed"][ii].shape
        assert np.array_equal(bits(runs["audio"][ii]), bits(runs["routed"][ii])), ii
    # the tracked pitch is used: the voiced items differ from the F0-net's audio; the silent item keeps the F0-net
    for ii in (0, 1, 3):
        assert not np.array_equal(bits(runs["audio"][ii]), bits(runs["net"][ii])), ii
    assert np.array_equal(bits(runs["audio"][2]), bits(runs["net"][2]))


def test_defaults_keep_the_bits_of_the_calls_without_the_arguments(runs):
    for ii in range(4):
        assert np.array_equal(bits(runs["net"][ii]), bits(runs["plain"][ii])), ii
        assert np.array_equal(bits(runs["none"][ii]), bits(runs["without"][ii])), ii
        assert np.array_equal(bits(runs["without"][ii]), bits(runs["plain"][ii])), ii


def test_the_oscillator_runs_on_the_filled_contour(inv, sounds, runs):
    """Stage "f0" of a voiced item alone: mbx_lin_interp of its filled contour, times that of its transposition row."""
    import torch
    names, snds, rates = sounds
    eng = inv.model
    ppf = eng.dims.pulse_per_frame

    def li(row):
        return eng.lin_interp(torch.as_tensor(np.ascontiguousarray(row, dtype=np.float32)[None, :, None]).cuda(), ppf).cpu().numpy()[0, :, 0]

    for ii, factor in ((1, 1.25), (3, 0.8)):
        alone = inv.transform_audio([snds[ii]], [rates[ii]], [names[ii]], transposition=factor, noise_seed=SEED, f0_source="audio")[0]
        got = eng.stage("f0").cpu().numpy()[0]
        assert np.array_equal(bits(alone), bits(runs["audio"][ii]))      # batch_invariant: alone as in the batch
        frames = runs["contours"][ii].size
        want = li(runs["contours"][ii]) * li(np.full(frames, factor, dtype=np.float32))
        assert want.dtype == np.float32 and np.array_equal(bits(got[:frames * ppf]), bits(want)), ii


def test_time_stretch_tracks_on_the_warped_frames(inv, sounds):
    names, snds, rates = sounds
    tracked = []
    dicts = analysis.generate_mels(snds[:2], rates[:2], inv.preprocess_config, time_maps=[1.5, None], f0_out=tracked,
                                   rows_per_frame=inv.model.dims.steps_per_frame)
    cc = timemap.centres(snds[0].size, inv.hop_size, SR, 1.5)
    assert tracked[0][0].shape == (cc.size,) == (dicts[0]["mell"].shape[1],) and cc.size == int(snds[0].size * 1.5) // inv.hop_size + 1
    want = f0track.track_f0_host(snds[0], cc, f0track.params(SR))
    assert np.array_equal(bits(tracked[0][0]), bits(want[0])) and np.array_equal(bits(tracked[0][1]), bits(want[1]))
    mid = tracked[0][0][4:-4]
    assert np.all(mid > 0) and np.max(np.abs(1200 * np.log2(mid / 150.0))) < 5.0                      # stretched, the same pitch
    out = inv.transform_audio(snds[:1], rates[:1], names[:1], noise_seed=SEED, time_stretch=1.5, f0_source="audio")[0]
    assert out.shape == (cc.size * inv.hop_size,) and np.all(np.isfinite(out))


def test_file_job_takes_the_pitch_from_the_audio_and_writes_the_contours(inv, sounds, host_tracks, runs, tmp_path):
    """batched.run_audio_job, the job of transform_audio.py: with f0_source="audio" the files decode to the 16-bit samples of
    transform_audio(f0_source="audio"), in micro-batches of two; write_f0 writes every file's tracked contour, with either
    source, and "net" without it writes the files of the job without the arguments."""
    from scipy.io import wavfile
    from mbexwn_vocoder_amd import flac
    from mbexwn_vocoder_amd.audioio import read_audio
    from mbexwn_vocoder_amd.batched import run_audio_job
    names, snds, rates = sounds
    files = []
    for name, snd, rate in zip(names, snds, rates):
        files.append(str(tmp_path / name))
        wavfile.write(files[-1], rate, snd)
    factors = [1.0, 1.25, 1.0, 0.8]
    outs = {}
    for tag, kw in (("plain", {}), ("net", {"f0_source": "net", "write_f0": True}), ("audio", {"f0_source": "audio", "write_f0": True})):
        outs[tag] = str(tmp_path / tag)
        os.makedirs(outs[tag])
        timings = {}
        assert run_audio_job(inv, files, outs[tag], "flac", factors=factors, noise_seed=SEED, batch=2, quiet=True, timings=timings,
                             **kw) == []
        assert ("f0" in timings) == bool(kw) and timings["wall"] > 0
    stems = [os.path.splitext(nn)[0] for nn in names]
    assert sorted(os.listdir(outs["plain"])) == sorted(f"syn_{ss}.flac" for ss in stems)
    for ii, stem in enumerate(stems):
        got, rate = read_audio(os.path.join(outs["audio"], f"syn_{stem}.flac"))
        assert rate == SR and np.array_equal(got, flac.to_pcm16(runs["audio"][ii]).astype(np.float32) / np.float32(32768.0)), stem
        plain = open(os.path.join(outs["plain"], f"syn_{stem}.flac"), "rb").read()
        assert open(os.path.join(outs["net"], f"syn_{stem}.flac"), "rb").read() == plain, stem
        for tag in ("net", "audio"):
            times, f0, per = f0track.read_f0(os.path.join(outs[tag], stem + ".f0"))
            assert np.array_equal(bits(f0), bits(host_tracks[ii][0])) and np.array_equal(bits(per), bits(host_tracks[ii][1])), (tag, stem)
            assert times.shape == f0.shape


@pytest.mark.timeout(600)
def test_cli_write_f0_then_f0_dir_equals_the_library_call(inv, model_dir, sounds, host_tracks, tmp_path):
    """generate_mel.py --write-f0 on one file, then resynth_mel.py --f0-dir on its .mell: the 16-bit samples of
    synth_from_mel(f0=filled contour) with the file's keyed noise -- one file at a time and through --batch."""
    from scipy.io import wavfile
    from mbexwn_vocoder_amd import flac
    from mbexwn_vocoder_amd.audioio import read_audio
    from mbexwn_vocoder_amd.fileio import load_var
    from mbexwn_vocoder_amd.noise import item_key
    _, snds, _ = sounds
    wav = str(tmp_path / "glide.wav")
    wavfile.write(wav, SR, snds[1])
    mells = str(tmp_path / "mells")
    res = run_script("generate_mel", [wav, "-o", mells, "--model_id", model_dir, "--write-f0", "-q"])
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(os.listdir(mells)) == ["glide.f0", "glide.mell"]
    saved = load_var(os.path.join(mells, "glide.mell"))
    _, f0, per = f0track.read_f0(os.path.join(mells, "glide.f0"), n_frames=saved["mell"].shape[1])
    assert np.array_equal(bits(f0), bits(host_tracks[1][0])) and np.array_equal(bits(per), bits(host_tracks[1][1]))
    mell = os.path.join(mells, "glide.mell")
    want = inv.synth_from_mel(inv.scale_mel(saved), f0=f0track.fill_unvoiced(f0), noise_seed=SEED, noise_key=item_key(mell))
    want16 = flac.to_pcm16(want).astype(np.float32) / np.float32(32768.0)
    for tag, extra in (("single", []), ("batch", ["--batch", "2"])):
        out = str(tmp_path / tag)
        res = run_script("resynth_mel", [model_dir, "-i", mell, "-o", out, "--f0-dir", mells, "--noise-seed", str(SEED),
                                         "--batch-invariant", "-q", *extra])
        assert res.returncode == 0, res.stderr[-3000:]
        got, rate = read_audio(os.path.join(out, "syn_glide.flac"))
        assert rate == SR and np.array_equal(got, want16), tag

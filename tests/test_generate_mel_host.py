"""bin/generate_mel.py with --host (numpy analysis, host resampler; no GPU): file names, the .mell dictionary of the
reference's tool (reference bin/generate_mel.py:41-52,64), and the Python routes that give the same arrays."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin", "generate_mel.py")
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 3}
RATES = (24000, 48000, 16000)


def signal(rate, n, seed):
    tt = np.arange(n) / rate
    return (0.3 * np.sin(2 * np.pi * 220.0 * tt) + 0.05 * np.random.default_rng(seed).normal(size=n)).astype(np.float32)


def host_inverter(pre):
    """A MELInverter without a model (no engine, no GPU) carrying the pre-processing attributes load_model copies."""
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    inv = MELInverter(None)
    inv.preprocess_config, inv._srate = pre, pre["sample_rate"]
    inv.hop_size, inv.fft_size, inv.win_len, inv.mel_channels = pre["hop_size"], pre["fft_size"], pre["win_size"], pre["mel_channels"]
    inv.fmin, inv.fmax = pre["fmin"], pre["fmax"]
    inv.lin_amp_off, inv.lin_amp_scale, inv.mel_amp_scale = pre["lin_amp_off"], pre["lin_amp_scale"], pre["mel_amp_scale"]
    return inv


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    return create_synthetic_model_dir(str(tmp_path_factory.mktemp("model") / "speech_small"), "SPEECH", **SMALL)


@pytest.fixture(scope="module")
def run(model_dir, tmp_path_factory):
    """One --host run of the tool on three float32 wav files: (sounds by rate, output directory, stderr)."""
    from scipy.io import wavfile
    root = tmp_path_factory.mktemp("sounds")
    sounds, files = {}, []
    for ii, rate in enumerate(RATES):
        sounds[rate] = signal(rate, int(0.3 * rate) + 7 * ii + 1, ii)
        files.append(str(root / f"snd_{rate}.wav"))
        wavfile.write(files[-1], rate, sounds[rate])
    out = str(root / "out" / "nested")                          # created if missing
    res = subprocess.run([sys.executable, CLI, *files, "-o", out, "--model_id", model_dir, "--host", "--batch", "2"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return sounds, out, res.stderr


def test_tool_writes_the_reference_schema(run, model_dir):
    from mbexwn_vocoder_amd.config import read_config
    from mbexwn_vocoder_amd.fileio import load_var
    sounds, out, stderr = run
    assert sorted(os.listdir(out)) == sorted(f"snd_{rate}.mell" for rate in RATES)
    assert all(f"snd_{rate}.wav" in stderr for rate in RATES)
    pre = read_config(os.path.join(model_dir, "config.yaml"))["preprocess_config"]
    want = {"nfft": pre["fft_size"], "hoplen": pre["hop_size"], "winlen": pre["win_size"], "nmels": pre["mel_channels"],
            "sr": pre["sample_rate"], "fmin": pre["fmin"], "fmax": pre["fmax"], "lin_spec_offset": pre["lin_amp_off"],
            "lin_spec_scale": pre["lin_amp_scale"], "log_spec_offset": 0., "log_spec_scale": pre["mel_amp_scale"],
            "time_axis": 1}
    assert (want["nfft"], want["hoplen"], want["winlen"], want["nmels"], want["sr"]) == (2048, 300, 1200, 80, 24000)
    for rate in RATES:
        dd = load_var(os.path.join(out, f"snd_{rate}.mell"))
        mell = dd.pop("mell")
        assert dd == want and list(dd) == list(want)
        assert type(dd["log_spec_offset"]) is float and type(dd["time_axis"]) is int
        n_out = -(-sounds[rate].size * 24000 // rate)
        assert mell.shape == (80, n_out // 300 + 1) and mell.dtype == np.float32 and np.all(np.isfinite(mell))
        # MELInverter.scale_mel accepts the file (it reads only the pre-processing attributes of the instance)
        scaled = host_inverter(pre).scale_mel(dict(dd, mell=mell))
        assert scaled.shape == (1, mell.shape[1], 80)


def test_python_routes_equal_the_tool(run, model_dir):
    """analysis.generate_mels(on_device=False) and the analysis the tool's file went through are one code path; the host
    resampler in front of analysis.compute_log_mel gives the same array by hand."""
    from mbexwn_vocoder_amd import resample
    from mbexwn_vocoder_amd.analysis import compute_log_mel, generate_mels
    from mbexwn_vocoder_amd.config import read_config
    from mbexwn_vocoder_amd.fileio import load_var
    sounds, out, _ = run
    pre = read_config(os.path.join(model_dir, "config.yaml"))["preprocess_config"]
    dicts = generate_mels([sounds[rate] for rate in RATES], list(RATES), pre, on_device=False)
    for rate, dd in zip(RATES, dicts):
        tool = load_var(os.path.join(out, f"snd_{rate}.mell"))["mell"]
        assert np.array_equal(dd["mell"], tool)
        by_hand, _ = compute_log_mel(resample.resample_host(sounds[rate], rate, 24000)[np.newaxis], pre, dtype=np.float32)
        assert np.array_equal(by_hand[0].T, tool)
    with pytest.raises(ValueError):
        generate_mels([np.zeros(0, dtype=np.float32)], [24000], pre, on_device=False)
    with pytest.raises(ValueError):
        generate_mels([sounds[24000]], [24000, 48000], pre, on_device=False)


def test_generate_mel_from_snd_with_the_reference_resampler_equals_the_tool(run, model_dir):
    """MELInverter.generate_mel_from_snd(resampler="reference") on the host; the default route keeps scipy's window and
    differs for a resampled sound.  (The method reads only the pre-processing attributes: no engine is built here.)"""
    from mbexwn_vocoder_amd.config import read_config
    from mbexwn_vocoder_amd.fileio import load_var
    sounds, out, _ = run
    pre = read_config(os.path.join(model_dir, "config.yaml"))["preprocess_config"]
    inv = host_inverter(pre)
    for rate in RATES:
        tool = load_var(os.path.join(out, f"snd_{rate}.mell"))
        got = inv.generate_mel_from_snd(sounds[rate], rate, resampler="reference")
        assert list(got) == list(tool) and np.array_equal(got["mell"], tool["mell"])
        default = inv.generate_mel_from_snd(sounds[rate], rate)
        assert list(default) == list(tool) and default["mell"].shape == tool["mell"].shape
        assert np.array_equal(default["mell"], tool["mell"]) == (rate == 24000)
    with pytest.raises(ValueError, match="resampler"):
        inv.generate_mel_from_snd(sounds[24000], 24000, resampler="sox")


def test_tool_refuses_missing_files_missing_gpu_and_lists_models(run, model_dir, tmp_path):
    import torch
    sounds, out, _ = run
    res = subprocess.run([sys.executable, CLI, str(tmp_path / "nothing.wav"), "-o", str(tmp_path / "o"), "--model_id", model_dir,
                          "--host"], capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "nothing.wav" in res.stderr and not os.path.exists(tmp_path / "o")
    res = subprocess.run([sys.executable, CLI, "x.wav", "-o", str(tmp_path / "o"), "--model_id"], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0 and "VOICE/" in res.stdout and "SPEECH/" in res.stdout
    if not torch.cuda.is_available():
        from scipy.io import wavfile
        wavfile.write(str(tmp_path / "a.wav"), 24000, sounds[24000])
        res = subprocess.run([sys.executable, CLI, str(tmp_path / "a.wav"), "-o", str(tmp_path / "o"), "--model_id", model_dir],
                             capture_output=True, text=True, timeout=300)
        assert res.returncode != 0 and "no GPU" in res.stderr and "--host" in res.stderr

"""Batched and sharded mel inversion on the GPU: the device FLAC encoder (mbx_encode_flac16) against the host writer, and
resynth_mel.py --batch / --gpus against the one-at-a-time CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin", "resynth_mel.py")
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 3}


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    return create_synthetic_model_dir(str(tmp_path_factory.mktemp("model") / "speech_small"), "SPEECH", **SMALL)


@pytest.fixture(scope="module")
def engine(model_dir):
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    return MELInverter(model_dir).model


def test_device_encoder_matches_the_host_writer(engine):
    """A ragged, seeded device batch (2- and 3-byte frame numbers, a last frame of exactly 4096, half-LSB ties, values
    beyond +-1, -0.0): every item's stream equals flac.encode of its host copy, every max |x| numpy's."""
    import torch
    from mbexwn_vocoder_amd import flac
    lengths = [1, 4095, 4096, 4097, 3 * 4096, 128 * 4096 + 1, 2048 * 4096 + 1]
    special = np.array([0.5, -0.5, -0.0, 1.5, -1.5, 1.2, -3.0, 1.0, -1.0, np.nextafter(np.float32(0.5), np.float32(1)),
                        np.nextafter(np.float32(-0.5), np.float32(0)), 16383.5 / 32767, 0.0], dtype=np.float32)
    rng = np.random.default_rng(11)
    host = np.zeros((len(lengths), max(lengths)), dtype=np.float32)
    for bb, nn in enumerate(lengths):
        xx = (0.5 * rng.standard_normal(nn)).astype(np.float32)
        pos = rng.integers(0, nn, size=special.size)
        xx[pos] = special
        host[bb, :nn] = xx
    enc = engine.encode_flac16(torch.as_tensor(host, device=engine.device), lengths, sample_rate=24000)
    for bb, nn in enumerate(lengths):
        xx = host[bb, :nn]
        assert enc.max_abs[bb] == np.max(np.abs(xx))
        assert enc.stream(bb) == flac.encode(xx, 24000), f"item {bb} ({nn} samples)"
    # a rate outside FLAC's table (code 0), a NaN item flagged through max |x|
    small = np.stack([0.3 * rng.standard_normal(5000), 0.3 * rng.standard_normal(5000)]).astype(np.float32)
    small[1, 777] = np.nan
    enc = engine.encode_flac16(torch.as_tensor(small, device=engine.device), [5000, 5000], sample_rate=12345)
    assert enc.stream(0) == flac.encode(small[0], 12345) and enc.max_abs[0] == np.max(np.abs(small[0]))
    assert not np.isfinite(enc.max_abs[1])
    with pytest.raises(ValueError, match="stride"):
        engine.encode_flac16(torch.as_tensor(small, device=engine.device), [5001, 10], sample_rate=24000)


def test_synth_from_mels_equals_synth_from_mel_one_at_a_time(model_dir):
    """MELInverter.synth_from_mels on a batch-invariant handle: same seed, the same audio bits as synth_from_mel called on
    the list one by one; flac=True gives the files the host writer makes of them."""
    import torch
    from mbexwn_vocoder_amd import flac
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    inv = MELInverter(model_dir, batch_invariant=True)
    rng = np.random.default_rng(2)
    mels = [rng.normal(-5, 2, size=(1, int(tt), 80)).astype(np.float32) for tt in (17, 4, 33, 9, 21)]
    torch.manual_seed(5)
    singles = [inv.synth_from_mel(mm) for mm in mels]
    torch.manual_seed(5)
    batched = inv.synth_from_mels(mels, max_batch=3)
    assert all(np.array_equal(aa, bb) for aa, bb in zip(singles, batched))
    torch.manual_seed(5)
    files = inv.synth_from_mels(mels, max_batch=2, flac=True)
    assert all(ff == flac.encode(aa, inv.srate) for ff, aa in zip(files, singles))


def mell_dict(frames, seed, hoplen=300):
    rng = np.random.default_rng(seed)
    return {"nfft": 2048, "hoplen": hoplen, "winlen": 1200, "nmels": 80, "sr": 24000, "fmin": 0.0, "fmax": 12000.0,
            "lin_spec_offset": 1e-5, "lin_spec_scale": 1, "log_spec_offset": 0.0, "log_spec_scale": 1, "time_axis": 1,
            "mell": rng.normal(-5, 2, size=(80, frames)).astype(np.float32)}


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """6 ragged .mell files; the third has a hop of 256 samples, which scale_mel resamples to the model's 300."""
    from mbexwn_vocoder_amd.fileio import save_var
    root = tmp_path_factory.mktemp("corpus")
    files = []
    for ii, (frames, hop) in enumerate([(23, 300), (7, 300), (52, 256), (15, 300), (36, 300), (11, 300)]):
        files.append(str(root / f"utt{ii}.mell"))
        save_var(files[-1], mell_dict(frames, 40 + ii, hop))
    return files


def run_cli(args, timeout=600):
    return subprocess.run([sys.executable, CLI, *args], capture_output=True, text=True, timeout=timeout)


def expected_names(files, fmt):
    return sorted(f"syn_{os.path.splitext(os.path.basename(ff))[0]}.{fmt}" for ff in files)


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("fmt", ["flac", "wav"])
def test_batched_and_sharded_files_are_bit_identical(model_dir, corpus, tmp_path, fmt):
    outs = {}
    for name, extra in (("single", []), ("batch", ["--batch", "4"]), ("gpus", ["--gpus", "2", "--batch", "3"])):
        out = str(tmp_path / name)
        res = run_cli([model_dir, "-i", *corpus, "-o", out, "--format", fmt, "--batch-invariant", *extra])
        assert res.returncode == 0, res.stderr[-3000:]
        assert sorted(os.listdir(out)) == expected_names(corpus, fmt)
        assert all(f"synthesize {ff} into" in res.stderr for ff in corpus)
        outs[name] = {nn: open(os.path.join(out, nn), "rb").read() for nn in os.listdir(out)}
    assert outs["batch"] == outs["single"]
    assert outs["gpus"] == outs["single"]


@pytest.mark.timeout(900)
def test_default_handle_batched_wav_within_float32_rounding(model_dir, corpus, tmp_path):
    """Without --batch-invariant large launches may take other res/skip kernels: the batched files stay within
    1e-4 * max(1, |audio|) of the one-at-a-time ones.  -v adds each file's mel error and the summary line."""
    from scipy.io import wavfile
    single, batch = str(tmp_path / "single"), str(tmp_path / "batch")
    res = run_cli([model_dir, "-i", *corpus, "-o", single, "--format", "wav", "-q"])
    assert res.returncode == 0, res.stderr[-3000:]
    res = run_cli([model_dir, "-i", *corpus, "-o", batch, "--format", "wav", "--batch", "4", "-v", "-nt", "3"])
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stderr.count("mel_error:") == len(corpus) and "x real time" in res.stderr and "MD5+write" in res.stderr
    for name in expected_names(corpus, "wav"):
        r1, a1 = wavfile.read(os.path.join(single, name))
        r2, a2 = wavfile.read(os.path.join(batch, name))
        assert r1 == r2 == 24000 and a1.shape == a2.shape
        assert np.max(np.abs(a1 - a2)) <= 1e-4 * max(1.0, float(np.max(np.abs(a1))))


@pytest.mark.timeout(900)
@pytest.mark.parametrize("extra", [["--batch", "4"], ["--gpus", "2", "--batch", "3"]])
def test_missing_input_fails_before_any_file_is_written(model_dir, corpus, tmp_path, extra):
    out = str(tmp_path / "out")
    files = corpus[:3] + [str(tmp_path / "missing.mell")] + corpus[3:]
    res = run_cli([model_dir, "-i", *files, "-o", out, *extra])
    assert res.returncode != 0 and "missing.mell" in res.stderr
    assert not os.path.exists(out) or os.listdir(out) == []

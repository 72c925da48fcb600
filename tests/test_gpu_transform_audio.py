"""The file-to-file tool on the GPU: with keyed noise a file's output is a function of the file -- not of the batch, the
order or the other files --, it equals the live stream of the file and the two-step route, and the command-line tools write
it."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 5}
SEED = 7
# 0.3 s, 0.45 s at 44.1 kHz, 0.6 s
SOUNDS = [("alto.wav", 7200, 24000, 1.25), ("basso.wav", 19845, 44100, 0.8), ("canto.wav", 14400, 24000, 1.0)]


def bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float32).view(np.int32)


def sound(seed, n, rate):
    rng = np.random.default_rng(seed)
    tt = np.arange(n) / float(rate)
    return (0.3 * np.sin(2 * np.pi * 170.0 * tt) + 0.05 * rng.normal(size=n)).astype(np.float32)


def run_script(name, args):
    return subprocess.run([sys.executable, os.path.join(BIN, name + ".py"), *args], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    return create_synthetic_model_dir(str(tmp_path_factory.mktemp("model") / "speech_small"), "SPEECH", **SMALL)


@pytest.fixture(scope="module")
def inv(model_dir):
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    return MELInverter(model_dir, conv_form="f23")


@pytest.fixture(scope="module")
def sounds():
    return [sound(30 + ii, nn, rate) for ii, (_, nn, rate, _) in enumerate(SOUNDS)]


@pytest.fixture(scope="module")
def transformed(inv, sounds):
    """transform_audio of the three sounds in one batch: the reference of the tests below, computed once."""
    names, rates, factors = [ss[0] for ss in SOUNDS], [ss[2] for ss in SOUNDS], [ss[3] for ss in SOUNDS]
    return inv.transform_audio(sounds, rates, names, transposition=factors, noise_seed=SEED, max_batch=3)


def model_frames(n, rate, hop=300):
    from mbexwn_vocoder_amd.resample import reference_filter
    if rate == 24000:
        return n // hop + 1
    _, up, down = reference_filter(rate, 24000)
    return -(-n * up // down) // hop + 1


def test_output_is_a_function_of_the_file(inv, sounds, transformed):
    """Batch 1, batch 3, the list reversed, and a file alone: identical samples per file, frames * hop of them."""
    names, rates, factors = [ss[0] for ss in SOUNDS], [ss[2] for ss in SOUNDS], [ss[3] for ss in SOUNDS]
    for got, (_, nn, rate, _) in zip(transformed, SOUNDS):
        assert got.dtype == np.float32 and got.shape == (model_frames(nn, rate) * inv.hop_size,)
        assert np.all(np.isfinite(got)) and np.max(np.abs(got)) > 0
    single = inv.transform_audio(sounds, rates, names, transposition=factors, noise_seed=SEED, max_batch=1)
    back = inv.transform_audio(sounds[::-1], rates[::-1], names[::-1], transposition=factors[::-1], noise_seed=SEED, max_batch=3)
    alone = inv.transform_audio(sounds[1:2], rates[1:2], names[1:2], transposition=factors[1], noise_seed=SEED)
    for ii, want in enumerate(transformed):
        assert np.array_equal(bits(single[ii]), bits(want)), ii
        assert np.array_equal(bits(back[len(SOUNDS) - 1 - ii]), bits(want)), ii
    assert np.array_equal(bits(alone[0]), bits(transformed[1]))
    # the seed, the name and the factor are part of the function
    other = inv.transform_audio(sounds[:1], rates[:1], names[:1], transposition=factors[0], noise_seed=SEED + 1)
    renamed = inv.transform_audio(sounds[:1], rates[:1], ["other.wav"], transposition=factors[0], noise_seed=SEED)
    assert not np.array_equal(other[0], transformed[0]) and not np.array_equal(renamed[0], transformed[0])


def test_equals_the_two_step_route(inv, sounds, transformed):
    """Each file equals synth_from_mel(scale_mel(generate_mels([s], [r])), noise_seed=, noise_key=, transposition=rows)."""
    from mbexwn_vocoder_amd.analysis import generate_mels
    from mbexwn_vocoder_amd.noise import item_key
    for snd, (name, _, rate, factor), want in zip(sounds, SOUNDS, transformed):
        scaled = inv.scale_mel(generate_mels([snd], [rate], inv.preprocess_config, on_device=True)[0])
        rows = np.full(scaled.shape[1], factor, dtype=np.float32)
        got = inv.synth_from_mel(scaled, noise_seed=SEED, noise_key=item_key(name), transposition=rows)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), name
    # the keyed draw is what the forward got: the injected noise of the same values gives the same audio
    spf = inv.model.dims.wn_in_rows_per_frame
    noise = inv.model.keyed_noise(SEED, [item_key(name)], [scaled.shape[1] * spf])
    again = inv.synth_from_mel(scaled, noise=noise, transposition=rows)
    assert np.array_equal(bits(again), bits(transformed[-1]))


def test_equals_the_live_stream(inv, sounds, transformed):
    """Each file equals stream_file(...) of a LiveResynthesizer opened with keyed_noise_fn(engine, seed) and the same factor,
    in 80 ms pushes."""
    from mbexwn_vocoder_amd.live import LiveResynthesizer, keyed_noise_fn
    spec = importlib.util.spec_from_file_location("stream_transpose", os.path.join(BIN, "stream_transpose.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    live = LiveResynthesizer(inv)
    fn = keyed_noise_fn(inv.model, SEED)
    for snd, (name, _, rate, factor), want in zip(sounds, SOUNDS, transformed):
        got = tool.stream_file(live, snd, int(round(0.08 * rate)), factor, stream_id=name, noise_fn=fn,
                               sample_rate=None if rate == 24000 else rate)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), name


@pytest.fixture(scope="module")
def wav_files(tmp_path_factory, sounds):
    from scipy.io import wavfile
    root = tmp_path_factory.mktemp("sounds")
    files = []
    for snd, (name, _, rate, _) in zip(sounds, SOUNDS):
        files.append(str(root / name))
        wavfile.write(files[-1], rate, snd)
    wavfile.write(str(root / "empty.wav"), 24000, np.zeros(0, dtype=np.float32))
    wavfile.write(str(root / "stereo.wav"), 24000, np.zeros((2400, 2), dtype=np.float32))
    factors = root / "factors.txt"
    factors.write_text("".join(f"{name} {factor}\n" for name, _, _, factor in SOUNDS[:2]))       # canto.wav: --transposition
    return files, str(root / "empty.wav"), str(root / "stereo.wav"), str(factors)


COMMON = ["--conv-form", "f23", "--noise-seed", str(SEED), "--transposition", "1.0", "--out-rate", "16000",
          "--flac-compression", "fixed"]


@pytest.fixture(scope="module")
def first_run(model_dir, wav_files, tmp_path_factory):
    """transform_audio.py --batch 2 on the three files: {name: bytes}, written once for the command-line tests."""
    files, _, _, factors = wav_files
    out = str(tmp_path_factory.mktemp("first"))
    res = run_script("transform_audio", [*files, "-o", out, "--batch", "2", "--model_id", model_dir, "--transposition-file", factors,
                                         *COMMON])
    assert res.returncode == 0, res.stderr[-3000:]
    return out, {nn: open(os.path.join(out, nn), "rb").read() for nn in sorted(os.listdir(out))}


@pytest.mark.timeout(600)
def test_cli_ranks_write_the_same_files(model_dir, wav_files, first_run, tmp_path):
    """--gpus 2 --batch 1 (fresh children, the files shared out by duration; the stereo file is skipped by the parent): the
    files of the single process, byte for byte, and exit status 1 for the skipped one."""
    files, _, stereo, factors = wav_files
    out = str(tmp_path / "ranks")
    res = run_script("transform_audio", [stereo, *files, "-o", out, "--gpus", "2", "--batch", "1", "--model_id", model_dir,
                                         "--transposition-file", factors, *COMMON])
    assert res.returncode == 1, res.stderr[-3000:]
    assert "skipped" in res.stderr and "stereo.wav" in res.stderr
    assert {nn: open(os.path.join(out, nn), "rb").read() for nn in sorted(os.listdir(out))} == first_run[1]


@pytest.mark.timeout(600)
def test_cli_writes_the_same_files_in_any_batch_and_order(model_dir, wav_files, inv, transformed, first_run, tmp_path):
    """transform_audio.py --batch 2 --out-rate 16000 --flac-compression fixed, then --batch 1 with the arguments reversed and
    an empty and a stereo file among them (reported, skipped, exit status 1): byte-identical syn_<basename>.flac files, read
    back at 16 kHz with ceil(frames * hop * 2 / 3) samples -- the 16-bit samples of the library call resampled."""
    from mbexwn_vocoder_amd import flac
    from mbexwn_vocoder_amd.audioio import read_audio
    files, empty, stereo, factors = wav_files
    common = ["--model_id", model_dir, "--transposition-file", factors, *COMMON]
    first, second = first_run[0], str(tmp_path / "second")
    res = run_script("transform_audio", [empty, *files[::-1], stereo, "-o", second, "--batch", "1", "-v", *common])
    assert res.returncode == 1, res.stderr[-3000:]
    assert "skipped" in res.stderr and "empty.wav: no samples" in res.stderr and "stereo.wav: 2 channels" in res.stderr
    assert "x real time" in res.stderr and "scale_mel" in res.stderr
    want_names = sorted("syn_" + os.path.splitext(name)[0] + ".flac" for name, _, _, _ in SOUNDS)
    assert sorted(os.listdir(first)) == want_names and sorted(os.listdir(second)) == want_names
    for name in want_names:
        assert open(os.path.join(first, name), "rb").read() == open(os.path.join(second, name), "rb").read(), name
    import torch
    for (name, nn, rate, _), model_audio in zip(SOUNDS, transformed):
        got, got_rate = read_audio(os.path.join(first, "syn_" + os.path.splitext(name)[0] + ".flac"))
        frames = model_frames(nn, rate)
        assert got_rate == 16000 and got.shape == (-(-frames * inv.hop_size * 2 // 3),)
        want = inv._to_rate(torch.as_tensor(model_audio[None]).to(inv.model.device), 16000)[0].cpu().numpy()
        assert np.array_equal(got, flac.to_pcm16(want).astype(np.float32) / np.float32(32768.0)), name


@pytest.mark.timeout(600)
def test_resynth_mel_noise_seed_and_default(model_dir, inv, sounds, tmp_path):
    """resynth_mel.py --noise-seed 7 on two .mell files in both orders (one at a time, and reversed with --batch 2): byte-identical files per
    basename.  Without the flag the files hold the draws of the one-at-a-time loop (batched.replay_noise), as before."""
    import torch
    from mbexwn_vocoder_amd import flac
    from mbexwn_vocoder_amd.analysis import generate_mels
    from mbexwn_vocoder_amd.batched import replay_noise
    from mbexwn_vocoder_amd.fileio import save_var
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    dicts = generate_mels([sounds[0], sounds[2]], [24000, 24000], inv.preprocess_config, on_device=True)
    mells = [str(tmp_path / "one.mell"), str(tmp_path / "two.mell")]
    for path, dd in zip(mells, dicts):
        save_var(path, dd)
    outs = {}
    for tag, order, extra in (("ab", mells, []), ("batch", mells[::-1], ["--batch", "2"])):
        out = str(tmp_path / tag)
        res = run_script("resynth_mel", [model_dir, "-i", *order, "-o", out, "--batch-invariant", "--noise-seed", "7",
                                         "--transposition", "1.5", *extra])
        assert res.returncode == 0, res.stderr[-3000:]
        outs[tag] = {nn: open(os.path.join(out, nn), "rb").read() for nn in sorted(os.listdir(out))}
    assert sorted(outs["ab"]) == ["syn_one.flac", "syn_two.flac"]
    assert outs["batch"] == outs["ab"]
    # without the new flags: torch.manual_seed(42), then the loop's draws in file order
    out = str(tmp_path / "plain")
    res = run_script("resynth_mel", [model_dir, "-i", *mells, "-o", out, "--batch-invariant"])
    assert res.returncode == 0, res.stderr[-3000:]
    plain = MELInverter(model_dir, batch_invariant=True)
    scaled = [plain.scale_mel(dd) for dd in dicts]
    torch.manual_seed(42)
    draws = replay_noise([mm.shape[1] for mm in scaled], plain.model.dims.wn_in_rows_per_frame, device=plain.model.device)
    for ii, name in enumerate(("syn_one.flac", "syn_two.flac")):
        audio = plain.synth_from_mel(scaled[ii], noise=draws[ii][None])
        assert open(os.path.join(out, name), "rb").read() == flac.encode(audio, plain.srate), name
        assert outs["ab"][name] != open(os.path.join(out, name), "rb").read()

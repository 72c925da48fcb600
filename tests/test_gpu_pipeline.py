"""The file job and the library method are one pipeline: with every option switched on, ``batched.run_audio_job``,
``MELInverter.transform_audio`` and ``bin/transform_audio.py`` give the same bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 5}
SEED = 11
# three sounds of 0.5 s (about 41 frames): one aligned to a guide of 0.6 s, one stretched by 1.5, one plain; two of the three
# input rates differ from the model's, the two files at 24 and 44.1 kHz share the last micro-batch of the synthesis
FILES = [("guided.wav", 24000, 210.0, 1.25, 1.1), ("slow.wav", 16000, 140.0, 0.8, 0.9), ("plain.wav", 44100, 170.0, 1.0, 1.0)]
STRETCH = [1.0, 1.5, 1.0]


def voice(seconds, rate, f0, seed):
    tt = np.arange(int(seconds * rate)) / rate
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 3.0 * tt) ** 2
    noise = np.random.default_rng(seed).standard_normal(tt.size)
    return (0.3 * env * (np.sin(2 * np.pi * f0 * tt) + 0.5 * np.sin(4 * np.pi * f0 * tt)) + 0.01 * noise).astype(np.float32)


def test_the_job_the_method_and_the_tool_write_the_same_bytes(tmp_path):
    from scipy.io import wavfile
    from mbexwn_vocoder_amd import f0decode
    from mbexwn_vocoder_amd.batched import have_soundfile, run_audio_job
    from mbexwn_vocoder_amd.mel_inverter import MELInverter, create_synthetic_model_dir
    model = create_synthetic_model_dir(str(tmp_path / "speech_small"), "SPEECH", **SMALL)
    inv = MELInverter(model, conv_form="f23")
    sounds = [voice(0.5, rate, f0, 40 + ii) for ii, (_, rate, f0, _, _) in enumerate(FILES)]
    guide = voice(0.6, 24000, 210.0, 50)
    paths = [str(tmp_path / name) for name, *_ in FILES]
    for path, snd, (_, rate, *_) in zip(paths, sounds, FILES):
        wavfile.write(path, rate, snd)
    wavfile.write(str(tmp_path / "guide.wav"), 24000, guide)
    factors, formants = [ff[3] for ff in FILES], [ff[4] for ff in FILES]
    out = str(tmp_path / "job")
    os.makedirs(out)
    skipped = run_audio_job(inv, paths, out, "flac", factors=factors, noise_seed=SEED, batch=2, quiet=True,
                            flac_compression="fixed", out_rate=16000, stretches=STRETCH, formants=formants, f0_source="audio",
                            f0_decode=f0decode.decode_params(), f0_fill="hold",
                            guides=[str(tmp_path / "guide.wav"), None, None], align_band_s=0.25)
    assert skipped == [] and sorted(os.listdir(out)) == sorted("syn_" + name[:-4] + ".flac" for name, *_ in FILES)
    job = [open(os.path.join(out, "syn_" + name[:-4] + ".flac"), "rb").read() for name, *_ in FILES]
    assert len(set(job)) == 3 and all(len(data) > 1000 for data in job)
    if not have_soundfile():                                 # the built-in writer: the device encoder's bytes on both sides
        method = inv.transform_audio(sounds, [ff[1] for ff in FILES], [ff[0] for ff in FILES], transposition=factors,
                                     noise_seed=SEED, out_rate=16000, max_batch=2, flac=True, flac_compression="fixed",
                                     time_stretch=[None, 1.5, None], formant=formants, f0_source="audio",
                                     f0_decode=f0decode.decode_params(), f0_fill="hold",
                                     align_to=[(guide, 24000), None, None], align_band_s=0.25)
        for name, got, want in zip(paths, job, method):
            assert got == bytes(want), name
    # the tool, one file per launch: the lists carry the per-file factors
    for listing, values in (("factors.txt", factors), ("formants.txt", formants)):
        (tmp_path / listing).write_text("".join(f"{name} {value}\n" for (name, *_), value in zip(FILES, values)))
    guided, others = str(tmp_path / "tool_guided"), str(tmp_path / "tool_others")
    common = ["--model_id", model, "--conv-form", "f23", "--noise-seed", str(SEED), "--batch", "1", "-q", "--flac-compression",
              "fixed", "--out-rate", "16000", "--transposition-file", str(tmp_path / "factors.txt"), "--formant-shift-file",
              str(tmp_path / "formants.txt"), "--f0-source", "audio", "--pitch-decode", "viterbi", "--f0-fill", "hold"]
    (tmp_path / "stretch.txt").write_text("slow.wav 1.5\n")
    for args in ([paths[0], "-o", guided, "--align-to", str(tmp_path / "guide.wav"), "--align-band", "0.25"],
                 [*paths[1:], "-o", others, "--time-stretch-file", str(tmp_path / "stretch.txt")]):
        res = subprocess.run([sys.executable, os.path.join(BIN, "transform_audio.py"), *args, *common], capture_output=True,
                             text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-3000:]
    for (name, *_), want, where in zip(FILES, job, (guided, others, others)):
        assert open(os.path.join(where, "syn_" + name[:-4] + ".flac"), "rb").read() == want, name

"""The file-to-file tool's host side (no GPU needed): argument handling of transform_audio.py and of the new resynth_mel.py and
stream_transpose.py flags, the transposition list, the rank plan of a --gpus job and the refusals of the keyed-noise
arguments of MELInverter."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")


def load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(BIN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_script(name, args):
    return subprocess.run([sys.executable, os.path.join(BIN, name + ".py"), *args], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def tool():
    return load_script("transform_audio")


def test_parser_defaults_and_flags(tool):
    args = tool.make_parser().parse_args(["a.wav", "b.flac", "-o", "out"])
    assert args.input_audio_files == ["a.wav", "b.flac"] and args.output_dir == "out" and args.model_id == "VOICE"
    assert args.transposition == 1.0 and args.transposition_file is None and args.noise_seed == 0
    assert args.batch == 16 and args.gpus == 1 and args.num_threads == 2 and args.out_rate is None
    assert args.format == "flac" and args.flac_compression == "verbatim" and args.conv_form == "auto"
    assert not args.batch_invariant and not args.verbose and not args.quiet and args.rank is None and args.job is None
    args = tool.make_parser().parse_args(["a.wav", "-o", "out", "--model_id", "m", "--transposition", "1.5", "--transposition-file",
                                          "t.txt", "--noise-seed", "7", "--batch", "4", "--gpus", "2", "-nt", "3", "--out-rate",
                                          "input", "--format", "wav", "--flac-compression", "fixed", "--conv-form", "f23",
                                          "--batch-invariant", "-v", "-q"])
    assert (args.transposition, args.transposition_file, args.noise_seed, args.batch, args.gpus, args.num_threads) == \
        (1.5, "t.txt", 7, 4, 2, 3)
    assert (args.out_rate, args.format, args.flac_compression, args.conv_form) == ("input", "wav", "fixed", "f23")
    assert args.batch_invariant and args.verbose and args.quiet
    assert tool.make_parser().parse_args(["a.wav", "-o", "o", "--out-rate", "16000"]).out_rate == 16000
    # every parsed name is an argument of main
    import inspect
    assert set(vars(args)) == set(inspect.signature(tool.main).parameters)


@pytest.mark.parametrize("flag,value", [("--transposition", "0"), ("--transposition", "-2"), ("--transposition", "nan"),
                                         ("--transposition", "inf"), ("--transposition", "x"), ("--out-rate", "0"),
                                         ("--out-rate", "fast"), ("--conv-form", "f99"), ("--flac-compression", "lpc")])
def test_parser_refuses(tool, flag, value, capsys):
    with pytest.raises(SystemExit) as exc:
        tool.make_parser().parse_args(["a.wav", "-o", "out", flag, value])
    assert exc.value.code == 2
    assert flag in capsys.readouterr().err


def test_transposition_file(tmp_path):
    from mbexwn_vocoder_amd.batched import file_factors, read_transposition_file
    path = tmp_path / "factors.txt"
    path.write_text("# per file\na.wav 1.5\n\n  dir/b.flac   0.5   # an octave down\nc.wav 2\n")
    table = read_transposition_file(str(path))
    assert table == {"a.wav": 1.5, "b.flac": 0.5, "c.wav": 2.0}
    files = ["/x/a.wav", "b.flac", "y/d.wav", "c.wav"]
    assert file_factors(files, 1.25, table) == [1.5, 0.5, 1.25, 2.0]
    assert file_factors(files) == [1.0] * 4 and file_factors(files, 3) == [3.0] * 4
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite and positive"):
            file_factors(files, bad)
    for text, what in (("a.wav 0\n", "finite and positive"), ("a.wav -1.5\n", "finite and positive"), ("a.wav nan\n", "finite"),
                       ("a.wav\n", "basename factor"), ("a.wav 1 2\n", "basename factor"), ("a.wav fast\n", "float"),
                       ("a.wav 1\nx/a.wav 2\n", "twice")):
        path.write_text("b.wav 1\n" + text)
        with pytest.raises(ValueError, match=what) as exc:
            read_transposition_file(str(path))
        assert f"{path}:{2 + text.count(chr(10)) - 1}:" in str(exc.value)          # the line is named


def test_tool_refuses_bad_jobs_before_any_gpu_call(tmp_path):
    """A bad list, a missing file and two files with one basename end the tool with status 1 and a message, before torch."""
    from scipy.io import wavfile
    aa, bb = tmp_path / "a.wav", tmp_path / "sub" / "a.wav"
    os.makedirs(bb.parent)
    for path in (aa, bb):
        wavfile.write(str(path), 24000, np.zeros(100, dtype=np.float32))
    bad = tmp_path / "factors.txt"
    bad.write_text("a.wav 0\n")
    out = str(tmp_path / "out")
    res = run_script("transform_audio", [str(aa), "-o", out, "--transposition-file", str(bad)])
    assert res.returncode == 1 and "finite and positive" in res.stderr and "factors.txt:1" in res.stderr
    res = run_script("transform_audio", [str(aa), "-o", out, "--transposition-file", str(tmp_path / "none.txt")])
    assert res.returncode == 1 and "none.txt" in res.stderr
    res = run_script("transform_audio", [str(aa), str(tmp_path / "missing.wav"), "-o", out])
    assert res.returncode == 1 and "no such file" in res.stderr and "missing.wav" in res.stderr
    res = run_script("transform_audio", [str(aa), str(bb), "-o", out])
    assert res.returncode == 1 and "share a basename" in res.stderr
    assert not os.path.exists(out)


def test_rank_plan_skips_bad_files_without_torch(tmp_path):
    """The parent of `transform_audio.py --gpus N` reads the files, skips an empty and a stereo one by name and partitions the
    others by duration -- without importing torch."""
    from scipy.io import wavfile
    names = []
    for name, data, rate in (("long.wav", np.zeros(48000, np.float32), 24000), ("empty.wav", np.zeros(0, np.float32), 24000),
                             ("short.wav", np.zeros(4410, np.float32), 44100), ("stereo.wav", np.zeros((100, 2), np.float32), 24000),
                             ("mid.wav", np.zeros(24000, np.float32), 24000)):
        names.append(str(tmp_path / name))
        wavfile.write(names[-1], rate, data)
    code = ("import json, sys; sys.path.insert(0, sys.argv[1]);"
            "from mbexwn_vocoder_amd.batched import plan_audio_ranks;"
            "plan = plan_audio_ranks(sys.argv[2:], 2);"
            "assert 'torch' not in sys.modules; print(json.dumps(plan))")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0,1,2")
    res = subprocess.run([sys.executable, "-c", code, ROOT, *names], capture_output=True, text=True, env=env, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    import json
    plan = json.loads(res.stdout.strip().splitlines()[-1])
    assert plan["devices"] == 3
    assert [os.path.basename(ff) for ff in plan["files"]] == ["long.wav", "short.wav", "mid.wav"]
    assert plan["shards"] == [[0], [2, 1]]                    # 2 s | 1 s + 0.1 s
    skipped = {os.path.basename(ff): why for ff, why in plan["skipped"]}
    assert set(skipped) == {"empty.wav", "stereo.wav"}
    assert "no samples" in skipped["empty.wav"] and "channels" in skipped["stereo.wav"]


def test_noise_and_noise_seed_exclude_each_other(tmp_path):
    from mbexwn_vocoder_amd.mel_inverter import MELInverter, check_factors, create_synthetic_model_dir
    model = create_synthetic_model_dir(str(tmp_path / "model"), "SPEECH")
    inv = MELInverter.host_only(model)
    mel = np.zeros((1, 4, 80), dtype=np.float32)
    with pytest.raises(ValueError, match="exclude each other"):
        inv.synth_from_mel(mel, noise=np.zeros((1, 4 * 20), dtype=np.float32), noise_seed=3)
    with pytest.raises(ValueError, match="exclude each other"):
        inv.synth_from_mels([mel], noises=[np.zeros(80, dtype=np.float32)], noise_seed=3)
    with pytest.raises(ValueError, match="needs noise_seed"):
        inv.synth_from_mels([mel], noise_keys=[1])
    assert check_factors(1.5, 3) == [1.5] * 3 and check_factors([1, 2], 2) == [1.0, 2.0]
    for bad in (0, [1, -1], float("nan"), [1, 2, 3]):
        with pytest.raises(ValueError):
            check_factors(bad, 2)
    with pytest.raises(ValueError, match="finite and positive"):
        inv.transform_audio([np.zeros(10, np.float32)], [24000], ["a.wav"], transposition=0)


def test_resynth_mel_flags():
    res = run_script("resynth_mel", ["--help"])
    assert res.returncode == 0 and "--noise-seed" in res.stdout and "--transposition" in res.stdout
    for value in ("0", "-1", "nan", "x"):
        res = run_script("resynth_mel", ["model", "-i", "a.mell", "--transposition", value])
        assert res.returncode == 2 and "--transposition" in res.stderr, value
    res = run_script("resynth_mel", ["model", "-i", "a.mell", "--noise-seed", "x"])
    assert res.returncode == 2 and "--noise-seed" in res.stderr
    import inspect
    params = inspect.signature(load_script("resynth_mel").main).parameters
    assert params["noise_seed"].default is None and params["transposition"].default is None


def test_stream_transpose_flag():
    res = run_script("stream_transpose", ["--help"])
    assert res.returncode == 0 and "--noise-seed" in res.stdout
    import inspect
    mod = load_script("stream_transpose")
    assert inspect.signature(mod.main).parameters["noise_seed"].default is None
    assert inspect.signature(mod.stream_file).parameters["noise_fn"].default is None
    from mbexwn_vocoder_amd.live import keyed_noise_fn

    class Engine:                                            # records what the stream's noise function asks the engine for
        class dims:
            steps_per_frame = 20

        def keyed_noise(self, seed, keys, counts, first_step=None):
            import torch
            self.asked = (seed, keys, counts, first_step)
            return torch.zeros((1, counts[0]))

    from mbexwn_vocoder_amd.noise import item_key
    eng = Engine()
    fn = keyed_noise_fn(eng, 7)
    assert fn("a.wav", 6, 13).shape == (140,) and eng.asked == (7, [item_key("a.wav")], [140], [120])
    assert fn(5, 0, 6).shape == (120,) and eng.asked == (7, [5], [120], [0])
    assert fn(5, 6, 6).shape == (0,)

"""The device resampler (csrc/resample_poly.hip through mbxa_resample_poly, include/mbexwn_audio.h) against the float64
evaluation of its definition and the reference's own run; its memory contract between guard bands (the guard-band case of
this export lives here: the export list of mbexwn.h, which tests/test_gpu_memory_contract.py covers, does not hold it);
bin/generate_mel.py end to end on the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import resample_reference as rr
from guarded import FILLS, GuardSet, fill_word

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATE = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin", "generate_mel.py")
RESYNTH = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin", "resynth_mel.py")
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 3}
# beyond the fixture: the two launches whose input span does not fit the LDS budget (float64 evaluation only) --
# decimation by 8 with the taps in LDS, and an odd rate whose 2.9 M taps stay in global memory as well
EXTRA = ((192000, 9000), (200001, 10000))


def design(in_sr):
    from mbexwn_vocoder_amd import resample
    taps, up, down = resample.reference_filter(in_sr, rr.OUT_SR)
    return resample.scaled_taps(taps, up), up, down


def run_batch(items, in_sr, max_samples=None):
    """One ragged launch through resample_device; returns the items' outputs (numpy) trimmed to n_out."""
    import torch
    from mbexwn_vocoder_amd import resample
    lengths = [xx.size for xx in items]
    host = np.zeros((len(items), max_samples or max(lengths)), dtype=np.float32)
    for bb, xx in enumerate(items):
        host[bb, :xx.size] = xx
    out, n_out = resample.resample_device(torch.as_tensor(host).cuda(), torch.as_tensor(lengths, dtype=torch.int32).cuda(),
                                          in_sr, rr.OUT_SR)
    _, up, down = design(in_sr)
    assert out.shape == (len(items), -(-host.shape[1] * up // down)) and out.dtype == torch.float32
    assert n_out.dtype == torch.int32 and n_out.is_cuda and n_out.cpu().tolist() == [-(-nn * up // down) for nn in lengths]
    got = out.cpu().numpy()
    return [got[bb, :-(-nn * up // down)].copy() for bb, nn in enumerate(lengths)]


@pytest.mark.parametrize("in_sr", sorted({sr for sr, _ in rr.CASES + EXTRA}))
def test_parity_with_the_definition_and_the_reference(in_sr):
    """One ragged launch per ratio: the fixture's cases of that ratio plus two seeded items of lengths 1 and n // 2.  Every
    output within B[k] of the float64 evaluation and within 2 B[k] of the reference's own float32 run.  Between them the
    ratios cover up = 1, down = 1, decimation by 4, the LDS table at 57.6 KB (11025 Hz), the global-memory table (12345 Hz)
    and the input span read from global memory (EXTRA)."""
    fx = rr.fixture()
    g, up, down = design(in_sr)
    rng = np.random.default_rng(in_sr)
    lengths = [nn for sr, nn in rr.CASES + EXTRA if sr == in_sr]
    items = [fx[f"sr{in_sr}_n{nn}/x"] if (in_sr, nn) in rr.CASES else rng.standard_normal(nn).astype(np.float32) for nn in lengths]
    items += [rng.standard_normal(nn).astype(np.float32) for nn in (1, max(1, max(lengths) // 2))]
    got = run_batch(items, in_sr)
    for xx, yy in zip(items, got):
        y64, bound = rr.evaluate_all(g, up, down, xx)
        assert yy.shape == y64.shape
        ratio = np.max(np.abs(yy - y64) / bound)
        print(f"{in_sr} Hz, n = {xx.size}: max |y - y64| / B = {ratio:.3f}")
        assert np.all(np.abs(yy - y64) <= bound), f"{in_sr} Hz, n = {xx.size}: {ratio:.3f} B"
    for nn, yy in zip(lengths, got):
        if (in_sr, nn) in rr.CASES:
            _, bound = rr.evaluate_all(g, up, down, fx[f"sr{in_sr}_n{nn}/x"])
            assert np.all(np.abs(yy - fx[f"sr{in_sr}_n{nn}/y"]) <= 2 * bound)


def length_for(n_out, up, down):
    """The longest input whose output length does not exceed n_out (equal to it whenever some input reaches it)."""
    return n_out * down // up


@pytest.mark.parametrize("in_sr", [44100, 16000])
def test_same_bits_alone_and_in_company(in_sr):
    """Outputs of DEVICE_TILE - 1, DEVICE_TILE, DEVICE_TILE + 1 and 2 DEVICE_TILE + 1 samples: an item alone and the same
    item inside a ragged batch with a larger max_samples give the same bits.  (At 16000 Hz the output length is ceil(1.5 n):
    1024 is no such number, and the case lands on 1023 again; 1023, 1025 and 2049 are reached.)"""
    from mbexwn_vocoder_amd.resample import DEVICE_TILE
    _, up, down = design(in_sr)
    rng = np.random.default_rng(in_sr + 1)
    reached = set()
    for target in (DEVICE_TILE - 1, DEVICE_TILE, DEVICE_TILE + 1, 2 * DEVICE_TILE + 1):
        nn = length_for(target, up, down)
        reached.add(-(-nn * up // down))
        item = rng.standard_normal(nn).astype(np.float32)
        alone = run_batch([item], in_sr)[0]
        others = [rng.standard_normal(mm).astype(np.float32) for mm in (nn + 977, 5, nn // 3)]
        company = run_batch(others[:2] + [item] + others[2:], in_sr, max_samples=nn + 2000)[2]
        assert alone.size == -(-nn * up // down) and np.array_equal(alone, company), f"{in_sr} Hz, n = {nn}"
    want = {DEVICE_TILE - 1, DEVICE_TILE, DEVICE_TILE + 1, 2 * DEVICE_TILE + 1}
    assert reached == want if in_sr == 44100 else reached == want - {DEVICE_TILE}


def call(lib, audio, n_samples, batch, max_samples, up, down, taps, n_taps, out, max_out):
    import torch
    return lib.mbxa_resample_poly(audio, n_samples, batch, max_samples, up, down, taps, n_taps, out, max_out,
                                  torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("fill", FILLS)
def test_memory_contract_between_guard_bands(fill):
    """audio, n_samples, taps and out between guard bands, each payload exactly the size the header states.  Ragged lengths
    with an empty and a one-sample item, then lengths -5 and 10^6, which must act as 0 and max_samples.  Both guards of every
    buffer unchanged; every word of out behind an item's n_out still the fill; what is written is the definition."""
    import torch
    from mbexwn_vocoder_amd.engine import load_library
    lib = load_library()
    in_sr, max_samples, batch = 44100, 5000, 5
    g, up, down = design(in_sr)
    max_out = -(-max_samples * up // down)
    rng = np.random.default_rng(77)
    full = rng.standard_normal((batch, max_samples)).astype(np.float32)
    word = fill_word(fill)
    for lengths, ragged in (([3001, 0, 1, 5000, 301], True), ([-5, 10 ** 6, 3001, 0, 1], False)):
        effective = [min(max(nn, 0), max_samples) for nn in lengths]
        host = full.copy()
        if ragged:                                     # behind an item's end its row holds the fill: a read there would show
            for bb, nn in enumerate(effective):
                host[bb, nn:].view(np.int32)[:] = word
        gs = GuardSet(fill, device="cuda")
        audio = gs.put("audio", host)
        n_dev = gs.put("n_samples", np.asarray(lengths, dtype=np.int32))
        taps = gs.put("taps", g)
        out = gs.new("out", batch * max_out * 4)
        status = call(lib, audio.ptr, n_dev.ptr, batch, max_samples, up, down, taps.ptr, g.size, out.ptr, max_out)
        torch.cuda.synchronize()
        assert status == 0, lib.mbx_last_error()
        gs.check()
        got = out.view(torch.float32, batch, max_out).cpu().numpy()
        for bb, nn in enumerate(effective):
            n_out = -(-nn * up // down)
            assert np.all(got[bb, n_out:].view(np.int32) == word), f"item {bb}: written behind its {n_out} outputs"
            if nn:
                y64, bound = rr.evaluate_all(g, up, down, full[bb, :nn])
                assert np.all(np.abs(got[bb, :n_out] - y64) <= bound), f"item {bb} (entry {lengths[bb]})"
        # the inputs are inputs
        assert np.array_equal(audio.view(torch.float32, batch, max_samples).cpu().numpy().view(np.int32), host.view(np.int32))
        assert n_dev.view(torch.int32).cpu().tolist() == lengths


def test_refusals_leave_out_untouched():
    """Every refusal of the header: status 1 and a message before any launch; out still holds its fill."""
    import torch
    from mbexwn_vocoder_amd.engine import load_library
    lib = load_library()
    g, up, down = design(48000)
    batch, max_samples = 2, 100
    max_out = -(-max_samples * up // down)
    gs = GuardSet("nan", device="cuda")
    audio = gs.put("audio", np.ones((batch, max_samples), dtype=np.float32))
    n_dev = gs.put("n_samples", np.asarray([100, 50], dtype=np.int32))
    taps = gs.put("taps", g)
    out = gs.new("out", batch * max_out * 4)
    good = dict(audio=audio.ptr, n_samples=n_dev.ptr, batch=batch, max_samples=max_samples, up=up, down=down, taps=taps.ptr,
                n_taps=g.size, out=out.ptr, max_out=max_out)
    bad = [dict(audio=None), dict(taps=None), dict(out=None), dict(batch=0), dict(up=0), dict(down=0), dict(n_taps=0),
           dict(batch=-1), dict(max_out=max_out - 1), dict(max_samples=-1)]
    for change in bad:
        status = call(lib, **dict(good, **change))
        message = lib.mbx_last_error().decode()
        assert status == 1 and message.startswith("resample poly:") and len(message) > 16, (change, status, message)
        torch.cuda.synchronize()
        assert out.payload_untouched(), change
        gs.check()
    # n_samples may be NULL: every item has max_samples
    assert call(lib, **dict(good, n_samples=None)) == 0
    torch.cuda.synchronize()
    gs.check()
    got = out.view(torch.float32, batch, max_out).cpu().numpy()
    y64, bound = rr.evaluate_all(g, up, down, np.ones(max_samples, dtype=np.float32))
    assert np.all(np.abs(got - y64[None]) <= bound[None])
    # the Python wrapper takes float32 cuda tensors only
    from mbexwn_vocoder_amd import resample
    with pytest.raises(ValueError):
        resample.resample_device(torch.zeros((2, 10), dtype=torch.float64).cuda(), None, 48000, 24000)


def test_indices_beyond_32_bits():
    """One item of 27 000 000 samples at 44100 Hz: (k + rem) * 147 passes 2^31 at k = 14.6 M.  The input is generated on the
    device from a seed; only the spans the checked outputs reach are copied back.  Outputs [14 608 000, 14 610 048) and the
    last 2 048 against the float64 evaluation of those outputs alone."""
    import torch
    from mbexwn_vocoder_amd import resample
    in_sr, n = 44100, 27_000_000
    g, up, down = design(in_sr)
    n_out = -(-n * up // down)
    assert 14_608_000 * down < 2 ** 31 < 14_610_048 * down and n_out > 14_610_048
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2024)
    x = torch.randn((1, n), generator=gen, device="cuda", dtype=torch.float32)
    out, n_dev = resample.resample_device(x, None, in_sr, rr.OUT_SR)
    assert out.shape == (1, n_out) and n_dev.cpu().tolist() == [n_out]
    half = (g.size - 1) // 2
    for k_lo, k_hi in ((14_608_000, 14_610_048), (n_out - 2048, n_out)):
        j_lo = max(0, (k_lo * down + half - g.size) // up - 1)
        j_hi = min(n, ((k_hi - 1) * down + half) // up + 2)
        span = x[0, j_lo:j_hi].cpu().numpy()
        y64, bound = rr.evaluate(g, up, down, span, n, np.arange(k_lo, k_hi), x_offset=j_lo)
        got = out[0, k_lo:k_hi].cpu().numpy()
        assert np.all(np.abs(got - y64) <= bound), f"outputs {k_lo} .. {k_hi}: {np.max(np.abs(got - y64) / bound):.3f} B"
        assert np.max(np.abs(y64)) > 0.1                           # real signal there, not zeros


# ---------------------------------------------------------------------------------------------------------------------
# the tool
# ---------------------------------------------------------------------------------------------------------------------
FILES = (("a24", 24000, 0.31), ("b44", 44100, 0.40), ("c44", 44100, 0.23), ("d48", 48000, 0.20), ("e16", 16000, 0.37))


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    return create_synthetic_model_dir(str(tmp_path_factory.mktemp("model") / "speech_small"), "SPEECH", **SMALL)


def run_tool(script, args, timeout=600):
    return subprocess.run([sys.executable, script, *args], capture_output=True, text=True, timeout=timeout)


@pytest.fixture(scope="module")
def tool_runs(model_dir, tmp_path_factory):
    """Five wav files (0.3 sin + 0.05 noise, the signal of test_gpu_dropin's analysis test) through the tool three times:
    --batch 4, --batch 1 and --host.  Returns {run: {name: mell dict}} and the directory."""
    from scipy.io import wavfile
    from mbexwn_vocoder_amd.fileio import load_var
    root = tmp_path_factory.mktemp("tool")
    rng = np.random.default_rng(17)
    files = []
    for ii, (name, rate, seconds) in enumerate(FILES):
        nn = int(seconds * rate) + ii
        tt = np.arange(nn) / rate
        snd = (0.3 * np.sin(2 * np.pi * (110.0 * (ii + 1)) * tt) + 0.05 * rng.normal(size=nn)).astype(np.float32)
        files.append(str(root / f"{name}.wav"))
        wavfile.write(files[-1], rate, snd)
    runs = {}
    for run, extra in (("batch4", ["--batch", "4"]), ("batch1", ["--batch", "1"]), ("host", ["--host"])):
        out = str(root / run)
        res = run_tool(GENERATE, [*files, "-o", out, "--model_id", model_dir, *extra])
        assert res.returncode == 0, res.stderr[-3000:]
        assert sorted(os.listdir(out)) == sorted(f"{name}.mell" for name, _, _ in FILES)
        runs[run] = {name: load_var(os.path.join(out, f"{name}.mell")) for name, _, _ in FILES}
    return runs, root


def test_tool_batched_equals_one_at_a_time_and_matches_the_host(tool_runs):
    """--batch 4 and --batch 1 write the same bits.  Against --host the amplitudes agree within 2e-5 of the item's largest
    (the bar of the device analysis against the host analysis, test_gpu_dropin.py); the log-domain bar of that test, 2e-3, is
    held by the files at or above 24000 Hz only: an upsampled file has empty bands at the filter's -70 dB floor, where
    float32 rounding alone moves the logarithm by up to 9e-3."""
    runs, _ = tool_runs
    for name, rate, _ in FILES:
        b4, b1, host = (runs[run][name] for run in ("batch4", "batch1", "host"))
        assert list(b4) == list(b1) == list(host)
        assert all(b4[kk] == host[kk] for kk in b4 if kk != "mell")
        assert b4["mell"].dtype == np.float32 and b4["mell"].shape == host["mell"].shape
        assert np.array_equal(b4["mell"], b1["mell"]), name
        err = np.abs(np.exp(b4["mell"]) - np.exp(host["mell"]))
        print(f"{name}: amplitude error {np.max(err) / np.max(np.exp(host['mell'])):.2e} of the maximum, log error "
              f"{np.max(np.abs(b4['mell'] - host['mell'])):.2e}")
        assert np.max(err) <= 2e-5 * np.max(np.exp(host["mell"])), name
        if rate >= 24000:
            assert np.max(np.abs(b4["mell"] - host["mell"])) <= 2e-3, name


def test_round_trip_through_resynth_mel(tool_runs, model_dir):
    """The .mell of a 44100 Hz file goes through resynth_mel.py: finite audio of frames * hop samples; without soundfile the
    .flac it writes goes back through generate_mel.py and gives len // hop + 1 frames."""
    from mbexwn_vocoder_amd.audioio import read_audio
    from mbexwn_vocoder_amd.fileio import load_var
    runs, root = tool_runs
    frames = runs["batch4"]["b44"]["mell"].shape[1]
    syn = str(root / "syn")
    res = run_tool(RESYNTH, [model_dir, "-i", str(root / "batch4" / "b44.mell"), "-o", syn, "-q"])
    assert res.returncode == 0, res.stderr[-3000:]
    audio, rate = read_audio(os.path.join(syn, "syn_b44.flac"))
    assert rate == 24000 and audio.shape == (frames * 300,) and np.all(np.isfinite(audio))
    try:
        import soundfile  # noqa: F401
        return                                                  # its FLAC is compressed: not the built-in reader's ground
    except ImportError:
        pass
    again = str(root / "again")
    res = run_tool(GENERATE, [os.path.join(syn, "syn_b44.flac"), "-o", again, "--model_id", model_dir, "-q"])
    assert res.returncode == 0, res.stderr[-3000:]
    assert load_var(os.path.join(again, "syn_b44.mell"))["mell"].shape == (80, audio.size // 300 + 1)


def test_python_routes_on_the_device_equal_the_tool(tool_runs, model_dir):
    """analysis.generate_mels(on_device=True) and MELInverter.generate_mel_from_snd(on_device=True, resampler="reference")
    are the tool's device path: same bits, whatever the micro-batch."""
    from mbexwn_vocoder_amd.analysis import generate_mels
    from mbexwn_vocoder_amd.audioio import read_audio
    from mbexwn_vocoder_amd.config import read_config
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    runs, root = tool_runs
    pre = read_config(os.path.join(model_dir, "config.yaml"))["preprocess_config"]
    sounds = [read_audio(str(root / f"{name}.wav")) for name, _, _ in FILES]
    dicts = generate_mels([ss for ss, _ in sounds], [rate for _, rate in sounds], pre, on_device=True, batch=3)
    for (name, _, _), dd in zip(FILES, dicts):
        assert np.array_equal(dd["mell"], runs["batch1"][name]["mell"]), name
    inv = MELInverter(None)                                    # no model: the method reads the pre-processing configuration
    inv.preprocess_config, inv._srate = pre, pre["sample_rate"]
    got = inv.generate_mel_from_snd(sounds[1][0], sounds[1][1], on_device=True, resampler="reference")
    assert list(got) == list(runs["batch1"]["b44"]) and np.array_equal(got["mell"], runs["batch1"]["b44"]["mell"])

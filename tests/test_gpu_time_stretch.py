"""Time stretching on the GPU: mbxw_mel_frames_at (csrc/mel_warp.hip) against the regular analysis kernel, bit for bit -- no
tolerance: tests/test_gpu_frontend_stages.py holds that kernel to the float64 reference, and a warped row is required to carry
the bits of the regular kernel's row for a frame with the same samples in front of it --, its memory contract and refusals,
and the stretch through generate_mels, MELInverter.transform_audio, run_audio_job and the command-line tools."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import frontend_reference as fr
from guarded import Guarded
from mbexwn_vocoder_amd import analysis, timemap

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")
EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def torch():
    import torch as tt
    return tt


def dev(torch, arr):
    return torch.as_tensor(np.ascontiguousarray(arr)).cuda()


def bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float32).view(np.uint32)


def table(rows, fill=0):
    """Ragged integer rows -> ((B, longest) int64, counts int32)."""
    out = np.full((len(rows), max(len(rr) for rr in rows)), fill, dtype=np.int64)
    for ii, rr in enumerate(rows):
        out[ii, :len(rr)] = rr
    return out, np.asarray([len(rr) for rr in rows], dtype=np.int32)


def frames_at(torch, cfg, sound, lengths, centres, counts):
    out, rate = analysis.compute_log_mel_device_at(dev(torch, sound), dev(torch, np.asarray(lengths, np.int32)),
                                                   dev(torch, np.asarray(centres, np.int64)),
                                                   dev(torch, np.asarray(counts, np.int32)), cfg)
    assert rate == cfg["sample_rate"] / cfg["hop_size"]
    return out.cpu().numpy()


def regular(torch, cfg, sound, lengths):
    out, _ = analysis.compute_log_mel_device(dev(torch, sound), cfg, n_samples=dev(torch, np.asarray(lengths, np.int32)))
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def launches(torch):
    """Per geometry: the ragged items of fr.mel_items and the regular kernel's output on them, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            cfg = fr.MEL_GEOMETRIES[name]
            sound, lengths, labels = fr.mel_items(cfg)
            cache[name] = (cfg, sound, lengths, labels, regular(torch, cfg, sound, lengths))
        return cache[name]
    return get


# ------------------------------------------------------------------------------------------------------------------------
# 1. regular centres
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["12_4_16_5", "800_200_1024_80_16k", "1200_300_2048_80"])
def test_regular_centres_give_the_regular_kernels_bits(torch, launches, name):
    cfg, sound, lengths, labels, want = launches(name)
    win, hop = cfg["win_size"], cfg["hop_size"]
    assert {0, 1, 2} <= set(lengths) and any(0 < nn < win // 2 for nn in lengths)
    assert any(nn % hop == 0 and nn > win for nn in lengths)                 # a last centre that equals n
    centres, counts = table([timemap.centres(nn, hop, cfg["sample_rate"], None) for nn in lengths])
    assert np.array_equal(counts, [nn // hop + 1 for nn in lengths]) and centres.shape[1] == want.shape[1]
    got = frames_at(torch, cfg, sound, lengths, centres, counts)
    assert got.shape == want.shape
    for ii, (nn, label) in enumerate(zip(lengths, labels)):
        rows = nn // hop + 1
        assert np.array_equal(bits(got[ii, :rows]), bits(want[ii, :rows])), (ii, label, nn)
        assert not got[ii, rows:].any()                                      # not written: the zeros of the allocation
    silent = labels.index("silence")
    empty = lengths.index(0)
    floor = np.float32(np.log(np.float64(np.float32(EPS))))
    assert np.all(got[empty, :1] == floor) and np.all(got[silent, :lengths[silent] // hop + 1] == floor)


# ------------------------------------------------------------------------------------------------------------------------
# 2. arbitrary centres against the regular kernel on an explicitly padded sound
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["12_4_16_5", "1200_300_2048_80"])
def test_arbitrary_centres_equal_interior_frames_of_the_padded_sound(torch, launches, name):
    """Centre c of item x: y = pad(x, (PL, win), "reflect") with PL = win//2 + ((-(win//2 + c)) % hop); frame (PL + c) / hop
    of y starts at sample c - win//2 of the reflect-padded x and lies inside y, so the regular kernel reads no padding of
    its own there."""
    cfg, sound, lengths, labels, _ = launches(name)
    win, hop = cfg["win_size"], cfg["hop_size"]
    above = min(nn for nn, label in zip(lengths, labels) if nn > win and label != "silence")
    picked = [lengths.index(nn) for nn in (1, 2, win // 2 - 1, win // 2 + 1, above, max(lengths))]
    rows_c, padded, frame_of = [], [], []
    for ii in picked:
        nn = lengths[ii]
        cc = [min(max(c, 0), nn) for c in (0, 1, hop - 1, hop + 1, nn // 2, nn - 1, nn, nn // 2)]     # the last: a repeated centre
        rows_c.append(cc)
        for c in cc:
            lead = win // 2 + ((-(win // 2 + c)) % hop)
            yy = np.pad(sound[ii, :nn], (lead, win), mode="reflect")
            assert (lead + c) % hop == 0 and lead + c - win // 2 >= 0 and lead + c - win // 2 + win <= yy.size
            padded.append(yy)
            frame_of.append((lead + c) // hop)
    centres, counts = table(rows_c)
    got = frames_at(torch, cfg, sound[picked], [lengths[ii] for ii in picked], centres, counts)
    ysound = np.zeros((len(padded), max(yy.size for yy in padded)), np.float32)
    for jj, yy in enumerate(padded):
        ysound[jj, :yy.size] = yy
    want = regular(torch, cfg, ysound, [yy.size for yy in padded])            # one launch for all of them
    jj = 0
    for bb, ii in enumerate(picked):
        for kk, c in enumerate(rows_c[bb]):
            assert np.array_equal(bits(got[bb, kk]), bits(want[jj, frame_of[jj]])), (labels[ii], lengths[ii], c)
            jj += 1
        assert np.array_equal(bits(got[bb, 4]), bits(got[bb, 7]))            # the repeated centre repeats the row
    assert jj == len(padded) == 8 * len(picked)


# ------------------------------------------------------------------------------------------------------------------------
# 3. factor 2 end to end through generate_mels
# ------------------------------------------------------------------------------------------------------------------------
def tone(seed, n, rate):
    rng = np.random.default_rng(seed)
    tt = np.arange(n) / float(rate)
    return (0.3 * np.sin(2 * np.pi * 170.0 * tt) + 0.05 * rng.normal(size=n)).astype(np.float32)


def test_generate_mels_with_time_maps(torch):
    cfg = dict(fr.MEL_GEOMETRIES["1200_300_2048_80"], lin_amp_off=1e-5, lin_amp_scale=1, mel_amp_scale=1)
    hop = cfg["hop_size"]
    sounds = [tone(1, 9600, 24000), tone(2, 35280, 44100), tone(3, 28800, 24000)]        # 0.4 s, 0.8 s at 44.1 kHz, 1.2 s
    rates = [24000, 44100, 24000]
    plain = analysis.generate_mels(sounds, rates, cfg, on_device=True, batch=16)
    got = analysis.generate_mels(sounds, rates, cfg, on_device=True, batch=16, time_maps=[2.0, None, 0.5])
    single = analysis.generate_mels(sounds, rates, cfg, on_device=True, batch=1, time_maps=[2.0, None, 0.5])
    frames = [dd["mell"].shape[1] for dd in plain]
    assert frames[0] == 9600 // hop + 1 and frames[1] == analysis.resampled_length(35280, 44100, 24000) // hop + 1
    assert got[0]["mell"].shape[1] == 2 * 9600 // hop + 1 and got[2]["mell"].shape[1] == 28800 // (2 * hop) + 1
    assert np.array_equal(bits(got[0]["mell"][:, 0:2 * frames[0]:2]), bits(plain[0]["mell"]))    # even columns: the regular frames
    assert not np.array_equal(got[0]["mell"][:, 1], plain[0]["mell"][:, 0])
    assert got[1]["mell"].tobytes() == plain[1]["mell"].tobytes()                                # None: today's output
    assert np.array_equal(bits(got[2]["mell"]), bits(plain[2]["mell"][:, 0:2 * got[2]["mell"].shape[1]:2]))
    for aa, bb in zip(got, single):                                                              # batch 16 against batch 1
        assert aa["mell"].tobytes() == bb["mell"].tobytes() and list(aa) == list(bb)
    # the resampled sound stretched: its centres come from the resampled length, its even columns are the regular frames
    slow = analysis.generate_mels(sounds[1:2], rates[1:2], cfg, on_device=True, time_maps=[2.0])[0]["mell"]
    assert slow.shape[1] == 2 * analysis.resampled_length(35280, 44100, 24000) // hop + 1
    assert np.array_equal(bits(slow[:, 0:2 * frames[1]:2]), bits(plain[1]["mell"]))
    # an item without a map in a micro-batch with a warped one runs on its regular centres: the regular analysis's bits
    mixed = analysis.generate_mels(sounds, rates, cfg, on_device=True, time_maps=[2.0, None, None])
    assert mixed[2]["mell"].tobytes() == plain[2]["mell"].tobytes() and mixed[0]["mell"].tobytes() == got[0]["mell"].tobytes()
    # all entries None: the regular launches
    same = analysis.generate_mels(sounds, rates, cfg, on_device=True, time_maps=[None] * 3)
    assert [dd["mell"].tobytes() for dd in same] == [dd["mell"].tobytes() for dd in plain]


# ------------------------------------------------------------------------------------------------------------------------
# 4. memory contract, 5. refusals
# ------------------------------------------------------------------------------------------------------------------------
class Call:
    """One raw call of mbxw_mel_frames_at with its own buffers: the output between guard bands, pre-filled."""

    def __init__(self, torch, cfg, sound, lengths, centres, counts, fill="nan"):
        from mbexwn_vocoder_amd.engine import load_library
        self.torch, self.cfg, self.lib = torch, cfg, load_library()
        self.sound = dev(torch, np.asarray(sound, np.float32))
        self.lengths, self.counts = dev(torch, np.asarray(lengths, np.int32)), dev(torch, np.asarray(counts, np.int32))
        self.centres = dev(torch, np.asarray(centres, np.int64))
        self.tables = [dev(torch, tt) for tt in analysis.mel_analysis_tables(cfg)]
        self.batch, self.frames, self.mels = int(self.sound.shape[0]), int(self.centres.shape[1]), int(cfg["mel_channels"])
        self.out = Guarded("out", 4 * self.batch * self.frames * self.mels, fill, device="cuda")

    def run(self, **kw):
        cfg = self.cfg
        args = dict(audio=self.sound.data_ptr(), stride=int(self.sound.shape[1]), batch=self.batch, n_samples=self.lengths.data_ptr(),
                    centres=self.centres.data_ptr(), n_frames=self.counts.data_ptr(), max_frames=self.frames,
                    win=int(cfg["win_size"]), fft_size=int(cfg["fft_size"]), n_mels=self.mels, window=self.tables[0].data_ptr(),
                    twiddle=self.tables[1].data_ptr(), basis=self.tables[2].data_ptr(), bin_lo=self.tables[3].data_ptr(),
                    bin_hi=self.tables[4].data_ptr(), out=self.out.ptr)
        args.update(kw)
        status = self.lib.mbxw_mel_frames_at(args["audio"], args["stride"], args["batch"], args["n_samples"], args["centres"],
                                             args["n_frames"], args["max_frames"], args["win"], args["fft_size"], args["n_mels"],
                                             args["window"], args["twiddle"], args["basis"], args["bin_lo"], args["bin_hi"],
                                             ctypes.c_float(EPS), args["out"], None)
        self.torch.cuda.synchronize()
        return status

    def result(self):
        return self.out.view(self.torch.float32, self.batch, self.frames, self.mels).cpu().numpy()


@pytest.mark.parametrize("name", ["12_4_16_5", "1200_300_2048_80"])
def test_memory_contract(torch, launches, name):
    cfg, sound, lengths, labels, want = launches(name)
    hop, nmax = cfg["hop_size"], sound.shape[1]
    rows = [timemap.centres(nn, hop, cfg["sample_rate"], None) for nn in lengths]
    centres, counts = table(rows, fill=nmax // 2)                        # entries behind a row's count: valid, and unused
    for fill, pad in (("nan", 0.0), ("huge", 1e30), ("zero", np.nan)):
        snd = sound.copy()
        for ii, nn in enumerate(lengths):
            snd[ii, nn:] = pad                                           # behind every item's end
        call = Call(torch, cfg, snd, lengths, centres, counts, fill=fill)
        assert call.run() == 0
        call.out.check()                                                 # the guards around out keep the pattern
        raw = call.out.view(torch.int32, call.batch, call.frames, call.mels).cpu().numpy()
        got = call.result()
        word = {"nan": -1, "huge": int(np.float32(1e30).view(np.int32)), "zero": 0}[fill]
        for ii in range(call.batch):
            assert np.array_equal(bits(got[ii, :counts[ii]]), bits(want[ii, :counts[ii]])), (fill, labels[ii])
            assert np.all(raw[ii, counts[ii]:] == word), (fill, labels[ii])              # rows k >= n_frames[b]: the pattern
    # wrong table entries are clamped, not followed: centres of -5 and n + 1000 are the rows of 0 and n; n_samples of -3 and
    # stride + 10 behave as 0 and stride; a count above max_frames and a negative one write max_frames rows and none
    longest, third = 0, lengths.index(2)
    nn = lengths[longest]
    assert nn == nmax
    snd = np.stack((sound[longest], sound[longest], sound[longest], sound[third]))
    cc = np.array([[-5, 0, nn + 1000, nn], [0, hop, nn, -5], [0, hop, nn, nn + 1000], [-5, 0, 2 + 1000, 2]], dtype=np.int64)
    call = Call(torch, cfg, snd, [nn, -3, nmax + 10, 2], cc, [4, 4, 4 + 3, 4])
    assert call.run() == 0
    call.out.check()
    got = call.result()
    assert np.array_equal(bits(got[0, 0]), bits(got[0, 1])) and np.array_equal(bits(got[0, 2]), bits(got[0, 3]))
    assert np.array_equal(bits(got[0, 1]), bits(want[longest, 0]))
    assert np.array_equal(bits(got[3, 0]), bits(got[3, 1])) and np.array_equal(bits(got[3, 2]), bits(got[3, 3]))
    assert np.array_equal(bits(got[3, 1]), bits(want[third, 0]))
    floor = np.float32(np.log(np.float64(np.float32(EPS))))
    assert np.all(got[1] == floor)                                       # n_samples -3: an empty item
    ref = Call(torch, cfg, snd[2:3], [nmax], cc[2:3], [4])               # n_samples stride + 10: the whole row
    assert ref.run() == 0
    assert np.array_equal(bits(got[2]), bits(ref.result()[0]))
    assert np.array_equal(bits(got[2, :2]), bits(want[longest, :2]))
    none = Call(torch, cfg, snd[:1], [nn], cc[:1], [-2])
    assert none.run() == 0 and none.out.payload_untouched()
    none.out.check()


def test_refusals_leave_the_output_untouched(torch, launches):
    cfg, sound, lengths, _, _ = launches("12_4_16_5")
    centres, counts = table([timemap.centres(nn, cfg["hop_size"], cfg["sample_rate"], None) for nn in lengths])
    call = Call(torch, cfg, sound, lengths, centres, counts, fill="huge")

    def why():
        return call.lib.mbx_last_error().decode()

    cases = [({name: None}, "null") for name in ("audio", "n_samples", "centres", "n_frames", "window", "twiddle", "basis",
                                                  "bin_lo", "bin_hi", "out")]
    cases += [({"fft_size": 4}, "fft_size"), ({"fft_size": 4096}, "fft_size"), ({"fft_size": 24}, "fft_size"),
              ({"win": 1}, "win"), ({"win": 17}, "win"), ({"n_mels": 0}, "n_mels"), ({"max_frames": 0}, "max_frames"),
              ({"stride": 0}, "stride"), ({"batch": 65536}, "batch")]
    for kw, what in cases:
        assert call.run(**kw) == 1, kw                                   # MBX_ERR_INVALID_ARGUMENT
        assert why().startswith("mel frames at:") and what in why(), (kw, why())
        assert call.out.payload_untouched(), kw
        call.out.check()
    assert call.run(batch=0) == 0 and call.out.payload_untouched()       # nothing to do
    assert call.run() == 0 and not call.out.payload_untouched()          # and the same buffers do run


# ------------------------------------------------------------------------------------------------------------------------
# 6. the tool, on a small model
# ------------------------------------------------------------------------------------------------------------------------
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 5}
SEED = 7
# 0.3 s, 0.45 s at 44.1 kHz; the third file is only ever skipped
FILES = [("alto.wav", 7200, 24000, 1.5), ("basso.wav", 19845, 44100, 0.75), ("canto.wav", 4800, 24000, 1e9)]


def run_script(name, args):
    return subprocess.run([sys.executable, os.path.join(BIN, name + ".py"), *args], capture_output=True, text=True, timeout=600)


def read_dir(path):
    return {nn: open(os.path.join(path, nn), "rb").read() for nn in sorted(os.listdir(path))}


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    return create_synthetic_model_dir(str(tmp_path_factory.mktemp("model") / "speech_small"), "SPEECH", **SMALL)


@pytest.fixture(scope="module")
def inv(model_dir):
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    return MELInverter(model_dir, conv_form="f23")


@pytest.fixture(scope="module")
def wavs(tmp_path_factory):
    from scipy.io import wavfile
    root = tmp_path_factory.mktemp("sounds")
    sounds, files = [], []
    for ii, (name, nn, rate, _) in enumerate(FILES):
        sounds.append(tone(30 + ii, nn, rate))
        files.append(str(root / name))
        wavfile.write(files[-1], rate, sounds[-1])
    listing = root / "stretch.txt"
    listing.write_text("".join(f"{name} {factor}\n" for name, _, _, factor in FILES[:2]))
    return sounds, files, str(listing)


@pytest.fixture(scope="module")
def job(inv, wavs, tmp_path_factory):
    """run_audio_job on the first two files with their factors, batch 4: {name: bytes}, written once."""
    from mbexwn_vocoder_amd.batched import run_audio_job
    _, files, _ = wavs
    out = str(tmp_path_factory.mktemp("job"))
    skipped = run_audio_job(inv, files[:2], out, "flac", noise_seed=SEED, batch=4, quiet=True,
                            stretches=[ff[3] for ff in FILES[:2]])
    assert skipped == []
    return read_dir(out)


def test_job_without_stretch_and_with_factor_one_write_the_same_bytes(inv, wavs, tmp_path):
    from mbexwn_vocoder_amd.batched import run_audio_job
    _, files, _ = wavs
    outs = []
    for tag, stretches in (("none", None), ("ones", [1.0, 1.0])):
        out = str(tmp_path / tag)
        os.makedirs(out)
        assert run_audio_job(inv, files[:2], out, "flac", noise_seed=SEED, batch=4, quiet=True, stretches=stretches) == []
        outs.append(read_dir(out))
    assert sorted(outs[0]) == ["syn_alto.flac", "syn_basso.flac"] and outs[0] == outs[1]


def test_job_equals_the_library_routes_in_any_batch(inv, wavs, job, tmp_path):
    """A stretched file has K * hop samples for the K centres of the time map and decodes to the 16-bit samples of
    MELInverter.transform_audio(time_stretch=) and of the two-step route; batch 1 writes the bytes of batch 4."""
    from mbexwn_vocoder_amd import flac
    from mbexwn_vocoder_amd.audioio import read_audio
    from mbexwn_vocoder_amd.batched import run_audio_job
    from mbexwn_vocoder_amd.noise import item_key
    sounds, files, _ = wavs
    names, rates, factors = [ff[0] for ff in FILES[:2]], [ff[2] for ff in FILES[:2]], [ff[3] for ff in FILES[:2]]
    assert sorted(job) == ["syn_alto.flac", "syn_basso.flac"]
    whole = inv.transform_audio(sounds[:2], rates, names, noise_seed=SEED, time_stretch=factors)
    for ii, (name, nn, rate, factor) in enumerate(FILES[:2]):
        frames = len(timemap.centres(analysis.resampled_length(nn, rate, inv.srate), inv.hop_size, inv.srate, factor))
        path = str(tmp_path / ("syn_" + name.replace(".wav", ".flac")))
        with open(path, "wb") as fo:
            fo.write(job["syn_" + name.replace(".wav", ".flac")])
        got, got_rate = read_audio(path)
        assert got_rate == inv.srate and got.shape == (frames * inv.hop_size,), name
        assert whole[ii].shape == got.shape
        assert np.array_equal(got, flac.to_pcm16(whole[ii]).astype(np.float32) / np.float32(32768.0)), name
        alone = inv.transform_audio(sounds[ii:ii + 1], [rate], [name], noise_seed=SEED, time_stretch=factor)[0]
        assert np.array_equal(bits(alone), bits(whole[ii])), name
        # the two-step route; the rows of ones are the job's transposition factor of 1 on every frame
        scaled = inv.scale_mel(analysis.generate_mels([sounds[ii]], [rate], inv.preprocess_config, time_maps=[factor])[0])
        assert scaled.shape[1] == frames
        two = inv.synth_from_mel(scaled, noise_seed=SEED, noise_key=item_key(name),
                                 transposition=np.ones(frames, dtype=np.float32))
        assert np.array_equal(bits(two), bits(whole[ii])), name
    out = str(tmp_path / "one")
    os.makedirs(out)
    assert run_audio_job(inv, files[:2], out, "flac", noise_seed=SEED, batch=1, quiet=True, stretches=factors) == []
    assert read_dir(out) == job
    # a breakpoint map through the library call: 0.1 s at speed 1, then held for 0.1 s
    held = inv.transform_audio(sounds[:1], rates[:1], names[:1], noise_seed=SEED,
                               time_stretch=np.array([[0.0, 0.0], [0.1, 0.1], [0.2, 0.1]]))[0]
    assert held.shape == ((int(0.2 * inv.srate) // inv.hop_size + 1) * inv.hop_size,) and np.all(np.isfinite(held))
    with pytest.raises(ValueError, match="limit of"):
        inv.transform_audio(sounds[:1], rates[:1], names[:1], noise_seed=SEED, time_stretch=1e9)


@pytest.mark.timeout(600)
def test_cli_time_stretch_file_and_a_factor_beyond_the_limit(model_dir, wavs, job, tmp_path):
    """transform_audio.py --time-stretch-file with the two files' factors writes the job's bytes; the third file takes
    --time-stretch 1e9, is reported and skipped, and the exit status is 1."""
    _, files, listing = wavs
    out = str(tmp_path / "cli")
    res = run_script("transform_audio", [*files, "-o", out, "--model_id", model_dir, "--conv-form", "f23", "--noise-seed", str(SEED),
                                         "--time-stretch-file", listing, "--time-stretch", "1e9", "--batch", "2", "-v"])
    assert res.returncode == 1, res.stderr[-3000:]
    assert "skipped" in res.stderr and "canto.wav" in res.stderr and "frames" in res.stderr
    assert "time-stretched from" in res.stderr and "x real time" in res.stderr
    assert read_dir(out) == job


@pytest.mark.timeout(600)
def test_cli_generate_mel_then_resynth_mel_equals_transform_audio(model_dir, wavs, tmp_path):
    """generate_mel.py --time-stretch 2, then resynth_mel.py --noise-seed on its file, writes the bytes of transform_audio.py
    --time-stretch 2 --noise-seed on the sound.  The noise key of a file is its basename with the extension, so the .mell
    file goes to resynth_mel.py under the sound's name; --transposition 1.0 is the factor transform_audio.py applies."""
    from mbexwn_vocoder_amd.fileio import load_var
    _, files, _ = wavs
    common = ["--conv-form", "f23", "--noise-seed", str(SEED), "--batch", "2"]
    direct = str(tmp_path / "direct")
    res = run_script("transform_audio", [files[0], "-o", direct, "--model_id", model_dir, "--time-stretch", "2", *common])
    assert res.returncode == 0, res.stderr[-3000:]
    mells = str(tmp_path / "mells")
    res = run_script("generate_mel", [files[0], "-o", mells, "--model_id", model_dir, "--time-stretch", "2", "-q"])
    assert res.returncode == 0, res.stderr[-3000:]
    saved = load_var(os.path.join(mells, "alto.mell"))
    assert saved["mell"].shape == (80, 2 * 7200 // 300 + 1) and saved["hoplen"] == 300
    renamed = str(tmp_path / "renamed")
    os.makedirs(renamed)
    shutil.copy(os.path.join(mells, "alto.mell"), os.path.join(renamed, "alto.wav"))
    steps = str(tmp_path / "steps")
    res = run_script("resynth_mel", [model_dir, "-i", os.path.join(renamed, "alto.wav"), "-o", steps, "--transposition", "1.0",
                                     *common])
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(read_dir(direct)) == ["syn_alto.flac"] and read_dir(steps) == read_dir(direct)

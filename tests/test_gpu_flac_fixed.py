"""The compressing FLAC encoder on the GPU (mbxf_encode_flac16_fixed, csrc/flac_fixed.hip) against the host writer
flac.encode(..., compression="fixed"): bytes, frame lengths, samples, max |x|, the memory contract, and the way up to
synth_from_mels and resynth_mel.py --flac-compression."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from guarded import FILLS, GuardSet
from mbexwn_vocoder_amd import flac

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin", "resynth_mel.py")
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 3}
RATE = 24000
# the lengths of tests/test_flac_fixed_host.py (every block-size edge, an odd last block, a last block of 4096 / 2) plus 0
LENGTHS = [0, 1, 2, 3, 4, 5, 6, 15, 16, 17, 48, 4095, 4096, 4097, 3 * 4096 + 77, 4096 + 333, 4096 + 2048, 0]


def _signals():
    """name -> function of the sample count: float32 signal."""
    def tt(n):
        return np.arange(n) / RATE

    def harmonic(n):
        xx = sum(np.sin(2 * np.pi * 120 * kk * tt(n)) / kk for kk in range(1, 40))
        return 0.5 * xx / max(1e-9, float(np.max(np.abs(xx)))) if n else xx * 0.0

    def patchy(n):                                           # silent in some partitions, loud in others
        xx = np.random.default_rng(n + 5).uniform(-0.9, 0.9, n)
        xx[(np.arange(n) // 256) % 3 != 1] = 0.0
        return xx

    def minus_zero(n):                                       # a quiet sine whose every third sample is -0.0
        xx = 0.001 * np.sin(2 * np.pi * 300 * tt(n))
        xx[::3] = -0.0
        return xx

    table = {
        "sine": lambda n: 0.5 * np.sin(2 * np.pi * 440 * tt(n)),
        "harmonic": harmonic,
        "ramp": lambda n: (7.0 * np.arange(n) - 3000.0) / 32767.0,
        "silence": lambda n: np.zeros(n),
        "constant": lambda n: np.full(n, 0.25),
        "noise": lambda n: np.random.default_rng(n + 1).uniform(-1.0, 1.0, n),
        "small-noise": lambda n: 0.01 * np.random.default_rng(n + 2).standard_normal(n),
        "square": lambda n: np.where(np.arange(n) % 2 == 0, 1.0, -1.0),
        "clipping": lambda n: 1.7 * np.sin(2 * np.pi * 97 * tt(n)),
        "minus-zero": minus_zero,
        "patchy": patchy,
        "walk": lambda n: np.cumsum(np.random.default_rng(n + 3).integers(-40, 41, n)) / 32767.0,    # order 1 is the cheapest
        "slow-sine": lambda n: 0.9 * np.sin(2 * np.pi * 1500 * tt(n)),
    }
    return {name: (lambda n, fn=fn: np.asarray(fn(n), dtype=np.float32)) for name, fn in table.items()}


def _ragged_items():
    """35 (signal name, length): every length of LENGTHS once with the signals in turn, then every signal on lengths of more
    than one frame; ordered (seeded search) so that the frames of the packed batch start at every residue mod 16."""
    names = list(_signals())
    items = [(names[ii % len(names)], nn) for ii, nn in enumerate(LENGTHS)]
    longer = [4097, 3 * 4096 + 77, 4096, 4096 + 333, 4096 + 2048, 4095]
    items += [(names[(ii + 3) % len(names)], longer[ii % len(longer)]) for ii in range(35 - len(items))]
    return items


@pytest.fixture(scope="module")
def ragged():
    """The ragged batch and what the host writer makes of it: computed once, never changed."""
    sig = _signals()
    items = _ragged_items()
    assert len(items) == 35
    audio = [sig[name](nn) for name, nn in items]
    frames = [flac.fixed_frames(flac.to_pcm16(xx), RATE) for xx in audio]
    rng = np.random.default_rng(0)
    order = None
    for _ in range(200):
        cand = rng.permutation(len(items))
        starts = np.cumsum([0] + [len(ff) for ii in cand for ff in frames[ii]])[:-1]
        if len(set(int(ss) % 16 for ss in starts)) == 16:
            order = [int(ii) for ii in cand]
            break
    assert order is not None, "no order of the items gives every frame start residue mod 16"
    audio = [audio[ii] for ii in order]
    frames = [frames[ii] for ii in order]
    lengths = [xx.size for xx in audio]
    host = np.zeros((len(audio), max(lengths)), dtype=np.float32)
    for bb, xx in enumerate(audio):
        host[bb, :xx.size] = xx
    return {"host": host, "lengths": lengths, "frames": frames,
            "streams": [flac.encode(xx, RATE, compression="fixed") for xx in audio]}


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    return create_synthetic_model_dir(str(tmp_path_factory.mktemp("model") / "speech_small"), "SPEECH", **SMALL)


@pytest.fixture(scope="module")
def engine(model_dir):
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    return MELInverter(model_dir).model


def test_ragged_batch_matches_the_host_writer(engine, ragged):
    """35 items (more than one launch of 32), every block-size edge and every kind of signal: streams, frame lengths, samples
    and max |x| equal the host's."""
    import torch
    import re
    header = open(os.path.join(ROOT, "mbexwn_vocoder_amd", "csrc", "mbx_kernels.h")).read()
    FLAC_ITEMS_PER_LAUNCH = int(re.search(r"FLAC_ITEMS_PER_LAUNCH = (\d+);", header).group(1))
    host, lengths = ragged["host"], ragged["lengths"]
    assert len(lengths) > FLAC_ITEMS_PER_LAUNCH
    enc = engine.encode_flac16(torch.as_tensor(host, device=engine.device), lengths, sample_rate=RATE, compression="fixed")
    kinds = set()
    for bb, nn in enumerate(lengths):
        xx = host[bb, :nn]
        want = ragged["frames"][bb]
        assert [int(ll) for ll in enc.frame_lengths(bb)] == [len(ff) for ff in want], f"item {bb} ({nn} samples)"
        assert np.array_equal(enc.pcm(bb), flac.to_pcm16(xx)), f"item {bb} ({nn} samples)"
        assert enc.frames(bb).tobytes() == b"".join(want), f"item {bb} ({nn} samples)"
        assert enc.stream(bb) == ragged["streams"][bb], f"item {bb} ({nn} samples)"
        assert enc.max_abs[bb] == (np.max(np.abs(xx)) if nn else 0.0)
        kinds |= {flac.plan_fixed_frame(flac.to_pcm16(xx)[ss:ss + flac.BLOCK])[:2] for ss in range(0, nn, flac.BLOCK)}
    # the batch holds what it is meant to: every kind of sub-frame and every order
    assert kinds >= {("constant", None), ("verbatim", None)} | {("fixed", oo) for oo in range(5)}, kinds


@pytest.mark.parametrize("compression", flac.COMPRESSIONS)
def test_encode_device_needs_no_engine(compression):
    """flac.encode_device on its own (the library, no model): a ragged batch with an empty item, one sample, a full block and
    a block plus one sample at a stride of 4 100 -- every stream is the host writer's, byte for byte."""
    import torch
    lengths = (0, 1, 4096, 4097)
    host = (0.5 * np.random.default_rng(6).uniform(-1.0, 1.0, size=(len(lengths), 4100))).astype(np.float32)
    enc = flac.encode_device(torch.as_tensor(host).cuda(), lengths, RATE, compression=compression)
    assert isinstance(enc, flac.EncodedFlac) and enc.compression == compression
    for bb, nn in enumerate(lengths):
        assert enc.stream(bb) == flac.encode(host[bb, :nn], RATE, compression=compression), f"item {bb} ({nn} samples)"
        assert enc.max_abs[bb] == (np.max(np.abs(host[bb, :nn])) if nn else 0.0)


def test_other_rate_and_two_byte_frame_numbers(engine):
    """A rate outside FLAC's table (code 0000: taken from STREAMINFO) and an item of 129 frames, whose last frame numbers
    take two bytes."""
    import torch
    nn = 128 * 4096 + 1000
    xx = (0.5 * np.sin(2 * np.pi * 440 * np.arange(nn) / 12345)).astype(np.float32)
    enc = engine.encode_flac16(torch.as_tensor(xx[None], device=engine.device), [nn], sample_rate=12345, compression="fixed")
    assert len(enc.frame_lengths(0)) == 129
    assert enc.stream(0) == flac.encode(xx, 12345, compression="fixed")
    pcm, rate = flac.decode(enc.stream(0))
    assert rate == 12345 and np.array_equal(pcm, flac.to_pcm16(xx))


def test_nan_item_is_flagged_and_the_others_still_match(engine):
    import torch
    rng = np.random.default_rng(4)
    host = np.stack([0.1 * rng.standard_normal(5000), 0.1 * rng.standard_normal(5000), 0.1 * rng.standard_normal(5000)])
    host = host.astype(np.float32)
    host[1, 777] = np.nan
    enc = engine.encode_flac16(torch.as_tensor(host, device=engine.device), [5000, 5000, 4000], sample_rate=RATE,
                               compression="fixed")
    assert not np.isfinite(enc.max_abs[1])
    assert enc.stream(0) == flac.encode(host[0], RATE, compression="fixed")
    assert enc.stream(2) == flac.encode(host[2, :4000], RATE, compression="fixed")
    assert enc.max_abs[0] == np.max(np.abs(host[0])) and enc.max_abs[2] == np.max(np.abs(host[2, :4000]))


@pytest.mark.parametrize("fill", FILLS)
def test_the_call_stays_inside_its_buffers(engine, ragged, fill):
    """out (declared at the VERBATIM worst case), frame_bytes, workspace, pcm_out and max_abs between guard bands
    (tests/guarded.py): the guards are intact, and nothing behind the packed total is written in out."""
    import torch
    host, lengths = ragged["host"], ragged["lengths"]
    B, stride = host.shape
    frames = sum(-(-nn // flac.BLOCK) for nn in lengths)
    capacity = sum(flac.frames_bytes(nn) for nn in lengths)
    want = b"".join(ff for item in ragged["frames"] for ff in item)
    gs = GuardSet(fill, engine.device)
    ag = gs.put("audio", host)
    tg = gs.put("crc_tables", flac.crc16_device_tables())
    og, fg = gs.new("out", capacity), gs.new("frame_bytes", 4 * frames)
    wg, pg, mg = gs.new("workspace", 8 * (3 * frames + 1)), gs.new("pcm_out", 2 * B * stride), gs.new("max_abs", 4 * B)
    counts_c = (ctypes.c_int64 * B)(*lengths)
    with torch.cuda.device(engine.device):
        status = engine._lib.mbxf_encode_flac16_fixed(ag.ptr, stride, B, counts_c, RATE, tg.ptr, og.ptr, capacity, fg.ptr, wg.ptr,
                                                      pg.ptr, mg.ptr, engine._stream())
    assert status == 0, engine._lib.mbx_last_error().decode()
    torch.cuda.synchronize()
    gs.check()
    assert len(want) < capacity
    og.check(payload_bytes=len(want))                        # nothing behind the packed total
    assert og.payload.cpu().numpy()[:len(want)].tobytes() == want
    assert fg.view(torch.int32).cpu().tolist() == [len(ff) for item in ragged["frames"] for ff in item]
    offsets = wg.view(torch.int64).cpu().numpy()[:frames + 1]
    assert offsets[-1] == len(want) and np.array_equal(np.diff(offsets), fg.view(torch.int32).cpu().numpy())
    pcm = pg.view(torch.int16, B, stride).cpu().numpy()
    assert all(np.array_equal(pcm[bb, :nn], flac.to_pcm16(host[bb, :nn])) for bb, nn in enumerate(lengths))
    # without pcm_out the same frames
    og.refill()
    with torch.cuda.device(engine.device):
        status = engine._lib.mbxf_encode_flac16_fixed(ag.ptr, stride, B, counts_c, RATE, tg.ptr, og.ptr, capacity, fg.ptr, wg.ptr,
                                                      None, mg.ptr, engine._stream())
    assert status == 0
    torch.cuda.synchronize()
    gs.check()
    assert og.payload.cpu().numpy()[:len(want)].tobytes() == want


def test_synth_from_mels_writes_the_host_writers_files(model_dir):
    import torch
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    inv = MELInverter(model_dir, batch_invariant=True)
    rng = np.random.default_rng(2)
    mels = [rng.normal(-5, 2, size=(1, int(tt), 80)).astype(np.float32) for tt in (17, 33)]
    torch.manual_seed(5)
    singles = [inv.synth_from_mel(mm) for mm in mels]
    torch.manual_seed(5)
    files = inv.synth_from_mels(mels, max_batch=2, flac=True, flac_compression="fixed")
    assert all(ff == flac.encode(aa, inv.srate, compression="fixed") for ff, aa in zip(files, singles))
    sizes = [(len(ff), len(flac.encode(aa, inv.srate))) for ff, aa in zip(files, singles)]
    assert all(got <= plain for got, plain in sizes) and any(got < plain for got, plain in sizes), sizes
    torch.manual_seed(5)
    files = inv.synth_from_mels(mels, max_batch=2, flac=True)                  # the default stays VERBATIM
    assert all(ff == flac.encode(aa, inv.srate) for ff, aa in zip(files, singles))


@pytest.mark.timeout(900)
def test_cli_flag_compresses_and_the_default_keeps_its_bytes(model_dir, tmp_path):
    """resynth_mel.py --batch 2 --flac-compression fixed: files that read_audio reads back; without the flag, today's
    bytes (VERBATIM frames of the same samples)."""
    from mbexwn_vocoder_amd.audioio import read_audio
    from mbexwn_vocoder_amd.batched import have_soundfile
    from mbexwn_vocoder_amd.fileio import save_var
    files = []
    for ii, frames in enumerate((23, 7)):
        rng = np.random.default_rng(40 + ii)
        files.append(str(tmp_path / f"utt{ii}.mell"))
        save_var(files[-1], {"nfft": 2048, "hoplen": 300, "winlen": 1200, "nmels": 80, "sr": 24000, "fmin": 0.0, "fmax": 12000.0,
                             "lin_spec_offset": 1e-5, "lin_spec_scale": 1, "log_spec_offset": 0.0, "log_spec_scale": 1,
                             "time_axis": 1, "mell": rng.normal(-5, 2, size=(80, frames)).astype(np.float32)})
    outs, res_notes = {}, {}
    for name, extra in (("fixed", ["--flac-compression", "fixed"]), ("default", [])):
        out = str(tmp_path / name)
        res = subprocess.run([sys.executable, CLI, model_dir, "-i", *files, "-o", out, "--batch", "2", "--batch-invariant", *extra],
                             capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-3000:]
        res_notes[name] = res.stderr
        outs[name] = {nn: os.path.join(out, nn) for nn in sorted(os.listdir(out))}
    assert list(outs["fixed"]) == list(outs["default"]) == ["syn_utt0.flac", "syn_utt1.flac"]
    if have_soundfile():                                     # soundfile writes the files: the flag is ignored, with a note
        assert "--flac-compression is ignored" in res_notes["fixed"]
        return
    smaller = 0
    for nn in outs["fixed"]:
        plain = open(outs["default"][nn], "rb").read()
        pcm, rate = flac.decode(plain)
        assert plain == flac.encode(pcm, rate)                                  # today's bytes
        packed = open(outs["fixed"][nn], "rb").read()
        # never larger than VERBATIM: a short, noise-like file (the model's weights are random) may save nothing
        assert packed == flac.encode(pcm, rate, compression="fixed") and len(packed) <= len(plain)
        smaller += len(packed) < len(plain)
        audio, rate2 = read_audio(outs["fixed"][nn])
        assert rate2 == rate and np.array_equal(np.rint(np.asarray(audio) * 32768.0).astype(np.int16), pcm)
    assert smaller, "the flag did not reach the writer: no file is smaller than its VERBATIM form"

"""flac.encode(..., compression="fixed") -- fixed predictors of orders 0-4 with partitioned Rice codes -- and the reader of
what it and other encoders of the same sub-frame kinds write; the host-side argument checks and the header of the device
encoder mbxf_encode_flac16_fixed (no GPU needed).  The definition of the stream is DESIGN.md's ("Compressed FLAC")."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from mbexwn_vocoder_amd import flac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 24000
# every block-size edge; 4096 + 333: an odd last block; 4096 + 2048: a last block of 4096 / 2
LENGTHS = [0, 1, 2, 3, 4, 5, 6, 15, 16, 17, 48, 4095, 4096, 4097, 3 * 4096 + 77, 4096 + 333, 4096 + 2048]


def sine(n):
    return 0.5 * np.sin(2 * np.pi * 440 * np.arange(n) / RATE)


def harmonic(n):
    xx = sum(np.sin(2 * np.pi * 120 * kk * np.arange(n) / RATE) / kk for kk in range(1, 40))
    return 0.5 * xx / np.max(np.abs(xx))


def kinds(data):
    """(kind, order) of every frame of a signal, by the encoder's own plan."""
    pcm = flac.to_pcm16(data)
    return [flac.plan_fixed_frame(pcm[ss:ss + flac.BLOCK])[:2] for ss in range(0, pcm.size, flac.BLOCK)]


def subframe_bytes(stream, n):
    """The sub-frame type byte of every frame of a mono stream this module wrote (the frames are found by decoding their
    lengths out of a re-encode: here simply by walking the known headers)."""
    out, pos = [], flac.HEADER_BYTES
    lengths = [len(ff) for ff in flac.fixed_frames(flac.decode(stream)[0], flac.decode(stream)[1])]
    _, _, heads = flac.frame_layout(n)
    for ll, hh in zip(lengths, heads):
        out.append(stream[pos + int(hh)])
        pos += ll
    assert pos == len(stream)
    return out


@pytest.mark.parametrize("n", LENGTHS)
def test_round_trip(n):
    rng = np.random.default_rng(n)
    for data in (sine(n), 0.2 * rng.standard_normal(n), rng.integers(-32768, 32768, n).astype(np.int16)):
        stream = flac.encode(data, RATE, compression="fixed")
        pcm, rate = flac.decode(stream)
        assert rate == RATE and pcm.dtype == np.int16 and np.array_equal(pcm, flac.to_pcm16(data))
        assert len(stream) <= len(flac.encode(data, RATE))                       # never larger than VERBATIM


def test_decisions_at_the_boundaries():
    """The choices follow from the definition; they were worked out from it on paper / with plain integers (the hand-assembled
    frame below does that for 5 samples)."""
    assert kinds(sine(1)) == [("constant", None)]
    assert kinds(sine(2)) == kinds(sine(3)) == [("verbatim", None)]
    assert kinds(sine(4)) == kinds(sine(5)) == kinds(sine(6)) == [("fixed", 2)]
    for n in (15, 16, 17, 48, 4095, 4096):
        assert kinds(sine(n)) == [("fixed", 4)], n
    assert kinds(np.zeros(2 * 4096 + 5)) == [("constant", None)] * 3
    rng = np.random.default_rng(0)
    assert kinds(rng.uniform(-1.0, 1.0, 3 * 4096 + 100)) == [("verbatim", None)] * 4
    assert kinds(np.where(np.arange(2 * 4096 + 9) % 2 == 0, 1.0, -1.0)) == [("verbatim", None)] * 3
    assert kinds((3 * np.arange(2 * 4096) - 12000).astype(np.int16)) == [("fixed", 2)] * 2
    assert kinds(0.01 * rng.standard_normal(3 * 4096)) == [("fixed", 0)] * 3
    # the plan is what the stream holds
    stream = flac.encode(sine(4097), RATE, compression="fixed")
    assert subframe_bytes(stream, 4097) == [0x10 + 2 * 4, 0x00]
    assert [flac.partition_order(nn) for nn in (1, 5, 16, 17, 48, 2048, 4096, 4095, 80, 64)] == [0, 0, 1, 0, 3, 4, 4, 0, 4, 3]


def rice_bits(res, k):
    """One residual as FLAC codes it, as a string of 0 / 1."""
    u = 2 * res if res >= 0 else -2 * res - 1
    return "0" * (u >> k) + "1" + (format(u & ((1 << k) - 1), f"0{k}b") if k else "")


def signed_bits(value, width):
    return format(value & ((1 << width) - 1), f"0{width}b") if width else ""


def frame_from_bits(index, size, bits, rate=RATE):
    """A frame from its header (flac.frame_header, unchanged by this feature) and the sub-frame given as a bit string."""
    bits += "0" * (-len(bits) % 8)                             # zero bits up to the byte boundary
    frame = flac.frame_header(index, size, rate) + int(bits, 2).to_bytes(len(bits) // 8, "big")
    return frame + flac.crc16(frame).to_bytes(2, "big")


def stream_of(frames, pcm, rate=RATE):
    pcm = np.asarray(pcm, dtype=np.int16)
    md5 = hashlib.md5(pcm.astype("<i2").tobytes()).digest()
    return flac.stream_header(pcm.size, rate, md5, frame_lengths=[len(ff) for ff in frames]) + b"".join(frames)


def test_hand_assembled_frame_equals_the_encoders():
    """The 5-sample sine frame, bit by bit from the format text with plain Python integers."""
    x = [int(vv) for vv in flac.to_pcm16(sine(5))]
    assert x == [0, 1883, 3741, 5550, 7285]                    # rint(32767 * 0.5 * sin(2 pi 440 n / 24000))
    # costs of the orders (one partition: 5 has no trailing zero bit, p = 0), T(o) = 16 o + 6 + 4 + min_k B(k)
    totals = {}
    for order in range(5):
        res = list(x)
        for _ in range(order):
            res = [bb - aa for aa, bb in zip(res, res[1:])]
        zig = [2 * rr if rr >= 0 else -2 * rr - 1 for rr in res]
        costs = [sum(uu >> kk for uu in zig) + (kk + 1) * len(zig) for kk in range(15)]
        totals[order] = (16 * order + 6 + 4 + min(costs), costs.index(min(costs)), res)
    order = min(totals, key=lambda oo: (totals[oo][0], oo))
    total, k, res = totals[order]
    assert order == 2 and res == [-25, -49, -74] and total < 16 * 5   # second differences; cheaper than 80 VERBATIM bits
    bits = format(0x10 + 2 * order, "08b")                     # 0 | 001 010 (FIXED, order 2) | 0 (no wasted bits)
    bits += "".join(signed_bits(vv, 16) for vv in x[:order])   # two warm-up samples
    bits += "00"                                               # Rice codes with 4-bit parameters
    bits += format(0, "04b")                                   # partition order 0
    bits += format(k, "04b")                                   # the one partition's parameter
    bits += "".join(rice_bits(rr, k) for rr in res)
    assert len(bits) == 8 + total
    frame = frame_from_bits(0, 5, bits)
    assert flac.fixed_frames(flac.to_pcm16(sine(5)), RATE) == [frame]
    assert flac.encode(sine(5), RATE, compression="fixed") == stream_of([frame], x)


def fixed_bits(x, order, part_order, params, method=0, raw=(), wasted=0):
    """A FIXED sub-frame as a bit string: any partition order, either Rice method, partitions listed in ``raw`` as escape
    partitions (their residuals in as many bits as the widest needs), ``wasted`` zero bits taken off every sample."""
    x = [vv >> wasted for vv in x]
    res = list(x)
    for _ in range(order):
        res = [bb - aa for aa, bb in zip(res, res[1:])]
    bits = format(0x10 + 2 * order + (1 if wasted else 0), "08b")
    if wasted:
        bits += "0" * (wasted - 1) + "1"
    bits += "".join(signed_bits(vv, 16 - wasted) for vv in x[:order])
    bits += format(method, "02b") + format(part_order, "04b")
    plen, pos = len(x) >> part_order, 0
    for part in range(1 << part_order):
        count = plen - (order if part == 0 else 0)
        chunk = res[pos:pos + count]
        pos += count
        if part in raw:
            width = max(max(vv.bit_length() for vv in chunk) + 1, 1) if any(chunk) else 0
            bits += "1" * (4 + method) + format(width, "05b") + "".join(signed_bits(vv, width) for vv in chunk)
        else:
            bits += format(params[part], f"0{4 + method}b") + "".join(rice_bits(vv, params[part]) for vv in chunk)
    return bits


def test_decoder_reads_streams_the_encoder_never_writes():
    rng = np.random.default_rng(8)
    x = [int(vv) for vv in np.cumsum(rng.integers(-300, 301, 64))]
    cases = {
        "5-bit parameters": fixed_bits(x, 2, 3, [9, 8, 17, 9, 9, 0, 9, 10], method=1),
        "escape partitions": fixed_bits(x, 1, 2, [8, 0, 8, 0], raw=(1, 3)),
        "escape with 5-bit parameters": fixed_bits(x, 3, 1, [10, 0], method=1, raw=(1,)),
        "another partition order": fixed_bits(x, 1, 2, [8, 7, 9, 8]),           # the rule gives 64 samples order 3
        "partition order 6": fixed_bits(x, 0, 6, [11] * 64),                    # one residual per partition
    }
    assert flac.partition_order(64) == 3
    for name, bits in cases.items():
        got, rate = flac.decode(stream_of([frame_from_bits(0, 64, bits)], x))
        assert rate == RATE and got.tolist() == x, name
    # a silent escape partition: 0 bits per residual
    flat = [5] * 32 + x[:32]
    bits = fixed_bits(flat, 1, 1, [0, 9], raw=(0,))
    assert flac.decode(stream_of([frame_from_bits(0, 64, bits)], flat))[0].tolist() == flat
    # wasted bits: FIXED, VERBATIM and CONSTANT sub-frames whose samples are multiples of 8
    y = [8 * vv for vv in x]
    got, _ = flac.decode(stream_of([frame_from_bits(0, 64, fixed_bits(y, 2, 3, [8] * 8, wasted=3))], y))
    assert got.tolist() == y
    verbatim = format(0x03, "08b") + "001" + "".join(signed_bits(vv >> 3, 13) for vv in y)
    constant = format(0x01, "08b") + "01" + signed_bits(-40 >> 2, 14)
    frames = [frame_from_bits(0, 64, verbatim), frame_from_bits(1, 7, constant)]
    got, _ = flac.decode(stream_of(frames, y + [-40] * 7))
    assert got.tolist() == y + [-40] * 7
    # two frames of different kinds, and the checks still hold: a flipped residual bit fails the CRC-16
    frames = [frame_from_bits(0, 64, cases["5-bit parameters"]), frame_from_bits(1, 64, cases["escape partitions"])]
    stream = stream_of(frames, x + x)
    assert flac.decode(stream)[0].tolist() == x + x
    bad = bytearray(stream)
    bad[flac.HEADER_BYTES + 30] ^= 0x10
    with pytest.raises(ValueError, match="CRC-16"):
        flac.decode(bad)
    with pytest.raises(ValueError, match="MD5"):
        flac.decode(stream_of(frames, x + x[::-1]))
    with pytest.raises(ValueError, match="STREAMINFO states"):
        flac.decode(flac.stream_header(200, RATE, bytes(16), frame_lengths=[len(ff) for ff in frames]) + b"".join(frames))
    with pytest.raises(ValueError, match="truncated|CRC-16|sync"):
        flac.decode(stream[:-40])


def test_decoder_still_refuses_lpc_and_stereo():
    x = list(range(16))
    lpc = format(0x40 | (1 << 1), "08b") + "0" * 200             # 1xxxxx: LPC of order 2
    with pytest.raises(ValueError, match="soundfile"):
        flac.decode(stream_of([frame_from_bits(0, 16, lpc)], x))
    stereo = flac.encode(np.zeros((100, 2), dtype=np.int16), 44100)
    with pytest.raises(ValueError, match="soundfile"):
        flac.decode(stereo)
    with pytest.raises(ValueError, match="mono"):
        flac.encode(np.zeros((100, 2), dtype=np.int16), 44100, compression="fixed")
    with pytest.raises(ValueError, match="compression"):
        flac.encode(np.zeros(100, dtype=np.int16), 44100, compression="lpc")


def test_default_is_unchanged_and_layout_helpers_take_frame_lengths(tmp_path):
    rng = np.random.default_rng(5)
    data = (0.3 * rng.standard_normal(3 * 4096 + 77)).astype(np.float32)
    assert flac.encode(data, RATE) == flac.encode(data, RATE, compression="verbatim") == flac.encode(data, RATE, "verbatim")
    both = np.stack([data, -data], axis=1)
    assert flac.encode(both, RATE) == flac.encode(both, RATE, compression="verbatim")
    # assemble / write_frames with the frame lengths and the PCM give the encoder's stream; audioio reads it
    pcm = flac.to_pcm16(data)
    frames = flac.fixed_frames(pcm, RATE)
    want = flac.encode(data, RATE, compression="fixed")
    lengths = [len(ff) for ff in frames]
    packed = np.frombuffer(b"".join(frames), dtype=np.uint8)
    assert flac.assemble(packed, pcm.size, RATE, frame_lengths=lengths, pcm=pcm) == want
    path = flac.write_frames(str(tmp_path / "a.flac"), packed, pcm.size, RATE, frame_lengths=lengths, pcm=pcm)
    assert open(path, "rb").read() == want
    assert open(flac.write(str(tmp_path / "b.flac"), data, RATE, compression="fixed"), "rb").read() == want
    info = want[8:42]
    assert int.from_bytes(info[4:7], "big") == min(lengths) and int.from_bytes(info[7:10], "big") == max(lengths)
    with pytest.raises(ValueError, match="lengths"):
        flac.assemble(packed, pcm.size, RATE, frame_lengths=lengths)
    from mbexwn_vocoder_amd.audioio import read_audio
    try:
        import soundfile  # noqa: F401
    except ImportError:
        audio, rate = read_audio(path)
        assert rate == RATE and np.array_equal(np.rint(audio * 32768.0).astype(np.int16), pcm)


def test_compressed_size():
    """From the definition, without headers: 3 * 4096 + 77 samples of the 440 Hz sine take 0.244 of the VERBATIM bits, the
    39-harmonic 120 Hz tone 0.69; with headers the frames stay below 0.30 and 0.75 of the VERBATIM frames."""
    n = 3 * 4096 + 77
    for data, bound in ((sine(n), 0.30), (harmonic(n), 0.75)):
        frames = flac.fixed_frames(flac.to_pcm16(data), RATE)
        assert sum(len(ff) for ff in frames) <= bound * flac.frames_bytes(n)
    rng = np.random.default_rng(1)
    for data in (sine(n), harmonic(n), rng.uniform(-1, 1, n), np.zeros(n), np.where(np.arange(n) % 2 == 0, 1.0, -1.0),
                 0.01 * rng.standard_normal(n), np.arange(n).astype(np.int16), rng.integers(-32768, 32768, n).astype(np.int16),
                 rng.integers(-2, 3, n).astype(np.int16), np.cumsum(rng.integers(-3000, 3001, n)).clip(-32768, 32767) / 32768.0):
        frames = flac.fixed_frames(flac.to_pcm16(data), RATE)
        offsets = flac.frame_layout(n)[0]
        assert all(len(ff) <= int(ll) for ff, ll in zip(frames, np.diff(offsets)))   # frame by frame, never above VERBATIM
        assert np.array_equal(flac.decode(flac.encode(data, RATE, compression="fixed"))[0], flac.to_pcm16(data))


def test_device_encoder_refuses_bad_arguments_before_touching_the_device():
    """mbxf_encode_flac16_fixed checks every argument on the host and returns MBX_ERR_INVALID_ARGUMENT without a launch."""
    from mbexwn_vocoder_amd import engine
    from mbexwn_vocoder_amd.build import build_library
    build_library()
    lib = engine.load_library()
    fake = ctypes.c_void_p(256)                              # never dereferenced: the checks fail first

    def call(counts, stride, out_bytes, rate=RATE, audio=fake, tables=fake, out=fake, lengths=fake, work=fake, peak=fake):
        arr = (ctypes.c_int64 * max(1, len(counts)))(*counts)
        return lib.mbxf_encode_flac16_fixed(audio, stride, len(counts), arr, rate, tables, out, out_bytes, lengths, work, None,
                                            peak, None)

    def why():
        return lib.mbx_last_error().decode()

    limit = 1 << 28
    # the capacity must cover the case that nothing compresses: one byte below it is refused
    assert call([4096, 100], 4096, flac.frames_bytes(4096) + flac.frames_bytes(100) - 1) == 1 and "output buffer" in why()
    assert call([-1], 4096, 1 << 20) == 1 and "n_samples" in why()
    assert call([10, 20], 15, 1 << 20) == 1 and "stride" in why()
    assert call([limit + 1], limit + 1, 1 << 40) == 1 and "2^28" in why()
    assert call([4096], 4096, 1 << 20, rate=1 << 20) == 1 and call([4096], 4096, 1 << 20, rate=0) == 1
    for name in ("audio", "tables", "out", "lengths", "work", "peak"):
        assert call([4096], 4096, 1 << 20, **{name: None}) == 1 and "null" in why(), name
    assert lib.mbxf_encode_flac16_fixed(fake, 4096, -1, None, RATE, fake, fake, 1 << 20, fake, fake, None, fake, None) == 1
    assert lib.mbxf_encode_flac16_fixed(fake, 4096, 1, None, RATE, fake, fake, 1 << 20, fake, fake, None, fake, None) == 1
    assert call([], 0, 0) == 0                               # an empty batch is nothing to do
    assert why().startswith("encode flac16 fixed:") or "encode flac16 fixed" in why()


def test_header_declares_the_encoder_and_the_library_exports_it(tmp_path):
    """(that the header declares exactly these names, no other header does and the library exports them: test_abi_headers.py)"""
    from mbexwn_vocoder_amd import abi
    from mbexwn_vocoder_amd.build import HEADERS, SOURCES
    path = os.path.join(ROOT, "include", "mbexwn_flac.h")
    text = open(path).read()
    assert "workspace" in text and "Refused" in text and "T(o)" in text    # the buffers, the refusals, the definition
    assert abi.symbols("mbexwn_flac.h") == ["mbxf_encode_flac16_fixed"]
    assert any(hh.endswith("mbexwn_flac.h") for hh in HEADERS) and "flac_fixed.hip" in SOURCES
    assert abi.MBX_ABI_VERSION == 11
    # the header compiles as C
    src = tmp_path / "use.c"
    src.write_text('#include "mbexwn_flac.h"\nint main(void){ (void)mbxf_encode_flac16_fixed; return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)

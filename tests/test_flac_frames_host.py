"""The FLAC format pieces the device encoder shares with the host writer (flac.py): frame layout, frame and stream headers,
the CRC-16 shift operators of the parallel CRC, and the argument checks of mbx_encode_flac16 (no GPU needed)."""
import ctypes
import hashlib
import struct

import numpy as np
import pytest

from mbexwn_vocoder_amd import flac


@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 3 * 4096, 128 * 4096 + 1, 2048 * 4096 + 1])
def test_layout_and_headers_rebuild_encode(n):
    """frame_layout / frame_header / stream_header put together by hand give flac.encode's bytes (2- and 3-byte frame
    numbers included); pcm16_from_frames and assemble read the samples back out of the frames."""
    rng = np.random.default_rng(n)
    x = np.clip(0.5 * rng.standard_normal(n), -1.3, 1.3).astype(np.float32)
    want = flac.encode(x, 24000)
    offsets, sizes, heads = flac.frame_layout(n)
    assert offsets[-1] == flac.frames_bytes(n) == len(want) - flac.HEADER_BYTES and sizes.sum() == n
    pcm = flac.to_pcm16(x)
    frames = bytearray(offsets[-1])
    for ff in range(sizes.size):
        block = pcm[ff * flac.BLOCK:ff * flac.BLOCK + sizes[ff]]
        frame = flac.frame_header(ff, int(sizes[ff]), 24000)
        assert len(frame) == heads[ff]
        frame += b"\x02" + block.astype(">i2").tobytes()
        frame += struct.pack(">H", flac.crc16(frame))
        assert len(frame) == offsets[ff + 1] - offsets[ff]
        frames[offsets[ff]:offsets[ff + 1]] = frame
    md5 = hashlib.md5(pcm.astype("<i2").tobytes()).digest()
    assert flac.stream_header(n, 24000, md5) + bytes(frames) == want
    assert np.array_equal(flac.pcm16_from_frames(bytes(frames), n), pcm)
    assert flac.assemble(np.frombuffer(bytes(frames), np.uint8), n, 24000) == want


def test_crc16_combine_joins_random_splits():
    rng = np.random.default_rng(3)
    for _ in range(200):
        data = rng.integers(0, 256, size=int(rng.integers(0, 300))).astype(np.uint8).tobytes()
        cut = int(rng.integers(0, len(data) + 1))
        a, b = data[:cut], data[cut:]
        assert flac.crc16_combine(flac.crc16(a), flac.crc16(b), len(b)) == flac.crc16(data)
    for a, b in ((b"", b"x"), (b"x", b""), (b"", b""), (b"1", b"23456789"), (b"12345678", b"9")):
        assert flac.crc16_combine(flac.crc16(a), flac.crc16(b), len(b)) == flac.crc16(a + b)
    big = bytes(rng.integers(0, 256, size=70000).astype(np.uint8))               # lengths beyond the device's 16 operators
    assert flac.crc16_combine(flac.crc16(big[:5]), flac.crc16(big[5:]), len(big) - 5) == flac.crc16(big)


def test_device_tables_layout():
    tab = flac.crc16_device_tables()
    assert tab.dtype == np.uint16 and tab.size == 256 + 16 * flac.CRC16_DEVICE_SHIFTS == 512
    assert list(tab[:256]) == [flac.crc16(bytes([bb])) for bb in range(256)]
    ops = tab[256:].reshape(flac.CRC16_DEVICE_SHIFTS, 16)
    for kk in (0, 3, 13):                                    # column j of M_{2^k}: register 1 << j over 2^k zero bytes
        for jj in (0, 7, 15):
            reg = 1 << jj
            for _ in range(1 << kk):
                reg = ((reg << 8) & 0xFFFF) ^ flac.crc16(bytes([reg >> 8]))
            assert ops[kk, jj] == reg


def test_encoder_refuses_bad_arguments_before_touching_the_device():
    """mbx_encode_flac16 checks every argument on the host and returns MBX_ERR_INVALID_ARGUMENT without a launch: items
    longer than 2^28 samples (frame numbers of more than 3 bytes), counts beyond the stride, a short output buffer."""
    from mbexwn_vocoder_amd import engine
    from mbexwn_vocoder_amd.build import build_library
    build_library()
    lib = engine.load_library()
    fake = ctypes.c_void_p(256)                              # never dereferenced: the checks fail first

    def call(counts, stride, out_bytes, rate=24000):
        arr = (ctypes.c_int64 * len(counts))(*counts)
        return lib.mbx_encode_flac16(fake, stride, len(counts), arr, rate, fake, fake, out_bytes, fake, None)

    limit = 1 << 28
    assert call([limit + 1], limit + 1, 1 << 40) == 1 and "2^28" in lib.mbx_last_error().decode()
    assert call([10, 20], 15, 1 << 20) == 1 and "stride" in lib.mbx_last_error().decode()
    assert call([4096], 4096, flac.frames_bytes(4096) - 1) == 1 and "output buffer" in lib.mbx_last_error().decode()
    assert call([4096], 4096, 1 << 20, rate=1 << 20) == 1
    assert call([], 0, 0) == 0                               # an empty batch is nothing to do

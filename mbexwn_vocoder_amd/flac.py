"""Minimal FLAC writer (mono / multi-channel 16-bit PCM, VERBATIM sub-frames; mono with FIXED predictors and Rice codes on
request) for the CLI's default output format, and a reader of what it writes (``decode``).

The reference CLI writes ``--format flac`` through its ``sndio`` module on top of libsndfile (reference
bin/resynth_mel.py:104-105), which is not part of this image.  A FLAC stream does not have to be compressed: a
VERBATIM sub-frame stores the samples as they are, and with 16-bit samples every field behind the frame header is byte
aligned, so a valid stream (magic, STREAMINFO with the MD5 of the samples, frames with CRC-8 / CRC-16) can be assembled
with numpy alone.  Any FLAC decoder reads the result; the files are the size of a wav.

The layout of the frames and the headers are defined here once (frame_layout, frame_header, stream_header): ``encode``
builds a stream from them, and the device encoder (csrc/flac_frames.hip through ``encode_device``) writes the
same frames, in front of which ``write_frames`` / ``assemble`` put the header with the MD5 of the samples.

``compression="fixed"`` compresses: every frame takes the cheapest of FLAC's fixed predictors of orders 0-4 with
partitioned Rice codes (``plan_fixed_frame`` makes the choices, DESIGN.md defines them), a CONSTANT sub-frame where all
samples are equal, and stays VERBATIM where no predictor saves a bit.  The device encoder of csrc/flac_fixed.hip
(``encode_device(..., compression="fixed")``) writes the same bytes.  Frame lengths then come from the data:
``stream_header`` / ``assemble`` / ``write_frames`` take them as a list.

Format: https://xiph.org/flac/format.html (STREAMINFO, FRAME_HEADER, SUBFRAME_VERBATIM / _CONSTANT / _FIXED, RESIDUAL,
FRAME_FOOTER).
"""
import hashlib
import struct

import numpy as np

BLOCK = 4096                                # samples per channel of every frame but the last
HEADER_BYTES = 42                           # "fLaC" + STREAMINFO in front of the frames
_RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
_NUMBER_LIMITS = (0x80, 0x800, 0x10000, 0x200000, 0x4000000)   # a "UTF-8" frame number takes one more byte at each


def _crc_table(poly, bits):
    table = []
    top = 1 << (bits - 1)
    mask = (1 << bits) - 1
    for byte in range(256):
        crc = byte << (bits - 8)
        for _ in range(8):
            crc = ((crc << 1) ^ poly) & mask if crc & top else (crc << 1) & mask
        table.append(crc)
    return table


_CRC8 = _crc_table(0x07, 8)
_CRC16 = _crc_table(0x8005, 16)


def crc8(data):
    crc = 0
    for byte in data:
        crc = _CRC8[crc ^ byte]
    return crc


def crc16(data):
    crc = 0
    for byte in data:
        crc = ((crc << 8) & 0xFFFF) ^ _CRC16[(crc >> 8) ^ byte]
    return crc


def _gf2_apply(columns, value):
    out = 0
    for jj in range(16):
        if value >> jj & 1:
            out ^= columns[jj]
    return out


_SHIFT_OPS = []
CRC16_DEVICE_SHIFTS = 16                    # operators the device encoder takes (its frames are shorter than 2^14 bytes)


def crc16_shift_operators(count):
    """The operators M_{2^k}, k < count, of the CRC-16: M_n advances the register over n zero bytes.  With init 0 and no
    final XOR the CRC is linear over GF(2), so crc16(a + b) = M_len(b) crc16(a) ^ crc16(b).  An operator is its 16 columns:
    column j is the register 1 << j advanced."""
    if not _SHIFT_OPS:
        _SHIFT_OPS.append([((1 << jj << 8) & 0xFFFF) ^ _CRC16[(1 << jj) >> 8] for jj in range(16)])
    while len(_SHIFT_OPS) < count:
        prev = _SHIFT_OPS[-1]
        _SHIFT_OPS.append([_gf2_apply(prev, _gf2_apply(prev, 1 << jj)) for jj in range(16)])
    return _SHIFT_OPS[:count]


def crc16_combine(crc_a, crc_b, len_b):
    """crc16(a + b) from crc16(a), crc16(b) and len(b): M_len(b) is the product of the operators of the set bits of len(b)."""
    nn = int(len_b)
    ops = crc16_shift_operators(max(1, nn.bit_length()))
    for kk in range(nn.bit_length()):
        if nn >> kk & 1:
            crc_a = _gf2_apply(ops[kk], crc_a)
    return crc_a ^ crc_b


def crc16_device_tables():
    """What mbx_encode_flac16 takes as ``crc_tables``: uint16 (256 + 16 * CRC16_DEVICE_SHIFTS), the byte table of crc16, then
    the columns of M_1, M_2, M_4, ... (include/mbexwn.h)."""
    ops = crc16_shift_operators(CRC16_DEVICE_SHIFTS)
    return np.asarray(_CRC16 + [cc for op in ops for cc in op], dtype=np.uint16)


def _utf8_number(value):
    """The "UTF-8" coding of a frame number (up to 31 bits)."""
    if value < 0x80:
        return bytes([value])
    out = []
    lead_bits = 6
    while value >= (1 << lead_bits):
        out.append(0x80 | (value & 0x3F))
        value >>= 6
        lead_bits -= 1
    lead = (0xFF << (lead_bits + 1)) & 0xFF
    out.append(lead | value)
    return bytes(reversed(out))


def to_pcm16(data):
    """float audio in [-1, 1] -> int16, scaled by 0x7FFF as libsndfile scales normalised floats for a 16-bit file (the
    reference's sndio path, bin/resynth_mel.py:104-105), rounded and clipped; int16 passes through; any other integer type
    is refused (its scale is ambiguous: convert it yourself).  (frames,) or (frames, channels)."""
    data = np.asarray(data)
    if data.dtype == np.int16:
        return data
    if not np.issubdtype(data.dtype, np.floating):
        raise TypeError(f"FLAC writer: float or int16 samples expected, got {data.dtype}")
    return np.clip(np.rint(data.astype(np.float64) * 32767.0), -32768, 32767).astype(np.int16)


def frame_layout(n, channels=1):
    """Where the frames of an n-sample stream lie behind its header: int64 arrays ``offsets`` (frames + 1: frame f spans
    bytes offsets[f]:offsets[f + 1]), ``sizes`` (samples per channel of every frame) and ``heads`` (bytes of every frame's
    header, CRC-8 included; the sub-frames follow it, each a 0x02 byte and 2 * size bytes)."""
    index = np.arange(-(-int(n) // BLOCK), dtype=np.int64)
    sizes = np.minimum(BLOCK, int(n) - index * BLOCK)
    number = 1 + sum((index >= lim).astype(np.int64) for lim in _NUMBER_LIMITS)
    heads = 4 + number + 2 * (sizes != BLOCK) + 1
    offsets = np.zeros(index.size + 1, dtype=np.int64)
    np.cumsum(heads + channels * (1 + 2 * sizes) + 2, out=offsets[1:])
    return offsets, sizes, heads


def frames_bytes(n, channels=1):
    """Bytes of the frames of an n-sample stream (the stream without its 42-byte header)."""
    return int(frame_layout(n, channels)[0][-1])


def frame_header(index, size, rate, channels=1):
    """Header of frame ``index`` holding ``size`` samples per channel of a ``rate`` Hz stream, CRC-8 included."""
    size_code = 12 if size == BLOCK else 7                       # 1100: 4096; 0111: 16-bit (blocksize - 1) follows
    rate_code = _RATE_CODES.get(int(rate), 0)                    # 0000: take the rate from STREAMINFO
    head = bytes([0xFF, 0xF8, (size_code << 4) | rate_code, ((channels - 1) << 4) | (4 << 1)])     # 100: 16 bits
    head += _utf8_number(index)
    if size_code == 7:
        head += struct.pack(">H", size - 1)
    return head + bytes([crc8(head)])


def stream_header(n, rate, md5, channels=1, frame_lengths=None):
    """The 42 bytes in front of the frames: "fLaC" and STREAMINFO (block sizes, the smallest and largest frame -- of
    ``frame_lengths`` where the frames are compressed, else of frame_layout --, rate, channels, 16 bits, sample count,
    ``md5`` = MD5 digest of the little-endian int16 samples)."""
    lengths = np.diff(frame_layout(n, channels)[0]) if frame_lengths is None else np.asarray(frame_lengths, dtype=np.int64)
    min_frame, max_frame = (int(lengths.min()), int(lengths.max())) if lengths.size else (0, 0)
    info = struct.pack(">HH", BLOCK, BLOCK) + min_frame.to_bytes(3, "big") + max_frame.to_bytes(3, "big")
    packed = (int(rate) << 44) | ((channels - 1) << 41) | ((16 - 1) << 36) | int(n)          # 20 + 3 + 5 + 36 bits
    info += packed.to_bytes(8, "big") + md5
    assert len(info) == 34
    return b"fLaC" + bytes([0x80]) + len(info).to_bytes(3, "big") + info         # last-block flag | STREAMINFO


MAX_FIXED_ORDER = 4
MAX_RICE = 14                               # Rice parameters 0..14 in 4 bits; 15 would mark an escape partition, never written
COMPRESSIONS = ("verbatim", "fixed")


def partition_order(size):
    """Partition order of a ``size``-sample frame: min(4, trailing zero bits of size), lowered while the partitions would
    hold 4 samples or fewer."""
    size = int(size)
    order = min(4, (size & -size).bit_length() - 1)
    while order > 0 and (size >> order) <= 4:
        order -= 1
    return order


def _fixed_costs(block):
    """Per fixed order o = 0 .. min(4, size - 1) of one frame: (T(o), Rice parameter per partition, zigzag residuals u of
    n >= o, first residual of every partition, residuals per partition)."""
    size = block.size
    parts = 1 << partition_order(size)
    plen = size // parts
    shifts = np.arange(MAX_RICE + 1, dtype=np.int64)[:, None]
    res = block.astype(np.int64)
    out = []
    for order in range(min(MAX_FIXED_ORDER, size - 1) + 1):
        if order:
            res = np.diff(res)
        zig = np.where(res >= 0, 2 * res, -2 * res - 1)
        starts = np.maximum(np.arange(parts, dtype=np.int64) * plen - order, 0)
        counts = np.diff(np.append(starts, size - order))
        cost = np.add.reduceat(zig[None, :] >> shifts, starts, axis=1) + (shifts + 1) * counts[None, :]
        rice = np.argmin(cost, axis=0)                        # the first minimum: ties go to the smaller parameter
        out.append((16 * order + 6 + int((4 + cost.min(axis=0)).sum()), rice, zig, starts, counts))
    return out


def plan_fixed_frame(block):
    """The choices ``compression="fixed"`` makes for one frame of int16 samples: ``(kind, order, partition order, Rice
    parameters)`` with kind "constant" (all samples equal), "fixed" (the smallest T(o) is below 16 * size bits; ties go to
    the smaller order) or "verbatim"; order and the rest are None unless the kind is "fixed"."""
    block = np.asarray(block)
    if np.all(block == block[0]):
        return "constant", None, None, None
    costs = _fixed_costs(block)
    order = min(range(len(costs)), key=lambda oo: (costs[oo][0], oo))
    if costs[order][0] >= 16 * block.size:
        return "verbatim", None, None, None
    return "fixed", order, partition_order(block.size), [int(kk) for kk in costs[order][1]]


def _pack_fields(zeros, widths, values):
    """Bit fields, most significant bit first, into bytes: field i is zeros[i] zero bits, then the widths[i] (<= 16) low
    bits of values[i]; zero bits up to the byte boundary."""
    ends = np.cumsum(zeros + widths)
    bits = np.zeros(-(-int(ends[-1]) // 8) * 8, dtype=np.uint8)
    for jj in range(int(widths.max())):
        sel = widths > jj
        bits[ends[sel] - 1 - jj] = (values[sel] >> jj) & 1
    return np.packbits(bits).tobytes()


def _fixed_subframe(block):
    """The sub-frame of one mono frame under ``compression="fixed"``: the type byte and what follows it, byte padded."""
    kind, order, part_order, _ = plan_fixed_frame(block)
    if kind == "constant":
        return b"\x00" + block[:1].astype(">i2").tobytes()
    if kind == "verbatim":
        return b"\x02" + block.astype(">i2").tobytes()
    total, rice, zig, starts, counts = _fixed_costs(block)[order]
    par = np.repeat(rice, counts)
    # the residual codes: u >> k zero bits, a one bit, the k low bits of u; in front of every partition its parameter in 4
    # bits; in front of all that the type byte, the warm-up samples, 00 (4-bit parameters) and the partition order
    zeros = np.insert(zig >> par, starts, 0)
    widths = np.insert(par + 1, starts, 4)
    values = np.insert((1 << par) | (zig & ((1 << par) - 1)), starts, rice)
    warm = block[:order].astype(np.int64) & 0xFFFF
    zeros = np.concatenate([np.zeros(order + 3, dtype=np.int64), zeros])
    widths = np.concatenate([[8], np.full(order, 16, dtype=np.int64), [2, 4], widths])
    values = np.concatenate([[0x10 + 2 * order], warm, [0, part_order], values])
    assert int((zeros + widths).sum()) == 8 + total
    return _pack_fields(zeros, widths, values)


def fixed_frames(pcm, rate):
    """The frames of the mono int16 samples ``pcm`` under ``compression="fixed"``: a list of bytes, one per frame."""
    frames = []
    for index, start in enumerate(range(0, pcm.size, BLOCK)):
        block = pcm[start:start + BLOCK]
        frame = frame_header(index, block.size, rate) + _fixed_subframe(block)
        frames.append(frame + struct.pack(">H", crc16(frame)))
    return frames


def encode(data, rate, compression="verbatim"):
    """bytes of a FLAC stream holding ``data`` (float or int16; (frames,) or (frames, channels <= 8)) at ``rate`` Hz.
    ``compression``: "verbatim" (uncompressed sub-frames) or "fixed" (mono only: fixed predictors and Rice codes)."""
    if compression not in COMPRESSIONS:
        raise ValueError(f"FLAC: compression must be one of {COMPRESSIONS}, got {compression!r}")
    pcm = to_pcm16(data)
    if pcm.ndim == 1:
        pcm = pcm[:, None]
    n, channels = pcm.shape
    if not 1 <= channels <= 8 or not 0 < rate < (1 << 20):
        raise ValueError("FLAC: 1..8 channels and a sample rate below 2^20 Hz")
    rate = int(rate)
    if compression == "fixed":
        if channels != 1:
            raise ValueError("FLAC: compression=\"fixed\" writes mono streams only")
        frames = fixed_frames(np.ascontiguousarray(pcm[:, 0]), rate)
        md5 = hashlib.md5(pcm.astype("<i2").tobytes()).digest()
        return stream_header(n, rate, md5, frame_lengths=[len(ff) for ff in frames]) + b"".join(frames)
    frames = []
    for index, start in enumerate(range(0, n, BLOCK)):
        block = pcm[start:start + BLOCK]
        frame = frame_header(index, block.shape[0], rate, channels)
        # one VERBATIM sub-frame per channel: 0 | 000001 | 0, then the samples big-endian
        frame += b"".join(b"\x02" + block[:, ch].astype(">i2").tobytes() for ch in range(channels))
        frame += struct.pack(">H", crc16(frame))
        frames.append(frame)
    md5 = hashlib.md5(pcm.astype("<i2").tobytes()).digest()
    return stream_header(n, rate, md5, channels) + b"".join(frames)


def pcm16_from_frames(frames, n):
    """The int16 samples of the mono frames of an n-sample stream (frame_layout): their big-endian sub-frame bodies,
    byte-swapped into a little-endian array (what the MD5 of STREAMINFO is taken over)."""
    offsets, sizes, heads = frame_layout(n)
    pcm = np.empty(int(n), dtype="<i2")
    for ff in range(sizes.size):
        pcm[ff * BLOCK:ff * BLOCK + sizes[ff]] = np.frombuffer(frames, dtype=">i2", count=int(sizes[ff]),
                                                               offset=int(offsets[ff] + heads[ff] + 1))
    return pcm


def _frames_md5(frames, n, pcm):
    """MD5 of the samples of mono frames: of ``pcm`` (int16, what compressed frames hold) if given, else read out of the
    VERBATIM frames themselves."""
    if pcm is None:
        return hashlib.md5(pcm16_from_frames(frames, n)).digest()
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16 or pcm.shape != (int(n),):
        raise ValueError("FLAC: pcm must hold the stream's n int16 samples")
    return hashlib.md5(pcm.astype("<i2").tobytes()).digest()


def assemble(frames, n, rate, frame_lengths=None, pcm=None):
    """The whole mono stream from frames encoded elsewhere (the device encoder): header with the MD5 of their samples, frames.
    Compressed frames come with the list of their lengths and the int16 samples they hold."""
    if (frame_lengths is None) != (pcm is None):
        raise ValueError("FLAC: compressed frames need both their lengths and their samples")
    return stream_header(n, rate, _frames_md5(frames, n, pcm), frame_lengths=frame_lengths) + bytes(frames)


_BLOCK_SIZES = {1: 192, **{cc: 576 << (cc - 2) for cc in range(2, 6)}, **{cc: 256 << (cc - 8) for cc in range(8, 16)}}


class _ShortWindow(Exception):
    """The bits of a sub-frame run past the window they are read from."""


def _parse_subframe_bits(bits, size, sub):
    """One mono 16-bit sub-frame from the 0/1 array ``bits`` that starts behind its type byte ``sub``: (int64 samples, bits
    read).  CONSTANT, VERBATIM and FIXED, each with or without wasted bits."""
    total = bits.size
    cursor = 0

    def read(width, signed=False):
        nonlocal cursor
        if cursor + width > total:
            raise _ShortWindow
        value = 0
        for bit in bits[cursor:cursor + width].tolist():
            value = (value << 1) | bit
        cursor += width
        return value - (1 << width) if signed and width and value >> (width - 1) else value

    def read_block(count, width):
        """count signed width-bit numbers"""
        nonlocal cursor
        if width == 0:
            return np.zeros(count, dtype=np.int64)
        if cursor + count * width > total:
            raise _ShortWindow
        field = bits[cursor:cursor + count * width].reshape(count, width).astype(np.int64)
        cursor += count * width
        value = field @ (1 << np.arange(width - 1, -1, -1, dtype=np.int64))
        return value - ((value >> (width - 1)) << width)

    wasted = 0
    if sub & 1:                                              # wasted bits: their number minus one in unary
        while read(1) == 0:
            wasted += 1
        wasted += 1
    depth = 16 - wasted
    if depth < 1:
        raise ValueError("FLAC reader: more wasted bits than bits per sample")
    kind = sub >> 1
    if kind == 0:
        block = np.full(size, read(depth, signed=True), dtype=np.int64)
    elif kind == 1:
        block = read_block(size, depth)
    else:
        order = kind - 8
        if order > size:
            raise ValueError("FLAC reader: a FIXED sub-frame with more warm-up samples than the frame holds")
        warm = read_block(order, depth)
        method = read(2)
        if method > 1:
            raise ValueError("FLAC reader: reserved residual coding method")
        par_bits = 4 + method
        part_order = read(4)
        parts = 1 << part_order
        if size % parts or (size >> part_order) < order:
            raise ValueError("FLAC reader: partition order does not fit the block size")
        nxt = None
        residual = []
        for part in range(parts):
            count = (size >> part_order) - (order if part == 0 else 0)
            par = read(par_bits)
            if par == (1 << par_bits) - 1:                   # escape: raw numbers
                residual.append(read_block(count, read(5)))
                continue
            if nxt is None:                                  # position of the first one bit at or behind every position
                idx = np.where(bits != 0, np.arange(total, dtype=np.int64), total)
                nxt = np.minimum.accumulate(idx[::-1])[::-1].tolist()
            ones = []
            for _ in range(count):
                if cursor >= total or nxt[cursor] + par >= total:
                    raise _ShortWindow
                one = nxt[cursor]
                ones.append(one - cursor)
                cursor = one + 1 + par
            quot = np.asarray(ones, dtype=np.int64)
            low = np.zeros(count, dtype=np.int64)
            if par and count:
                first = np.cumsum(quot + 1 + par) - par + (cursor - int((quot + 1 + par).sum()))
                for jj in range(par):
                    low = (low << 1) | bits[first + jj]
            zig = (quot << par) | low
            residual.append((zig >> 1) ^ -(zig & 1))
        seq = np.concatenate(residual) if residual else np.zeros(0, dtype=np.int64)
        for level in range(order - 1, -1, -1):               # undo one difference at a time
            seq = np.diff(warm, n=level)[-1] + np.cumsum(seq)
        block = np.concatenate([warm, seq])
    return block << wasted, cursor


def _decode_subframe_bits(data, pos, size, sub):
    """A sub-frame that is not byte aligned, from byte ``pos`` of ``data`` (behind the type byte): (big-endian int16 block,
    position of the byte behind its padding).  The bits are unpacked from a window that grows when the codes run past it."""
    window = 2 * size + 64
    while True:
        chunk = np.frombuffer(data, dtype=np.uint8, count=min(window, len(data) - pos), offset=pos)
        try:
            block, used = _parse_subframe_bits(np.unpackbits(chunk), size, sub)
            break
        except _ShortWindow:
            if pos + window >= len(data):
                raise ValueError("FLAC reader: truncated frame") from None
            window *= 4
    if block.size and (block.min() < -32768 or block.max() > 32767):
        raise ValueError("FLAC reader: a decoded sample does not fit 16 bits")
    return block.astype(">i2"), pos + -(-used // 8)


def decode(stream):
    """``(int16 samples, rate)`` of a mono 16-bit FLAC stream with VERBATIM, CONSTANT or FIXED sub-frames: what this module's
    writers produce, and what other encoders make of the same kinds (partitioned Rice residuals with 4- or 5-bit parameters,
    escape partitions, wasted bits, any partition order).  Every frame's CRC-8 and CRC-16 and the MD5 of STREAMINFO are
    checked (an all-zero MD5 means "not computed" and is accepted).  Anything else -- more channels, another sample size,
    an LPC sub-frame -- raises ``ValueError`` that says to install ``soundfile``."""
    data = bytes(stream)

    def refuse(what):
        return ValueError(f"FLAC reader: {what}; only mono 16-bit streams with VERBATIM / CONSTANT / FIXED sub-frames are "
                          "built in -- install soundfile to read other FLAC files")

    if len(data) < HEADER_BYTES or data[:4] != b"fLaC":
        raise ValueError("FLAC reader: not a FLAC stream (no fLaC marker)")
    pos, info = 4, None
    while True:
        if pos + 4 > len(data):
            raise ValueError("FLAC reader: truncated metadata")
        last, kind, size = data[pos] >> 7, data[pos] & 0x7F, int.from_bytes(data[pos + 1:pos + 4], "big")
        if kind == 0:
            info = data[pos + 4:pos + 4 + size]
        pos += 4 + size
        if last:
            break
    if info is None or len(info) != 34 or pos > len(data):
        raise ValueError("FLAC reader: no STREAMINFO block")
    packed = int.from_bytes(info[10:18], "big")
    rate, channels, bits, total = packed >> 44, ((packed >> 41) & 7) + 1, ((packed >> 36) & 31) + 1, packed & ((1 << 36) - 1)
    if channels != 1:
        raise refuse(f"{channels} channels")
    if bits != 16:
        raise refuse(f"{bits}-bit samples")
    blocks = []
    while pos < len(data):
        start = pos
        if pos + 5 > len(data) or data[pos] != 0xFF or data[pos + 1] & 0xFE != 0xF8:
            raise ValueError(f"FLAC reader: no frame sync at byte {pos}")
        size_code, rate_code = data[pos + 2] >> 4, data[pos + 2] & 15
        if data[pos + 3] >> 4 != 0 or (data[pos + 3] >> 1) & 7 not in (0, 4) or data[pos + 3] & 1:
            raise refuse("a frame with more than one channel or a sample size other than 16 bits")
        pos += 4
        lead = data[pos]                                     # the "UTF-8" coded frame / sample number: skipped
        pos += 1 if lead < 0x80 else max(2, 8 - (lead ^ 0xFF).bit_length())
        if size_code in (6, 7):
            width = size_code - 5
            size = int.from_bytes(data[pos:pos + width], "big") + 1
            pos += width
        elif size_code in _BLOCK_SIZES:
            size = _BLOCK_SIZES[size_code]
        else:
            raise ValueError("FLAC reader: reserved block size code")
        pos += {12: 1, 13: 2, 14: 2}.get(rate_code, 0)
        if pos + 2 > len(data) or crc8(data[start:pos]) != data[pos]:
            raise ValueError(f"FLAC reader: CRC-8 mismatch in the header of the frame at byte {start}")
        pos += 1
        sub = data[pos]
        pos += 1
        if sub == 0x02:                                      # VERBATIM, no wasted bits
            block = np.frombuffer(data[pos:pos + 2 * size], dtype=">i2")
            pos += 2 * size
        elif sub == 0x00:                                    # CONSTANT
            block = np.full(size, np.frombuffer(data[pos:pos + 2], dtype=">i2")[0] if pos + 2 <= len(data) else 0, dtype=">i2")
            pos += 2
        elif sub & 0x80:
            raise ValueError(f"FLAC reader: sub-frame type byte 0x{sub:02x} with its padding bit set")
        elif sub & 0x40:
            raise refuse("an LPC sub-frame")
        elif sub >> 1 > 1 and not 8 <= sub >> 1 <= 8 + MAX_FIXED_ORDER:
            raise ValueError(f"FLAC reader: reserved sub-frame type byte 0x{sub:02x}")
        else:                                                # FIXED, or wasted bits: not byte aligned
            block, pos = _decode_subframe_bits(data, pos, size, sub)
        if block.size != size or pos + 2 > len(data):
            raise ValueError("FLAC reader: truncated frame")
        if crc16(data[start:pos]) != int.from_bytes(data[pos:pos + 2], "big"):
            raise ValueError(f"FLAC reader: CRC-16 mismatch in the frame at byte {start}")
        pos += 2
        blocks.append(block)
    pcm = np.concatenate(blocks).astype("<i2") if blocks else np.zeros(0, dtype="<i2")
    if total and pcm.size != total:
        raise ValueError(f"FLAC reader: {pcm.size} samples decoded, STREAMINFO states {total}")
    if info[18:34] != bytes(16) and hashlib.md5(pcm.tobytes()).digest() != info[18:34]:
        raise ValueError("FLAC reader: MD5 mismatch")
    return pcm.astype(np.int16), int(rate)


def write(path, data, rate, compression="verbatim"):
    with open(path, "wb") as fo:
        fo.write(encode(data, rate, compression))
    return path


def write_frames(path, frames, n, rate, frame_lengths=None, pcm=None):
    """``assemble`` into a file, the frames written as they are (no copy)."""
    if (frame_lengths is None) != (pcm is None):
        raise ValueError("FLAC: compressed frames need both their lengths and their samples")
    md5 = _frames_md5(frames, n, pcm)
    with open(path, "wb") as fo:
        fo.write(stream_header(n, rate, md5, frame_lengths=frame_lengths))
        fo.write(frames)
    return path


# ------------------------------------------------------------------------------------------------
# the device encoders (mbx_encode_flac16, mbxf_encode_flac16_fixed): no engine handle, only the library
# ------------------------------------------------------------------------------------------------
class EncodedFlac:
    """What :func:`encode_device` (``MBExWNEngine.encode_flac16``) returns: the frames of every item in one pinned host buffer
    (item b at ``offsets[b]:offsets[b + 1]``) and max |x| per item, behind the event of their device-to-host copies.  Compressed
    frames (``compression="fixed"``) come with their lengths (``frame_lengths(b)``) and the int16 samples they hold (``pcm(b)``)."""

    def __init__(self, host, offsets, max_abs, n_samples, rate, event, frame_lengths=None, frame_bounds=None, pcm=None):
        self._host, self._host_max, self._event = host, max_abs, event
        self.offsets, self.n_samples, self.rate = offsets, list(n_samples), rate
        self._lengths, self._bounds, self._pcm = frame_lengths, frame_bounds, pcm
        self.compression = "verbatim" if frame_lengths is None else "fixed"
        self.max_abs = None

    def wait(self):
        if self._event is not None:
            self._event.synchronize()
            self._event = None
            self.max_abs = self._host_max.numpy()[:len(self.n_samples)]
        return self

    def frames(self, b):
        """The frames of item b (a numpy view of the pinned buffer)."""
        self.wait()
        return self._host.numpy()[self.offsets[b]:self.offsets[b + 1]]

    def frame_lengths(self, b):
        """The lengths of the compressed frames of item b; None for uncompressed frames (``frame_layout`` has those)."""
        if self._lengths is None:
            return None
        return self._lengths[self._bounds[b]:self._bounds[b + 1]]

    def pcm(self, b):
        """The int16 samples the compressed frames of item b hold; None for uncompressed frames (they hold them as they are)."""
        if self._pcm is None:
            return None
        self.wait()
        return self._pcm.numpy()[b, :self.n_samples[b]]

    def stream(self, b):
        """The whole FLAC stream of item b (``assemble``); only for an item whose max |x| is finite -- any other goes
        through the host writer, ``encode``."""
        return assemble(self.frames(b), self.n_samples[b], self.rate, frame_lengths=self.frame_lengths(b), pcm=self.pcm(b))

    def write(self, path, b):
        """``stream(b)`` into a file (``write_frames``: the frames are written as they are)."""
        return write_frames(path, self.frames(b), self.n_samples[b], self.rate, frame_lengths=self.frame_lengths(b),
                            pcm=self.pcm(b))


_device_tables = {}


def device_crc_tables(device):
    """``crc16_device_tables`` on the device (as int16 words), uploaded once per device."""
    import torch
    key = str(device)
    if key not in _device_tables:
        _device_tables[key] = torch.as_tensor(crc16_device_tables().view(np.int16)).to(device)
    return _device_tables[key]


def encode_device(audio, n_samples, rate, compression="verbatim", wait=True):
    """The FLAC frames (``encode`` of the item without its 42-byte header) and max |x| of every item audio[b, :n_samples[b]]
    of a float32 cuda batch (B, stride), encoded on the current stream of its device and copied into pinned host memory
    asynchronously.  ``n_samples``: host integers.  ``compression="verbatim"`` is mbx_encode_flac16; ``"fixed"`` is
    mbxf_encode_flac16_fixed (the bytes of ``encode(..., compression="fixed")``): frames packed densely, so their lengths come
    back first (the call waits for them) and say how many bytes to copy, and the int16 samples come along for the MD5.
    Returns an :class:`EncodedFlac`; with ``wait=False`` the copies may still be in flight."""
    import ctypes
    import torch
    from .abi import _check, load_library
    if compression not in COMPRESSIONS:
        raise ValueError(f"compression must be one of {COMPRESSIONS}, got {compression!r}")
    if not torch.is_tensor(audio) or audio.dim() != 2 or audio.dtype != torch.float32 or not audio.is_cuda:
        raise ValueError("audio must be a float32 cuda tensor (batch, stride)")
    dev = audio.device
    audio = audio.contiguous()
    B, stride = int(audio.shape[0]), int(audio.shape[1])
    counts = [int(nn) for nn in n_samples]
    if len(counts) != B:
        raise ValueError(f"n_samples must hold one count per item ({B})")
    rate = int(rate)
    capacity = sum(frames_bytes(nn) for nn in counts)            # the VERBATIM frames: no compressed frame is longer
    tables = device_crc_tables(dev)
    out = torch.empty(max(capacity, 1), dtype=torch.uint8, device=dev)
    max_abs = torch.empty(max(B, 1), dtype=torch.float32, device=dev)
    counts_c = (ctypes.c_int64 * max(B, 1))(*counts)
    lib = load_library()

    def to_host(src):
        host = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
        host.copy_(src, non_blocking=True)
        return host

    def record():
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(dev))
        return event

    # no handle, hence no device of its own: the launch goes to the CURRENT device, which must be the buffers'
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if compression == "verbatim":
            _check(lib.mbx_encode_flac16(audio.data_ptr(), stride, B, counts_c, rate, tables.data_ptr(), out.data_ptr(), capacity,
                                         max_abs.data_ptr(), stream))
            offsets = np.zeros(B + 1, dtype=np.int64)
            np.cumsum([frames_bytes(nn) for nn in counts], out=offsets[1:])
            res = EncodedFlac(to_host(out), offsets, to_host(max_abs), counts, rate, record())
        else:
            frame_counts = [-(-nn // BLOCK) for nn in counts]
            frames = sum(frame_counts)
            frame_bytes = torch.empty(max(frames, 1), dtype=torch.int32, device=dev)
            workspace = torch.empty(3 * frames + 1, dtype=torch.int64, device=dev)
            pcm = torch.empty((max(B, 1), max(stride, 1)), dtype=torch.int16, device=dev)
            _check(lib.mbxf_encode_flac16_fixed(audio.data_ptr(), stride, B, counts_c, rate, tables.data_ptr(), out.data_ptr(),
                                                capacity, frame_bytes.data_ptr(), workspace.data_ptr(), pcm.data_ptr(),
                                                max_abs.data_ptr(), stream))
            host_lengths = to_host(frame_bytes)
            first = record()
            host_pcm, host_max = to_host(pcm), to_host(max_abs)
            first.synchronize()                              # the lengths say how many bytes the frames take
            lengths = host_lengths.numpy()[:frames].astype(np.int64)
            used = int(lengths.sum())
            if used > capacity:
                raise RuntimeError("mbexwn_hip: the frame lengths exceed the output buffer")
            host = to_host(out[:max(used, 1)])
            bounds = np.zeros(B + 1, dtype=np.int64)
            np.cumsum(frame_counts, out=bounds[1:])
            offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)[bounds]
            res = EncodedFlac(host, offsets, host_max, counts, rate, record(), frame_lengths=lengths, frame_bounds=bounds,
                              pcm=host_pcm)
    return res.wait() if wait else res

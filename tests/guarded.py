"""Buffers between guard bands, for the memory contract of the C ABI (include/mbexwn.h: "the caller owns all buffers").

One ``torch.uint8`` allocation per buffer, laid out as [guard | payload | guard].  The payload starts 256-byte aligned and has
exactly the byte size the header states for that argument; each guard is 4 MiB.  That size is derived, not measured: the
largest single tile any kernel stores is 256 rows of the 2C-wide gate at C = 340, 256 x 680 x 4 B = 0.7 MB, so an overhang of
several tiles still lands in memory the test owns.  The point of the guards is that an overrun is observed, never that it
faults.

The whole allocation is filled before the call (the payload included: scratch a kernel must not rely on, output a kernel
must write), the inputs are copied into their payloads, and after the call ``check()`` compares both guards byte for byte
with the fill.  The fills:

    zero   0x00            the friendly content a fresh process sees
    nan    0xFF            NaN as float32, float16 and float64; survives a multiply by zero
    huge   float32 1e30    finite: survives fmaxf / fminf / clamps that swallow a NaN, overflows a sum

Works on CPU tensors (plain or pinned) and on device tensors alike."""
import numpy as np

GUARD_BYTES = 4 << 20
ALIGN = 256
FILLS = ("zero", "nan", "huge")
_PATTERN = {"zero": b"\x00\x00\x00\x00", "nan": b"\xff\xff\xff\xff", "huge": np.float32(1e30).tobytes()}


def fill_word(fill):
    """The fill as the int32 whose little-endian bytes repeat through the allocation."""
    return int(np.frombuffer(_PATTERN[fill], dtype="<i4")[0])


class GuardError(AssertionError):
    """A guard band changed; ``hits`` lists what ``Guarded.hits`` found."""

    def __init__(self, hits):
        self.hits = hits
        super().__init__("; ".join(
            f"{hh['name']}: {hh['count']} byte(s) changed {hh['side']} the payload, offsets {hh['first']} .. {hh['last']} "
            f"from the payload edge (fill {hh['fill']})" for hh in hits))


class Guarded:
    """``nbytes`` of payload between two guards inside one allocation on ``device`` (``pinned``: page-locked host memory)."""

    def __init__(self, name, nbytes, fill, device="cpu", pinned=False, guard_bytes=GUARD_BYTES):
        import torch
        assert fill in FILLS and nbytes >= 0 and guard_bytes % 4 == 0
        self.name, self.nbytes, self.fill = name, int(nbytes), fill
        total = (2 * guard_bytes + ALIGN + self.nbytes + 3) // 4 * 4
        if pinned:
            self.raw = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        else:
            self.raw = torch.empty(total, dtype=torch.uint8, device=device)
        base = self.raw.data_ptr()
        assert base % 4 == 0
        # the 4-byte pattern is anchored at the allocation's start; lead % 4 == 0, so a float32 payload reads whole words of it
        self.lead = guard_bytes + (-(base + guard_bytes)) % ALIGN
        assert self.lead % 4 == 0 and self.lead + self.nbytes + guard_bytes <= total
        self.refill()

    # -- layout
    @property
    def ptr(self):
        return self.raw.data_ptr() + self.lead

    @property
    def payload(self):
        return self.raw[self.lead:self.lead + self.nbytes]

    def view(self, dtype, *shape):
        out = self.payload.view(dtype)
        return out.view(*shape) if shape else out

    def refill(self, fill=None):
        """Fill the whole allocation, payload included."""
        import torch
        if fill is not None:
            assert fill in FILLS
            self.fill = fill
        self.raw.view(torch.int32).fill_(fill_word(self.fill))
        return self

    def put(self, data):
        """Copy ``data`` (tensor or array of exactly the payload's byte size) into the payload."""
        import torch
        src = data if torch.is_tensor(data) else torch.as_tensor(np.ascontiguousarray(data))
        src = src.contiguous().view(-1).view(torch.uint8)
        assert src.numel() == self.nbytes, f"{self.name}: {src.numel()} bytes for a payload of {self.nbytes}"
        self.payload.copy_(src)
        return self

    # -- checks
    def _changed(self, begin, end):
        """Bool tensor over the bytes [begin, end) of the allocation: differs from the fill."""
        import torch
        lo, hi = begin // 4 * 4, (end + 3) // 4 * 4
        words = self.raw[lo:hi].view(torch.int32) ^ fill_word(self.fill)
        return (words.view(torch.uint8) != 0)[begin - lo:end - lo]

    def hits(self, payload_bytes=None):
        """Changed guard bytes as a list of {name, side, first, last, count, fill}: ``front`` offsets are negative (-1 is the
        byte in front of the payload), ``behind`` offsets count from the first byte behind it.  ``payload_bytes`` < nbytes tells
        the checker that the payload ends earlier than it does (the detector's own test: everything stays in one allocation)."""
        import torch
        size = self.nbytes if payload_bytes is None else int(payload_bytes)
        assert 0 <= size <= self.nbytes
        out = []
        for side, begin, end, origin in (("front", 0, self.lead, self.lead),
                                         ("behind", self.lead + size, self.raw.numel(), self.lead + size)):
            idx = torch.nonzero(self._changed(begin, end)).view(-1)
            if idx.numel():
                out.append({"name": self.name, "side": side, "first": int(idx[0]) + begin - origin,
                            "last": int(idx[-1]) + begin - origin, "count": int(idx.numel()), "fill": self.fill})
        return out

    def check(self, payload_bytes=None):
        found = self.hits(payload_bytes)
        if found:
            raise GuardError(found)

    def payload_untouched(self):
        """True when every byte of the payload still holds the fill (a refused call must not have written anything)."""
        return not bool(self._changed(self.lead, self.lead + self.nbytes).any())


class GuardSet:
    """The guarded buffers of one call: ``new`` allocates, ``check`` holds every guard of every buffer."""

    def __init__(self, fill, device="cpu"):
        self.fill, self.device, self.buffers = fill, device, []

    def new(self, name, nbytes, data=None, pinned=False):
        buf = Guarded(name, nbytes, self.fill, device=self.device, pinned=pinned)
        if data is not None:
            buf.put(data)
        self.buffers.append(buf)
        return buf

    def put(self, name, data, pinned=False):
        """A guarded copy of an input: the payload is exactly the array's bytes."""
        arr = data if hasattr(data, "numel") else np.ascontiguousarray(data)
        nbytes = arr.numel() * arr.element_size() if hasattr(arr, "numel") else arr.nbytes
        return self.new(name, nbytes, data=arr, pinned=pinned)

    def check(self):
        found = [hh for buf in self.buffers for hh in buf.hits()]
        if found:
            raise GuardError(found)

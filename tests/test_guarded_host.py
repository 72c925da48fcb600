"""The guard-band helper of the memory-contract tests (tests/guarded.py) on CPU tensors: what it must report, and what not."""
import numpy as np
import pytest
import torch

from guarded import ALIGN, FILLS, GUARD_BYTES, GuardError, Guarded, GuardSet, fill_word


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nbytes", [0, 1, 4, 13, 4096, 100003])
def test_layout_fill_and_payload(fill, nbytes):
    buf = Guarded("x", nbytes, fill)
    assert buf.ptr % ALIGN == 0 and buf.payload.numel() == nbytes and (nbytes == 0 or buf.payload.data_ptr() == buf.ptr)
    assert buf.lead >= GUARD_BYTES and buf.raw.numel() - buf.lead - nbytes >= GUARD_BYTES
    assert buf.hits() == [] and buf.payload_untouched()
    words = buf.raw.view(torch.int32)
    assert bool((words == fill_word(fill)).all())
    if nbytes >= 4:
        as_float = buf.view(torch.float32)[:1] if nbytes % 4 == 0 else buf.payload[:4].clone().view(torch.float32)
        want = {"zero": 0.0, "nan": float("nan"), "huge": float(np.float32(1e30))}[fill]
        assert np.array_equal(as_float.numpy(), np.asarray([want], dtype=np.float32), equal_nan=True)


def test_the_fills_poison_every_float_format():
    nan = Guarded("x", 64, "nan")
    assert bool(torch.isnan(nan.view(torch.float32)).all()) and bool(torch.isnan(nan.view(torch.float16)).all())
    assert bool(torch.isnan(nan.view(torch.float64)).all())
    huge = Guarded("x", 64, "huge").view(torch.float32)
    assert bool(torch.isfinite(huge).all()) and bool(torch.isinf(huge * huge).all()) and float(huge[0]) == float(np.float32(1e30))


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nbytes", [16, 13, 4099])
def test_one_byte_in_front_and_one_behind_are_reported(fill, nbytes):
    buf = Guarded("victim", nbytes, fill)
    other = 0x5A                                   # no byte of any fill pattern
    buf.raw[buf.lead - 1] = other
    assert buf.hits() == [{"name": "victim", "side": "front", "first": -1, "last": -1, "count": 1, "fill": fill}]
    buf.refill()
    buf.raw[buf.lead + nbytes] = other
    assert buf.hits() == [{"name": "victim", "side": "behind", "first": 0, "last": 0, "count": 1, "fill": fill}]
    with pytest.raises(GuardError, match="victim: 1 byte.s. changed behind the payload, offsets 0 .. 0"):
        buf.check()
    buf.refill()
    buf.raw[0] = other                             # the far ends of both guards
    buf.raw[-1] = other
    buf.raw[buf.lead + nbytes + 7] = other
    found = {hh["side"]: hh for hh in buf.hits()}
    assert (found["front"]["first"], found["front"]["last"], found["front"]["count"]) == (-buf.lead, -buf.lead, 1)
    assert (found["behind"]["first"], found["behind"]["last"], found["behind"]["count"]) == \
        (7, buf.raw.numel() - buf.lead - nbytes - 1, 2)


def test_a_write_inside_the_payload_is_not_reported():
    for fill in FILLS:
        buf = Guarded("x", 4096, fill)
        buf.payload[:] = 0x5A
        buf.payload[0] = 1
        buf.payload[-1] = 2
        assert buf.hits() == [] and not buf.payload_untouched()
        buf.check()
        buf.put(np.arange(1024, dtype=np.float32))
        assert np.array_equal(buf.view(torch.float32).numpy(), np.arange(1024, dtype=np.float32)) and buf.hits() == []


def test_a_write_that_equals_one_fill_shows_under_the_others():
    """A stray float32 0.0 behind the payload is invisible under the zero fill and four changed bytes under nan; under huge
    the bytes of 1e30 that are zero themselves stay unseen: the three fills together see every stray value."""
    zero_bytes = sum(bb == 0 for bb in np.float32(1e30).tobytes())
    for fill, count in (("zero", 0), ("nan", 4), ("huge", 4 - zero_bytes)):
        buf = Guarded("y", 400, fill)
        buf.raw[buf.lead + 400:buf.lead + 404] = 0
        found = buf.hits()
        assert sum(hh["count"] for hh in found) == count and all(hh["side"] == "behind" for hh in found)
    buf = Guarded("y", 400, "zero")                # and a stray NaN under the zero fill
    buf.raw[buf.lead - 4:buf.lead] = 0xFF
    assert buf.hits() == [{"name": "y", "side": "front", "first": -4, "last": -1, "count": 4, "fill": "zero"}]


def test_a_shorter_claimed_payload_turns_the_last_row_into_guard():
    cout = 7
    buf = Guarded("out", 5 * cout * 4, "nan")
    buf.put(np.arange(5 * cout, dtype=np.float32))
    assert buf.hits() == []
    found = buf.hits(payload_bytes=4 * cout * 4)
    assert found == [{"name": "out", "side": "behind", "first": 0, "last": cout * 4 - 1, "count": cout * 4, "fill": "nan"}]


def test_guard_set_names_the_buffer():
    gs = GuardSet("huge")
    a = gs.put("a", np.ones(10, dtype=np.float32))
    b = gs.new("b", 40)
    assert np.array_equal(a.view(torch.float32).numpy(), np.ones(10, dtype=np.float32)) and b.payload_untouched()
    gs.check()
    b.raw[b.lead + 40 + 3] = 0x5A
    with pytest.raises(GuardError) as err:
        gs.check()
    assert [hh["name"] for hh in err.value.hits] == ["b"] and err.value.hits[0]["first"] == 3

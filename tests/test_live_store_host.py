"""The ring store of the live streams (mbexwn_vocoder_amd/live.py::_RingStore) without the library and without a GPU: the
order in which it hands out slots, and what its growth does to the samples the rings hold (the tensor lives on the CPU)."""
import numpy as np

from mbexwn_vocoder_amd import live


def test_ring_store_hands_out_the_lowest_new_slot_and_a_released_one_first():
    store = live._RingStore(10, 2)
    assert (store.ring_samples, store.slots, store.rings) == (16, 0, None)
    assert [store.take() for _ in range(3)] == [0, 1, 2] and store.slots == 4          # 2 at first, then doubling
    store.release(0)
    assert [store.take() for _ in range(3)] == [0, 3, 4] and store.slots == 8
    store.release(3)
    store.release(1)
    assert [store.take() for _ in range(4)] == [1, 3, 5, 6] and store.slots == 8       # the last one released goes first
    assert live._RingStore(16, 0).take() == 0                                          # at least one slot


def test_ring_store_moves_a_wrapped_span_to_the_longer_ring():
    """A ring of 8 samples that holds the samples [5, 13) of its stream (they wrap) becomes one of 32: sample s moves from
    place s & 7 to place s & 31, held against a numpy ring written sample by sample.  The tensor lives on the CPU here."""
    import torch
    store = live._RingStore(8, 2)
    slot = [store.take(), store.take()][1]
    assert store.ensure("cpu", 8, ()) is True and tuple(store.rings.shape) == (2, 8)
    old = np.zeros(8, dtype=np.float32)
    for ss in range(5, 13):
        old[ss & 7] = ss + 0.5
    store.rings[slot] = torch.as_tensor(old)
    store.rings[0] = 99.0                                           # a fresh slot: another stream's samples, not held
    assert store.ensure("cpu", 8, [(slot, 13)]) is False            # nothing to do: nothing allocated
    store.take()
    assert store.ensure("cpu", 8, [(slot, 13)]) is True and tuple(store.rings.shape) == (4, 8)     # more slots: rows copied
    assert np.array_equal(store.rings[slot].numpy(), old) and np.all(store.rings[2:].numpy() == 0)
    assert store.ensure("cpu", 20, [(slot, 13)]) is True and store.ring_samples == 32
    want = np.zeros((4, 32), dtype=np.float32)
    for ss in range(5, 13):
        want[slot, ss & 31] = ss + 0.5
    assert np.array_equal(store.rings.numpy(), want)
    # a stream of 40 samples so far has the newest 32 of them in the ring: whatever lies at s & 31 is sample s, 8 <= s < 40
    ring32, want = want[slot], np.zeros((4, 64), dtype=np.float32)
    assert store.ensure("cpu", 33, [(slot, 40)]) is True and store.ring_samples == 64
    for ss in range(8, 40):
        want[slot, ss & 63] = ring32[ss & 31]
    assert want[slot, 37] == 5.5 and want[slot, 12] == 12.5 and want[slot, 5] == 0
    assert np.array_equal(store.rings.numpy(), want)

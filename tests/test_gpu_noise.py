"""Keyed noise on the GPU: mbxn_fill_normal (csrc/noise_keyed.hip) against the host mirror's float64 evaluation, windows
against the whole fill bit for bit, and what the kernel must leave untouched."""
import ctypes

import numpy as np
import pytest

from mbexwn_vocoder_amd import noise

pytestmark = pytest.mark.gpu
SENTINEL = -12345.5
STRIDE = 4100
COUNTS = [0, 1, 3, 4, 5, 1023, 4096, 4099]
BIG = (1 << 34) + 3                           # a first step whose quads have a non-zero high counter word


@pytest.fixture(scope="module")
def lib():
    from mbexwn_vocoder_amd import engine
    from mbexwn_vocoder_amd.build import build_library
    build_library()
    return engine.load_library()


def fill(lib, keys, counts, first=None, stride=None, max_count=None, guard=64):
    """mbxn_fill_normal into a sentinel-filled buffer with `guard` floats in front of the first row and behind the last:
    returns (rows (B, stride) ndarray, front guard, back guard)."""
    import torch
    B = len(counts)
    stride = max(counts) if stride is None else stride
    max_count = max(counts) if max_count is None else max_count
    buf = torch.full((2 * guard + B * stride,), SENTINEL, dtype=torch.float32, device="cuda")
    keys_dev = torch.as_tensor(np.asarray(keys, dtype=np.uint64).reshape(B, 2).view(np.int64)).cuda()
    counts_dev = torch.as_tensor(np.asarray(counts, dtype=np.int32)).cuda()
    first_dev = None if first is None else torch.as_tensor(np.asarray(first, dtype=np.int64)).cuda()
    status = lib.mbxn_fill_normal(buf.data_ptr() + 4 * guard, stride, B, keys_dev.data_ptr(),
                                  None if first is None else first_dev.data_ptr(), counts_dev.data_ptr(), max_count,
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert status == 0, lib.mbx_last_error().decode()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    return host[guard:guard + B * stride].reshape(B, stride), host[:guard], host[guard + B * stride:]


def bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def port_error():
    """max |float32 port - float64 reference| over the 2^20 values of the bar's item: computed on the CPU from the mirror,
    before and independently of anything the device gives (1.1e-6 with numpy's float32 functions)."""
    nn = 1 << 20
    ref = noise.normals_reference(7, noise.item_key("a.wav"), 0, nn)
    return ref, float(np.max(np.abs(noise.normals_float32_port(7, noise.item_key("a.wav"), 0, nn) - ref)))


def test_device_normals_match_the_mirror(lib, port_error):
    """2^20 values of one item: |z - ref| <= max(8 x the float32 port's own error, 4e-6 max(1, |ref|)) against the float64
    evaluation of the mirror's uniforms.  A wrong word, lane, key or counter would miss by the order of 1, so this is also
    the test of the integer part through the kernel.  The 8 x is there because the device's logf and cosf are allowed a few
    ulp where numpy's are near one."""
    ref, port = port_error
    nn = ref.size
    rows, front, back = fill(lib, [[7, noise.item_key("a.wav")]], [nn])
    got = rows[0].astype(np.float64)
    err = np.abs(got - ref)
    bar = np.maximum(8 * port, 4e-6 * np.maximum(1.0, np.abs(ref)))
    print(f"keyed noise: max |z - ref| {err.max():.3e}, float32 port {port:.3e}, ratio {err.max() / port:.2f}, "
          f"worst err / bar {np.max(err / bar):.3f}")
    assert np.all(np.isfinite(got)) and np.all(err <= bar)
    assert np.all(front == SENTINEL) and np.all(back == SENTINEL)
    assert abs(got.mean()) < 0.005 and abs(got.var() - 1) < 0.01


@pytest.mark.parametrize("guard", [64, 61])               # rows 16-byte aligned, and not
def test_ragged_batch_writes_its_counts_and_nothing_else(lib, port_error, guard):
    """Counts {0, 1, 3, 4, 5, 1023, 4096, 4099} at stride 4100, one row from step 2^34 + 3, and a row with a negative first
    step: row b holds counts[b] values of its own item, the values behind them, the skipped row and the guard words keep
    the sentinel."""
    counts = COUNTS + [100]
    keys = [[5, 100 + bb] for bb in range(len(counts))]
    first = [0, 0, 0, 2, 0, 1, BIG, 0, -1]
    rows, front, back = fill(lib, keys, counts, first=first, stride=STRIDE, guard=guard)
    assert np.all(front == SENTINEL) and np.all(back == SENTINEL)
    bar = 8 * port_error[1]
    for bb, (cc, ff) in enumerate(zip(counts, first)):
        if ff < 0:
            assert np.all(rows[bb] == SENTINEL)
            continue
        assert np.all(rows[bb, cc:] == SENTINEL), bb
        ref = noise.normals_reference(5, 100 + bb, ff, cc)
        assert np.all(np.abs(rows[bb, :cc] - ref) <= np.maximum(bar, 4e-6 * np.maximum(1.0, np.abs(ref)))), bb
    # a count above max_count or the stride is clamped: the grid covers max_count values
    rows, front, back = fill(lib, [[5, 107]], [1 << 20], stride=STRIDE, max_count=4099, guard=guard)
    assert np.all(rows[0, 4099:] == SENTINEL) and np.all(back == SENTINEL) and not np.any(rows[0, :4099] == SENTINEL)


@pytest.mark.parametrize("base", [0, BIG])
def test_window_equals_whole(lib, base):
    """Sub-windows [a, a + n), a in {1, 2, 3, 4, 4095, 4097}, n in {1, 2, 7, 130}, refilled in one ragged batch (and each
    row at another alignment): bit for bit the slices of the whole fill, wherever a window starts or ends inside a quad or a
    tile."""
    whole = fill(lib, [[9, 77]], [4352], first=[base])[0][0]
    windows = [(aa, nn) for aa in (1, 2, 3, 4, 4095, 4097) for nn in (1, 2, 7, 130)]
    for stride, guard in ((130, 64), (131, 61)):
        rows, front, back = fill(lib, [[9, 77]] * len(windows), [nn for _, nn in windows], first=[base + aa for aa, _ in windows],
                                 stride=stride, guard=guard)
        assert np.all(front == SENTINEL) and np.all(back == SENTINEL)
        for row, (aa, nn) in zip(rows, windows):
            assert np.array_equal(bits(row[:nn]), bits(whole[aa:aa + nn])), (aa, nn, stride)
            assert np.all(row[nn:] == SENTINEL)
    # the ragged whole fills themselves: a row of any count is the head of the whole
    rows = fill(lib, [[9, 77]] * len(COUNTS), COUNTS, first=[base] * len(COUNTS), stride=STRIDE)[0]
    for row, cc in zip(rows, COUNTS):
        assert np.array_equal(bits(row[:cc]), bits(whole[:cc]))
    # another seed or key is another stream
    other = fill(lib, [[9, 78], [10, 77]], [64, 64], first=[base, base])[0]
    assert not np.array_equal(other[0], whole[:64]) and not np.array_equal(other[1], whole[:64])


def test_engine_keyed_noise(lib):
    """MBExWNEngine.keyed_noise: (B, max count) with zeros behind each count, the rows of the direct call."""
    import torch
    from mbexwn_vocoder_amd.engine import MBExWNEngine

    class Bare(MBExWNEngine):                                # the method needs the library, a device and a stream only
        def __init__(self):
            self._torch, self._lib, self.device = torch, lib, torch.device("cuda", torch.cuda.current_device())
            self._handle = None

    eng = Bare()
    out = eng.keyed_noise(3, [11, 12, 13], [40, 0, 4097], first_step=[5, 0, BIG]).cpu().numpy()
    assert out.shape == (3, 4097) and np.all(out[0, 40:] == 0) and np.all(out[1] == 0)
    want = fill(lib, [[3, 11], [3, 13]], [40, 4097], first=[5, BIG])[0]
    assert np.array_equal(bits(out[0, :40]), bits(want[0, :40])) and np.array_equal(bits(out[2]), bits(want[1]))
    assert np.array_equal(bits(eng.keyed_noise([3, 3, 3], [11, 12, 13], [40, 0, 4097], [5, 0, BIG]).cpu().numpy()), bits(out))
    assert tuple(eng.keyed_noise(3, [], []).shape) == (0, 0) and tuple(eng.keyed_noise(3, [1], [0]).shape) == (1, 0)
    with pytest.raises(ValueError):
        eng.keyed_noise(3, [1, 2], [4])
    with pytest.raises(ValueError):
        eng.keyed_noise(3, [1], [4], first_step=[-1])


def test_fill_normal_device_needs_no_engine(lib, port_error):
    """noise.fill_normal_device on its own: counts (0, 1, 5) from the steps (0, 3, 2^32 + 1) under two seeds -- (B, max count)
    with zeros behind each count, the bits of the direct call (as test_engine_keyed_noise asks of the method), and within the
    bar of test_device_normals_match_the_mirror of the host mirror's float64 values."""
    counts, first, seeds, keys = [0, 1, 5], [0, 3, 2 ** 32 + 1], [3, 4, 3], [11, 12, 13]
    out = noise.fill_normal_device(seeds, keys, counts, first_step=first).cpu().numpy()
    assert out.shape == (3, 5) and out.dtype == np.float32 and np.all(out[0] == 0) and np.all(out[1, 1:] == 0)
    want = fill(lib, [[ss, kk] for ss, kk in zip(seeds, keys)], counts, first=first, stride=5)[0]
    for bb, (ss, kk, cc, ff) in enumerate(zip(seeds, keys, counts, first)):
        assert np.array_equal(bits(out[bb, :cc]), bits(want[bb, :cc])), bb
        ref = noise.normals_reference(ss, kk, ff, cc)
        assert np.all(np.abs(out[bb, :cc] - ref) <= np.maximum(8 * port_error[1], 4e-6 * np.maximum(1.0, np.abs(ref)))), bb
    assert not np.array_equal(out[2], noise.fill_normal_device(4, keys, counts, first_step=first).cpu().numpy()[2])   # the seed counts
    import torch
    filled = noise.fill_normal_device(seeds, keys, counts, first_step=first, out=torch.zeros((3, 8), device="cuda")).cpu().numpy()
    assert np.array_equal(bits(filled[:, :5]), bits(out)) and np.all(filled[:, 5:] == 0)

"""Level control of whole items: ITU-R BS.1770 integrated loudness, sample and true peak, and one static gain per item, on
the host (numpy: the definition) and on the device (csrc/level.hip through ``mbxl_measure`` / ``mbxl_gains`` / ``mbxl_apply``
of include/mbexwn_level.h).  DESIGN.md section 6m.

THE DEFINITION.  Everything but the peaks and the applied gain is float64, every product and every sum rounded on its own
(no fused multiply-add).

  K-weighting at ``rate``: two biquads from their analogue prototypes through K = tan(pi f0 / rate) (:func:`k_weighting`;
    at 48 kHz the table of the standard to better than 1e-12).
  hop = floor(rate / 10 + 0.5) samples; an n-sample item has H = n // hop hops, the tail is not measured.  Hop h is filtered
    on its own: from zero state 2 * hop samples in front of its first sample (zeros in front of the item), each biquad in
    transposed direct form II on x = float64(sample)

        y = b0 * x + s1;   s1 = (b1 * x - a1 * y) + s2;   s2 = b2 * x - a2 * y

    the shelf feeding the high-pass; e[h] = sum of y^2 over the hop's own samples, ascending, from 0.  The warm-up makes the
    hops independent (under 1e-13 relative from filtering the whole item), which is the device's parallelism and keeps the
    bits independent of the batch.
  blocks of 400 ms, 75 % overlap: z[j] = (((e[j] + e[j+1]) + e[j+2]) + e[j+3]) / (4 * hop), j = 0 .. H - 4.
  gates: absolute z > ABS_GATE = 10^((-70 + 0.691) / 10); relative z > 0.1 * (ascending sum of the absolutely gated z /
    their number).  P = ascending sum of the z passing both / their number ``count``; count == 0 (an item under 0.4 s,
    silence): not measurable, P = 0.  Loudness = -0.691 + 10 log10 P (:func:`lufs`; host only).
  sample peak: max |x| as the maximum of the bit patterns (a NaN item shows as NaN); true peak: the maximum of the sample
    peak and max |y|, y the item at 4 * rate by the project's own resampler (resample.py; on the device the fmaf chain of
    csrc/resample_chain.h over all 4 n outputs, never stored; on the host ``resample_host``, which rounds once -- the
    device is held to ``resample_device``'s bits, the host function to the tolerance of its tests).
  gain (:func:`gain_host`): g = sqrt(Pt / P) for a target power Pt and a measurable item, else 1; if g * peak > ceiling then
    g = ceiling / peak; rounded to float32.  A NaN or zero peak: 1.  Output sample = float32(x) * g, one float32 product.

Live streams are out of scope: integrated loudness needs the whole item.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

ABS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)
SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196)     # f0, gain in dB, Q
SHELF_VB_EXP = 0.4996667741545416
HIGH_PASS = (38.13547087602444, 0.5003270373238773)                     # f0, Q
DEFAULT_PEAK_LIMIT = -1.0   # dBFS: the ceiling a loudness target comes with when none is given
RECORD_WORDS = 6            # int32 words of a device record: P (float64), count, n_abs, sample peak, true peak (float32)


def k_weighting(rate):
    """The ten float64 coefficients at ``rate``: b0 b1 b2 a1 a2 of the shelf, then of the high-pass."""
    rate = float(rate)
    if not np.isfinite(rate) or rate <= 0:
        raise ValueError(f"k_weighting: the rate must be positive, got {rate!r}")
    f0, gain, q = SHELF
    k = np.tan(np.pi * f0 / rate)
    vh = 10.0 ** (gain / 20.0)
    vb = vh ** SHELF_VB_EXP
    a0 = 1.0 + k / q + k * k
    shelf = [(vh + vb * k / q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0,
             2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0]
    f0, q = HIGH_PASS
    k = np.tan(np.pi * f0 / rate)
    a0 = 1.0 + k / q + k * k
    high = [1.0, -2.0, 1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0]
    return np.asarray(shelf + high, dtype=np.float64)


def hop_samples(rate):
    """Samples of a 100 ms hop: floor(rate / 10 + 0.5)."""
    return int(np.floor(float(rate) / 10.0 + 0.5))


def lufs(power):
    """-0.691 + 10 log10 P; -inf for P = 0 (not measurable)."""
    power = np.asarray(power, dtype=np.float64)
    with np.errstate(divide="ignore"):
        out = -0.691 + 10.0 * np.log10(power)
    return float(out) if out.ndim == 0 else out


def target_power(loudness):
    """The P of a loudness in LUFS: 10^((LUFS + 0.691) / 10)."""
    return float(10.0 ** ((float(loudness) + 0.691) / 10.0))


def hop_energies_host(x, rate, coefs=None):
    """e[h] of the definition for a 1-D signal: float64 (n // hop,), vectorised over the hops.  ``coefs``: ten coefficients
    in place of ``k_weighting(rate)`` (the device takes any two biquads)."""
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("hop_energies_host: a 1-D signal is expected")
    hop = hop_samples(rate)
    if hop < 1:
        raise ValueError(f"hop_energies_host: the rate {rate!r} gives no hop")
    hops = x.size // hop
    if hops == 0:
        return np.zeros(0, dtype=np.float64)
    coef = k_weighting(rate) if coefs is None else np.asarray(coefs, dtype=np.float64).reshape(10)
    padded = np.concatenate((np.zeros(2 * hop), x[:hops * hop].astype(np.float64)))
    # row h: the samples from 2 * hop in front of hop h to its end
    rows = np.lib.stride_tricks.as_strided(padded, shape=(hops, 3 * hop), strides=(hop * padded.strides[0], padded.strides[0]),
                                           writeable=False)
    b0, b1, b2, a1, a2 = coef[:5]
    c0, c1, c2, d1, d2 = coef[5:]
    s1, s2, t1, t2, e = (np.zeros(hops) for _ in range(5))
    for tt in range(3 * hop):
        xx = rows[:, tt]
        y = b0 * xx + s1
        s1 = (b1 * xx - a1 * y) + s2
        s2 = b2 * xx - a2 * y
        w = c0 * y + t1
        t1 = (c1 * y - d1 * w) + t2
        t2 = c2 * y - d2 * w
        if tt >= 2 * hop:
            e = e + w * w
    return e


def block_powers_host(e, hop):
    """z[j] of the definition from the hop energies: float64 (max(0, H - 3),)."""
    e = np.asarray(e, dtype=np.float64)
    if e.size < 4:
        return np.zeros(0, dtype=np.float64)
    return (((e[:-3] + e[1:-2]) + e[2:-1]) + e[3:]) / float(4 * hop)


def _ascending_mean(values):
    total = 0.0
    for vv in values:
        total = total + float(vv)
    return total / len(values)


def gate_host(z):
    """(P, count, n_abs) of the definition from the block powers."""
    z = np.asarray(z, dtype=np.float64)
    loud = z[z > ABS_GATE]
    if loud.size == 0:
        return 0.0, 0, 0
    threshold = 0.1 * _ascending_mean(loud)
    kept = loud[loud > threshold]
    if kept.size == 0:
        return 0.0, 0, int(loud.size)
    return _ascending_mean(kept), int(kept.size), int(loud.size)


def bits_peak(x):
    """max |x| of float32 samples as the maximum of the bit patterns: float32; 0 for no samples, NaN for a NaN item."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.size == 0:
        return np.float32(0.0)
    return np.abs(x).view(np.uint32).max().view(np.float32)


@dataclass
class Measure:
    """What a measurement says of one item.  ``power``: P; ``count``: blocks behind it (0: not measurable); ``n_abs``: blocks
    that passed the absolute gate; ``sample_peak`` / ``true_peak``: float32 (``true_peak`` is the sample peak where no true
    peak was asked for); ``energies`` / ``blocks``: e and z."""
    power: float
    count: int
    n_abs: int
    sample_peak: np.float32
    true_peak: np.float32
    energies: np.ndarray = None
    blocks: np.ndarray = None

    @property
    def lufs(self):
        return lufs(self.power) if self.count else float("-inf")

    def peak(self, true_peak=False):
        return self.true_peak if true_peak else self.sample_peak


def measure_host(x, rate, true_peak=False):
    """The :class:`Measure` of a 1-D signal at ``rate``."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 1:
        raise ValueError("measure_host: a 1-D signal is expected")
    rate = int(round(rate))
    e = hop_energies_host(x, rate)
    z = block_powers_host(e, hop_samples(rate))
    power, count, n_abs = gate_host(z)
    peak = bits_peak(x)
    over = peak
    if true_peak and x.size:
        from .resample import resample_host
        over = np.maximum(peak, bits_peak(resample_host(x, rate, 4 * rate))) if not np.isnan(peak) else peak
    return Measure(power, count, n_abs, peak, np.float32(over), e, z)


def gain_host(power, count, peak, target=None, ceiling=None):
    """(gain as float32, whether the ceiling set it) of the definition.  ``target``: a power Pt or None; ``ceiling``: linear
    or None; ``peak``: the item's sample or true peak."""
    peak = float(peak)
    if np.isnan(peak) or peak == 0.0:
        return np.float32(1.0), False
    gain = 1.0
    if target is not None and count > 0 and power > 0 and target > 0:
        gain = float(np.sqrt(np.float64(target) / np.float64(power)))
    limited = False
    if ceiling is not None and gain * peak > float(ceiling):
        gain, limited = float(ceiling) / peak, True
    return np.float32(gain), limited


def ceiling_linear(dbfs):
    """A ceiling in dBFS as a linear value; None stays None."""
    return None if dbfs is None else float(10.0 ** (float(dbfs) / 20.0))


class LevelControl:
    """What ``run_micro_batches(level=)`` takes.  ``target``: None, a loudness in LUFS, or a list with one entry per item of
    the job -- a target POWER (the P of a source) or None; ``peak_limit``: the ceiling in dBFS or None; ``true_peak``: the
    ceiling and the reported peak are about the 4x true peak; ``limiter``: the ceiling is kept by the look-ahead limiter
    (limiter.py) with the window ``lookahead_ms`` / ``hold_ms``, and the loudness gain stands.  All go
    through :func:`check_options`."""

    def __init__(self, target=None, peak_limit=None, true_peak=False, limiter=False, lookahead_ms=None, hold_ms=None):
        self.target, self.peak_limit, self.true_peak = check_options(target, peak_limit, true_peak, limiter=limiter,
                                                                     lookahead_ms=lookahead_ms, hold_ms=hold_ms)
        self.limiter, self.lookahead_ms, self.hold_ms = bool(limiter), lookahead_ms, hold_ms       # None: limiter.window's default

    def window(self, rate):
        """(h, H) of the limiter at ``rate`` (``limiter.window``: ValueError for a hold shorter than half the look-ahead)."""
        from .limiter import window
        return window(rate, self.lookahead_ms, self.hold_ms)

    def check_rates(self, rates):
        """ValueError when the limiter's window is refused at one of the rates a job writes at: before anything runs."""
        if self.limiter:
            from .limiter import check_rates
            check_rates(rates, self.lookahead_ms, self.hold_ms, self.true_peak)

    def sliced(self, indices):
        """The control of the items ``indices`` of the job: a per-item target list is cut, everything else is kept."""
        target = [self.target[ii] for ii in indices] if isinstance(self.target, (list, tuple)) else self.target
        return LevelControl(target, self.peak_limit, self.true_peak, self.limiter, self.lookahead_ms, self.hold_ms)

    def powers(self, indices):
        """The target power (or None) of the items ``indices``."""
        if self.target is None:
            return [None] * len(indices)
        if isinstance(self.target, float):
            return [target_power(self.target)] * len(indices)
        return [None if self.target[ii] is None or not self.target[ii] > 0 else float(self.target[ii]) for ii in indices]


def check_options(loudness=None, peak_limit=None, true_peak=False, allow_input=False, limiter=False, lookahead_ms=None,
                  hold_ms=None):
    """THE validation of the public options, of the tools and of the methods: ``(loudness, peak_limit, true_peak)``
    with the default ceiling filled in -- ``DEFAULT_PEAK_LIMIT`` dBFS with a loudness, none without.  ``loudness``: None, a
    finite number of LUFS, a list of per-item target powers, or -- ``allow_input``, for a caller that has source sounds --
    the word "input".  ValueError for anything else, for a peak limit that is not finite, and for ``true_peak`` (--true-peak)
    without a peak to limit.  ``limiter`` (--limiter) comes with the default ceiling too, with or without a loudness; its
    window ``lookahead_ms`` / ``hold_ms`` (None: not given, ``limiter.window`` fills in 1.5 / 20) is an error without it and
    must be finite and positive with it (the hold against the look-ahead, and the window against the device, are checked at
    the rates of the job: ``LevelControl.check_rates``)."""
    given = [name for name, value in (("lookahead_ms", lookahead_ms), ("hold_ms", hold_ms)) if value is not None]
    if given and not limiter:
        raise ValueError(f"{' and '.join(given)} shape the limiter's window: give limiter (--limiter) too")
    if limiter:
        for name, value in (("lookahead_ms", lookahead_ms), ("hold_ms", hold_ms)):
            if value is not None and not (isinstance(value, (int, float)) and np.isfinite(value) and value > 0):
                raise ValueError(f"limiter: {name} must be a finite positive number of ms, got {value!r}")
    if isinstance(loudness, str):
        if loudness != "input" or not allow_input:
            raise ValueError("loudness is a number of LUFS" + (" or 'input'" if allow_input else "") + f", got {loudness!r}")
    elif isinstance(loudness, (list, tuple)):
        loudness = list(loudness)
    elif loudness is not None:
        loudness = float(loudness)
        if not np.isfinite(loudness):
            raise ValueError(f"loudness must be a finite number of LUFS, got {loudness!r}")
    if peak_limit is not None:
        peak_limit = float(peak_limit)
        if not np.isfinite(peak_limit):
            raise ValueError(f"peak_limit must be a finite number of dBFS, got {peak_limit!r}")
    if loudness is None and peak_limit is None and true_peak and not limiter:
        raise ValueError("true_peak (--true-peak) chooses the peak of a peak limit or a loudness: give one of them")
    if (loudness is not None or limiter) and peak_limit is None:
        peak_limit = DEFAULT_PEAK_LIMIT
    return loudness, peak_limit, bool(true_peak)


def level_control(loudness=None, peak_limit=None, true_peak=False, limiter=False, lookahead_ms=None, hold_ms=None):
    """The :class:`LevelControl` of the public options (:func:`check_options`), or None when none is given."""
    loudness, peak_limit, true_peak = check_options(loudness, peak_limit, true_peak, limiter=limiter,
                                                    lookahead_ms=lookahead_ms, hold_ms=hold_ms)
    if loudness is None and peak_limit is None:
        return None
    return LevelControl(loudness, peak_limit, true_peak, limiter, lookahead_ms, hold_ms)


# ------------------------------------------------------------------------------------------------
# the device stage: what is small -- lengths, hops, coefficient rows, target powers, the gate and the ceiling -- goes to the
# library as host arrays and travels in the kernel arguments, so that nothing is uploaded behind the work already enqueued
# (an upload from pageable memory would wait for the stream)
# ------------------------------------------------------------------------------------------------
@lru_cache(maxsize=64)
def _rate_coefficients(rate):
    return k_weighting(rate)


class DeviceMeasure:
    """What :func:`measure_device` enqueued: ``records`` int32 (B, 6) -- per item P as float64 in words 0-1, count, n_abs,
    the sample peak and the true peak as float32 bits -- and ``workspace`` float64 (B, 2, hops_cap): e, then z.  All on the
    device; :meth:`host` copies and waits."""

    def __init__(self, records, workspace, n_samples, hops, true_peak):
        self.records, self.workspace = records, workspace
        self.n_samples, self.hops, self.true_peak = list(n_samples), list(hops), true_peak

    @staticmethod
    def unpack(words, b):
        """(P, count, n_abs, sample peak, true peak) of item b from host records (numpy int32 (B, 6))."""
        row = np.ascontiguousarray(words[b])
        return (float(row[:2].view(np.float64)[0]), int(row[2]), int(row[3]), row[4:5].view(np.float32)[0],
                row[5:6].view(np.float32)[0])

    def host(self, details=True):
        """One :class:`Measure` per item (waits for the stream)."""
        words = self.records.cpu().numpy()
        work = self.workspace.cpu().numpy() if details else None
        out = []
        for b, (nn, hop) in enumerate(zip(self.n_samples, self.hops)):
            hops = nn // hop
            mm = Measure(*self.unpack(words, b))
            if details:
                mm.energies, mm.blocks = work[b, 0, :hops].copy(), work[b, 1, :max(0, hops - 3)].copy()
            out.append(mm)
        return out


def _check_audio(audio, n_samples, who):
    import torch
    if not torch.is_tensor(audio) or audio.dim() != 2 or audio.dtype != torch.float32 or not audio.is_cuda:
        raise ValueError(f"{who}: audio must be a float32 cuda tensor (batch, stride)")
    if not audio.is_contiguous():
        raise ValueError(f"{who}: audio must be contiguous")
    counts = [int(nn) for nn in n_samples]
    if len(counts) != int(audio.shape[0]):
        raise ValueError(f"{who}: n_samples must hold one count per item ({int(audio.shape[0])})")
    return counts


def measure_device(audio, n_samples, rates, true_peak=False, coefs=None):
    """The measure of every item audio[b, :n_samples[b]] of a float32 cuda batch (B, stride) at ``rates`` (one rate, or one
    per item), enqueued on the current stream of its device: nothing is uploaded behind the enqueued work and nothing is
    waited for.  ``n_samples``: host integers.  Returns a
    :class:`DeviceMeasure`.  ``coefs``: float64 (B, 10) rows in place of ``k_weighting`` of the rates."""
    import ctypes
    import torch
    from .abi import _check, load_library
    counts = _check_audio(audio, n_samples, "measure_device")
    B, stride, dev = int(audio.shape[0]), int(audio.shape[1]), audio.device
    rates = [int(round(rates))] * B if np.isscalar(rates) else [int(round(rr)) for rr in rates]
    if len(rates) != B:
        raise ValueError(f"measure_device: rates must be one rate or one per item ({B})")
    hops = [hop_samples(rr) for rr in rates]
    if any(hh < 1 for hh in hops):
        raise ValueError("measure_device: every rate must be at least 5 Hz")
    hops_cap = max([1] + [nn // hh for nn, hh in zip(counts, hops)])
    if B == 0 or stride == 0:                              # nothing to measure (and no buffer to point at)
        return DeviceMeasure(torch.zeros((B, RECORD_WORDS), dtype=torch.int32, device=dev),
                             torch.zeros((B, 2, hops_cap), dtype=torch.float64, device=dev), counts, hops, bool(true_peak))
    records = torch.empty((B, RECORD_WORDS), dtype=torch.int32, device=dev)
    workspace = torch.empty((B, 2, hops_cap), dtype=torch.float64, device=dev)
    if coefs is None:
        coefs = np.stack([_rate_coefficients(rr) for rr in rates])
    coefs = np.ascontiguousarray(coefs, dtype=np.float64).reshape(B, 10)
    taps, n_taps = None, 0
    if true_peak:
        from .resample import device_taps
        # up = 4, down = 1 and the design depends on the ratio alone: one set serves every rate
        # (they are uploaded once per device, by the first call that asks for them)
        taps, up, down = device_taps(rates[0], 4 * rates[0], dev)
        assert (up, down) == (4, 1)
        n_taps = int(taps.numel())
    counts_c = (ctypes.c_int64 * B)(*counts)
    hops_c = (ctypes.c_int32 * B)(*hops)
    gate = ctypes.c_double(ABS_GATE)
    with torch.cuda.device(dev):
        _check(load_library().mbxl_measure(audio.data_ptr(), stride, B, counts_c, hops_c,
                                           coefs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(gate),
                                           taps.data_ptr() if taps is not None else None, n_taps, workspace.data_ptr(),
                                           hops_cap, records.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return DeviceMeasure(records, workspace, counts, hops, bool(true_peak))


def gains_device(measure, targets=None, target_records=None, ceiling=None, true_peak=False):
    """float32 (B,) gains on the device from a :class:`DeviceMeasure`: enqueued only, nothing uploaded, nothing waited for
    (the records stay on the device, the targets travel in the kernel arguments).  ``targets``: None, one power,
    or per item a power or None; ``target_records``: None, or another DeviceMeasure (or its ``records``) of B items -- item
    b then takes the P of record b as its target where that record is measurable, and no target where it is not, whatever
    ``targets`` says; ``ceiling``: linear or None; ``true_peak``: the ceiling is about the true peak."""
    import ctypes
    import torch
    from .abi import _check, load_library
    records = measure.records if isinstance(measure, DeviceMeasure) else measure
    B, dev = int(records.shape[0]), records.device
    if targets is None or np.isscalar(targets):
        targets = [targets] * B
    if len(targets) != B:
        raise ValueError(f"gains_device: targets must be one power or one per item ({B})")
    powers = (ctypes.c_double * max(B, 1))(*[0.0 if tt is None or not tt > 0 else float(tt) for tt in targets])
    other = None
    if target_records is not None:
        other = target_records.records if isinstance(target_records, DeviceMeasure) else target_records
        if tuple(other.shape) != tuple(records.shape) or other.device != dev:
            raise ValueError("gains_device: target_records must hold one record per item on the same device")
    gains = torch.empty((max(B, 1),), dtype=torch.float32, device=dev)
    limit = None if ceiling is None else ctypes.byref(ctypes.c_double(float(ceiling)))
    with torch.cuda.device(dev):
        _check(load_library().mbxl_gains(records.data_ptr(), B, powers, other.data_ptr() if other is not None else None,
                                         limit, int(bool(true_peak)), gains.data_ptr(),
                                         torch.cuda.current_stream(dev).cuda_stream))
    return gains[:B]


def apply_device(audio, n_samples, gains, out=None):
    """Item b times gains[b] over [0, n_samples[b]): in place (``out`` None) or into ``out`` (B, any stride >= the longest
    item).  Nothing behind an item's end is read or written.  Returns the tensor written."""
    import ctypes
    import torch
    from .abi import _check, load_library
    counts = _check_audio(audio, n_samples, "apply_device")
    B, dev = int(audio.shape[0]), audio.device
    out = audio if out is None else out
    _check_audio(out, n_samples, "apply_device (out)")
    if out.device != dev:
        raise ValueError("apply_device: out must be on the device of audio")
    if gains.dtype != torch.float32 or tuple(gains.shape) != (B,) or gains.device != dev or not gains.is_contiguous():
        raise ValueError("apply_device: gains must be a contiguous float32 tensor (batch,) on the device of audio")
    if B == 0 or max(counts) == 0:                          # nothing to multiply (and maybe no buffer to point at)
        return out
    counts_c = (ctypes.c_int64 * B)(*counts)
    with torch.cuda.device(dev):
        _check(load_library().mbxl_apply(audio.data_ptr(), int(audio.shape[1]), B, counts_c, gains.data_ptr(), out.data_ptr(),
                                         int(out.shape[1]), torch.cuda.current_stream(dev).cuda_stream))
    return out

"""Live streams: audio in, audio out.

``StreamingAnalyzer`` is the mel analysis of ``analysis.compute_log_mel_device`` for sounds that are still arriving: every
stream keeps its recent samples in a ring on the device (csrc/mel_stream.hip, include/mbexwn_live.h) and a frame is computed
as soon as the samples of its window are there -- with exactly the bits the offline analysis gives that frame on the whole
sound, however the sound was cut into pushes.  ``LiveResynthesizer`` joins it to ``MELInverter.scale_mel`` and a
``StreamingSynthesizer``: the promise of the synthesis streams, "a stream equals the offline run, bit for bit", reaches back
to the microphone.

A stream opened with ``sample_rate=R`` takes its pushes at R Hz: a streaming form of the reference's resampler
(csrc/resample_stream.hip, include/mbexwn_live_resample.h) writes the model-rate samples straight into the ring the analysis
reads, with the bits ``resample.resample_device`` gives on the whole sound, so the promise does not end at a resampler of
the caller's.  Streams opened without a rate run exactly what they ran before.

On the way out, a stream opened with ``output_rate=R`` gets its audio at R Hz: ``StreamingOutputResampler`` runs the same
chain from a ring of the synthesizer's model-rate samples into packed rows (include/mbexwn_live_out.h), with the bits
``resample.resample_device`` gives on the stream's whole synthesis.  Streams without an output rate get what they got.

The readiness rules (``frames_ready``, ``outputs_ready``, ``input_keep_from``) and the mapping of per-push transposition
factors to mel frames (``FrameFactors``) are pure host logic and run without a device.
"""
import ctypes

import numpy as np

from .analysis import mel_analysis_tables, mell_header


def check_rate(sample_rate, model_rate, what="samples"):
    """A stream opened without a rate of its own, and a tool run without --resample, take input at the model's rate only."""
    if int(round(sample_rate)) != int(round(model_rate)):
        raise ValueError(f"{what} at {sample_rate} Hz: live streams take audio at the model rate {model_rate} Hz only; resample "
                         "first (bin/generate_mel.py does it for files, resample.resample_host for arrays)")


def frames_total(n_samples, hop):
    """Rows of the offline analysis of a sound of n_samples samples."""
    return n_samples // hop + 1


def frames_ready(have, hop, win, closed=False):
    """Frames of a stream that can be computed once ``have`` samples have arrived: frame t needs the samples in front of
    t * hop - win // 2 + win while the stream is open; a closed stream has all frames_total(have) frames (the end is
    reflected)."""
    if closed:
        return frames_total(have, hop)
    need = win - win // 2
    return 0 if have < need else (have - need) // hop + 1


def outputs_ready(have, up, down, half, closed=False):
    """Model-rate samples of a resampled stream that are final once ``have`` input samples have arrived: output k reads the
    input up to sample (k * down + half) // up, so while the stream is open it is final when k * down + half <=
    have * up - 1; a closed stream of ``have`` samples has all ceil(have * up / down) outputs (the tail of the filter is
    clipped at the end, as offline).  ``half`` is (n_taps - 1) // 2 of the stream's filter."""
    if closed:
        return -(-have * up // down)
    top = have * up - 1 - half
    return 0 if top < 0 else top // down + 1


def input_keep_from(k, up, down, half, n_taps):
    """First input sample output ``k`` of a resampled stream reads: with k the next output not yet produced, everything in
    front of it may leave the input ring."""
    return max(0, -(-(k * down + half - (n_taps - 1)) // up))


class FrameFactors:
    """Per-push transposition factors as per-frame factors: a factor given with a push applies to the mel frames whose
    centre sample t * hop lies in that push's sample range [start, start + count).  A sound whose length is a multiple of
    hop has one last frame centred on the sample behind its end: it takes the factor of the last non-empty push.

    ``up`` / ``down``: the pushes are counted at an input rate of down / up times the model rate (a resampled stream); the
    centre of frame t is then input sample (t * hop * down) // up, a push that ends after ``end`` input samples decides
    the frames in front of (end * up - 1) // (hop * down) + 1, and at the end the frames up to
    ceil(n * up / down) // hop + 1 that are still undecided (at most one) take the last push's factor."""

    def __init__(self, hop, up=1, down=1):
        self.hop, self.samples = int(hop), 0
        self.up, self.down = int(up), int(down)
        self._base, self._values, self._last = 0, [], 1.0

    @property
    def frames(self):
        """Frames whose factor is decided."""
        return self._base + len(self._values)

    def add(self, count, factor=None):
        factor = 1.0 if factor is None else float(factor)
        if count > 0:
            end = self.samples + int(count)
            self._values += [factor] * ((end * self.up - 1) // (self.hop * self.down) + 1 - self.frames)
            self.samples, self._last = end, factor

    def close(self):
        total = frames_total(-(-self.samples * self.up // self.down), self.hop)
        self._values += [self._last] * max(0, total - self.frames)

    def take(self, first, end):
        """Factors of the frames [first, end) as float32; frames in front of ``first`` are forgotten."""
        if first < self._base or end > self.frames:
            raise IndexError(f"frames [{first}, {end}) are not the decided frames [{self._base}, {self.frames})")
        out = np.asarray(self._values[first - self._base:end - self._base], dtype=np.float32)
        del self._values[:first - self._base]
        self._base = first
        return out


def frame_factors(pushes, hop, up=1, down=1):
    """``pushes``: (count, factor or None) per push of one whole stream -> the factor of each of its frames; with ``up`` /
    ``down`` the counts are input samples of a resampled stream."""
    ff = FrameFactors(hop, up, down)
    for count, factor in pushes:
        ff.add(count, factor)
    ff.close()
    return ff.take(0, frames_total(-(-ff.samples * ff.up // ff.down), hop))


def _pow2_at_least(n):
    out = 1
    while out < n:
        out *= 2
    return out


class _AStream:
    def __init__(self, slot, rate=None, in_slot=None, filt=None):
        self.slot = slot
        self.rate = rate          # None: pushes at the model rate; else the stream's own input rate
        self.in_slot = in_slot    # ... its slot in the input-rate ring store
        self.filt = filt          # ... and its filter: (up, down, half, n_taps)
        self.in_have = 0          # samples pushed at the stream's own rate (== have for a stream at the model rate)
        self.in_on_device = 0     # ... of which the input ring holds the newest (resampled streams only)
        self.have = 0             # model-rate samples so far: pushed, or final outputs of the resampler (outputs_ready)
        self.on_device = 0        # ... of which the ring holds [max(0, on_device - ring), on_device)
        self.emitted = 0          # frames handed out
        self.closed = False
        self.queue = []           # pushed since the last tick
        self.fresh = True         # the slot's ring still holds another stream's samples


class _RingStore:
    """One ring store of include/mbexwn_live.h: ``slots`` rings of ``ring_samples`` samples, a power of two.  It hands out
    slots -- ``first_slots`` at first, then doubling; the lowest new slot first, a released slot before any other -- and
    keeps the device tensor ``rings``, which follows lazily: ``ensure`` brings it up to date at the next tick."""

    def __init__(self, ring_samples, first_slots):
        self.ring_samples = _pow2_at_least(ring_samples)
        self.slots, self._first_slots, self._free = 0, max(1, int(first_slots)), []
        self.rings = None             # (slots, ring_samples) float32 on the device

    def take(self):
        if not self._free:
            n_new = max(self._first_slots, 2 * self.slots)
            self._free = list(range(n_new - 1, self.slots - 1, -1))
            self.slots = n_new
        return self._free.pop()

    def release(self, slot):
        self._free.append(slot)

    def ensure(self, device, ring_needed, held_spans):
        """``rings`` on ``device`` with a row per slot and rings of at least ``ring_needed`` samples (doubling).  When only the
        slot count grew the rows are copied over; when the ring lengthened, every (slot, hi) of ``held_spans`` -- the slot
        holds its stream's samples [max(0, hi - ring_samples), hi) -- moves to its place in the longer ring.
        -> whether it allocated."""
        import torch
        ring = self.ring_samples
        while ring < ring_needed:
            ring *= 2
        old = self.rings
        if old is not None and old.shape[0] >= self.slots and ring == self.ring_samples:
            return False
        new = torch.zeros((self.slots, ring), dtype=torch.float32, device=device)
        if old is not None and ring == self.ring_samples:
            new[:old.shape[0]] = old
        elif old is not None:
            for slot, hi in held_spans:
                idx = torch.arange(max(0, hi - self.ring_samples), hi, device=device)
                new[slot, idx & (ring - 1)] = old[slot, idx & (self.ring_samples - 1)]
        self.rings, self.ring_samples = new, ring
        return True


class StreamingAnalyzer:
    """Log-mel analysis of any number of concurrent streams, a tick at a time.

    The concatenated rows ``tick`` hands out for a stream are the rows [0, n // hop + 1) of ``compute_log_mel_device`` on the
    stream's whole sound (n samples), bit for bit, however the sound was cut into pushes.  Frame t is handed out by the
    first tick after t * hop - win // 2 + win samples have arrived; after ``push(..., last=True)`` the remaining frames
    follow, with the reflection at the end (as often as a stream shorter than half a window needs it).

    Samples must be at ``preprocess_config["sample_rate"]``, unless the stream was opened with a ``sample_rate`` of its own
    (below).  A steady tick costs one host-to-device copy (descriptors and samples packed in one pinned buffer), two
    launches and one copy back, and allocates no device memory: the stores grow by doubling when more streams are open than
    slots exist, when a tick carries more than any before it, and -- the rings -- when a stream's pushes would overwrite
    samples a pending frame still needs.  ``ring_samples`` (default 4 windows) and ``slots`` are the sizes the stores start
    from.

    ``open(stream_id, sample_rate=R)`` with R another rate than the model's gives a resampled stream: its pushes are at R
    and go to a slot of a second ring store, (slots, ``input_ring_samples``) at the input rate, from where the tick's
    ``mbxr_resample_rings`` launches (one per distinct rate among the streams with work) write every output that became
    final -- ``outputs_ready`` -- into the stream's model-rate ring.  Behind that ring nothing differs: the stream's
    model-rate length is the count of outputs produced, and the rows are those of ``generate_mels`` on the whole sound at R,
    bit for bit.  The input store grows as the other does; its rule is ``input_keep_from``.  A tick without resampled
    streams is the tick described above, launch for launch."""

    def __init__(self, preprocess_config, device=None, ring_samples=None, slots=16, input_ring_samples=None):
        cfg = preprocess_config
        self.config = cfg
        self.sample_rate = cfg["sample_rate"]
        self.win = int(cfg.get("win_size", cfg["fft_size"]))
        self.hop, self.fft_size, self.n_mels = int(cfg["hop_size"]), int(cfg["fft_size"]), int(cfg["mel_channels"])
        self._tables_host = mel_analysis_tables(cfg)
        # Frame 0 of an even window reads sample win / 2 (the fold of index -win / 2), which the readiness rule does not wait
        # for.  The symmetric Hann window is exactly 0 there, the product is a zero whatever finite value the ring holds, and
        # a zero's sign does not survive the magnitudes: same bits.  A window that is not 0 there waits for that sample.
        self._hold_first = self.win % 2 == 0 and float(self._tables_host[0][0]) != 0.0
        self.device = device
        self.streams = {}
        self._store = _RingStore(max(self.win, int(ring_samples or 4 * self.win)), slots)      # at the model rate
        self._in_store = _RingStore(int(input_ring_samples or 4096), slots)     # the input-rate store of the resampled streams
        self._taps = {}               # input rate -> (taps on the device, up, down)
        self._tables = None
        self._stage_host = self._stage_dev = None     # one tick's descriptors and samples: pinned, and its device twin
        self._out_dev = self._out_host = None         # one tick's frames
        self.ticks = 0
        self.device_allocations = 0   # how often a device store was (re)allocated: constant over steady ticks
        self.time_device = False      # probe: bracket the two launches of a tick with events
        self.last_tick_device_ms = None

    ring_samples = property(lambda self: self._store.ring_samples)
    input_ring_samples = property(lambda self: self._in_store.ring_samples)
    _rings = property(lambda self: self._store.rings)          # the stores' tensors, under the names they have had
    _in_rings = property(lambda self: self._in_store.rings)

    # -- host side ----------------------------------------------------------------------------------------------------
    def open(self, stream_id, sample_rate=None):
        """Open a stream; ``sample_rate``: the rate its pushes will be at (None or the model's: no resampling)."""
        if stream_id in self.streams:
            raise ValueError(f"stream {stream_id!r} is open already")
        rate, filt = None, None
        if sample_rate is not None:
            if not np.isfinite(sample_rate) or int(round(sample_rate)) <= 0:
                raise ValueError(f"stream {stream_id!r}: sample_rate must be a positive rate in Hz, got {sample_rate!r}")
            if int(round(sample_rate)) != int(round(self.sample_rate)):
                from .resample import _host_taps
                rate = int(round(sample_rate))
                taps, up, down = _host_taps(rate, int(round(self.sample_rate)))
                filt = (up, down, (taps.size - 1) // 2, int(taps.size))
        slot = self._store.take()       # the device stores follow at the next tick (_RingStore.ensure)
        self.streams[stream_id] = _AStream(slot) if rate is None else _AStream(slot, rate, self._in_store.take(), filt)

    def close(self, stream_id):
        """Forget a stream (its slots are reused)."""
        st = self.streams.pop(stream_id)
        self._store.release(st.slot)
        if st.rate is not None:
            self._in_store.release(st.in_slot)

    def push(self, stream_id, samples, last=False, sample_rate=None):
        """Append mono float32 samples to a stream; ``last`` closes it.  ``sample_rate``, when given, must be the stream's
        own: the model's, unless the stream was opened at another."""
        if sample_rate is not None:
            own = getattr(self.streams.get(stream_id), "rate", None)
            if own is None:
                check_rate(sample_rate, self.sample_rate)
            elif int(round(sample_rate)) != own:
                raise ValueError(f"samples at {sample_rate} Hz: stream {stream_id!r} was opened at {own} Hz and takes every "
                                 "push at that rate")
        st = self.streams[stream_id]
        if st.closed:
            raise ValueError(f"stream {stream_id!r} is closed")
        samples = np.asarray(samples, dtype=np.float32)
        if samples.ndim != 1:
            raise ValueError(f"samples must be 1-D (mono), got shape {samples.shape}")
        if last and st.in_have + samples.size == 0:
            raise ValueError(f"stream {stream_id!r} is closed with no samples at all: there is nothing to analyse")
        if samples.size:
            st.queue.append(samples.copy())
            st.in_have += samples.size
        st.closed = bool(last)
        # the model-rate length: what was pushed, or the resampler's outputs that no later sample can change
        st.have = st.in_have if st.rate is None else outputs_ready(st.in_have, *st.filt[:3], closed=st.closed)

    def _ready(self, st):
        if self._hold_first and not st.closed and st.have < self.win // 2 + 1:
            return 0
        return frames_ready(st.have, self.hop, self.win, st.closed)

    def finished(self, stream_id):
        st = self.streams[stream_id]
        return st.closed and st.emitted >= frames_total(st.have, self.hop)

    def _keep_from(self, st):
        """First sample a pending frame of the stream may still read: the start of the window of the next frame to hand
        out, less the two samples the reflection at the end can reach in front of it."""
        return max(0, st.emitted * self.hop - self.win // 2 - 2)

    @staticmethod
    def _in_keep_from(st):
        """First input sample a pending output of a resampled stream may still read (never behind what is to be appended)."""
        return min(input_keep_from(st.on_device, *st.filt), st.in_on_device)

    # -- device side --------------------------------------------------------------------------------------------------
    def _ensure_device(self, ring_needed):
        import torch
        if self.device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("StreamingAnalyzer: no GPU available (there is no host path)")
            self.device = torch.device("cuda", torch.cuda.current_device())
        dev = self.device = torch.device(self.device)
        if self._tables is None:
            self._tables = [torch.as_tensor(np.ascontiguousarray(tt), device=dev) for tt in self._tables_host]
        # a fresh stream's slot still holds another stream's samples: nothing of it moves to a longer ring
        held = ((st.slot, st.on_device) for st in self.streams.values() if st.on_device and not st.fresh)
        self.device_allocations += self._store.ensure(dev, ring_needed, held)

    def _device_taps(self, rate):
        if rate not in self._taps:
            from .resample import device_taps
            self._taps[rate] = device_taps(rate, int(round(self.sample_rate)), self.device)
            self.device_allocations += 1
        return self._taps[rate]

    def _grown_pair(self, host, dev_buf, floats):
        """A pinned host buffer and its device twin of at least `floats` float32 words (doubling)."""
        import torch
        if host is not None and host.numel() >= floats:
            return host, dev_buf
        size = _pow2_at_least(max(floats, 1024))
        self.device_allocations += 1
        return torch.zeros(size, dtype=torch.float32).pin_memory(), torch.zeros(size, dtype=torch.float32, device=self.device)

    def tick(self):
        """Append what was pushed to the rings and compute every frame that became ready.
        Returns {stream_id: ndarray (n, mel_channels) float32} for the streams with new frames."""
        work = [(sid, st, self._ready(st) - st.emitted) for sid, st in self.streams.items()]
        work = [(sid, st, max(0, nn)) for sid, st, nn in work if nn > 0 or st.queue or st.have > st.on_device]
        if not work:
            return {}
        import torch
        from .engine import _check, load_library
        # the rings hold every sample from the first one a pending frame reads to the newest one pushed
        self._ensure_device(max(st.have - self._keep_from(st) for _, st, _ in work))
        lib, dev = load_library(), self.device
        S, max_new = len(work), max(nn for _, _, nn in work)
        # resampled streams, grouped by rate: their samples go to the input-rate store, their model-rate samples are made
        # on the device.  Without any, everything below is the tick of the model-rate streams, word for word.
        rs = sorted((row for row, (_, st, _) in enumerate(work) if st.rate is not None), key=lambda row: work[row][1].rate)
        R = len(rs)
        if R:
            held = ((st.in_slot, st.in_on_device) for st in self.streams.values() if st.rate is not None and st.in_on_device)
            self.device_allocations += self._in_store.ensure(
                dev, max(work[row][1].in_have - self._in_keep_from(work[row][1]) for row in rs), held)
            for row in rs:
                self._device_taps(work[row][1].rate)
        counts = [st.in_have - st.in_on_device if st.rate is not None else st.have - st.on_device for _, st, _ in work]
        max_model = max((cc for (_, st, _), cc in zip(work, counts) if st.rate is None), default=0)
        head = 16 * S                                         # two (S, 4) int64 descriptor tables, in float32 words
        body = head + 20 * R                                  # ... an (R, 4) and an (R, 6) one for the resampled streams
        self._stage_host, self._stage_dev = self._grown_pair(self._stage_host, self._stage_dev, body + sum(counts))
        self._out_host, self._out_dev = self._grown_pair(self._out_host, self._out_dev, S * max_new * self.n_mels)
        stage = self._stage_host.numpy()
        desc = stage[:head].view(np.int64).reshape(2, S, 4)
        in_append = stage[head:head + 8 * R].view(np.int64).reshape(R, 4)
        in_resample = stage[head + 8 * R:body].view(np.int64).reshape(R, 6)
        offset, offsets = 0, []
        for row, ((_, st, nn), count) in enumerate(zip(work, counts)):
            # a resampled stream appends nothing to its model-rate ring: mbxr_resample_rings writes it
            desc[0, row] = (st.slot, st.on_device, count if st.rate is None else 0, offset)
            desc[1, row] = (st.slot, st.emitted, nn, st.have if st.closed else -1)
            offsets.append(offset)
            for part in st.queue:
                stage[body + offset:body + offset + part.size] = part
                offset += part.size
        for ii, row in enumerate(rs):
            st = work[row][1]
            in_append[ii] = (st.in_slot, st.in_on_device, counts[row], offsets[row])
            in_resample[ii] = (st.in_slot, st.slot, st.on_device, st.have - st.on_device, st.in_have if st.closed else -1, 0)
        used = body + offset
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            for _, st, _ in work:
                if st.fresh:                                  # a reused slot starts from silence (first tick of a stream)
                    self._rings[st.slot].zero_()
                    st.fresh = False
            self._stage_dev[:used].copy_(self._stage_host[:used], non_blocking=True)
            base = self._stage_dev.data_ptr()
            if self.time_device:
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
            _check(lib.mbxl_ring_append(base + 4 * body, offset, base, S, max_model, self._rings.data_ptr(),
                                        int(self._rings.shape[0]), self.ring_samples, stream.cuda_stream))
            if R:
                _check(lib.mbxl_ring_append(base + 4 * body, offset, base + 4 * head, R, max(counts[row] for row in rs),
                                            self._in_rings.data_ptr(), int(self._in_rings.shape[0]),
                                            self.input_ring_samples, stream.cuda_stream))
            first = 0
            while first < R:                                  # one launch per distinct input rate
                rate = work[rs[first]][1].rate
                end = first
                while end < R and work[rs[end]][1].rate == rate:
                    end += 1
                taps, up, down = self._taps[rate]
                _check(lib.mbxr_resample_rings(self._in_rings.data_ptr(), int(self._in_rings.shape[0]),
                                               self.input_ring_samples, base + 4 * (head + 8 * R) + 48 * first, end - first,
                                               int(max(in_resample[first:end, 3].max(), 0)), up, down, taps.data_ptr(),
                                               int(taps.numel()), self._rings.data_ptr(), int(self._rings.shape[0]),
                                               self.ring_samples, stream.cuda_stream))
                first = end
            tabs = self._tables
            _check(lib.mbxl_mel_frames(self._rings.data_ptr(), int(self._rings.shape[0]), self.ring_samples, base + 32 * S, S,
                                       max_new, self.win, self.hop, self.fft_size, self.n_mels, tabs[0].data_ptr(),
                                       tabs[1].data_ptr(), tabs[2].data_ptr(), tabs[3].data_ptr(), tabs[4].data_ptr(),
                                       ctypes.c_float(float(np.finfo(np.float32).eps)), self._out_dev.data_ptr(),
                                       stream.cuda_stream))
            if self.time_device:
                ev1.record()
            floats = S * max_new * self.n_mels
            if floats:
                self._out_host[:floats].copy_(self._out_dev[:floats], non_blocking=True)
            stream.synchronize()
            if self.time_device:
                self.last_tick_device_ms = ev0.elapsed_time(ev1)
        rows = self._out_host.numpy()[:S * max_new * self.n_mels].reshape(S, max_new, self.n_mels)
        result = {}
        for row, (sid, st, nn) in enumerate(work):
            st.on_device, st.in_on_device, st.queue = st.have, st.in_have, []
            if nn:
                result[sid] = rows[row, :nn].copy()
                st.emitted += nn
        self.ticks += 1
        return result


def output_filter(model_rate, output_rate):
    """``(up, down, half, n_taps)`` of the reference's filter for model rate -> output rate (``resample.reference_filter``)."""
    from .resample import _host_taps
    taps, up, down = _host_taps(int(round(model_rate)), int(round(output_rate)))
    return up, down, (taps.size - 1) // 2, int(taps.size)


def resolve_output_rate(output_rate, sample_rate, model_rate):
    """The rate an output stage works at for a stream opened with ``output_rate`` and ``sample_rate``, or None when the
    stream needs none: ``"input"`` is the stream's own ``sample_rate`` (the model's for a stream without one), and the
    model's rate needs no stage."""
    if output_rate is None:
        return None
    if isinstance(output_rate, str):
        if output_rate != "input":
            raise ValueError(f"output_rate must be a rate in Hz or 'input', got {output_rate!r}")
        if sample_rate is None:
            return None
        output_rate = sample_rate
    from .resample import positive_rate
    rate = positive_rate(output_rate, "output_rate")
    return None if rate == int(round(model_rate)) else rate


def output_lookahead_ms(model_rate, output_rate):
    """What the output stage adds to a stream's look-ahead: half the output filter, half / up model-rate samples."""
    up, _, half, _ = output_filter(model_rate, output_rate)
    return 1000.0 * half / (up * int(round(model_rate)))


class _OStream:
    def __init__(self, slot, rate, filt):
        self.slot, self.rate, self.filt = slot, rate, filt     # filt: (up, down, half, n_taps), model rate -> rate
        self.have = 0             # model-rate samples pushed
        self.on_device = 0        # ... of which the ring holds the newest
        self.emitted = 0          # outputs handed out
        self.closed = False
        self.queue = []           # (source, offset, count) pushed since the last tick

    def keep_from(self):
        """First model-rate sample a pending output may still read (never behind what is to be appended)."""
        return min(input_keep_from(self.emitted, *self.filt), self.on_device)

    def total(self):
        return outputs_ready(self.have, *self.filt[:3], closed=True)


class OutputPlan:
    """One tick of the output stage, planned on the host: ``rows`` -- (stream_id, first_out, n_out_new, n_total_in) per
    stream with work, grouped by output rate -- and ``ring_needed``, the samples the longest-held stream's ring must hold."""

    def __init__(self, rows, ring_needed):
        self.rows, self.ring_needed = rows, ring_needed


class StreamingOutputResampler:
    """The way out of a live stream: model-rate audio that is still being produced, resampled on the device to each
    stream's own output rate, a tick at a time (csrc/resample_stream.hip through include/mbexwn_live_out.h).

    The concatenated arrays ``tick`` hands out for a stream opened at rate R are ``resample.resample_device(the stream's
    whole model-rate sound, None, model_rate, R)`` bit for bit, ceil(n * up / down) samples, however the sound was cut into
    pushes.  The rules are those of the resampled input streams read in the other direction: with ``have`` model-rate
    samples appended, ``outputs_ready(have, up, down, half, closed)`` outputs are final; the ring (a third ``_RingStore``,
    at the model rate) holds every sample from ``input_keep_from(next output, ...)`` on and grows by doubling before it
    would not; after ``push(..., last=True)`` the remaining outputs follow with the filter's tail clipped at the end.

    A push names where the samples ARE on the device -- ``source``, a contiguous float32 tensor, ``count`` samples from flat
    element ``offset`` -- and the tick's ``mbxl_ring_append`` reads them from there: the audio never visits the host on its
    way in.  A steady tick is one small pinned upload (the descriptor tables), one append per distinct source tensor, one
    ``mbxo_resample_emit`` per distinct output rate into one packed buffer, and one copy back; it allocates no device
    memory (``device_allocations`` counts every (re)allocation)."""

    def __init__(self, model_rate, device=None, ring_samples=None, slots=16):
        from .resample import positive_rate
        self.model_rate = positive_rate(model_rate, "model_rate")
        self.device = device
        self.streams = {}
        # 4096: a synthesis tick of the 80 ms schedule hands over up to 7 frames = 2100 samples at once, behind the 44 to 130
        # samples (48 kHz to 8 kHz) a pending output still reads
        self._store = _RingStore(int(ring_samples or 4096), slots)
        self._taps = {}               # output rate -> (taps on the device, up, down)
        self._desc_host = self._desc_dev = None       # one tick's descriptor tables (int64): pinned, and its device twin
        self._out_dev = self._out_host = None         # one tick's outputs, packed
        self.ticks = 0
        self.device_allocations = 0   # how often a device store was (re)allocated: constant over steady ticks
        self.time_device = False      # probe: bracket the launches of a tick with events
        self.last_tick_device_ms = None

    ring_samples = property(lambda self: self._store.ring_samples)
    rings = property(lambda self: self._store.rings)     # None until the first tick with work: nothing is allocated before

    # -- host side ----------------------------------------------------------------------------------------------------
    def open(self, stream_id, output_rate):
        if stream_id in self.streams:
            raise ValueError(f"stream {stream_id!r} is open already")
        from .resample import positive_rate
        rate = positive_rate(output_rate, f"stream {stream_id!r}: output_rate")
        filt = output_filter(self.model_rate, rate)
        self.streams[stream_id] = _OStream(self._store.take(), rate, filt)

    def close(self, stream_id):
        """Forget a stream (its slot is reused)."""
        self._store.release(self.streams.pop(stream_id).slot)

    def push(self, stream_id, source, offset, count, last=False):
        """The stream's next ``count`` model-rate samples are the flat elements [offset, offset + count) of ``source``, a
        contiguous float32 tensor on the stage's device that stays valid until the next ``tick``; ``last`` closes the
        stream.  ``count`` 0 needs no source."""
        st = self.streams[stream_id]
        if st.closed:
            raise ValueError(f"stream {stream_id!r} is closed")
        offset, count = int(offset), int(count)
        if count < 0 or offset < 0:
            raise ValueError("offset and count must not be negative")
        if count:
            import torch
            if not isinstance(source, torch.Tensor) or source.dtype != torch.float32 or not source.is_contiguous():
                raise ValueError("source must be a contiguous float32 tensor")
            if offset + count > source.numel():
                raise ValueError(f"samples [{offset}, {offset + count}) lie outside a source of {source.numel()} elements")
            st.queue.append((source, offset, count))
            st.have += count
        st.closed = bool(last)

    def finished(self, stream_id):
        st = self.streams[stream_id]
        return st.closed and st.emitted >= st.total()

    def plan(self):
        """What the next tick does, from the host state alone (no device): the streams with samples to append or outputs
        that became final, grouped by output rate."""
        rows, ring_needed = [], 0
        for sid, st in sorted(self.streams.items(), key=lambda kv: kv[1].rate):
            n_new = outputs_ready(st.have, *st.filt[:3], closed=st.closed) - st.emitted
            if n_new > 0 or st.queue:
                rows.append((sid, st.emitted, n_new, st.have if st.closed else -1))
                ring_needed = max(ring_needed, st.have - st.keep_from())
        return OutputPlan(rows, ring_needed)

    def commit(self, plan):
        """Move the streams on to behind the planned tick."""
        for sid, _, n_new, _ in plan.rows:
            st = self.streams[sid]
            st.on_device, st.queue = st.have, []
            st.emitted += n_new

    # -- device side --------------------------------------------------------------------------------------------------
    def _device_taps(self, rate):
        if rate not in self._taps:
            from .resample import device_taps
            self._taps[rate] = device_taps(self.model_rate, rate, self.device)
            self.device_allocations += 1
        return self._taps[rate]

    def _grown_pair(self, host, dev_buf, size, dtype):
        """A pinned host buffer and its device twin of at least `size` elements (doubling)."""
        import torch
        if host is not None and host.numel() >= size:
            return host, dev_buf
        size = _pow2_at_least(max(size, 1024))
        self.device_allocations += 1
        return torch.zeros(size, dtype=dtype).pin_memory(), torch.zeros(size, dtype=dtype, device=self.device)

    def tick(self):
        """Append what was pushed to the rings and resample every output that became final.
        Returns {stream_id: float32 ndarray at the stream's output rate} for the streams with new output."""
        plan = self.plan()
        if not plan.rows:
            return {}
        import torch
        from .engine import _check, load_library
        if self.device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("StreamingOutputResampler: no GPU available (there is no host path)")
            self.device = torch.device("cuda", torch.cuda.current_device())
        lib, dev = load_library(), torch.device(self.device)
        self.device = dev
        held = ((st.slot, st.on_device) for st in self.streams.values() if st.on_device)
        self.device_allocations += self._store.ensure(dev, plan.ring_needed, held)
        rings, ring = self._store.rings, self._store.ring_samples
        # the append rows: one call per distinct source tensor (and per place in its stream's queue: two rows of one call
        # never name the same slot)
        calls, total = {}, 0
        for sid, _, _, _ in plan.rows:
            st, at = self.streams[sid], self.streams[sid].on_device
            for turn, (source, offset, count) in enumerate(st.queue):
                if source.device != dev:
                    raise ValueError(f"stream {sid!r}: source is on {source.device}, the stage on {dev}")
                calls.setdefault((turn, source.data_ptr(), source.numel()), []).append((st.slot, at, count, offset))
                at += count
        n_app, S = sum(len(rr) for rr in calls.values()), len(plan.rows)
        self._desc_host, self._desc_dev = self._grown_pair(self._desc_host, self._desc_dev, 4 * n_app + 6 * S, torch.int64)
        table = self._desc_host.numpy()
        app, emit = table[:4 * n_app].reshape(n_app, 4), table[4 * n_app:4 * n_app + 6 * S].reshape(S, 6)
        first = 0
        for rows in calls.values():
            app[first:first + len(rows)] = rows
            first += len(rows)
        for row, (sid, first_out, n_new, n_total) in enumerate(plan.rows):
            emit[row] = (self.streams[sid].slot, first_out, n_new, n_total, total, 0)
            total += max(n_new, 0)
        self._out_host, self._out_dev = self._grown_pair(self._out_host, self._out_dev, total, torch.float32)
        for sid, _, _, _ in plan.rows:
            self._device_taps(self.streams[sid].rate)
        used = 4 * n_app + 6 * S
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            self._desc_dev[:used].copy_(self._desc_host[:used], non_blocking=True)
            base = self._desc_dev.data_ptr()
            if self.time_device:
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
            first = 0
            for (_, ptr, numel), rows in calls.items():
                _check(lib.mbxl_ring_append(ptr, numel, base + 32 * first, len(rows), max(rr[2] for rr in rows),
                                            rings.data_ptr(), int(rings.shape[0]), ring, stream.cuda_stream))
                first += len(rows)
            first = 0
            while first < S:                                  # one launch per distinct output rate
                rate = self.streams[plan.rows[first][0]].rate
                end = first
                while end < S and self.streams[plan.rows[end][0]].rate == rate:
                    end += 1
                taps, up, down = self._taps[rate]
                _check(lib.mbxo_resample_emit(rings.data_ptr(), int(rings.shape[0]), ring, base + 32 * n_app + 48 * first,
                                              end - first, int(max(emit[first:end, 2].max(), 0)), up, down, taps.data_ptr(),
                                              int(taps.numel()), self._out_dev.data_ptr(), int(self._out_dev.numel()),
                                              stream.cuda_stream))
                first = end
            if self.time_device:
                ev1.record()
            if total:
                self._out_host[:total].copy_(self._out_dev[:total], non_blocking=True)
            stream.synchronize()
            if self.time_device:
                self.last_tick_device_ms = ev0.elapsed_time(ev1)
        packed = self._out_host.numpy()
        result = {sid: packed[int(emit[row, 4]):int(emit[row, 4]) + n_new].copy()
                  for row, (sid, _, n_new, _) in enumerate(plan.rows) if n_new > 0}
        self.commit(plan)
        self.ticks += 1
        return result


class _LStream:
    def __init__(self, hop, rng, noise_fn, up=1, down=1):
        self.factors = FrameFactors(hop, up, down)
        self.frames = 0               # mel frames handed to the synthesizer
        self.rng, self.noise_fn = rng, noise_fn
        self.flushed = False          # the synthesizer has been told that the stream is over
        self.out_rate = None          # the stream's output rate when it is not the model's: it goes through the output stage


class LiveResynthesizer:
    """Audio in, audio out: a ``StreamingAnalyzer``, ``MELInverter.scale_mel`` (on the host: it is elementwise, so a chunk
    of frames scales to the bits the whole file scales to) and a ``StreamingSynthesizer``, a tick at a time.

    Transposition rule: a ``transposition`` factor given with ``push_audio`` applies to the mel frames whose centre sample
    t * hop lies in that push's sample range (``FrameFactors``); a push without one has factor 1.  For a stream opened at a
    ``sample_rate`` of its own (resampled on the device, see ``StreamingAnalyzer``) the centre of frame t is input sample
    (t * hop * down) // up.

    Noise: the N(0,1) draw of the frames [a, b) of a stream is ``noise_fn(stream_id, a, b)`` ((b - a) * steps_per_frame
    float32 values); by default consecutive draws of a per-stream ``numpy.random.Generator`` seeded with ``seed``.

    A stream's output then equals ``mel_inverter.synth_from_mel(scale_mel(mell dictionary of the whole sound), noise=the
    same draw, transposition=the per-frame factors)`` bit for bit, when the engine is pinned to ``conv_form="f23"`` (the
    form the streams run) and the mel is the device analysis of the sound (``compute_log_mel_device``)."""

    def __init__(self, mel_inverter, chunk_frames=(6, 6, 7, 6, 7)):
        from .streaming import StreamingSynthesizer
        engine = mel_inverter.model
        info = engine.conv_form_info()
        if info.get("split_f16_layers", 0) > 0 or info.get("split_f16_gate_layers", 0) > 0:
            raise ValueError("LiveResynthesizer needs a float32 engine: this one runs its whole-item forwards in split half "
                             "precision (precision='split_f16'), streams would not be bit-equal to its offline synthesis")
        self.mel_inverter = mel_inverter
        self.synthesizer = StreamingSynthesizer(engine, chunk_frames=chunk_frames)
        self.analyzer = StreamingAnalyzer(mel_inverter.preprocess_config, device=engine.device)
        self.dims = engine.dims
        self._header = mell_header(mel_inverter.preprocess_config)
        self.streams = {}
        # streams with an output rate of their own leave through this stage; its store is allocated by its first tick
        self.output = StreamingOutputResampler(self.analyzer.sample_rate, device=engine.device)
        self._out_streams = 0

    @property
    def lookahead_ms(self):
        """The analysis look-ahead -- half a window, rounded up to the next frame -- plus the synthesizer's own."""
        an = self.analyzer
        frames = -(-(an.win - an.win // 2) // an.hop)
        return 1000.0 * frames * an.hop / an.sample_rate + self.synthesizer.lookahead_ms

    def lookahead_ms_for(self, sample_rate=None, output_rate=None):
        """``lookahead_ms`` of a stream opened at ``sample_rate`` and ``output_rate``: a resampled stream waits for half
        its filter as well, half / up input samples (0.92 ms at 44.1 and 48 kHz, 1.4 ms at 16 kHz for a 24 kHz model); a
        stream with an output rate waits for half the output filter, half / up model-rate samples (0.92 ms to 48 kHz,
        0.94 ms to 44.1 kHz, 1.4 ms to 16 kHz)."""
        model = int(round(self.analyzer.sample_rate))
        ms = self.lookahead_ms
        if sample_rate is not None and int(round(sample_rate)) != model:
            from .resample import _host_taps
            taps, up, _ = _host_taps(int(round(sample_rate)), model)
            ms += 1000.0 * ((taps.size - 1) // 2) / up / int(round(sample_rate))
        out_rate = resolve_output_rate(output_rate, sample_rate, model)
        if out_rate is not None:
            ms += output_lookahead_ms(model, out_rate)
        return ms

    def open(self, stream_id, seed=None, noise_fn=None, sample_rate=None, output_rate=None):
        """``output_rate``: the rate the stream's audio comes back at -- a rate in Hz, or ``"input"`` for the stream's own
        ``sample_rate``; None or the model's rate: the model-rate audio, as the synthesizer emits it."""
        out_rate = resolve_output_rate(output_rate, sample_rate, self.analyzer.sample_rate)
        self.analyzer.open(stream_id, sample_rate=sample_rate)
        self.synthesizer.open(stream_id)
        up, down = (self.analyzer.streams[stream_id].filt or (1, 1))[:2]
        st = self.streams[stream_id] = _LStream(self.analyzer.hop, None if noise_fn else np.random.default_rng(seed),
                                                noise_fn, up, down)
        if out_rate is not None:
            self.output.open(stream_id, out_rate)
            st.out_rate = out_rate
            self._out_streams += 1

    def close(self, stream_id):
        self.analyzer.close(stream_id)
        self.synthesizer.close(stream_id)
        if self.streams.pop(stream_id).out_rate is not None:
            self.output.close(stream_id)
            self._out_streams -= 1

    def push_audio(self, stream_id, samples, last=False, transposition=None, sample_rate=None):
        """Append samples at the stream's rate (the model's, unless it was opened at another); ``transposition``: one finite
        positive factor for the frames centred in this push (see the class docstring)."""
        if transposition is not None:
            transposition = float(transposition)
            if not (np.isfinite(transposition) and transposition > 0):
                raise ValueError("transposition must be finite and positive")
        st = self.streams[stream_id]
        before = self.analyzer.streams[stream_id].in_have
        self.analyzer.push(stream_id, samples, last=last, sample_rate=sample_rate)
        st.factors.add(self.analyzer.streams[stream_id].in_have - before, transposition)
        if last:
            st.factors.close()

    def _noise(self, stream_id, st, first, end):
        spf = self.dims.steps_per_frame
        if st.noise_fn is not None:
            noise = np.asarray(st.noise_fn(stream_id, first, end), dtype=np.float32).reshape(-1)
            if noise.size != (end - first) * spf:
                raise ValueError(f"noise_fn must return {(end - first) * spf} values for frames [{first}, {end})")
            return noise
        return st.rng.standard_normal((end - first) * spf).astype(np.float32)

    def tick(self):
        """One analysis tick, then one synthesis tick.  Returns {stream_id: audio ndarray} of the streams that emitted."""
        mels = self.analyzer.tick()
        for sid, st in self.streams.items():
            rows = mels.get(sid)
            done = self.analyzer.finished(sid)
            if rows is None and not (done and not st.flushed):
                continue
            n = 0 if rows is None else rows.shape[0]
            first, end = st.frames, st.frames + n
            if n:
                scaled = self.mel_inverter.scale_mel(dict(self._header, mell=rows.T))[0]
            else:
                scaled = np.zeros((0, self.dims.mel_channels), dtype=np.float32)
            noise = self._noise(sid, st, first, end) if self.dims.noise_sigma else None
            self.synthesizer.push(sid, scaled, noise, last=done, transposition=st.factors.take(first, end))
            st.frames, st.flushed = end, done
        audio = self.synthesizer.tick()
        if not self._out_streams:
            return audio
        # the streams with an output rate: their chunks go on, from where the synthesizer left them on the device, to the
        # output stage, and what that stage has final comes back in their place
        source, spans = self.synthesizer.last_emit_device or (None, {})
        for sid, st in self.streams.items():
            if st.out_rate is None or self.output.streams[sid].closed:
                continue
            offset, count = spans.get(sid, (0, 0))
            last = st.flushed and self.synthesizer.finished(sid)
            if count or last:
                self.output.push(sid, source, offset, count, last=last)
            audio.pop(sid, None)
        audio.update(self.output.tick())
        return audio

    def finished(self, stream_id):
        st = self.streams[stream_id]
        if st.out_rate is not None:
            return self.output.finished(stream_id)
        return st.flushed and self.synthesizer.finished(stream_id)

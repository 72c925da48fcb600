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

The readiness rules (``frames_ready``, ``outputs_ready``, ``input_keep_from``), the mapping of per-push transposition factors
to mel frames (``FrameFactors``) and what a tick does (``AnalysisPlan``, ``EmitPlan``) are pure host logic: live_plan.py.
"""
import ctypes

import numpy as np

from .analysis import mel_analysis_tables, mell_header
from .live_plan import (AnalysisPlan, EmitPlan, FrameFactors, LimiterPlan, OutputPlan, _AStream, _DStream,  # noqa: F401
                        _OStream, _pow2_at_least, check_rate,
                        f0_frames_ready, frame_factors, frames_ready, frames_total, input_keep_from, outputs_ready,
                        stream_frames_ready)
from .resample import _host_taps, device_taps, positive_rate


def resampling_filter(from_rate, to_rate):
    """``(up, down, half, n_taps)`` of the reference's filter from_rate -> to_rate (``resample.reference_filter``)."""
    taps, up, down = _host_taps(int(round(from_rate)), int(round(to_rate)))
    return up, down, (taps.size - 1) // 2, int(taps.size)


def resampling_lookahead_ms(from_rate, to_rate):
    """What a resampling stage adds to a stream's look-ahead: half its filter, half / up samples at from_rate."""
    up, _, half, _ = resampling_filter(from_rate, to_rate)
    return 1000.0 * half / (up * int(round(from_rate)))


output_filter, output_lookahead_ms = resampling_filter, resampling_lookahead_ms        # ... of (model_rate, output_rate)


class _RingStore:
    """One ring store of include/mbexwn_live.h: ``slots`` rings of ``ring_samples`` samples, a power of two.  It hands out
    slots -- ``first_slots`` at first, then doubling; the lowest new slot first, a released slot before any other -- and
    keeps the device tensor ``rings``, which follows lazily: ``ensure`` brings it up to date at the next tick."""

    def __init__(self, ring_samples, first_slots):
        self.ring_samples = _pow2_at_least(ring_samples)
        self.slots, self._first_slots, self._free = 0, max(1, int(first_slots)), []
        self.rings = None             # (slots, ring_samples) float32 on the device

    def at_least(self, ring_samples):
        """Rings of at least ``ring_samples`` samples from the start (before the store is on the device; later ``ensure``
        grows it)."""
        if self.rings is None:
            self.ring_samples = max(self.ring_samples, _pow2_at_least(ring_samples))

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


class _Stage:
    """What the two device stages share around their plans and launches: the device, the filters' taps on it, pinned buffers
    with their device twins, the upload, the event bracket of ``time_device`` and the packed copy back."""
    _taps_to_model = True         # the stage's filters: a stream's rate -> model rate, or model rate -> a stream's rate
    ring_samples = property(lambda self: self._store.ring_samples)       # of ``_store``, the stage's _RingStore at the model rate
    rings = property(lambda self: self._store.rings)     # None until the first tick with work: nothing is allocated before

    def __init__(self, model_rate, device):
        self.model_rate, self.device = model_rate, device
        self.streams = {}
        self._taps = {}               # a stream's rate -> (taps on the device, up, down)
        self._out_dev = self._out_host = None         # one tick's results, packed
        self.ticks = 0
        self.device_allocations = 0   # how often a device store was (re)allocated: constant over steady ticks
        self.time_device = False      # probe: bracket the launches of a tick with events
        self.last_tick_device_ms = None

    def _resolve_device(self):
        import torch
        if self.device is None:
            if not torch.cuda.is_available():
                raise RuntimeError(f"{type(self).__name__}: no GPU available (there is no host path)")
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(self.device)
        return self.device

    def _device_taps(self, rate):
        if rate not in self._taps:
            rates = (rate, self.model_rate) if self._taps_to_model else (self.model_rate, rate)
            self._taps[rate] = device_taps(*rates, self.device)
            self.device_allocations += 1

    def _grown_pair(self, host, dev_buf, size, dtype):
        """A pinned host buffer and its device twin of at least `size` elements (doubling)."""
        import torch
        if host is not None and host.numel() >= size:
            return host, dev_buf
        size = _pow2_at_least(max(size, 1024))
        self.device_allocations += 1
        return torch.zeros(size, dtype=dtype).pin_memory(), torch.zeros(size, dtype=dtype, device=self.device)

    def _state_rows(self, table, slots, words):
        """A table of int32 state rows on the device, one per ring slot: ``table`` itself when it has ``slots`` rows, else
        a longer one that keeps its rows and starts the new ones from zero."""
        import torch
        if table is not None and table.shape[0] >= slots:
            return table
        new = torch.zeros((slots, words), dtype=torch.int32, device=self.device)
        if table is not None:
            new[:table.shape[0]] = table
        self.device_allocations += 1
        return new

    def _upload(self, host, dev_buf, used):
        """The tick's one upload on the current stream -> (the stream, the device address, the events around the launches)."""
        import torch
        stream = torch.cuda.current_stream(self.device)
        dev_buf[:used].copy_(host[:used], non_blocking=True)
        events = [torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)] if self.time_device else None
        if events:
            events[0].record()
        return stream, dev_buf.data_ptr(), events

    def _copy_back(self, stream, events, used):
        """The packed copy back behind the launches, and the wait for it -> the first ``used`` results on the host."""
        if events:
            events[1].record()
        if used:
            self._out_host[:used].copy_(self._out_dev[:used], non_blocking=True)
        stream.synchronize()
        if events:
            self.last_tick_device_ms = events[0].elapsed_time(events[1])
        return self._out_host.numpy()[:used]


class StreamingAnalyzer(_Stage):
    """Log-mel analysis of any number of concurrent streams, a tick at a time.

    The concatenated rows ``tick`` hands out for a stream are the rows [0, n // hop + 1) of ``compute_log_mel_device`` on the
    stream's whole sound (n samples), bit for bit, however the sound was cut into pushes.  Frame t is handed out by the
    first tick after t * hop - win // 2 + win samples have arrived; after ``push(..., last=True)`` the remaining frames
    follow, with the reflection at the end (as often as a stream shorter than half a window needs it).

    Samples must be at ``preprocess_config["sample_rate"]``, unless the stream was opened with a ``sample_rate`` of its own
    (below).  A tick is planned on the host (``plan``: an ``AnalysisPlan``, no device), packed into one pinned buffer
    (descriptors and samples), uploaded in one copy, launched -- ``mbxl_ring_append`` and ``mbxl_mel_frames``; with resampled
    streams a second append and the resampler between them --, copied back once and committed (``commit``).  A steady tick
    allocates no device memory: the stores grow by doubling when more streams are open than slots exist, when a tick carries
    more than any before it, and -- the rings -- when a stream's pushes would overwrite samples a pending frame still needs.
    ``ring_samples`` (default 4 windows) and ``slots`` are the sizes the stores start from.

    ``open(stream_id, sample_rate=R)`` with R another rate than the model's gives a resampled stream: its pushes are at R
    and go to a slot of a second ring store, (slots, ``input_ring_samples``) at the input rate, from where the tick's
    ``mbxr_resample_rings`` launches (one per distinct rate among the streams with work) write every output that became
    final -- ``outputs_ready`` -- into the stream's model-rate ring.  Behind that ring nothing differs: the stream's
    model-rate length is the count of outputs produced, and the rows are those of ``generate_mels`` on the whole sound at R,
    bit for bit.  The input store grows as the other does; its rule is ``input_keep_from``.  A tick without resampled
    streams is the tick described above, launch for launch.

    ``open(stream_id, f0_params=P)`` with P an ``f0track.params`` dictionary at the model rate gives a stream that tracks its
    F0 (csrc/f0_stream.hip, include/mbexwn_live_pitch.h): a frame is handed out when its mel window and
    the L = window + tau_max samples of its F0 frame have both arrived (``f0_frames_ready``), a tick with such streams adds one
    ``mbxt_f0_frames`` launch behind ``mbxl_mel_frames`` on the same descriptor table, and the tick's values are in
    ``last_f0`` -- {stream_id: (f0, periodicity)}, float32, one value per mel row handed out, 0 = unvoiced.  Concatenated they
    are ``f0track.track_f0_host(sound, arange(0, n + 1, hop), P)`` bit for bit.  The tracker reads the model-rate ring, so a
    resampled stream needs nothing special.  All tracking streams of an analyzer share one P.  A tick without tracking
    streams makes the launches it made before and no others.

    ``open(stream_id, f0_params=P, f0_lag=N, f0_decode=D)`` gives a tracking stream whose contour is DECODED with a fixed lag
    of N frames (csrc/f0_lag.hip, include/mbexwn_live_contour.h; D: an ``f0decode.decode_params``
    dictionary, None: the defaults).  Mel rows and readiness are those of a tracking stream.  In place of ``mbxt_f0_frames``
    the tick launches ``mbxv_f0_candidate_frames`` and ``mbxv_decode_f0_frames`` on the same descriptor table; the candidate
    tables stay on the device, and so does a state row per slot.  ``last_f0[stream_id]`` holds the frames DECIDED in the tick
    -- ``f0decode.lag_frames_decided`` of the frames seen, all of them at the stream's end; a stream with none is absent --
    so it trails the mel rows by N frames until the closing tick.  Concatenated they are ``f0decode.viterbi_lag_host`` of
    ``candidates_host`` on the whole sound, bit for bit.  All tracking streams of an analyzer share one (P, D, N)."""

    def __init__(self, preprocess_config, device=None, ring_samples=None, slots=16, input_ring_samples=None):
        cfg = preprocess_config
        super().__init__(int(round(cfg["sample_rate"])), device)
        self.config = cfg
        self.sample_rate = cfg["sample_rate"]
        self.win = int(cfg.get("win_size", cfg["fft_size"]))
        self.hop, self.fft_size, self.n_mels = int(cfg["hop_size"]), int(cfg["fft_size"]), int(cfg["mel_channels"])
        self._tables_host = mel_analysis_tables(cfg)
        # Frame 0 of an even window reads sample win / 2 (the fold of index -win / 2), which the readiness rule does not wait
        # for.  The symmetric Hann window is exactly 0 there, the product is a zero whatever finite value the ring holds, and
        # a zero's sign does not survive the magnitudes: same bits.  A window that is not 0 there waits for that sample.
        self._hold_first = self.win % 2 == 0 and float(self._tables_host[0][0]) != 0.0
        self._store = _RingStore(max(self.win, int(ring_samples or 4 * self.win)), slots)      # at the model rate
        self._in_store = _RingStore(int(input_ring_samples or 4096), slots)     # the input-rate store of the resampled streams
        self._tables = None
        self._stage_host = self._stage_dev = None     # one tick's descriptors and samples: pinned, and its device twin
        self.f0_params = None         # the parameters of the tracking streams: set by the first one opened
        self.f0_decode = self.f0_lag = None           # ... and their decoder's and its lag, when they decode (section 6l)
        self._lag_state = None        # (slots, mbxv_lag_state_words()) int32 on the device: a decoder state per ring slot
        self._cand = None             # one tick's three candidate tables, on the device only
        self.last_f0 = {}             # {stream_id: (f0, periodicity)} of the last tick's rows of the tracking streams

    input_ring_samples = property(lambda self: self._in_store.ring_samples)
    input_rings = property(lambda self: self._in_store.rings)   # None until the first tick with a resampled stream

    # -- host side ----------------------------------------------------------------------------------------------------
    def open(self, stream_id, sample_rate=None, f0_params=None, f0_decode=None, f0_lag=None):
        """Open a stream; ``sample_rate``: the rate its pushes will be at (None or the model's: no resampling);
        ``f0_params``: an ``f0track.params`` dictionary at the model rate -- the stream tracks its F0 (``last_f0``);
        ``f0_lag``: frames of look-ahead (0 .. 128) -- the stream decodes its contour with that lag, by ``f0_decode``, an
        ``f0decode.decode_params`` dictionary (None: the defaults)."""
        if stream_id in self.streams:
            raise ValueError(f"stream {stream_id!r} is open already")
        if f0_decode is not None and f0_lag is None:
            raise ValueError(f"stream {stream_id!r}: f0_decode decodes the contour over the whole sound (f0decode.py), which a "
                             "stream does not have; streams track every frame on its own")
        if f0_lag is not None:
            from .f0decode import check_decode, check_lag, decode_params
            if f0_params is None:
                raise ValueError(f"stream {stream_id!r}: f0_lag is the look-ahead of a stream that tracks its F0: give f0_params")
            f0_lag = check_lag(f0_lag)
            f0_decode = decode_params() if f0_decode is None else check_decode(dict(f0_decode))
        f0_len = None
        if f0_params is not None:
            from .f0track import check_params
            f0_params = check_params(dict(f0_params))
            if int(f0_params["sample_rate"]) != self.model_rate:
                raise ValueError(f"stream {stream_id!r}: f0_params are for {f0_params['sample_rate']} Hz, the tracker reads the "
                                 f"model-rate samples at {self.model_rate} Hz")
            if self.f0_params is not None and any(st.f0_len is not None for st in self.streams.values()):
                if f0_params != self.f0_params:
                    raise ValueError(f"stream {stream_id!r}: the tracking streams of an analyzer share one set of f0_params")
                if f0_lag != self.f0_lag or not _same_decode(f0_decode, self.f0_decode):
                    raise ValueError(f"stream {stream_id!r}: the tracking streams of an analyzer share one f0_decode and one "
                                     f"f0_lag (open: lag {self.f0_lag!r})")
            f0_len = int(f0_params["window"]) + int(f0_params["tau_max"])
        rate, filt = None, None
        if sample_rate is not None:
            if not np.isfinite(sample_rate) or int(round(sample_rate)) <= 0:
                raise ValueError(f"stream {stream_id!r}: sample_rate must be a positive rate in Hz, got {sample_rate!r}")
            if int(round(sample_rate)) != self.model_rate:
                rate = int(round(sample_rate))
                filt = resampling_filter(rate, self.model_rate)
        slot = self._store.take()       # the device stores follow at the next tick (_RingStore.ensure)
        self.streams[stream_id] = (_AStream(slot, f0_len=f0_len) if rate is None else
                                   _AStream(slot, rate, self._in_store.take(), filt, f0_len=f0_len))
        if f0_len is not None:
            self.f0_params, self.f0_decode, self.f0_lag = f0_params, f0_decode, f0_lag
            self._store.at_least(f0_len)        # the tracker's frame must fit the ring

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
        return stream_frames_ready(st, self.hop, self.win, self._hold_first)

    def finished(self, stream_id):
        st = self.streams[stream_id]
        return st.closed and st.emitted >= frames_total(st.have, self.hop)

    def plan(self):
        """What the next tick does, from the host state alone (no device, nothing changes)."""
        return AnalysisPlan(self.streams, self.hop, self.win, self._hold_first)

    def commit(self, plan):
        """Move the streams on to behind the planned tick."""
        for sid, nn in plan.rows:
            st = self.streams[sid]
            st.on_device, st.in_on_device, st.queue, st.fresh = st.have, st.in_have, [], False
            if st.f0_len is not None and self.f0_lag is not None:
                st.f0_decided = self._decided_after(st, nn)
            st.emitted += nn

    # -- device side --------------------------------------------------------------------------------------------------
    def _ensure(self, plan):
        """The device, the analysis tables, both stores at the sizes the plan needs and the taps of its rates."""
        import torch
        dev = self._resolve_device()
        if self._tables is None:
            self._tables = [torch.as_tensor(np.ascontiguousarray(tt), device=dev) for tt in self._tables_host]
        # a fresh stream's slot still holds another stream's samples: nothing of it moves to a longer ring
        held = ((st.slot, st.on_device) for st in self.streams.values() if st.on_device and not st.fresh)
        ring_needed = max(plan.ring_needed, self._f0_len() if plan.T else 0)
        self.device_allocations += self._store.ensure(dev, ring_needed, held)
        if plan.R:
            held = ((st.in_slot, st.in_on_device) for st in self.streams.values() if st.rate is not None and st.in_on_device)
            self.device_allocations += self._in_store.ensure(dev, plan.in_ring_needed, held)
            for rate, _, _, _ in plan.groups:
                self._device_taps(rate)

    def _f0_len(self):
        return int(self.f0_params["window"]) + int(self.f0_params["tau_max"])

    def _decided_after(self, st, nn):
        """Frames of a decoding stream that are decided behind a tick that computes its next ``nn`` frames: the rule of
        ``mbxv_decode_f0_frames``."""
        from .f0decode import lag_frames_decided
        done = st.emitted + nn
        return max(st.f0_decided, lag_frames_decided(done, self.f0_lag, st.closed and done >= frames_total(st.have, self.hop)))

    def _ensure_decoder(self, plan):
        """The decoder's state rows, one per ring slot, and room for the tick's candidate tables (``tick`` zeroes the row of a
        fresh stream beside its ring, whether or not the tick launches the decoder)."""
        import torch
        from .abi import load_library
        words = int(load_library().mbxv_lag_state_words())
        self._lag_state = self._state_rows(self._lag_state, int(self.rings.shape[0]), words)
        need = 3 * plan.T * plan.max_new * 8
        if self._cand is None or self._cand.numel() < need:
            self._cand = torch.zeros(_pow2_at_least(max(need, 1024)), dtype=torch.float32, device=self.device)
            self.device_allocations += 1

    def tick(self):
        """Append what was pushed to the rings and compute every frame that became ready.
        Returns {stream_id: ndarray (n, mel_channels) float32} for the streams with new frames; ``last_f0`` then holds the
        tracked (f0, periodicity) of those rows for the streams that track."""
        plan = self.plan()
        self.last_f0 = {}
        if not plan.rows:
            return {}
        import torch
        from .abi import _check, load_library
        self._ensure(plan)
        if self.f0_lag is not None:
            self._ensure_decoder(plan)
        lib, rings, in_rings, tabs = load_library(), self.rings, self.input_rings, self._tables
        S, R, body, used, mel_floats = plan.S, plan.R, plan.body, plan.body + plan.samples, plan.S * plan.max_new * self.n_mels
        lag = self.f0_lag if plan.T else None
        # the two planes of the tracker ride behind the mel rows in the one copy back; a decoder's are `lag` frames wider
        width = plan.max_new + (lag or 0)
        plane = plan.T * width
        floats = mel_floats + 2 * plane
        self._stage_host, self._stage_dev = self._grown_pair(self._stage_host, self._stage_dev, used, torch.float32)
        self._out_host, self._out_dev = self._grown_pair(self._out_host, self._out_dev, floats, torch.float32)
        plan.pack(self._stage_host.numpy())
        with torch.cuda.device(self.device):
            for slot in plan.fresh:                           # a reused slot starts from silence (first tick of a stream)
                rings[slot].zero_()
                if self._lag_state is not None:               # ... and from a decoder that has seen no frame
                    self._lag_state[slot].zero_()
            stream, base, events = self._upload(self._stage_host, self._stage_dev, used)
            _check(lib.mbxl_ring_append(base + 4 * body, plan.samples, base, S, plan.max_model, rings.data_ptr(),
                                        int(rings.shape[0]), self.ring_samples, stream.cuda_stream))
            if R:
                _check(lib.mbxl_ring_append(base + 4 * body, plan.samples, base + 64 * S, R, plan.max_in, in_rings.data_ptr(),
                                            int(in_rings.shape[0]), self.input_ring_samples, stream.cuda_stream))
            for rate, first, end, max_out in plan.groups:     # one launch per distinct input rate
                taps, up, down = self._taps[rate]
                _check(lib.mbxr_resample_rings(in_rings.data_ptr(), int(in_rings.shape[0]), self.input_ring_samples,
                                               base + 64 * S + 32 * R + 48 * first, end - first, max_out, up, down,
                                               taps.data_ptr(), int(taps.numel()), rings.data_ptr(), int(rings.shape[0]),
                                               self.ring_samples, stream.cuda_stream))
            _check(lib.mbxl_mel_frames(rings.data_ptr(), int(rings.shape[0]), self.ring_samples, base + 32 * S, S,
                                       plan.max_new, self.win, self.hop, self.fft_size, self.n_mels, tabs[0].data_ptr(),
                                       tabs[1].data_ptr(), tabs[2].data_ptr(), tabs[3].data_ptr(), tabs[4].data_ptr(),
                                       ctypes.c_float(float(np.finfo(np.float32).eps)), self._out_dev.data_ptr(),
                                       stream.cuda_stream))
            if plane and lag is not None:
                self._decode_frames(lib, plan, base + 32 * S, width, self._out_dev.data_ptr() + 4 * mel_floats, stream)
            elif plane:
                prm, out = self.f0_params, self._out_dev.data_ptr() + 4 * mel_floats
                _check(lib.mbxt_f0_frames(rings.data_ptr(), int(rings.shape[0]), self.ring_samples, base + 32 * S, plan.T,
                                          plan.max_new, self.hop, int(prm["sample_rate"]), int(prm["window"]),
                                          int(prm["tau_min"]), int(prm["tau_max"]), ctypes.c_float(float(prm["threshold"])),
                                          ctypes.c_float(float(prm["e_min"])), out, out + 4 * plane, stream.cuda_stream))
            packed = self._copy_back(stream, events, floats)
            rows = packed[:mel_floats].reshape(S, plan.max_new, self.n_mels)
            tracked = packed[mel_floats:].reshape(2, plan.T, width)
        result = {sid: rows[row, :nn].copy() for row, (sid, nn) in enumerate(plan.rows) if nn}
        if lag is not None:           # a decoder hands out what became decided, which is not what was computed
            counts = [self._decided_after(self.streams[sid], nn) - self.streams[sid].f0_decided for sid, nn in plan.rows[:plan.T]]
        else:
            counts = [nn for _, nn in plan.rows[:plan.T]]
        self.last_f0 = {sid: (tracked[0, row, :cc].copy(), tracked[1, row, :cc].copy())
                        for row, ((sid, _), cc) in enumerate(zip(plan.rows[:plan.T], counts)) if cc}
        self.commit(plan)
        self.ticks += 1
        return result

    def _decode_frames(self, lib, plan, desc, width, out, stream):
        """The two launches of a tick with decoding streams, on the first T rows of the mel launch's table: the candidates of
        the new frames into ``_cand``, then the recursion continued from ``_lag_state`` into the two (T, width) planes."""
        from .abi import _check
        from .f0decode import _host_tables
        prm, dec, rings = self.f0_params, self.f0_decode, self.rings
        th, ww = _host_tables(dec)
        fpp = ctypes.POINTER(ctypes.c_float)
        table = 4 * plan.T * plan.max_new * 8
        cand = [self._cand.data_ptr() + kk * table for kk in range(3)]
        _check(lib.mbxv_f0_candidate_frames(rings.data_ptr(), int(rings.shape[0]), self.ring_samples, desc, plan.T, plan.max_new,
                                            self.hop, int(prm["sample_rate"]), int(prm["window"]), int(prm["tau_min"]),
                                            int(prm["tau_max"]), ctypes.c_float(float(prm["e_min"])), th.ctypes.data_as(fpp),
                                            ww.ctypes.data_as(fpp), int(th.size), int(dec["n_cand"]), *cand, stream.cuda_stream))
        _check(lib.mbxv_decode_f0_frames(*cand, desc, plan.T, plan.max_new, self.hop, self._lag_state.data_ptr(),
                                         int(self._lag_state.shape[0]), self.f0_lag, int(prm["sample_rate"]),
                                         ctypes.c_float(float(dec["w_jump"])), ctypes.c_float(float(dec["w_switch"])), out,
                                         out + 4 * plan.T * width, width, stream.cuda_stream))


def _same_decode(one, other):
    """Whether two checked ``f0decode.decode_params`` dictionaries (or None) say the same."""
    if one is None or other is None:
        return one is other
    return all(np.array_equal(np.asarray(one[key], dtype=np.float32), np.asarray(other[key], dtype=np.float32)) for key in one)


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
    rate = positive_rate(output_rate, "output_rate")
    return None if rate == int(round(model_rate)) else rate


class _EmitStage(_Stage):
    """What the stages behind the synthesizer share: model-rate or output-rate audio that is still
    being produced goes into a ring per stream, and every output that became final leaves in packed rows.

    A push names where the samples ARE on the device -- ``source``, a contiguous float32 tensor, ``count`` samples from flat
    element ``offset`` -- and the tick's ``mbxl_ring_append`` reads them from there: the audio never visits the host on its
    way in.  A tick is planned on the host (``plan``: an ``EmitPlan``, no device); a steady one is one small pinned upload
    (the descriptor tables), one append per distinct source tensor, one launch of the stage's kernel per distinct key among
    the streams with work into one packed buffer, and one copy back; it allocates no device memory (``device_allocations``
    counts every (re)allocation).  The ring store grows by doubling before a stream's pushes would overwrite samples a
    pending output still reads.

    ``last_emit_device``, like the synthesizer's: where the last tick left its outputs on the device, ``(tensor, {stream_id:
    (flat offset, count)})``, valid until the next tick; None after a tick without output.  The next stage reads from there.

    A stage gives ``open``, the streams' records (``live_plan._EStream``: their two rules and their key) and three hooks:
    ``_prepare`` -- what the groups of a tick need on the device before the launches --, ``_word5`` -- the sixth word of a
    stream's descriptor row -- and ``_launch``, the one launch of a group."""

    def __init__(self, model_rate, device, ring_samples, slots):
        super().__init__(model_rate, device)
        self._store = _RingStore(ring_samples, slots)
        self._desc_host = self._desc_dev = None       # one tick's descriptor tables (int64): pinned, and its device twin
        self.last_emit_device = None

    # -- host side ----------------------------------------------------------------------------------------------------
    def close(self, stream_id):
        """Forget a stream (its slot is reused)."""
        self._store.release(self.streams.pop(stream_id).slot)

    def push(self, stream_id, source, offset, count, last=False):
        """The stream's next ``count`` samples are the flat elements [offset, offset + count) of ``source``, a contiguous
        float32 tensor on the stage's device that stays valid until the next ``tick``; ``last`` closes the stream.
        ``count`` 0 needs no source."""
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
        return st.closed and st.emitted >= st.ready()

    def plan(self):
        """What the next tick does, from the host state alone (no device, nothing changes)."""
        return EmitPlan(self.streams)

    def commit(self, plan):
        """Move the streams on to behind the planned tick."""
        for sid, _, n_new, _ in plan.rows:
            st = self.streams[sid]
            st.on_device, st.queue = st.have, []
            st.emitted += n_new

    # -- device side --------------------------------------------------------------------------------------------------
    def _word5(self, st):
        return 0

    def tick(self):
        """Append what was pushed to the rings and emit every output that became final.
        Returns {stream_id: float32 ndarray} for the streams with new output."""
        plan = self.plan()
        self.last_emit_device = None
        if not plan.rows:
            return {}
        import torch
        from .abi import _check, load_library
        lib, dev = load_library(), self._resolve_device()
        held = ((st.slot, st.on_device) for st in self.streams.values() if st.on_device)
        self.device_allocations += self._store.ensure(dev, plan.ring_needed, held)
        for sid, _, _, _ in plan.rows:
            for source, _, _ in self.streams[sid].queue:
                if source.device != dev:
                    raise ValueError(f"stream {sid!r}: source is on {source.device}, the stage on {dev}")
        rings, n_app, used, total = self._store.rings, plan.n_app, plan.words, plan.starts[-1]
        store = (rings.data_ptr(), int(rings.shape[0]), self._store.ring_samples)
        self._desc_host, self._desc_dev = self._grown_pair(self._desc_host, self._desc_dev, used, torch.int64)
        plan.pack(self._desc_host.numpy(), self._word5)
        self._out_host, self._out_dev = self._grown_pair(self._out_host, self._out_dev, total, torch.float32)
        self._prepare(plan)
        with torch.cuda.device(dev):
            stream, base, events = self._upload(self._desc_host, self._desc_dev, used)
            first = 0
            for (_, ptr, numel), rows in plan.calls.items():
                _check(lib.mbxl_ring_append(ptr, numel, base + 32 * first, len(rows), max(rr[2] for rr in rows), *store,
                                            stream.cuda_stream))
                first += len(rows)
            for key, first, end, max_new in plan.groups:      # one launch per distinct key
                _check(self._launch(lib, key, store, base + 32 * n_app + 48 * first, end - first, max_new, stream.cuda_stream))
            packed = self._copy_back(stream, events, total)
        spans = {sid: (at, n_new) for (sid, _, n_new, _), at in zip(plan.rows, plan.starts) if n_new > 0}
        if total:
            self.last_emit_device = (self._out_dev, spans)
        self.commit(plan)
        self.ticks += 1
        return {sid: packed[at:at + n_new].copy() for sid, (at, n_new) in spans.items()}


class StreamingOutputResampler(_EmitStage):
    """The way out of a live stream: model-rate audio that is still being produced, resampled on the device to each
    stream's own output rate, a tick at a time (csrc/resample_stream.hip through include/mbexwn_live_out.h).

    The concatenated arrays ``tick`` hands out for a stream opened at rate R are ``resample.resample_device(the stream's
    whole model-rate sound, None, model_rate, R)`` bit for bit, ceil(n * up / down) samples, however the sound was cut into
    pushes.  The rules are those of the resampled input streams read in the other direction: with ``have`` model-rate
    samples appended, ``outputs_ready(have, up, down, half, closed)`` outputs are final; the ring (a third ``_RingStore``,
    at the model rate) holds every sample from ``input_keep_from(next output, ...)`` on; after ``push(..., last=True)`` the
    remaining outputs follow with the filter's tail clipped at the end.

    An emit stage (``_EmitStage``) whose key is the output rate: one ``mbxo_resample_emit`` per distinct rate."""
    _taps_to_model = False

    def __init__(self, model_rate, device=None, ring_samples=None, slots=16):
        # 4096: a synthesis tick of the 80 ms schedule hands over up to 7 frames = 2100 samples at once, behind the 44 to 130
        # samples (48 kHz to 8 kHz) a pending output still reads
        super().__init__(positive_rate(model_rate, "model_rate"), device, int(ring_samples or 4096), slots)

    def open(self, stream_id, output_rate):
        if stream_id in self.streams:
            raise ValueError(f"stream {stream_id!r} is open already")
        rate = positive_rate(output_rate, f"stream {stream_id!r}: output_rate")
        self.streams[stream_id] = _OStream(self._store.take(), rate, output_filter(self.model_rate, rate))

    def _prepare(self, plan):
        for rate, _, _, _ in plan.groups:
            self._device_taps(rate)

    def _launch(self, lib, rate, store, desc, n_rows, max_new, stream):
        taps, up, down = self._taps[rate]
        return lib.mbxo_resample_emit(*store, desc, n_rows, max_new, up, down, taps.data_ptr(), int(taps.numel()),
                                      self._out_dev.data_ptr(), int(self._out_dev.numel()), stream)


class StreamingLimiter(_EmitStage):
    """The last stage of a live stream: the look-ahead peak limiter of limiter.py on audio that is
    still being produced, a tick at a time (csrc/limiter.hip through ``mbxd_limit_emit``).

    The concatenated arrays ``tick`` hands out for a stream are ``limiter.limit_device`` on the stream's whole sound, bit
    for bit -- and so is ``stats(stream_id)`` --, however the sound was cut into pushes: with ``have`` samples appended,
    ``limiter.ready_outputs(have, h)`` outputs are final (output i once sample i + 2 h is there), every one once the
    stream is closed; the ring (a ``_RingStore`` at the stream's own rate) holds every sample from
    ``limiter.keep_from(next output, h, H)`` on.

    A stream has a fixed gain (it has no integrated loudness), a ceiling and a window at its rate.  An emit stage
    (``_EmitStage``) whose key is (window, ceiling): one ``mbxd_limit_emit`` per distinct one."""

    def __init__(self, device=None, ring_samples=None, slots=16):
        # 8192: two ticks of the 80 ms schedule at 48 kHz behind the 1068 samples a pending output still reads
        super().__init__(None, device, int(ring_samples or 8192), slots)
        self._stats = None            # int32 (slots, 4) on the device
        self._fresh = []              # slots of streams opened since the last tick: their statistics start over
        self._weights = {}            # h -> the weights on the device

    @staticmethod
    def check_open(stream_id, rate, gain_db=0.0, peak_limit=-1.0, lookahead_ms=None, hold_ms=None):
        """What ``open`` refuses, without opening: -> (rate, h, H, gain_db, peak_limit)."""
        from . import limiter
        rate = positive_rate(rate, f"stream {stream_id!r}: rate")
        gain_db, peak_limit = float(gain_db), float(peak_limit)
        if not (np.isfinite(gain_db) and np.isfinite(peak_limit)):
            raise ValueError(f"stream {stream_id!r}: gain_db and peak_limit must be finite, got {gain_db!r} and {peak_limit!r}")
        h, hold = limiter.window(rate, lookahead_ms, hold_ms)
        limiter.check_window(h, hold)
        return rate, h, hold, gain_db, peak_limit

    def open(self, stream_id, rate, gain_db=0.0, peak_limit=-1.0, lookahead_ms=None, hold_ms=None):
        if stream_id in self.streams:
            raise ValueError(f"stream {stream_id!r} is open already")
        rate, h, hold, gain_db, peak_limit = self.check_open(stream_id, rate, gain_db, peak_limit, lookahead_ms, hold_ms)
        slot = self._store.take()
        self.streams[stream_id] = _DStream(slot, rate, h, hold, np.float32(10.0 ** (gain_db / 20.0)),
                                           float(np.float32(10.0 ** (peak_limit / 20.0))))
        self._fresh.append(slot)

    def stats(self, stream_id):
        """``limiter.LimitStats`` of what the stream has been handed so far (a copy back; waits for the device)."""
        from .limiter import LimitStats
        st = self.streams[stream_id]
        if self._stats is None or st.slot in self._fresh:
            return LimitStats(np.float32(1.0), 0, 0)
        return LimitStats.from_words(self._stats[st.slot].cpu().numpy())

    def _prepare(self, plan):
        import torch
        from . import limiter
        self._stats = self._state_rows(self._stats, self._store.slots, limiter.STAT_WORDS)
        if self._fresh:
            # the tick behind an open: a small temporary on the device, counted like every other allocation
            self._stats[self._fresh] = torch.as_tensor([limiter.ONE_BITS, 0, 0, 0], dtype=torch.int32, device=self.device)
            self.device_allocations += 1
            self._fresh = []
        for (h, _, _), _, _, _ in plan.groups:
            if h not in self._weights:
                self._weights[h] = limiter.device_weights(h, self.device)
                self.device_allocations += 1

    def _word5(self, st):
        from .limiter import gain_bits
        return gain_bits(st.g0)

    def _launch(self, lib, key, store, desc, n_rows, max_new, stream):
        h, hold, ceiling = key
        return lib.mbxd_limit_emit(*store, desc, n_rows, max_new, ceiling, h, hold, self._weights[h].data_ptr(),
                                   self._out_dev.data_ptr(), int(self._out_dev.numel()), self._stats.data_ptr(), stream)


class _LStream:
    def __init__(self, hop, rng, noise_fn, up=1, down=1):
        self.factors = FrameFactors(hop, up, down)
        self.formants = None          # FrameFactors of the formant shift, from the first push that gives one
        self._rates = (hop, up, down)
        self.frames = 0               # mel frames handed to the synthesizer
        self.rng, self.noise_fn = rng, noise_fn
        self.flushed = False          # the synthesizer has been told that the stream is over
        self.out_rate = None          # the stream's output rate when it is not the model's: it goes through the output stage
        self.limited = False          # the stream leaves through the limiter, the last stage
        self.f0_hold = None           # f0_source="audio": the last voiced F0 (float32), what an unvoiced frame takes
        self.pending = None           # a decoding stream (f0_lag): the scaled mel rows that still wait for their decided F0


class LiveResynthesizer:
    """Audio in, audio out: a ``StreamingAnalyzer``, ``MELInverter.scale_mel`` (on the host: it is elementwise, so a chunk
    of frames scales to the bits the whole file scales to) and a ``StreamingSynthesizer``, a tick at a time.

    Transposition rule: a ``transposition`` factor given with ``push_audio`` applies to the mel frames whose centre sample
    t * hop lies in that push's sample range (``FrameFactors``); a push without one has factor 1.  For a stream opened at a
    ``sample_rate`` of its own (resampled on the device, see ``StreamingAnalyzer``) the centre of frame t is input sample
    (t * hop * down) // up.  A ``formant`` factor (formant shift) follows the same rule.

    Noise: the N(0,1) draw of the frames [a, b) of a stream is ``noise_fn(stream_id, a, b)`` ((b - a) * steps_per_frame
    float32 values); by default consecutive draws of a per-stream ``numpy.random.Generator`` seeded with ``seed``.

    A stream's output then equals ``mel_inverter.synth_from_mel(scale_mel(mell dictionary of the whole sound), noise=the
    same draw, transposition=the per-frame factors)`` bit for bit, when the engine is pinned to ``conv_form="f23"`` (the
    form the streams run) and the mel is the device analysis of the sound (``compute_log_mel_device``).

    Pitch source: a stream opened with ``f0_source="audio"`` sings with the pitch that is in the sound:
    the analyzer tracks its F0 on the device, every tick turns the tracked values into a positive contour by the causal
    rule of ``f0track.fill_hold`` -- an unvoiced frame holds the last voiced value, ``f0_initial`` in front of the first --
    and pushes it with the mel rows to a synthesizer stream opened with ``f0="frames"``.  The stream then equals
    ``MELInverter.transform_audio(f0_source="audio", f0_fill="hold", f0_initial=...)`` of the sound under the same noise.
    ``last_f0`` holds the raw tracked values of the last tick (0 = unvoiced).

    With ``f0_lag=N`` as well the stream's contour is decoded with a fixed lag of N frames (``StreamingAnalyzer``, DESIGN.md
    section 6l; ``f0_decode``: an ``f0decode.decode_params`` dictionary, None = the defaults).  Its scaled mel rows wait in
    a FIFO on the host: a tick pushes as many of them to the synthesizer as frames were decided, with the contour, noise,
    transposition and formant factors of exactly those frames; a tick that decides nothing pushes nothing, the closing tick
    everything.  The stream then equals ``MELInverter.transform_audio(f0_source="audio", f0_decode=..., f0_lag=N,
    f0_fill="hold")`` of the sound under the same noise, N frames later."""

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
        # streams with a peak limit leave through the limiter, at the rate they are handed out at; allocated by its first tick
        self.limiter = StreamingLimiter(device=engine.device)

    @property
    def lookahead_ms(self):
        """The analysis look-ahead -- half a window, rounded up to the next frame -- plus the synthesizer's own."""
        an = self.analyzer
        frames = -(-(an.win - an.win // 2) // an.hop)
        return 1000.0 * frames * an.hop / an.sample_rate + self.synthesizer.lookahead_ms

    last_f0 = property(lambda self: self.analyzer.last_f0)      # {stream_id: (f0, periodicity)} of the last tick

    def _f0_params(self, f0_params):
        from .f0track import check_params, params
        return params(self.analyzer.model_rate) if f0_params is None else check_params(dict(f0_params))

    def lookahead_ms_for(self, sample_rate=None, output_rate=None, f0_source="net", f0_params=None, f0_lag=None,
                         peak_limit=None, limiter_lookahead_ms=None):
        """``lookahead_ms`` of a stream opened at ``sample_rate`` and ``output_rate``: a resampled stream waits for half
        its filter as well, half / up input samples (0.92 ms at 44.1 and 48 kHz, 1.4 ms at 16 kHz for a 24 kHz model); a
        stream with an output rate waits for half the output filter, half / up model-rate samples (0.92 ms to 48 kHz,
        0.94 ms to 44.1 kHz, 1.4 ms to 16 kHz).  With ``f0_source="audio"`` a frame waits for its F0 frame too, L = window
        + tau_max of ``f0_params`` (None: the defaults) samples about its centre: the analysis part is
        ceil(max(win - win // 2, L - L // 2) / hop) frames -- 3 instead of 2 with the defaults at 24 kHz.  ``f0_lag=N`` adds
        the decoder's N frames, 1000 N hop / sample_rate ms.  A stream with a ``peak_limit`` waits for the limiter's
        look-ahead, 2 h samples at the rate it is handed out at (``limiter.window`` of ``limiter_lookahead_ms``)."""
        model = self.analyzer.model_rate
        ms = self.lookahead_ms
        if f0_source not in ("net", "audio"):
            raise ValueError(f"f0_source must be 'net' or 'audio', got {f0_source!r}")
        if f0_source == "audio":
            an, prm = self.analyzer, self._f0_params(f0_params)
            reach, f0_len = an.win - an.win // 2, int(prm["window"]) + int(prm["tau_max"])
            frames = -(-max(reach, f0_len - f0_len // 2) // an.hop)
            ms += 1000.0 * (frames - -(-reach // an.hop)) * an.hop / an.sample_rate
        if f0_lag is not None:
            from .f0decode import check_lag
            ms += 1000.0 * check_lag(f0_lag) * self.analyzer.hop / self.analyzer.sample_rate
        if sample_rate is not None and int(round(sample_rate)) != model:
            ms += resampling_lookahead_ms(sample_rate, model)
        out_rate = resolve_output_rate(output_rate, sample_rate, model)
        if out_rate is not None:
            ms += output_lookahead_ms(model, out_rate)
        if peak_limit is not None:
            from .limiter import window
            rate = model if out_rate is None else out_rate
            ms += 1000.0 * 2 * window(rate, limiter_lookahead_ms, 1000.0)[0] / rate
        return ms

    def open(self, stream_id, seed=None, noise_fn=None, sample_rate=None, output_rate=None, f0_source="net", f0_params=None,
             f0_initial=150.0, f0_decode=None, f0_lag=None, gain_db=0.0, peak_limit=None, limiter_lookahead_ms=None,
             limiter_hold_ms=None):
        """``output_rate``: the rate the stream's audio comes back at -- a rate in Hz, or ``"input"`` for the stream's own
        ``sample_rate``; None or the model's rate: the model-rate audio, as the synthesizer emits it.  ``f0_source``:
        ``"net"`` -- the F0-net's contour -- or ``"audio"``: the tracked pitch of the sound (``f0_params``: an
        ``f0track.params`` dictionary at the model rate, None = its defaults; ``f0_initial``: Hz of the frames in front of the
        first voiced one).  ``f0_lag``: frames of look-ahead of a decoded contour (0 .. 128, with ``f0_source="audio"``), by
        ``f0_decode`` (None: the defaults); ``f0_decode`` without a lag is refused: decoding the contour over the whole sound
        needs the whole sound.  ``peak_limit``: a ceiling in dBFS the stream is kept under by the look-ahead limiter
        (``StreamingLimiter``), the last stage, at the rate the stream is handed out at, behind the fixed
        gain ``gain_db`` -- a stream has no integrated loudness -- and with the window ``limiter_lookahead_ms`` /
        ``limiter_hold_ms``; the stream then equals ``limiter.limit_device`` on the whole output of the same stream without
        a peak limit.  None: the stream of before (the gain and the window go with a peak limit)."""
        if f0_source not in ("net", "audio"):
            raise ValueError(f"f0_source must be 'net' or 'audio', got {f0_source!r}")
        if peak_limit is None and (float(gain_db) != 0.0 or limiter_lookahead_ms is not None or limiter_hold_ms is not None):
            raise ValueError("gain_db, limiter_lookahead_ms and limiter_hold_ms go with a peak_limit")
        if f0_decode is not None and f0_lag is None:
            raise ValueError(f"stream {stream_id!r}: f0_decode decodes the contour over the whole sound (f0decode.py), which a "
                             "stream does not have; streams track every frame on its own")
        if f0_lag is not None and f0_source != "audio":
            raise ValueError("f0_lag goes with f0_source='audio'")
        hold = None
        if f0_source == "audio":
            f0_params = self._f0_params(f0_params)
            hold = np.float32(f0_initial)
            if not (np.isfinite(hold) and hold > 0):
                raise ValueError(f"f0_initial must be a finite positive frequency in Hz, got {f0_initial!r}")
        elif f0_params is not None:
            raise ValueError("f0_params go with f0_source='audio'")
        out_rate = resolve_output_rate(output_rate, sample_rate, self.analyzer.sample_rate)
        limit = None
        if peak_limit is not None:                          # before any stage knows the stream: a window the rate refuses
            limit = (self.analyzer.sample_rate if out_rate is None else out_rate, gain_db, peak_limit, limiter_lookahead_ms,
                     limiter_hold_ms)
            self.limiter.check_open(stream_id, *limit)
            if stream_id in self.limiter.streams:
                raise ValueError(f"stream {stream_id!r} is open already")
        self.analyzer.open(stream_id, sample_rate=sample_rate, f0_params=f0_params, f0_decode=f0_decode, f0_lag=f0_lag)
        self.synthesizer.open(stream_id, f0="net" if hold is None else "frames")
        up, down = (self.analyzer.streams[stream_id].filt or (1, 1))[:2]
        st = self.streams[stream_id] = _LStream(self.analyzer.hop, None if noise_fn else np.random.default_rng(seed),
                                                noise_fn, up, down)
        st.f0_hold = hold
        st.pending = None if f0_lag is None else np.zeros((0, self.dims.mel_channels), dtype=np.float32)
        st.limited = limit is not None
        if limit is not None:                               # the last stage, opened last: the checks above cannot fail it
            self.limiter.open(stream_id, *limit)
        if out_rate is not None:
            self.output.open(stream_id, out_rate)
            st.out_rate = out_rate

    def close(self, stream_id):
        self.analyzer.close(stream_id)
        self.synthesizer.close(stream_id)
        st = self.streams.pop(stream_id)
        if st.out_rate is not None:
            self.output.close(stream_id)
        if st.limited:
            self.limiter.close(stream_id)

    def push_audio(self, stream_id, samples, last=False, transposition=None, sample_rate=None, formant=None):
        """Append samples at the stream's rate (the model's, unless it was opened at another); ``transposition``: one finite
        positive factor for the frames centred in this push (see the class docstring); ``formant``: one finite positive
        formant-shift factor for the same frames -- the stream then equals ``MELInverter.transform_audio(formant=)`` of the
        sound under the same noise."""
        if formant is not None:
            formant = float(formant)
            if not (np.isfinite(formant) and formant > 0):
                raise ValueError("formant must be finite and positive")
        if transposition is not None:
            transposition = float(transposition)
            if not (np.isfinite(transposition) and transposition > 0):
                raise ValueError("transposition must be finite and positive")
        st = self.streams[stream_id]
        before = self.analyzer.streams[stream_id].in_have
        self.analyzer.push(stream_id, samples, last=last, sample_rate=sample_rate)
        count = self.analyzer.streams[stream_id].in_have - before
        if formant is not None and st.formants is None:
            # the first formant factor of the stream: the samples pushed so far had factor 1
            st.formants = FrameFactors(*st._rates)
            st.formants.add(st.factors.samples)
        st.factors.add(count, transposition)
        if st.formants is not None:
            st.formants.add(count, formant)
        if last:
            st.factors.close()
            if st.formants is not None:
                st.formants.close()

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
            tracked = self.analyzer.last_f0.get(sid, (np.zeros(0, dtype=np.float32),))[0]
            scaled = np.zeros((0, self.dims.mel_channels), dtype=np.float32)
            if rows is not None:
                scaled = self.mel_inverter.scale_mel(dict(self._header, mell=rows.T))[0]
            if st.pending is not None:
                # a decoding stream: the rows wait for their F0, and as many leave as frames were decided in this tick
                st.pending = np.concatenate((st.pending, scaled))
                scaled, st.pending = st.pending[:tracked.size], st.pending[tracked.size:]
                rows = scaled if tracked.size else None
            if rows is None and not (done and not st.flushed):
                continue
            n = 0 if rows is None else rows.shape[0]
            first, end = st.frames, st.frames + n
            noise = self._noise(sid, st, first, end) if self.dims.noise_sigma else None
            shift = {} if st.formants is None else {"formant": st.formants.take(first, end)}
            if st.f0_hold is not None:
                # the tick's tracked values as a positive contour, causally (the flush push carries an empty one)
                from .f0track import fill_hold
                shift["f0"] = fill_hold(tracked, st.f0_hold)
                if n:
                    st.f0_hold = shift["f0"][-1]
            self.synthesizer.push(sid, scaled, noise, last=done, transposition=st.factors.take(first, end), **shift)
            st.frames, st.flushed = end, done
        audio = self.synthesizer.tick()
        for stage in (self.output, self.limiter):
            if stage.streams:
                audio = self._hand_on(stage, audio)
        return audio

    def _hand_on(self, stage, audio):
        # the streams of an emit stage: what the stage in front of it left on the device in this tick -- the output resampler
        # for a limited stream with an output rate, else the synthesizer -- goes on to the stage, and what that has final
        # comes back in its place
        fronts = (self.synthesizer, self.output)
        places = [front.last_emit_device or (None, {}) for front in fronts]      # asked once: the synthesizer makes its own
        for sid, st in self.streams.items():
            if sid not in stage.streams or stage.streams[sid].closed:
                continue
            resampled = stage is self.limiter and st.out_rate is not None
            front, (source, spans) = fronts[resampled], places[resampled]
            offset, count = spans.get(sid, (0, 0))
            last = (front is self.output or st.flushed) and front.finished(sid)
            if count or last:
                stage.push(sid, source, offset, count, last=last)
            audio.pop(sid, None)
        audio.update(stage.tick())
        return audio

    def finished(self, stream_id):
        st = self.streams[stream_id]
        if st.limited:
            return self.limiter.finished(stream_id)
        if st.out_rate is not None:
            return self.output.finished(stream_id)
        return st.flushed and self.synthesizer.finished(stream_id)


def keyed_noise_fn(engine, seed):
    """A ``noise_fn(stream_id, a, b)`` for :meth:`LiveResynthesizer.open`: the keyed noise (include/mbexwn_noise.h,
    ``engine.keyed_noise``) of the frames [a, b) of the item ``stream_id`` -- an integer key, or a name whose key is
    ``noise.item_key(name)`` -- under ``seed``, counted from step ``a * steps_per_frame``, copied back to the host.  The
    stream then takes the values ``MELInverter.synth_from_mel(..., noise_seed=seed, noise_key=key)`` takes for the whole
    item, bit for bit, whatever its ticks are."""
    from .noise import item_key
    spf = int(engine.dims.steps_per_frame)

    def noise_fn(stream_id, first, end):
        count = (int(end) - int(first)) * spf
        if count <= 0:
            return np.zeros(0, dtype=np.float32)
        return engine.keyed_noise(seed, [item_key(stream_id)], [count], first_step=[int(first) * spf])[0].cpu().numpy()

    return noise_fn

"""The host side of the live streams (live.py) as pure arithmetic: the readiness rules (``frames_ready``, ``outputs_ready``,
``input_keep_from``), the mapping of per-push transposition factors to mel frames (``FrameFactors``), the counters of a
stream, and what one tick of the analyzer and of an emit stage does (``AnalysisPlan``, ``EmitPlan``).  numpy only -- no
torch, no engine -- so it runs and is tested without a device; live.py packs and uploads what a plan holds, launches, commits."""
from itertools import accumulate

import numpy as np


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


def f0_frames_ready(have, hop, L, closed=False):
    """Frames of a stream whose F0 the streaming tracker can compute once ``have`` samples have arrived: frame t reads the L =
    window + tau_max samples from t * hop - L // 2 on, so while the stream is open it is ready when t * hop - L // 2 + L <=
    have; a closed stream has all frames_total(have) frames (behind the end is silence, as offline)."""
    if closed:
        return frames_total(have, hop)
    need = L - L // 2
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


def rate_groups(rates, new):
    """(rate, first, end, largest of new[first:end] or 0) of every run of equal neighbours in ``rates``: one launch each."""
    first = 0
    for end in range(1, len(rates) + 1):
        if end == len(rates) or rates[end] != rates[first]:
            yield rates[first], first, end, max(0, *new[first:end])
            first = end


class _AStream:
    def __init__(self, slot, rate=None, in_slot=None, filt=None, f0_len=None):
        self.slot = slot
        self.f0_len = f0_len      # None, or L = window + tau_max of the stream's F0 tracker: a frame waits for its F0 frame too
        self.rate = rate          # None: pushes at the model rate; else the stream's own input rate
        self.in_slot = in_slot    # ... its slot in the input-rate ring store
        self.filt = filt          # ... and its filter: (up, down, half, n_taps)
        self.in_have = 0          # samples pushed at the stream's own rate (== have for a stream at the model rate)
        self.in_on_device = 0     # ... of which the input ring holds the newest (resampled streams only)
        self.have = 0             # model-rate samples so far: pushed, or final outputs of the resampler (outputs_ready)
        self.on_device = 0        # ... of which the ring holds [max(0, on_device - ring), on_device)
        self.emitted = 0          # frames handed out
        self.f0_decided = 0       # ... of which a decoding stream's fixed-lag decoder has decided the F0 (live.py, section 6l)
        self.closed = False
        self.queue = []           # pushed since the last tick
        self.fresh = True         # the slot's ring still holds another stream's samples: the stream's first tick zeroes it


def stream_frames_ready(st, hop, win, hold_first=False):
    """``frames_ready`` of an analyzer's stream; ``hold_first``: frame 0 waits for sample win // 2 (StreamingAnalyzer)."""
    if hold_first and not st.closed and st.have < win // 2 + 1:
        return 0
    ready = frames_ready(st.have, hop, win, st.closed)
    if st.f0_len is not None:     # a tracking stream hands out a frame when its mel window AND its F0 frame are there
        ready = min(ready, f0_frames_ready(st.have, hop, st.f0_len, st.closed))
    return ready


def _table(rows, width):
    return np.array(rows, dtype=np.int64).reshape(len(rows), width)


class AnalysisPlan:
    """One tick of the analyzer, planned on the host from its ``streams`` ({id: _AStream}) alone; building one changes
    nothing.  S streams have work -- samples to append or frames that became ready --, R of them are resampled.  The tables
    are int64, one row per stream, as include/mbexwn_live.h and include/mbexwn_live_resample.h lay them out.

    The streams that track F0 (``_AStream.f0_len``) come first among the rows, T of them: the tracker's launch reads the
    first T rows of ``frames``, the table of the mel launch.  Without such a stream the rows are in the order of ``streams``
    and T = 0: the plan of an analyzer that knows no tracker, field for field."""

    def __init__(self, streams, hop, win, hold_first=False):
        work = [(sid, st, stream_frames_ready(st, hop, win, hold_first) - st.emitted) for sid, st in streams.items()]
        work = [(sid, st, max(0, nn)) for sid, st, nn in work if nn > 0 or st.queue or st.have > st.on_device]
        work.sort(key=lambda item: item[1].f0_len is None)        # stable: the tracking streams in front
        self.T = sum(st.f0_len is not None for _, st, _ in work)
        sts = [st for _, st, _ in work]
        self.rows = [(sid, nn) for sid, _, nn in work]        # (stream_id, frames to hand out), in the order of ``streams``
        # the rows of the resampled streams, by rate (stable), are the rows of the two (R, .) tables: their samples go to the
        # input-rate store, their model-rate samples are made on the device
        self.resampled = sorted((row for row, st in enumerate(sts) if st.rate is not None), key=lambda row: sts[row].rate)
        rs = [sts[row] for row in self.resampled]
        self.S, self.R = S, R = len(sts), len(rs)
        # per row: the samples queued, at the stream's own rate (at the model rate in_have == have and in_on_device ==
        # on_device), where they start among the tick's packed samples, and the pushed arrays themselves
        self.counts = counts = [st.in_have - st.in_on_device for st in sts]
        self.offsets = offsets = list(accumulate(counts, initial=0))[:-1]
        self.queues = [st.queue for st in sts]
        self.body, self.samples = 16 * S + 20 * R, sum(counts)      # float32 words of the tables, in front of the samples
        # (S, 4) slot, abs_start, count, offset; a resampled stream appends nothing to its model-rate ring: the resampler does
        own = [cc if st.rate is None else 0 for st, cc in zip(sts, counts)]
        self.append = _table([(st.slot, st.on_device, cc, at) for st, cc, at in zip(sts, own, offsets)], 4)
        # (S, 4) slot, first_frame, n_frames, n_total or -1
        self.frames = _table([(st.slot, st.emitted, nn, st.have if st.closed else -1) for _, st, nn in work], 4)
        # (R, 4) in_slot, abs_start, count, offset and (R, 6) in_slot, out_slot, first_out, n_out_new, n_total_in or -1, 0
        self.in_append = _table([(sts[row].in_slot, sts[row].in_on_device, counts[row], offsets[row])
                                 for row in self.resampled], 4)
        new = [st.have - st.on_device for st in rs]
        self.in_resample = _table([(st.in_slot, st.slot, st.on_device, nn, st.in_have if st.closed else -1, 0)
                                   for st, nn in zip(rs, new)], 6)
        self.groups = list(rate_groups([st.rate for st in rs], new))      # (rate, first, end, max_out) over the (R, .) tables
        self.max_new, self.max_model = max((nn for _, nn in self.rows), default=0), max(own, default=0)   # the launches' sizes
        self.max_in = max((counts[row] for row in self.resampled), default=0)
        # the rings hold every sample from the first one a pending frame may read -- the start of the window of the next frame
        # to hand out, less the two samples the reflection at the end can reach in front of it -- to the newest one pushed
        # (a tracking stream's next F0 frame starts L // 2 in front of its centre, which may be further back)
        self.ring_needed = max((st.have - max(0, st.emitted * hop - max(win // 2 + 2, (st.f0_len or 0) // 2)) for st in sts),
                               default=0)
        # ... the input rings from the first one a pending output may read (never behind what is to be appended)
        self.in_ring_needed = max((st.in_have - min(input_keep_from(st.on_device, *st.filt), st.in_on_device) for st in rs),
                                  default=0)
        self.fresh = [st.slot for st in sts if st.fresh]      # slots that still hold another stream's samples

    def pack(self, stage):
        """The tick's upload into ``stage`` (float32, ``body + samples`` words or more): the two (S, 4) tables in 16 S
        words, the (R, 4) one in 8 R, the (R, 6) one in 12 R, then the queued samples back to back."""
        np.concatenate([tt.ravel() for tt in (self.append, self.frames, self.in_append, self.in_resample)],
                       out=stage[:self.body].view(np.int64))
        if self.samples:
            np.concatenate([part for queue in self.queues for part in queue], out=stage[self.body:self.body + self.samples])


class _EStream:
    """A stream of an emit stage (live.py: ``_EmitStage``): samples that are named on the device go into its ring, the outputs
    that became final leave in packed rows.  A subclass gives the two rules: ``ready()``, how many outputs are final, and
    ``keep_from()``, the first sample a pending output still reads."""

    def __init__(self, slot, rate, key):
        self.slot, self.rate = slot, rate
        self.key = key            # what one launch of the stage shares: the streams of a tick are grouped by it
        self.have = 0             # samples pushed
        self.on_device = 0        # ... of which the ring holds the newest
        self.emitted = 0          # outputs handed out
        self.closed = False
        self.queue = []           # (source, offset, count) pushed since the last tick


class _OStream(_EStream):
    def __init__(self, slot, rate, filt):
        super().__init__(slot, rate, rate)
        self.filt = filt          # (up, down, half, n_taps), model rate -> rate

    def ready(self):
        return outputs_ready(self.have, *self.filt[:3], closed=self.closed)

    def keep_from(self):
        return input_keep_from(self.emitted, *self.filt)


class _DStream(_EStream):
    def __init__(self, slot, rate, h, hold, g0, ceiling):
        super().__init__(slot, rate, (h, hold, ceiling))      # one launch of the limiter shares the window and the ceiling
        self.g0 = g0

    def ready(self):
        """``limiter.ready_outputs``: output i once sample i + 2 h is there, or the stream is closed."""
        from .limiter import ready_outputs
        return ready_outputs(self.have, self.key[0], self.have if self.closed else None)

    def keep_from(self):
        from .limiter import keep_from
        return keep_from(self.emitted, *self.key[:2])


class EmitPlan:
    """One tick of an emit stage, planned on the host from its ``streams`` ({id: _EStream}) alone; building one changes
    nothing.  The streams with work have samples to append or outputs that became final.  The descriptor tables are int64
    as include/mbexwn_live.h (append rows), include/mbexwn_live_out.h and include/mbexwn_limiter.h (emit rows) lay them
    out; a source is anything with ``data_ptr()`` and ``numel()``, and is asked only when the tables are."""

    def __init__(self, streams):
        self.rows, self._streams = [], []     # (stream_id, first_out, n_new, n_total or -1) per stream with work, by key (stable)
        self.ring_needed = 0                  # the samples the longest-held stream's ring must hold
        for sid, st in sorted(streams.items(), key=lambda kv: kv[1].key):
            n_new = st.ready() - st.emitted
            if n_new > 0 or st.queue:
                self.rows.append((sid, st.emitted, n_new, st.have if st.closed else -1))
                self._streams.append(st)
                # from the first sample a pending output may still read (never behind what is to be appended)
                self.ring_needed = max(self.ring_needed, st.have - min(st.keep_from(), st.on_device))
        new = [row[2] for row in self.rows]
        self.groups = list(rate_groups([st.key for st in self._streams], new))      # (key, first, end, max_new) over the rows
        self.starts = list(accumulate((max(nn, 0) for nn in new), initial=0))       # where a row's outputs go; [-1]: their sum
        self._calls = None

    @property
    def calls(self):
        """The append rows of the tick: one call per distinct source tensor (and per place in its stream's queue: two rows of
        one call never name the same slot) -> {(turn, address, elements): [(slot, abs_start, count, offset)]}."""
        if self._calls is None:
            self._calls = calls = {}
            for st in self._streams:
                at = st.on_device
                for turn, (source, offset, count) in enumerate(st.queue):
                    calls.setdefault((turn, source.data_ptr(), source.numel()), []).append((st.slot, at, count, offset))
                    at += count
        return self._calls

    @property
    def n_app(self):
        return sum(len(rows) for rows in self.calls.values())

    @property
    def words(self):
        """int64 words of the tick's upload: the (n_app, 4) append rows, call by call, then the (S, 6) emit rows."""
        return 4 * self.n_app + 6 * len(self.rows)

    def pack(self, desc, word5_of):
        """The tick's upload into ``desc`` (int64, ``words`` or more); ``word5_of(stream)``: the sixth word of its emit row."""
        app = [row for rows in self.calls.values() for row in rows]
        emit = [(st.slot, first_out, n_new, n_total, at, word5_of(st))
                for st, (_, first_out, n_new, n_total), at in zip(self._streams, self.rows, self.starts)]
        desc[:self.words] = [word for row in app + emit for word in row]


OutputPlan = LimiterPlan = EmitPlan       # the names the two emit stages' plans had when they were two classes

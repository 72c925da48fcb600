"""Chunked (streaming) mel inversion that reproduces the whole-utterance output.

The reference has no streaming mode: its graph is non-causal (``padding="SAME"``) and the author notes that causal
operation "would require a dedicated implementation" (reference custom_pulsed_generator.py:213-217).  This module
serves BASELINE config 5 (many concurrent streams, short ticks) on top of the offline engine:

* every op of the graph has a finite receptive field, so the audio of mel frames [t0, t0+chunk) only depends on
  the mel frames [t0-LEFT, t0+chunk+RIGHT): a tick runs the engine on that window and keeps the middle;
* the one unbounded dependency is the wavetable phase accumulator (float32 running sum in 1000-sample chunks,
  reference tf_wavetable.py:429-492): its state (running sum of the chunk in progress, un-wrapped offset sum,
  position in the chunk) is carried from tick to tick through ``mbx_forward_stream`` -- the phase inside a window is
  then bit-identical to the offline phase;
* at the true start / end of an utterance the window edge IS the utterance edge, so the reference's boundary
  semantics (symmetric / zero padding, un-normalised head and tail of the inverse STFT) apply where they should.

Receptive field in mel frames (canonical model): F0-net 3 convs k=3 (+-3) and the interpolator (+1); the phase needs
valid F0, so pulses are valid from window frame 4; WaveNet (dilations 1..16, k=3: +-31 steps, + 9 steps of conditioning
interpolation towards a row that a region's end clamps = 2 frames) -> 6;
PQMF (+-4 steps) -> 7; STFT frame + overlap-add (-3 / +4 frames) -> LEFT = 10, RIGHT = 11 (look-ahead 137.5 ms).
``StreamingSynthesizer`` derives the margins from the model configuration.  A force_causal model (every convolution
padded in front only) needs no look-ahead in its sub-nets and WaveNet: 87.5 ms of the same model (stream_margins).
"""
from dataclasses import dataclass, field, fields
from types import SimpleNamespace

import numpy as np

from .stream_plan import StreamGeometry, plan_tick


def pack_state(cum=0.0, offset_sum=0.0, pos_in_chunk=0, start_sample=0, save_sample=-1):
    """One ``mbx_stream_state`` as 6 int32 words (floats bit-cast)."""
    ff = np.asarray([cum, offset_sum], dtype=np.float32).view(np.int32)
    return np.asarray([ff[0], ff[1], pos_in_chunk, start_sample, save_sample, 0], dtype=np.int32)


def norm_reach(dims, config):
    """Reach in mel frames of the optional RMS normalisation of the mel input (reference wavegen_1d.py:697-726): every
    smoothing iteration overlap-adds the per-frame RMS with the smoothing window and re-estimates it through the analysis
    window, i.e. frame t then depends on the frames within (smooth_win + win) / (2 hop) of it; 0 without normalisation."""
    if not dims.normalize_rms_from_mell:
        return 0
    from .norm_mel import NormMel
    nm = NormMel(config)
    return nm.iters * ((nm.smooth_win_size + nm.win) // (2 * nm.hop))


def cond_chain_reach(dims):
    """(left, right) reach in mel frames of the conditioning chain -- the conditioning layer and the pre-conditioning
    convolutions in front of it, all with kernel size cond_kernel_size and zero SAME padding, which the library pads
    (k - 1) // 2 frames in front and k // 2 behind (csrc/mbx_create.hip, cond_chain): an even kernel size reaches one frame
    further to the right than to the left, per convolution.  CAUSAL WaveNet padding: k - 1 frames in front, none behind."""
    n_cond = 0 if dims.wn_disable_conditioning else 1 + len(dims.wn_pre_cond_channels)
    if dims.wn_padding == "CAUSAL":
        return n_cond * (dims.cond_kernel_size - 1), 0
    return n_cond * ((dims.cond_kernel_size - 1) // 2), n_cond * (dims.cond_kernel_size // 2)


def subnet_reach(specs, causal=False):
    """(left, right) reach in mel frames of an F0- / VTF-net: per convolution its pads (subnet.build_subnet), counted in
    frames whatever the rate the layer runs at -- the larger half in front, or everything in front under force_causal."""
    left = right = 0
    for spec in specs:
        if spec[0] == "L":
            continue
        ks = int(spec[0])
        left += ks - 1 if causal else (ks - 1) // 2 + ((ks - 1) % 2)
        right += 0 if causal else (ks - 1) // 2
    return left, right


def wavenet_reach(dims):
    """(left, right) reach in mel frames of the WaveNet: the rows at the start / end of a region that are not those of a
    whole-utterance run.  SAME padding: the receptive field (k - 1) / 2 * d per layer, plus the cond_lin_upsampling - 1 last
    rows of every layer, which interpolate the conditioning towards a clamped row -- an error that spreads backwards
    through the layers behind -- on both sides.  CAUSAL padding: (k - 1) d per layer to the left; to the right only the
    clamped conditioning tail, which no layer carries backwards."""
    spf = dims.steps_per_frame
    tail = dims.cond_lin_upsampling - 1
    if dims.wn_padding == "CAUSAL":
        left = sum(dims.wn_dilation(ll) * (dims.wn_kernel_size - 1) for ll in range(dims.wn_layers))
        return -(-left // spf), -(-tail // spf)
    steps = sum(dims.wn_dilation(ll) * (dims.wn_kernel_size - 1) // 2 for ll in range(dims.wn_layers)) + tail
    return -(-steps // spf), -(-steps // spf)


def stream_margins(dims, config):
    """(left, right, pulse_lead, act_left, act_right, wn_reach) in mel frames, from the layer geometry of the model;
    wn_reach = the WaveNet's reach behind a region's end (wavenet_reach; SAME padding: the same in front).

    Every reach follows the model's padding.  force_causal sub-nets reach ks - 1 frames to the left and none to the right,
    a CAUSAL WaveNet 2 sum(d) steps to the left and its conditioning tail to the right.  The SMALL model of
    tests/test_gpu_streaming.py (C = 32, 5 layers, d = 1 .. 16, PQMF 1 frame, STFT 3 / 4 frames):

        model                 lead       WaveNet (l, r)   left   right   look-ahead
        SAME                  3 + 1 = 4  (2, 2)           10     11      137.5 ms
        force_causal          6 + 1 = 7  (4, 1)           15      7       87.5 ms
        WaveNet CAUSAL only   3 + 1 = 4  (4, 1)           12     10      125.0 ms

    (force_causal: left = lead 7 + WaveNet 4 + PQMF 1 + STFT 3 = 15; right = max(F0-net 0 + interpolation 1, conditioning
    chain 0 + 1) + 1 + 1 + 4 = 7.  WaveNet CAUSAL only: the SAME sub-nets keep right = max(3 + 1, 1 + 1) + 1 + 1 + 4 = 10.
    What is left of the look-ahead is the non-causal back end: PQMF, the STFT frame / overlap-add and the F0 smoother.)"""
    mb = config["mbexwn_config"]
    nr = norm_reach(dims, config)      # the normalised mel of a window is reproducible nr frames inside its edges only
    causal = dims.force_causal
    f0_l, f0_r = subnet_reach(mb["pp_subnet"], causal)
    f0_r += 1                                             # interpolation towards the next frame
    # the conditioning is interpolated towards the next conditioning row, which at the end of a region is the clamped
    # last one: the last cond_lin_upsampling - 1 rows of every layer's gate are off (wavenet_reach)
    wn_left, wn_right = wavenet_reach(dims)
    pqmf_frames = -(-(int(mb["multi_band_config"]["taps"]) // 2) // dims.hop_size)
    # conditioning chain: the conditioning layer and the pre-conditioning convolutions in front of it (same kernel size,
    # zero SAME padding: (k - 1) // 2 frames to the left, k // 2 to the right, per convolution); + 1: the interpolation
    # towards the next conditioning row
    cond_l, cond_r = cond_chain_reach(dims)
    cond_r += 1
    vt_l, vt_r = (0, 0) if dims.no_envelope else subnet_reach(mb["ps_subnet"], causal)     # cepstrum of a frame <- mel frames around it
    stft_l, stft_r = 3, 4                                  # frame t reaches excitation frames t-3 .. t+4
    # first window frame whose mel-rate inputs of the WaveNet -- F0 / phase and the conditioning rows -- are reproducible
    pulse_lead = nr + max(f0_l + 1, cond_l)
    left = pulse_lead + wn_left + pqmf_frames + stft_l
    right = nr + max(f0_r, cond_r) + wn_right + pqmf_frames + stft_r
    # the envelope filter of the frames around the emitted ones needs their cepstra
    left = max(left, nr + vt_l + stft_l)
    right = max(right, nr + vt_r + stft_r)
    smooth = 3                                             # F0 smoother of the lifter selection: +-3 frames of valid F0
    left = max(left, pulse_lead + smooth + 1)
    right = max(right, nr + f0_r + smooth + 2)
    # margins of the stages from the WaveNet on (the active region of a window, mbx_forward_options.active_begin)
    act_left = wn_left + pqmf_frames + stft_l
    act_right = wn_right + pqmf_frames + stft_r
    return left, right, pulse_lead, act_left, act_right, wn_right


def frontend_reach(dims, config):
    """(left, right) reach in mel frames of the mel-rate front end (F0-net, VTF-net, conditioning convolution): the output
    of frame t depends on the mel frames [t - left, t + right]."""
    mb = config["mbexwn_config"]
    f0_l, f0_r = subnet_reach(mb["pp_subnet"], dims.force_causal)
    vt_l, vt_r = subnet_reach(mb["ps_subnet"], dims.force_causal)
    # the conditioning layer and the pre-conditioning convolutions in front of it (same kernel size and padding)
    ck_l, ck_r = cond_chain_reach(dims)
    # + 1: the interpolators (F0 contour, conditioning rows) reach the next frame
    return max(f0_l, vt_l, ck_l), max(f0_r, vt_r, ck_r) + 1


class _Stream:
    def __init__(self):
        # the frames a stream has received live in the synthesizer's shared input buffers (row `slot`): absolute frame f
        # sits at column f - base; frames in front of the next window are dropped when the row runs full
        self.base = 0             # absolute frame at column 0 of the stream's row
        self.have = 0             # frames received so far (absolute)
        self.emitted = 0          # frames of audio already produced
        self.closed = False
        self.slot = -1            # row of the synthesizer's sub-band store
        self.carry_pos = None     # the store holds the sub-bands of frames [carry_pos - sr_left, + carry_frames)
        self.carry_frames = 0
        self.layer_end = None     # the layer store holds the WaveNet state of a region that ended at this frame
        # phase state valid just in front of absolute pulse sample `state_frame * pulse_per_frame`
        self.state = (0.0, 0.0, 0)
        self.state_frame = 0
        self.ticks = 0            # chunks emitted so far: position in the synthesizer's tick schedule
        self.f0_mode = "net"      # "frames": the contour comes from push(f0=...) instead of the F0-net


class _InputRows:
    """Input frames of every stream, one row per slot (shared so that a tick gathers its frames with one indexed copy): mel
    and noise, and next to them the per-frame pitch control -- F0 in Hz ("frames" streams; 1 where none was given, never
    read there) and the transposition factor (1 where none was given) -- and the formant-shift factor (1 where none was given)."""

    def __init__(self, mel_channels, steps_per_frame, cap=256):
        self._widths = (mel_channels, steps_per_frame)
        self.cap = cap            # frames per row (grows on demand)
        self.mel, self.noise, self.f0, self.scale, self.formant = self._alloc(0, cap)

    def _alloc(self, slots, cap):
        return (np.zeros((slots, cap, self._widths[0]), dtype=np.float32),
                np.zeros((slots, cap, self._widths[1]), dtype=np.float32),
                np.ones((slots, cap), dtype=np.float32), np.ones((slots, cap), dtype=np.float32),
                np.ones((slots, cap), dtype=np.float32))

    def _arrays(self):
        return self.mel, self.noise, self.f0, self.scale, self.formant

    @property
    def slots(self):
        return self.mel.shape[0]

    def grow(self, slots, cap):
        """Make the rows at least (slots, cap frames) large, keeping their contents."""
        if slots <= self.slots and cap <= self.cap:
            return
        old = self._arrays()
        self.mel, self.noise, self.f0, self.scale, self.formant = self._alloc(max(slots, self.slots), max(cap, self.cap))
        for new, was in zip(self._arrays(), old):
            new[:was.shape[0], :was.shape[1]] = was
        self.cap = self.mel.shape[1]

    def drop_front(self, slot, n, live):
        """Move the `live` frames behind the first n of a row to its front."""
        for arr in self._arrays():
            arr[slot, :live] = arr[slot, n:n + live]

    def append(self, slot, col, mel, noise=None, f0=None, scale=None, formant=None):
        n = mel.shape[0]
        self.mel[slot, col:col + n] = mel
        if noise is not None:
            self.noise[slot, col:col + n] = noise
        self.f0[slot, col:col + n] = 1.0 if f0 is None else f0
        self.scale[slot, col:col + n] = 1.0 if scale is None else scale
        self.formant[slot, col:col + n] = 1.0 if formant is None else formant

    def window(self, slot, lo, hi):
        """(mel, noise, f0, scale, formant) of the columns [lo, hi) of a row (views)."""
        return tuple(arr[slot, lo:hi] for arr in self._arrays())

    def gather(self, slots, cols, **into):
        """Copy the columns cols (n, k) of the rows slots (n,) of the named arrays into the given destinations, e.g.
        ``gather(slots, cols, mel=dst)``: one indexed copy per array."""
        for name, dst in into.items():
            np.copyto(dst, getattr(self, name)[slots[:, None], cols])


class _Layout:
    """Named fields packed back to back into one flat 4-byte buffer (what a tick uploads in one copy).  ``fields``: (name,
    shape, "int32" / "float32"); ``views`` cuts any such buffer -- host or device, numpy or torch -- into its fields,
    bit-casting those whose type is not the buffer's.  An empty field is None.  The only place that knows an offset."""

    def __init__(self, fields):
        self.fields, self.size = [], 0
        for name, shape, dtype in fields:
            count = int(np.prod(shape))
            self.fields.append((name, slice(self.size, self.size + count), tuple(shape), dtype))
            self.size += count

    def views(self, buf):
        if isinstance(buf, np.ndarray):
            ns = np
        else:
            import torch as ns
        out = SimpleNamespace()
        for name, where, shape, dtype in self.fields:
            part = buf[where] if where.stop > where.start else None
            if part is not None and part.dtype != getattr(ns, dtype):
                part = part.view(getattr(ns, dtype))
            setattr(out, name, None if part is None else part.reshape(shape))
        return out


def _stage_layout(B, chunk, tpad, mel_channels, spf, use_noise, control, formant=False):
    """The (float32) stage buffer of a replayed tick: new mel frames, new noise, phase states, ring positions and -- once
    the synthesizer has seen pitch control / a formant shift -- the control rows / the formant factors of the whole windows
    (what a tick does not upload is empty)."""
    return _Layout([("mel", (B, chunk, mel_channels), "float32"), ("noise", (B, chunk * spf * use_noise), "float32"),
                    ("states", (B, 6), "int32"), ("fpos", (B,), "int32"),
                    ("f0_frames", (B, tpad * control), "float32"), ("f0_scale", (B, tpad * control), "float32"),
                    ("formant", (B, tpad * formant), "float32")])


@dataclass
class _TickInputs:
    """What a launch-by-launch tick uploaded: the windows and every int32 argument of the call (one buffer, cut)."""
    mel: object
    noise: object
    tpad: int
    args: object              # device views: states, desc, ldesc, nfr, act, wn, fpos, f0_item_mask, f0_frames, f0_scale, formant
    use_fe: bool
    control: bool
    f0_mask: object           # host copy of f0_item_mask, or None without control
    formant: bool = False     # the call carries the formant factors of the whole windows


@dataclass
class _Phase:
    """A recorded steady tick of one phase of the schedule: the window-relative constants of its engine call."""
    phase: int
    chunk: int
    T: int
    tpad: int
    a0: int
    wa: int
    lo: int                   # the emitted samples are the columns [lo, hi) of the audio
    hi: int
    layer_rows: int
    act: np.ndarray
    wn: np.ndarray
    nfr: np.ndarray
    desc: np.ndarray
    ldesc: np.ndarray
    state_consts: np.ndarray
    rel0: int                 # frame of the window at which the emitted frames start
    use_fe: bool
    frames: int
    active_frames: int
    wavenet_frames: int
    control: bool
    f0_mask: object
    formant: bool = False

    def same_geometry(self, other):
        for ff in fields(self):
            mine, theirs = getattr(self, ff.name), getattr(other, ff.name)
            same = np.array_equal(mine, theirs) if isinstance(mine, np.ndarray) else mine == theirs
            if not same:
                return False
        return True


@dataclass
class _CapturedTick:
    """The captured launch sequence of one phase and the fixed buffers it works on."""
    graph: object
    stage_host: object        # pinned; `host` are its fields as numpy views (_stage_layout)
    host: object
    arange: np.ndarray
    arange_win: np.ndarray
    audio_host: object
    state_host: object
    shift: int
    keep: int
    keep_alive: tuple


@dataclass
class _SteadyRun:
    """A run of steady ticks: its streams, the recorded phases and their graphs, and where it stands -- the streams'
    progress and phase states as vectors (replayed ticks keep them there, _sync_streams writes them back)."""
    sids: list
    streams: list
    B: int
    tpad: int
    slots: np.ndarray
    phases: dict = field(default_factory=dict)        # phase of the schedule -> _Phase
    graphs: dict = field(default_factory=dict)        # phase of the schedule -> _CapturedTick
    win: object = None        # the device-resident windows (mel, noise) all captured phases work on
    audio_buf: object = None  # ... and their shared outputs
    state_out: object = None
    state_host: object = None
    win_src: object = None    # the tensors that hold the windows of the last tick: `win`, or what that tick uploaded
    state_v: object = None
    emitted_v: object = None
    next_phase: int = 0
    pending: int = 0          # replayed ticks (and their frames) not yet written back to the streams
    pending_frames: int = 0
    need_v: object = None     # cached per-stream vectors; only push() changes them
    base_v: object = None


class StreamingSynthesizer:
    """Serves any number of concurrent streams with one batched engine call per tick."""

    def __init__(self, engine, chunk_frames=8):
        """``chunk_frames``: frames a stream emits per tick -- an int, or a cyclic schedule of ints for tick lengths that
        are not a whole number of frames: BASELINE config 5's 80 ms are 6.4 frames of 12.5 ms, which the schedule
        (6, 6, 7, 6, 7) delivers exactly on average (32 frames = 400 ms per period).  Every stream walks the schedule from
        its own first tick.  The geometry of a steady tick (position of the aligned window start relative to the emitted
        frames, window length) repeats with the period of the schedule when that period is a multiple of the window
        alignment (8 frames for the canonical model: 8-frame ticks, or the 32-frame period of the 80 ms schedule): each
        phase of the period then has its own captured hipGraph, all of them working on one device-resident window; any
        other schedule runs launch by launch (still with the carried sub-bands, per-layer state and phase)."""
        self.engine = engine
        self.dims = engine.dims
        # stream windows run the float32 F(2,3) / direct gate kernels whatever the handle's precision: an engine with the
        # opt-in split half precision would synthesise offline with other kernels than its streams, and the documented
        # bit-equality between a stream and the offline synthesis would silently not hold
        info = engine.conv_form_info()
        if info.get("split_f16_layers", 0) > 0 or info.get("split_f16_gate_layers", 0) > 0:
            raise ValueError("StreamingSynthesizer needs a float32 engine: this one runs its whole-item forwards in split half "
                             "precision (precision='split_f16'), streams would not be bit-equal to its offline synthesis")
        self.schedule = [int(chunk_frames)] if np.isscalar(chunk_frames) else [int(cc) for cc in chunk_frames]
        if not self.schedule or min(self.schedule) < 1:
            raise ValueError("chunk_frames must be a positive int or a non-empty schedule of positive ints")
        self.uniform = len(set(self.schedule)) == 1
        if self.uniform:
            self.schedule = self.schedule[:1]
        self.chunk = self.schedule[0] if self.uniform else min(self.schedule)
        (self.left, self.right, self.lead, self.act_left, self.act_right,
         self.wn_reach) = stream_margins(engine.dims, engine.config)
        # the WaveNet's reach in front of a region (wn_left) and behind it (wn_reach); equal under SAME padding
        self.wn_left = wavenet_reach(engine.dims)[0]
        # sub-band rows carried from tick to tick: the stages behind the WaveNet reach sr_left frames in front of the
        # emitted ones and sr_right behind them; these frames were computed exactly by the previous tick, so the WaveNet
        # of a tick only runs on the frames behind them (plus its own reach)
        self.sr_left = self.act_left - self.wn_left
        self.sr_right = self.act_right - self.wn_reach
        self.carry = True
        self._store = None            # (slots, (sr_left + sr_right) * steps_per_frame, subbands) on the device
        # per-layer WaveNet state carried from tick to tick (mbx_forward_options.layer_store): layer l is exact up to its
        # own reach in front of layer l-1, so a steady tick runs every layer on the new rows only instead of on the
        # region [emitted, emitted + chunk + act_right) with the WaveNet's reach recomputed on both sides
        ff, reach, min_rows = engine.layer_state_info()
        self.layer_carry = ff > 0 and reach == self.wn_reach * engine.dims.steps_per_frame
        self._layer_floats = ff
        self._layer_store = None      # (slots, floats per slot) on the device
        # mel-rate front end (conditioning rows, cepstrum, F0 contour) carried from tick to tick in a ring per stream: a
        # replayed steady tick runs the sub-nets only on the frames its new mel frames can reach
        self.fe_left, self.fe_right = frontend_reach(engine.dims, engine.config)
        self.fe_carry = bool(getattr(engine, "frontend_carry_supported", False)) and self.chunk >= self.fe_left
        ring = 1
        while ring < self.left + self.chunk + self.right + 2 * 16:
            ring *= 2
        self._fe_ring = ring
        self._fe_store = None         # (slots, ring frames, floats per frame) on the device
        self._free_slots = []
        self._rows = _InputRows(self.dims.mel_channels, self.dims.steps_per_frame)
        # Sticky: set by the first "frames" stream or the first transposition other than 1.  Until then a tick passes none
        # of the control arguments (the launch sequence and the captured graphs of a synthesizer that only resynthesises are
        # unchanged); from then on every tick passes the control rows of its whole windows -- factor 1 and mask 0 for the
        # streams without control, which changes no bit of theirs (the interpolated factor is exactly 1).
        self._control = False
        # The same for the formant shift: set by the first factor other than 1; from then on every tick passes the factors of
        # its whole windows -- 1 for the streams without, whose rows are then copied bit for bit.
        self._formant = False
        # The Winograd form of the dilated convolution pairs outputs t and t+d inside blocks of 2d steps counted from
        # the first row of the item; a window that starts on a multiple of 2*d_max steps pairs exactly like the offline
        # run, which keeps the streamed audio bit-identical (any other start is equal up to float32 rounding only).
        import math
        d_max = max(engine.dims.wn_dilation(ll) for ll in range(engine.dims.wn_layers))
        self.align = (2 * d_max) // math.gcd(2 * d_max, engine.dims.steps_per_frame)
        if engine.dims.wn_padding == "CAUSAL":
            # a causal WaveNet reaches further left than right: the carried sub-bands start far enough in front of the
            # emitted frames that the aligned start of a tick's WaveNet region never lies in front of them (the region
            # stays inside the active one), whatever the phase of the tick schedule
            self.sr_left = max(self.sr_left, self.align - 1 + self.wn_left - self.sr_right)
        # everything plan_tick needs to lay a tick out
        self.geometry = StreamGeometry(
            left=self.left, right=self.right, lead=self.lead, act_left=self.act_left, act_right=self.act_right,
            wn_left=self.wn_left, wn_reach=self.wn_reach, sr_left=self.sr_left, sr_right=self.sr_right, align=self.align,
            steps_per_frame=self.dims.steps_per_frame, pulse_per_frame=self.dims.pulse_per_frame,
            hop_size=self.dims.hop_size, carry=self.carry, layer_carry=self.layer_carry, layer_min_rows=min_rows,
            fe_ring=self._fe_ring)
        self.streams = {}
        # ticks of a schedule whose period is a whole number of alignment steps have a geometry that repeats per phase
        self.periodic = sum(self.schedule) % self.align == 0
        # frames of the device windows of such a schedule: every phase's window fits (uniform: the window length itself)
        self._tcap = 0 if self.uniform else self.left + max(self.schedule) + self.right + self.align
        # Steady ticks (every stream continues with the geometry of the tick before) are replayed as a captured hipGraph:
        # the windows stay on the device (mbx_window_advance appends the new frames), every integer argument of the call is
        # a constant of the capture, and one graph launch stands for the ~30 kernel launches of a tick.  This is the
        # practical form of BASELINE config 5's "persistent-kernel path": the launch sequence persists, not a kernel.
        self.use_graph = True
        self._inputs_changed = True
        self._steady = None               # the steady run in progress (_SteadyRun)
        self.graph_ticks = 0              # ticks served by a graph replay
        self.last_tick_replayed = False
        self._last_emit = None            # what last_emit_device is made from, on demand: a tick pays nothing for it
        self.time_device = False          # bench: bracket the engine call of a tick with events on its stream
        self.last_tick_device_ms = None
        self.last_tick_frames = 0         # window frames of the last tick (all streams): mel-rate stages
        self.last_tick_active_frames = 0  # frames of the active regions: PQMF, STFT filter, overlap-add
        self.last_tick_wavenet_frames = 0 # frames the WaveNet ran on
        self.last_tick_layer_rows = 0     # > 0: steady tick (every WaveNet layer ran on that many new rows per stream only)

    @property
    def lookahead_ms(self):
        return 1000.0 * self.right * self.dims.hop_size / self.dims.sample_rate

    @property
    def last_emit_device(self):
        """Where the last tick left its audio on the device: ``(tensor, {stream_id: (flat offset, count)})`` -- stream_id's
        chunk is the ``count`` elements from flat element ``offset`` of the contiguous float32 ``tensor`` (the forward's
        output of a launch-by-launch tick, the shared buffer of a replayed graph), valid until the next tick.  None after
        a tick that emitted nothing."""
        if self._last_emit is None:
            return None
        tensor, sids, spans = self._last_emit
        if isinstance(spans, tuple):                      # a replayed tick: every stream's chunk at the same place of its row
            row, at, count = spans
            spans = [(bb * row + at, count) for bb in range(len(sids))]
        return tensor, dict(zip(sids, spans))

    # the shared input rows under the names they had before _InputRows owned them (read by the host tests)
    _in_cap = property(lambda self: self._rows.cap)
    _in_mel = property(lambda self: self._rows.mel)
    _in_noise = property(lambda self: self._rows.noise)
    _in_f0 = property(lambda self: self._rows.f0)
    _in_scale = property(lambda self: self._rows.scale)

    def _grown(self, old, slots, *shape):
        """A zeroed device store of `slots` slots that starts with the contents of the old one."""
        import torch
        new = torch.zeros((slots,) + shape, dtype=torch.float32, device=self.engine.device)
        if old is not None:
            new[:old.shape[0]] = old
        return new

    def open(self, stream_id, f0="net"):
        """``f0``: "net" -- the stream's contour is the F0-net's; "frames" -- it is given from outside, one value in Hz per
        mel frame with every ``push`` (an F0 tracker's output)."""
        if f0 not in ("net", "frames"):
            raise ValueError('f0 must be "net" or "frames"')
        self._leave_steady()
        st = _Stream()
        st.f0_mode = f0
        if not self._free_slots:
            n_old = 0 if self._store is None else int(self._store.shape[0])
            n_new = max(16, 2 * n_old)
            rows = (self.sr_left + self.sr_right) * self.dims.steps_per_frame
            self._store = self._grown(self._store, n_new, rows, self.dims.subbands)
            if self.layer_carry:
                self._layer_store = self._grown(self._layer_store, n_new, self._layer_floats)
            if self.fe_carry:
                self._fe_store = self._grown(self._fe_store, n_new, self._fe_ring, self.engine.frontend_frame_floats)
            self._free_slots = list(range(n_new - 1, n_old - 1, -1))
            # (the stores moved: captured ticks point at the old ones -- open() has left the steady run above)
            self._rows.grow(n_new, self._rows.cap)
        st.slot = self._free_slots.pop()
        self.streams[stream_id] = st
        if f0 == "frames":
            self._control = True

    def close(self, stream_id):
        """Forget a finished stream (its slot of the sub-band store is reused)."""
        self._leave_steady()
        st = self.streams.pop(stream_id)
        self._free_slots.append(st.slot)

    def push(self, stream_id, mel_frames, noise=None, last=False, f0=None, transposition=None, formant=None):
        """Append mel frames (n, mel_channels) and the matching N(0,1) draw (n*steps_per_frame,) to a stream.

        ``f0``: (n,) Hz, one value per pushed frame -- required for a stream opened with ``f0="frames"``, refused for any
        other.  ``transposition``: factor on the stream's contour, a scalar or (n,) values (default 1).  Both are brought to
        the pulse rate by the model's linear interpolator, towards the next frame's value; they must be finite and
        positive.  ``formant``: formant-shift factor, a scalar or (n,) values, finite and positive (default 1): a frame's
        factor travels with the frame and warps that frame's envelope only, so the streamed audio
        equals the offline ``forward(formant=)`` of the whole utterance."""
        st = self.streams[stream_id]
        mel_frames = np.asarray(mel_frames, dtype=np.float32).reshape(-1, self.dims.mel_channels)
        n = mel_frames.shape[0]
        spf = self.dims.steps_per_frame
        if (f0 is not None) != (st.f0_mode == "frames"):
            raise ValueError('f0 goes with every push of a stream opened with f0="frames", and with no other stream')
        if f0 is not None:
            f0 = np.asarray(f0, dtype=np.float32).reshape(-1)
            if f0.shape[0] != n:
                raise ValueError("f0 must hold one value per pushed mel frame")
            if not (np.all(np.isfinite(f0)) and np.all(f0 > 0)):
                raise ValueError("f0 must be finite and positive")
        if transposition is not None:
            transposition = np.asarray(transposition, dtype=np.float32)
            if transposition.ndim > 0:
                transposition = transposition.reshape(-1)
                if transposition.shape[0] != n:
                    raise ValueError("transposition must be a scalar or hold one value per pushed mel frame")
            if not (np.all(np.isfinite(transposition)) and np.all(transposition > 0)):
                raise ValueError("transposition must be finite and positive")
        if formant is not None:
            formant = np.asarray(formant, dtype=np.float32)
            if formant.ndim > 0:
                formant = formant.reshape(-1)
                if formant.shape[0] != n:
                    raise ValueError("formant must be a scalar or hold one value per pushed mel frame")
            if not (np.all(np.isfinite(formant)) and np.all(formant > 0)):
                raise ValueError("formant must be finite and positive")
        if self.dims.noise_sigma:
            if noise is None:
                raise ValueError("noise is required (explicit input of the path)")
            noise = np.asarray(noise, dtype=np.float32).reshape(-1, spf)
            if noise.shape[0] != n:
                raise ValueError("noise must hold steps_per_frame values per pushed mel frame")
        rows = self._rows
        if st.have - st.base + n > rows.cap:
            # drop the frames no later window can reach (windows start at aligned(emitted - left); a stale `emitted` of a
            # stream inside a run of replayed ticks only keeps more than necessary), then grow the rows if that is not enough
            keep_from = max(st.base, ((st.emitted - self.left) // self.align) * self.align)
            if keep_from > st.base:
                rows.drop_front(st.slot, keep_from - st.base, st.have - keep_from)
                st.base = keep_from
            if st.have - st.base + n > rows.cap:
                rows.grow(rows.slots, max(2 * rows.cap, st.have - st.base + n))
        rows.append(st.slot, st.have - st.base, mel_frames, noise if self.dims.noise_sigma else None, f0, transposition,
                    formant)
        if not self._formant and formant is not None and np.any(formant != 1.0):
            self._leave_steady()                  # (as for the first pitch control below)
            self._formant = True
        if not self._control and transposition is not None and np.any(transposition != 1.0):
            # the first control this synthesizer sees: a steady run recorded without the control arguments is left and
            # captured anew
            self._leave_steady()
            self._control = True
        st.have += n
        st.closed = st.closed or last
        self._inputs_changed = True       # cached per-stream vectors of a run of replayed ticks are stale

    def _ready(self, st):
        have = st.have
        if st.emitted >= have:
            return 0
        chunk = self.schedule[st.ticks % len(self.schedule)]
        if st.closed:
            return min(chunk, have - st.emitted)
        return chunk if have >= st.emitted + chunk + self.right else 0

    # ------------------------------------------------------------------------------------------------------------------
    # a tick launch by launch: plan (stream_plan.plan_tick), upload, engine call, commit, record
    # ------------------------------------------------------------------------------------------------------------------
    def tick(self):
        """One batched engine call over every stream that can emit. Returns {stream_id: audio ndarray}."""
        import torch
        self.last_tick_replayed = False
        self._last_emit = None
        if self._steady is not None:
            status = self._steady_status()
            if status == "replay" and self.use_graph:
                return self._graph_tick()
            if status == "broken":
                self._leave_steady()
            else:                                     # a phase of the schedule that has no recorded tick yet
                self._sync_streams()
        todo = [(sid, st, self._ready(st)) for sid, st in self.streams.items()]
        todo = [(sid, st, nn) for sid, st, nn in todo if nn > 0]
        if not todo:
            return {}
        plan = plan_tick(self.geometry, [(st, nn) for _, st, nn in todo])
        up = self._upload(plan, [st for _, st, _ in todo])
        args, B = up.args, len(todo)
        self.last_tick_frames = int(plan.nfr.sum())
        self.last_tick_active_frames = int(plan.act.sum())
        self.last_tick_wavenet_frames = int(plan.act.sum()) if plan.wn is None else int(plan.wn.sum())
        self.last_tick_layer_rows = plan.layer_rows
        if plan.layer_rows:
            self.last_tick_wavenet_frames = B * plan.layer_rows // self.dims.steps_per_frame
        if self.time_device:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        pitch = {}
        if up.control:
            pitch = {"f0_item_mask": args.f0_item_mask, "f0_frames": args.f0_frames, "f0_scale": args.f0_scale}
        if up.formant:
            pitch["formant"] = args.formant
        audio, state_out = self.engine.forward(
            up.mel, n_frames=args.nfr, noise=up.noise, stream_state=args.states,
            active=(plan.a0, args.act, int(plan.act.max())),
            wavenet=(plan.wa, args.wn, int(plan.wn.max())) if plan.wn is not None else None,
            carry=(self._store, args.desc) if self.carry else None,
            layers=(self._layer_store, args.ldesc, plan.layer_rows) if self.layer_carry else None,
            frontend=(self._fe_store, args.fpos, 0, 0) if up.use_fe else None,    # whole window computed, every frame kept
            **pitch)
        if self.time_device:
            ev1.record()
            ev1.synchronize()
            self.last_tick_device_ms = ev0.elapsed_time(ev1)
        # only the emitted samples come back: the columns [lo, hi) of the window that hold some item's chunk
        hop = self.dims.hop_size
        lo = min(rel * hop for rel in plan.rel)
        hi = max((rel + nn) * hop for rel, nn in zip(plan.rel, plan.emit))
        # where this tick left its chunks on the device, for a stage behind the synthesizer (live.StreamingOutputResampler)
        self._last_emit = (audio, [sid for sid, _, _ in todo],
                           [(item * audio.stride(0) + plan.rel[item] * hop, nn * hop) for item, (_, _, nn) in enumerate(todo)])
        audio, state_out = audio[:, lo:hi].cpu().numpy(), state_out.cpu().numpy()
        result = self._commit(plan, todo, audio, lo, state_out)
        self._record_steady(plan, todo, up, lo, hi, state_out)
        return result

    def _upload(self, plan, streams):
        """The windows of a plan, gathered from the shared input rows, and every int32 argument of the call in one upload
        (with the control rows / the formant factors, floats bit-cast, once the synthesizer has seen pitch control / a formant
        shift)."""
        import torch
        B, spf, control, formant = len(streams), self.dims.steps_per_frame, self._control, self._formant
        tpad = max(plan.tmax, self._tcap)         # periodic schedules keep one window size for all phases (n_frames masks)
        mel = np.zeros((B, tpad, self.dims.mel_channels), dtype=np.float32)
        noise = np.zeros((B, tpad * spf), dtype=np.float32)
        # the control rows of the whole windows (the frames behind an item's end are not read)
        f0_rows = np.ones((B, tpad * control), dtype=np.float32)
        scale_rows = np.ones((B, tpad * control), dtype=np.float32)
        formant_rows = np.ones((B, tpad * formant), dtype=np.float32)
        for item, (st, (first, end)) in enumerate(zip(streams, plan.windows)):
            w_mel, w_noise, w_f0, w_scale, w_formant = self._rows.window(st.slot, first - st.base, end - st.base)
            mel[item, :end - first] = w_mel
            if self.dims.noise_sigma:
                noise[item, :(end - first) * spf] = w_noise.reshape(-1)
            if control:
                f0_rows[item, :end - first], scale_rows[item, :end - first] = w_f0, w_scale
            if formant:
                formant_rows[item, :end - first] = w_formant
        f0_mask = np.asarray([st.f0_mode == "frames" for st in streams], dtype=np.int32) if control else None
        parts = [("states", plan.states, "int32"), ("desc", plan.desc, "int32"), ("ldesc", plan.ldesc, "int32"),
                 ("nfr", plan.nfr, "int32"), ("act", plan.act, "int32"),
                 ("wn", plan.wn if plan.wn is not None else plan.act, "int32"), ("fpos", plan.fpos, "int32"),
                 ("f0_item_mask", f0_mask if control else np.zeros(0, np.int32), "int32"),
                 ("f0_frames", f0_rows, "float32"), ("f0_scale", scale_rows, "float32"), ("formant", formant_rows, "float32")]
        dev = self.engine.device
        flat = np.concatenate([arr.ravel().view(np.int32) for _, arr, _ in parts])
        args = _Layout([(name, arr.shape, dtype) for name, arr, dtype in parts]).views(torch.as_tensor(flat, device=dev))
        return _TickInputs(mel=torch.as_tensor(mel, device=dev),
                           noise=torch.as_tensor(noise, device=dev) if self.dims.noise_sigma else None, tpad=tpad, args=args,
                           use_fe=self.fe_carry and self.carry and tpad <= self._fe_ring, control=control, f0_mask=f0_mask,
                           formant=formant)

    def _commit(self, plan, todo, audio, lo, state_out):
        """Cut every stream's chunk out of the audio (whose column 0 is sample `lo` of the windows) and move the streams on
        to what the plan says they carry from this tick."""
        hop = self.dims.hop_size
        result = {}
        for item, (sid, st, nn) in enumerate(todo):
            at = plan.rel[item] * hop - lo
            result[sid] = audio[item, at:at + nn * hop].copy()
            st.emitted += nn
            st.ticks += 1
            st.carry_pos, st.carry_frames = plan.next_carry[item]
            st.layer_end = plan.next_layer_end[item]
            if plan.next_state_frame[item] < plan.windows[item][1]:
                sums = state_out[item, :2].copy().view(np.float32)
                st.state = (float(sums[0]), float(sums[1]), int(state_out[item, 2]))
                st.state_frame = plan.next_state_frame[item]
        return result

    def _record_steady(self, plan, todo, up, lo, hi, state_out):
        """After a committed tick: if it was a steady tick that a graph could stand for, record it as its phase of the
        steady run (starting a new run if the streams or the window size changed); any other tick ends the run."""
        n_ph, spf = len(self.schedule), self.dims.steps_per_frame
        streams = [st for _, st, _ in todo]
        # (mbx_window_advance keeps the part of a window that stays in LDS: at most 64 KB per item -- wide windows, e.g. the
        # RMS normalisation with several smoothing iterations or deep pre-conditioning chains, run launch by launch)
        window_fits = up.tpad * max(self.dims.mel_channels, spf) * 4 <= 64 * 1024
        phases = {(st.ticks - 1) % n_ph for st in streams}
        if not (plan.layer_rows and self.use_graph and self.periodic and window_fits and len(phases) == 1 and
                len(set(plan.emit)) == 1 and len(set(zip(plan.rel, plan.nfr.tolist()))) == 1):
            self._steady = None                   # not a steady tick: whatever run was being recorded is over
            return
        # a steady tick: when this phase of the schedule comes round again with every stream continuing the same way,
        # it is this launch sequence on windows that moved on by one period -- every window-relative argument is the
        # same (_steady_status checks it)
        new = _Phase(
            phase=phases.pop(), chunk=plan.emit[0], T=int(plan.nfr[0]), tpad=up.tpad, a0=plan.a0, wa=plan.wa, lo=lo, hi=hi,
            layer_rows=plan.layer_rows, act=plan.act.copy(), wn=plan.wn.copy(), nfr=plan.nfr.copy(), desc=plan.desc.copy(),
            ldesc=plan.ldesc.copy(), state_consts=plan.states[:, 3:5].copy(), rel0=plan.rel[0], use_fe=up.use_fe,
            frames=self.last_tick_frames, active_frames=self.last_tick_active_frames,
            wavenet_frames=self.last_tick_wavenet_frames, control=up.control, f0_mask=up.f0_mask, formant=up.formant)
        sids = [sid for sid, _, _ in todo]
        run = self._steady
        if run is None or run.sids != sids or run.tpad != up.tpad:
            run = self._steady = _SteadyRun(sids=sids, streams=streams, B=len(todo), tpad=up.tpad,
                                            slots=np.asarray([st.slot for st in streams], dtype=np.int64))
        old = run.phases.get(new.phase)
        if old is not None and not old.same_geometry(new):
            run.graphs.pop(new.phase, None)               # the geometry of this phase changed: capture it anew
        run.phases[new.phase] = new
        # where the run stands: the windows this tick worked on (device tensors), the streams' progress and phase states
        run.win_src = (up.mel, up.noise)
        run.state_v = state_out.copy()
        run.emitted_v = np.asarray([st.emitted for st in streams], dtype=np.int64)
        run.next_phase = streams[0].ticks % n_ph
        run.pending, run.pending_frames = 0, 0
        run.need_v = None

    # ------------------------------------------------------------------------------------------------------------------
    # steady ticks as replayed hipGraphs (one per phase of the tick schedule)
    # ------------------------------------------------------------------------------------------------------------------
    def _sync_streams(self):
        """Write the progress of the replayed ticks back to the stream objects (inside a run of replayed ticks it is kept
        in vectors: emitted frames, carried phase states)."""
        run = self._steady
        if run is None or not run.pending:
            return
        adv = run.pending_frames
        sf = run.state_v[:, :2].copy().view(np.float32)
        for bb, st in enumerate(run.streams):
            st.ticks += run.pending
            st.emitted += adv
            st.carry_pos = st.emitted
            st.layer_end += adv
            st.state_frame += adv
            st.state = (float(sf[bb, 0]), float(sf[bb, 1]), int(run.state_v[bb, 2]))
        run.pending, run.pending_frames = 0, 0

    def _leave_steady(self):
        self._sync_streams()
        self._steady = None

    def _steady_status(self):
        """What the tick about to run is for the steady run in self._steady: "replay" -- its phase of the schedule has been
        recorded and this tick is that recorded tick moved on (the same streams and no other one ready, each with a whole
        chunk and its look-ahead available and no utterance end inside the window, the same position of the window
        relative to the emitted frames: then every window-relative argument of the engine call is unchanged); "record" --
        the streams continue but this phase has no recorded tick yet (it runs launch by launch and is recorded);
        "broken" -- anything else."""
        run = self._steady
        streams, B = run.streams, run.B
        if self._inputs_changed or run.need_v is None:
            # frames received (+ whether the stream is closed: its last frame must then lie behind the window) and the
            # column of absolute frame 0 in the shared input rows; only push() changes them
            run.need_v = np.fromiter((st.have - st.closed for st in streams), np.int64, B)
            run.base_v = np.fromiter((st.base for st in streams), np.int64, B)
            self._inputs_changed = False
        phase = run.next_phase
        chunk = self.schedule[phase]
        emitted = run.emitted_v
        if int((run.need_v - emitted).min()) < chunk + self.right:
            return "broken"
        if len(self.streams) != B:                        # a stream outside the recorded set must not be ready
            inside = set(run.sids)
            if any(self._ready(st) > 0 for sid, st in self.streams.items() if sid not in inside):
                return "broken"
        rec = run.phases.get(phase)
        if rec is None or (phase - 1) % len(self.schedule) not in run.phases:
            return "record"                               # (a phase's graph shifts the window of the phase before it)
        ws = np.maximum(0, ((emitted - self.left) // self.align) * self.align)
        if np.any(emitted - ws != rec.rel0) or rec.chunk != chunk:
            return "broken"
        return "replay"

    def _capture(self, run, phase):
        """Fixed buffers + the captured launch sequence of the steady tick of one phase of the schedule.  All phases of a
        run work on ONE pair of device-resident windows (run.win: mel (B, tpad, channels), noise (B, tpad * spf)); a
        tick moves them on -- shift by the frames the aligned window start advanced since the tick before, append the
        tick's new frames -- and runs the forward pass with the phase's constant arguments."""
        import torch
        rec = run.phases[phase]
        n_ph = len(self.schedule)
        prev = run.phases[(phase - 1) % n_ph]
        eng, dims, dev = self.engine, self.dims, self.engine.device
        B, tpad, chunk, spf, hop = run.B, run.tpad, rec.chunk, dims.steps_per_frame, dims.hop_size
        # the window of the tick before held T_prev frames from ws_prev on; this one T frames from ws on: the start moved
        # by `shift` = (emitted - rel0) - (emitted_prev - rel0_prev) frames, `chunk` frames are new at the end
        shift = prev.chunk - (rec.rel0 - prev.rel0)
        keep = prev.T - shift
        if shift < 0 or keep < 0 or keep + chunk != rec.T or rec.T > tpad:
            raise RuntimeError(f"steady ticks of phases {(phase - 1) % n_ph} and {phase} do not chain: shift {shift}, "
                               f"windows {prev.T} -> {rec.T} frames, chunk {chunk}")
        use_noise = bool(dims.noise_sigma)
        if run.win is None:
            mel_win = torch.zeros((B, tpad, dims.mel_channels), dtype=torch.float32, device=dev)
            noise_win = torch.zeros((B, tpad * spf), dtype=torch.float32, device=dev) if use_noise else None
            run.win = (mel_win, noise_win)
            run.audio_buf = torch.empty((B, tpad * hop), dtype=torch.float32, device=dev)
            run.state_out = torch.empty((B, 6), dtype=torch.int32, device=dev)
            run.state_host = torch.empty((B, 6), dtype=torch.int32).pin_memory()
        mel_win, noise_win = run.win
        # one pinned host buffer / one device buffer for everything a tick uploads: new mel frames, new noise, phase states,
        # ring positions and -- once the synthesizer has seen pitch control -- the control rows of the whole windows
        # (B, tpad) each: small next to the mel frames, and the window they belong to is known to the host anyway, so they
        # need no device-resident window and no second move launch
        layout = _stage_layout(B, chunk, tpad, dims.mel_channels, spf, use_noise, rec.control, rec.formant)
        stage_host = torch.ones(layout.size, dtype=torch.float32).pin_memory()
        stage_dev = torch.empty_like(stage_host, device=dev)
        new = layout.views(stage_dev)
        pitch = {}
        if rec.control:
            pitch = {"f0_frames": new.f0_frames, "f0_scale": new.f0_scale,
                     "f0_item_mask": torch.as_tensor(rec.f0_mask, device=dev)}
        if rec.formant:
            pitch["formant"] = new.formant
        # front end: the window gained `chunk` frames and the last fe_right frames of the window before were inexact: the
        # sub-nets run on the last chunk + fe_right (+ their reach) frames in front of the window's end (frame rec.T of the
        # buffer: fe_end_frames), everything in front of that comes from the ring
        fe_new, fe_margin = chunk + self.fe_right, self.fe_left
        use_fe = rec.use_fe and fe_new + fe_margin <= rec.T
        ints = {kk: torch.as_tensor(getattr(rec, kk), device=dev) for kk in ("act", "wn", "nfr", "desc", "ldesc")}
        audio_buf, state_out, state_host = run.audio_buf, run.state_out, run.state_host
        audio_host = torch.empty((B, rec.hi - rec.lo), dtype=torch.float32).pin_memory()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize(dev)
        # thread_local: another thread of the process (the RCCL watchdog of a multi-rank job) may touch the runtime while
        # this one captures
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            stage_dev.copy_(stage_host, non_blocking=True)
            # shift the kept frames to the front and append the tick's new ones: one launch whatever the schedule
            eng.window_update(mel_win, new.mel, noise_win, new.noise, shift, keep)
            eng.forward(mel_win, n_frames=ints["nfr"], noise=noise_win, stream_state=new.states,
                        active=(rec.a0, ints["act"], int(rec.act.max())),
                        wavenet=(rec.wa, ints["wn"], int(rec.wn.max())),
                        carry=(self._store, ints["desc"].view(B, 5)) if self.carry else None,
                        layers=(self._layer_store, ints["ldesc"].view(B, 3), rec.layer_rows),
                        frontend=(self._fe_store, new.fpos, fe_new if use_fe else 0, fe_margin if use_fe else 0, rec.T)
                        if rec.use_fe else None,
                        out=audio_buf, state_out=state_out, **pitch)
            # the emitted samples of every stream: one strided device-to-host copy (no device-side gather in between)
            eng.emit_rows(audio_buf, rec.lo, rec.hi - rec.lo, audio_host)
            state_host.copy_(state_out, non_blocking=True)
        return _CapturedTick(graph=graph, stage_host=stage_host, host=layout.views(stage_host.numpy()),
                             arange=np.arange(chunk, dtype=np.int64), arange_win=np.arange(rec.T, dtype=np.int64),
                             audio_host=audio_host, state_host=state_host, shift=shift, keep=keep,
                             # (the engine's scratch of the warped rows, sized by this phase's recorded tick: a later,
                             # larger forward gives the engine a new one, the graph keeps writing this one)
                             keep_alive=(stage_dev, ints, pitch, getattr(eng, "_env_mel", None) if rec.formant else None))

    def _graph_tick(self):
        """A steady tick as one graph launch: gather and upload the new frames and the phase states, replay, read the
        chunk back.  Nothing here loops over the streams."""
        import torch
        run = self._steady
        phase = run.next_phase
        rec = run.phases[phase]
        n_ph = len(self.schedule)
        cap = run.graphs.get(phase)
        if cap is None:
            try:
                if (phase - 1) % n_ph not in run.phases:
                    raise RuntimeError("the phase in front of this one has no recorded tick")
                cap = run.graphs[phase] = self._capture(run, phase)
            except Exception as exc:                          # noqa: BLE001 -- whatever made the capture fail
                # the streams must not get stuck retrying a capture that cannot succeed: from here on every tick runs
                # launch by launch (bit-identical results, more host time)
                import sys
                print(f"mbexwn_vocoder_amd.streaming: hipGraph capture of the steady tick failed ({type(exc).__name__}: "
                      f"{exc}); ticks run launch by launch from here on", file=sys.stderr)
                self.use_graph = False
                self._leave_steady()
                return self.tick()
        chunk, hop = rec.chunk, self.dims.hop_size
        # the device windows hold the window of the tick before: written there by a replayed tick, or still in the tensors a
        # launch-by-launch tick uploaded
        if run.win_src is not run.win:
            src_mel, src_noise = run.win_src
            run.win[0].copy_(src_mel)
            if run.win[1] is not None:
                run.win[1].copy_(src_noise)
            run.win_src = run.win
        host, emitted, slots, base = cap.host, run.emitted_v, run.slots, run.base_v
        # the frames the windows gain: [emitted + right, emitted + right + chunk) of every stream
        cols = (emitted + self.right - base)[:, None] + cap.arange
        self._rows.gather(slots, cols, mel=host.mel)
        if host.noise is not None:
            self._rows.gather(slots, cols, noise=host.noise.reshape(run.B, chunk, -1))
        host.fpos[:] = (emitted - rec.rel0) % self._fe_ring                   # ring frame of each window's first frame
        if host.f0_frames is not None:
            # the control rows of the whole windows [emitted - rel0, + T): one gather per row
            wcols = (emitted - rec.rel0 - base)[:, None] + cap.arange_win
            self._rows.gather(slots, wcols, f0=host.f0_frames[:, :rec.T], scale=host.f0_scale[:, :rec.T])
        if host.formant is not None:
            wcols = (emitted - rec.rel0 - base)[:, None] + cap.arange_win
            self._rows.gather(slots, wcols, formant=host.formant[:, :rec.T])
        host.states[:, :3] = run.state_v[:, :3]
        host.states[:, 3:5] = rec.state_consts
        host.states[:, 5] = 0
        if self.time_device:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        cap.graph.replay()
        if self.time_device:
            ev1.record()
        torch.cuda.current_stream(self.engine.device).synchronize()
        if self.time_device:
            self.last_tick_device_ms = ev0.elapsed_time(ev1)
        audio = cap.audio_host.numpy().copy()
        run.state_v = cap.state_host.numpy().copy()
        at = rec.rel0 * hop - rec.lo
        result = dict(zip(run.sids, audio[:, at:at + chunk * hop]))
        self._last_emit = (run.audio_buf, run.sids, (run.audio_buf.stride(0), rec.rel0 * hop, chunk * hop))
        emitted += chunk
        run.pending += 1
        run.pending_frames += chunk
        run.next_phase = (phase + 1) % n_ph
        self.last_tick_frames, self.last_tick_active_frames = rec.frames, rec.active_frames
        self.last_tick_wavenet_frames, self.last_tick_layer_rows = rec.wavenet_frames, rec.layer_rows
        self.last_tick_replayed = True
        self.graph_ticks += 1
        return result

    def finished(self, stream_id):
        self._sync_streams()
        st = self.streams[stream_id]
        return st.closed and st.emitted >= st.have

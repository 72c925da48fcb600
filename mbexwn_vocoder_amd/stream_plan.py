"""The geometry of one streaming tick as a pure function: which window, active region, WaveNet region, carried sub-band
rows, per-layer state and phase-state positions every stream of the tick gets (``plan_tick``).  Host-only integer
arithmetic on numpy arrays -- no torch, no engine -- so it runs and is tested without a device;
streaming.StreamingSynthesizer uploads what a plan holds, calls the engine and applies the plan's successor values."""
from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class StreamGeometry:
    """The constants of a model and a synthesizer that the arithmetic of a tick needs, in mel frames unless named
    otherwise (streaming.stream_margins and StreamingSynthesizer.__init__ derive them)."""
    left: int                 # window margins around the emitted frames
    right: int
    lead: int                 # first window frame with reproducible pulses / conditioning rows
    act_left: int             # margins of the stages from the WaveNet on
    act_right: int
    wn_left: int              # the WaveNet's reach in front of a region and behind it
    wn_reach: int
    sr_left: int              # carried sub-band rows around the emit position
    sr_right: int
    align: int                # window and region starts are multiples of it (Winograd pairing as offline)
    steps_per_frame: int
    pulse_per_frame: int
    hop_size: int
    carry: bool               # sub-band rows are carried from tick to tick
    layer_carry: bool         # per-layer WaveNet state is carried
    layer_min_rows: int       # smallest number of new rows of a steady tick
    fe_ring: int              # frames of a stream's front-end ring


@dataclass
class TickPlan:
    """What one tick runs on, item by item (B items), and what every stream carries on from it."""
    emit: list                # frames every item emits
    rel: list                 # frame of the window at which an item's emitted frames start
    windows: list             # (first, end) absolute frame of every item's window
    tmax: int                 # frames of the longest window
    a0: int                   # active region: first window frame (the same for every item) ...
    act: np.ndarray           # ... and its frames per item (B,)
    wa: object                # WaveNet region inside the active one: first window frame, or None (= the active region)
    wn: object                # ... and its frames per item (B,), or None
    desc: np.ndarray          # (B, 5) sub-band carry: slot, rows to read (at, count), rows to store (at, count)
    ldesc: np.ndarray         # (B, 3) layer state: slot, row the stored state ends at or -1, row to store a state at or -1
    layer_rows: int           # > 0: steady tick, every WaveNet layer runs on that many new rows only
    nfr: np.ndarray           # (B,) frames of every window
    states: np.ndarray        # (B, 6) one mbx_stream_state per item (streaming.pack_state)
    fpos: np.ndarray          # (B,) ring frame of every window's first frame
    next_carry: list          # per item (carry_pos, carry_frames) after the tick
    next_layer_end: list      # per item layer_end after the tick
    next_state_frame: list    # per item state_frame, if the tick captures a phase state there (it lies inside the window)


def _aligned(frame, align):
    return (frame // align) * align


def _windows(geo, items):
    windows = []
    for st, emit in items:
        first = max(0, _aligned(st.emitted - geo.left, geo.align))
        end = st.have if st.closed and st.emitted + emit + geo.right >= st.have else st.emitted + emit + geo.right
        windows.append((first, min(end, st.have)))
    return windows


def _active_region(geo, items, windows):
    """-> (first window frame of the region, absolute end frame of every item's region)."""
    # active region: the mel-rate stages and the phase need the whole window (their receptive fields are long: F0-net,
    # smoother of the lifter selection), the stages from the WaveNet on only the frames around what is emitted.
    # It starts on an aligned frame (same Winograd pairing as offline), at least `lead` frames inside a window that
    # does not start the utterance (pulses are reproducible from there), and is the same offset for every item.
    begin = None
    for (st, emit), (first, end) in zip(items, windows):
        item_begin = max(0, _aligned(st.emitted - geo.act_left, geo.align)) - first
        if first > 0 and item_begin < geo.lead:
            item_begin = 0
        begin = item_begin if begin is None else min(begin, item_begin)
    if any(first > 0 for first, _ in windows) and 0 < begin < geo.lead:
        begin = 0
    ends = [end if end - (st.emitted + emit) <= geo.act_right else st.emitted + emit + geo.act_right
            for (st, emit), (first, end) in zip(items, windows)]
    return begin, ends


def _carried_subbands(geo, items, windows):
    """-> (window frame of the first carried sub-band row, window frame the WaveNet region starts at), or None."""
    # carried sub-bands: usable when every item of the tick has a valid store and the same geometry
    if not geo.carry:
        return None
    common = None
    for (st, emit), (first, end) in zip(items, windows):
        sub_begin = st.emitted - geo.sr_left - first
        wn_begin = _aligned(st.emitted + min(geo.sr_right, st.carry_frames - geo.sr_left) - geo.wn_left, geo.align) - first
        usable = (st.carry_pos == st.emitted and st.emitted - geo.sr_left >= first and wn_begin >= sub_begin and
                  (first == 0 or wn_begin >= geo.lead) and st.carry_frames > geo.sr_left)
        if not usable or (common is not None and common != (sub_begin, wn_begin)):
            return None
        common = (sub_begin, wn_begin)
    return common


def _rows_to_carry(geo, items, windows, ends, region_begin, carried, desc):
    """Fills desc[:, 0] and desc[:, 3:5]; -> per item (carry_pos, carry_frames) after the tick."""
    # rows the next tick will need: frames [e' - sr_left, e' + sr_right) around the next emit position e', if this tick
    # computes them exactly (its region reaches wn_reach frames beyond them, or to the end of the utterance)
    spf = geo.steps_per_frame
    next_carry = []
    for item, ((st, emit), (first, end)) in enumerate(zip(items, windows)):
        emit_end = st.emitted + emit
        lo = emit_end - geo.sr_left
        hi = min(emit_end + geo.sr_right, ends[item] if ends[item] == end and st.closed else ends[item] - geo.wn_reach)
        exact_from = first + region_begin
        if not carried and exact_from > 0:
            exact_from += geo.wn_left
        good = geo.carry and lo >= exact_from and hi > lo + geo.sr_left and lo >= first
        desc[item, 0] = st.slot
        if good:
            desc[item, 3:5] = (lo - first) * spf, (hi - lo) * spf
        next_carry.append((emit_end, hi - lo) if good else (None, 0))
    return next_carry


def _layer_state(geo, items, windows, ends, region_begin, sub_begin, ldesc):
    """Fills ldesc; -> (steady, new rows and region end inside the window of a steady tick, per item layer_end after
    the tick).  ``region_begin``: window frame the WaveNet region starts at; ``sub_begin``: of the first carried
    sub-band row, or None without usable carried sub-bands."""
    # per-layer WaveNet state.  Steady tick: every item has the state of a region that ended layer_rows rows in front
    # of this tick's region end, the sub-bands up to the WaveNet's reach in front of that, the same geometry inside
    # its window, and does not end its utterance here.  Any other tick runs the whole region and stores the state.
    spf = geo.steps_per_frame
    steady = sub_begin is not None
    common = None
    finals = []
    for item, ((st, emit), (first, end)) in enumerate(zip(items, windows)):
        final = st.closed and ends[item] >= end
        finals.append(final)
        ldesc[item, 0] = st.slot
        if st.layer_end is None or final or st.layer_end >= ends[item]:
            steady = False
        elif steady:
            new = ((ends[item] - st.layer_end) * spf, ends[item] - first)
            steady = (new[0] >= geo.layer_min_rows and (common is None or new == common) and
                      st.layer_end - geo.wn_reach >= first + sub_begin and
                      st.emitted - geo.sr_left + st.carry_frames == st.layer_end - geo.wn_reach)
            common = new
    next_layer_end = [None] * len(items)
    for item, ((st, emit), (first, end)) in enumerate(zip(items, windows)):
        # state of this tick's region: exact if the region starts the utterance or reaches 2 * reach + 1 frames back
        # in front of its last exact row (SAME: 3 * reach + 1 frames in all)
        long_enough = (first + region_begin == 0 or
                       ends[item] - first - region_begin >= 2 * geo.wn_left + geo.wn_reach + 1)
        if not finals[item] and (steady or long_enough):
            ldesc[item, 2] = (ends[item] - first) * spf
            next_layer_end[item] = ends[item]
    if steady:
        for item, ((st, emit), (first, end)) in enumerate(zip(items, windows)):
            ldesc[item, 1] = (st.layer_end - first) * spf
    return steady, common, next_layer_end


def _phase_state(geo, items, windows):
    """-> (states (B, 6), per item the frame the next state is captured at)."""
    ppf = geo.pulse_per_frame
    states = np.zeros((len(items), 6), dtype=np.int32)
    sums = np.zeros((len(items), 2), dtype=np.float32)
    next_state_frame = []
    for item, ((st, emit), (first, end)) in enumerate(zip(items, windows)):
        # the carried state sits at frame st.state_frame (>= first + lead, or 0 at the utterance start): pulses are
        # reproducible from there on.  The next state is captured where the NEXT window's reproducible region
        # starts: `lag` = left - lead frames in front of the next emit position.
        capture = max(st.state_frame, st.emitted + emit - (geo.left - geo.lead))
        sums[item] = st.state[0], st.state[1]
        states[item, 2:5] = st.state[2], (st.state_frame - first) * ppf, (capture - first) * ppf if capture < end else -1
        next_state_frame.append(capture)
    states[:, :2] = sums.view(np.int32)                       # one mbx_stream_state per item (pack_state)
    return states, next_state_frame


def plan_tick(geometry, items):
    """The plan of a tick over ``items``: (stream, frames to emit) of every stream that can emit.  A stream is any
    object with the fields slot, emitted, have, closed, carry_pos, carry_frames, layer_end, state, state_frame (f0_mode
    travels with it for the caller; the geometry does not depend on it).  Reads the streams, changes nothing."""
    geo, B, spf = geometry, len(items), geometry.steps_per_frame
    windows = _windows(geo, items)
    a0, ends = _active_region(geo, items, windows)
    wa = wn = None
    desc = np.zeros((B, 5), dtype=np.int32)
    carried = _carried_subbands(geo, items, windows)
    if carried is not None:
        # the active region starts with the carried rows, the WaveNet runs behind them
        a0, wa = carried
        wn = np.asarray([ends[item] - first - wa for item, (first, _) in enumerate(windows)], dtype=np.int32)
        desc[:, 1] = a0 * spf
        desc[:, 2] = [st.carry_frames * spf for st, _ in items]
    act = np.asarray([ends[item] - first - a0 for item, (first, _) in enumerate(windows)], dtype=np.int32)
    next_carry = _rows_to_carry(geo, items, windows, ends, a0, carried is not None, desc)
    ldesc = np.full((B, 3), -1, dtype=np.int32)
    layer_rows = 0
    next_layer_end = [None] * B
    if geo.layer_carry:
        steady, new, next_layer_end = _layer_state(geo, items, windows, ends, a0 if carried is None else wa,
                                                   None if carried is None else a0, ldesc)
        if steady:
            layer_rows = new[0]
            wa = new[1] - layer_rows // spf - geo.wn_reach            # frame of the first new sub-band row
            wn = np.asarray([ends[item] - first - wa for item, (first, _) in enumerate(windows)], dtype=np.int32)
    states, next_state_frame = _phase_state(geo, items, windows)
    return TickPlan(
        emit=[emit for _, emit in items], rel=[st.emitted - first for (st, _), (first, _) in zip(items, windows)],
        windows=windows, tmax=max(end - first for first, end in windows), a0=a0, act=act, wa=wa, wn=wn, desc=desc,
        ldesc=ldesc, layer_rows=layer_rows, nfr=np.asarray([end - first for first, end in windows], dtype=np.int32),
        states=states, fpos=np.asarray([first % geo.fe_ring for first, _ in windows], dtype=np.int32),
        next_carry=next_carry, next_layer_end=next_layer_end, next_state_frame=next_state_frame)

"""Batched synthesis behind the drop-in surface: ``MELInverter.synth_from_mels`` and ``resynth_mel.py --batch N --gpus N``.

The reference's CLI synthesises one file at a time (reference bin/resynth_mel.py:74-104).  Here the files of a job go
through padded micro-batches of whole utterances (``sharding.plan_batches``; every boundary op of the engine honours the
item's own length), the FLAC frames are encoded on the device (``MBExWNEngine.encode_flac16``) and copied into pinned host
memory while the next micro-batch runs, and host thread pools read the ``.mell`` files and write the results.  A
``--gpus N`` job partitions the files by frames (``sharding.lpt_partition``) over N fresh child processes, each of which
writes its own files: no gather, no process group.

Noise: after ``torch.manual_seed(seed)`` the one-at-a-time loop draws ``torch.randn((1, T_i * wn_in_rows_per_frame))`` on
the device once per file, in file order (``engine._prepare``), and nothing else takes numbers from the device generator in
between (``MELInverter.calibrate`` draws from numpy).  :func:`replay_noise` makes the same draws in the same order and keeps
those of the files a process owns.  With ``batch_invariant`` on both sides (include/mbexwn.h) batched files are then
bit-identical to one-at-a-time files.
"""
import json
import os
import subprocess
import sys
import tempfile
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .fileio import load_var
from .sharding import lpt_partition, plan_batches, visible_gpu_count


def output_path(mell_file, output_dir, fmt):
    """syn_<basename>.<format> in ``output_dir`` (reference bin/resynth_mel.py)."""
    return os.path.join(output_dir or "", "syn_" + os.path.splitext(os.path.basename(mell_file))[0] + "." + fmt)


def have_soundfile():
    try:
        import soundfile  # noqa: F401
    except ImportError:
        return False
    return True


def write_audio(outfile, data, rate, format, flac_compression="verbatim"):
    """reference bin/resynth_mel.py:104-105 (sndio.write): libsndfile through soundfile where it is installed, else the
    built-in writers -- flac (mbexwn_vocoder_amd/flac.py: 16-bit; uncompressed sub-frames, or with
    ``flac_compression="fixed"`` fixed predictors and Rice codes) and wav (float32).  soundfile compresses FLAC by itself
    and ignores ``flac_compression``."""
    try:
        import soundfile
        soundfile.write(outfile, data, rate, format=format.upper())
        return outfile
    except ImportError:
        pass
    if format.lower() == "flac":
        from . import flac
        return flac.write(outfile, data, rate, flac_compression)
    if format.lower() == "wav":
        from scipy.io import wavfile
        wavfile.write(outfile, rate, np.asarray(data, dtype=np.float32))
        return outfile
    raise RuntimeError(f"cannot write format {format}: soundfile is not installed, only flac and wav are built in")


def replay_noise(frames, rows_per_frame, keep=None, device=None, generator=None):
    """The N(0,1) draws of the one-at-a-time loop over files of ``frames`` frames (after scale_mel), in file order: returns
    {i: (frames[i] * rows_per_frame,) tensor} for the files in ``keep`` (default: all); the others are drawn and dropped."""
    import torch
    keep = set(range(len(frames))) if keep is None else set(keep)
    draws = {}
    for ii, tt in enumerate(frames):
        zz = torch.randn((1, int(tt) * rows_per_frame), device=device, dtype=torch.float32, generator=generator)
        if ii in keep:
            draws[ii] = zz[0]
    return draws


def stage_micro_batch(mels, noises, rows_per_frame, device=None):
    """Padded inputs of one micro-batch: ``mels`` (list of (T_j, C) float32 arrays), ``noises`` (list of (T_j *
    rows_per_frame,) tensors, or None) -> mel (B, Tmax, C), n_frames int32 (B,), noise (B, Tmax * rows_per_frame) or None,
    on ``device``; item j's draw at the front of row j, zeros behind it."""
    import torch
    lengths = [int(mm.shape[0]) for mm in mels]
    tmax = max(lengths)
    mel = np.zeros((len(mels), tmax, mels[0].shape[1]), dtype=np.float32)
    for jj, mm in enumerate(mels):
        mel[jj, :lengths[jj]] = mm
    noise = None
    if noises is not None:
        noise = torch.zeros((len(mels), tmax * rows_per_frame), dtype=torch.float32, device=device)
        for jj, zz in enumerate(noises):
            noise[jj, :lengths[jj] * rows_per_frame] = zz
    return (torch.as_tensor(mel, device=device), torch.as_tensor(np.asarray(lengths, dtype=np.int32), device=device),
            noise)


class SynthBatch:
    """One micro-batch in flight: ``indices`` into the caller's list, the samples of every item, the device audio (B, stride)
    and what was enqueued behind the forward -- the FLAC frames (``engine.EncodedFlac``) and / or the audio in pinned host
    memory.  :meth:`wait` before reading; ``device_ms`` / ``copy_ms`` are then the forward's and the encode + copies' time."""

    def __init__(self, indices, n_samples, audio, flac, host_audio, events, model_audio=None, level=None):
        self.indices, self.n_samples, self.device_audio = list(indices), list(n_samples), audio
        self.flac, self.host_audio, self._events = flac, host_audio, events
        # with a level stage: (LevelControl, the items' target powers, host records, host gains) -- see level()
        self._level = level
        # with an output rate: (device audio at the model rate, its lengths) -- everything above is at the output rate
        self._model_audio = model_audio
        self.device_ms = self.copy_ms = 0.0

    def wait(self):
        if self._events is not None:
            ev0, ev1, ev2 = self._events
            ev2.synchronize()
            self.device_ms, self.copy_ms = ev0.elapsed_time(ev1), ev1.elapsed_time(ev2)
            if self.flac is not None:
                self.flac.wait()
            self._events = None
        return self

    def audio(self, jj):
        """float32 audio of item jj (numpy)."""
        nn = self.n_samples[jj]
        if self.host_audio is not None:
            return self.host_audio[jj, :nn].numpy()
        return self.device_audio[jj, :nn].cpu().numpy()

    def model_audio(self, jj):
        """float32 audio of item jj at the model rate (numpy): ``audio(jj)`` unless the batch has an output rate."""
        if self._model_audio is None:
            return self.audio(jj)
        audio, n_samples = self._model_audio
        return audio[jj, :n_samples[jj]].cpu().numpy()

    def level(self, jj):
        """What the level stage did to item jj (after :meth:`wait`; None for a batch without the stage): a dict with
        ``loudness_in`` and ``loudness_out`` in LUFS (-inf: not measurable), ``gain`` (the float32 factor), ``gain_db``,
        ``peak_in`` and ``peak_out`` (linear; the true peak where the stage was asked for it) and ``limited`` -- the
        ceiling, not the target, set the gain.  With the limiter ``limited`` is False, the loudness and
        the peak that came out are those of a second measurement, and ``limiter`` holds ``reduction_db`` (the deepest gain
        reduction), ``limited`` and ``clamped`` (samples with a gain below 1, samples the clamp moved) and ``trim_db`` (the
        ceiling-only gain behind the limiter with ``true_peak``; 0 without)."""
        if self._level is None:
            return None
        from . import level as lv
        control, powers, records, gains = self._level[:4]
        self.wait()
        power, count, _, sample_peak, true_peak = lv.DeviceMeasure.unpack(records.numpy(), jj)
        peak = true_peak if control.true_peak else sample_peak
        gain = float(gains.numpy()[jj])
        loud = lv.lufs(power) if count else float("-inf")
        with np.errstate(divide="ignore"):
            gain_db = float(20.0 * np.log10(np.float64(gain)))
        if not control.limiter:
            _, limited = lv.gain_host(power, count, peak, powers[jj], lv.ceiling_linear(control.peak_limit))
            return {"loudness_in": loud, "loudness_out": loud + gain_db, "gain": gain, "gain_db": gain_db, "peak_in": float(peak),
                    "peak_out": float(np.float32(peak) * np.float32(gain)), "limited": bool(limited)}
        # the limiter: the loudness and the peak that came out are measured, not derived
        from .limiter import LimitStats
        stats = LimitStats.from_words(self._level[4].numpy()[jj])
        power_out, count_out, _, sample_out, true_out = lv.DeviceMeasure.unpack(self._level[5].numpy(), jj)
        trim = float(self._level[6].numpy()[jj]) if len(self._level) > 6 else 1.0
        with np.errstate(divide="ignore"):
            trim_db = float(20.0 * np.log10(np.float64(trim)))
        return {"loudness_in": loud, "loudness_out": (lv.lufs(power_out) if count_out else float("-inf")) + trim_db, "gain": gain,
                "gain_db": gain_db, "peak_in": float(peak),
                "peak_out": float(np.float32(true_out if control.true_peak else sample_out) * np.float32(trim)),
                "limited": False, "limiter": {"reduction_db": stats.reduction_db, "limited": stats.limited,
                                              "clamped": stats.clamped, "trim_db": trim_db}}

    def max_abs(self, jj):
        if self.flac is not None:
            return float(self.flac.max_abs[jj])
        return float(np.max(np.abs(self.audio(jj)))) if self.n_samples[jj] else 0.0


def stage_factors(rows, device=None):
    """Per-frame transposition factors of one micro-batch: ``rows`` (list of (T_j,) float32 arrays) -> (B, Tmax) float32 on
    ``device``, every row continued with its last factor (the padding frames belong to no item)."""
    import torch
    tmax = max(int(rr.shape[0]) for rr in rows)
    scale = np.ones((len(rows), tmax), dtype=np.float32)
    for jj, rr in enumerate(rows):
        if rr.shape[0]:
            scale[jj, :rr.shape[0]] = rr
            scale[jj, rr.shape[0]:] = rr[-1]
    return torch.as_tensor(scale, device=device)


def _control_rows(control, key, name, rows, group, lengths, device, drop_ones=False, mask_key=None):
    """``control[key]``: the rows of the micro-batch ``group`` out of the per-item ``rows`` (run_micro_batches' argument
    ``name``; None: ones), or nothing without the argument; a row of another length than its mel is refused by name.
    ``drop_ones``: nothing when every value is exactly 1.  ``mask_key``: with ``control[mask_key]``, int32 (B,), 0 for the
    items with None -- and nothing when all are."""
    import torch
    if rows is None or (mask_key and all(rows[ii] is None for ii in group)):
        return
    for ii in group:
        if rows[ii] is not None and np.shape(rows[ii]) != (lengths[ii],):
            raise ValueError(f"{name}[{ii}] must hold one factor per mel frame ({lengths[ii]})")
    staged = [np.ones(lengths[ii], dtype=np.float32) if rows[ii] is None else np.asarray(rows[ii], dtype=np.float32)
              for ii in group]
    if drop_ones and not any(np.any(rr != 1.0) for rr in staged):
        return
    control[key] = stage_factors(staged, device)
    if mask_key:
        control[mask_key] = torch.as_tensor(np.asarray([rows[ii] is not None for ii in group], dtype=np.int32), device=device)


def check_f0s(f0s, lengths):
    """The per-item F0 contours of a job, checked before anything runs: None, or a list with, per item, None or a float32
    array (T_i,) of positive finite Hz.  A list of Nones counts as None."""
    if f0s is None:
        return None
    f0s = list(f0s)
    if len(f0s) != len(lengths):
        raise ValueError(f"f0s must hold one entry per item ({len(lengths)}), got {len(f0s)}")
    out = []
    for ii, (ff, tt) in enumerate(zip(f0s, lengths)):
        if ff is not None:
            ff = np.ascontiguousarray(ff, dtype=np.float32)
            if ff.shape != (tt,):
                raise ValueError(f"f0s[{ii}] must hold one value per mel frame ({tt}), got shape {ff.shape}")
            if not (np.all(np.isfinite(ff)) and np.all(ff > 0)):
                raise ValueError(f"f0s[{ii}] must be finite and positive (f0track.fill_unvoiced fills the unvoiced frames)")
        out.append(ff)
    return None if all(ff is None for ff in out) else out


def run_micro_batches(engine, mels, noises=None, max_batch=16, max_padded_frames=16 * 1200, flac=False, host_audio=True,
                      flac_compression="verbatim", out_rate=None, transpositions=None, formants=None, f0s=None, level=None):
    """Generator over the padded micro-batches of ``mels`` (list of (T_i, C) float32 arrays) on ``engine``: each is staged
    and run (engine.forward with the items' lengths), its FLAC frames encoded (``flac``) and / or its audio copied to pinned
    host memory (``host_audio``), all enqueued on the current stream; the SynthBatch is yielded without waiting, so that a
    writer can take it while the next one runs.  ``flac_compression``: "verbatim" or "fixed" (engine.encode_flac16; the
    compressed encoder waits for its frame lengths before the batch is yielded).  ``noises``: per-item device tensors (T_i * wn_in_rows_per_frame,), or
    None for a model without noise channel.  ``out_rate`` (None or the model's rate: nothing changes): the micro-batch is
    resampled on the device behind the forward (``resample.resample_device`` with the items' own lengths), and the FLAC
    frames, the host audio and ``n_samples`` of the SynthBatch are at that rate; ``SynthBatch.model_audio`` keeps the
    model-rate audio.

    ``noises`` may also be a ``mel_inverter.KeyedNoise`` (a seed and one key per item): each micro-batch's draw is then filled
    on the device by ``engine.keyed_noise``, a function of the seed, the item's key and the step alone.  ``transpositions``:
    per item None or (T_i,) factors, one per mel frame -- the ``f0_scale`` rows of the forward; None: the forward of today.
    ``formants``: the same for the formant shift (the ``formant`` rows of the forward).  A micro-batch
    whose factors are all exactly 1 runs the forward without them: a factor of 1 copies the row, so the bits are the same.
    ``f0s``: per item None or (T_i,) Hz, one value per mel frame, positive and finite (an F0 tracker's output through
    ``f0track.fill_unvoiced``): the ``f0_frames`` rows of the forward, with ``f0_item_mask`` 0 for the None items, which keep
    the F0-net; every entry is checked before anything runs, and a job whose entries are all None runs the forward
    without them.

    ``level``: None, or a ``level.LevelControl``: behind the forward and the output resampler, and in
    front of the FLAC encoder and the host copy, every item is measured at the rate it is written at (``level.measure_device``),
    takes one gain from its target and the ceiling (``level.gains_device``) and is multiplied by it (``level.apply_device``)
    -- all on the device, nothing waited for.  The FLAC frames, ``pcm``, MD5, ``max_abs`` and the host audio are those of the
    gained audio; ``SynthBatch.model_audio`` keeps the ungained model-rate audio and ``SynthBatch.level`` reports.  A
    per-item target list is indexed like ``mels``.  None: the launches of before.  With ``level.limiter`` (DESIGN.md section
    6n) the gain comes without the ceiling, the look-ahead limiter (``limiter.limit_device``) keeps the ceiling, the result
    is measured again, and with ``true_peak`` a ceiling-only gain follows; without it, the launches of before."""
    f0s = check_f0s(f0s, [int(mm.shape[0]) for mm in mels])
    import torch
    from .mel_inverter import KeyedNoise
    dims = engine.dims
    if out_rate is not None and int(round(out_rate)) == int(round(dims.sample_rate)):
        out_rate = None
    if level is not None:
        level.check_rates([dims.sample_rate if out_rate is None else out_rate])     # the limiter's window: before anything runs
    lengths = [int(mm.shape[0]) for mm in mels]
    stream = torch.cuda.current_stream(engine.device)
    for group in plan_batches(range(len(mels)), lengths, max_batch, max_padded_frames):
        keyed = isinstance(noises, KeyedNoise)
        mel, n_frames, noise = stage_micro_batch([mels[ii] for ii in group],
                                                 None if noises is None or keyed else [noises[ii] for ii in group],
                                                 dims.wn_in_rows_per_frame, engine.device)
        control = {}
        _control_rows(control, "f0_scale", "transpositions", transpositions, group, lengths, engine.device)
        _control_rows(control, "formant", "formants", formants, group, lengths, engine.device, drop_ones=True)
        _control_rows(control, "f0_frames", "f0s", f0s, group, lengths, engine.device, mask_key="f0_item_mask")
        events = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        events[0].record(stream)
        if keyed:                                           # the draw is part of the step: inside the device time
            noise = engine.keyed_noise(noises.seed, [noises.keys[ii] for ii in group],
                                       [lengths[ii] * dims.wn_in_rows_per_frame for ii in group])
        audio = engine.forward(mel, n_frames=n_frames, noise=noise, **control)
        events[1].record(stream)
        n_samples = [lengths[ii] * dims.hop_size for ii in group]
        model_audio = None
        if out_rate is not None:
            from .resample import device_taps, resample_device
            _, up, down = device_taps(int(round(dims.sample_rate)), int(round(out_rate)), engine.device)
            model_audio = (audio, n_samples)
            audio, _ = resample_device(audio, n_frames * dims.hop_size, int(round(dims.sample_rate)), int(round(out_rate)))
            n_samples = [-(-nn * up // down) for nn in n_samples]
        report = None
        if level is not None:
            from . import level as lv
            powers = level.powers(group)
            if model_audio is None:                         # the gain goes into a copy: the forward's audio stays as it is
                model_audio, gained = (audio, n_samples), torch.empty_like(audio.contiguous())
            else:
                gained = None                               # the resampler's output is this batch's own: in place
            audio = audio.contiguous()
            rate = dims.sample_rate if out_rate is None else out_rate
            measure = lv.measure_device(audio, n_samples, rate, level.true_peak)
            if not level.limiter:
                gains = lv.gains_device(measure, powers, ceiling=lv.ceiling_linear(level.peak_limit), true_peak=level.true_peak)
                audio = lv.apply_device(audio, n_samples, gains, out=gained)
                results = (measure.records, gains)
            else:
                # the loudness gain stands: no ceiling in it.  The limiter keeps the ceiling; what it wrote is measured again, and with the true peak a ceiling-only gain follows,
                # because the gain's modulation moves the peaks between the samples a little
                from . import limiter as lm
                ceiling = lv.ceiling_linear(level.peak_limit)
                h, hold = level.window(rate)
                gains = lv.gains_device(measure, powers)
                # the resampler's output is this batch's own: in place, as the static gain (the margins of the tiles go
                # through a workspace of (3 h + hold) / 2048 of the audio)
                audio, stats = lm.limit_device(audio, n_samples, gains, ceiling, h, hold, rate=rate, true_peak=level.true_peak,
                                               out=audio if gained is None else gained)
                after = lv.measure_device(audio, n_samples, rate, level.true_peak)
                results = (measure.records, gains, stats, after.records)
                if level.true_peak:
                    trim = lv.gains_device(after, None, ceiling=lm.trim_ceiling(ceiling), true_peak=True)
                    audio = lv.apply_device(audio, n_samples, trim)
                    results += (trim,)
            pinned = [torch.empty(tuple(tt.shape), dtype=tt.dtype, pin_memory=True) for tt in results]
            for host_copy, tt in zip(pinned, results):
                host_copy.copy_(tt, non_blocking=True)
            report = (level, powers) + tuple(pinned)
        enc = None
        if flac:
            enc = engine.encode_flac16(audio, n_samples, sample_rate=None if out_rate is None else int(round(out_rate)),
                                       wait=False, compression=flac_compression)
        host = None
        if host_audio:
            host = torch.empty(tuple(audio.shape), dtype=torch.float32, pin_memory=True)
            host.copy_(audio, non_blocking=True)
        events[2].record(stream)
        yield SynthBatch(group, n_samples, audio, enc, host, events, model_audio, report)


class _Clock:
    """Seconds per stage, summed over the threads of a pool."""

    def __init__(self):
        self._lock = threading.Lock()
        self.seconds = {}

    def add(self, key, seconds):
        with self._lock:
            self.seconds[key] = self.seconds.get(key, 0.0) + seconds


class _Job:
    """What run_job and run_audio_job share: the start time, the clock of the pool stages, a locked ``log``, "submit every
    micro-batch to the writers and wait", and the verbose line around the tool's own stages."""

    def __init__(self, threads):
        self.t_start, self.threads = time.perf_counter(), max(1, threads)
        self.clock, self._lock = _Clock(), threading.Lock()

    def log(self, lines):
        with self._lock:
            for line in lines:
                print(line, file=sys.stderr)

    def timed(self, key, func):
        """``func``, its seconds added to the clock under ``key``."""
        def call(*args):
            t0 = time.perf_counter()
            try:
                return func(*args)
            finally:
                self.clock.add(key, time.perf_counter() - t0)
        return call

    def write_all(self, work):
        """``work`` yields (writer task, SynthBatch) as the micro-batches are enqueued: submitted at once, all waited for."""
        with ThreadPoolExecutor(max_workers=self.threads) as writers:
            pending = [writers.submit(write, sb) for write, sb in work]
            for fu in pending:
                fu.result()

    def summary(self, tool, count, audio_s, stages, device, copy, note=""):
        """The verbose line: the tool's own ``stages`` between the totals and the micro-batches' device and copy time."""
        wall, sec = time.perf_counter() - self.t_start, self.clock.seconds
        print(f"{tool}: {count} files, {audio_s:.1f} s of audio{note} in {wall:.2f} s wall ({audio_s / max(wall, 1e-9):.1f} x "
              f"real time); {stages}, {device} {sec.get('device_ms', 0.0) / 1e3:.3f} s, {copy} "
              f"{sec.get('copy_ms', 0.0) / 1e3:.3f} s, MD5+write {sec.get('write', 0.0):.2f} s (pool stages summed over "
              f"{self.threads} threads each)", file=sys.stderr)


def level_line(outfile, report):
    """The writer's line about a file that went through the level stage (``SynthBatch.level``)."""
    def db(value):
        return "-inf" if not value > 0 else f"{20.0 * np.log10(value):.2f}"

    if np.isfinite(report["loudness_in"]):
        loud = f"{report['loudness_in']:.2f} -> {report['loudness_out']:.2f} LUFS"
    else:
        loud = "loudness not measurable (under 0.4 s, or silent)"
    why = " (the peak limit, not the loudness, set the gain)" if report["limited"] else ""
    if report.get("limiter"):
        lim = report["limiter"]
        why = (f", limiter: {lim['reduction_db']:.2f} dB at most, {lim['limited']} samples limited, {lim['clamped']} clamped"
               + (f", trim {lim['trim_db']:+.3f} dB" if lim["trim_db"] != 0.0 else ""))
    return f"    level of {outfile}: {loud}, gain {report['gain_db']:+.2f} dB, peak {db(report['peak_out'])} dBFS{why}"


def _file_writer(job, inv, files, mine, scaled, output_dir, fmt, device_flac, file_rate, flac_compression, verbose, quiet):
    """The writer-pool task of run_job and run_audio_job: ``write(sb)`` waits for the micro-batch ``sb`` (whose indices
    point into ``mine``) and writes syn_<basename>.<fmt> of each of its items, with the clipping note -- or, for a batch
    that went through the level stage, :func:`level_line` in its place -- and, ``verbose``, the mel error against ``scaled``."""
    from .mel_inverter import log_to_db
    rate = inv.srate

    def write(sb):
        sb.wait()
        t0 = time.perf_counter()
        for jj, local in enumerate(sb.indices):
            ii = mine[local]
            outfile = output_path(files[ii], output_dir, fmt)
            lines = [] if quiet else [f"synthesize {files[ii]} into {outfile}"]
            audio = sb.audio(jj) if (verbose or not device_flac) else None
            if verbose:                                  # as the one-at-a-time loop (reference :90-96)
                resyn = inv.generate_mel_from_snd(sb.model_audio(jj), srate=rate)['mell'].T[np.newaxis]
                err = log_to_db * np.mean(np.abs(scaled[ii] - resyn[:, :scaled[ii].shape[1]]))
                lines.append(f"    synthesized audio with {audio.size} samples in a micro-batch of {len(sb.indices)} "
                             f"({sb.device_ms:.1f} ms on the device), mel_error: {err:.3f}dB")
            peak, report = sb.max_abs(jj), sb.level(jj)
            if report is not None:
                lines.append(level_line(outfile, report))
            elif peak > 1:
                lines.append(f'    to prevent clipping you would need to normalize {outfile} by {0.99 / peak:.3f}')
            if verbose:
                lines.append(f"    save audio under {outfile}")
            if device_flac and np.isfinite(peak):
                sb.flac.write(outfile, jj)
            else:                                        # soundfile, wav, or an item the host writer must take
                write_audio(outfile, audio if audio is not None else sb.audio(jj), file_rate, fmt, flac_compression)
            job.log(lines)
        job.clock.add("write", time.perf_counter() - t0)
        job.clock.add("device_ms", sb.device_ms)
        job.clock.add("copy_ms", sb.copy_ms)

    return write


def f0_path(name, directory):
    """``directory/NAME.f0`` of a sound or ``.mell`` file ``name``: where the tools write and look for its F0 contour."""
    return os.path.join(directory or "", os.path.splitext(os.path.basename(name))[0] + ".f0")


def load_contour(name, directory, frames):
    """The contour ``resynth_mel.py --f0-dir`` gives the file ``name``: ``directory/NAME.f0`` (f0track.read_f0; one row per
    mel frame, another count is refused) through ``f0track.fill_unvoiced`` -- None when no frame is voiced: the F0-net."""
    from .f0track import fill_unvoiced, read_f0
    return fill_unvoiced(read_f0(f0_path(name, directory), n_frames=frames)[1])


def run_job(inv, files, output_dir, fmt, frames=None, mine=None, batch=16, threads=2, verbose=False, quiet=False,
            flac_compression="verbatim", out_rate=None, noise_seed=None, transposition=None, formant=None, f0_dir=None,
            level=None):
    """The batched CLI on this process's GPU: ``files[mine]`` -> syn_<basename>.<fmt> in ``output_dir``.

    ``frames``: the frame count after scale_mel of EVERY file of the job, in file order (the noise replay needs all of
    them; default: read here, which needs ``mine`` = all files).  Reader pool (load_var + scale_mel; a missing or bad file
    fails before anything runs), device (forward, FLAC frames, asynchronous copies into pinned memory), writer pool (MD5,
    header, file write); both pools have ``threads`` threads.  ``flac_compression``: what the built-in FLAC writers emit,
    on the device and on the host ("verbatim" or "fixed").  ``out_rate``: the files are written at that rate (resampled on
    the device, ``run_micro_batches``); the verbose ``mel_error`` stays computed on the model-rate audio, the clipping note
    is about what is written.  ``noise_seed``: the noise channel takes the keyed noise of that seed instead of the replayed
    draws, the key of a file being ``noise.item_key`` of its basename -- a file's audio then does not depend on the other
    files; ``transposition``: a factor on every mel frame of every file (``f0_scale`` rows); ``formant``: a formant-shift
    factor on every mel frame of every file (``formant`` rows).  ``f0_dir``: every file takes the contour of
    ``f0_dir/NAME.f0`` (:func:`load_contour`; a missing file or a wrong row count fails before anything runs) in place of the
    F0-net's.  ``level``: a ``level.LevelControl`` with a loudness in LUFS and / or a peak limit (``run_micro_batches``): the
    files are written at that level and the writer reports it in place of the clipping note.  All None: today's job."""
    job = _Job(threads)
    mine = list(range(len(files))) if mine is None else list(mine)

    def read(ii):
        if verbose:
            job.log([f"load mell  from {files[ii]}"])
        return inv.scale_mel(load_var(files[ii]), verbose=verbose)

    with ThreadPoolExecutor(max_workers=job.threads) as pool:
        scaled = dict(zip(mine, pool.map(job.timed("read", read), mine)))
    if frames is None:
        if sorted(mine) != list(range(len(files))):
            raise ValueError("run_job: the frames of every file are needed when this process writes only some of them")
        frames = [int(scaled[ii].shape[1]) for ii in range(len(files))]
    for ii in mine:
        if int(scaled[ii].shape[1]) != int(frames[ii]):
            raise RuntimeError(f"{files[ii]}: {scaled[ii].shape[1]} frames after scale_mel, the job plan says {frames[ii]}")
    dims = inv.model.dims
    draws = (replay_noise(frames, dims.wn_in_rows_per_frame, keep=mine, device=inv.model.device)
             if dims.noise_sigma and noise_seed is None else None)
    device_flac = fmt.lower() == "flac" and not have_soundfile()
    rate = inv.srate
    out_rate = inv._output_rate(out_rate)
    write = _file_writer(job, inv, files, mine, scaled, output_dir, fmt, device_flac, rate if out_rate is None else out_rate,
                         flac_compression, verbose, quiet)
    mels = [scaled[ii][0] for ii in mine]
    noises = None if draws is None else [draws[ii] for ii in mine]
    if noise_seed is not None and dims.noise_sigma:
        from .mel_inverter import KeyedNoise
        from .noise import item_key
        noises = KeyedNoise(noise_seed, [item_key(files[ii]) for ii in mine])
    rows = None if transposition is None else [np.full(int(mm.shape[0]), transposition, dtype=np.float32) for mm in mels]
    shifts = None if formant is None else [np.full(int(mm.shape[0]), formant, dtype=np.float32) for mm in mels]
    contours = None if f0_dir is None else [load_contour(files[ii], f0_dir, int(scaled[ii].shape[1])) for ii in mine]
    job.write_all((write, sb) for sb in run_micro_batches(inv.model, mels, noises, max(1, batch), flac=device_flac,
                                                          host_audio=verbose or not device_flac,
                                                          flac_compression=flac_compression, out_rate=out_rate,
                                                          transpositions=rows, formants=shifts, f0s=contours, level=level))
    if verbose:
        job.summary("resynth_mel", len(mine), sum(int(frames[ii]) for ii in mine) * inv.hop_size / rate,
                    f"read+scale {job.clock.seconds.get('read', 0.0):.2f} s", "device", "encode+D2H")


def read_transposition_file(path):
    """``--transposition-file``: lines ``basename factor`` -> {basename: factor}.  Blank lines and what follows a ``#`` are
    ignored; a line of another shape, a factor that is not a finite positive number or a basename given twice raises
    ValueError with the line number."""
    table = {}
    with open(path) as fi:
        for number, line in enumerate(fi, 1):
            fields = line.split("#", 1)[0].split()
            if not fields:
                continue
            try:
                if len(fields) != 2:
                    raise ValueError("expected `basename factor`")
                factor = float(fields[1])
                if not (np.isfinite(factor) and factor > 0):
                    raise ValueError("the factor must be finite and positive")
                if os.path.basename(fields[0]) in table:
                    raise ValueError(f"{fields[0]} is listed twice")
            except ValueError as err:
                raise ValueError(f"{path}:{number}: {err}") from None
            table[os.path.basename(fields[0])] = factor
    return table


def file_factors(files, transposition=1.0, table=None, what="transposition"):
    """The transposition factor of every file: ``table[basename]`` (read_transposition_file) where it is listed, else
    ``transposition``; every factor finite and positive, or ValueError.  ``what`` names the factor in the message
    (``--formant-shift-file`` has the format and the reader of ``--transposition-file``)."""
    table = table or {}
    factors = [float(table.get(os.path.basename(ff), transposition)) for ff in files]
    if not all(np.isfinite(ff) and ff > 0 for ff in factors):
        raise ValueError(f"{what} must be finite and positive")
    return factors


def file_stretches(files, stretch=1.0, table=None):
    """The time-stretch factor of every file: ``table[basename]`` (read_transposition_file: ``--time-stretch-file`` has the
    format of ``--transposition-file``) where it is listed, else ``stretch``; every factor finite and positive, or
    ValueError."""
    return file_factors(files, stretch, table, what="time stretch")


def read_sound(path):
    """``audioio.read_audio`` for the file-to-file tool: (samples, rate), or ValueError for what the tool skips -- a file
    with more than one channel, without samples or with an invalid rate."""
    from .audioio import read_audio
    snd, rate = read_audio(path)
    if snd.size == 0:
        raise ValueError(f"{path}: no samples")
    if int(round(rate)) <= 0:
        raise ValueError(f"{path}: invalid sample rate {rate}")
    return snd, int(round(rate))


def run_audio_job(inv, files, output_dir, fmt, factors=None, noise_seed=0, mine=None, batch=16, threads=2, verbose=False,
                  quiet=False, flac_compression="verbatim", out_rate=None, stretches=None, formants=None, f0_source="net",
                  f0_params=None, write_f0=False, timings=None, f0_decode=None, f0_fill="interpolate", f0_initial=150.0,
                  guides=None, align_band_s=1.0, loudness=None, peak_limit=None, true_peak=False, *, limiter=False,
                  lookahead_ms=None, hold_ms=None, f0_lag=None):
    """The file-to-file tool on this process's GPU: sound files ``files[mine]`` -> transposed syn_<basename>.<fmt> in
    ``output_dir``.  Returns the (file, reason) pairs it skipped: files without samples or with more than one channel.

    Reader pool (``read_sound``), device (``analysis.generate_mels``: resampler and mel analysis in micro-batches grouped by
    rate), pool again (``scale_mel``, on the host: the mel then has the bits of generate_mel.py followed by resynth_mel.py),
    device (``run_micro_batches`` with the keyed noise of ``noise_seed`` -- the key of a file is ``noise.item_key`` of its
    basename --, ``factors[i]`` on every frame of file i, the output resampler and the FLAC frames), writer pool.  A file
    gives frames * hop samples at the model rate before the output resampler, as a live stream of it emits.
    ``out_rate``: a rate in Hz, ``"input"`` (every file at its own rate) or None (the model rate).  Nothing is replayed and
    nothing depends on ``mine``: a file's audio is a function of the file, the model, the seed, its factor and the rate.

    ``stretches``: a time-stretch factor per file (timemap.py), None = 1 for all.  File i is analysed
    at the centres of ``timemap.centres`` for ``stretches[i]`` and gives K_i * hop samples, ``stretches[i]`` times as long
    at the same pitch.  With every factor 1 the job makes the launches and writes the bytes it does without the argument.  A
    file whose stretched length exceeds the engine's limit is reported and skipped like the unreadable ones.

    ``formants``: a formant-shift factor per file, None = 1 for all: ``formants[i]`` on every frame of
    file i, pitch and duration kept.  With every factor 1 the job makes the launches and writes the bytes it does without.

    ``f0_source``: "net", or "audio" -- the F0 tracker (f0track.py; ``f0_params``: keywords of
    ``f0track.params``) runs behind the analysis of every micro-batch, on the frames of the mel, and a file's filled contour
    replaces the F0-net's; ``factors`` multiply on top; a file without a voiced frame keeps the F0-net.  ``write_f0``:
    the tracked contour (0 = unvoiced) is written as NAME.f0 into ``output_dir``, with either source.  "net" without
    ``write_f0``: the launches and the bytes of before.  ``f0_decode``: None, or a ``f0decode.decode_params`` dictionary: the
    contour, used and written, is the Viterbi path over the YIN candidates of the file's frames;
    it needs "audio" or ``write_f0``.  ``f0_lag``: None, or the decoder's look-ahead in frames: the
    contour a live stream with that lag decides; it needs ``f0_decode``.  ``f0_fill``: "interpolate", or "hold" -- the causal fill of the live streams
    (``f0track.fill_hold`` with ``f0_initial`` Hz in front of the first voiced frame); it needs "audio".
    ``guides``: per file None or the path of a guide recording, None = none for all: file i comes out
    with the TIMING of its guide -- the guide's frame count, hence its length -- through ``generate_mels(guides=)`` with a
    band of ``align_band_s`` seconds; it takes no ``stretches`` entry other than 1.  A guide that cannot be read, and a file
    that cannot be aligned to its guide, is reported and skipped like the unreadable ones; ``verbose`` prints the path's mean
    cost per node and its largest offset from the diagonal.  No guide: the launches and the bytes of before.
    ``loudness``: None, a number of LUFS, or ``"input"`` -- every file comes out at the loudness of its source, measured as
    read, at its own rate, on the device in the micro-batches the analysis stages (``generate_mels(levels_out=)``); a source
    that is not measurable leaves the loudness gain at 1.  ``peak_limit``: a ceiling in dBFS (default: -1 with a loudness, else
    none); ``true_peak``: on the 4x true peak.  DESIGN.md section 6m.  None of them: the launches and the bytes of before.
    ``limiter``: the look-ahead limiter keeps the ceiling in place of the static gain (``lookahead_ms`` / ``hold_ms``: its
    window); without it, the launches and the bytes of before.
    ``timings``: a dict that receives the seconds per stage the
    verbose line reports (upload, resample, analysis, f0, copy_back from ``generate_mels``; read, scale, device, copy, write
    from the pools and the micro-batches' events; wall)."""
    from . import f0track
    from .level import check_options, level_control
    loudness, peak_limit, true_peak = check_options(loudness, peak_limit, true_peak, allow_input=True, limiter=limiter,
                                                    lookahead_ms=lookahead_ms, hold_ms=hold_ms)   # before anything runs
    window_check = level_control(None if isinstance(loudness, str) else loudness, peak_limit, true_peak, limiter, lookahead_ms,
                                 hold_ms)
    if window_check is not None and out_rate != "input":   # the limiter's window at the rate of the files: before anything runs
        window_check.check_rates([inv.srate if out_rate is None else out_rate])
    job = _Job(threads)
    mine = list(range(len(files))) if mine is None else list(mine)
    factors = [1.0] * len(files) if factors is None else list(factors)
    guides = None if guides is None or all(gg is None for gg in guides) else list(guides)
    if guides is not None and len(guides) != len(files):
        raise ValueError(f"run_audio_job: guides takes one entry per file ({len(files)}), got {len(guides)}")
    stats = {}
    with ThreadPoolExecutor(max_workers=job.threads) as pool:                                   # the readers, then scale_mel
        loaded, guide_sounds, mine, maps, skipped = _load_sounds(job, pool, inv, files, mine, guides, stretches)
        if window_check is not None and out_rate == "input":       # ... at every file's own rate: known once they are read
            window_check.check_rates([loaded[ii][1] for ii in mine] or [inv.srate])
        have_guides = guides is not None and any(guides[ii] is not None for ii in mine)
        scale = job.timed("scale", lambda dd: inv.scale_mel(dd, verbose=verbose))
        try:
            done = analyse_for_synthesis(
                inv, [loaded[ii][0] for ii in mine], [loaded[ii][1] for ii in mine], time_maps=[maps[ii] for ii in mine],
                guides=[None if guides[ii] is None else guide_sounds[guides[ii]][0] for ii in mine] if have_guides else None,
                guide_rates=[None if guides[ii] is None else guide_sounds[guides[ii]][1] for ii in mine] if have_guides else None,
                align_band_s=align_band_s, f0_source=f0_source, f0_params=f0_params, f0_decode=f0_decode, f0_fill=f0_fill,
                f0_initial=f0_initial, write_f0=bool(write_f0), batch=batch, stats=stats,
                scale_map=lambda dicts: list(pool.map(scale, dicts)), who="run_audio_job", f0_lag=f0_lag,
                source_levels=loudness == "input")
        except ValueError as err:
            if not have_guides:
                raise
            raise ValueError(f"align: {err}") from None
    lines = []
    for local, ii in enumerate(mine):                          # the files without a path leave the job here
        note = done.notes.get(local)
        if note is not None and "error" in note:
            skipped.append((files[ii], f"{note['error']} (guide {guides[ii]})"))
            lines.append(f"transform_audio::error:: skipped {files[ii]}: {note['error']} (guide {guides[ii]})")
        elif note is not None and verbose:
            lines.append(f"    aligned {files[ii]} to {guides[ii]}: {note['nodes']} nodes, mean cost per node "
                         f"{note['mean_cost']:.3f}, largest offset from the diagonal {note['max_offset_ms']:.1f} ms")
    job.log(lines)
    keep = [local for local in range(len(mine)) if done.scaled[local] is not None]
    scaled = {mine[local]: done.scaled[local] for local in keep}
    contours = None if done.contours is None else {mine[local]: done.contours[local] for local in keep}
    if write_f0:
        for local in keep:
            f0, periodicity = done.tracked[local]
            f0track.write_f0(f0_path(files[mine[local]], output_dir), f0track.frame_times(f0.size, inv.hop_size, inv.srate),
                             f0, periodicity)
    if loudness == "input":                                    # the source's P is the target of its output
        loudness = [None] * len(files)
        for local in keep:
            power, count = done.levels[local]
            loudness[mine[local]] = power if count else None
    control = level_control(loudness, peak_limit, true_peak, limiter, lookahead_ms, hold_ms)
    mine = [mine[local] for local in keep]
    rates = {ii: loaded[ii][1] if out_rate == "input" else out_rate for ii in mine}
    _synthesise_files(job, inv, files, mine, scaled, contours, rates, output_dir, fmt, factors, formants, noise_seed, batch,
                      flac_compression, verbose, quiet, control)
    if timings is not None:
        sec = job.clock.seconds
        timings.update(stats, read=sec.get("read", 0.0), scale=sec.get("scale", 0.0), device=sec.get("device_ms", 0.0) / 1e3,
                       copy=sec.get("copy_ms", 0.0) / 1e3, write=sec.get("write", 0.0), wall=time.perf_counter() - job.t_start)
    if verbose:
        in_s = sum(loaded[ii][0].size / loaded[ii][1] for ii in mine)
        note = "" if all(maps[ii] is None for ii in mine) else f" (time-stretched from {in_s:.1f} s of input)"
        if guides is not None:
            note = f" (aligned to guides, from {in_s:.1f} s of input)"
        sec = job.clock.seconds
        job.summary("transform_audio", len(mine), sum(int(scaled[ii].shape[1]) for ii in mine) * inv.hop_size / inv.srate,
                    f"read {sec.get('read', 0.0):.2f} s, upload {stats.get('upload', 0.0):.3f} s, resample "
                    f"{stats.get('resample', 0.0):.3f} s, analysis {stats.get('analysis', 0.0):.3f} s, "
                    + (f"f0 tracker {stats.get('f0', 0.0):.3f} s, " if done.tracked is not None else "") + "mel copy-back "
                    f"{stats.get('copy_back', 0.0):.3f} s, scale_mel {sec.get('scale', 0.0):.2f} s", "noise+forward",
                    "resample+encode+D2H", note)
    return skipped


def check_stretch(n_samples, rate, factor, hop, target, rows_per_frame):
    """ValueError (``timemap.frame_count``) when ``n_samples`` at ``rate``, stretched by ``factor``, exceed the engine's
    limit.  A factor of exactly 1 is the regular analysis: never refused."""
    from . import timemap
    from .analysis import resampled_length
    if factor != 1.0:
        timemap.frame_count(resampled_length(n_samples, rate, target), hop, target, factor, rows_per_frame)


def _load_sounds(job, pool, inv, files, mine, guides, stretches):
    """Phase one of run_audio_job, on the reader ``pool``: the sounds {index: (samples, rate)}, the guides {path: (samples,
    rate)}, the indices that stay in the job, their time maps {index: None or a factor} and the (file, reason) pairs of
    the others, reported here: an unreadable file or guide, a stretched length beyond the engine's limit."""
    def read(path):
        try:
            return read_sound(path)
        except ValueError as err:
            return err

    def read_guide(path):
        try:
            return read_sound(path)
        except (OSError, ValueError) as err:
            return ValueError(f"guide {path}: {err}")

    loaded = dict(zip(mine, pool.map(job.timed("read", read), [files[ii] for ii in mine])))
    why = {ii: str(loaded[ii]) for ii in mine if isinstance(loaded[ii], ValueError)}
    paths = sorted({guides[ii] for ii in mine if ii not in why and guides is not None and guides[ii] is not None})
    guide_sounds = dict(zip(paths, pool.map(read_guide, paths)))
    # a factor of exactly 1 is the regular analysis; every other one is checked against the engine's limit below
    maps = {ii: None if stretches is None or float(stretches[ii]) == 1.0 else float(stretches[ii]) for ii in mine}
    for ii in [ii for ii in mine if ii not in why]:
        guide = None if guides is None or guides[ii] is None else guide_sounds[guides[ii]]
        if isinstance(guide, ValueError):
            why[ii] = str(guide)
        elif guide is not None and maps[ii] is not None:
            raise ValueError(f"run_audio_job: {files[ii]} has a guide and a time stretch; the guide sets its timing")
    for ii in [ii for ii in mine if ii not in why and maps[ii] is not None]:
        try:
            check_stretch(loaded[ii][0].size, loaded[ii][1], maps[ii], inv.hop_size, inv.srate, inv.model.dims.steps_per_frame)
        except ValueError as err:
            why[ii] = str(err)
    skipped = [(files[ii], reason) for ii, reason in why.items()]
    job.log([f"transform_audio::error:: skipped {name}: {reason}" for name, reason in skipped])
    return loaded, guide_sounds, [ii for ii in mine if ii not in why], maps, skipped


def analyse_for_synthesis(inv, sounds, rates, time_maps=None, guides=None, guide_rates=None, align_band_s=1.0, f0_source="net",
                          f0_params=None, f0_decode=None, f0_fill="interpolate", f0_initial=150.0, write_f0=None, batch=16,
                          stats=None, scale_map=None, on_device=True, rows_per_frame=None, who="analyse_for_synthesis",
                          source_levels=False, f0_lag=None):
    """Sounds in, what the synthesis takes out: the step between reading and ``run_micro_batches``, the same code under
    ``MELInverter.transform_audio`` and :func:`run_audio_job`.  ``sounds`` at ``rates`` go through ``analysis.generate_mels``
    (``time_maps``, ``guides``, ``guide_rates``, ``align_band_s``, ``batch``, ``stats``, ``on_device`` and ``rows_per_frame``
    -- default: the engine's -- as there) and ``inv.scale_mel``; ``scale_map``: a function from the list of ``.mell``
    dictionaries to the list of scaled mels, for a caller with a thread pool.  The pitch options are checked before anything
    runs, ``who`` naming the caller: ``f0_source`` "net" or "audio", ``f0_params`` keywords of ``f0track.params``,
    ``f0_decode`` None or ``f0decode.decode_params`` (it needs a tracked contour), ``f0_lag`` None or the decoder's fixed
    lag in frames (it needs ``f0_decode``; ``analysis.generate_mels``), ``f0_fill`` / ``f0_initial`` as
    ``f0track.fill_tracked`` takes them; ``write_f0``: None for a caller without the option, else whether "net" tracks too.

    Returns a namespace: ``scaled`` (1, T, mel_channels), ``contours`` (filled; an item without a voiced frame: None; not
    "audio": None as a whole) and ``tracked`` (raw (f0, periodicity); nothing tracked: None as a whole) hold one entry per
    sound; ``notes`` is {item: ``align.path_stats`` or {"error": message}}.  An item that cannot be aligned to its guide
    has its note and None in all three lists.  ``source_levels``: ``levels`` holds, per sound, (P, count) of the sound as it
    was handed in, at its own rate (``level.py``; ``generate_mels(levels_out=)``); else None."""
    from types import SimpleNamespace
    from . import f0track
    from .analysis import generate_mels
    if f0_source not in ("net", "audio"):
        raise ValueError(f"{who}: f0_source must be 'net' or 'audio', got {f0_source!r}")
    f0track.check_fill(f0_fill, f0_source, who)
    tracked = [] if f0_source == "audio" or write_f0 else None
    if f0_decode is not None and tracked is None:
        raise ValueError(f"{who}: f0_decode decodes the tracked contour and needs f0_source='audio'"
                         + ("" if write_f0 is None else " or write_f0"))
    if f0_lag is not None and f0_decode is None:
        raise ValueError(f"{who}: f0_lag is the look-ahead of the decoder and needs f0_decode")
    if tracked is not None:
        f0_params = f0track.params(int(round(inv.srate)), **(f0_params or {}))
    guided = guides is not None and any(gg is not None for gg in guides)
    notes = {}
    dicts = []
    levels = [] if source_levels else None
    if len(sounds):
        dicts = generate_mels(sounds, rates, inv.preprocess_config, on_device=on_device, batch=max(1, batch), stats=stats,
                              time_maps=None if time_maps is None or all(mm is None for mm in time_maps) else list(time_maps),
                              rows_per_frame=inv.model.dims.steps_per_frame if rows_per_frame is None else rows_per_frame,
                              f0_out=tracked, f0_params=f0_params if tracked is not None else None, f0_decode=f0_decode,
                              guides=guides if guided else None, guide_rates=guide_rates if guided else None,
                              align_band_s=align_band_s, align_out=notes if guided else None, f0_lag=f0_lag,
                              levels_out=levels)
    keep = [ii for ii, dd in enumerate(dicts) if dd is not None]
    scale_map = scale_map or (lambda some: [inv.scale_mel(dd) for dd in some])
    scaled = [None] * len(dicts)
    for ii, mel in zip(keep, scale_map([dicts[ii] for ii in keep])):
        scaled[ii] = mel
    contours = None
    if f0_source == "audio":
        contours = [None if pair is None else f0track.fill_tracked(pair[0], f0_fill, f0_initial) for pair in tracked]
    return SimpleNamespace(scaled=scaled, contours=contours, tracked=tracked, notes=notes, levels=levels)


def _synthesise_files(job, inv, files, mine, scaled, contours, rates, output_dir, fmt, factors, formants, noise_seed, batch,
                      flac_compression, verbose, quiet, level=None):
    """Phase three of run_audio_job: the files ``mine`` grouped by the rate they are written at (``rates``: {index: a rate
    or None}), each group through ``run_micro_batches`` with keyed noise and per-file factors, then to the writers.
    ``level``: None or the job's ``level.LevelControl``, a target list indexed like ``files``."""
    from .level import LevelControl
    from .mel_inverter import KeyedNoise
    from .noise import item_key
    dims = inv.model.dims
    device_flac = fmt.lower() == "flac" and not have_soundfile()
    groups = {}
    for ii in mine:
        groups.setdefault(inv._output_rate(rates[ii]), []).append(ii)

    def work():
        for rate, sub in groups.items():
            write = _file_writer(job, inv, files, sub, scaled, output_dir, fmt, device_flac, inv.srate if rate is None else rate,
                                 flac_compression, verbose, quiet)
            noises = KeyedNoise(noise_seed, [item_key(files[ii]) for ii in sub]) if dims.noise_sigma else None
            rows = [np.full(int(scaled[ii].shape[1]), factors[ii], dtype=np.float32) for ii in sub]
            shifts = None if formants is None else [np.full(int(scaled[ii].shape[1]), formants[ii], dtype=np.float32) for ii in sub]
            part = level
            if level is not None and isinstance(level.target, (list, tuple)):
                part = level.sliced(sub)
            for sb in run_micro_batches(inv.model, [scaled[ii][0] for ii in sub], noises, max(1, batch), flac=device_flac,
                                        host_audio=verbose or not device_flac, flac_compression=flac_compression, out_rate=rate,
                                        transpositions=rows, formants=shifts,
                                        f0s=None if contours is None else [contours[ii] for ii in sub], level=part):
                yield write, sb

    job.write_all(work())


def plan_audio_ranks(files, ranks, threads=2, stretches=None, frame_limit=None, guides=None):
    """What the parent of a ``transform_audio.py --gpus N`` job decides before it starts its ranks, without importing torch:
    the visible GPUs, the files it skips -- (file, reason) pairs, ``read_sound`` -- and the LPT partition of the others by
    duration times ``stretches[i]`` (the seconds the file comes out with; None = 1 for all).  ``files`` in the plan are the
    ones the ranks share out.  ``frame_limit``: (hop, model rate, sub-band rows per frame) -- a file whose stretched length
    exceeds the engine's limit (``timemap.frame_count``) is skipped here, as ``run_audio_job`` would skip it.  ``guides``: per
    file None or the path of its guide (``run_audio_job``): an aligned file comes out with its guide's duration and is
    weighed by it; a guide that cannot be read skips the file."""
    def seconds_of(item):
        path, factor, guide = item
        try:
            snd, rate = read_sound(path)
            if guide is not None:
                try:
                    snd, rate = read_sound(guide)
                except (OSError, ValueError) as err:
                    raise ValueError(f"guide {guide}: {err}") from None
            if frame_limit is not None:
                check_stretch(snd.size, rate, factor, *frame_limit)
            return snd.size / rate
        except ValueError as err:
            return err

    factors = [1.0] * len(files) if stretches is None else [float(ff) for ff in stretches]
    guides = [None] * len(files) if guides is None else list(guides)
    with ThreadPoolExecutor(max_workers=max(1, threads)) as pool:
        seconds = list(pool.map(seconds_of, zip(files, factors, guides)))
    good = [ii for ii, ss in enumerate(seconds) if not isinstance(ss, ValueError)]
    cost = [int(np.ceil(seconds[ii] * factors[ii] * 1000)) for ii in good]
    return {"devices": visible_gpu_count(), "files": [files[ii] for ii in good], "shards": lpt_partition(cost, ranks),
            "skipped": [[files[ii], str(ss)] for ii, ss in enumerate(seconds) if isinstance(ss, ValueError)]}


def plan_ranks(model_id_or_path, files, ranks, threads=2):
    """What the parent of a ``--gpus N`` job decides before it starts its ranks, without importing torch: the number of
    visible GPUs (sharding.visible_gpu_count), the frames after scale_mel of every file (a missing or bad file fails here,
    before any rank starts) and the LPT partition of the files by frames."""
    from .mel_inverter import MELInverter
    inv = MELInverter.host_only(model_id_or_path)

    def frames_of(path):
        return int(inv.scale_mel(load_var(path)).shape[1])

    with ThreadPoolExecutor(max_workers=max(1, threads)) as pool:
        frames = list(pool.map(frames_of, files))
    return {"devices": visible_gpu_count(), "frames": frames, "shards": lpt_partition(frames, ranks)}


def run_ranks(script, child_argv, model_id_or_path, files, ranks, threads=2, quiet=False, poll_s=0.05, plan=None,
              tool="resynth_mel"):
    """``resynth_mel.py --gpus N``: plan the job (:func:`plan_ranks`), start N fresh child processes ``script child_argv
    --rank r --job <plan>`` (rank r on visible device r % count), poll them; when one fails, end the others.  Returns the
    exit status of the job.  ``plan``: a plan made by the caller (``plan_audio_ranks``) instead; ``tool`` names the messages."""
    plan = plan_ranks(model_id_or_path, files, ranks, threads) if plan is None else plan
    if plan["devices"] < 1:
        print(f"{tool}::error:: no GPU visible", file=sys.stderr)
        return 1
    if ranks > plan["devices"] and not quiet:
        print(f"{tool}::note:: {ranks} ranks on {plan['devices']} visible GPU(s): rank r runs on device r % "
              f"{plan['devices']}, ranks share a GPU", file=sys.stderr)
    with tempfile.TemporaryDirectory() as tmp:
        job = os.path.join(tmp, "job.json")
        with open(job, "w") as fo:
            json.dump(plan, fo)
        procs = [subprocess.Popen([sys.executable, script, *child_argv, "--rank", str(rr), "--job", job])
                 for rr in range(ranks)]
        try:
            while True:
                codes = [pp.poll() for pp in procs]
                if any(cc not in (None, 0) for cc in codes):
                    return 1
                if all(cc == 0 for cc in codes):
                    return 0
                time.sleep(poll_s)
        finally:
            for pp in procs:
                if pp.poll() is None:
                    pp.terminate()
            for pp in procs:
                try:
                    pp.wait(timeout=30)
                except subprocess.TimeoutExpired:
                    pp.kill()
                    pp.wait()

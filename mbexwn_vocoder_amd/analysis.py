"""Audio -> log-mel analysis (the step in front of the hot path).  Host side, numpy.

Restates, for the configuration the CLI uses (no band limiting, ``do_post=False``):
  compute_mel_spectrogram_internal   reference MBExWN_NVoc/vocoder/model/preprocess.py:417-572
  calc_stft (magnitude, centred)     reference MBExWN_NVoc/sig_proc/spec/stft.py:14-96
  window("hann", N)                  reference MBExWN_NVoc/sig_proc/Mwindows.py:60-67,176-185 (symmetric, zero end points)
  get_mel_filter                     reference preprocess.py:51-74 -> librosa.filters.mel(htk=False, norm="slaney")

librosa (requirements.txt: librosa >= 0.8, unpinned) is a third-party dependency that is neither in the reference
tree nor installable here; its mel basis is restated from the published Slaney Auditory-Toolbox formulas that the
librosa documentation gives (linear below 1 kHz with 200/3 Hz per mel, logarithmic above with step ln(6.4)/27,
triangles normalised by 2 / bandwidth).  The STFT part is pinned by golden vectors captured from the reference's
importable numpy code (tests/golden/reference_constants.npz); the mel basis is pinned only by its defining properties.
"""
import numpy as np


def hann_symmetric(n):
    """reference Mwindows.window("hann", n): 0.5 - 0.5 cos(2 pi k / (n-1)), mirrored around the centre."""
    win = np.zeros((n,))
    mid = (n - 1) // 2
    xx = np.arange(mid + 1)
    half = 0.5 - 0.5 * np.cos(2.0 * np.pi * xx / (n - 1))
    win[:mid + 1] = half
    win[n - 1:n - 2 - mid:-1] = half
    return win


def stft_magnitude(x, win_len, hop_len, fft_size, dtype=np.float32, pad_mode="reflect"):
    """|STFT| of x (batch, time): frames centred on multiples of hop_len, reference calc_stft(center=True, do_mag=True).
    Returns (batch, n_frames, fft_size//2+1)."""
    x = np.atleast_2d(np.asarray(x))
    win = hann_symmetric(win_len).astype(dtype)
    n_frames = x.shape[-1] // hop_len + 1
    xp = np.pad(x.astype(dtype, copy=False), ((0, 0), (win_len // 2, win_len)), mode=pad_mode)
    out = np.empty((x.shape[0], n_frames, fft_size // 2 + 1), dtype=dtype)
    for ii in range(n_frames):
        seg = xp[:, ii * hop_len: ii * hop_len + win_len]
        out[:, ii] = np.abs(np.fft.rfft(win * seg, fft_size))
    return out


def _hz_to_mel_slaney(freq):
    freq = np.asarray(freq, dtype=np.float64)
    f_sp = 200.0 / 3
    mels = freq / f_sp
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(freq >= min_log_hz, min_log_mel + np.log(np.maximum(freq, 1e-30) / min_log_hz) / logstep, mels)


def _mel_to_hz_slaney(mels):
    mels = np.asarray(mels, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(mels >= min_log_mel, min_log_hz * np.exp(logstep * (mels - min_log_mel)), f_sp * mels)


def mel_frequencies(n_mels, fmin, fmax):
    """n_mels frequencies uniformly spaced on the Slaney mel scale between fmin and fmax."""
    return _mel_to_hz_slaney(np.linspace(_hz_to_mel_slaney(fmin), _hz_to_mel_slaney(fmax), n_mels))


def mel_basis_slaney(sr, n_fft, n_mels, fmin, fmax, dtype=np.float32):
    """(n_mels, n_fft//2+1) triangular filters, area-normalised ("slaney" norm)."""
    if fmax is None:
        fmax = sr / 2.0
    fft_freqs = np.linspace(0, sr / 2.0, n_fft // 2 + 1)
    mel_f = mel_frequencies(n_mels + 2, fmin, fmax)
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_freqs[None, :]
    weights = np.zeros((n_mels, n_fft // 2 + 1))
    for ii in range(n_mels):
        lower = -ramps[ii] / fdiff[ii]
        upper = ramps[ii + 2] / fdiff[ii + 1]
        weights[ii] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    return (weights * enorm[:, None]).astype(dtype)


def compute_log_mel(sound, preprocess_config, dtype=np.float32):
    """reference compute_mel_spectrogram_internal(sound, cfg, band_limit=None, do_post=False):
    (batch, time) audio -> (batch, frames, mel_channels) natural-log mel amplitudes, and the mel frame rate."""
    sound = np.atleast_2d(np.asarray(sound))
    win_len = preprocess_config.get("win_size", preprocess_config["fft_size"])
    spec = stft_magnitude(sound, win_len, preprocess_config["hop_size"], preprocess_config["fft_size"], dtype=dtype)
    basis = mel_basis_slaney(preprocess_config["sample_rate"], preprocess_config["fft_size"],
                             preprocess_config["mel_channels"], preprocess_config["fmin"], preprocess_config["fmax"], dtype=dtype)
    mel = np.dot(spec, basis.T)
    mell = np.log(np.fmax(mel, np.finfo(mel.dtype).eps))
    return mell, preprocess_config["sample_rate"] / preprocess_config["hop_size"]


def compute_log_mel_at(sound, centres, preprocess_config, dtype=np.float32):
    """:func:`compute_log_mel` with the frames centred where ``centres`` says (timemap.py): the host
    definition of ``mbxw_mel_frames_at``.  ``sound``: (time,) or (batch, time); ``centres``: (K,) for all items or
    (batch, K), integers, clipped to [0, time].  Frame k of an item holds the ``win`` samples of the reflect-padded sound
    from ``c - win // 2`` on and goes through the numpy steps of :func:`stft_magnitude` and :func:`compute_log_mel`:
    centres ``k * hop`` therefore give ``compute_log_mel``'s bits.  Returns (batch, K, mel_channels) and the frame rate."""
    cfg = preprocess_config
    sound = np.atleast_2d(np.asarray(sound))
    win_len, fft_size = int(cfg.get("win_size", cfg["fft_size"])), int(cfg["fft_size"])
    cc = np.asarray(centres)
    if cc.dtype.kind not in "iu" or cc.ndim not in (1, 2):
        raise ValueError("compute_log_mel_at: centres must be an integer array (K,) or (batch, K)")
    cc = np.clip(np.broadcast_to(np.atleast_2d(cc).astype(np.int64), (sound.shape[0], cc.shape[-1])), 0, sound.shape[-1])
    win = hann_symmetric(win_len).astype(dtype)
    xp = np.pad(sound.astype(dtype, copy=False), ((0, 0), (win_len // 2, win_len)), mode="reflect")
    spec = np.empty((sound.shape[0], cc.shape[1], fft_size // 2 + 1), dtype=dtype)
    for ii in range(cc.shape[1]):
        seg = xp[np.arange(sound.shape[0])[:, None], cc[:, ii, None] + np.arange(win_len)[None, :]]
        spec[:, ii] = np.abs(np.fft.rfft(win * seg, fft_size))
    basis = mel_basis_slaney(cfg["sample_rate"], fft_size, cfg["mel_channels"], cfg["fmin"], cfg["fmax"], dtype=dtype)
    mel = np.dot(spec, basis.T)
    mell = np.log(np.fmax(mel, np.finfo(mel.dtype).eps))
    return mell, cfg["sample_rate"] / cfg["hop_size"]


def mel_analysis_tables(preprocess_config):
    """The tables :func:`compute_log_mel_device` uploads, as numpy arrays: the float32 analysis window (win,), the twiddles
    exp(-2 pi i m / fft_size) as (fft_size / 2, 2) float32, the float32 mel basis (mel_channels, fft_size / 2 + 1) and the
    first / last non-zero bin of every basis row as int32 (an all-zero row: lo = 1, hi = 0)."""
    cfg = preprocess_config
    win_len = int(cfg.get("win_size", cfg["fft_size"]))
    fft_size, n_mels = int(cfg["fft_size"]), int(cfg["mel_channels"])
    basis = mel_basis_slaney(cfg["sample_rate"], fft_size, n_mels, cfg["fmin"], cfg["fmax"], dtype=np.float32)
    nz = basis != 0
    lo = np.where(nz.any(axis=1), nz.argmax(axis=1), 1).astype(np.int32)
    hi = np.where(nz.any(axis=1), basis.shape[1] - 1 - nz[:, ::-1].argmax(axis=1), 0).astype(np.int32)
    ang = -2.0 * np.pi * np.arange(fft_size // 2) / fft_size
    return (hann_symmetric(win_len).astype(np.float32), np.stack((np.cos(ang), np.sin(ang)), axis=1).astype(np.float32),
            basis, lo, hi)


def compute_log_mel_device(sound, preprocess_config, n_samples=None):
    """:func:`compute_log_mel` on the GPU (csrc/mel_analysis.hip through ``mbx_mel_analysis``): sound is a float32 cuda
    tensor (batch, time), ``n_samples`` an optional int32 cuda tensor (batch,) of item lengths.  Returns a cuda tensor
    (batch, time // hop + 1, mel_channels) -- rows of item b beyond ``n_samples[b] // hop + 1`` are not written -- and the
    mel frame rate.  The window and the mel basis are the tables of this module; the transform runs in float32 (the
    host path transforms in float64 and rounds: the two agree to float32 rounding of the magnitudes)."""
    import ctypes
    import torch
    from .abi import _check, load_library
    if sound.dim() != 2 or sound.dtype != torch.float32 or not sound.is_cuda:
        raise ValueError("sound must be a float32 cuda tensor of shape (batch, time)")
    cfg = preprocess_config
    win_len = int(cfg.get("win_size", cfg["fft_size"]))
    hop, fft_size, n_mels = int(cfg["hop_size"]), int(cfg["fft_size"]), int(cfg["mel_channels"])
    dev = sound.device
    tables = [torch.as_tensor(np.ascontiguousarray(tt), device=dev) for tt in mel_analysis_tables(cfg)]
    sound = sound.contiguous()
    B, N = int(sound.shape[0]), int(sound.shape[1])
    frames = N // hop + 1
    out = torch.zeros((B, frames, n_mels), dtype=torch.float32, device=dev)
    if n_samples is not None:
        if n_samples.dtype != torch.int32 or tuple(n_samples.shape) != (B,) or n_samples.device != dev:
            raise ValueError("n_samples must be an int32 tensor of shape (batch,) on the device of sound")
        n_samples = n_samples.contiguous()
    # mbx_mel_analysis has no handle (hence no device of its own): it launches on the CURRENT device, which must be the one
    # the buffers and the stream belong to
    with torch.cuda.device(dev):
        _check(load_library().mbx_mel_analysis(sound.data_ptr(), n_samples.data_ptr() if n_samples is not None else None, B, N,
                                               win_len, hop, fft_size, n_mels, tables[0].data_ptr(), tables[1].data_ptr(),
                                               tables[2].data_ptr(), tables[3].data_ptr(), tables[4].data_ptr(),
                                               ctypes.c_float(float(np.finfo(np.float32).eps)), out.data_ptr(), frames,
                                               torch.cuda.current_stream(dev).cuda_stream))
    return out, cfg["sample_rate"] / hop


def compute_log_mel_device_at(sound, n_samples, centres, n_frames, preprocess_config):
    """:func:`compute_log_mel_at` on the GPU (csrc/mel_warp.hip through ``mbxw_mel_frames_at``, include/mbexwn_warp.h):
    ``sound`` float32 cuda (batch, stride), ``n_samples`` int32 cuda (batch,), ``centres`` int64 cuda (batch, max_frames),
    ``n_frames`` int32 cuda (batch,).  Returns a cuda tensor (batch, max_frames, mel_channels) -- rows of item b from
    ``n_frames[b]`` on are not written (they stay zero) -- and the mel frame rate.  A row carries the bits of the row
    :func:`compute_log_mel_device` computes for a frame with the same samples in front of it."""
    import ctypes
    import torch
    from .abi import _check, load_library
    if sound.dim() != 2 or sound.dtype != torch.float32 or not sound.is_cuda:
        raise ValueError("sound must be a float32 cuda tensor of shape (batch, time)")
    cfg = preprocess_config
    win_len = int(cfg.get("win_size", cfg["fft_size"]))
    fft_size, n_mels = int(cfg["fft_size"]), int(cfg["mel_channels"])
    dev = sound.device
    sound = sound.contiguous()
    B, N = int(sound.shape[0]), int(sound.shape[1])
    for name, tt in (("n_samples", n_samples), ("n_frames", n_frames)):
        if tt.dtype != torch.int32 or tuple(tt.shape) != (B,) or tt.device != dev:
            raise ValueError(f"{name} must be an int32 tensor of shape (batch,) on the device of sound")
    if centres.dtype != torch.int64 or centres.dim() != 2 or int(centres.shape[0]) != B or centres.device != dev:
        raise ValueError("centres must be an int64 tensor of shape (batch, max_frames) on the device of sound")
    n_samples, n_frames, centres = n_samples.contiguous(), n_frames.contiguous(), centres.contiguous()
    frames = int(centres.shape[1])
    tables = [torch.as_tensor(np.ascontiguousarray(tt), device=dev) for tt in mel_analysis_tables(cfg)]
    out = torch.zeros((B, frames, n_mels), dtype=torch.float32, device=dev)
    # no handle, hence no device of its own: the launch goes to the CURRENT device, which must be the buffers' device
    with torch.cuda.device(dev):
        _check(load_library().mbxw_mel_frames_at(sound.data_ptr(), N, B, n_samples.data_ptr(), centres.data_ptr(),
                                                 n_frames.data_ptr(), frames, win_len, fft_size, n_mels, tables[0].data_ptr(),
                                                 tables[1].data_ptr(), tables[2].data_ptr(), tables[3].data_ptr(),
                                                 tables[4].data_ptr(), ctypes.c_float(float(np.finfo(np.float32).eps)),
                                                 out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return out, cfg["sample_rate"] / int(cfg["hop_size"])


def mell_header(preprocess_config):
    """The entries of a ``.mell`` dictionary apart from ``mell`` itself (reference bin/generate_mel.py:41-52)."""
    cfg = preprocess_config
    return {'nfft': cfg["fft_size"],
            'hoplen': cfg["hop_size"],
            'winlen': cfg.get("win_size", cfg["fft_size"]),
            'nmels': cfg["mel_channels"],
            'sr': cfg['sample_rate'],
            'fmin': cfg['fmin'],
            'fmax': cfg['fmax'],
            'lin_spec_offset': cfg['lin_amp_off'],
            'lin_spec_scale': cfg['lin_amp_scale'],
            'log_spec_offset': 0.,
            'log_spec_scale': cfg['mel_amp_scale'],
            "time_axis": 1}


def _add(stats, key, seconds):
    if stats is not None:
        stats[key] = stats.get(key, 0.0) + seconds


def resampled_length(n, rate, target):
    """Samples of an n-sample sound at ``rate`` once it is at ``target``: ceil(n * up / down), as both resamplers give."""
    from math import gcd
    gg = gcd(int(rate), int(target))
    return -(-int(n) * (int(target) // gg) // (int(rate) // gg))


def _plan_mels(sounds, rates, preprocess_config, time_maps, rows_per_frame, f0_out, f0_params, f0_decode, guides, guide_rates,
               align_band_s, align_out, f0_lag=None):
    """What :func:`generate_mels` decides before anything runs, and every refusal of the call: a namespace of the checked
    ``sounds`` and ``rates``, the F0 settings (``track``, ``f0_params`` resolved, ``f0_decode`` checked), ``warped`` {item:
    centres of its time map}, ``guided`` {item: (guide, rate)} with their ``band``, and ``align_out`` / ``failed``."""
    from types import SimpleNamespace
    from . import align, f0decode, f0track, timemap
    cfg = preprocess_config
    target, hop = int(cfg["sample_rate"]), int(cfg["hop_size"])
    sounds = [np.ascontiguousarray(ss, dtype=np.float32) for ss in sounds]
    rates = [int(round(rr)) for rr in rates]
    if len(sounds) != len(rates):
        raise ValueError("generate_mels: one rate per sound")
    for ii, ss in enumerate(sounds):
        if ss.ndim != 1 or ss.size == 0:
            raise ValueError(f"generate_mels: sound {ii} must be a non-empty 1-D array, got shape {ss.shape}")
    if f0_decode is not None:
        if f0_out is None:
            raise ValueError("generate_mels: f0_decode needs f0_out, the list the contours go to")
        f0decode.check_decode(f0_decode)
    if f0_lag is not None:
        if f0_decode is None:
            raise ValueError("generate_mels: f0_lag is the look-ahead of the decoder and needs f0_decode")
        f0_lag = f0decode.check_lag(f0_lag)
    if f0_out is not None:
        f0_params = f0track.check_params(dict(f0_params)) if f0_params is not None else f0track.params(target)
        if int(f0_params["sample_rate"]) != target:
            raise ValueError(f"generate_mels: f0_params are for {f0_params['sample_rate']} Hz, the model rate is {target}")
    maps = timemap.per_item(list(time_maps) if time_maps is not None else None, len(sounds), "generate_mels: time_maps")
    # every map is checked, and its centres are made, before anything runs
    warped = {ii: timemap.centres(resampled_length(sounds[ii].size, rates[ii], target), hop, target, mm, rows_per_frame)
              for ii, mm in enumerate(maps) if mm is not None}
    guided, band = {}, None
    if guides is not None and any(gg is not None for gg in guides):
        if guide_rates is None or len(guides) != len(sounds) or len(guide_rates) != len(sounds):
            raise ValueError("generate_mels: guides and guide_rates take one entry per sound")
        band = align.band_frames(align_band_s, target, hop)
        for ii, gg in enumerate(guides):
            if gg is None:
                continue
            if maps[ii] is not None:
                raise ValueError(f"generate_mels: sound {ii} has a guide and a time map; the guide IS its time map")
            gg = np.ascontiguousarray(gg, dtype=np.float32)
            if gg.ndim != 1 or gg.size == 0:
                raise ValueError(f"generate_mels: guide {ii} must be a non-empty 1-D array, got shape {gg.shape}")
            guided[ii] = (gg, int(round(guide_rates[ii])))
            frames_a = resampled_length(gg.size, guided[ii][1], target) // hop + 1
            align.check_sizes(frames_a, resampled_length(sounds[ii].size, rates[ii], target) // hop + 1, band)
            timemap._check_frames(float(frames_a), rows_per_frame)
    return SimpleNamespace(cfg=cfg, target=target, hop=hop, win_len=int(cfg.get("win_size", cfg["fft_size"])), sounds=sounds,
                           rates=rates, rows_per_frame=rows_per_frame, track=f0_out is not None, f0_params=f0_params,
                           f0_decode=f0_decode, f0_lag=f0_lag, warped=warped, guided=guided, band=band, align_out=align_out, failed=set())


def _aligned_centres(plan, ii, nodes, cost, frames_a, frames_b, n_source):
    """The centres of guided item ``ii`` from its path: its time map in ``plan.warped``, the path's statistics in
    ``plan.align_out``.  No path: ``align.AlignError`` or, where notes are taken, the note, ``plan.failed`` and None."""
    from . import align, timemap
    if len(nodes) == 0:
        err = align.cannot_align(frames_a, frames_b, plan.band)
        if plan.align_out is None:
            raise err
        plan.align_out[ii] = {"error": str(err)}
        plan.failed.add(ii)
        return None
    if plan.align_out is not None:
        plan.align_out[ii] = align.path_stats(nodes, cost, frames_a, frames_b, plan.hop, plan.target)
    plan.warped[ii] = timemap.centres(n_source, plan.hop, plan.target,
                                      timemap.Centres(align.centres_from_path(nodes, plan.hop, n_source)), plan.rows_per_frame)
    return plan.warped[ii]


def _analyse_host(plan, ii, stats):
    """Item ``ii`` in numpy: its mel (frames, mel_channels) and its tracked pair (None unless ``plan.track``); (None, None)
    for a guided item without a path."""
    import time
    from . import align, f0decode, f0track, resample, timemap
    cfg, ss = plan.cfg, plan.sounds[ii]
    t0 = time.perf_counter()
    if plan.rates[ii] != plan.target:
        ss = resample.resample_host(ss, plan.rates[ii], plan.target)
    t1 = time.perf_counter()
    if ii in plan.guided:
        gg, gr = plan.guided[ii]
        if gr != plan.target:
            gg = resample.resample_host(gg, gr, plan.target)
        mel_a = compute_log_mel(gg[np.newaxis], cfg, dtype=np.float32)[0][0]
        mel_b = compute_log_mel(ss[np.newaxis], cfg, dtype=np.float32)[0][0]
        nodes, cost = align.align_host(mel_a, mel_b, plan.band)
        if _aligned_centres(plan, ii, nodes, cost, mel_a.shape[0], mel_b.shape[0], ss.size) is None:
            return None, None
    if ii in plan.warped:
        mel, _ = compute_log_mel_at(ss[np.newaxis], plan.warped[ii], cfg, dtype=np.float32)
    else:
        mel, _ = compute_log_mel(ss[np.newaxis], cfg, dtype=np.float32)
    _add(stats, "resample", t1 - t0)
    _add(stats, "analysis", time.perf_counter() - t1)
    if not plan.track:
        return mel[0], None
    t2 = time.perf_counter()
    cc = plan.warped[ii] if ii in plan.warped else timemap.centres(ss.size, plan.hop, plan.target, None)
    if plan.f0_lag is not None:                             # what a live stream with this lag decides
        tables = f0decode.candidates_host(*f0track.difference_host(ss, cc, plan.f0_params), plan.f0_params, plan.f0_decode)
        pair = f0decode.viterbi_lag_host(*tables, int(plan.f0_params["sample_rate"]), plan.f0_decode, plan.f0_lag)
    elif plan.f0_decode is not None:
        pair = f0decode.track_f0_viterbi_host(ss, cc, plan.f0_params, plan.f0_decode)
    else:
        pair = f0track.track_f0_host(ss, cc, plan.f0_params)
    _add(stats, "f0", time.perf_counter() - t2)
    return mel[0], pair


def _device_batches(sounds, rates, preprocess_config, batch, dev, timed=False, levels=None):
    """The device micro-batches of ``sounds``: grouped by rate, sorted by length (neighbours share a launch: less padding),
    at most ``batch`` items, padded, uploaded, resampled to the model rate and padded to half a window.  Yields (group of
    indices, device sound (B, stride), device lengths int32 (B,), host lengths, marks); ``marks``: None, or with ``timed``
    five timing events, the first three recorded around the upload and the resampler.  ``levels``: None, or a list that
    receives (group, ``level.DeviceMeasure``) of every micro-batch as uploaded, at its own rate, in front of the resampler
    (enqueued only)."""
    import torch
    from . import resample
    cfg = preprocess_config
    target, win_len = int(cfg["sample_rate"]), int(cfg.get("win_size", cfg["fft_size"]))
    by_rate = {}
    for ii, rr in enumerate(rates):
        by_rate.setdefault(rr, []).append(ii)
    for rr, members in by_rate.items():
        members = sorted(members, key=lambda ii: -sounds[ii].size)
        for start in range(0, len(members), max(1, int(batch))):
            group = members[start:start + max(1, int(batch))]
            lengths = [sounds[ii].size for ii in group]
            host = np.zeros((len(group), max(lengths)), dtype=np.float32)
            for bb, ii in enumerate(group):
                host[bb, :lengths[bb]] = sounds[ii]
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if timed else None
            if marks:
                marks[0].record()
            snd = torch.as_tensor(host).to(dev)
            n_dev = torch.as_tensor(np.asarray(lengths, dtype=np.int32)).to(dev)
            if levels is not None:                             # counted with the upload, not with the resampler
                from . import level
                levels.append((group, level.measure_device(snd, lengths, rr)))
            if marks:
                marks[1].record()
            if rr != target:
                _, up, down = resample.device_taps(rr, target, dev)
                snd, n_dev = resample.resample_device(snd, n_dev, rr, target)
                lengths = [-(-nn * up // down) for nn in lengths]
            if snd.shape[1] < win_len // 2 + 1:                # the analysis kernel wants rows of at least half a window
                snd = torch.nn.functional.pad(snd, (0, win_len // 2 + 1 - snd.shape[1]))
            if marks:
                marks[2].record()
            yield group, snd, n_dev, lengths, marks


def _guide_mels_device(plan, batch, dev):
    """{guided item: the regular log-mel of its guide as a device tensor (frames, mel_channels)}: the guides go through the
    micro-batches of the sounds, without the copy back."""
    order = sorted(plan.guided)
    out = {}
    for group, snd, n_dev, lengths, _ in _device_batches([plan.guided[ii][0] for ii in order],
                                                         [plan.guided[ii][1] for ii in order], plan.cfg, batch, dev):
        mel_dev, _ = compute_log_mel_device(snd, plan.cfg, n_samples=n_dev)
        for bb, kk in enumerate(group):
            out[order[kk]] = mel_dev[bb, :lengths[bb] // plan.hop + 1]
    return out


def _align_device(plan, group, snd, n_dev, lengths, guide_mel):
    """The guided items of one micro-batch: its regular analysis, the two alignment kernels on those rows, one copy back
    with the nodes, and the items' centres (:func:`_aligned_centres`)."""
    import torch
    from . import align
    rows = [bb for bb, ii in enumerate(group) if ii in guide_mel]
    if not rows:
        return
    dev = snd.device
    regular, _ = compute_log_mel_device(snd, plan.cfg, n_samples=n_dev)
    n_a = [int(guide_mel[group[bb]].shape[0]) for bb in rows]
    n_b = [lengths[bb] // plan.hop + 1 for bb in rows]
    mel_a = torch.zeros((len(rows), max(n_a), regular.shape[2]), dtype=torch.float32, device=dev)
    for kk, bb in enumerate(rows):
        mel_a[kk, :n_a[kk]] = guide_mel[group[bb]]
    mel_b = regular[rows, :max(n_b)].contiguous()
    found = align.align_device(mel_a, torch.as_tensor(np.asarray(n_a, dtype=np.int32)).to(dev), mel_b,
                               torch.as_tensor(np.asarray(n_b, dtype=np.int32)).to(dev), plan.band)
    packed = torch.cat([found[0], found[1], found[2][:, None], found[3][:, None]], dim=1).cpu().numpy()
    for kk, bb in enumerate(rows):
        count = int(packed[kk, -2])
        nodes = np.stack((packed[kk, :count], packed[kk, max(n_a):max(n_a) + count]), axis=1)
        _aligned_centres(plan, group[bb], nodes, int(packed[kk, -1]), n_a[kk], n_b[kk], lengths[bb])


def _analyse_device(plan, micro_batch, guide_mel, stats):
    """One micro-batch of :func:`_device_batches` on the device: per item of its group the mel (frames, mel_channels) and
    the tracked pair (None unless ``plan.track``), after one copy back.  ``stats`` costs the one wait."""
    import time
    import torch
    from . import f0decode, f0track, timemap
    group, snd, n_dev, lengths, marks = micro_batch
    cfg, dev = plan.cfg, snd.device
    _align_device(plan, group, snd, n_dev, lengths, guide_mel)
    warped = any(ii in plan.warped for ii in group)
    if warped or plan.track:
        cents = [plan.warped[ii] if ii in plan.warped else timemap.centres(nn, plan.hop, plan.target, None)
                 for ii, nn in zip(group, lengths)]
        table = np.zeros((len(group), max(cc.size for cc in cents)), dtype=np.int64)
        for bb, cc in enumerate(cents):
            table[bb, :cc.size] = cc
        counts = [int(cc.size) for cc in cents]
        table_dev = torch.as_tensor(table).to(dev)
        counts_dev = torch.as_tensor(np.asarray(counts, dtype=np.int32)).to(dev)
    if warped:
        mel_dev, _ = compute_log_mel_device_at(snd, n_dev, table_dev, counts_dev, cfg)
    else:
        counts = [nn // plan.hop + 1 for nn in lengths]
        mel_dev, _ = compute_log_mel_device(snd, cfg, n_samples=n_dev)
    last = 3
    if marks:
        marks[3].record()
    if plan.track:                                          # the regular centres are t * hop: the analysis's own frames
        if plan.f0_lag is not None:
            tables = f0decode.candidates_device(snd, n_dev, table_dev, counts_dev, plan.f0_params, plan.f0_decode)
            f0_dev, per_dev = f0decode.decode_lag_device(*tables, counts_dev, int(plan.f0_params["sample_rate"]), plan.f0_decode,
                                                         plan.f0_lag)
        elif plan.f0_decode is not None:
            f0_dev, per_dev = f0decode.track_f0_viterbi_device(snd, n_dev, table_dev, counts_dev, plan.f0_params, plan.f0_decode)
        else:
            f0_dev, per_dev = f0track.track_f0_device(snd, n_dev, table_dev, counts_dev, plan.f0_params)
        last = 4
        if marks:
            marks[4].record()
    if marks:
        marks[last].synchronize()
        t0 = time.perf_counter()
    mel = mel_dev.cpu().numpy()
    pairs = [None] * len(group)
    if plan.track:
        f0_host, per_host = f0_dev.cpu().numpy(), per_dev.cpu().numpy()
        pairs = [(f0_host[bb, :counts[bb]].copy(), per_host[bb, :counts[bb]].copy()) for bb in range(len(group))]
    if marks:
        _add(stats, "copy_back", time.perf_counter() - t0)
        for key, first in (("f0", 3), ("upload", 0), ("resample", 1), ("analysis", 2))[4 - last:]:
            _add(stats, key, marks[first].elapsed_time(marks[first + 1]) * 1e-3)
    return [(mel[bb, :counts[bb]], pairs[bb]) for bb in range(len(group))]


def generate_mels(sounds, rates, preprocess_config, on_device=True, batch=16, stats=None, time_maps=None, rows_per_frame=1,
                  f0_out=None, f0_params=None, f0_decode=None, guides=None, guide_rates=None, align_band_s=1.0,
                  align_out=None, levels_out=None, f0_lag=None):
    """Sounds -> ``.mell`` dictionaries (reference bin/generate_mel.py:54-64 for a list of files): ``sounds`` is a list of 1-D
    float32 arrays, ``rates`` their sample rates.  A sound that is not at the model rate goes through the reference's resampler
    (resample.py); one already at it skips that step.  Needs the ``preprocess_config`` alone: no engine, no weights.

    ``on_device``: the items are grouped by rate and run in padded micro-batches of at most ``batch`` items through
    ``resample_device`` straight into ``compute_log_mel_device`` (the lengths stay on the device), with one copy back per
    micro-batch; an item's bits do not depend on the batch it ran in.  Otherwise numpy, one item at a time (``resample_host``,
    ``compute_log_mel``).  ``stats``: a dict that collects seconds per step (resample, analysis, upload, copy_back); on the
    device that costs one wait per micro-batch.

    ``time_maps``: per sound None, a factor or a breakpoint array (timemap.py): the item's frames lie
    on ``timemap.centres`` of its length at the model rate (``resampled_length``, which the host knows), K of them, and the
    ``.mell`` has K columns.  A micro-batch with such an item goes through ``compute_log_mel_device_at`` (on the host:
    ``compute_log_mel_at``), its other items on their regular centres, which gives them the regular analysis's bits; a
    call without maps makes the launches it made before there were any.  ``rows_per_frame``: ``timemap.centres``' limit.

    ``f0_out``: a list, or None.  Given a list, item i's ``(f0, periodicity)`` -- float32 arrays with one value per column
    of its ``.mell``, f0 in Hz and 0 where unvoiced -- is appended to it, in the order of ``sounds``: the F0 tracker
    (f0track.py) on the item's model-rate samples at the centres of its mel frames, warped or regular
    (on the device ``mbxp_track_f0`` behind the analysis of the micro-batch, else ``f0track.track_f0_host``: the same
    bits).  ``f0_params``: ``f0track.params`` of the model rate (default: its defaults).  None makes today's launches;
    the dictionaries have the same keys either way.

    ``f0_decode``: None, or a ``f0decode.decode_params`` dictionary.  Given one, every item's pair is
    the decoded one: Viterbi over the YIN candidates of all its frames instead of the pick of every frame on its own (on
    the device ``mbxc_f0_candidates`` and ``mbxc_decode_f0`` in place of ``mbxp_track_f0``, else
    ``f0decode.track_f0_viterbi_host``: the same bits).  It needs ``f0_out``.  None makes exactly the launches of before.
    ``f0_lag``: None, or a number of frames 0 .. 128: the decoder decides frame t from the frames up
    to t + lag only, as a live stream opened with that lag does -- a file then has the stream's contour (on the device
    ``mbxv_decode_f0_frames`` in place of ``mbxc_decode_f0``, else ``f0decode.viterbi_lag_host``).  It needs ``f0_decode``.

    ``guides``: None, or per sound None or a 1-D float32 array at ``guide_rates[i]``: the item takes the TIMING of its guide
    (align.py).  Guide and source go through the resampler and the regular analysis; the band costs
    and the DTW path of ``align_band_s`` seconds around the diagonal follow (on the device ``mbxg_local_cost`` and
    ``mbxg_align_path`` on the micro-batch, one small copy bringing the nodes back; else ``align.align_host``: the same
    bits given the same mels); ``align.centres_from_path`` makes the centres, which then are the item's time map
    (``timemap.Centres``): its ``.mell`` has the guide's frame count.  A guided item takes no ``time_maps`` entry.  An item
    without a guide keeps its regular bits; a call without guides makes the launches of before.  ``align_out``: a dict, or
    None.  Given a dict, item i's ``align.path_stats`` go to ``align_out[i]``, and an item that cannot be aligned
    (``align.AlignError``) leaves ``{"error": message}`` there and None in the result (and in ``f0_out``) instead of raising.

    ``levels_out``: a list, or None.  Given a list, (P, count) of every sound -- its BS.1770 power and the number of gated
    blocks behind it, 0 for a sound that is not measurable (level.py) -- is appended to it in the order
    of ``sounds``: the sound as handed in, at its own rate, measured on the device in the micro-batch that uploads it (else
    ``level.measure_host``: the same bits).  None makes exactly the launches of before."""
    plan = _plan_mels(sounds, rates, preprocess_config, time_maps, rows_per_frame, f0_out, f0_params, f0_decode, guides,
                      guide_rates, align_band_s, align_out, f0_lag)
    results = [(None, None)] * len(plan.sounds)
    measured = [] if levels_out is not None else None
    if not on_device:
        results = [_analyse_host(plan, ii, stats) for ii in range(len(plan.sounds))]
        if measured is not None:
            from . import level
            found = [level.measure_host(ss, rr) for ss, rr in zip(plan.sounds, plan.rates)]
            levels_out.extend((mm.power, mm.count) for mm in found)
    else:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("generate_mels(on_device=True): no GPU available (on_device=False is the host path)")
        dev = torch.device("cuda", torch.cuda.current_device())
        guide_mel = _guide_mels_device(plan, batch, dev) if plan.guided else {}
        for micro_batch in _device_batches(plan.sounds, plan.rates, plan.cfg, batch, dev, timed=stats is not None,
                                           levels=measured):
            for ii, result in zip(micro_batch[0], _analyse_device(plan, micro_batch, guide_mel, stats)):
                results[ii] = result
        if measured is not None:
            powers = [None] * len(plan.sounds)
            for group, measure in measured:
                for ii, mm in zip(group, measure.host(details=False)):
                    powers[ii] = (mm.power, mm.count)
            levels_out.extend(powers)
    for ii in plan.failed:
        results[ii] = (None, None)
    if f0_out is not None:
        f0_out.extend(pair for _, pair in results)
    return [None if mel is None else dict(mell_header(plan.cfg), mell=np.ascontiguousarray(mel.T)) for mel, _ in results]

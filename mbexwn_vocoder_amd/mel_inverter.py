"""``MELInverter``: the reference's inference object, backed by the MI355X HIP engine.

Mirrors reference MBExWN_NVoc/mel_inverter.py:21-239 (same constructor, attributes, methods and error
behaviour).  What differs is what ``self.model`` is: an ``MBExWNEngine`` (HIP kernels behind the C ABI of
include/mbexwn.h) instead of a Keras model on TensorFlow.
"""
import os
import sys
from typing import Dict, Union

import numpy as np
from scipy.interpolate import interp1d

log_to_db = 20 * np.log10(np.exp(1))   # reference vocoder/model/preprocess.py:78


class MELInverter(object):
    def __init__(self, model_id_or_path: Union[str, None] = None, verbose: bool = False, calibrate: bool = False,
                 batch_invariant: Union[bool, None] = None, conv_form: Union[str, None] = None):
        """As the reference's constructor (mel_inverter.py:22-41); ``calibrate``, ``batch_invariant`` and ``conv_form`` (this
        build) are handed to :meth:`load_model`."""
        self.model = None
        self._calibrate_pending = False
        self._verbose = verbose
        self.model_id_or_path = model_id_or_path
        self.config_file = None
        self.preprocess_config = None
        self.mel_channels = None
        self.hop_size = None
        self.fft_size = None
        self.fmin = None
        self.fmax = None
        self._srate = None
        self.win_len = None

        self.lin_amp_scale = 1
        self.lin_amp_off = 1.e-5
        self.mel_amp_scale = 1
        self.use_max_limit = False

        if model_id_or_path:
            self.load_model(model_id_or_path=model_id_or_path, verbose=verbose, calibrate=calibrate,
                            batch_invariant=batch_invariant, conv_form=conv_form)

    @classmethod
    def host_only(cls, model_id_or_path):
        """An instance with a model's pre-processing parameters and no engine: :meth:`scale_mel` in a process that must not
        initialise HIP (the parent of a multi-GPU job, batched.plan_ranks)."""
        from . import get_config_file
        from .config import read_config
        inv = cls()
        inv.model_id_or_path = model_id_or_path
        inv.config_file = get_config_file(model_id_or_path=model_id_or_path)
        inv._set_preprocess_config(read_config(config_file=inv.config_file)["preprocess_config"])
        return inv

    @property
    def srate(self):
        return self._srate

    # ------------------------------------------------------------------------------------------
    def scale_mel(self, mel_config: Dict, verbose=False):
        """Convert the content of a ``.mell`` dictionary into the (1, T, mel_channels) float32 log-mel
        conditioning of the model (reference mel_inverter.py:48-148; host side, numpy).

        Arithmetic is carried out in the dtype of the stored spectrogram, in the reference's order, so the
        result is bit-identical to the reference's (tests/golden/reference_scale_mel.npz).  Unlike the
        reference the caller's array is not modified in place.
        """
        hop_ratio = (mel_config['hoplen'] / mel_config['sr']) / (self.hop_size / self.srate)
        resample_hop = np.abs(hop_ratio - 1) > 0.001
        if resample_hop and verbose:
            print(f"compensate change in analysis hop size. mel analysis has {mel_config['hoplen'] / mel_config['sr']}"
                  f" while the model expects {self.hop_size / self.srate}.", file=sys.stderr)
        if mel_config['sr'] != self.srate and verbose:
            print(f"    WARNING::sample rate of mel analysis is  {mel_config['sr']} model expects {self.srate}.",
                  file=sys.stderr)

        if mel_config['fmin'] != self.fmin:
            raise RuntimeError(f"mell fmin {mel_config['fmin']} does not match model fmin {self.fmin}")
        if ((mel_config['fmax'] is None) and self.fmax != mel_config['sr'] / 2) \
                or ((mel_config['fmax'] is not None) and mel_config['fmax'] != self.fmax):
            raise RuntimeError(f"mell fmax {mel_config['fmax']} does not match model fmax {self.fmax}")

        if "mell" in mel_config:
            log_mel = np.array(mel_config['mell'].T[np.newaxis])
            if mel_config.get("log_spec_offset", 0) != 0:
                log_mel -= mel_config["log_spec_offset"]
            if mel_config.get("log_spec_scale", 1) != 1:
                log_mel /= mel_config["log_spec_scale"]
            mel = np.exp(log_mel)
        elif "mel" in mel_config:
            mel = np.array(mel_config['mel'].T[np.newaxis])
        else:
            raise RuntimeError("error::no supported mel spectrum (keys:mell or mel) in the mel dictionary")

        n_fft = mel_config.get("nfft", None)
        if n_fft is None:
            n_fft = mel_config.get("n_fft", None)
        if n_fft is None:
            n_fft = mel_config.get("fft_size", None)
        fft_scale_factor = self.fft_size // n_fft
        if fft_scale_factor != 1:
            mel *= fft_scale_factor
        if mel_config.get("lin_spec_offset", None) is not None and mel_config["lin_spec_offset"] != 0:
            mel -= mel_config["lin_spec_offset"]
        if mel_config.get("lin_spec_scale", 1) != 1:
            mel /= mel_config["lin_spec_scale"]
        if self.lin_amp_scale != 1:
            mel *= self.lin_amp_scale

        if self.use_max_limit:
            mell = np.log(np.fmax(mel, self.lin_amp_off)).astype(np.float32)
        else:
            mell = np.log(mel + self.lin_amp_off).astype(np.float32)

        if verbose:
            # diagnostics only (the reference prints comparable statistics at mel_inverter.py:110-116)
            db = log_to_db * mell
            print(f"    scaled log-mel {mell.shape}: level in dB -- min {db.min():.3f}, median {np.median(db):.3f}, "
                  f"mean {db.mean():.3f}, max {db.max():.3f}", file=sys.stderr)
            print(f"    analysis of the input mel: sample rate {mel_config['sr']}, hop {mel_config['hoplen']}, "
                  f"window {mel_config.get('winlen')}, FFT {n_fft}", file=sys.stderr)

        if resample_hop:
            # same expression order as the reference (mel_inverter.py:133-146): the grids decide the rounding
            mell = interp1d(np.arange(mell.shape[1]) * mel_config['hoplen'] / mel_config['sr'], mell, axis=1,
                            bounds_error=False, fill_value="extrapolate")(
                np.arange(0, (mell.shape[1] - 1 + 0.1) * mel_config['hoplen'] / mel_config['sr'],
                          self.hop_size / self.srate)).astype(np.float32)

        return mell * self.mel_amp_scale

    # ------------------------------------------------------------------------------------------
    def _output_rate(self, out_rate):
        """``out_rate`` as an int, or None when it is the model's rate (or None): today's path, launch for launch."""
        if out_rate is None:
            return None
        from .resample import positive_rate
        rate = positive_rate(out_rate, "out_rate")
        return None if rate == int(round(self.srate)) else rate

    def _to_rate(self, audio, out_rate):
        """Device audio (B, N) at the model rate -> (B, ceil(N * up / down)) at ``out_rate`` (resample.resample_device)."""
        from .resample import resample_device
        return resample_device(audio.contiguous(), None, int(round(self.srate)), out_rate)[0]

    def _keyed_noise(self, noise, noise_seed, keys, frames):
        """The keyed draw of items of ``frames`` frames (engine.keyed_noise: a function of the seed, the item's key and the
        step alone), or None for a model without noise channel; ``noise`` together with ``noise_seed`` is refused."""
        if noise is not None:
            raise ValueError("noise= and noise_seed= exclude each other: the keyed draw replaces the injected one")
        dims = self.model.dims
        if not dims.noise_sigma:
            return None
        return self.model.keyed_noise(int(noise_seed), keys, [int(tt) * dims.wn_in_rows_per_frame for tt in frames])

    def synth_from_mel(self, scaled_mell, noise=None, f0=None, transposition=None, out_rate=None, noise_seed=None,
                       noise_key=0, formant=None):
        """(1, T, mel_channels) log-mel -> float32 audio of T*hop_size samples
        (reference mel_inverter.py:151-154; like there, a batch is flattened by ``ravel``).

        ``noise`` optionally injects the N(0,1) draw of the noise channel (shape (B, T*steps_per_frame));
        by default it is drawn on the device, as the reference draws tf.random.normal.

        Pitch control (this build): ``f0`` -- (T,) or (B, T) Hz, one value per mel frame, replaces the F0-net's contour;
        ``transposition`` -- a factor on the contour, a scalar (the ``transposition_factor`` of ``infer_components``, same
        bits) or one value per mel frame.  Per-frame values are brought to the pulse rate by the model's linear
        interpolator (``mbx_forward_options.f0_frames / f0_scale``); they must be finite and positive.

        ``out_rate`` (this build): the audio comes back at that rate, ceil(T * hop_size * up / down) samples --
        ``resample.resample_device`` (the reference's resampler, model rate -> ``out_rate``) on the device audio before it
        is copied back.  None or the model's rate: the audio as the model makes it.

        ``noise_seed`` (this build): the noise channel takes the keyed draw of the item ``noise_key`` (an integer, e.g.
        ``noise.item_key(file name)``; one per row of a batch, or one for all) under that seed -- ``engine.keyed_noise``,
        handed to the forward as ``noise`` is.  The audio is then a function of (mel, seed, key) and does not depend on what
        was synthesised before.  Not together with ``noise``.

        ``formant`` (this build): a formant shift -- one factor or one per mel frame, finite and positive
        (:func:`check_factors`), > 1 moves the formants up.  The spectral envelope of every frame is read at ``f / factor``
        (``envelope.warp_envelope_host`` is the definition) by the VTF-net and the WaveNet conditioning,
        while the F0-net reads the mel as it is: pitch and timing stay.  The level is not compensated.  It combines freely
        with ``f0`` / ``transposition``."""
        out_rate = self._output_rate(out_rate)
        if noise_seed is not None:
            shape = np.shape(scaled_mell)
            keys = [int(kk) for kk in np.broadcast_to(np.asarray(noise_key, dtype=object), (int(shape[0]),))]
            noise = self._keyed_noise(noise, noise_seed, keys, [int(shape[1])] * int(shape[0]))
        self._calibrate_if_pending(scaled_mell)
        if formant is not None:
            formant = np.asarray(check_factors(formant, int(np.shape(scaled_mell)[1]), "formant"), dtype=np.float32)
        if f0 is not None or transposition is not None or formant is not None:
            return self._synth_with_pitch(scaled_mell, noise, f0, transposition, out_rate, formant)
        syn_audio = self.model.infer(scaled_mell, sigma=None, synth_length=scaled_mell.shape[1] * self.hop_size,
                                     noise=noise)
        if out_rate is not None:
            return self._to_rate(syn_audio.tensor, out_rate).cpu().numpy().ravel()
        return syn_audio.numpy().ravel()

    def _synth_with_pitch(self, scaled_mell, noise, f0, transposition, out_rate=None, formant=None):
        import torch
        model = self.model
        n_frames = int(scaled_mell.shape[1])
        mel, noise = model._prepare(scaled_mell, n_frames * self.hop_size, noise)
        B, T = int(mel.shape[0]), int(mel.shape[1])

        def rows(values, name):
            values = np.asarray(values, dtype=np.float32)
            if not (np.all(np.isfinite(values)) and np.all(values > 0)):
                raise ValueError(f"{name} must be finite and positive")
            if values.ndim == 0:
                return values
            values = values.reshape(-1, values.shape[-1])
            if values.shape[1] != T or values.shape[0] not in (1, B):
                raise ValueError(f"{name} must hold one value per mel frame ({T})")
            return torch.as_tensor(np.array(np.broadcast_to(values, (B, T))), device=model.device)

        f0_rows = None if f0 is None else rows(f0, "f0")
        if f0_rows is not None and not torch.is_tensor(f0_rows):
            raise ValueError(f"f0 must hold one value per mel frame ({T})")
        scale = None if transposition is None else rows(transposition, "transposition")
        # (a mel shorter than the synthesis was continued by one frame in _prepare: that frame repeats the last factor)
        shift = None if formant is None else rows(np.concatenate((formant, formant[-1:]))[:T], "formant")
        if scale is None or torch.is_tensor(scale):
            audio = model.forward(mel, noise=noise, f0_frames=f0_rows, f0_scale=scale, formant=shift)
        elif f0_rows is None:                                # a scalar: the whole-item option, as infer_components applies it
            audio = model.forward(mel, noise=noise, transposition=float(scale), formant=shift)
        else:
            audio = model.forward(mel, noise=noise, f0_frames=f0_rows, formant=shift,
                                  f0_scale=torch.full((B, T), float(scale), dtype=torch.float32, device=model.device))
        if out_rate is not None:
            return self._to_rate(audio[:, :n_frames * self.hop_size], out_rate).cpu().numpy().ravel()
        return audio[:, :n_frames * self.hop_size].cpu().numpy().ravel()

    def _calibrate_if_pending(self, scaled_mell):
        if self._calibrate_pending:
            # load_model(..., calibrate=True): the FIRST mel synthesised decides the form for every later call (at most 400 of
            # its frames are used) -- results therefore depend on which utterance came first; calibrate([...]) on a fixed set
            # (resynth_mel.py --calibrate N) is the reproducible way.  A calibration that cannot run (e.g. a form pinned by the
            # configuration) must not fail the synthesis: keep the creation-time form and say so.
            self._calibrate_pending = False
            try:
                self.calibrate([scaled_mell], verbose=self._verbose)
            except Exception as exc:                # noqa: BLE001 -- any engine error: the form of mbx_create stays
                import warnings
                warnings.warn(f"MELInverter: calibration on the first mel failed ({exc}); keeping the convolution form "
                              f"chosen at creation ({self.model.conv_form_info()['form']})", RuntimeWarning)

    def synth_from_mels(self, scaled_mels, noises=None, max_batch=16, max_padded_frames=16 * 1200, flac=False,
                        flac_compression="verbatim", out_rate=None, noise_seed=None, noise_keys=None, transpositions=None,
                        formants=None, f0s=None, loudness=None, peak_limit=None, true_peak=False, levels_out=None,
                        limiter=False, lookahead_ms=None, hold_ms=None):
        """Batched :meth:`synth_from_mel` (this build): a list of ``scale_mel`` outputs (1, T_i, mel_channels) -> a list of
        float32 audio (T_i * hop_size,), or with ``flac=True`` of complete FLAC files (bytes; frames encoded on the device).

        The mels run in padded micro-batches (sharding.plan_batches, at most ``max_batch`` items and ``max_padded_frames``
        padded frames each) through the engine's forward with per-item lengths.  ``noises``: per-item N(0,1) draws
        (T_i * wn_in_rows_per_frame,), default: the draws :meth:`synth_from_mel` would make called on the list one by one
        (batched.replay_noise) -- with a ``batch_invariant`` engine the results are then bit-identical to those calls.

        ``out_rate``: every item comes back at that rate (audio, or FLAC files whose header, frames and MD5 are at that
        rate and length): the micro-batch is resampled on the device (``resample.resample_device`` with the items' own
        lengths, so each tail is clipped at its item's end), and item b equals ``resample_device`` of its own model-rate
        audio alone.  None or the model's rate: today's path.

        ``noise_seed``: item i takes the keyed draw of ``noise_keys[i]`` (default: its index) under that seed, as
        :meth:`synth_from_mel` with ``noise_seed`` / ``noise_key`` does -- nothing is replayed, and an item's draw does not
        depend on the list it is in.  Not together with ``noises``.  ``transpositions``: per item None, or (T_i,) factors,
        one per mel frame (``f0_scale`` rows of the forward).  ``formants``: per item None, one formant-shift factor, or
        (T_i,) of them (:meth:`synth_from_mel` ``formant``; the ``formant`` rows of the forward).  ``f0s``: per item None, or
        (T_i,) Hz, one value per mel frame, positive and finite, in place of the F0-net's contour (:meth:`synth_from_mel`
        ``f0``; the ``f0_frames`` rows of the forward) -- an item with None keeps the F0-net (``f0_item_mask``), the
        transposition multiplies on top, and a wrong length or value is refused before anything runs.

        Level (level.py): ``loudness`` -- None, a BS.1770 integrated loudness in LUFS every item comes
        out at, or a list with, per item, a target POWER (``level.target_power``, or the P of another measurement) or None;
        ``peak_limit`` -- a ceiling in dBFS on the item's peak (default: -1 with a loudness, else none; alone it only ever
        scales down); ``true_peak`` -- the ceiling is about the 4x oversampled peak.  One static gain per item, measured and
        applied on the device behind the forward and the output resampler: what comes back -- audio or FLAC -- is the
        gained audio, measured at the rate it has.  ``levels_out``: a list that receives ``SynthBatch.level`` of every item,
        in item order.  None of them: the launches of before.

        ``limiter`` (limiter.py): the ceiling -- -1 dBFS unless ``peak_limit`` says otherwise, with or
        without a loudness -- is kept by a look-ahead peak limiter in place of the static gain, so the loudness gain stands;
        ``lookahead_ms`` and ``hold_ms`` shape its window (None: 1.5 and 20 ms).  The report then carries the loudness and the peak measured
        behind the limiter and a ``limiter`` entry (``SynthBatch.level``).  False: the launches and the bytes of before."""
        import torch
        from .batched import check_f0s, replay_noise, run_micro_batches
        from .level import level_control
        control = level_control(loudness, peak_limit, true_peak, limiter, lookahead_ms, hold_ms)
        if control is not None:
            control.check_rates([self.srate if out_rate is None else out_rate])   # a window the rate refuses: before anything runs
        if control is not None and isinstance(control.target, list) and len(control.target) != len(scaled_mels):
            raise ValueError("synth_from_mels: a loudness list takes one entry per mel")
        if noise_seed is not None and noises is not None:
            raise ValueError("noises= and noise_seed= exclude each other: the keyed draw replaces the injected one")
        if noise_seed is None and noise_keys is not None:
            raise ValueError("synth_from_mels: noise_keys needs noise_seed")
        out_rate = self._output_rate(out_rate)
        rate = self.srate if out_rate is None else out_rate
        if len(scaled_mels):
            self._calibrate_if_pending(scaled_mels[0])
        mels =[np.asarray(mm, dtype=np.float32).reshape(-1, mm.shape[-2], mm.shape[-1])[0] for mm in scaled_mels]
        f0s = check_f0s(f0s, [int(mm.shape[0]) for mm in mels])
        if formants is not None:
            if len(formants) != len(mels):
                raise ValueError("synth_from_mels: one formants entry per mel")
            formants = [None if ff is None else np.asarray(check_factors(ff, int(mm.shape[0]), "formant"), dtype=np.float32)
                        for ff, mm in zip(formants, mels)]
        dims = self.model.dims
        if noise_seed is not None:
            keys = list(range(len(mels))) if noise_keys is None else [int(kk) for kk in noise_keys]
            if len(keys) != len(mels):
                raise ValueError("synth_from_mels: one noise key per mel")
            noises = None if not dims.noise_sigma else KeyedNoise(int(noise_seed), keys)
        elif not dims.noise_sigma:
            noises = None
        elif noises is None:
            noises = replay_noise([mm.shape[0] for mm in mels], dims.wn_in_rows_per_frame, device=self.model.device)
        else:
            noises = [torch.as_tensor(np.asarray(zz) if not torch.is_tensor(zz) else zz).to(self.model.device, torch.float32)
                      .reshape(-1) for zz in noises]
        out, reports = [None] * len(mels), [None] * len(mels)
        for batch in run_micro_batches(self.model, mels, noises, max_batch, max_padded_frames, flac=flac, host_audio=not flac,
                                       flac_compression=flac_compression, out_rate=out_rate, transpositions=transpositions,
                                       formants=formants, f0s=f0s, level=control):
            batch.wait()
            for jj, ii in enumerate(batch.indices):
                reports[ii] = batch.level(jj)
                if not flac:
                    out[ii] = batch.audio(jj)
                elif np.isfinite(batch.flac.max_abs[jj]):
                    out[ii] = batch.flac.stream(jj)
                else:
                    from . import flac as flac_writer
                    out[ii] = flac_writer.encode(batch.audio(jj), rate, flac_compression)
        if levels_out is not None:
            levels_out.extend(reports)
        return out

    def measure_loudness(self, snd, srate, true_peak=False):
        """The BS.1770 measure of a single sound at ``srate`` (this build; level.py), on the device: a
        ``level.Measure`` -- ``lufs`` (-inf when ``count`` is 0: under 0.4 s, or silent), ``power``, ``sample_peak`` and,
        asked for, the 4x ``true_peak``.  ``level.measure_host`` is its definition."""
        import torch
        from . import level
        snd = np.ascontiguousarray(np.asarray(snd).reshape(-1), dtype=np.float32)
        audio = torch.as_tensor(snd[np.newaxis]).to(self.model.device)
        return level.measure_device(audio, [snd.size], int(round(srate)), true_peak).host()[0]

    def transform_audio(self, sounds, rates, names, transposition=1.0, noise_seed=0, out_rate=None, max_batch=16,
                        max_padded_frames=16 * 1200, flac=False, flac_compression="verbatim", time_stretch=None, formant=None,
                        f0_source="net", f0_params=None, f0_decode=None, f0_fill="interpolate", f0_initial=150.0,
                        align_to=None, align_band_s=1.0, loudness=None, peak_limit=None, true_peak=False, levels_out=None,
                        *, limiter=False, lookahead_ms=None, hold_ms=None, f0_lag=None):
        """Sounds in, transposed sounds out (this build): ``sounds`` -- 1-D float32 arrays at ``rates``; ``names`` -- what
        keys each item's noise (``noise.item_key``: the basename of a file name, or an integer); ``transposition`` -- one
        factor for all, or one per item.  Device resampler and mel analysis (``analysis.generate_mels``), :meth:`scale_mel`
        on the host, then :meth:`synth_from_mels` with the keyed noise of ``noise_seed``, the factor on every frame, and
        ``out_rate`` / ``flac`` as there.  Item i has ``frames_i * hop_size`` samples at the model rate before the output
        resampler (frames_i = resampled length // hop_size + 1), as a live stream of it emits: not trimmed to its input.

        ``time_stretch``: a change of duration at the same pitch (timemap.py) -- None, one factor or
        one breakpoint array for all items, or a list with one of these per item.  The analysis then places item i's frames
        on ``timemap.centres`` of its resampled length, K_i of them, and the item has ``K_i * hop_size`` samples at the model
        rate before the output resampler; the transposition rows, the keyed noise (counted by output step), ``out_rate``
        and ``flac`` work on those frames as on any others.

        ``formant``: a formant shift at the same pitch and duration -- None, or a list with one entry
        per item, each a factor or one factor per mel frame of the item (:meth:`synth_from_mels` ``formants``).  It combines
        freely with ``transposition`` and ``time_stretch``.

        ``f0_source``: ``"net"`` -- the pitch the model infers from the mel, as before -- or ``"audio"``: the pitch that is in
        the sound.  The F0 tracker (f0track.py; ``f0_params``: keywords of ``f0track.params``) runs on
        the model-rate samples at the centres of the item's mel frames, warped ones included, its unvoiced frames are filled
        (``f0track.fill_unvoiced``) and the contour replaces the F0-net's (:meth:`synth_from_mels` ``f0s``); the transposition
        multiplies on top.  An item without a voiced frame keeps the F0-net.  ``f0_decode``: None -- every frame's pick on its
        own -- or a ``f0decode.decode_params`` dictionary: the contour is the Viterbi path over the YIN candidates of the
        item's frames, which does not jump an octave for single frames.  It needs ``"audio"``.
        ``f0_lag``: None -- the path over the whole item -- or the fixed lag in frames, 0 .. 128, of a live stream's decoder
        (DESIGN.md section 6l): frame t is decided from the frames up to t + lag.  It needs ``f0_decode``, and with
        ``f0_fill="hold"`` the run has the bits of ``LiveResynthesizer.open(f0_source="audio", f0_decode=..., f0_lag=...)``.
        ``f0_fill``: ``"interpolate"`` -- the fill described above -- or ``"hold"``, the causal fill of the live streams
        (``f0track.fill_hold``): an unvoiced frame holds the last voiced value, the frames in front of
        the first voiced one take ``f0_initial`` Hz, and every item takes its contour.  It needs ``"audio"`` and exists so that
        an offline run has the bits of ``LiveResynthesizer.open(f0_source="audio")``.

        ``align_to``: None, or a list with, per item, None or a ``(guide, rate)`` pair -- a 1-D float32 recording whose TIMING
        the item takes (align.py; the ``guides`` of ``analysis.generate_mels`` and of
        ``batched.run_audio_job``): the mel frames of guide and item are aligned by dynamic time warping within
        ``align_band_s`` seconds of the diagonal, and the item comes out with the guide's frame count.  Such an item takes no
        ``time_stretch``; one that cannot be aligned raises ``align.AlignError``.  Everything else works on its frames as on
        any others.

        ``loudness`` / ``peak_limit`` / ``true_peak`` / ``levels_out``: the level of what comes back, as in
        :meth:`synth_from_mels` -- and ``loudness="input"``: every item comes out at the loudness of its source, which is
        measured as handed in, at its own rate, on the device in the micro-batches the analysis stages; a source that is not
        measurable leaves the loudness gain at 1 (the ceiling still applies).  ``limiter`` / ``lookahead_ms`` / ``hold_ms``:
        the look-ahead limiter of :meth:`synth_from_mels`.

        An item's audio is a function of (sound, rate, name, factor, stretch, formant, seed, out_rate): with a ``batch_invariant``
        engine or one pinned to a convolution form it does not depend on the batch, the order or the other items."""
        from . import align, timemap
        from .batched import analyse_for_synthesis
        from .level import check_options
        from .noise import item_key
        factors = check_factors(transposition, len(sounds))
        if not (len(sounds) == len(rates) == len(names)):
            raise ValueError("transform_audio: one rate and one name per sound")
        if formant is not None and (not isinstance(formant, (list, tuple)) or len(formant) != len(sounds)):
            raise ValueError("transform_audio: formant takes one entry per sound")
        loudness, peak_limit, true_peak = check_options(loudness, peak_limit, true_peak, allow_input=True, limiter=limiter,
                                                        lookahead_ms=lookahead_ms, hold_ms=hold_ms)   # before anything runs
        guided = align_to is not None and any(gg is not None for gg in align_to)
        if guided and len(align_to) != len(sounds):
            raise ValueError("transform_audio: align_to takes one entry per sound")
        done = analyse_for_synthesis(self, sounds, rates, time_maps=timemap.per_item(time_stretch, len(sounds), "transform_audio: time_stretch"),
                                     guides=[None if gg is None else gg[0] for gg in align_to] if guided else None,
                                     guide_rates=[None if gg is None else gg[1] for gg in align_to] if guided else None,
                                     align_band_s=align_band_s, f0_source=f0_source, f0_params=f0_params, f0_decode=f0_decode,
                                     f0_fill=f0_fill, f0_initial=f0_initial, batch=max_batch, who="transform_audio",
                                     f0_lag=f0_lag, source_levels=isinstance(loudness, str))
        if isinstance(loudness, str):
            loudness = [power if count else None for power, count in done.levels]
        for ii, mel in enumerate(done.scaled):
            if mel is None:
                raise align.AlignError(done.notes[ii]["error"])
        rows = [np.full(int(mm.shape[1]), ff, dtype=np.float32) for mm, ff in zip(done.scaled, factors)]
        return self.synth_from_mels(done.scaled, max_batch=max_batch, max_padded_frames=max_padded_frames, flac=flac,
                                    flac_compression=flac_compression, out_rate=out_rate, noise_seed=noise_seed,
                                    noise_keys=[item_key(nn) for nn in names], transpositions=rows, formants=formant,
                                    f0s=done.contours, loudness=loudness, peak_limit=peak_limit, true_peak=true_peak,
                                    levels_out=levels_out, limiter=limiter, lookahead_ms=lookahead_ms, hold_ms=hold_ms)

    def track_f0(self, snd, srate, on_device=False, decode=None, f0_lag=None, **f0_params):
        """The pitch of a single sound (this build): (times in s, f0 in Hz with 0 = unvoiced, periodicity), one value per mel
        frame :meth:`generate_mel_from_snd` with ``resampler="reference"`` gives for it.  ``f0_params``: keywords of
        ``f0track.params`` (f0_min, f0_max, window, threshold, rms_floor).  Host (numpy) or, ``on_device``, the HIP kernel:
        the same bits on the same model-rate samples (a sound at another rate goes through the host or
        the device resampler first, as in ``generate_mels``).  ``decode``: None, or a ``f0decode.decode_params`` dictionary --
        the contour is then decoded over the whole sound, on the host or on the device alike; with
        ``f0_lag`` (frames, 0 .. 128; it needs ``decode``) as a live stream with that lag decides it (section 6l)."""
        from . import f0track
        from .analysis import generate_mels
        snd = np.asarray(snd)
        if snd.ndim == 2 and snd.shape[0] == 1:
            snd = snd[0]
        tracked = []
        generate_mels([snd], [srate], self.preprocess_config, on_device=on_device, batch=1, f0_out=tracked,
                      f0_params=f0track.params(int(round(self.srate)), **f0_params), f0_decode=decode, f0_lag=f0_lag)
        f0, periodicity = tracked[0]
        return f0track.frame_times(f0.size, self.hop_size, self.srate), f0, periodicity

    def calibrate(self, scaled_mells, verbose=False, max_frames=400, seed=42):
        """Decide the form of the WaveNet's dilated convolution on REAL data (this build; C ABI mbx_calibrate).

        The engine runs Winograd F(4,3) only where its own rounding stays within a quarter of the float32 parity budget of
        the direct form; at creation that is measured on a seeded synthetic mel (mbx_create), which a louder or otherwise
        unusual corpus need not resemble.  ``scaled_mells``: a list of ``scale_mel`` outputs (1, T, mel_channels), e.g. the
        first utterances of the job; at most ``max_frames`` frames of each are used.  The same procedure (direct form,
        F(4,3), F(2,3) on these inputs, the fastest form within the threshold is kept) then binds every later
        ``synth_from_mel``.  Returns ``self.model.conv_form_info()``; ``verbose`` prints the decision."""
        import torch
        mels = [np.asarray(mm, dtype=np.float32).reshape(-1, mm.shape[-2], mm.shape[-1])[0][:max_frames] for mm in scaled_mells]
        if not mels:
            raise ValueError("calibrate() needs at least one mel spectrogram")
        lengths = [int(mm.shape[0]) for mm in mels]
        batch = np.zeros((len(mels), max(lengths), mels[0].shape[1]), dtype=np.float32)
        for ii, mm in enumerate(mels):
            batch[ii, :lengths[ii]] = mm
        dims = self.model.dims
        noise = np.random.default_rng(seed).normal(size=(len(mels), max(lengths) * dims.wn_in_rows_per_frame)).astype(np.float32)
        dev = self.model.device
        info = self.model.calibrate(torch.as_tensor(batch, device=dev),
                                    n_frames=torch.as_tensor(lengths, dtype=torch.int32, device=dev),
                                    noise=torch.as_tensor(noise, device=dev) if dims.noise_sigma else None)
        self._calibrate_pending = False
        if verbose:
            e43 = "n/a" if info["err_f43"] is None else f"{info['err_f43']:.2e}"
            e23 = "n/a" if info["err_f23"] is None else f"{info['err_f23']:.2e}"
            print(f"    calibrated the convolution form on {len(mels)} mel spectrogram(s), {sum(lengths)} frames: {info['form']} "
                  f"(|audio(F(4,3)) - audio(direct)| {e43}, F(2,3) {e23}, threshold {info['threshold']:.2e} on |audio| <= "
                  f"{info['ref_max']:.2f})", file=sys.stderr)
        return info

    def generate_mel_from_snd(self, snd, srate, on_device=False, resampler="scipy"):
        """Audio -> ``.mell`` dictionary (reference mel_inverter.py:156-182); host side (analysis.py) or, with
        ``on_device=True``, the HIP kernel of csrc/mel_analysis.hip (same tables, float32 transform).
        The reference resamples when ``srate`` differs from the model rate through a function it never imports
        (mel_inverter.py:173, a NameError there); here the sound is resampled with a polyphase FIR
        (scipy.signal.resample_poly, Kaiser window) along the last axis.

        ``resampler="reference"`` (this build) resamples as the reference's TOOL does instead (bin/generate_mel.py:58-59,
        sig_proc/resample.py): resample.py::resample_host, or resample_device when ``on_device`` is set; a 1-D sound
        (or one row), as the tool reads them.  The result equals the file bin/generate_mel.py of this package writes."""
        from .analysis import compute_log_mel
        if resampler not in ("scipy", "reference"):
            raise ValueError(f"generate_mel_from_snd: resampler must be 'scipy' or 'reference', got {resampler!r}")
        if resampler == "reference":
            from .analysis import generate_mels
            snd = np.asarray(snd)
            if snd.ndim == 2 and snd.shape[0] == 1:
                snd = snd[0]
            return generate_mels([snd], [srate], self.preprocess_config, on_device=on_device, batch=1)[0]
        if srate != self.srate:
            from math import gcd
            from scipy.signal import resample_poly
            srate, target = int(round(srate)), int(round(self.srate))
            if srate <= 0:
                raise ValueError(f"generate_mel_from_snd: invalid sample rate {srate}")
            gg = gcd(srate, target)
            snd = resample_poly(np.asarray(snd, dtype=np.float64), target // gg, srate // gg, axis=-1)
        data_dict = {'nfft': self.fft_size,
                     'hoplen': self.hop_size,
                     'winlen': self.win_len,
                     'nmels': self.mel_channels,
                     'sr': self.srate,
                     'fmin': self.fmin,
                     'fmax': self.fmax,
                     'lin_spec_offset': self.lin_amp_off,
                     'lin_spec_scale': self.lin_amp_scale,
                     'log_spec_offset': 0.,
                     'log_spec_scale': self.mel_amp_scale,
                     "time_axis": 1}
        snd = np.asarray(snd)
        if snd.ndim == 1:
            snd = snd[np.newaxis]
        if on_device:
            import torch
            from .analysis import compute_log_mel_device
            mel_dev, _ = compute_log_mel_device(torch.as_tensor(np.ascontiguousarray(snd, dtype=np.float32)).cuda(),
                                                self.preprocess_config)
            mel_ref = mel_dev.cpu().numpy()
        else:
            mel_ref, _ = compute_log_mel(snd, self.preprocess_config, dtype=np.float32)
        data_dict['mell'] = mel_ref[0].T
        return data_dict

    # ------------------------------------------------------------------------------------------
    def load_model(self, model_id_or_path, verbose=False, calibrate=False, batch_invariant=None, conv_form=None):
        """reference mel_inverter.py:184-239: resolve the model directory, read ``config.yaml``, build the
        generator, restore the weights and copy the pre-processing parameters onto the instance.

        ``batch_invariant`` (this build; ``mbx_config.batch_invariant``, None = the engine's default): True pins the engine's
        kernels so that an utterance's bits do not depend on the batch it runs in (:meth:`synth_from_mels`).

        ``conv_form`` (this build; ``mbx_config.wn_conv_form``, None = "auto"): "auto" | "direct" | "f23" | "f43" pins the form
        of the WaveNet's dilated convolution.  A force_causal / CAUSAL-padded model runs its Winograd kernels only when a form
        is pinned ("f23" / "f43"); under "auto" it keeps the direct form.

        ``calibrate=True`` (this build; ORDER DEPENDENT: the decision is taken on at most 400 frames of the first utterance and
        binds every later one, a failing calibration keeps the creation-time form with a warning): the first mel handed to
        :meth:`synth_from_mel` goes through :meth:`calibrate`
        before it is synthesised -- the form of the WaveNet's convolution is then decided on the job's own data instead
        of on the synthetic mel of ``mbx_create`` (``resynth_mel.py --calibrate N`` does the same on the first N files)."""
        from . import get_config_file
        from .config import read_config
        from .engine import MBExWNEngine
        from .weights import load_weights

        config_file = get_config_file(model_id_or_path=model_id_or_path)
        model_dir = os.path.dirname(config_file)
        hparams = read_config(config_file=config_file)
        if "mbexwn_config" not in hparams:
            raise NotImplementedError(f"create_model::error::unkown config requested {list(hparams.keys())}. "
                                      "Only mbexwn_config is currently supported.")   # reference models.py:22-31
        self.config_file = config_file
        self.preprocess_config = hparams["preprocess_config"]

        weights_npz = os.path.join(model_dir, "weights.npz")
        weights_tf = os.path.join(model_dir, "weights.tf")            # reference mel_inverter.py:206
        if os.path.exists(weights_npz):
            if verbose:
                print(f"restore from {weights_npz}", file=sys.stderr)
            raw = load_weights(weights_npz)
        elif os.path.exists(weights_tf + ".index"):
            # the pretrained models of the reference ship as TensorFlow checkpoints; read without TensorFlow
            from .tf_checkpoint import load_reference_checkpoint
            if verbose:
                print(f"restore from {weights_tf}", file=sys.stderr)
            raw = load_reference_checkpoint(weights_tf, hparams)
        else:
            raise FileNotFoundError(f"error::no weights found under {model_dir} (expected weights.npz or weights.tf.index)")
        self.model = MBExWNEngine(hparams, raw, batch_invariant=batch_invariant, conv_form=conv_form)
        self._calibrate_pending = bool(calibrate)
        self._verbose = bool(verbose)
        if verbose:
            info = self.model.conv_form_info()
            print(f"convolution form {info['form']} (requested {info['requested']}, calibrated at creation on a synthetic mel: "
                  f"{'yes' if info['calibrated'] == 1 else 'no'})", file=sys.stderr)
        self._set_preprocess_config(self.preprocess_config)

    def _set_preprocess_config(self, preprocess_config):
        self.preprocess_config = preprocess_config
        self.mel_channels = self.preprocess_config["mel_channels"]
        self.hop_size = self.preprocess_config["hop_size"]
        self.fft_size = self.preprocess_config["fft_size"]
        self.fmin = self.preprocess_config["fmin"]
        self.fmax = self.preprocess_config["fmax"]
        self._srate = self.preprocess_config['sample_rate']
        # the reference falls back to an undefined name here (mel_inverter.py:221); the fft size is what it means
        self.win_len = self.preprocess_config.get('win_size', self.fft_size)

        self.lin_amp_scale = 1
        if self.preprocess_config.get("lin_amp_scale", 1) != 1:
            self.lin_amp_scale = self.preprocess_config["lin_amp_scale"]
        self.lin_amp_off = 1.e-5
        if self.preprocess_config.get("lin_amp_off", None) is not None:
            self.lin_amp_off = self.preprocess_config["lin_amp_off"]
        self.mel_amp_scale = 1
        if self.preprocess_config.get("mel_amp_scale", 1) != 1:
            self.mel_amp_scale = self.preprocess_config["mel_amp_scale"]
        self.use_max_limit = False
        if self.preprocess_config.get("use_max_limit", False):
            self.use_max_limit = self.preprocess_config["use_max_limit"]


# where the pitch of transform_audio comes from: the model's F0-net, or the F0 tracker on the sound itself
F0_SOURCES = ("net", "audio")


class KeyedNoise:
    """Per-item keyed noise for ``batched.run_micro_batches``: the seed and the items' keys; each micro-batch's draw is
    filled on the device by ``engine.keyed_noise`` when the batch is staged."""

    def __init__(self, seed, keys):
        self.seed, self.keys = int(seed), [int(kk) for kk in keys]


def check_factors(transposition, count, what="transposition"):
    """``transposition`` -- one factor or ``count`` of them -- as a list of ``count`` finite positive floats.  ``what`` names
    the factor in the messages (the formant shift is checked here too: one factor, or one per mel frame)."""
    factors = np.asarray(transposition, dtype=np.float64)
    if factors.ndim == 0:
        factors = np.full(count, float(factors))
    if factors.shape != (count,):
        raise ValueError(f"{what} must be one factor or one per item ({count})")
    if not (np.all(np.isfinite(factors)) and np.all(factors > 0)):
        raise ValueError(f"{what} must be finite and positive")
    return [float(ff) for ff in factors]


def create_synthetic_model_dir(path, voice_type="SPEECH", seed=1234, weights_format="npz", **config_overrides):
    """Write a model directory (config.yaml + weights.npz, or weights.tf.* in the TensorFlow checkpoint format of the
    reference's model zips) with the canonical architecture and seeded synthetic weights -- the stand-in for the
    pretrained model zip that is not part of the reference tree."""
    from .config import canonical_config, dump_config
    from .weights import save_weights, synthetic_weights
    os.makedirs(path, exist_ok=True)
    cfg = canonical_config(voice_type, **config_overrides)
    dump_config(os.path.join(path, "config.yaml"), cfg)
    raw = synthetic_weights(cfg, seed=seed)
    if weights_format == "tf":
        from .tf_checkpoint import to_reference_variables, write_checkpoint
        write_checkpoint(os.path.join(path, "weights.tf"), to_reference_variables(raw, config=cfg))
    else:
        save_weights(os.path.join(path, "weights.npz"), raw)
    return path

#!/usr/bin/env python3
"""Transpose a running voice: feeds a sound file through a ``LiveResynthesizer`` (mbexwn_vocoder_amd/live.py) in tick-sized
pushes, as a live source would deliver it, and writes what the stream gives back.

    stream_transpose.py in.wav -o out.wav --model_id VOICE --transposition 1.5 [--formant-shift F] [--tick-ms 80]
                        [--resample] [--output-rate R|input]
                        [--peak-limit DBFS [--gain DB] [--limiter-lookahead MS] [--limiter-hold MS]]
                        [--f0-source audio [--f0-min HZ --f0-max HZ --f0-initial HZ] [--write-f0]
                         [--pitch-decode viterbi [--pitch-lag N --pitch-jump W --pitch-switch W]]]

The demonstration of the live path (streaming mel analysis -> scale_mel -> streaming synthesis with per-frame pitch control).
The input must be at the model's sample rate, unless ``--resample`` is given: then a file at another rate streams at its own
rate (``--tick-ms`` of its own samples per push), is resampled on the device by the stream, and the output is written at the
model rate -- or, with ``--output-rate R``, at R Hz (``input``: the file's own rate): the stream resamples its output on the
device too.  A ``.wav`` output holds the float32 samples as they are; any other extension goes through the writers of
resynth_mel.py.

``--f0-source audio`` keeps the pitch that is in the sound: the stream tracks its F0 on the device
between ``--f0-min`` and ``--f0-max`` Hz and drives the oscillator with it, an unvoiced frame holding the last voiced value
(``--f0-initial`` Hz in front of the first); ``--transposition`` multiplies on top.  The output is what ``transform_audio.py
--f0-source audio --f0-fill hold`` writes for the file under the same ``--noise-seed``.  ``--write-f0`` writes the raw tracked
rows as NAME.f0 beside the output (text rows `time_s f0_hz periodicity`, one per mel frame, 0 = unvoiced).

``--pitch-decode viterbi`` decodes the tracked contour with a fixed lag of ``--pitch-lag`` frames (8
frames are 100 ms at hop 300 / 24 kHz): a frame is decided, and synthesised, once that many later frames have been seen,
which removes the octave jumps of the frame-by-frame pick at the price of that much more look-ahead.  The output -- and the
contour ``--write-f0`` writes -- is then what ``transform_audio.py --f0-source audio --pitch-decode viterbi --pitch-lag N
--f0-fill hold`` gives for the file under the same ``--noise-seed``.

``--peak-limit DBFS`` keeps the stream under that ceiling with the look-ahead peak limiter, the last
stage of the stream, at the rate the output is written at; ``--gain DB`` is the fixed gain in front of it (a stream has no
integrated loudness), ``--limiter-lookahead`` and ``--limiter-hold`` its window in ms.  A stream that overshoots -- a formant
shift or a transposition does that -- is otherwise handed out over full scale.
"""
import os
import sys

import numpy as np

test_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'mbexwn_vocoder_amd')
if os.path.exists(test_path):
    sys.path.insert(0, os.path.dirname(os.path.abspath(test_path)))

from mbexwn_vocoder_amd import cli, get_config_file  # noqa: E402
from mbexwn_vocoder_amd.audioio import read_audio  # noqa: E402
from mbexwn_vocoder_amd.config import read_config  # noqa: E402
from mbexwn_vocoder_amd.live import check_rate  # noqa: E402


def stream_file(live, samples, tick_samples, transposition, seed=0, stream_id=0, sample_rate=None, output_rate=None,
                noise_fn=None, formant=None, f0_source="net", f0_params=None, f0_initial=150.0, f0_out=None, f0_decode=None,
                f0_lag=None, level=None):
    """Push `samples` in pieces of tick_samples, one tick per push, until the stream is finished; returns its audio.
    ``sample_rate``: the rate of `samples` when it is not the model's (the stream resamples); ``output_rate``: the rate the
    audio comes back at when it is not the model's (a rate in Hz, or "input"); ``noise_fn``: the stream's noise instead of the
    generator seeded with ``seed`` (``live.keyed_noise_fn``); ``formant``: a formant-shift factor given with every push; ``f0_source``,
    ``f0_params``, ``f0_initial``, ``f0_decode``, ``f0_lag``: as for ``LiveResynthesizer.open``; ``f0_out``: a list that
    receives the stream's tracked (f0, periodicity), one pair of arrays per tick that handed out (with a lag: decided) rows;
    ``level``: None, or the keywords ``gain_db``, ``peak_limit``, ``limiter_lookahead_ms``, ``limiter_hold_ms`` of
    ``LiveResynthesizer.open``."""
    rates = {} if sample_rate is None else {"sample_rate": sample_rate}
    if f0_source != "net":
        rates.update(f0_source=f0_source, f0_params=f0_params, f0_initial=f0_initial)
    if f0_lag is not None:
        rates.update(f0_decode=f0_decode, f0_lag=f0_lag)

    def tick():
        audio = live.tick().get(stream_id)
        if f0_out is not None and stream_id in live.last_f0:
            f0_out.append(live.last_f0[stream_id])
        return audio

    if output_rate is not None:
        rates["output_rate"] = output_rate
    rates.update(level or {})
    live.open(stream_id, seed=seed, noise_fn=noise_fn, **rates)
    out = []
    for start in range(0, samples.size, tick_samples):
        end = min(start + tick_samples, samples.size)
        live.push_audio(stream_id, samples[start:end], last=end == samples.size, transposition=transposition,
                        **({} if formant is None else {"formant": formant}))
        out += [audio for audio in [tick()] if audio is not None]
    while not live.finished(stream_id):
        audio = tick()
        if audio is None:                                     # a closed stream emits with every tick until it is finished
            raise RuntimeError("the closed stream did not advance")
        out.append(audio)
    live.close(stream_id)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.float32)


def main(input_audio_file, output_file, model_id="VOICE", transposition=1.0, tick_ms=80.0, seed=0, quiet=False,
         resample=False, output_rate=None, noise_seed=None, formant_shift=1.0, f0_source="net", f0_min=55.0, f0_max=1000.0,
         f0_initial=150.0, write_f0=False, pitch_decode="greedy", pitch_lag=8, pitch_jump=4.0, pitch_switch=0.5, gain=None,
         peak_limit=None, limiter_lookahead=None, limiter_hold=None):
    preprocess_config = read_config(config_file=get_config_file(model_id_or_path=model_id))['preprocess_config']
    if not os.path.isfile(input_audio_file):
        print(f"stream_transpose::error:: no such file: {input_audio_file}", file=sys.stderr)
        sys.exit(1)
    samples, rate = read_audio(input_audio_file)
    model_rate = int(round(preprocess_config["sample_rate"]))
    try:
        if output_rate == "input" and not resample and int(round(rate)) != model_rate:
            raise ValueError(f"--output-rate input: {input_audio_file} is at {rate} Hz, not the model rate {model_rate} Hz; "
                             "stream it at its own rate with --resample")
        if not resample:
            check_rate(rate, preprocess_config["sample_rate"], what=input_audio_file)
        elif int(round(rate)) <= 0:
            raise ValueError(f"{input_audio_file}: invalid sample rate {rate}")
        if samples.size == 0:
            raise ValueError(f"{input_audio_file}: no samples")
        if not (np.isfinite(transposition) and transposition > 0):
            raise ValueError("--transposition must be finite and positive")
        if not (np.isfinite(formant_shift) and formant_shift > 0):
            raise ValueError("--formant-shift must be finite and positive")
        if f0_source not in ("net", "audio"):
            raise ValueError(f"--f0-source must be net or audio, got {f0_source!r}")
        if write_f0 and f0_source != "audio":
            raise ValueError("--write-f0 writes what the stream tracked: it needs --f0-source audio")
        f0_decode = cli.pitch_decode_params(pitch_decode, pitch_jump, pitch_switch)
        if f0_decode is not None and f0_source != "audio":
            raise ValueError("--pitch-decode viterbi decodes what the stream tracked: it needs --f0-source audio")
        f0_lag = None if f0_decode is None else cli.lag_arg(str(pitch_lag))
        f0_params = None
        if f0_source == "audio":
            from mbexwn_vocoder_amd import f0track
            f0_params = f0track.params(model_rate, f0_min=f0_min, f0_max=f0_max)
            if not (np.isfinite(f0_initial) and f0_initial > 0):
                raise ValueError("--f0-initial must be finite and positive")
        level = None
        if peak_limit is None:
            if gain is not None or limiter_lookahead is not None or limiter_hold is not None:
                raise ValueError("--gain, --limiter-lookahead and --limiter-hold go with --peak-limit")
        else:
            from mbexwn_vocoder_amd import limiter
            level = {"gain_db": 0.0 if gain is None else gain, "peak_limit": peak_limit,
                     "limiter_lookahead_ms": limiter_lookahead, "limiter_hold_ms": limiter_hold}
            written_rate = model_rate if output_rate is None else int(round(rate)) if output_rate == "input" else int(output_rate)
            limiter.check_window(*limiter.window(written_rate, level["limiter_lookahead_ms"], level["limiter_hold_ms"]))
    except (ValueError, cli.ArgumentTypeError) as err:
        print(f"stream_transpose::error:: {err}", file=sys.stderr)
        sys.exit(1)
    import torch
    if not torch.cuda.is_available():
        print("stream_transpose::error:: no GPU available; this build has no CPU path", file=sys.stderr)
        sys.exit(1)
    from mbexwn_vocoder_amd.batched import write_audio
    from mbexwn_vocoder_amd.live import LiveResynthesizer, keyed_noise_fn
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    live = LiveResynthesizer(MELInverter(model_id_or_path=model_id))
    tick_samples = max(1, int(round(tick_ms * 1e-3 * rate)))
    own_rate = int(round(rate)) if int(round(rate)) != model_rate else None
    out_rate = (own_rate or model_rate) if output_rate == "input" else int(output_rate or model_rate)
    # --noise-seed: the keyed noise of the file (its basename is the key), what transform_audio.py draws for it
    keyed = {} if noise_seed is None else {"noise_fn": keyed_noise_fn(live.mel_inverter.model, noise_seed),
                                           "stream_id": os.path.basename(input_audio_file)}
    tracked = [] if write_f0 else None
    audio = stream_file(live, samples, tick_samples, transposition, seed=seed, sample_rate=own_rate,
                        output_rate=out_rate if out_rate != model_rate else None,
                        formant=None if formant_shift == 1.0 else formant_shift, f0_source=f0_source, f0_params=f0_params,
                        f0_initial=f0_initial, f0_out=tracked, f0_decode=f0_decode, f0_lag=f0_lag, level=level, **keyed)
    out_dir = os.path.dirname(os.path.abspath(output_file))
    os.makedirs(out_dir, exist_ok=True)
    ext = os.path.splitext(output_file)[1].lower().lstrip(".") or "wav"
    if ext == "wav":
        from scipy.io import wavfile
        wavfile.write(output_file, out_rate, audio.astype(np.float32, copy=False))
    else:
        write_audio(output_file, audio, out_rate, ext)
    if write_f0:
        f0, periodicity = (np.concatenate([pair[kk] for pair in tracked]) if tracked else np.zeros(0, np.float32) for kk in (0, 1))
        f0track.write_f0(os.path.splitext(output_file)[0] + ".f0",
                         f0track.frame_times(f0.size, int(preprocess_config["hop_size"]), model_rate), f0, periodicity)
    if not quiet:
        print(f"{input_audio_file}: {samples.size} samples in pushes of {tick_samples} -> {audio.size} samples, transposed by "
              f"{transposition}, look-ahead {live.lookahead_ms_for(own_rate, out_rate, f0_source, f0_params, f0_lag, peak_limit, limiter_lookahead):.1f} ms, saved at {out_rate} Hz under {output_file}",
              file=sys.stderr)


output_rate_arg = cli.rate_arg(allow_input=True)


def make_parser():
    from argparse import ArgumentParser
    parser = ArgumentParser(description="transpose a sound file through the live path: streaming analysis and synthesis")
    parser.add_argument("input_audio_file", help="mono sound file at the model's sample rate (any rate with --resample)")
    parser.add_argument("-o", "--output_file", required=True, help="sound file to write (.wav: float32 samples)")
    parser.add_argument("--model_id", default="VOICE", nargs="?", const="",
                        help="model identifier or path to a model directory. Given without a value the script lists all known "
                             "models. (Def: %(default)s)")
    parser.add_argument("--transposition", default=1.0, type=float, metavar="F", help="factor on the pitch (Def: %(default)s)")
    parser.add_argument("--formant-shift", dest="formant_shift", default=1.0, type=float, metavar="F",
                        help="factor on the formant frequencies at the same pitch: F > 1 moves them up (Def: %(default)s)")
    parser.add_argument("--tick-ms", dest="tick_ms", default=80.0, type=float,
                        help="milliseconds of audio per push and tick (Def: %(default)s)")
    parser.add_argument("--resample", action="store_true",
                        help="stream a file at another rate at its own rate: the stream resamples on the device, the output "
                             "is at the model rate")
    parser.add_argument("--output-rate", dest="output_rate", default=None, type=output_rate_arg, metavar="R|input",
                        help="write the output at R Hz, resampled on the device by the stream; input = the file's own rate, "
                             "which needs --resample when that is not the model's (Def: the model rate)")
    parser.add_argument("--f0-source", dest="f0_source", default="net", choices=["net", "audio"],
                        help="where the pitch comes from: net = what the model infers from the mel; audio = the streaming F0 "
                             "tracker on the sound itself, unvoiced frames holding the last voiced value; --transposition "
                             "multiplies on top of either (Def: %(default)s)")
    parser.add_argument("--f0-min", dest="f0_min", default=55.0, type=float, metavar="HZ",
                        help="lowest pitch the F0 tracker looks for (Def: %(default)s)")
    parser.add_argument("--f0-max", dest="f0_max", default=1000.0, type=float, metavar="HZ",
                        help="highest pitch the F0 tracker looks for (Def: %(default)s)")
    parser.add_argument("--f0-initial", dest="f0_initial", default=150.0, type=float, metavar="HZ",
                        help="--f0-source audio: the pitch in front of the first voiced frame (Def: %(default)s)")
    parser.add_argument("--write-f0", dest="write_f0", action="store_true",
                        help="--f0-source audio: write the tracked rows as NAME.f0 beside the output: text rows `time_s f0_hz "
                             "periodicity`, one per mel frame, 0 = unvoiced")
    parser.add_argument("--pitch-decode", dest="pitch_decode", default="greedy", choices=["greedy", "viterbi"],
                        help="--f0-source audio: greedy = every frame's pick on its own; viterbi = one path over the YIN "
                             "candidates, each frame decided --pitch-lag frames later: no octave jumps (Def: %(default)s)")
    parser.add_argument("--pitch-lag", dest="pitch_lag", default=8, type=cli.lag_arg, metavar="N",
                        help="--pitch-decode viterbi: frames of look-ahead of the decoder, 0 .. 128 (Def: %(default)s)")
    parser.add_argument("--pitch-jump", dest="pitch_jump", default=4.0, type=cli.weight_arg, metavar="W",
                        help="--pitch-decode viterbi: weight of a pitch jump between two frames (Def: %(default)s)")
    parser.add_argument("--pitch-switch", dest="pitch_switch", default=0.5, type=cli.weight_arg, metavar="W",
                        help="--pitch-decode viterbi: cost of a change between voiced and unvoiced (Def: %(default)s)")
    parser.add_argument("--peak-limit", dest="peak_limit", default=None, type=cli.decibel_arg, metavar="DBFS",
                        help="keep the stream under DBFS with the look-ahead peak limiter on the device, the last stage of the "
                             "stream (Def: no limiter)")
    parser.add_argument("--gain", default=None, type=cli.decibel_arg, metavar="DB",
                        help="--peak-limit: a fixed gain in front of the limiter (Def: 0)")
    parser.add_argument("--limiter-lookahead", dest="limiter_lookahead", default=None, type=cli.positive_ms_arg, metavar="MS",
                        help="--peak-limit: the limiter's look-ahead, which the stream's look-ahead grows by (Def: 1.5)")
    parser.add_argument("--limiter-hold", dest="limiter_hold", default=None, type=cli.positive_ms_arg, metavar="MS",
                        help="--peak-limit: the limiter's hold (Def: 20)")
    parser.add_argument("--seed", default=0, type=int, help="seed of the stream's noise generator (Def: %(default)s)")
    parser.add_argument("--noise-seed", dest="noise_seed", default=None, type=int, metavar="S",
                        help="draw the stream's noise keyed by (S, the file's basename) and the absolute step, as "
                             "transform_audio.py --noise-seed S does for the file; --seed is then unused (Def: the generator "
                             "seeded with --seed)")
    parser.add_argument("-q", "--quiet", action="store_true", help="dont display progress")
    return parser


if __name__ == "__main__":
    args = make_parser().parse_args()

    if not args.model_id:
        cli.print_models()
    else:
        main(**vars(args))

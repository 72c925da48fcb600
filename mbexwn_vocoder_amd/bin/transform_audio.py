#!/usr/bin/env python3
"""Transpose sound files in batches: sound files in, transposed sound files out, on the MI355X HIP path.

    transform_audio.py FILES... -o DIR --model_id VOICE [--transposition F | --transposition-file LIST] [--noise-seed S]
                       [--time-stretch F | --time-stretch-file LIST] [--formant-shift F | --formant-shift-file LIST]
                       [--align-to GUIDE | --align-to-dir DIR] [--align-band SECONDS]
                       [--batch N] [--gpus N] [--out-rate R|input]
                       [--format flac] [--flac-compression fixed]

Joins the stages of generate_mel.py and resynth_mel.py in one process (mbexwn_vocoder_amd/batched.py::run_audio_job): the
device resampler and mel analysis, scale_mel on the host, the synthesis in padded micro-batches with the factor on every mel
frame, the output resampler and the FLAC frames on the device.  The outputs are named syn_<basename>.<format>.

The noise channel takes keyed noise (include/mbexwn_noise.h): a function of (--noise-seed, the file's basename, the step).
With --batch-invariant or a pinned --conv-form a file's samples therefore do not depend on the batch size, the order of the
arguments, the number of ranks or the other files of the job, and on an f23 engine they are what stream_transpose.py
--noise-seed S streams for the file.

A file gives frames * hop samples at the model rate before the output resampler (frames = resampled length // hop + 1), as
the live path emits: the output is not trimmed to the input's length.  A file without samples or with more than one channel
is reported and skipped; the others are written and the exit status is 1.

--time-stretch F makes a file F times as long at the same pitch (mbexwn_vocoder_amd/timemap.py): the
analysis places its frames at the warped positions of the sound (include/mbexwn_warp.h) and the file gives K * hop samples
for the K frames of the time map.  A factor of 1 is the regular analysis.  A file whose stretched length exceeds the engine's
limit is reported and skipped like the others.

--align-to GUIDE gives every file the TIMING of the recording GUIDE, --align-to-dir DIR that of DIR/<the file's basename>
(mbexwn_vocoder_amd/align.py; include/mbexwn_align.h): the mel frames of guide and file are aligned by
dynamic time warping within --align-band seconds of the diagonal, with local slope between 1/2 and 2, the analysis places one
frame per guide frame where the path says, and the file comes out with the guide's sample count: dubbing to a guide track,
stacking doubles.  Both recordings must hold the same material from start to end.  A file that cannot be aligned (a length
ratio outside about 1/2 .. 2, a band too narrow) is reported and skipped like the others.  Not combinable with --time-stretch.

--formant-shift F moves the formants of a file by the factor F (F > 1: up) at the same pitch and duration (DESIGN.md section
6g; include/mbexwn_envelope.h): the VTF-net and the WaveNet conditioning read every mel row at f / F, the F0-net reads it as
it is.  A factor of 1 is the job without the flag, launch by launch.  The level is not compensated (--loudness input does
that).  The three controls combine freely.

--loudness LUFS writes every file at that BS.1770 integrated loudness, --loudness input at the loudness of its source sound,
measured as read (mbexwn_vocoder_amd/level.py; include/mbexwn_level.h): one static gain per file,
measured and applied on the GPU between the output resampler and the FLAC encoder.  --peak-limit DBFS (default -1 with
--loudness) scales a file down as a whole where it would peak above; alone it only ever scales down, so no file is written
clipped.  --true-peak puts the limit on the 4x oversampled peak.  The writer reports loudness in -> out, gain and peak per file.
--limiter keeps the ceiling (-1 dBFS unless --peak-limit says otherwise) with a look-ahead peak limiter on the GPU in place of
the one gain, so that the loudness stands although single peaks are in its way (--limiter-lookahead / --limiter-hold MS: its
window); the writer then reports the loudness and the peak measured behind it and what it did.

--f0-source audio keeps the pitch that is in the sound instead of the pitch the model infers from the mel (DESIGN.md section
6h; include/mbexwn_pitch.h): an F0 tracker runs on the frames of the mel analysis, between --f0-min and --f0-max Hz, its
unvoiced frames are filled from their neighbours and the contour drives the oscillator; --transposition multiplies on top; a
file without a voiced frame keeps the model's F0.  --f0-fill hold fills causally instead, as a live stream must (DESIGN.md
section 6j): an unvoiced frame holds the last voiced value and the frames in front of the first take --f0-initial Hz; the file
then has the samples stream_transpose.py --f0-source audio streams for it.  --write-f0 writes the tracked contour as NAME.f0 into the output directory
(text rows `time_s f0_hz periodicity`, one per mel frame, 0 = unvoiced), with either source.

--pitch-decode viterbi decodes that contour over the whole file instead of picking every frame on its own (DESIGN.md section
6i; include/mbexwn_contour.h): every frame offers several YIN candidates and an unvoiced state, and the cheapest path wins,
with --pitch-jump on the relative change of period between frames and --pitch-switch on a change between voiced and
unvoiced.  A frame whose pick alone would land an octave off no longer does.  The default, greedy, is the job of before.
"""
import json
import os
import sys
from functools import partial

test_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'mbexwn_vocoder_amd')
if os.path.exists(test_path):
    sys.path.insert(0, os.path.dirname(os.path.abspath(test_path)))

from mbexwn_vocoder_amd import cli  # noqa: E402
from mbexwn_vocoder_amd.batched import file_factors, file_stretches, read_transposition_file  # noqa: E402
from mbexwn_vocoder_amd.cli import pitch_decode_params, weight_arg  # noqa: E402
from mbexwn_vocoder_amd.level import check_options  # noqa: E402

file_guides = partial(cli.file_guides, stretch_flags="--time-stretch or --time-stretch-file")
factor_arg = stretch_arg = cli.positive_arg("factor")
hertz_arg = cli.positive_arg("frequency in Hz")
band_arg = cli.positive_arg("number of seconds")
out_rate_arg = cli.rate_arg(allow_input=True)


def main(input_audio_files, output_dir, model_id="VOICE", transposition=1.0, transposition_file=None, noise_seed=0, batch=16,
         gpus=1, num_threads=2, out_rate=None, format="flac", flac_compression="verbatim", conv_form="auto",
         batch_invariant=False, verbose=False, quiet=False, rank=None, job=None, time_stretch=1.0, time_stretch_file=None,
         formant_shift=1.0, formant_shift_file=None, f0_source="net", f0_min=55.0, f0_max=1000.0, write_f0=False,
         pitch_decode="greedy", pitch_jump=4.0, pitch_switch=0.5, f0_fill="interpolate", f0_initial=150.0, align_to=None,
         align_to_dir=None, align_band=1.0, pitch_lag=None, loudness=None, peak_limit=None, true_peak=False, limiter=False,
         limiter_lookahead=None, limiter_hold=None):
    values = dict(locals())
    try:
        check_options(loudness, peak_limit, true_peak, allow_input=True, limiter=limiter, lookahead_ms=limiter_lookahead,
                      hold_ms=limiter_hold)
        cli.check_limiter_rate(model_id, out_rate, limiter, limiter_lookahead, limiter_hold, true_peak)
        guides, f0_decode, factors, stretches, formants = file_options(values)
        check_files(input_audio_files)
    except (OSError, ValueError) as err:
        print(f"transform_audio::error:: {err}", file=sys.stderr)
        sys.exit(1)
    if gpus > 1 and rank is None:
        sys.exit(run_parent(values, stretches, guides))
    import torch
    if not torch.cuda.is_available():
        print("transform_audio::error:: no GPU available; this build has no CPU path", file=sys.stderr)
        sys.exit(1)
    plan = None
    if job is not None:                                       # a rank of a --gpus job: its device and its files
        with open(job) as fo:
            plan = json.load(fo)
        torch.cuda.set_device(rank % plan["devices"])
    if num_threads:
        torch.set_num_threads(max(1, int(num_threads)))
    from mbexwn_vocoder_amd.batched import run_audio_job
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    inv = MELInverter(model_id_or_path=model_id, verbose=verbose, batch_invariant=True if batch_invariant else None,
                      conv_form=None if conv_form == "auto" else conv_form)
    os.makedirs(output_dir, exist_ok=True)
    try:
        skipped = run_audio_job(inv, input_audio_files, output_dir, format, factors=factors, noise_seed=noise_seed,
                                mine=plan["shards"][rank] if plan else None, batch=batch, threads=num_threads, verbose=verbose,
                                quiet=quiet, flac_compression=flac_compression, out_rate=out_rate,
                                stretches=None if all(ss == 1.0 for ss in stretches) else stretches,
                                formants=None if all(ff == 1.0 for ff in formants) else formants, f0_source=f0_source,
                                f0_params={"f0_min": f0_min, "f0_max": f0_max}, write_f0=write_f0, f0_decode=f0_decode,
                                f0_fill=f0_fill, f0_initial=f0_initial, guides=guides, align_band_s=align_band,
                                f0_lag=pitch_lag, loudness=loudness, peak_limit=peak_limit, true_peak=true_peak,
                                limiter=limiter, lookahead_ms=limiter_lookahead, hold_ms=limiter_hold)
    except ValueError as err:
        if guides is None and not str(err).startswith("limiter:"):
            raise
        print(f"transform_audio::error:: {err}", file=sys.stderr)       # a band or a length the alignment refuses
        sys.exit(1)
    if skipped:
        sys.exit(1)


def file_options(v):
    """What ``main``'s arguments ``v`` say per file, checked: the guides (or None), the decode parameters (or None), the
    transposition, time-stretch and formant-shift factors.  ValueError or OSError for what the tool refuses."""
    files = v["input_audio_files"]
    guides = file_guides(files, v["align_to"], v["align_to_dir"], v["align_band"], v["time_stretch"], v["time_stretch_file"])
    if v["f0_source"] not in ("net", "audio"):
        raise ValueError(f"--f0-source must be net or audio, got {v['f0_source']!r}")
    if not 0.0 < v["f0_min"] < v["f0_max"]:
        raise ValueError(f"--f0-min must lie below --f0-max, got {v['f0_min']} and {v['f0_max']}")
    if v["f0_fill"] not in ("interpolate", "hold"):
        raise ValueError(f"--f0-fill must be interpolate or hold, got {v['f0_fill']!r}")
    if v["f0_fill"] == "hold" and v["f0_source"] != "audio":
        raise ValueError("--f0-fill hold fills the tracked contour: it needs --f0-source audio")
    f0_decode = pitch_decode_params(v["pitch_decode"], v["pitch_jump"], v["pitch_switch"])
    if f0_decode is not None and v["f0_source"] != "audio" and not v["write_f0"]:
        raise ValueError("--pitch-decode viterbi decodes the tracked contour: it needs --f0-source audio or --write-f0")
    if v.get("pitch_lag") is not None and f0_decode is None:
        raise ValueError("--pitch-lag is the look-ahead of the decoder: it needs --pitch-decode viterbi")

    def table(path):
        return read_transposition_file(path) if path else None

    return (guides, f0_decode, file_factors(files, v["transposition"], table(v["transposition_file"])),
            file_stretches(files, v["time_stretch"], table(v["time_stretch_file"])),
            file_factors(files, v["formant_shift"], table(v["formant_shift_file"]), what="formant shift"))


def check_files(files):
    """ValueError for a file that is not there and for two files with one basename."""
    missing = [ff for ff in files if not os.path.isfile(ff)]
    if missing:
        raise ValueError(f"no such file: {', '.join(missing)}")
    if len({os.path.basename(ff) for ff in files}) != len(files):
        raise ValueError("two input files share a basename: they would share an output file and a noise key")


def run_parent(v, stretches, guides):
    """--gpus N: this parent never initialises HIP; N fresh child processes write their share of the files each.  Returns
    the exit status of the job."""
    from mbexwn_vocoder_amd import batched, get_config_file
    from mbexwn_vocoder_amd.config import ModelDims, read_config
    dims = ModelDims(read_config(config_file=get_config_file(model_id_or_path=v["model_id"])))
    plan = batched.plan_audio_ranks(v["input_audio_files"], v["gpus"], threads=v["num_threads"], stretches=stretches,
                                    frame_limit=(dims.hop_size, dims.sample_rate, dims.steps_per_frame), guides=guides)
    for name, why in plan["skipped"]:
        print(f"transform_audio::error:: skipped {name}: {why}", file=sys.stderr)
    # the tracker's range travels with whatever tracks, also at its default
    always = ("f0_min", "f0_max") if v["f0_source"] != "net" or v["write_f0"] else ()
    argv = cli.rank_argv(make_parser(), v, plan["files"], always=always)
    status = batched.run_ranks(os.path.abspath(__file__), argv, v["model_id"], plan["files"], v["gpus"],
                               threads=v["num_threads"], quiet=v["quiet"], plan=plan, tool="transform_audio") if plan["files"] else 0
    return 1 if status or plan["skipped"] else 0


def make_parser():
    from argparse import SUPPRESS, ArgumentParser, ArgumentTypeError

    class Parser(ArgumentParser):
        """The align flags exclude the time stretch: refused at parse time, with exit status 2."""

        def parse_args(self, args=None, namespace=None):
            parsed = super().parse_args(args, namespace)
            try:
                file_guides([], parsed.align_to, parsed.align_to_dir, parsed.align_band, parsed.time_stretch,
                            parsed.time_stretch_file)
            except (ValueError, ArgumentTypeError) as err:
                self.error(str(err))
            return parsed

    parser = Parser(description="transpose sound files with an MBExWN model: analysis, pitch control and synthesis in "
                                        "batches (MI355X HIP path)")
    parser.add_argument("input_audio_files", nargs="+", help="mono sound files, at any sample rate")
    parser.add_argument("-o", "--output_dir", required=True, help="output directory where the transposed sounds will be stored")
    parser.add_argument("--model_id", default="VOICE", nargs="?", const="",
                        help="model identifier or path to a model directory. Given without a value the script lists all known "
                             "models. (Def: %(default)s)")
    parser.add_argument("--transposition", default=1.0, type=factor_arg, metavar="F", help="factor on the pitch (Def: %(default)s)")
    parser.add_argument("--transposition-file", dest="transposition_file", default=None, metavar="LIST",
                        help="text file with lines `basename factor`: the factor of the files it lists, instead of "
                             "--transposition")
    parser.add_argument("--time-stretch", dest="time_stretch", default=1.0, type=stretch_arg, metavar="F",
                        help="factor on the duration at the same pitch: the output lasts F times as long (Def: %(default)s)")
    parser.add_argument("--time-stretch-file", dest="time_stretch_file", default=None, metavar="LIST",
                        help="text file with lines `basename factor`: the time-stretch factor of the files it lists, instead "
                             "of --time-stretch")
    parser.add_argument("--align-to", dest="align_to", default=None, metavar="GUIDE",
                        help="give every file the timing of the recording GUIDE: its mel frames are aligned to the guide's by "
                             "dynamic time warping and it comes out with the guide's length; excludes --time-stretch")
    parser.add_argument("--align-to-dir", dest="align_to_dir", default=None, metavar="DIR",
                        help="as --align-to, every file taking the guide DIR/<its basename>")
    parser.add_argument("--align-band", dest="align_band", default=1.0, type=band_arg, metavar="SECONDS",
                        help="how far the alignment may leave the diagonal (Def: %(default)s)")
    parser.add_argument("--formant-shift", dest="formant_shift", default=1.0, type=factor_arg, metavar="F",
                        help="factor on the formant frequencies at the same pitch and duration: F > 1 moves them up "
                             "(Def: %(default)s)")
    parser.add_argument("--formant-shift-file", dest="formant_shift_file", default=None, metavar="LIST",
                        help="text file with lines `basename factor`: the formant-shift factor of the files it lists, instead "
                             "of --formant-shift")
    parser.add_argument("--f0-source", dest="f0_source", default="net", choices=["net", "audio"],
                        help="where the pitch comes from: net = what the model infers from the mel; audio = the F0 tracker on "
                             "the sound itself, which keeps the pitch that is in the recording; --transposition multiplies on "
                             "top of either (Def: %(default)s)")
    parser.add_argument("--f0-min", dest="f0_min", default=55.0, type=hertz_arg, metavar="HZ",
                        help="lowest pitch the F0 tracker looks for (Def: %(default)s)")
    parser.add_argument("--f0-max", dest="f0_max", default=1000.0, type=hertz_arg, metavar="HZ",
                        help="highest pitch the F0 tracker looks for (Def: %(default)s)")
    parser.add_argument("--f0-fill", dest="f0_fill", default="interpolate", choices=["interpolate", "hold"],
                        help="how --f0-source audio fills unvoiced frames: interpolate = between the voiced neighbours; hold = "
                             "the last voiced value, --f0-initial in front of the first: the causal fill of "
                             "stream_transpose.py --f0-source audio, whose samples the file then has (Def: %(default)s)")
    parser.add_argument("--f0-initial", dest="f0_initial", default=150.0, type=hertz_arg, metavar="HZ",
                        help="--f0-fill hold: the pitch in front of the first voiced frame (Def: %(default)s)")
    parser.add_argument("--write-f0", dest="write_f0", action="store_true",
                        help="write the tracked contour of every file as NAME.f0 into the output directory: text rows `time_s "
                             "f0_hz periodicity`, one per mel frame, 0 = unvoiced")
    parser.add_argument("--pitch-decode", dest="pitch_decode", default="greedy", choices=["greedy", "viterbi"],
                        help="how the tracker's contour is made: greedy = every frame picks on its own; viterbi = the cheapest "
                             "path over several candidates per frame and an unvoiced state, which removes single-frame octave "
                             "jumps (Def: %(default)s)")
    parser.add_argument("--pitch-jump", dest="pitch_jump", default=4.0, type=weight_arg, metavar="W",
                        help="viterbi: weight on the relative change of period between neighbouring frames (Def: %(default)s)")
    parser.add_argument("--pitch-switch", dest="pitch_switch", default=0.5, type=weight_arg, metavar="W",
                        help="viterbi: cost of a change between voiced and unvoiced (Def: %(default)s)")
    parser.add_argument("--pitch-lag", dest="pitch_lag", default=None, type=cli.lag_arg, metavar="N",
                        help="--pitch-decode viterbi: decide every frame once N later frames are seen, 0 .. 128, as "
                             "stream_transpose.py --pitch-lag N does -- with --f0-fill hold the file then has the stream's "
                             "samples (Def: the path over the whole file)")
    parser.add_argument("--noise-seed", dest="noise_seed", default=0, type=int, metavar="S",
                        help="seed of the keyed noise: a file's noise is a function of (S, its basename, the step) "
                             "(Def: %(default)s)")
    parser.add_argument("--batch", default=16, type=int, metavar="N",
                        help="analyse and synthesise up to N files per launch in padded micro-batches (Def: %(default)s)")
    parser.add_argument("--gpus", default=1, type=int, metavar="N",
                        help="shard the files by duration over N child processes, rank r on visible GPU r %% count, each "
                             "writing its own files (Def: %(default)s)")
    parser.add_argument("-nt", "--num_threads", default=2, type=int, help="reader and writer threads (Def: %(default)s)")
    parser.add_argument("--out-rate", dest="out_rate", default=None, type=out_rate_arg, metavar="R|input",
                        help="write the files at R Hz, resampled on the GPU from the model rate; input = every file at its "
                             "own rate (Def: the model rate)")
    cli.add_level_options(parser, allow_input=True)
    parser.add_argument("--format", default="flac", help="file format for generated audio files (Def: %(default)s)")
    parser.add_argument("--flac-compression", default="verbatim", choices=["verbatim", "fixed"],
                        help="what the built-in FLAC writer emits, on the GPU: verbatim = uncompressed sub-frames; fixed = fixed "
                             "predictors with Rice codes; ignored when soundfile writes the files (Def: %(default)s)")
    parser.add_argument("--conv-form", default="auto", choices=["auto", "direct", "f23", "f43"],
                        help="form of the WaveNet's dilated convolution; pinned, a file's samples do not depend on the batch "
                             "(f23: they equal what stream_transpose.py --noise-seed streams) (Def: %(default)s)")
    parser.add_argument("--batch-invariant", action="store_true",
                        help="pin the engine's kernels so that a file's audio does not depend on the batch it ran in")
    parser.add_argument("-v", "--verbose", action="store_true", help="display verbose progress info and the time per stage")
    parser.add_argument("-q", "--quiet", action="store_true", help="dont display progress")
    parser.add_argument("--rank", type=int, default=None, help=SUPPRESS)       # set by the parent of a --gpus job
    parser.add_argument("--job", default=None, help=SUPPRESS)
    return parser


if __name__ == "__main__":
    args = make_parser().parse_args()
    if not args.model_id:
        cli.print_models()
    else:
        main(**vars(args))

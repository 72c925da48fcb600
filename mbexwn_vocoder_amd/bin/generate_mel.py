#!/usr/bin/env python3
"""Mel analysis CLI: sound files -> ``.mell`` files, the inputs of resynth_mel.py -- same flags, file naming and dictionary
as the reference's bin/generate_mel.py (reference bin/generate_mel.py:27-94), with the reference's resampler
(sig_proc/resample.py) and the mel analysis running on the MI355X HIP path.

Deviations (documented in INTEGRATION.md):
  * sound files are read with ``soundfile`` if it is installed, otherwise through the built-in readers (wav through scipy,
    flac as this package writes it; the reference uses pysndfile)
  * a file with more than one channel is refused by name (the reference raises there too)
  * additionally ``--batch N`` (padded micro-batches per input rate through the device resampler and the device analysis),
    ``-nt`` (reader / writer threads), ``--host`` (numpy analysis and host resampler, no GPU needed), ``-v``, ``-q``
  * additionally ``--time-stretch F``: the frames lie at the positions of a sound F times as long (timemap.py, DESIGN.md
    section 6f), the file has the reference's dictionary with K columns, and resynth_mel.py synthesises it F times as long at
    the same pitch; with ``--host`` too
  * additionally ``--write-f0`` (``--f0-min``, ``--f0-max``): the F0 tracker (f0track.py) runs on the
    frames of the mel and NAME.f0 is written next to NAME.mell, for ``resynth_mel.py --f0-dir``; with ``--host`` too, same bits
  * additionally ``--pitch-decode viterbi`` (``--pitch-jump``, ``--pitch-switch``): the written contour is decoded over the
    whole file (f0decode.py) instead of picked frame by frame; with ``--host`` too, same bits
  * additionally ``--align-to GUIDE`` / ``--align-to-dir DIR`` (``--align-band SECONDS``): the frames lie where the guide's
    timing puts them (align.py), the file has the guide's frame count, and resynth_mel.py synthesises
    the sound with the guide's timing; with ``--host`` too; not combinable with ``--time-stretch``
  * without ``--host`` and without a GPU the script fails loudly; there is no ``--gpus``
"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

test_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'mbexwn_vocoder_amd')
if os.path.exists(test_path):
    sys.path.insert(0, os.path.dirname(os.path.abspath(test_path)))

from mbexwn_vocoder_amd import cli, f0track, get_config_file  # noqa: E402
from mbexwn_vocoder_amd.analysis import generate_mels  # noqa: E402
from mbexwn_vocoder_amd.batched import f0_path  # noqa: E402
from mbexwn_vocoder_amd.cli import file_guides, lag_arg, pitch_decode_params  # noqa: E402,F401
from mbexwn_vocoder_amd.audioio import read_audio  # noqa: E402
from mbexwn_vocoder_amd.config import ModelDims, read_config  # noqa: E402
from mbexwn_vocoder_amd.fileio import save_var  # noqa: E402
from mbexwn_vocoder_amd.timemap import check_factor  # noqa: E402


def main(input_audio_files, output_dir, model_id="VOICE", batch=1, num_threads=2, host=False, verbose=False, quiet=False,
         time_stretch=1.0, write_f0=False, f0_min=55.0, f0_max=1000.0, pitch_decode="greedy", pitch_jump=4.0, pitch_switch=0.5,
         align_to=None, align_to_dir=None, align_band=1.0, pitch_lag=None):
    config = read_config(config_file=get_config_file(model_id_or_path=model_id))
    preprocess_config = config['preprocess_config']
    try:
        time_stretch = check_factor(time_stretch, "--time-stretch")
        # a stretched file is made for resynth_mel.py: held to the limit of the model's engine (sub-band rows per frame)
        rows_per_frame = ModelDims(config).steps_per_frame if time_stretch != 1.0 else 1
        f0_params = f0track.params(int(preprocess_config["sample_rate"]), f0_min=f0_min, f0_max=f0_max) if write_f0 else None
        # (greedy: the weights are not looked at, as before there was a decoder)
        f0_decode = None if pitch_decode == "greedy" else pitch_decode_params(pitch_decode, pitch_jump, pitch_switch)
        if f0_decode is not None and not write_f0:
            raise ValueError("--pitch-decode viterbi decodes the contour that --write-f0 writes: it needs --write-f0")
        if pitch_lag is not None and f0_decode is None:
            raise ValueError("--pitch-lag is the look-ahead of the decoder: it needs --pitch-decode viterbi")
        guide_of = file_guides(input_audio_files, align_to, align_to_dir, align_band, time_stretch)
        if guide_of is not None:
            rows_per_frame = ModelDims(config).steps_per_frame
            guide_of = dict(zip(input_audio_files, guide_of))
    except ValueError as err:
        print(f"generate_mel::error:: {err}", file=sys.stderr)
        sys.exit(1)
    missing = [ff for ff in input_audio_files + sorted(set((guide_of or {}).values())) if not os.path.isfile(ff)]
    if missing:
        print(f"generate_mel::error:: no such file: {', '.join(missing)}", file=sys.stderr)
        sys.exit(1)
    if not host:
        import torch
        if not torch.cuda.is_available():
            print("generate_mel::error:: no GPU available; --host runs the numpy analysis", file=sys.stderr)
            sys.exit(1)
    if output_dir and not os.path.exists(output_dir):
        os.makedirs(output_dir)
    batch, threads = max(1, int(batch)), max(1, int(num_threads))
    seconds = {"read": 0.0, "write": 0.0}
    stats = {} if verbose else None

    def read(path):
        t0 = time.perf_counter()
        snd, rate = read_audio(path)
        if snd.size == 0:
            raise ValueError(f"{path}: no samples")
        return snd, rate, time.perf_counter() - t0

    def timed(func, *args):
        t0 = time.perf_counter()
        func(*args)
        return time.perf_counter() - t0

    guide_sound = lru_cache(maxsize=None)(lambda path: read(path)[:2])           # a guide shared by many files is read once
    t_start = time.perf_counter()
    samples = 0
    unaligned = []
    windows = [input_audio_files[ii:ii + batch] for ii in range(0, len(input_audio_files), batch)]
    with ThreadPoolExecutor(max_workers=threads) as readers, ThreadPoolExecutor(max_workers=threads) as writers:
        pending = [readers.submit(read, ff) for ff in windows[0]] if windows else []
        written = []
        for wi, files in enumerate(windows):
            loaded = [fu.result() for fu in pending]
            # the next window is read while this one is analysed
            pending = [readers.submit(read, ff) for ff in windows[wi + 1]] if wi + 1 < len(windows) else []
            seconds["read"] += sum(ll[2] for ll in loaded)
            if not quiet:
                for ff in files:
                    print(f"process {ff}", file=sys.stderr)
            try:
                tracked = [] if write_f0 else None
                aligned = {}
                pairs = [(None, None) if guide_of is None else guide_sound(guide_of[ff]) for ff in files]
                mells = generate_mels([ll[0] for ll in loaded], [ll[1] for ll in loaded], preprocess_config, on_device=not host,
                                      batch=batch, stats=stats, rows_per_frame=rows_per_frame,
                                      time_maps=None if time_stretch == 1.0 else [time_stretch] * len(loaded),
                                      f0_out=tracked, f0_params=f0_params, f0_decode=f0_decode,
                                      guides=[pp[0] for pp in pairs], guide_rates=[pp[1] for pp in pairs],
                                      align_band_s=align_band, align_out=aligned, f0_lag=pitch_lag)
            except ValueError as err:
                print(f"generate_mel::error:: {err}", file=sys.stderr)
                sys.exit(1)
            for local, (ff, ll, dd) in enumerate(zip(files, loaded, mells)):
                note = aligned.get(local)
                if dd is None:                              # cannot be aligned: reported, skipped, exit status 1
                    print(f"generate_mel::error:: skipped {ff}: {note['error']} (guide {guide_of[ff]})", file=sys.stderr)
                    unaligned.append(ff)
                    continue
                if note is not None and verbose:
                    print(f"    aligned to {guide_of[ff]}: {note['nodes']} nodes, mean cost per node {note['mean_cost']:.3f}, "
                          f"largest offset from the diagonal {note['max_offset_ms']:.1f} ms", file=sys.stderr)
                outfile = os.path.join(output_dir, os.path.splitext(os.path.basename(ff))[0] + ".mell")
                samples += ll[0].size / ll[1]
                if verbose:
                    print(f"    {ll[0].size} samples at {ll[1]} Hz -> {dd['mell'].shape[1]} frames, save under {outfile}",
                          file=sys.stderr)
                written.append(writers.submit(timed, save_var, outfile, dd))
            for ff, contour in zip(files, tracked or []):
                if contour is None:
                    continue
                times = f0track.frame_times(contour[0].size, preprocess_config["hop_size"], preprocess_config["sample_rate"])
                written.append(writers.submit(timed, f0track.write_f0, f0_path(ff, output_dir), times, *contour))
        seconds["write"] = sum(fu.result() for fu in written)
    if verbose:
        wall = time.perf_counter() - t_start
        where = "host" if host else "device"
        print(f"generate_mel: {len(input_audio_files)} files, {samples:.1f} s of audio in {wall:.2f} s wall "
              f"({samples / max(wall, 1e-9):.1f} x real time); read {seconds['read']:.2f} s, "
              + (f"upload {stats.get('upload', 0.0):.3f} s, " if not host else "")
              + f"{where} resample {stats.get('resample', 0.0):.3f} s, {where} analysis {stats.get('analysis', 0.0):.3f} s, "
              + (f"copy-back {stats.get('copy_back', 0.0):.3f} s, " if not host else "")
              + f"write {seconds['write']:.2f} s (read and write summed over {threads} threads each)", file=sys.stderr)
    if unaligned:
        sys.exit(1)


def make_parser():
    from argparse import ArgumentParser

    class Parser(ArgumentParser):
        """The align flags exclude the time stretch: refused at parse time, with exit status 2."""

        def parse_args(self, args=None, namespace=None):
            parsed = super().parse_args(args, namespace)
            try:
                file_guides([], parsed.align_to, parsed.align_to_dir, parsed.align_band, parsed.time_stretch)
            except ValueError as err:
                self.error(str(err))
            return parsed

    parser = Parser(description="create mel analysis from sound files using the analysis configuration of a model")
    parser.add_argument("input_audio_files", nargs="+", help="input files to process")
    parser.add_argument("-o", "--output_dir", required=True, help="output directory where the .mell files will be stored")
    parser.add_argument("--model_id", default="VOICE", nargs="?", const="",
                        help="model identifier or path to a model directory whose config.yaml holds the analysis "
                             "configuration; all models share it, so the default is fine. Given without a value the script "
                             "lists all known models. (Def: %(default)s)")
    parser.add_argument("--batch", default=1, type=int, metavar="N",
                        help="analyse up to N files per launch, grouped by input rate, in padded micro-batches "
                             "(Def: %(default)s = one file at a time)")
    parser.add_argument("-nt", "--num_threads", default=2, type=int, help="reader and writer threads (Def: %(default)s)")
    parser.add_argument("--time-stretch", dest="time_stretch", default=1.0, type=float, metavar="F",
                        help="place the frames for a sound F times as long at the same pitch (Def: %(default)s)")
    parser.add_argument("--align-to", dest="align_to", default=None, metavar="GUIDE",
                        help="place the frames where the timing of the recording GUIDE puts them: the .mell has the guide's "
                             "frame count; excludes --time-stretch")
    parser.add_argument("--align-to-dir", dest="align_to_dir", default=None, metavar="DIR",
                        help="as --align-to, every file taking the guide DIR/<its basename>")
    parser.add_argument("--align-band", dest="align_band", default=1.0, type=float, metavar="SECONDS",
                        help="how far the alignment may leave the diagonal (Def: %(default)s)")
    parser.add_argument("--write-f0", dest="write_f0", action="store_true",
                        help="also track the pitch of every file from its samples and write NAME.f0 next to NAME.mell: text "
                             "rows `time_s f0_hz periodicity`, one per mel frame, 0 = unvoiced; resynth_mel.py --f0-dir reads it")
    parser.add_argument("--f0-min", dest="f0_min", default=55.0, type=float, metavar="HZ",
                        help="lowest pitch the F0 tracker looks for (Def: %(default)s)")
    parser.add_argument("--f0-max", dest="f0_max", default=1000.0, type=float, metavar="HZ",
                        help="highest pitch the F0 tracker looks for (Def: %(default)s)")
    parser.add_argument("--pitch-decode", dest="pitch_decode", default="greedy", choices=["greedy", "viterbi"],
                        help="--write-f0: greedy = every frame picks on its own; viterbi = the cheapest path over several "
                             "candidates per frame and an unvoiced state (Def: %(default)s)")
    parser.add_argument("--pitch-jump", dest="pitch_jump", default=4.0, type=float, metavar="W",
                        help="viterbi: weight on the relative change of period between neighbouring frames (Def: %(default)s)")
    parser.add_argument("--pitch-switch", dest="pitch_switch", default=0.5, type=float, metavar="W",
                        help="viterbi: cost of a change between voiced and unvoiced (Def: %(default)s)")
    parser.add_argument("--pitch-lag", dest="pitch_lag", default=None, type=lag_arg, metavar="N",
                        help="--pitch-decode viterbi: decide every frame once N later frames are seen, 0 .. 128: the contour "
                             "of a live stream with that lag (Def: the path over the whole file)")
    parser.add_argument("--host", action="store_true", help="numpy analysis and host resampler; needs no GPU")
    parser.add_argument("-v", "--verbose", action="store_true", help="display verbose progress info")
    parser.add_argument("-q", "--quiet", action="store_true", help="dont display progress")
    return parser


if __name__ == "__main__":
    args = make_parser().parse_args()

    if not args.model_id:
        cli.print_models()
    else:
        main(**vars(args))

#!/usr/bin/env python3
"""Mel-spectrogram inversion CLI -- same flags and file naming as the reference's bin/resynth_mel.py
(reference bin/resynth_mel.py:34-135), running on the MI355X HIP path.

Deviations (documented in INTEGRATION.md):
  * this build has only the GPU path: ``-g`` is accepted and implied; without a GPU the script fails loudly
  * ``-nt`` (TensorFlow CPU threads) is accepted and ignored
  * audio files are written with ``soundfile`` if it is installed, otherwise through the built-in writers (flac: 16-bit
    VERBATIM frames, or with ``--flac-compression fixed`` fixed predictors and Rice codes, about half the size on speech;
    wav: float32 through scipy; the reference uses pysndfile, default format flac)
  * additionally ``--batch N`` (padded micro-batches, FLAC frames encoded on the GPU, reader / writer pools of -nt
    threads), ``--gpus N`` (the files sharded over N child processes by frames) and ``--batch-invariant``
  * additionally ``--noise-seed S`` (keyed noise, include/mbexwn_noise.h) and ``--transposition F``
  * additionally ``--out-rate R``: the files are written at R Hz, resampled on the GPU from the model rate with the
    reference's resampler (mbexwn_vocoder_amd/resample.py)
  * additionally ``--f0-dir DIR``: every file takes its pitch from ``DIR/NAME.f0`` (``generate_mel.py --write-f0``; text rows
    ``time_s f0_hz periodicity``, one per mel frame, 0 = unvoiced and filled from its neighbours) instead of the model's own F0
  * additionally ``--loudness LUFS``, ``--peak-limit DBFS`` and ``--true-peak`` (mbexwn_vocoder_amd/level.py; DESIGN.md section
    6m): every file is written at that BS.1770 loudness and / or below that peak, by one gain per file measured and applied on
    the GPU; such a job runs through the micro-batches, of one file with ``--batch 1``, and the writer reports the level in
    place of the clipping note
"""
import json
import os
import sys
import time

import numpy as np

test_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'mbexwn_vocoder_amd')
if os.path.exists(test_path):
    sys.path.insert(0, os.path.dirname(os.path.abspath(test_path)))

from mbexwn_vocoder_amd import cli, mel_inverter  # noqa: E402
from mbexwn_vocoder_amd.batched import load_contour, write_audio  # noqa: E402 -- the one-at-a-time loop's
from mbexwn_vocoder_amd.level import level_control  # noqa: E402
from mbexwn_vocoder_amd.noise import item_key  # noqa: E402
from mbexwn_vocoder_amd.fileio import load_var  # noqa: E402


def main(model_id, input_mell_files, output_dir, use_gpu=False, sigma=None, format=None, verbose=False, seed=42,
         num_threads=2, quiet=False, calibrate=0, batch=1, gpus=1, batch_invariant=False, conv_form="auto", rank=None, job=None,
         flac_compression="verbatim", out_rate=None, noise_seed=None, transposition=None, formant_shift=None, f0_dir=None,
         loudness=None, peak_limit=None, true_peak=False, limiter=False, limiter_lookahead=None, limiter_hold=None):
    values = dict(locals())
    format = format or "flac"                                   # the reference's default (bin/resynth_mel.py:119)
    try:
        level = level_control(loudness, peak_limit, true_peak, limiter, limiter_lookahead, limiter_hold)
        cli.check_limiter_rate(model_id, out_rate, limiter, limiter_lookahead, limiter_hold, true_peak)
    except ValueError as err:
        print(f"resynth_mel::error:: {err}", file=sys.stderr)
        sys.exit(1)
    if flac_compression != "verbatim" and rank is None and not quiet:
        from mbexwn_vocoder_amd.batched import have_soundfile
        if format.lower() != "flac" or have_soundfile():
            print("resynth_mel::note:: --flac-compression is ignored: " + ("soundfile writes the files and compresses FLAC "
                  "by itself" if format.lower() == "flac" else f"the format is {format}"), file=sys.stderr)
    if gpus > 1 and rank is None:
        # --gpus N: this parent never initialises HIP; N fresh child processes write their share of the files each
        # (the model is the positional; the files follow -i like any other option)
        from mbexwn_vocoder_amd import batched
        argv = cli.rank_argv(make_parser(), dict(values, format=format), [model_id])
        sys.exit(batched.run_ranks(os.path.abspath(__file__), argv, model_id, input_mell_files, gpus, threads=num_threads,
                                   quiet=quiet))
    import torch
    if not torch.cuda.is_available():
        print("resynth_mel::error:: no GPU available; this build has no CPU path", file=sys.stderr)
        sys.exit(1)
    if not use_gpu and not quiet:
        print("resynth_mel::note:: running on the MI355X HIP path (this build has no CPU path, -g is implied)",
              file=sys.stderr)
    plan = None
    if job is not None:                                       # a rank of a --gpus job: its device and its files
        with open(job) as fo:
            plan = json.load(fo)
        torch.cuda.set_device(rank % plan["devices"])
    if num_threads:                                           # -nt: host threads (numpy / torch CPU work around the HIP path)
        torch.set_num_threads(max(1, int(num_threads)))
        try:
            from threadpoolctl import threadpool_limits
            threadpool_limits(limits=max(1, int(num_threads)))
        except ImportError:
            pass
    if seed >= 0:                                  # reference :65-67
        np.random.seed(seed)
        torch.manual_seed(seed)

    MelInv = mel_inverter.MELInverter(model_id_or_path=model_id, verbose=verbose,
                                      batch_invariant=True if batch_invariant else None,
                                      conv_form=None if conv_form == "auto" else conv_form)
    if output_dir:
        os.makedirs(output_dir, exist_ok=True)
    if calibrate and input_mell_files:
        # --calibrate N (this build): the form of the WaveNet's convolution is decided on the first N mels of the job
        # (MELInverter.calibrate -> mbx_calibrate) instead of on the synthetic mel of the engine's creation
        first = [MelInv.scale_mel(load_var(ff)) for ff in input_mell_files[:int(calibrate)]]
        info = MelInv.calibrate(first, verbose=verbose)
        if not quiet and not verbose:
            print(f"calibrated on {len(first)} file(s): convolution form {info['form']}", file=sys.stderr)

    if batch > 1 or plan is not None or level is not None:     # the level stage lives in the micro-batches, of one file too
        from mbexwn_vocoder_amd.batched import run_job
        run_job(MelInv, input_mell_files, output_dir, format, frames=plan["frames"] if plan else None,
                mine=plan["shards"][rank] if plan else None, batch=batch, threads=num_threads, verbose=verbose, quiet=quiet,
                flac_compression=flac_compression, out_rate=out_rate, noise_seed=noise_seed, transposition=transposition,
                formant=formant_shift, f0_dir=f0_dir, level=level)
        return
    out_rate = MelInv._output_rate(out_rate)

    for mell_file in input_mell_files:
        outfile = os.path.join(output_dir or "", "syn_" + os.path.splitext(os.path.basename(mell_file))[0] + "." + format)
        if not quiet:
            print(f"synthesize {mell_file} into {outfile}", file=sys.stderr)
        if verbose:
            print(f"load mell  from {mell_file}", file=sys.stderr)
        dd = load_var(mell_file)
        log_mel_spectrogram = MelInv.scale_mel(dd, verbose=verbose)

        start_time = time.time()
        # keyed noise: a function of the seed, the file's basename and the step; the factor on every mel frame, as run_job
        # applies it (a formant factor of 1: the call without it); the file's own contour in place of the F0-net's (none
        # voiced: the F0-net)
        rows = None if transposition is None else np.full(log_mel_spectrogram.shape[1], transposition, dtype=np.float32)
        contour = None if f0_dir is None else load_contour(mell_file, f0_dir, log_mel_spectrogram.shape[1])
        syn_audio = MelInv.synth_from_mel(log_mel_spectrogram, noise_seed=noise_seed, noise_key=item_key(mell_file),
                                          transposition=rows, formant=None if formant_shift == 1.0 else formant_shift, f0=contour)
        end_time = time.time()

        if verbose:                                  # reference :90-96
            mel_resyn = MelInv.generate_mel_from_snd(syn_audio, srate=MelInv.srate)['mell'].T[np.newaxis]
            mell_err = mel_inverter.log_to_db * np.mean(np.abs(log_mel_spectrogram
                                                               - mel_resyn[:, :log_mel_spectrogram.shape[1]]))
            print(f"    synthesized audio with {syn_audio.size} samples in {end_time - start_time:.3f}s "
                  f"({syn_audio.size / (end_time - start_time):.2f}Hz), mel_error: {mell_err:.3f}dB", file=sys.stderr)
        if out_rate is not None:                     # --out-rate: what is written is the resampled audio (mel_error above is not)
            syn_audio = MelInv._to_rate(torch.as_tensor(syn_audio[np.newaxis]).to(MelInv.model.device), out_rate)[0].cpu().numpy()
        if np.max(np.abs(syn_audio)) > 1:
            norm = 0.99 / np.max(np.abs(syn_audio))
            print(f'    to prevent clipping you would need to normalize {outfile} by {norm:.3f}', file=sys.stderr)
        if verbose:
            print(f"    save audio under {outfile}", file=sys.stderr)
        write_audio(outfile, syn_audio, MelInv.srate if out_rate is None else out_rate, format, flac_compression)


positive_factor = cli.positive_arg("factor")
positive_rate = cli.rate_arg()


def make_parser():
    from argparse import SUPPRESS, ArgumentParser
    parser = ArgumentParser(description="invert mel spectrograms into audio with an MBExWN model (MI355X HIP path)")
    parser.add_argument("model_id", default=None, nargs="?", const=None,
                        help="model identifier or path to a model directory. If not given the script lists all known "
                             "model names; the first model whose DOMAIN/name contains the identifier is used.")
    parser.add_argument("-i", "--input_mell_files", nargs="+", help="list of mell spectra stored in pickle files")
    parser.add_argument("-o", "--output_dir", help="output directory where synthetic sounds will be stored")
    parser.add_argument("--format", default="flac", help="file format for generated audio files (Def: %(default)s)")
    parser.add_argument("-nt", "--num_threads", default=2, type=int,
                        help="number of cpu threads of the host-side work (Def: %(default)s)")
    parser.add_argument("-g", "--use_gpu", action="store_true", help="run on gpu (implied)")
    parser.add_argument("-v", "--verbose", action="store_true", help="display verbose progress info")
    parser.add_argument("-q", "--quiet", action="store_true", help="dont display progress")
    parser.add_argument("--calibrate", default=0, type=int, metavar="N",
                        help="decide the form of the WaveNet's convolution on the first N input files before synthesis "
                             "(Def: %(default)s = keep the decision made at model load on a synthetic mel); the decision then "
                             "binds every file of the job, so the output depends on which N files come first")
    parser.add_argument("--batch", default=1, type=int, metavar="N",
                        help="synthesise up to N files per launch in padded micro-batches, with the FLAC frames encoded on "
                             "the GPU and reader / writer pools of -nt threads (Def: %(default)s = one file at a time)")
    parser.add_argument("--gpus", default=1, type=int, metavar="N",
                        help="shard the files by frames over N child processes, rank r on visible GPU r %% count, each "
                             "writing its own files (Def: %(default)s)")
    parser.add_argument("--batch-invariant", action="store_true",
                        help="pin the engine's kernels so that a file's audio does not depend on the batch it ran in: with "
                             "this flag on both sides, batched files are bit-identical to one-at-a-time files")
    parser.add_argument("--conv-form", default="auto", choices=["auto", "direct", "f23", "f43"],
                        help="form of the WaveNet's dilated convolution: auto = calibrated at model load; a causal model "
                             "(force_causal) runs its Winograd kernels only when f23 / f43 is pinned (Def: %(default)s)")
    parser.add_argument("--flac-compression", default="verbatim", choices=["verbatim", "fixed"],
                        help="what the built-in FLAC writer emits: verbatim = uncompressed sub-frames, the size of a wav; fixed "
                             "= fixed predictors of orders 0-4 with Rice codes, on the GPU with --batch / --gpus; ignored when "
                             "soundfile writes the files (Def: %(default)s)")
    parser.add_argument("--out-rate", dest="out_rate", default=None, type=positive_rate, metavar="R",
                        help="write the files at R Hz: the audio is resampled on the GPU from the model rate with the "
                             "reference's resampler; with -v, mel_error stays computed on the model-rate audio, the clipping "
                             "note is about what is written (Def: the model rate)")
    parser.add_argument("--noise-seed", dest="noise_seed", default=None, type=int, metavar="S",
                        help="draw the noise channel keyed by (S, the .mell file's basename, the step): a file's audio then "
                             "does not depend on the other files of the job or their order (Def: the draws of the "
                             "one-at-a-time loop)")
    parser.add_argument("--transposition", default=None, type=positive_factor, metavar="F",
                        help="factor on the pitch, applied to every mel frame (Def: none)")
    parser.add_argument("--formant-shift", dest="formant_shift", default=None, type=positive_factor, metavar="F",
                        help="factor on the formant frequencies at the same pitch, applied to every mel frame: F > 1 moves "
                             "them up (Def: none)")
    parser.add_argument("--f0-dir", dest="f0_dir", default=None, metavar="DIR",
                        help="take the pitch of every file from DIR/NAME.f0 (as generate_mel.py --write-f0 writes it: text rows "
                             "`time_s f0_hz periodicity`, one per mel frame, 0 = unvoiced, filled from its neighbours) instead of "
                             "the model's own F0; --transposition multiplies on top (Def: none)")
    cli.add_level_options(parser)                              # no source sound here: --loudness input is refused by name
    parser.add_argument("--rank", type=int, default=None, help=SUPPRESS)       # set by the parent of a --gpus job
    parser.add_argument("--job", default=None, help=SUPPRESS)
    return parser


if __name__ == "__main__":
    args = make_parser().parse_args()
    if not args.model_id:
        cli.print_models(" for mel inversion", "\nFor example just specifying SPEECH will select the default SPEECH model.")
    else:
        main(**vars(args))

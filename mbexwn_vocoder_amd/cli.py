"""What the command-line tools under ``bin/`` share: argparse types, the guide, pitch-decode and level options, the model listing
and the argv of a ``--gpus`` rank.  Plain functions; nothing here imports torch (the parent of a ``--gpus`` job never does)."""
import os
from argparse import ArgumentTypeError  # noqa: F401  (the tools catch it by this name)


def _number(text):
    try:
        return float(text)
    except ValueError:
        return float("nan")


def positive_arg(what):
    """argparse type "a finite positive number"; ``what`` names it in the refusal: factor, frequency in Hz, number of seconds."""
    def parse(text):
        value = _number(text)
        if not (value > 0 and value != float("inf")):
            raise ArgumentTypeError(f"a finite positive {what} is expected, got {text!r}")
        return value
    return parse


def rate_arg(allow_input=False):
    """argparse type of an output rate: a positive whole number of Hz, with ``allow_input`` also the word "input"."""
    words = "a sample rate in Hz or 'input'" if allow_input else "a sample rate in Hz"

    def parse(text):
        if allow_input and text == "input":
            return text
        try:
            rate = int(text)
        except ValueError:
            raise ArgumentTypeError(f"{words} is expected, got {text!r}") from None
        if rate <= 0:
            raise ArgumentTypeError(f"a sample rate must be positive, got {rate}")
        return rate
    return parse


def weight_arg(text):
    """argparse type of --pitch-jump and --pitch-switch: a weight in [0, 1e6]."""
    value = _number(text)
    if not 0.0 <= value <= 1e6:
        raise ArgumentTypeError(f"a weight in 0 .. 1e6 is expected, got {text!r}")
    return value


def lag_arg(text):
    """argparse type of --pitch-lag: the decoder's look-ahead, a whole number of frames in 0 .. 128."""
    try:
        value = int(text)
    except ValueError:
        value = -1
    if not 0 <= value <= 128:
        raise ArgumentTypeError(f"a whole number of frames in 0 .. 128 is expected, got {text!r}")
    return value


def loudness_arg(allow_input=False):
    """argparse type of --loudness: a finite number of LUFS, with ``allow_input`` also the word "input".  A tool without a
    source sound refuses "input" by name."""
    def parse(text):
        if text == "input":
            if allow_input:
                return text
            raise ArgumentTypeError("'input' is the loudness of the source sound, and this tool reads none: a number of "
                                    "LUFS is expected")
        value = _number(text)
        if value != value or value in (float("inf"), float("-inf")):
            raise ArgumentTypeError("a loudness in LUFS" + (" or 'input'" if allow_input else "") + f" is expected, got {text!r}")
        return value
    return parse


def decibel_arg(text):
    """argparse type of --peak-limit: a finite number of dBFS."""
    value = _number(text)
    if value != value or value in (float("inf"), float("-inf")):
        raise ArgumentTypeError(f"a peak level in dBFS is expected, got {text!r}")
    return value


def add_level_options(parser, allow_input=False):
    """--loudness, --peak-limit and --true-peak (level.py) and --limiter, --limiter-lookahead and
    --limiter-hold (limiter.py; section 6n), the same in every file tool; what they say together -- the default of
    --peak-limit, --true-peak without a peak to limit, a window without --limiter -- is ``level.check_options``."""
    parser.add_argument("--loudness", default=None, type=loudness_arg(allow_input), metavar="LUFS|input" if allow_input else "LUFS",
                        help="write every file at this BS.1770 integrated loudness, measured and gained on the GPU"
                             + ("; input = at the loudness of its source sound" if allow_input else "")
                             + " (Def: the level the model gives)")
    parser.add_argument("--peak-limit", dest="peak_limit", default=None, type=decibel_arg, metavar="DBFS",
                        help="no file peaks above DBFS: a file that would is scaled down as a whole; usable without "
                             "--loudness, where it only ever scales down (Def: -1.0 with --loudness, else none)")
    parser.add_argument("--true-peak", dest="true_peak", action="store_true",
                        help="--peak-limit is about the true peak, the maximum of the signal at four times its rate, not the "
                             "sample peak")
    parser.add_argument("--limiter", action="store_true",
                        help="keep the ceiling with a look-ahead peak limiter on the GPU in place of one gain for the whole "
                             "file, so that a --loudness stands although single peaks are in its way; brings --peak-limit -1.0 "
                             "along, with or without --loudness")
    parser.add_argument("--limiter-lookahead", dest="limiter_lookahead", default=None, type=positive_ms_arg, metavar="MS",
                        help="the limiter's look-ahead, the time its gain takes to come down in front of a peak (Def: 1.5)")
    parser.add_argument("--limiter-hold", dest="limiter_hold", default=None, type=positive_ms_arg, metavar="MS",
                        help="the limiter's hold, the time its gain stays down behind a peak: peaks that repeat within it see "
                             "one constant gain (Def: 20)")


def positive_ms_arg(text):
    """argparse type of --limiter-lookahead and --limiter-hold: a finite positive number of milliseconds."""
    value = _number(text)
    if not (0 < value < float("inf")):
        raise ArgumentTypeError(f"a positive time in ms is expected, got {text!r}")
    return value


def check_limiter_rate(model_id, out_rate, limiter, lookahead_ms, hold_ms, true_peak):
    """ValueError when the limiter's window is refused at the rate the files are written at, from the model's configuration
    alone: before a model is loaded.  ``out_rate`` "input" is every file's own rate, which the job checks once they are read."""
    if limiter and out_rate != "input":
        from . import get_config_file
        from .config import read_config
        from .limiter import check_rates
        rate = read_config(config_file=get_config_file(model_id_or_path=model_id))["preprocess_config"]["sample_rate"]
        check_rates([rate if out_rate is None else out_rate], lookahead_ms, hold_ms, true_peak)


def file_guides(files, align_to=None, align_to_dir=None, align_band=1.0, time_stretch=1.0, time_stretch_file=None,
                stretch_flags="--time-stretch"):
    """The guide of every file: ``align_to`` for all, or ``align_to_dir/<basename>``; None without either flag.  ValueError
    for both flags, for a guide beside a time stretch (``stretch_flags``: how the tool names what it excludes), for a band
    that is not finite and positive."""
    if align_to is None and align_to_dir is None:
        return None
    if align_to is not None and align_to_dir is not None:
        raise ValueError("--align-to and --align-to-dir exclude each other")
    if time_stretch != 1.0 or time_stretch_file:
        raise ValueError(f"--align-to / --align-to-dir set the timing of a file: not combinable with {stretch_flags}")
    band = float(align_band)
    if not (band > 0 and band != float("inf")):
        raise ValueError(f"--align-band: a finite positive number of seconds is expected, got {align_band!r}")
    return [align_to if align_to is not None else os.path.join(align_to_dir, os.path.basename(ff)) for ff in files]


def pitch_decode_params(pitch_decode, pitch_jump, pitch_switch):
    """None for --pitch-decode greedy, else the ``f0decode.decode_params`` dictionary of the three flags."""
    if pitch_decode not in ("greedy", "viterbi"):
        raise ValueError(f"--pitch-decode must be greedy or viterbi, got {pitch_decode!r}")
    from . import f0decode
    dec = f0decode.decode_params(w_jump=pitch_jump, w_switch=pitch_switch)               # checked with either choice
    return dec if pitch_decode == "viterbi" else None


def print_models(purpose="", example=""):
    """What a tool prints when ``model_id`` is given without a value: the known models."""
    from . import list_models
    print(f"Please select one of the following models{purpose}.\nYou don't need to select with a full ID. "
          f"The first model containing the model_id you provide will be selected.{example}")
    for kk, ll in list_models().items():
        for md in ll:
            print(f" - {kk}/{md}")


def rank_argv(parser, values, files, drop=("gpus", "rank", "job"), always=()):
    """The argv of a rank of a ``--gpus`` job, from the parser's own actions and ``values`` (``main``'s arguments by name): the
    positionals are replaced by ``files``; every option whose value differs from its default -- and every one named in
    ``always`` -- follows with its first option string, floats as ``repr(float)``, a list as one word per entry, a
    store-true flag as the flag alone.  The options in ``drop`` are the parent's own."""
    argv = [str(ff) for ff in files]
    for action in parser._actions:
        if not action.option_strings or action.dest in drop or action.dest not in values:
            continue
        value = values[action.dest]
        if value == action.default and action.dest not in always:
            continue
        if action.nargs == 0:
            argv += [action.option_strings[0]] if value else []
            continue
        words = value if isinstance(value, (list, tuple)) else [value]
        argv += [action.option_strings[0], *(repr(float(ww)) if isinstance(ww, float) else str(ww) for ww in words)]
    return argv

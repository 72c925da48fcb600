"""Reading sound files for the analysis side (reference bin/generate_mel.py:56: ``sndio.read(file, dtype=float32)``).

The reference reads through pysndfile on top of libsndfile.  Here ``soundfile`` (the same library) is used where it is
installed; otherwise the two formats this package itself writes are built in: ``.wav`` through scipy with libsndfile's
scaling of integer samples to [-1, 1), and ``.flac`` through ``flac.decode`` (mono 16-bit streams of uncompressed
sub-frames: what ``resynth_mel.py`` writes without soundfile).
"""
import os

import numpy as np


def _mono(data, path):
    data = np.asarray(data)
    if data.ndim > 1 and data.shape[1] == 1:
        data = data[:, 0]
    if data.ndim != 1:
        # the reference's analysis refuses such input too (reference preprocess.py:483-485)
        raise ValueError(f"{path}: {data.shape[1]} channels; the mel analysis takes mono files only")
    return data


def _wav_to_float(data, path):
    """libsndfile's normalisation of PCM to float: int16 / 2^15, int32 / 2^31, uint8 (x - 128) / 2^7; floats pass."""
    if data.dtype == np.int16:
        return data.astype(np.float32) / np.float32(32768.0)
    if data.dtype == np.int32:
        return (data.astype(np.float64) / 2147483648.0).astype(np.float32)
    if data.dtype == np.uint8:
        return (data.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
    if np.issubdtype(data.dtype, np.floating):
        return data.astype(np.float32, copy=False)
    raise ValueError(f"{path}: unsupported wav sample type {data.dtype}; install soundfile to read it")


def read_audio(path):
    """``(float32 mono samples, sample rate)`` of a sound file; a file with more than one channel raises ``ValueError``."""
    try:
        import soundfile
    except ImportError:
        soundfile = None
    if soundfile is not None:
        data, rate = soundfile.read(path, dtype="float32", always_2d=False)
        return np.ascontiguousarray(_mono(data, path), dtype=np.float32), int(rate)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".wav":
        import warnings
        from scipy.io import wavfile
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", wavfile.WavFileWarning)       # chunks behind the data are not an error
            rate, data = wavfile.read(path)
        return np.ascontiguousarray(_wav_to_float(_mono(data, path), path)), int(rate)
    if ext == ".flac":
        from . import flac
        with open(path, "rb") as fi:
            try:
                pcm, rate = flac.decode(fi.read())
            except ValueError as err:
                raise ValueError(f"{path}: {err}") from None
        return _wav_to_float(pcm, path), rate
    raise RuntimeError(f"cannot read {path}: soundfile is not installed, only .wav and .flac (as this package writes them) "
                       "are built in")

#!/usr/bin/env python3
"""Golden vectors of the reference's own magnitude STFT on SHORT signals (reference MBExWN_NVoc/sig_proc/spec/stft.py:14-96,
calc_stft(center=True, pad_mode="reflect", do_mag=True)): signals of 1 .. 601 samples, shorter than, equal to and just
longer than a hop, half a window and the reflect period, where np.pad reflects more than once.  Two analysis geometries
(window / hop / FFT): 1200 / 300 / 2048 and 800 / 200 / 1024; float32 and float64 runs.

Keys: "<win>_<hop>_<fft>/n<length>/snd" (float32 signal), ".../mag32", ".../mag64" ((frames, fft / 2 + 1)).
Writes tests/golden/reference_stft_short.npz.   (build container only; needs /root/reference)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import tf_numpy_shim as shim  # noqa: E402

LENGTHS = (1, 2, 3, 299, 300, 301, 599, 600, 601)
GEOMETRIES = ((1200, 300, 2048), (800, 200, 1024))


def main():
    shim.install("/root/reference")
    from MBExWN_NVoc.sig_proc.spec.stft import calc_stft
    out = {}
    for gi, (win, hop, fft) in enumerate(GEOMETRIES):
        for nn in LENGTHS:
            rng = np.random.default_rng(1000 * (gi + 1) + nn)
            snd = rng.normal(size=nn).astype(np.float32)
            key = f"{win}_{hop}_{fft}/n{nn}"
            out[key + "/snd"] = snd
            for tag, ftype in (("mag32", np.float32), ("mag64", np.float64)):
                out[f"{key}/{tag}"] = calc_stft(snd, win_len=win, hop_len=hop, fft_size=fft, win_type="hann", center=True,
                                                pad_mode="reflect", do_mag=True, axis=-1, dtype=ftype)
            print(key, out[key + "/mag64"].shape, out[key + "/mag32"].dtype)
    np.savez_compressed(os.path.join(HERE, "reference_stft_short.npz"), **out)


if __name__ == "__main__":
    main()

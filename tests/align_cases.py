"""The sounds and the analysis configuration the alignment tests share (tests/test_align_host.py, tests/test_gpu_align.py):
a synthetic "score" of sung syllables rendered at score time (the source) and at a warped time (the guide), so that the map
an alignment should recover is known."""
import functools

import numpy as np

RATE, HOP, WIN, FFT, MELS = 24000, 300, 1200, 2048, 80
PRE = {"sample_rate": RATE, "hop_size": HOP, "win_size": WIN, "fft_size": FFT, "mel_channels": MELS, "fmin": 0.0, "fmax": None,
       "lin_amp_off": 1e-5, "lin_amp_scale": 1.0, "mel_amp_scale": 1.0}
SECONDS, SYLLABLES, SYLLABLE_S, HARMONICS = 8.0, 64, 0.18, 10


def sine_warp(t):
    """w(t) = t + 0.25 sin(2 pi t / 4): the guide at time t sounds what the score has at w(t); w(0) = 0, w(8) = 8."""
    return t + 0.25 * np.sin(2.0 * np.pi * t / 4.0)


def render(score_time, seed=0, noise_seed=1):
    """The score heard at ``score_time`` (seconds, one entry per output sample): 64 syllables, one every 8 / 64 s and 0.18 s
    long, each ten harmonics with amplitudes rand / h under a sqrt(sin) envelope, F0 drawn from the 13 semitones from 110 Hz
    up.  The score time moves the syllables and their envelopes; the harmonics run on the output's own clock, so a warped
    rendering changes the timing and keeps the pitch, as a second take does.  Plus noise of 1e-3 from ``noise_seed`` (guide
    and source take different draws).  float32."""
    clock = np.arange(score_time.size) / RATE
    rng = np.random.RandomState(seed)
    out = np.zeros(score_time.shape, dtype=np.float64)
    for kk in range(SYLLABLES):
        start = kk * SECONDS / SYLLABLES
        f0 = 110.0 * 2.0 ** (rng.randint(0, 13) / 12.0)
        amps = rng.rand(HARMONICS) / np.arange(1, HARMONICS + 1)
        local = score_time - start
        on = (local > 0) & (local < SYLLABLE_S)
        env = np.sqrt(np.sin(np.pi * local[on] / SYLLABLE_S))
        for hh in range(HARMONICS):
            out[on] += amps[hh] * env * np.sin(2.0 * np.pi * f0 * (hh + 1) * clock[on])
    out = 0.1 * out + 1e-3 * np.random.RandomState(noise_seed).randn(out.size)
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def sine_case():
    """(guide, source): 8 s at 24 kHz each, 641 regular frames each; the guide is the source's score at ``sine_warp``."""
    t = np.arange(int(SECONDS * RATE)) / RATE
    guide, source = render(sine_warp(t), noise_seed=2), render(t, noise_seed=1)
    guide.setflags(write=False)
    source.setflags(write=False)
    return guide, source


def warp_error(nodes, warp=sine_warp):
    """(max, mean) over the nodes of |j_k - w(i_k HOP / RATE) RATE / HOP|: how far, in frames, the path's source time is
    from the true map."""
    nodes = np.asarray(nodes, dtype=np.float64)
    err = np.abs(nodes[:, 1] - warp(nodes[:, 0] * HOP / RATE) * RATE / HOP)
    return float(err.max()), float(err.mean())

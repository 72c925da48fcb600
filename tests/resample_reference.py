"""The resampler's definition, evaluated directly in float64, and the float32 error bound the tests hold it to.

    y[k] = sum_j g[k * down + half - j * up] * x[j],   half = (n_taps - 1) // 2

over 0 <= j < n with the tap index inside [0, n_taps)  (mbexwn_vocoder_amd/resample.py; ``half + pre`` of ``plan`` is a multiple
of ``down``, so this is ``g[(k + rem) * down - j * up - pre]``).

The bound of output k is  B[k] = (m_k + 2) * 2^-24 * sum_j |g| |x|,  m_k the number of terms: the standard bound of an m-term
float32 dot product (every partial sum is bounded by sum |g||x| and each of the m fused multiply-adds rounds once, relative
2^-24; the two extra units absorb the second-order terms of (1 + 2^-24)^m and a last-bit difference between two designs
of g).  Derived, not measured.  The reference's own float32 run stays within 0.18 B on every fixture case, so the bar is
not vacuous and the reference alone is inside it.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_resample.npz")
OUT_SR = 24000
CASES = ((48000, 1), (48000, 2), (48000, 777), (44100, 1000), (16000, 301), (22050, 500), (8000, 100), (32000, 1023),
         (96000, 900), (11025, 200), (12345, 400))
U32 = 2.0 ** -24

_fixture = None


def fixture():
    """The golden file as a dict, loaded once and shared."""
    global _fixture
    if _fixture is None:
        with np.load(GOLDEN) as data:
            _fixture = {kk: data[kk] for kk in data.files}
        for vv in _fixture.values():
            vv.setflags(write=False)
    return _fixture


def evaluate(g, up, down, x, n, ks, x_offset=0):
    """(y64, bound) of the outputs ``ks`` of an n-sample signal.  ``x`` holds the samples x_offset .. x_offset + len(x) of it
    (the whole signal by default); every sample the outputs reach must lie inside."""
    g = np.asarray(g, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    ks = np.asarray(ks, dtype=np.int64)
    n_taps = g.size
    half = (n_taps - 1) // 2
    c = ks * down + half
    jh, ph = c // up, c % up
    ii = np.arange((n_taps - 1) // up + 1, dtype=np.int64)
    tap = ph[:, None] + ii[None, :] * up
    jj = jh[:, None] - ii[None, :]
    valid = (tap < n_taps) & (jj >= 0) & (jj < n)
    local = jj - x_offset
    assert np.all((local[valid] >= 0) & (local[valid] < x.size)), "the given span does not cover these outputs"
    terms = np.where(valid, g[np.where(valid, tap, 0)] * x[np.where(valid, local, 0)], 0.0)
    # ascending j like the kernel (the order is immaterial in float64 at the bound's scale)
    y = terms[:, ::-1].sum(axis=1)
    bound = (valid.sum(axis=1) + 2) * U32 * np.abs(terms).sum(axis=1)
    return y, bound


def evaluate_all(g, up, down, x):
    x = np.asarray(x)
    n_out = -(-x.size * up // down)
    return evaluate(g, up, down, x, x.size, np.arange(n_out))

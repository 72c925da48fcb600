"""(CPU) The references of tests/control_reference.py held to something themselves: the float64 warp against the float32 host
definition at a bound derived per element, with two doctored references that must miss it; and the composed oracle must tell
an F0-net that read the warped rows from one that read the rows as they came."""
import numpy as np
import pytest

import control_reference as cref
import test_gpu_envelope as tenv
from helpers import build_case, synthetic_inputs
from mbexwn_vocoder_amd.envelope import channel_centres, warp_envelope_host

SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 5}
TABLES = tenv.TABLES            # {mel_channels: (fmin, fmax)}: every table the kernel is run on
U = 2.0 ** -24                 # unit roundoff of float32, round to nearest: fl(a op b) = (a op b)(1 + d), |d| <= U
TINY = 2.0 ** -149             # an underflowing product is off by at most this instead


def _gamma(k):
    return k * U / (1.0 - k * U)


def warp_bound(mel, factors, centres):
    """The largest distance a correctly rounded float32 evaluation of THE DEFINITION can have from its exact value, per
    element; ``mel`` (frames, n), ``factors`` (frames,), all taken as exact numbers.

    The float32 evaluation is seven operations, each (exact result)(1 + d), |d| <= U = 2^-24:

        f^  = (c[m] / phi)(1 + d1)                       f = c[m] / phi exact:  |f^ - f| <= U f
        a^  = (f^ - c[i])(1 + d2)      b^ = (c[i+1] - c[i])(1 + d3)      w^ = (a^ / b^)(1 + d4)
        d^  = (x[i+1] - x[i])(1 + d5)  p^ = (w^ d^)(1 + d6)              out = (x[i] + p^)(1 + d7)

    With D = c[i+1] - c[i], d = x[i+1] - x[i], w = (f - c[i]) / D in [0, 1] and g_k = k U / (1 - k U) >= (1 + U)^k - 1:

        (f^ - c[i]) / D = w + (f^ - f) / D,  so  |w^ - w| <= (U f / D)(1 + g3) + w g3           (d2, d3, d4)
        |p^ - w d| <= |d| (|w^ - w|(1 + g2) + w g2)                                            (d5, d6)
        |out - (x[i] + w d)| <= |p^ - w d|(1 + U) + U |x[i] + w d|                              (d7)

    The error of f reaches the result as U f |d| / D: the slope of the envelope times the error of the abscissa.  When f^
    lands on the other side of a centre than f, the evaluation runs in the neighbouring segment with a weight within U f / D'
    of 0 or 1; the envelope is continuous, so the result differs from the exact one by at most U f times the larger of the two
    slopes.  The bound therefore takes, for an f within 2 U f of a centre, the larger slope of the two segments that meet
    there (0 outside [c[0], c[n-1]]), and is otherwise the bound of f's own segment.  Outside the centres the value is x[0] or
    x[n-1] without arithmetic: the bound there is 0 unless f is that close to the outermost centre.  A frame with phi == 1 is
    a copy: bound 0.  Products that underflow add at most 2^-149."""
    x = np.asarray(mel, dtype=np.float64)
    c = np.asarray(centres, dtype=np.float64)
    n = c.shape[0]
    phi = np.asarray(factors, dtype=np.float64)[:, None]
    f = c[None, :] / phi
    k = np.searchsorted(c, f.reshape(-1), side="right").reshape(f.shape)
    inside = (k > 0) & (k < n)
    i = np.clip(k - 1, 0, n - 2)
    D = c[i + 1] - c[i]
    d = np.abs(np.take_along_axis(x, i + 1, axis=1) - np.take_along_axis(x, i, axis=1))
    w = np.where(inside, (f - c[i]) / D, 0.0)
    slope_of = np.abs(np.diff(x, axis=1)) / np.diff(c)[None, :]                  # (frames, n - 1), segment j = [c[j], c[j+1]]
    slope_of = np.concatenate((np.zeros((x.shape[0], 1)), slope_of, np.zeros((x.shape[0], 1))), axis=1)    # j = -1 .. n - 1
    slope = np.take_along_axis(slope_of, k, axis=1)                              # own segment k - 1 -> column k
    near_lo = (k > 0) & (f - c[np.clip(k - 1, 0, n - 1)] <= 2.0 * U * f)         # the centre below f: segment k - 2 meets it
    near_hi = (k < n) & (c[np.clip(k, 0, n - 1)] - f <= 2.0 * U * f)             # the centre above f: segment k
    slope = np.maximum(slope, np.where(near_lo, np.take_along_axis(slope_of, np.clip(k - 1, 0, n), axis=1), 0.0))
    slope = np.maximum(slope, np.where(near_hi, np.take_along_axis(slope_of, np.clip(k + 1, 0, n), axis=1), 0.0))
    ref = cref.warp_envelope_f64(x, phi[:, 0], c)
    e_w_d = U * f * slope * (1.0 + _gamma(3)) + w * d * _gamma(3)                # |w^ - w| |d|
    e_p = e_w_d * (1.0 + _gamma(2)) + w * d * _gamma(2) + TINY
    bound = e_p * (1.0 + U) + U * np.abs(ref)
    bound = np.where(inside | near_lo | near_hi, bound, 0.0)
    return np.where(phi == 1.0, 0.0, bound)


def _doctored(mel, factors, centres, what):
    """warp_envelope_f64 with one mistake: "times" reads the envelope at c[m] * phi, "k-2" takes the segment below."""
    x = np.asarray(mel, dtype=np.float64)
    c = np.asarray(centres, dtype=np.float64)
    n = c.shape[0]
    out = x.copy()
    for t, phi in enumerate(np.asarray(factors, dtype=np.float64)):
        if phi == 1.0:
            continue
        f = c * phi if what == "times" else c / phi
        k = np.searchsorted(c, f, side="right")
        i = np.clip(k - (2 if what == "k-2" else 1), 0, n - 2)
        val = x[t, i] + (f - c[i]) / (c[i + 1] - c[i]) * (x[t, i + 1] - x[t, i])
        out[t] = np.where(k == 0, x[t, 0], np.where(k == n, x[t, n - 1], val))
    return out


@pytest.mark.parametrize("n_mels", sorted(TABLES))
def test_float64_warp_against_the_host_definition(n_mels):
    """envelope.warp_envelope_host (float32, what the kernel is bit-equal to) within warp_bound of warp_envelope_f64, element by
    element, for every table of tests/test_gpu_envelope.py: rows in [-11.5, 2], factors in [0.7, 1.4] that change every frame,
    frames of exactly 1.  Channel 0 reads below c[0] (k == 0) and the last channel above c[n-1] (k == n).  The reference with
    c[m] * phi, and the one with segment k - 2, exceed the bound."""
    fmin, fmax = TABLES[n_mels]
    centres = channel_centres({"mel_channels": n_mels, "fmin": fmin, "fmax": fmax, "sample_rate": 24000})
    rng = np.random.default_rng(5100 + n_mels)
    frames = 257
    mel = np.clip(rng.normal(-5.0, 2.0, size=(frames, n_mels)), -11.5, 2.0).astype(np.float32)
    mel[0, 0], mel[1, -1] = -11.5, 2.0
    phi = cref.formant_rows(rng, 1, frames)[0]
    phi[:3] = (1.4, 0.7, 1.0)
    assert phi.min() >= 0.7 and phi.max() <= 1.4 and np.all(np.diff(phi)[phi[1:] != 1.0] != 0) and 10 < np.sum(phi == 1.0) < frames // 2
    f32 = centres[None, :] / phi[:, None]
    assert f32.dtype == np.float32
    k = np.searchsorted(centres, f32.reshape(-1), side="right").reshape(f32.shape)
    assert np.any(k[phi != 1.0, 0] == 0) and np.any(k[phi != 1.0, -1] == n_mels)          # both held ends are read
    got = warp_envelope_host(mel, phi, centres)
    ref = cref.warp_envelope_f64(mel, phi, centres)
    assert got.dtype == np.float32 and ref.dtype == np.float64
    bound = warp_bound(mel, phi, centres)
    err = np.abs(got.astype(np.float64) - ref)
    assert np.array_equal(got[phi == 1.0], mel[phi == 1.0]) and np.array_equal(ref[phi == 1.0], mel[phi == 1.0].astype(np.float64))
    assert np.all(err[bound == 0.0] == 0.0)
    ratio = float(np.max(err[bound > 0] / bound[bound > 0]))
    print(f"\nwarp n_mels {n_mels}: max |host - f64| {err.max():.3e}, largest error / bound {ratio:.3f}")
    assert ratio <= 1.0, f"n_mels {n_mels}: the float32 definition is {ratio:.3f} of its rounding bound from the float64 one"
    where = bound > 0
    for what in ("times", "k-2"):
        if what == "k-2" and n_mels == 2:
            # one segment: the segment below is clamped to the only one there is, the mistake is no mistake in this table
            assert np.array_equal(_doctored(mel, phi, centres, what), ref)
            continue
        bad = np.abs(got.astype(np.float64) - _doctored(mel, phi, centres, what))
        worst = float(np.max(bad[where] / bound[where]))
        print(f"warp n_mels {n_mels}: doctored reference '{what}' largest error / bound {worst:.3e}")
        assert worst > 1.0, f"n_mels {n_mels}: the bound does not see a reference that reads {what}"
    # n_frames: rows at or behind an item's count are copies
    cut = cref.warp_envelope_f64(mel[None, :9], phi[None, :9], centres, n_frames=[4])
    assert np.array_equal(cut[0, :4], ref[:4]) and np.array_equal(cut[0, 4:], mel[4:9].astype(np.float64))


@pytest.mark.parametrize("case", ["causal_canon", "causal_grammar", "causal_valid"])
def test_force_causal_oracle_against_the_reference_float64_run(case):
    """ForceCausalOracle, the same graph in float64 end to end, against the reference's own float64 run of the three
    force_causal models of tests/golden/make_reference_causal.py, at the bars tests/test_oracle_vs_reference.py holds
    OracleModel to (rounding noise of float64); and OracleModel itself misses them on such a model."""
    import os
    from helpers import load_golden
    from test_causal_host import CAUSAL_CASES as CASES
    from oracle import mbexwn_oracle as orc
    gold = load_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_causal_f64.npz"))
    voice, over, batch, frames = CASES[case]
    cfg, raw, wt = build_case(voice, over)
    om = cref.oracle_model(cfg, raw, wt, dtype=np.float64, float32_constants=False)
    assert isinstance(om, cref.ForceCausalOracle)
    mel, noise = gold[f"{case}/mell"], gold[f"{case}/noise"]
    audio, st = om.forward(mel, noise, return_stages=True)
    assert audio.shape == (batch, frames * 300)
    errs = {name: float(np.max(np.abs(arr - gold[f"{case}/{name}"])))
            for name, arr in (("f0", st["f0"]), ("excitation", st["excitation"]), ("audio", audio))}
    print(f"\nforce_causal oracle {case}: {errs}")
    assert errs["f0"] < 1e-10 and errs["excitation"] < 1e-8 and errs["audio"] < 1e-8
    plain = orc.OracleModel(cfg, raw, wt, dtype=np.float64, float32_constants=False).forward(mel, noise)
    assert float(np.max(np.abs(plain - gold[f"{case}/audio"]))) > 1e-3


def test_the_oracle_tells_the_rows_of_the_f0_net_apart():
    """A SMALL item of 21 frames with a formant factor of 1.3: controlled_oracle_audio with the F0-net on the unwarped rows
    (what mbxe_forward promises) against the same with the F0-net on the warped rows (the mistake a mixed launch group could
    make).  They differ by more than 10 x the end-to-end bar, so the bar of the GPU tests can see that mistake."""
    from oracle import mbexwn_oracle as orc
    from test_gpu_parity import E2E_TOL
    cfg, raw, wt = build_case("SPEECH", SMALL)
    mel, noise = synthetic_inputs(5200, 1, 21)
    centres = channel_centres(cfg["preprocess_config"])
    warped = warp_envelope_host(mel, np.full((1, 21), 1.3, dtype=np.float32), centres)
    right = cref.controlled_oracle_audio(cfg, raw, wt, mel, noise, None, env_rows=warped)
    om = orc.OracleModel(cfg, raw, wt)
    wrong_contour = om.generate_f0(warped.astype(om.dtype))
    wrong = cref.controlled_oracle_audio(cfg, raw, wt, mel, noise, wrong_contour, env_rows=warped)
    # the default contour is the oracle's own of the unwarped rows, and without env_rows the composition is OracleModel.forward
    assert np.array_equal(right, cref.controlled_oracle_audio(cfg, raw, wt, mel, noise, cref.oracle_contour(cfg, raw, wt, mel),
                                                              env_rows=warped))
    plain = om.forward(mel, noise)
    assert np.max(np.abs(cref.controlled_oracle_audio(cfg, raw, wt, mel, noise, None) - plain)) <= 1e-9 * max(1.0, np.max(np.abs(plain)))
    diff = float(np.max(np.abs(right - wrong)))
    bar = 10.0 * E2E_TOL * max(1.0, float(np.max(np.abs(right))))
    print(f"\nF0-net on unwarped against warped rows: max difference {diff:.3e}, 10 x bar {bar:.3e}")
    assert diff > bar

"""(CPU) The comparators of tests/frontend_reference.py accept the float32 port on every case list of
test_gpu_frontend_stages.py and reject planted defects that the suite let through before.  Every defect is planted in the
port, never in product code, and for every defect an assertion says why the earlier tests miss it: it stays inside their
bar on their inputs, or their case lists hold no input that reaches it (then the defect leaves their inputs bit for bit).
Two defects turned out to be caught by the earlier analysis test where it reaches them, and the assertions say that instead:
the frame count at a multiple of the hop (its 3000-sample item is one) and bin_hi one bin short at its own geometry (what went
unseen there is every other geometry's bin ranges).  The normalisation defects are planted on items of 2 to 5 frames, which no
earlier case holds.

The earlier bars and inputs, restated here:
  analysis        test_gpu_dropin.py::test_mel_analysis_on_the_device_matches_the_host_analysis: 1200 / 300 / 2048 / 80, items
                  of 7231, 3000 and 1201 samples, 2e-3 in the log domain and 2e-5 of the item's largest amplitude against
                  compute_log_mel(dtype=np.float32)
  normalisation   test_gpu_configs.py: NORM_CASES on goldens of 17 (ragged: 17 and 9) frames at 2e-5; the back-end stage
                  tests: iters2_comp on items of 26, 1, 41, 7, 13, 33 and 6 frames; no case sets use_max_limit
  oscillator      test_gpu_parity.py: smooth contours between 30 and 680 Hz, uniform batches, 2e-6

The host path analysis.stft_magnitude and the log-mel reference itself are pinned on short signals to the reference's own
calc_stft (tests/golden/reference_stft_short.npz)."""
import os

import numpy as np
import pytest

import frontend_reference as fr
from mbexwn_vocoder_amd import analysis
from mbexwn_vocoder_amd.config import ModelDims, canonical_config
from test_gpu_backend_stages import _NORM as BACKEND_NORM
from test_gpu_backend_stages import RAGGED as BACKEND_RAGGED
from test_gpu_configs import NORM_CASES

MIN_BARS = 4.0          # every planted defect breaks its bar at least this many times over
CANON = "1200_300_2048_80"
TODAY_NORM_LENGTHS = [17, 9] + BACKEND_RAGGED


def _mel_case(name):
    cfg = fr.MEL_GEOMETRIES[name]
    sound, lengths, labels = fr.mel_items(cfg)
    return cfg, fr.MelReference(sound, lengths, analysis.mel_analysis_tables(cfg), cfg, fr.F_MEL[name]), labels


@pytest.fixture(scope="module")
def mel_cases():
    return {name: _mel_case(name) for name in fr.MEL_GEOMETRIES}


@pytest.fixture(scope="module")
def today_mel():
    """The batch of the earlier analysis test with its reference and its two bars."""
    pre = canonical_config("SPEECH")["preprocess_config"]
    rng = np.random.default_rng(17)
    lengths = [7231, 3000, 1201]
    snd = np.zeros((3, max(lengths)), dtype=np.float32)
    for ii, ll in enumerate(lengths):
        tt = np.arange(ll) / pre["sample_rate"]
        snd[ii, :ll] = (0.3 * np.sin(2 * np.pi * (110.0 * (ii + 1)) * tt) + 0.05 * rng.normal(size=ll)).astype(np.float32)
    mr = fr.MelReference(snd, lengths, analysis.mel_analysis_tables(pre), pre, fr.F_MEL[CANON])
    refs = [analysis.compute_log_mel(snd[ii:ii + 1, :ll], pre, dtype=np.float32)[0][0] for ii, ll in enumerate(lengths)]

    def bars(got):
        """(inside the amplitude bar, inside the log-domain bar) of the earlier test."""
        amp_ok = log_ok = True
        for ii, ll in enumerate(lengths):
            nfr = ll // pre["hop_size"] + 1
            err = np.abs(np.exp(got[ii, :nfr]) - np.exp(refs[ii]))
            amp_ok &= bool(np.max(err) <= 2e-5 * np.max(np.exp(refs[ii])))
            log_ok &= bool(np.max(np.abs(got[ii, :nfr] - refs[ii])) <= 2e-3)
        return amp_ok, log_ok

    def passes(got):
        return all(bars(got))
    passes.bars = bars
    assert passes(mr.port_result())
    return mr, passes


# ------------------------------------------------------------------------------------------------------------------------
# audio -> log-mel
# ------------------------------------------------------------------------------------------------------------------------
def test_port_transform_is_float32():
    """The port's transform shows float32 arithmetic: torch's float32 rfft is NOT the float64 transform rounded once.
    numpy's is, bit for bit, where this was written (a newer numpy may transform float32 natively: the port does not
    depend on which) -- a port built on it sets bars that no float32 transform meets."""
    x = np.random.default_rng(0).normal(size=(3, 2048)).astype(np.float32)
    rounded = np.fft.rfft(x.astype(np.float64), axis=-1).astype(np.complex64)
    spec = fr.float32_rfft(x, 2048)
    assert spec.dtype == np.complex64 and np.mean(spec == rounded) < 0.5
    err = np.abs(spec - np.fft.rfft(x.astype(np.float64), axis=-1)).max() / np.abs(rounded).max()
    assert 3e-8 < err < 1e-6, err
    print(f"\nnumpy float32 rfft equals the rounded float64 transform in {np.mean(np.fft.rfft(x, axis=-1) == rounded):.0%} of the bins, "
          f"torch's in {np.mean(spec == rounded):.0%}; torch's error {err:.2e} of the largest bin")


def test_port_sets_the_mel_floor(mel_cases):
    """The comparator accepts the float32 port on every geometry, and every geometry's F_MEL is four times the worst
    relative error the port shows there against the float64 reference (a band, not an equality: the float32 sums of a BLAS
    may be ordered differently); none is above four times the worst over all geometries."""
    worst = {}
    for name, (cfg, mr, labels) in mel_cases.items():
        rec = mr.compare(mr.port_result())
        assert rec["ok"] and rec["ratio"] <= 1.0 / fr.K_PORT + 1e-12, fr.mel_failure(rec, labels)
        assert rec["silent_frames"] >= 4, name                       # silence, the empty item, the impulse items' far frames
        worst[name] = mr.port_relative_error()
        assert 3.0 * worst[name] <= fr.F_MEL[name] <= 5.0 * worst[name], (name, worst[name])
    print("\nmel port relative error per geometry: " + ", ".join(f"{kk} {vv:.2e} (F {fr.F_MEL[kk]:.1e})" for kk, vv in worst.items()))
    assert max(fr.F_MEL.values()) <= 4.0 * max(worst.values()) * 1.01


def _reject(mr, got, labels, what):
    rec = mr.compare(got)
    assert not rec["ok"] and (rec["ratio"] >= MIN_BARS or rec["silent_wrong"]), f"{what}: {rec['ratio']:.3g} bars only"
    msg = fr.mel_failure(rec, labels)
    w = rec["where"]
    assert f"item {w['item']}" in msg and f"of {w['length']} samples" in msg and "n % hop" in msg and "channel" in msg
    print(f"\n{what}: {msg}")
    return rec


def test_mel_defect_reflect_twice_then_clamp(mel_cases, today_mel):
    """The index rule the kernel had (one fold at each end, then a clamp): wrong below half a window, where the earlier
    cases have no item -- on their batch the defect changes no bit."""
    cfg, mr, labels = mel_cases[CANON]
    rec = _reject(mr, mr.port_result(index=fr.reflect_twice_then_clamp_index), labels, "reflect twice, then clamp")
    assert 2 <= rec["where"]["length"] < cfg["win_size"] // 2
    today, passes = today_mel
    assert min(today.lengths) >= cfg["win_size"] // 2 + 1
    assert np.array_equal(today.port_result(index=fr.reflect_twice_then_clamp_index), today.port_result())
    # only items that need a third fold differ
    for ii, nn in enumerate(mr.lengths):
        same = np.array_equal(fr.log_mel_port(mr.sound[ii, :nn], mr.window, mr.basis, mr.hop, mr.fft,
                                              index=fr.reflect_twice_then_clamp_index), mr.port[ii])
        if fr.reflections_needed(nn, cfg["win_size"], cfg["hop_size"]) <= 1:
            assert same, f"item {ii} ({nn} samples)"


def test_mel_defect_symmetric_on_short_items(mel_cases, today_mel):
    """"symmetric" instead of "reflect" (the edge sample repeated) in the folding of items below half a window: out of reach
    of the earlier cases."""
    cfg, mr, labels = mel_cases[CANON]
    index = fr.symmetric_short_index(cfg["win_size"])
    rec = _reject(mr, mr.port_result(index=index), labels, "symmetric folding of short items")
    assert rec["where"]["length"] < cfg["win_size"] // 2 + 1
    today, _ = today_mel
    assert np.array_equal(today.port_result(index=index), today.port_result())


def _narrow_channel(mr):
    """The channel of at most 8 bins whose last bin carries the smallest share of its row, and that share."""
    width = mr.hi - mr.lo + 1
    share = [mr.basis[m, mr.hi[m]] / mr.basis[m].sum() if 2 <= width[m] <= 8 else np.inf for m in range(len(width))]
    return int(np.argmin(share)), float(np.min(share))


def _one_bin_short(mr, m):
    basis = mr.basis.copy()
    basis[m, mr.hi[m]] = 0.0
    return basis


def test_mel_defect_bin_hi_one_short(mel_cases, today_mel):
    """bin_hi one bin short on one narrow channel.  The earlier test runs one geometry, so the bin ranges of every other one
    are out of its reach: planted at 200 / 50 / 256 / 128 (rows of at most 7 bins, 22 of them empty) and at 800 / 200 / 1024
    the defect is rejected.  Found while writing this test: at the earlier geometry both earlier bars do catch it on the
    earlier batch, even on the narrow channel whose last bin weighs least (0.18 % of its row: 7e-3 in the log against
    2e-3), so it is the other geometries' bin ranges that went unseen."""
    for name in ("200_50_256_128", "800_200_1024_80_16k", CANON):
        cfg, mr, labels = mel_cases[name]
        m, share = _narrow_channel(mr)
        rec = _reject(mr, mr.port_result(basis=_one_bin_short(mr, m)), labels,
                      f"{name}: bin_hi one short on channel {m} (last bin: {share:.2%} of the row)")
        assert rec["where"]["channel"] == m
    today, passes = today_mel
    assert (today.fft, today.hop, len(today.window)) == (2048, 300, 1200)          # the one geometry of the earlier test
    m, share = _narrow_channel(today)
    got = today.port_result(basis=_one_bin_short(today, m))
    assert passes.bars(got) == (False, False)
    assert today.compare(got)["ratio"] >= MIN_BARS


def test_mel_defect_confined_to_fft_1024(mel_cases, today_mel):
    """Bins k and fft/2 - k exchanged in the real split of a 1024-point transform: the earlier cases transform 2048 points
    only."""
    cfg, mr, labels = mel_cases["800_200_1024_80_16k"]
    assert cfg["fft_size"] == 1024
    _reject(mr, mr.port_result(spec_hook=fr.swap_bins_1024), labels, "bins exchanged in the 1024-point real split")
    today, _ = today_mel
    assert today.fft == 2048 and np.array_equal(today.port_result(spec_hook=fr.swap_bins_1024), today.port_result())
    for name, (gcfg, gmr, glabels) in mel_cases.items():
        if gcfg["fft_size"] != 1024:
            assert gmr.compare(gmr.port_result(spec_hook=fr.swap_bins_1024))["ok"], name


def test_mel_defect_frame_count_at_hop_multiples(mel_cases, today_mel):
    """(n - 1) // hop + 1 frames where n is a multiple of hop: the last frame is not written.  Found while writing this
    test: the earlier batch does hold such an item (3000 = 10 hops), so the earlier test catches this one as well; the
    new cases hold one at every geometry, down to n = hop."""
    for name, (cfg, mr, labels) in mel_cases.items():
        rec = _reject(mr, mr.port_result(n_frames=fr.frames_short_at_hop_multiples), labels, f"{name}: frame count")
        assert rec["where"]["n%hop"] == 0 and rec["where"]["frame"] == rec["where"]["frames"] - 1
    today, passes = today_mel
    assert any(nn % today.hop == 0 for nn in today.lengths)
    assert not passes(today.port_result(n_frames=fr.frames_short_at_hop_multiples))


def test_mel_comparator_judges_a_quiet_frame_on_its_own_scale(mel_cases):
    """One channel of one quiet item moved by 1e-4 of its own frame's scale: rejected, although it is 1e-8 of the launch's
    largest amplitude; and a silent frame one ulp off log(eps) is rejected."""
    cfg, mr, labels = mel_cases[CANON]
    scales = [np.maximum(mr.ref[ii], mr.eps).max() for ii in range(len(mr.lengths))]
    quiet = int(np.argmin([ss if mr.ref[ii].max() >= 1e3 * mr.eps else np.inf for ii, ss in enumerate(scales)]))
    got = mr.port_result()
    ch = int(np.argmax(mr.ref[quiet][0]))
    got[quiet, 0, ch] = np.log(np.exp(np.float64(got[quiet, 0, ch])) + 1e-4 * mr.ref[quiet][0].max())
    rec = mr.compare(got)
    assert not rec["ok"] and rec["where"]["item"] == quiet and 1e-4 * mr.ref[quiet][0].max() < 1e-7 * max(scales)
    got = mr.port_result()
    silent = labels.index("silence")
    got[silent, 1, 0] = np.nextafter(got[silent, 1, 0], np.float32(0))
    rec = mr.compare(got)
    assert not rec["ok"] and rec["silent_wrong"] == 1 and rec["silent_where"]["item"] == silent
    assert "log(eps) exactly" in fr.mel_failure(rec, labels)


def test_short_signals_match_the_reference_stft(golden_dir):
    """analysis.stft_magnitude (the host path) and the STFT inside log_mel_reference against the reference's own calc_stft on
    signals of 1 .. 601 samples, float32 and float64: the host path bit for bit."""
    gold = np.load(os.path.join(golden_dir, "reference_stft_short.npz"))
    keys = sorted({kk.rsplit("/", 1)[0] for kk in gold.files})
    assert len(keys) == 18
    for key in keys:
        win, hop, fft = (int(vv) for vv in key.split("/")[0].split("_"))
        snd = gold[key + "/snd"]
        assert key.endswith(f"/n{snd.size}") and snd.dtype == np.float32
        for tag, dt in (("mag32", np.float32), ("mag64", np.float64)):
            got = analysis.stft_magnitude(snd[None], win, hop, fft, dtype=dt)[0]
            assert got.dtype == gold[f"{key}/{tag}"].dtype and np.array_equal(got, gold[f"{key}/{tag}"]), f"{key} {tag}"
        window = analysis.hann_symmetric(win).astype(np.float64)
        mag = fr.log_mel_reference(snd, window, np.eye(fft // 2 + 1), hop, fft)
        np.testing.assert_allclose(mag, gold[key + "/mag64"], rtol=0, atol=1e-12 * max(1.0, gold[key + "/mag64"].max()))
        # the port's index map is numpy's reflect
        idx = fr.reflect_index(np.arange(-(win // 2), snd.size + win), snd.size)
        assert np.array_equal(snd[idx], np.pad(snd, (win // 2, win), mode="reflect"))


# ------------------------------------------------------------------------------------------------------------------------
# RMS normalisation
# ------------------------------------------------------------------------------------------------------------------------
def _norm_cfg(extra):
    cfg = canonical_config("SPEECH")
    cfg["mbexwn_config"].update(normalize_rms_from_mell=True, **extra)
    return cfg


MAX_LIMIT = {"normalize_rms_num_smooth_iters": 1, "use_max_limit": True, "lin_amp_off": 1e-4}


@pytest.mark.parametrize("case", sorted(NORM_CASES) + ["max_limit"])
def test_norm_port_passes_at_every_level(case):
    """The float32 run of the oracle stays inside the bar on the ragged batch at all three levels; everything is finite; the
    bars are tighter than the earlier 2e-5 (normalize_use_pinv aside, whose float32 contraction over 1025 bins is larger)."""
    cfg = _norm_cfg(MAX_LIMIT if case == "max_limit" else NORM_CASES[case])
    for level in fr.NORM_LEVELS:
        mel = fr.norm_inputs(level)
        nr = fr.NormReference(mel, fr.NORM_LENGTHS, cfg)
        got = nr.port_result()
        rep = nr.compare(got)
        fr.assert_matches(rep, f"normalisation {case} {level}")
        for ii, ll in enumerate(fr.NORM_LENGTHS):
            assert np.all(np.isfinite(nr.ref[ii][0])) and np.all(np.isfinite(nr.ref[ii][1]))
        print(f"\nnorm {case} {level}: " + "  ".join(f"{kk} port {vv['port_err']:.2e} tol {vv['tol']:.2e} |ref| {vv['ref_max']:.3g}"
                                                      for kk, vv in rep.items()))
        if case != "pinv":
            assert rep["mel_norm"]["tol"] < 2e-5 and rep["gain"]["tol"] < 2e-5


def test_norm_port_with_room_for_defects_is_the_oracle_float32_run():
    for extra in (NORM_CASES["iters2_comp"], NORM_CASES["scaled_win"], MAX_LIMIT):
        cfg = _norm_cfg(extra)
        mel = fr.norm_inputs("mid", lengths=[5, 17])
        for ii, ll in enumerate((5, 17)):
            a, b = fr.norm_port_with_defect(mel[ii, :ll], cfg), fr.norm_reference(mel[ii, :ll], cfg, dtype=np.float32)
            np.testing.assert_allclose(a[0], b[0], rtol=0, atol=2e-6)
            np.testing.assert_allclose(a[1], b[1], rtol=1e-6, atol=0)


@pytest.mark.parametrize("defect,case", [("edge_k_minus_1", "iters2_comp"), ("edge_k_minus_1", "scaled_win"),
                                         ("gain_one_early", "iters1"), ("gain_one_early", "scaled_win")])
def test_norm_defects_on_short_items(defect, case):
    """k - 1 for k - 2 in the edge extension, and the output gain read at win / 2 - 1, on items of 2 to 5 frames (where the
    clamps of the edge extension decide every term): the earlier cases hold items of 1, 6 and more frames only."""
    only = lambda ll: 2 <= ll <= 5          # noqa: E731
    assert not any(only(ll) for ll in TODAY_NORM_LENGTHS)
    cfg = _norm_cfg(NORM_CASES[case])
    nr = fr.NormReference(fr.norm_inputs("mid"), fr.NORM_LENGTHS, cfg)
    rep = nr.compare(nr.port_result(defect=defect, only=only))
    worst = max(rep.values(), key=lambda rr: rr["err"] / rr["tol"])
    assert not worst["ok"] and worst["err"] >= MIN_BARS * worst["tol"], rep
    assert only(worst["where"]["frames"])
    print(f"\n{defect} {case}: " + fr.failures(rep))
    # the planted items aside, nothing moved: a 1-frame item cannot see either defect's edge term
    rep1 = nr.compare(nr.port_result(defect="edge_k_minus_1", only=lambda ll: ll == 1))
    assert all(rr["ok"] for rr in rep1.values())


def test_norm_defect_sum_where_use_max_limit_asks_for_max():
    """log(m + off) where use_max_limit asks for log(max(m, off)): no earlier device test sets use_max_limit."""
    assert not any("use_max_limit" in extra for extra in NORM_CASES.values())
    assert not any(kk.endswith("use_max_limit") for kk in BACKEND_NORM)
    cfg = _norm_cfg(MAX_LIMIT)
    for level in fr.NORM_LEVELS:
        nr = fr.NormReference(fr.norm_inputs(level), fr.NORM_LENGTHS, cfg)
        rep = nr.compare(nr.port_result(defect="sum_not_max"), names=("mel_norm",))
        assert rep["mel_norm"]["err"] >= MIN_BARS * rep["mel_norm"]["tol"], (level, rep)
    # without use_max_limit the defect is no defect
    plain = _norm_cfg(NORM_CASES["iters1"])
    nr = fr.NormReference(fr.norm_inputs("mid", lengths=[5, 17]), [5, 17], plain)
    assert all(rr["ok"] for rr in nr.compare(nr.port_result(defect="sum_not_max")).values())


# ------------------------------------------------------------------------------------------------------------------------
# oscillator
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pulse_case():
    cfg, raw, wt = fr.pulse_model("canon")
    d = ModelDims(cfg)
    f0, frames = fr.pulse_contours(wt, d.pulse_rate, d.pulse_per_frame)
    om64, om32 = fr.oracle_models(cfg, raw, wt)
    return d, wt, om64, om32, fr.PulseReference(om64, om32, f0, [ff * d.pulse_per_frame for ff in frames])


def _today_contours(d, n=2400):
    tt = np.arange(n) / d.pulse_rate
    return np.stack([355.0 + 325.0 * np.sin(2 * np.pi * (1.3 + ii) * tt + ii) for ii in range(3)]).astype(np.float32)


@pytest.mark.parametrize("model", sorted(fr.PULSE_MODELS))
def test_pulse_port_passes(model):
    cfg, raw, wt = fr.pulse_model(model)
    d = ModelDims(cfg)
    f0, frames = fr.pulse_contours(wt, d.pulse_rate, d.pulse_per_frame)
    om64, om32 = fr.oracle_models(cfg, raw, wt)
    pr = fr.PulseReference(om64, om32, f0, [ff * d.pulse_per_frame for ff in frames])
    rep = pr.compare(pr.port_result())
    fr.assert_matches(rep, f"oscillator {model}")
    assert rep["phase"]["bit_equal"] and rep["pulse"]["port_err"] <= fr.PULSE_TOL / MIN_BARS
    assert np.asarray(pr.ref[0][0]).shape == ((2000, 1 + d.wt_subharm) if d.wt_subharm else (2000,))


def test_pulse_contours_reach_what_they_claim(pulse_case):
    """Both clamps of the table grid, every grid point with a neighbour on either side, 0 Hz, phase velocities 0.5 and 1,
    1-frame items, an item of whole chunks and items that end inside a chunk."""
    d, wt, om64, om32, pr = pulse_case
    vals = fr.pulse_values(wt, d.pulse_rate)
    ratio = vals / np.float32(wt.nominalF0)
    q = np.log(np.clip(ratio, wt.min_transposition, wt.max_transposition)) * wt.grid_norm
    assert (ratio < wt.min_transposition).any() and (ratio > wt.max_transposition).any() and (vals == 0).any()
    for r in range(wt.n_tables):
        near = np.abs(q - r) < 1e-5
        assert near.sum() >= 3 or r in (0, wt.n_tables - 1), r               # the point and a neighbour on either side
    assert {0.5, 1.0} <= set((vals / np.float32(d.pulse_rate)).tolist())
    assert all(vv in pr.f0[0, :2000] and vv in pr.f0[7, :2500] for vv in vals)
    assert 100 in pr.samples and any(nn % 1000 == 0 for nn in pr.samples) and any(nn % 1000 for nn in pr.samples if nn > 1000)
    assert sum(nn < max(pr.samples) for nn in pr.samples) >= 8               # ragged


def test_pulse_defect_grid_weight_not_clamped_at_the_last_table(pulse_case):
    """Above max_tf the last table's weight must stay 1: the earlier contours end at 680 Hz, below the last table's
    frequency, so the defect leaves them bit for bit."""
    d, wt, om64, om32, pr = pulse_case
    bad = fr.unclamped_top_model(om32)
    rep = pr.compare(pr.port_result(model=bad))
    assert rep["pulse"]["err"] >= MIN_BARS * fr.PULSE_TOL and rep["pulse"]["where"]["f0"] > wt.max_transposition * wt.nominalF0
    today = _today_contours(d)
    assert today.max() <= 680.0 < float(wt.max_transposition) * wt.nominalF0 and today.min() >= 30.0
    assert np.array_equal(bad.wavetable(today), om32.wavetable(today))


def test_pulse_defect_chunk_ends_one_sample_late_in_a_ragged_item(pulse_case):
    """The chunks of an item shorter than its batch end one sample late: the phase is off from the second chunk on.  The
    earlier oscillator cases are uniform batches, which the defect does not touch."""
    d, wt, om64, om32, pr = pulse_case
    rep = pr.compare(pr.port_result(phase_fn=fr.phase_chunk_one_late))
    assert not rep["phase"]["ok"] and rep["phase"]["where"]["chunk"] == 1 and rep["phase"]["where"]["sample_in_chunk"] == 0
    assert rep["phase"]["where"]["samples"] < max(pr.samples)
    assert rep["pulse"]["err"] >= MIN_BARS * fr.PULSE_TOL
    today = _today_contours(d)
    for ii in range(today.shape[0]):
        assert np.array_equal(fr.phase_chunk_one_late(om32, today[ii:ii + 1], today.shape[1]), om32.phase_from_f0(today[ii:ii + 1]))
    # the defect's own restatement of the chunked sum is the oracle's where no chunk is late
    f = pr.f0[7:8, :2500]
    ok = fr.phase_chunk_one_late(om32, f[:, :2500], 2500)
    assert np.array_equal(ok, om32.phase_from_f0(f))


def test_f0_comparator_counts_ulps():
    ref = {0: np.array([100.0, 200.0, 400.0])}
    got = np.array([[100.0, 200.0, 400.0]], np.float32)
    assert fr.compare_f0(got, ref, [3], 1)["ok"]
    got[0, 1] = np.nextafter(np.float32(200.0), np.float32(300.0))
    rec = fr.compare_f0(got, ref, [3], 1)
    assert not rec["ok"] and rec["where"]["sample"] == 1 and abs(rec["ulps"] - 1.0) < 1e-6

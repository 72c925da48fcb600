"""The stages in front of the WaveNet against float64 references (tests/frontend_reference.py): audio -> log-mel
(mbx_mel_analysis), the RMS normalisation (mbx_norm_mel, and inside mbx_forward) and the oscillator with its F0 contour
(mbx_wavetable, and inside mbx_forward with caller-supplied contours and transposition).

Every case is a ragged launch compared item by item at the item's own length; each prints one JSON line ("frontend stages
record ...") with its error against its bar (profiles/frontend_stages.json).  The padding contract is held on the three
stages too: the rows behind every item's end at 0, 1e30 and NaN leave the valid rows bit for bit.  Engines are created once
per model (module cache)."""
import json

import numpy as np
import pytest

import frontend_reference as fr
from backend_reference import overlap_add_f32
from helpers import synthetic_inputs
from mbexwn_vocoder_amd import analysis
from mbexwn_vocoder_amd.config import ModelDims, canonical_config
from test_gpu_configs import NORM_CASES

_SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 3}
NORM_MODELS = dict(NORM_CASES, max_limit={"normalize_rms_num_smooth_iters": 1, "use_max_limit": True, "lin_amp_off": 1e-4})
# normalize_use_pinv: measured on an MI355X against the float64 oracle, the device meets the common bar (see
# profiles/frontend_stages.json), so no bar of its own
PAD_FILLS = (0.0, 1e30, np.nan)
_ENGINES = {}


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    if not _torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return _torch


def _dev(torch, arr, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(arr), dtype=dtype).cuda()


def _engine(key, build):
    """(engine, cfg, raw, wt, om64, om32) of a model, created once."""
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    if key not in _ENGINES:
        cfg, raw, wt = build()
        _ENGINES[key] = (MBExWNEngine(cfg, raw, wt), cfg, raw, wt) + fr.oracle_models(cfg, raw, wt)
    return _ENGINES[key]


def _print_record(cid, rec):
    print("frontend stages record " + json.dumps({cid: rec}))            # with -s: one JSON line per case


# ------------------------------------------------------------------------------------------------------------------------
# audio -> log-mel
# ------------------------------------------------------------------------------------------------------------------------
def test_mel_cases_reach_what_they_claim():
    """(CPU) Counted from the geometry alone: both pass structures of the LDS FFT (radix-4 only, and with the radix-2 pass),
    transforms with fewer points than the block has threads (with and without the radix-2 pass), window = FFT and window <
    FFT, an odd window and hop, basis rows without a bin and rows wider than the 64 lanes of a wave, a single row over 1023
    bins, and in every launch items folded 0, 1, 2 and 3 or more times by the reflect padding."""
    geoms = fr.MEL_GEOMETRIES
    passes = {name: fr.fft_passes(cfg["fft_size"]) for name, cfg in geoms.items()}
    assert {pp[1] for pp in passes.values()} == {0, 1}
    small = {name for name, cfg in geoms.items() if cfg["fft_size"] // 2 < fr.FFT_THREADS}
    assert {passes[name][1] for name in small} == {0, 1}
    assert min(cfg["fft_size"] for cfg in geoms.values()) == 8                       # launch_mel_analysis's lower limit
    assert any(cfg["win_size"] == cfg["fft_size"] for cfg in geoms.values())
    assert any(cfg["win_size"] % 2 and cfg["hop_size"] % 2 for cfg in geoms.values())
    assert any(cfg["fft_size"] == 1024 for cfg in geoms.values()) and any(cfg["fft_size"] == 512 for cfg in geoms.values())
    empty, widest = {}, {}
    for name, cfg in geoms.items():
        _, _, basis, lo, hi = analysis.mel_analysis_tables(cfg)
        empty[name] = int(np.sum(lo > hi))
        widest[name] = int(np.max(hi - lo + 1))
        assert np.all(lo[lo > hi] == 1) and np.all(hi[lo > hi] == 0)
        win, hop = cfg["win_size"], cfg["hop_size"]
        sound, lengths, labels = fr.mel_items(cfg)
        assert lengths[0] == max(lengths) >= win // 2 + 1
        assert set(fr.mel_lengths(cfg)) <= set(lengths)
        assert {0, 1, 2, hop - 1, hop, hop + 1, win // 2 - 1, win // 2, win // 2 + 1, win - 1, win} <= set(lengths)
        assert any(nn % hop == 0 and nn > win for nn in lengths) and any(nn % hop == hop - 1 and nn > win for nn in lengths)
        folds = {min(fr.reflections_needed(nn, win, hop), 3) for nn in lengths}
        assert folds == {0, 1, 2, 3}, (name, folds)
        for want in ("silence", "constant", "impulse0", "impulse-last", "impulse-mid", "sine-on-bin", "sine-between-bins", "noise1e4"):
            assert want in labels, (name, want)
        assert np.abs(sound[labels.index("noise1e4")]).max() > 1e4
    assert empty["200_50_256_128"] == 22 and empty["1200_300_2048_80"] == 0
    assert widest["1200_300_2048_80"] > 64 and widest["1200_300_2048_1"] == 1023
    print("\nmel geometries: " + "; ".join(f"{name}: passes {passes[name]}, empty rows {empty[name]}, widest row {widest[name]}"
                                           for name in geoms))


def _mel_launch(torch, cfg, sound, lengths):
    out, rate = analysis.compute_log_mel_device(_dev(torch, sound), cfg, n_samples=_dev(torch, np.asarray(lengths, np.int32)))
    assert rate == cfg["sample_rate"] / cfg["hop_size"]
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(fr.MEL_GEOMETRIES))
def test_mel_analysis_matches_the_float64_reference(torch, name):
    """One ragged launch per geometry, every item compared per frame on amplitudes; a frame that is silent in the reference
    is log(eps) exactly.  Items below half a window are reflected as numpy reflects them, as often as it takes."""
    cfg = fr.MEL_GEOMETRIES[name]
    sound, lengths, labels = fr.mel_items(cfg)
    got = _mel_launch(torch, cfg, sound, lengths)
    mr = fr.MelReference(sound, lengths, analysis.mel_analysis_tables(cfg), cfg, fr.F_MEL[name])
    rec = mr.compare(got)
    print(f"\nmel analysis {name}: {rec['ratio']:.3f} of the bar (err {rec['err']:.3e}, tol {rec['tol']:.3e}) at {rec['where']}")
    _print_record("mel/" + name, {kk: rec[kk] for kk in ("ratio", "err", "tol", "port_err", "scale", "silent_frames", "silent_wrong")})
    # per class of item, for the report: the worst ratio among the items below half a window and among the others
    short = [ii for ii, nn in enumerate(lengths) if nn < cfg["win_size"] // 2 + 1]
    rec_short = mr.compare(got, items=short)
    assert rec_short["ok"], "items below half a window: " + fr.mel_failure(rec_short, labels)
    assert rec["ok"], fr.mel_failure(rec, labels)
    assert rec["silent_frames"] >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1200_300_2048_80", "800_200_1024_80_16k", "12_4_16_5"])
def test_mel_analysis_never_reads_behind_an_item(torch, name):
    cfg = fr.MEL_GEOMETRIES[name]
    sound, lengths, labels = fr.mel_items(cfg)
    hop = cfg["hop_size"]
    runs = []
    for fill in PAD_FILLS:
        snd = sound.copy()
        for ii, nn in enumerate(lengths):
            snd[ii, nn:] = fill
        runs.append(_mel_launch(torch, cfg, snd, lengths))
    for fill, run in zip(PAD_FILLS[1:], runs[1:]):
        for ii, nn in enumerate(lengths):
            a, b = run[ii, :nn // hop + 1], runs[0][ii, :nn // hop + 1]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"item {ii} ({labels[ii]}, {nn} samples), padding {fill}"


# ------------------------------------------------------------------------------------------------------------------------
# RMS normalisation
# ------------------------------------------------------------------------------------------------------------------------
def _norm_model(case):
    def build():
        from mbexwn_vocoder_amd.tables import WaveTables
        from mbexwn_vocoder_amd.weights import synthetic_weights
        cfg = canonical_config("SPEECH", **_SMALL)
        cfg["mbexwn_config"].update(normalize_rms_from_mell=True, **NORM_MODELS[case])
        raw = synthetic_weights(cfg, seed=1234, bias_std=0.05, alpha_jitter=0.05)
        return cfg, raw, WaveTables(sample_rate=ModelDims(cfg).pulse_rate, **cfg["mbexwn_config"]["wavetable_config"])
    return _engine("norm/" + case, build)


def _norm_stage(torch, eng, mel, lengths):
    out, gain = eng.norm_mel_stage(_dev(torch, mel), n_frames=_dev(torch, np.asarray(lengths, np.int32)))
    return {"mel_norm": out.cpu().numpy(), "gain": gain.cpu().numpy()}


def _norm_forward(torch, eng, mel, noise, lengths):
    """The normalisation as mbx_forward runs it: its "mel_norm" stage, and the gain as the audio over the overlap-add of
    the engine's own frames (float64 quotient of float32 values: the gain to 6e-8; where the overlap-add is 0 nothing is
    learnt and the entry is NaN-free by taking the reference there -- see the caller)."""
    d = eng.dims
    B, T = mel.shape[:2]
    audio = eng.forward(_dev(torch, mel), n_frames=_dev(torch, np.asarray(lengths, np.int32)), noise=_dev(torch, noise)).cpu().numpy()
    mel_norm = eng.stage("mel_norm").cpu().numpy().reshape(B, T, d.mel_channels)
    frames = eng.stage("frames").cpu().numpy().reshape(B, T, d.stft_win)
    return audio, mel_norm, frames


@pytest.mark.gpu
@pytest.mark.parametrize("level", list(fr.NORM_LEVELS))
@pytest.mark.parametrize("case", list(NORM_MODELS))
def test_norm_mel_matches_the_float64_oracle(torch, case, level):
    """mel_norm and the per-sample gain of a ragged batch of 1 .. 800 frames, through mbx_norm_mel and through a forward."""
    eng, cfg = _norm_model(case)[:2]
    d = eng.dims
    lengths = fr.NORM_LENGTHS
    mel = fr.norm_inputs(level)
    nr = fr.NormReference(mel, lengths, cfg)
    rep = nr.compare(_norm_stage(torch, eng, mel, lengths))
    rec = {"stage": fr.record(rep)}
    if case == "pinv":
        ko = {ii: fr.norm_port_kernel_order(mel[ii, :ll], cfg) for ii, ll in enumerate(lengths)}
        rec["stage_kernel_order_port_bar"] = fr.record(nr.compare(_norm_stage(torch, eng, mel, lengths), port=ko))
    # through the forward
    noise = np.random.default_rng(43).normal(size=(len(lengths), max(lengths) * d.wn_in_rows_per_frame)).astype(np.float32)
    audio, mel_norm, frames = _norm_forward(torch, eng, mel, noise, lengths)
    gain = np.zeros((len(lengths), max(lengths) * d.hop_size), np.float64)
    learnt = 0
    for ii, ll in enumerate(lengths):
        n = ll * d.hop_size
        base = overlap_add_f32(frames[ii, :ll], ll, d.hop_size).astype(np.float64)
        live = base != 0.0
        gain[ii, :n] = np.where(live, audio[ii, :n].astype(np.float64) / np.where(live, base, 1.0), nr.ref[ii][1])
        assert np.all(audio[ii, :n][~live] == 0.0) and np.all(audio[ii, n:] == 0.0)
        learnt += int(live.sum())
        # the last hop of every item carries a gain
        assert live[n - d.hop_size:].any(), f"item {ii}: the overlap-add is 0 over the last hop"
    assert learnt >= 0.99 * sum(lengths) * d.hop_size
    rep_fw = nr.compare({"mel_norm": mel_norm, "gain": gain})
    rec["forward"] = fr.record(rep_fw)
    print(f"\nnorm {case} {level}: stage " + "  ".join(f"{kk} {vv['err']:.2e}/{vv['tol']:.2e}" for kk, vv in rep.items())
          + "; forward " + "  ".join(f"{kk} {vv['err']:.2e}/{vv['tol']:.2e}" for kk, vv in rep_fw.items()))
    _print_record(f"norm/{case}/{level}", rec)
    fr.assert_matches(rep, f"mbx_norm_mel {case} {level}")
    fr.assert_matches(rep_fw, f"normalisation inside the forward {case} {level}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["iters2_comp", "scaled_win", "max_limit"])
def test_norm_mel_never_reads_behind_an_item(torch, case):
    eng, cfg = _norm_model(case)[:2]
    hop = eng.dims.hop_size
    lengths = fr.NORM_LENGTHS
    runs = []
    for fill in PAD_FILLS:
        mel = fr.norm_inputs("mid")
        for ii, ll in enumerate(lengths):
            mel[ii, ll:] = fill
        runs.append(_norm_stage(torch, eng, mel, lengths))
    for fill, run in zip(PAD_FILLS[1:], runs[1:]):
        for ii, ll in enumerate(lengths):
            assert np.array_equal(run["mel_norm"][ii, :ll].view(np.uint32), runs[0]["mel_norm"][ii, :ll].view(np.uint32)), (ii, fill)
            assert np.array_equal(run["gain"][ii, :ll * hop].view(np.uint32), runs[0]["gain"][ii, :ll * hop].view(np.uint32)), (ii, fill)


# ------------------------------------------------------------------------------------------------------------------------
# oscillator and contour
# ------------------------------------------------------------------------------------------------------------------------
def _pulse_model(name):
    return _engine("pulse/" + name, lambda: fr.pulse_model(name))


def _pulse_forward(torch, eng, mel, noise, frames, f0, transposition):
    d = eng.dims
    B, T = len(frames), max(frames)
    eng.forward(_dev(torch, mel), n_frames=_dev(torch, np.asarray(frames, np.int32)), noise=_dev(torch, noise), f0=_dev(torch, f0),
                transposition=transposition)
    n = T * d.pulse_per_frame
    f0_stage = eng.stage("f0").cpu().numpy().reshape(B, n)
    pulse = eng.stage("pulse").cpu().numpy()
    return f0_stage, (pulse.reshape(B, n, 1 + d.wt_subharm) if d.wt_subharm else pulse.reshape(B, n))


@pytest.mark.gpu
@pytest.mark.parametrize("transposition", [1.0, 0.5, 2.0])
@pytest.mark.parametrize("model", list(fr.PULSE_MODELS))
def test_oscillator_matches_the_oracle_on_caller_contours(torch, model, transposition):
    """Contours at and beyond both clamps of the table grid, on every grid point and one ulp to either side, 0 Hz, phase
    velocities 0.5 and 1, steps between them inside a chunk: through forward(f0=..., transposition=...) on a ragged batch
    (the "pulse" stage against OracleModel.wavetable on the engine's own "f0" stage, per item at its own length) and
    through mbx_wavetable (the phase bit for bit)."""
    eng, cfg, raw, wt, om64, om32 = _pulse_model(model)
    d = eng.dims
    f0, frames = fr.pulse_contours(wt, d.pulse_rate, d.pulse_per_frame)
    B, T = len(frames), max(frames)
    mel, noise = synthetic_inputs(71, B, T, steps_per_frame=d.wn_in_rows_per_frame)
    f0_stage, pulse = _pulse_forward(torch, eng, mel, noise, frames, f0, transposition)
    samples = [ff * d.pulse_per_frame for ff in frames]
    for ii, nn in enumerate(samples):
        want = (f0[ii, :nn] * np.float32(transposition)).astype(np.float32)
        assert np.array_equal(f0_stage[ii, :nn], want), f"item {ii}: the \"f0\" stage is not the given contour times the transposition"
    pr = fr.PulseReference(om64, om32, f0_stage, samples)
    rep = pr.compare({"pulse": pulse})
    # mbx_wavetable: uniform, every row whole (the rows behind an item's end hold the fill value)
    f0_all = (f0 * np.float32(transposition)).astype(np.float32)
    p_all, ph_all = eng.wavetable(_dev(torch, f0_all))
    pr_all = fr.PulseReference(om64, om32, f0_all, [f0_all.shape[1]] * B)
    rep_all = pr_all.compare({"pulse": p_all.cpu().numpy(), "phase": ph_all.cpu().numpy()})
    print(f"\noscillator {model} x{transposition}: forward pulse {rep['pulse']['err']:.2e}/{rep['pulse']['tol']:.1e}; mbx_wavetable "
          f"pulse {rep_all['pulse']['err']:.2e}, phase {'bit-equal' if rep_all['phase']['bit_equal'] else 'DIFFERS'}")
    _print_record(f"pulse/{model}/x{transposition}", {"forward": fr.record(rep), "wavetable": fr.record(rep_all)})
    fr.assert_matches(rep, f"oscillator inside the forward ({model}, transposition {transposition})")
    fr.assert_matches(rep_all, f"mbx_wavetable ({model}, transposition {transposition})")


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["canon", "sinfun"])
def test_oscillator_never_reads_behind_an_item(torch, model):
    """The contour rows behind every item's end at 0, 1e30 and NaN (and the mel and noise rows with them): "f0" and "pulse"
    over every item's own samples keep their bits."""
    eng, cfg, raw, wt, om64, om32 = _pulse_model(model)
    d = eng.dims
    f0, frames = fr.pulse_contours(wt, d.pulse_rate, d.pulse_per_frame)
    B, T = len(frames), max(frames)
    mel, noise = synthetic_inputs(71, B, T, steps_per_frame=d.wn_in_rows_per_frame)
    runs = []
    for fill in PAD_FILLS:
        ff, mm, nz = f0.copy(), mel.copy(), noise.copy()
        for ii, ll in enumerate(frames):
            ff[ii, ll * d.pulse_per_frame:], mm[ii, ll:], nz[ii, ll * d.wn_in_rows_per_frame:] = fill, fill, fill
        runs.append(_pulse_forward(torch, eng, mm, nz, frames, ff, 1.0))
    for fill, (f0_s, pulse) in zip(PAD_FILLS[1:], runs[1:]):
        for ii, ll in enumerate(frames):
            n = ll * d.pulse_per_frame
            assert np.array_equal(f0_s[ii, :n].view(np.uint32), runs[0][0][ii, :n].view(np.uint32)), (ii, fill)
            assert np.array_equal(pulse[ii, :n].view(np.uint32), runs[0][1][ii, :n].view(np.uint32)), (ii, fill)


F0_RAGGED = [26, 1, 2, 41, 7, 3, 13]
F0_LARGE = [800, 700, 900, 760, 880, 720, 840, 740, 860, 780, 820, 710, 890, 750, 870, 800]


@pytest.mark.gpu
@pytest.mark.parametrize("cid,lengths", [("ragged", F0_RAGGED), ("16x800", F0_LARGE)], ids=["ragged", "16x800"])
def test_f0_contour_of_a_ragged_batch_is_the_nearest_float32(torch, cid, lengths):
    """The "f0" stage of a ragged batch against OracleModel.generate_f0 in float64 on each item's own frames (the F0-net's
    SYMMETRIC padding reflects at the item's own end): half a float32 ulp, 1- and 2-frame items included."""
    eng, cfg, raw, wt, om64, om32 = _pulse_model("canon")
    d = eng.dims
    B, T = len(lengths), max(lengths)
    mel, noise = synthetic_inputs(73, B, T, steps_per_frame=d.wn_in_rows_per_frame)
    for ii, ll in enumerate(lengths):
        mel[ii, ll:] = np.nan                                   # frames behind an item's end are never read
    eng.forward(_dev(torch, mel), n_frames=_dev(torch, np.asarray(lengths, np.int32)), noise=_dev(torch, noise))
    f0 = eng.stage("f0").cpu().numpy().reshape(B, T * d.pulse_per_frame)
    items = None if B < 16 else [lengths.index(max(lengths)), lengths.index(min(lengths)), 0, B - 1]
    rec = fr.compare_f0(f0, fr.f0_reference(om64, mel, lengths, items), lengths, d.pulse_per_frame)
    print(f"\nf0 contour {cid}: {rec['ulps']:.4f} ulps at {rec['where']}")
    _print_record("f0/" + cid, {"ulps": rec["ulps"], "bar": 0.5, "lengths": lengths if items is None else [lengths[ii] for ii in items]})
    assert rec["ok"], f"the F0 contour is {rec['ulps']:.3f} float32 ulps off the float64 oracle at {rec['where']}"
    assert eng.conv_form_info()["f0_float64_chain"]

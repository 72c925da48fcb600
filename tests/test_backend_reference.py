"""The back-end stage comparator (tests/backend_reference.py) sees what it claims to see, on the CPU: it accepts the float32
port of the synthesis back end fed its own upstream stages, and it rejects planted defects that the end-to-end bars of the
suite let through -- VTF-net coefficients above the first 128-column tile (which the lifter rows of synthetic inputs
multiply by 0), an item's STFT frames padded at the batch length, a short item's PQMF reading one step of its neighbour,
the post-net losing the bias of one band.  Canonical SPEECH, a ragged batch of 9, 1 and 14 frames.

The "engine" here is the float32 port, computed stage by stage per item at its own length (port_backend_stages); a defect
alters a copy of its stages and the stages downstream are recomputed from the altered copy, as the engine would.  Each
defect is first shown to pass the bars the suite holds today: it moves the audio by less than 1e-4 * max(1, |audio|) and the
excitation by less than 2e-5 * max(1, |excitation|)."""
import numpy as np
import pytest

from backend_reference import (EPS_POS, K_PORT, BackendReference, backend_kind, failures, oracle_ceps_index,
                               oracle_excitation, oracle_frames, oracle_models, oracle_subbands, overlap_add_f32,
                               port_backend_stages)
from helpers import build_case, synthetic_inputs
from mbexwn_vocoder_amd.config import ModelDims

LENGTHS = [9, 1, 14]
# the bars the suite holds today: audio within 1e-4 * max(1, |audio|), excitation within 2e-5 * max(1, |excitation|)
OLD_BAR = {"audio": 1e-4, "excitation": 2e-5}


@pytest.fixture(scope="module")
def case():
    cfg, raw, wt = build_case("SPEECH", {})
    dims = ModelDims(cfg)
    om64, om32 = oracle_models(cfg, raw, wt)
    mel, noise = synthetic_inputs(5, len(LENGTHS), max(LENGTHS))
    got = port_backend_stages(om32, mel, noise, LENGTHS)
    ref = BackendReference(om64, om32, dims, cfg, got, mel, LENGTHS)
    return dims, om32, got, ref, mel


def _copy(got):
    return {kk: vv.copy() for kk, vv in got.items()}


def _downstream(om, dims, got, ii, changed):
    """Recompute item ii's stages behind the altered stage ``changed`` (cepstrum | subbands | excitation | frames) from the
    altered copy, as the engine would: subbands -> excitation -> frames -> audio, cepstrum -> frames."""
    T, hop, spf = LENGTHS[ii], dims.hop_size, dims.steps_per_frame
    if changed == "subbands":
        got["excitation"][ii, :T * hop] = oracle_excitation(om, got["subbands"][ii, :T * spf], dims).astype(np.float32)
    if changed in ("cepstrum", "subbands", "excitation"):
        got["frames"][ii, :T] = oracle_frames(om, got["excitation"][ii], got["cepstrum"][ii, :T], got["ceps_index"][ii, :T],
                                              T).astype(np.float32)
    got["audio"][ii, :T * hop] = overlap_add_f32(got["frames"][ii, :T], T, hop)
    return got


def _passes_todays_bars(dims, clean, bad):
    """The defect moves the audio and the excitation by less than the end-to-end bars (max over the items' valid range)."""
    moved = {}
    for name in ("audio", "excitation"):
        diff = amp = 0.0
        for ii, ll in enumerate(LENGTHS):
            n = ll * dims.hop_size
            diff = max(diff, float(np.abs(bad[name][ii, :n].astype(np.float64) - clean[name][ii, :n]).max()))
            amp = max(amp, float(np.abs(clean[name][ii, :n]).max()))
        moved[name] = (diff, OLD_BAR[name] * max(1.0, amp))
        assert diff <= OLD_BAR[name] * max(1.0, amp), f"the planted defect already fails today's {name} bar: {diff:.2e}"
    return moved


def _rejects(ref, mel, bad, label, moved):
    """The comparator as the GPU tests run it: the oracle fed the (defective) engine's own upstream stages."""
    ref = BackendReference(ref.om64, ref.om32, ref.dims, ref.cfg, bad, mel, LENGTHS)
    rep = ref.compare(bad)
    msg = failures(rep)
    print(f"\n{label}: audio moved {moved['audio'][0]:.2e} (today's bar {moved['audio'][1]:.1e}), excitation moved "
          f"{moved['excitation'][0]:.2e} (bar {moved['excitation'][1]:.1e})\n  comparator: {msg}")
    assert msg, f"{label}: the comparator accepted a planted defect"
    return rep, msg


def test_branches_of_the_canonical_model(case):
    dims = case[0]
    assert backend_kind(dims, case[3].cfg) == {"envelope": True, "lifter": True, "stft": "wave10_2", "pqmf": "mfma",
                                               "gain": False, "norm": False, "tail": "fused"}


def test_accepts_the_float32_port(case):
    dims, om32, got, ref, mel = case
    rep = ref.compare(got)
    print("\nfloat32 port: " + "  ".join(f"{kk} {rr['err']:.2e} (|ref| {rr['ref_max']:.3g}, tol {rr['tol']:.2e})"
                                           for kk, rr in rep.items() if "port_err" in rr))
    assert not failures(rep), failures(rep)
    assert set(rep) == {"cepstrum", "ceps_index", "subbands", "excitation", "frames", "audio"}
    assert rep["audio"]["bit_equal"] and rep["ceps_index"]["mismatch"] == 0
    for name in ("cepstrum", "subbands", "excitation", "frames"):
        rr = rep[name]
        assert 0.0 < rr["port_err"] <= 1e-5 * max(1.0, rr["ref_max"]), name


def test_synthetic_f0_leaves_the_upper_cepstrum_unused(case):
    """The blind spot this comparator closes: at synthetic-input F0 the selected lifter rows are all zero beyond coefficient
    127, so the second 128-column tile of the VTF-net's last convolution never reaches the audio."""
    dims, om32, got, ref, mel = case
    rows = set()
    for ii, ll in enumerate(LENGTHS):
        rows.update(int(rr) for rr in got["ceps_index"][ii, :ll])
    assert rows and max(rows) < 29 and min(rows) > 0
    assert np.all(om32.ceps_windows[sorted(rows)][:, 128:] == 0.0)


def test_rejects_upper_cepstrum_perturbed(case):
    """(a) Coefficient 200 of one frame scaled by 1 + 1e-4 (a second-tile column of the VTF-net's last convolution off)."""
    dims, om32, got, ref, mel = case
    bad = _copy(got)
    bad["cepstrum"][2, 5, 200] *= np.float32(1 + 1e-4)
    bad = _downstream(om32, dims, bad, 2, "cepstrum")
    moved = _passes_todays_bars(dims, got, bad)
    assert moved["audio"][0] == 0.0          # multiplied by exactly 0 before the audio
    rep, msg = _rejects(ref, mel, bad, "(a) cepstrum coefficient 200 x (1 + 1e-4)", moved)
    w = rep["cepstrum"]["where"]
    assert (w["item"], w["frame"], w["coefficient"], w["column_tile"], w["column_in_tile"]) == (2, 5, 200, 1, 72), msg
    assert [kk for kk, rr in rep.items() if not rr["ok"]] == ["cepstrum"], msg


def test_rejects_upper_cepstrum_dropped(case):
    """(a') The last coefficient (239) dropped in every frame of every item (a partly filled tile's last column lost)."""
    dims, om32, got, ref, mel = case
    bad = _copy(got)
    for ii, ll in enumerate(LENGTHS):
        bad["cepstrum"][ii, :ll, 239] = 0.0
        bad = _downstream(om32, dims, bad, ii, "cepstrum")
    moved = _passes_todays_bars(dims, got, bad)
    assert moved["audio"][0] == 0.0
    rep, msg = _rejects(ref, mel, bad, "(a') cepstrum coefficient 239 dropped", moved)
    assert rep["cepstrum"]["where"]["coefficient"] == 239, msg


def test_rejects_frames_padded_at_the_batch_length(case):
    """(b) Item 0 (9 frames of a 14-frame batch): its STFT frames see the excitation up to the batch length, where the
    padding holds 1/1000 of the PQMF ring-out of its last sub-band rows (what a synthesis at the batch length writes)."""
    dims, om32, got, ref, mel = case
    ii, T, Tm = 0, LENGTHS[0], max(LENGTHS)
    hop, spf, M = dims.hop_size, dims.steps_per_frame, dims.subbands
    sub = np.zeros((Tm * spf, M), np.float32)
    sub[:T * spf] = got["subbands"][ii, :T * spf]
    ext = oracle_excitation(om32, sub, dims).astype(np.float32)
    ext[:T * hop] = got["excitation"][ii, :T * hop]
    ext[T * hop:] *= np.float32(1e-3)
    assert np.abs(ext[T * hop:]).max() > 0.0
    bad = _copy(got)
    bad["frames"][ii, :T] = oracle_frames(om32, ext, got["cepstrum"][ii, :T], got["ceps_index"][ii, :T], T,
                                          signal_len=Tm * hop).astype(np.float32)
    bad = _downstream(om32, dims, bad, ii, "frames")
    moved = _passes_todays_bars(dims, got, bad)
    rep, msg = _rejects(ref, mel, bad, "(b) item 0's frames padded at the batch length", moved)
    w = rep["frames"]["where"]
    assert w["item"] == 0 and w["frames_to_end"] <= 2, msg
    assert [kk for kk, rr in rep.items() if not rr["ok"]] == ["frames"], msg


@pytest.mark.parametrize("source", ["neighbour", "own_padding"])
def test_rejects_pqmf_reading_one_step_past_the_end(case, source):
    """(c) The PQMF of item 0 reads one sub-band step past its end: the first row of its neighbour (item 1) or its own first
    padding row (here the row its WaveNet would have produced there), at 2e-5 of its size."""
    dims, om32, got, ref, mel = case
    ii, T = 0, LENGTHS[0]
    spf = dims.steps_per_frame
    if source == "neighbour":
        extra = got["subbands"][1, :1]
    else:
        # the row item 0's own WaveNet and post-net give at step T * spf when the item runs at the batch length
        mel, noise = synthetic_inputs(5, len(LENGTHS), max(LENGTHS))
        extra = port_backend_stages(om32, mel[:1], noise[:1], [max(LENGTHS)])["subbands"][0, T * spf:T * spf + 1]
    sub = np.concatenate((got["subbands"][ii, :T * spf], np.float32(2e-5) * extra))
    bad = _copy(got)
    bad["excitation"][ii, :T * dims.hop_size] = oracle_excitation(om32, sub, dims)[:T * dims.hop_size].astype(np.float32)
    bad = _downstream(om32, dims, bad, ii, "excitation")
    moved = _passes_todays_bars(dims, got, bad)
    rep, msg = _rejects(ref, mel, bad, f"(c) item 0's PQMF reads one step of {source}", moved)
    w = rep["excitation"]["where"]
    assert w["item"] == 0 and w["samples_to_end"] <= 60, msg
    assert not rep["excitation"]["ok"] and rep["frames"]["ok"], msg


def test_rejects_post_net_losing_the_bias_of_one_band(case):
    """(d) The post-net of every item losing 30 % of the bias of band 13 (|b| = 3.6e-5 with these weights; the whole bias
    moves the excitation by 5e-5, which today's excitation bar catches)."""
    dims, om32, got, ref, mel = case
    band = 13
    assert abs(float(om32.weight("post")[1][band])) < 1e-4
    bad = _copy(got)
    for ii, ll in enumerate(LENGTHS):
        bad["subbands"][ii, :ll * dims.steps_per_frame] = oracle_subbands(
            om32, got["wn_out"][ii, :ll * dims.steps_per_frame], None, dims, drop_bias=(band, 0.3)).astype(np.float32)
        bad = _downstream(om32, dims, bad, ii, "subbands")
    moved = _passes_todays_bars(dims, got, bad)
    rep, msg = _rejects(ref, mel, bad, f"(d) post-net losing 30 % of the bias of band {band}", moved)
    assert rep["subbands"]["where"]["band"] == band, msg
    assert not rep["subbands"]["ok"], msg


def test_index_comparator_equality_and_half_integer_excuse(case):
    """Lifter rows: one row off fails; a frame whose position lies within EPS_POS of a half-integer accepts either neighbour
    and is counted as excused; too many excused frames fail the case."""
    dims, om32, got, ref, mel = case
    bad = _copy(got)
    bad["ceps_index"][2, 3] += 1
    rep = ref.compare(bad, names=["ceps_index"])
    assert not rep["ceps_index"]["ok"] and rep["ceps_index"]["where"]["frame"] == 3, failures(rep)
    # a synthetic half-integer position: the oracle's own position moved onto 8.5 + EPS_POS / 2
    f0 = got["f0"][0, :LENGTHS[0] * dims.pulse_per_frame]
    idx, pos = oracle_ceps_index(ref.om64, f0)
    saved = {kk: vv.copy() for kk, vv in ref.ref[0].items()}
    try:
        ref.ref[0]["ceps_pos"] = pos.copy()
        ref.ref[0]["ceps_pos"][4] = 8.5 + EPS_POS / 2
        ref.ref[0]["ceps_index"] = idx.copy()
        ref.ref[0]["ceps_index"][4] = 9
        alt = _copy(got)
        alt["ceps_index"][0, :LENGTHS[0]] = idx
        alt["ceps_index"][0, 4] = 8
        rep = ref.compare(alt, names=["ceps_index"])
        assert rep["ceps_index"]["mismatch"] == 0 and rep["ceps_index"]["excused"] == 1
        assert not rep["ceps_index"]["ok"]            # 1 of 24 frames excused: above the 3 % a case may excuse
        ref.ref[0]["ceps_pos"][4] = 8.5 + 2 * EPS_POS
        rep = ref.compare(alt, names=["ceps_index"])
        assert rep["ceps_index"]["mismatch"] == 1 and not rep["ceps_index"]["ok"]
    finally:
        ref.ref[0] = saved


def test_audio_is_held_bit_for_bit(case):
    """The audio is the exact overlap-add of the engine's own frames: one ulp off in one sample fails, and so does a non-zero
    sample behind an item's end."""
    dims, om32, got, ref, mel = case
    bad = _copy(got)
    a = bad["audio"][2]
    a[777] = np.nextafter(a[777], np.float32(np.inf))
    rep = ref.compare(bad, names=["audio"])
    assert not rep["audio"]["ok"] and rep["audio"]["where"]["sample"] == 777, failures(rep)
    bad = _copy(got)
    bad["audio"][0, LENGTHS[0] * dims.hop_size + 5] = 1e-30
    rep = ref.compare(bad, names=["audio"])
    assert not rep["audio"]["ok"] and rep["audio"]["where"]["behind_the_end"], failures(rep)
    assert K_PORT == 8.0


@pytest.mark.parametrize("over,win,fft", [({"mbexwn_config:internal_win_size_s": 0.08}, 1920, 2048),
                                          ({"mbexwn_config:internal_fft_over": 1}, 1200, 4096)])
def test_oracle_follows_the_internal_stft_settings(over, win, fft):
    """The oracle's STFT window and FFT size follow internal_win_size_s / internal_fft_over as the reference does
    (custom_pulsed_generator.py:391-400), with the same values as ModelDims, and its synthesis window is the engine's
    (tables.inverse_stft_window_f32) also for a window that is not a whole number of hops."""
    from mbexwn_vocoder_amd.tables import inverse_stft_window_f32
    cfg, raw, wt = build_case("SPEECH", dict(over, **{"mbexwn_config:pp_mod_subnet:n_channels": 32,
                                                      "mbexwn_config:pp_mod_subnet:n_layers": 2}))
    dims = ModelDims(cfg)
    om = oracle_models(cfg, raw, wt)[0]
    assert (om.stft_win, om.fft_size) == (dims.stft_win, dims.fft_size) == (win, fft)
    eng_win = inverse_stft_window_f32(win, dims.hop_size)     # (float32 cos arguments: a few float32 ulps apart)
    np.testing.assert_allclose(om.inv_win, eng_win, rtol=0, atol=1e-6 * float(np.abs(eng_win).max()))

"""The synthesis back end stage by stage against the float64 oracle (tests/backend_reference.py).

Every case runs a ragged batch (short items next to long ones, one item of 1 frame) through the engine and holds its
"cepstrum", "ceps_index", "subbands", "excitation" and "frames" stages to the oracle fed the engine's own upstream stages,
item by item at the item's own length, at tol = max(K * float32-port error, F * max(1, |ref|)) (the lifter row: equal); the
audio is held bit for bit to the overlap-add of the engine's own frames.  The cases cover every branch of the back end
(test_gpu_cases_cover_every_backend_branch), the whole lifter table with both clamps of the log-F0 range (an external
contour sweeping 25 -> 800 Hz, and transposition), and one 16-item launch large enough for the LDS-DMA mel-rate tiles.
Each case prints one JSON line ("backend stages record ...") with its errors against their bars.

The padding contract of include/mbexwn.h is held bit for bit on the back-end stages too: the same ragged batch with its
padding frames of mel and noise at 0, 1e30 and NaN gives the same stages over every item's valid range."""
import json

import numpy as np
import pytest

from backend_reference import (N_LIFTER_ROWS, BackendReference, assert_matches, backend_kind, engine_backend_stages,
                               oracle_models, record, summary)
from helpers import GOLDEN_CASES, build_case, synthetic_inputs
from mbexwn_vocoder_amd.config import ModelDims
from test_gpu_configs import _GEOMETRIES as CONFIG_GEOMETRIES

# ragged lengths in frames: the 1-frame item and short items next to long ones; none a multiple of the 4 frames of a
# wave-per-frame STFT block, the longest across the 64-step PQMF blocks
RAGGED = [26, 1, 41, 7, 13, 33, 6]
# the lifter sweep: item 0 rises 25 -> 800 Hz over 50 of its 70 frames (flat 10 frames beyond each clamp), item 2 falls
# 800 -> 25 Hz over 30 frames, the short items sit beyond the clamps
SWEEP = [70, 1, 44, 7, 3]
# one launch of 16 items of 700 - 900 frames: 16 x 900 rows >= 3 * 4096, the mel-rate convolutions take the LDS-DMA tile
LARGE = [800, 700, 900, 760, 880, 720, 840, 740, 860, 780, 820, 710, 890, 750, 870, 730]
LARGE_CHECK = [LARGE.index(max(LARGE)), LARGE.index(min(LARGE)), LARGE.index(800)]

_P, _M, _W = "preprocess_config:", "mbexwn_config:", "mbexwn_config:pp_mod_subnet:"
_SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 3}
_NORM = dict(_SMALL, **{"mbexwn_config:normalize_rms_from_mell": True, "mbexwn_config:normalize_rms_num_smooth_iters": 2,
                        "mbexwn_config:normalize_compressor_exp": 0.8, "mbexwn_config:max_norm_fact": 200.0})
GEOMETRIES = {
    "speech": ("SPEECH", {}),
    "voice": ("VOICE", {}),
    **{name: ("SPEECH", CONFIG_GEOMETRIES[name]) for name in ("ceps400", "win1600", "sr16k_hop200", "bands30_out60",
                                                             "bands12_fold4")},
    **{name: GOLDEN_CASES[name][:2] for name in ("nopqmf", "subgain", "subgain_e", "energy", "mixed_b", "psoff")},
    "normmel": ("SPEECH", _NORM),
    # more than 256 cepstral coefficients (stft_filter_wave_kernel<16,16>) with the energy-preserving gain
    "ceps400_energy": ("SPEECH", dict(CONFIG_GEOMETRIES["ceps400"], **{"mbexwn_config:spect_filters_preserve_energy": True})),
    # hop 400: an STFT window of 4 hop = 1600 > 1280 samples (stft_filter_wave_kernel<16,16> through its window condition,
    # 240 coefficients), 16 bands of 25 rows, 8 pulse channels at 12 kHz
    "hop400": ("SPEECH", {_P + "hop_size": 400, _P + "win_size": 1600, _M + "pulse_rate_factor": 2, _M + "pulse_channels": 8,
                          _M + "multi_band_config": {"subbands": 16, "taps": 128, "cutoff_ratio": 0.06, "beta": 9.0},
                          _W + "cond_lin_upsampling": 5, _W + "n_channels": 32, _W + "n_layers": 2}),
}

# (id, geometry, lengths, forward arguments: "sweep" = the external F0 sweep, or {"transposition": x})
CASES = [
    ("speech", "speech", RAGGED, {}),
    ("voice", "voice", RAGGED, {}),
    ("speech-f0-sweep", "speech", SWEEP, {"f0": "sweep"}),
    ("speech-transpose-0.4", "speech", RAGGED, {"transposition": 0.4}),
    ("speech-transpose-2.5", "speech", RAGGED, {"transposition": 2.5}),
    ("ceps400", "ceps400", RAGGED, {}),
    ("ceps400_energy", "ceps400_energy", RAGGED, {}),
    ("hop400", "hop400", RAGGED, {}),
    ("win1600", "win1600", RAGGED, {}),
    ("sr16k_hop200", "sr16k_hop200", RAGGED, {}),
    ("bands30_out60", "bands30_out60", RAGGED, {}),
    ("bands12_fold4", "bands12_fold4", RAGGED, {}),
    ("nopqmf", "nopqmf", RAGGED, {}),
    ("subgain", "subgain", RAGGED, {}),
    ("subgain_e", "subgain_e", RAGGED, {}),
    ("energy", "energy", RAGGED, {}),
    ("mixed_b", "mixed_b", RAGGED, {}),       # valid padding, cepstral constraint: no lifter row, ceps_index not written
    ("psoff", "psoff", RAGGED, {}),
    ("normmel", "normmel", RAGGED, {}),
    ("speech-large", "speech", LARGE, {}),
]
# the branches the cases must take (backend_reference.backend_kind)
EXPECTED = {
    "speech": {"stft": "wave10_2", "pqmf": "mfma", "tail": "fused"},
    "voice": {"stft": "wave10_2", "pqmf": "mfma", "tail": "fused"},
    "ceps400": {"stft": "wave16_16"},
    "ceps400_energy": {"stft": "wave16_16"},
    "hop400": {"stft": "wave16_16", "pqmf": "mfma"},
    # preprocess win_size is the mel analysis window (RMS normalisation); the STFT filter's window is 4 hop = 1200 here
    "win1600": {"stft": "wave10_2"},
    "sr16k_hop200": {"stft": "generic"},
    "bands30_out60": {"pqmf": "generic", "tail": "unfused"},
    "bands12_fold4": {"pqmf": "mfma"},
    "nopqmf": {"pqmf": "reshape"},
    "subgain": {"gain": True, "envelope": False},
    "subgain_e": {"gain": True, "envelope": False},
    "mixed_b": {"lifter": False, "envelope": True},
    "psoff": {"envelope": False, "gain": False},
    "normmel": {"norm": True},
}
# the tail kernel the library must report (mbx_kernel_report): 60 output channels do not fit wn_tail2_kernel / wn_tail_kernel
TAIL_KERNELS = {"speech": "tail2_nj20", "voice": "tail2_nj22", "bands30_out60": "unfused"}


def _model(geom):
    voice, over = GEOMETRIES[geom]
    return build_case(voice, over)


def test_gpu_cases_cover_every_backend_branch():
    """(CPU) The cases take every branch of the back end that the dispatch code can take: the three STFT kernels (the
    wide one through both of its conditions), the three PQMF forms, the fused and the unfused tail (at that level: "fused"
    covers wn_tail2_kernel, wn_tail_kernel and the folded tail alike), the sub-band gains (with and without the
    energy-preserving mean), no envelope at all, no lifter row, the RMS-normalisation gain -- derived from ModelDims /
    config by the conditions of launch_stft_filter, launch_pqmf, launch_wn_tail and mbx_forward.hip (run_tail, run_backend).  The overlap-add loop for
    windows longer than 4 hop is not reachable: mbx_create refuses such a model (test_wide_window_is_refused)."""
    kinds = {}
    for geom in GEOMETRIES:
        cfg, _, _ = _model(geom)
        kinds[geom] = backend_kind(ModelDims(cfg), cfg)
    for geom, want in EXPECTED.items():
        got = {kk: kinds[geom][kk] for kk in want}
        assert got == want, f"{geom}: branches {kinds[geom]}, expected {want}"
    used = [kinds[case[1]] for case in CASES]
    assert {kk["stft"] for kk in used} == {"wave10_2", "wave16_16", "generic", None}
    # <16,16> through both of its conditions: more than 256 coefficients, a window of more than 1280 samples
    dims = {case[1]: ModelDims(_model(case[1])[0]) for case in CASES}
    assert any(kinds[gg]["stft"] == "wave16_16" and dd.n_ceps > 256 and dd.stft_win <= 1280 for gg, dd in dims.items())
    assert any(kinds[gg]["stft"] == "wave16_16" and dd.n_ceps <= 256 and dd.stft_win > 1280 for gg, dd in dims.items())
    # the overlap-add runs its four-frame form: mbx_create refuses a window other than 4 hop (test_wide_window_is_refused)
    assert all(dd.stft_win == 4 * dd.hop_size for dd in dims.values())
    assert {kk["pqmf"] for kk in used} == {"mfma", "generic", "reshape"}
    assert {kk["tail"] for kk in used} == {"fused", "unfused"}
    for flag in ("envelope", "lifter", "gain", "norm"):
        assert {kk[flag] for kk in used} == {True, False}, flag
    assert any(kk["gain"] and ModelDims(_model(case[1])[0]).preserve_energy for case, kk in zip(CASES, used))
    assert any(kk["envelope"] and ModelDims(_model(case[1])[0]).preserve_energy for case, kk in zip(CASES, used))
    assert len({case[0] for case in CASES}) == len(CASES)
    assert len(LARGE) == 16 and len(LARGE) * max(LARGE) >= 3 * 4096 and min(LARGE) >= 700
    for case in CASES:
        assert case[1] in GEOMETRIES
        assert case[2] is LARGE or 1 in case[2], f"{case[0]}: no 1-frame item"
    print("\nback-end branches: " + "; ".join(f"{case[0]}: {kinds[case[1]]}" for case in CASES))


def sweep_contour(lengths, ppf):
    """External F0 (B, T * ppf) in Hz: item 0 rises 25 -> 800 Hz on a log scale, item 2 falls, the others sit beyond the
    clamps (25 Hz and 800 Hz); every item is flat for 10 frames before and after its sweep."""
    B, T = len(lengths), max(lengths)
    f0 = np.full((B, T * ppf), 25.0, dtype=np.float64)
    for ii, ll in enumerate(lengths):
        n = ll * ppf
        if ii in (0, 2) and ll > 20:
            sw = np.geomspace(25.0, 800.0, (ll - 20) * ppf)
            if ii == 2:
                sw = sw[::-1]
            f0[ii, :10 * ppf] = sw[0]
            f0[ii, 10 * ppf:10 * ppf + sw.size] = sw
            f0[ii, 10 * ppf + sw.size:] = sw[-1]
        else:
            f0[ii, :n] = 800.0 if ii % 2 else 25.0
    return f0.astype(np.float32)


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    if not _torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return _torch


def _inputs(dims, lengths, seed):
    B, T = len(lengths), max(lengths)
    mel, noise = synthetic_inputs(seed, B, T, steps_per_frame=dims.wn_in_rows_per_frame)
    return mel, noise if dims.noise_sigma else None


def _forward(torch, eng, mel, noise, lengths, **kwargs):
    nf = torch.as_tensor(lengths, dtype=torch.int32).cuda()
    dev = {kk: (torch.as_tensor(vv).cuda() if isinstance(vv, np.ndarray) else vv) for kk, vv in kwargs.items()}
    audio = eng.forward(torch.as_tensor(mel).cuda(), n_frames=nf,
                        noise=torch.as_tensor(noise).cuda() if noise is not None else None, **dev)
    return audio.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("cid,geom,lengths,kwargs", CASES, ids=[case[0] for case in CASES])
def test_backend_stages_match_the_oracle(torch, cid, geom, lengths, kwargs):
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    cfg, raw, wt = _model(geom)
    eng = MBExWNEngine(cfg, raw, wt)
    try:
        dims = eng.dims
        B, T = len(lengths), max(lengths)
        mel, noise = _inputs(dims, lengths, seed=613)
        fw = dict(kwargs)
        if fw.get("f0") == "sweep":
            fw["f0"] = sweep_contour(lengths, dims.pulse_per_frame)
        audio = _forward(torch, eng, mel, noise, lengths, **fw)
        got = engine_backend_stages(eng, B, T)
        got["audio"] = audio
        tail = eng.conv_form_info()["tail_kernel"]
    finally:
        eng.close()
    if geom in TAIL_KERNELS:
        assert tail == TAIL_KERNELS[geom], f"{cid}: tail kernel {tail}, expected {TAIL_KERNELS[geom]}"
    items = LARGE_CHECK if lengths is LARGE else None
    om64, om32 = oracle_models(cfg, raw, wt)
    ref = BackendReference(om64, om32, dims, cfg, got, mel, lengths, items=items)
    rep = ref.compare(got)
    kind = backend_kind(dims, cfg)
    rec = {"kind": kind, "lengths": lengths if items is None else [lengths[ii] for ii in items], **record(rep)}
    if "ceps_index" in rep:
        ci = rep["ceps_index"]
        rec["ceps_index"].update(rows_selected=ci["rows"])
    print(f"\nbackend stages {cid}: {summary(rep)}")
    print("backend stages record " + json.dumps({cid: rec}))        # with -s: one JSON line per case
    assert_matches(rep)
    if kind["lifter"]:
        ci = rep["ceps_index"]
        if "f0" in kwargs:
            # the sweep selects every lifter row and both clamp ends of the log-F0 range
            assert ci["rows"] == list(range(N_LIFTER_ROWS)), f"{cid}: lifter rows selected {ci['rows']}"
            assert ci["low_clamp_frames"] > 0 and ci["high_clamp_frames"] > 0, ci
        elif kwargs.get("transposition", 1.0) != 1.0:
            lo, hi = min(ci["rows"]), max(ci["rows"])
            assert (lo <= 2) if kwargs["transposition"] < 1 else (hi >= 18), f"{cid}: lifter rows {ci['rows']}"
    else:
        assert "ceps_index" not in rep


PAD_GEOMS = ["speech", "sr16k_hop200", "bands30_out60", "subgain", "normmel"]


@pytest.mark.gpu
@pytest.mark.parametrize("geom", PAD_GEOMS)
def test_backend_padding_frames_are_never_read(torch, geom):
    """The same ragged batch three times, its padding frames of mel and noise at 0, 1e30 and NaN: every back-end stage over
    each item's valid range is bit-identical across the three, and the audio behind each item's end is exactly 0."""
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    cfg, raw, wt = _model(geom)
    eng = MBExWNEngine(cfg, raw, wt)
    dims = eng.dims
    lengths = RAGGED
    B, T = len(lengths), max(lengths)
    rpf = dims.wn_in_rows_per_frame
    mel, noise = _inputs(dims, lengths, seed=617)
    per_frame = {"mel_in": 1, "cepstrum": 1, "ceps_index": 1, "subbands": dims.steps_per_frame, "excitation": dims.hop_size, "frames": 1,
                 "f0": dims.pulse_per_frame}
    runs = {}
    try:
        for fill in (0.0, 1e30, np.nan):
            m = mel.copy()
            n = None if noise is None else noise.copy()
            for ii, ll in enumerate(lengths):
                m[ii, ll:] = fill
                if n is not None:
                    n[ii, ll * rpf:] = fill
            audio = _forward(torch, eng, m, n, lengths)
            st = engine_backend_stages(eng, B, T)
            st.pop("wn_out")
            runs[fill] = (audio, st)
    finally:
        eng.close()
    base_audio, base = runs[0.0]
    for fill in (1e30, np.nan):
        audio, st = runs[fill]
        for ii, ll in enumerate(lengths):
            assert np.all(audio[ii, ll * dims.hop_size:] == 0.0), f"{geom}: audio behind item {ii}'s end, padding {fill}"
            assert np.array_equal(audio[ii, :ll * dims.hop_size], base_audio[ii, :ll * dims.hop_size])
            for name, arr in st.items():
                a, b = arr[ii, :ll * per_frame[name]], base[name][ii, :ll * per_frame[name]]
                bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32)) if a.dtype == np.float32 else np.argwhere(a != b)
                assert bad.size == 0, f"{geom}: {name} of item {ii} ({ll} frames) differs with padding {fill}: first at " \
                                      f"{tuple(bad[0])}"
    for ii, ll in enumerate(lengths):
        assert np.all(np.isfinite(base_audio[ii, :ll * dims.hop_size]))


@pytest.mark.gpu
def test_wide_window_is_refused(torch):
    """A model whose STFT window is not 4 hop (internal_win_size_s = 0.08 s: 1920 samples at hop 300; the reference allows
    it, custom_pulsed_generator.py:391-400) is refused by mbx_create with MBX_ERR_UNSUPPORTED before anything runs, so
    overlap_add_kernel's loop for windows longer than 4 hop and a window that is not a whole number of hops are never
    reached by the forward pass."""
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    cfg, raw, wt = build_case("SPEECH", dict(_SMALL, **{_M + "internal_win_size_s": 0.08}))
    dims = ModelDims(cfg)
    assert (dims.stft_win, dims.fft_size) == (1920, 2048) and dims.stft_win > 4 * dims.hop_size
    with pytest.raises(NotImplementedError, match="win == 4\\*hop"):
        MBExWNEngine(cfg, raw, wt)

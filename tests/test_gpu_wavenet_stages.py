"""The WaveNet kernels stage by stage against the float64 oracle at float32-rounding tolerance (tests/wn_reference.py).

Every case runs a ragged batch through the engine, asserts which gate kernels ran (mbx_conv_form_info.gate_kernel) and holds
"wn_out", "wn_hidden" and (with keep_skip) "wn_skip" to the oracle's WaveNet fed the engine's own excitation rows, over every
item's valid rows, at tol = max(K * float32-port error, F * max(1, |ref|)).  The lengths straddle the 128- and 256-row tiles
(20 rows per frame) and an item of one frame is shorter than every dilation >= 32; the ragged order puts short items next
to long ones, so that one item leaking into its neighbour shows.  The end-to-end tests hold the audio to 1e-4: a lost low
half of one channel tile, a row off at a tile seam or a leak between items passes that bar (test_wn_reference.py) and not
this one.  A failure names the worst item, row and channel and the row's place in its 256- and 128-row tiles.

The padding contract of include/mbexwn.h ("every boundary op honours the item's own length") is held bit for bit: the same
ragged batch with its padding frames of mel and noise at 0, 1e30 and NaN."""
import json

import numpy as np
import pytest

from helpers import build_case, synthetic_inputs
from wn_reference import WaveNetReference, assert_matches, engine_stages, oracle_models, summary, wavenet_inputs

# ragged lengths in frames: 20 - 1040 rows around the 128- / 256-row tiles, short next to long
RAGGED = [26, 1, 52, 7, 13, 51, 6, 25, 12]
# the 12-layer model (dilations 1 .. 2048): items shorter and longer than the deepest layers reach (110 frames = 2200 rows)
DEEP = [13, 110, 1, 52, 7]
# one launch of 16 items of 400 - 700 frames: the large-launch kernel shapes (256-row F(4,3), wn_resskip_wide, wn_gate_f16w);
# the oracle checks the longest, the shortest and one in the middle
LARGE = [560, 400, 700, 420, 640, 460, 520, 680, 440, 600, 480, 620, 500, 660, 540, 580]
LARGE_CHECK = [LARGE.index(max(LARGE)), LARGE.index(min(LARGE)), LARGE.index(560)]
LENGTHS = {"ragged": (RAGGED, None), "deep": (DEEP, None), "large": (LARGE, LARGE_CHECK)}

_WN = "mbexwn_config:pp_mod_subnet:"
GEOMETRIES = {
    "speech": ("SPEECH", {}),                                                   # C = 320, 5 layers, d <= 16
    "voice": ("VOICE", {}),                                                     # C = 340: a partial 32-channel tile
    "deep12": ("SPEECH", {_WN + "n_layers": 12}),                               # d <= 2048: strided F(4,3), direct fall-back
    "c36": ("SPEECH", {_WN + "n_channels": 36, _WN + "n_layers": 3}),
    "c12": ("SPEECH", {_WN + "n_channels": 12, _WN + "n_layers": 3}),           # too narrow for the Winograd kernels; wn_tail_kernel
    "l3": ("SPEECH", {_WN + "n_layers": 3}),
    "lin5": ("SPEECH", {_WN + "cond_lin_upsampling": 5}),                       # layer 0 not folded (conditioning rows)
    "lin20": ("SPEECH", {_WN + "cond_lin_upsampling": 20}),
    "gfu": ("SPEECH", {_WN + "activation": "gfu"}),
    "gsu": ("SPEECH", {_WN + "activation": "gsu"}),
    "glu": ("SPEECH", {_WN + "activation": "glu"}),
    "groups2": ("SPEECH", {_WN + "n_ch_groups": 2}),
    "causal": ("SPEECH", {_WN + "padding": "CAUSAL"}),
}

F43 = {"conv_form": "f43"}
FS, PS = "folded_start", "f43_psplit"
# (id, geometry, lengths, engine arguments, the gate kernels the forward must run)
CASES = [
    # the forms on SPEECH (9 items, 1040 rows: 450 256-row blocks -> the product-split shape under the default policy)
    ("speech-direct", "speech", "ragged", {"conv_form": "direct"}, {FS, "direct"}),
    ("speech-f23", "speech", "ragged", {"conv_form": "f23"}, {FS, "f23"}),
    ("speech-f43", "speech", "ragged", F43, {FS, PS}),
    ("speech-f43-invariant", "speech", "ragged", {"conv_form": "f43", "batch_invariant": True}, {FS, "f43"}),
    ("speech-auto", "speech", "ragged", {"conv_form": "auto"}, {FS, PS}),
    # the F(4,3) block shapes pinned (tune_gate_shape 1 | 2 | 3: 256-row, product-split, product-split half column tiles)
    ("speech-f43-256row", "speech", "ragged", dict(F43, tune={"gate_shape": 1}), {FS, "f43"}),
    ("speech-f43-psplit", "speech", "ragged", dict(F43, tune={"gate_shape": 2}), {FS, PS}),
    ("speech-f43-hsplit", "speech", "ragged", dict(F43, tune={"gate_shape": 3}), {FS, "f43_hsplit"}),
    # the res/skip variants: the wave-tiled kernel's three column splits, and the plain kernel (wave tiles off)
    ("speech-rs-split1", "speech", "ragged", dict(F43, tune={"resskip_split": 1}), {FS, PS}),
    ("speech-rs-split2", "speech", "ragged", dict(F43, tune={"resskip_split": 2}), {FS, PS}),
    ("speech-rs-split3", "speech", "ragged", dict(F43, tune={"resskip_split": 3}), {FS, PS}),
    ("speech-rs-nowave", "speech", "ragged", dict(F43, tune={"resskip_wave_tiles": -1}), {FS, PS}),
    # geometries
    ("voice-f43", "voice", "ragged", F43, {FS, PS}),
    ("voice-f43-256row", "voice", "ragged", dict(F43, tune={"gate_shape": 1}), {FS, "f43"}),
    ("deep12-f43", "deep12", "deep", F43, {FS, PS, "f43_strided_psplit", "direct"}),
    # batch_invariant keeps F(4,3) at every dilation (no direct fall-back); the strided block shape still follows the cost
    # rule (both shapes give the same bits)
    ("deep12-f43-invariant", "deep12", "deep", {"conv_form": "f43", "batch_invariant": True},
     {FS, "f43", "f43_strided", "f43_strided_psplit"}),
    ("c36-f43", "c36", "ragged", F43, {FS, "f43_hsplit"}),
    ("c12-f43", "c12", "ragged", F43, {FS, "direct"}),
    ("lin5-f43", "lin5", "ragged", F43, {"f43"}),
    ("lin20-f43", "lin20", "ragged", F43, {FS, PS}),
    ("gfu-f43", "gfu", "ragged", F43, {FS, PS}),
    ("gsu-f43", "gsu", "ragged", F43, {FS, PS}),
    ("glu-f43", "glu", "ragged", F43, {FS, PS}),
    ("groups2-f43", "groups2", "ragged", F43, {FS, PS}),
    ("causal-auto", "causal", "ragged", {"conv_form": "auto"}, {"direct"}),
    ("speech-keep-skip", "speech", "ragged", dict(F43, keep_skip=True), {PS}),
    ("speech-keep-start", "speech", "ragged", dict(F43, keep_start=True), {PS}),
    # split half precision, held to the same bar; SPEECH and the 3-layer model take the plane-only hidden state, the 12-layer
    # model does not (dilations above 16 run the float32 gate kernels)
    ("speech-split", "speech", "ragged", dict(F43, precision="split_f16"), {FS, "split_f16"}),
    ("l3-split", "l3", "ragged", dict(F43, precision="split_f16"), {FS, "split_f16"}),
    ("deep12-split", "deep12", "deep", dict(F43, precision="split_f16"), {FS, "split_f16", "f43_strided_psplit", "direct"}),
    # large launches
    ("large-f43", "speech", "large", F43, {FS, "f43"}),
    ("large-split", "speech", "large", dict(F43, precision="split_f16"), {FS, "split_f16"}),
]
PLANES_ONLY = {"speech-split", "l3-split", "large-split"}
_REFS = {}


def test_gpu_cases_cover_every_gate_kernel():
    """(CPU) Every gate kernel the library reports is expected by at least one stage case: a new kernel without a case here
    fails the suite."""
    from mbexwn_vocoder_amd.engine import GATE_KERNEL_NAMES
    declared = set().union(*(case[4] for case in CASES))
    assert declared <= set(GATE_KERNEL_NAMES.values())
    assert declared == set(GATE_KERNEL_NAMES.values()) - {"none"}
    assert len({case[0] for case in CASES}) == len(CASES)
    for case in CASES:
        assert case[1] in GEOMETRIES and case[2] in LENGTHS


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    if not _torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return _torch


def _inputs(lengths, seed=907):
    T = max(lengths)
    mel, noise = synthetic_inputs(seed, len(lengths), T)
    return mel, noise


def _reference(geom, lkey, cfg, raw, wt, mel, noise, pulse):
    """The oracle's WaveNet stages for the checked items, cached per geometry, batch and excitation bits (the forms share
    one F0-net and oscillator, so their engines feed the WaveNet the same rows)."""
    lengths, items = LENGTHS[lkey]
    key = (geom, lkey, hash(pulse.tobytes()))
    if key not in _REFS:
        om64, om32 = oracle_models(cfg, raw, wt)
        xs = wavenet_inputs(om64, pulse, noise, lengths, 20)
        _REFS[key] = WaveNetReference(om64, om32, xs, mel, lengths, 20, items=items)
    return _REFS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("cid,geom,lkey,kwargs,kernels", CASES, ids=[case[0] for case in CASES])
def test_wavenet_stages_match_the_oracle(torch, cid, geom, lkey, kwargs, kernels):
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    voice, over = GEOMETRIES[geom]
    cfg, raw, wt = build_case(voice, over)
    lengths, items = LENGTHS[lkey]
    B, T = len(lengths), max(lengths)
    mel, noise = _inputs(lengths)
    eng = MBExWNEngine(cfg, raw, wt, **kwargs)
    rpf = eng.dims.wn_in_rows_per_frame
    assert rpf == 20
    nf = torch.as_tensor(lengths, dtype=torch.int32).cuda()
    audio = eng.forward(torch.as_tensor(mel).cuda(), n_frames=nf, noise=torch.as_tensor(noise).cuda()).cpu().numpy()
    info = eng.conv_form_info()
    ran = info["gate_kernels"]
    assert len(ran) == eng.dims.wn_layers and set(ran) == kernels, f"{cid}: gate kernels {ran}, expected {sorted(kernels)}"
    if kwargs.get("precision") == "split_f16":
        assert not info["split_rejected"] and info["split_f16_layers"] == eng.dims.wn_layers - 1, info
    names = ["wn_out", "wn_hidden"] + (["wn_skip"] if kwargs.get("keep_skip") else [])
    got = engine_stages(eng, names, B, T, items=items)
    planes = True
    try:
        eng.stage("wn_hidden_planes")
    except ValueError:
        planes = False
    assert planes == (cid in PLANES_ONLY), f"{cid}: plane-only hidden state {planes}"
    pulse = eng.stage("pulse").cpu().numpy().reshape(B, T * rpf, -1)
    eng.close()
    for ii, ll in enumerate(lengths):
        assert np.all(np.isfinite(audio[ii, :ll * 300])) and np.all(audio[ii, ll * 300:] == 0.0), f"{cid}: audio of item {ii}"
    ref = _reference(geom, lkey, cfg, raw, wt, mel, noise, pulse)
    rep = ref.compare(got, names=names)
    record = {"kernels": ran, **{kk: {"err": vv["err"], "tol": vv["tol"], "port_err": vv["port_err"],
                                      "ref_max": vv["ref_max"]} for kk, vv in rep.items()}}
    print(f"\nwavenet stages {cid}: {summary(rep)}  kernels {ran}")
    print("wavenet stages record " + json.dumps({cid: record}))       # with -s: one JSON line per case
    assert_matches(rep)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["f43", "direct", "split_f16"])
def test_padding_frames_are_never_read(torch, form):
    """The same ragged batch three times, its padding frames of mel and noise at 0, 1e30 and NaN: the audio and every WaveNet
    stage of the items' valid rows are bit-identical across the three, and the audio behind each item's end is exactly 0."""
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    cfg, raw, wt = build_case("SPEECH", {})
    kwargs = {"conv_form": "f43", "precision": "split_f16"} if form == "split_f16" else {"conv_form": form}
    eng = MBExWNEngine(cfg, raw, wt, **kwargs)
    lengths = RAGGED
    B, T = len(lengths), max(lengths)
    mel, noise = _inputs(lengths, seed=911)
    nf = torch.as_tensor(lengths, dtype=torch.int32).cuda()
    runs = {}
    for fill in (0.0, 1e30, np.nan):
        m, n = mel.copy(), noise.copy()
        for ii, ll in enumerate(lengths):
            m[ii, ll:] = fill
            n[ii, ll * 20:] = fill
        audio = eng.forward(torch.as_tensor(m).cuda(), n_frames=nf, noise=torch.as_tensor(n).cuda()).cpu().numpy()
        st = engine_stages(eng, ["wn_out", "wn_hidden"], B, T)
        st["pulse"] = eng.stage("pulse").cpu().numpy().reshape(B, T * 20, -1)
        runs[fill] = (audio, st)
    eng.close()
    base_audio, base_st = runs[0.0]
    for fill in (1e30, np.nan):
        audio, st = runs[fill]
        for ii, ll in enumerate(lengths):
            assert np.array_equal(audio[ii, :ll * 300], base_audio[ii, :ll * 300]), f"{form}: audio of item {ii}, padding {fill}"
            assert np.all(audio[ii, ll * 300:] == 0.0), f"{form}: audio behind item {ii}'s end, padding {fill}"
            for name in st:
                a, b = st[name][ii, :ll * 20], base_st[name][ii, :ll * 20]
                bad = np.argwhere(a != b)
                assert bad.size == 0, f"{form}: {name} of item {ii} ({ll} frames) differs with padding {fill}: first at row " \
                                      f"{bad[0][0]} channel {bad[0][1]}"
    for ii, ll in enumerate(lengths):
        assert np.all(np.isfinite(base_audio[ii, :ll * 300]))

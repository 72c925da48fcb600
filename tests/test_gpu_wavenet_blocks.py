"""The multi-block WaveNet (run_wavenet_blocks), the generic kernels of handles without weight images, and the pulse-PQMF and
sub-harmonic inputs, stage by stage against the float64 oracle at float32-rounding tolerance (tests/wn_blocks_reference.py).

Every case runs one ragged batch, asserts the gate kernel of every layer of every block (mbx_conv_form_info.gate_kernel,
block-major), on the block runner and on handles without weight images the res/skip kernel of every layer and the tail kernel
too (mbx_kernel_report), and holds "pulse_ana", "cond" / "cond<b>", the last block's "wn_hidden" and "wn_skip", and "wn_out" to the
oracle fed the engine's own WaveNet input, over every item's valid rows, at tol = max(8 * float32-port error, 5e-7 *
max(1, |ref|)).  The lengths straddle the 128- and 256-row tiles at 5, 10 and 20 rows per frame (the rates of the blocks)
and put a 1-frame item next to long ones.  Each case prints one JSON line with the worst error and the bar per tensor.

The padding contract (every boundary op honours the item's own length) is held bit for bit: the padding frames of mel and
noise at 0, 1e30 and NaN."""
import json

import numpy as np
import pytest

from helpers import GOLDEN_CASES, build_case, synthetic_inputs
from mbexwn_vocoder_amd.config import ModelDims
from wn_blocks_reference import (BlocksReference, assert_matches, block_geometry, engine_stages, oracle_models, stage_layout,
                                 summary)

# ragged lengths in frames, short next to long: 5 - 1040 rows around the 128- / 256-row tiles at 5, 10 and 20 rows per frame
RAGGED = [26, 1, 52, 7, 13, 51, 6, 25, 12]
# the 12-layer model (dilations 1 .. 2048): items shorter and longer than the deepest layers reach
DEEP = [13, 110, 1, 52, 7]
# one launch of 16 items of 400 - 700 frames (>= 64 000 rows at block 0: the large-launch tiles of conv1d); the oracle checks
# the longest, the shortest and one in the middle
LARGE = [560, 400, 700, 420, 640, 460, 520, 680, 440, 600, 480, 620, 500, 660, 540, 580]
LARGE_CHECK = [LARGE.index(max(LARGE)), LARGE.index(min(LARGE)), LARGE.index(560)]
LENGTHS = {"ragged": (RAGGED, None), "deep": (DEEP, None), "large": (LARGE, LARGE_CHECK)}

_MB, _WN = "mbexwn_config:", "mbexwn_config:pp_mod_subnet:"


def _blocks(ups, factors, pulse_channels, lin, C, L, **extra):
    over = {_MB + "pp_mod_subnet_upsampling_factors": ups, _MB + "pp_mod_subnet_channel_factors": factors,
            _WN + "cond_lin_upsampling": lin, _WN + "n_channels": C, _WN + "n_layers": L}
    if pulse_channels:
        over[_MB + "pulse_channels"] = pulse_channels
    over.update({(_WN + kk): vv for kk, vv in extra.items()})
    return ("SPEECH", over)


GEOMETRIES = {
    "blocks": GOLDEN_CASES["blocks"][:2],                                        # [2, 1], C = 32 / 16
    "up2": _blocks([2], [1], 10, 10, 32, 2),                                     # one block with up-sampling
    "three": _blocks([2, 2, 1], [1, 0.75, 0.5], 20, 5, 32, 2, pre_cond_layer_channels=[24], activation="gfu"),
    "nocond": _blocks([1, 1], [1, 2], None, 20, 16, 2, disable_conditioning=True),
    "c64": _blocks([2, 1], [1, 0.5], 10, 5, 64, 3),                              # C = 64 / 32
    "deep6": _blocks([2, 1], [1, 0.5], 10, 5, 64, 6),                            # d = 32: the strided F(4,3) gate
    "lin2": _blocks([2, 1], [1, 0.5], 10, 2, 64, 3),                             # 2 conditioning rows / 256: F(4,3) declines
    "causal": GOLDEN_CASES["causal"][:2],                                        # blocks with causal padding
    "speech": ("SPEECH", {}),                                                    # C = 320
    "voice": ("VOICE", {}),                                                      # C = 340
    "deep12": ("SPEECH", {_WN + "n_layers": 12}),                                # d <= 2048
    "causal1": GOLDEN_CASES["causal1"][:2],
    "pqmf": GOLDEN_CASES["pulsepqmf"][:2],
    "subharm": GOLDEN_CASES["subharm"][:2],                                      # 1 sub-harmonic channel, layer 0 unfolded
    "subharm_fold": ("SPEECH", {_WN + "n_channels": 32, _WN + "n_layers": 3, _MB + "pulse_rate_factor": 5,
                                _MB + "pulse_channels": 3, _MB + "wavetable_config:add_subharm_chans": 1}),
}
F43, DIRECT, NOIMG = {"conv_form": "f43"}, {"conv_form": "direct"}, {"weight_images": False}
# (id, geometry, lengths, engine arguments); the gate kernels each case must run follow from expected_gate_kernels
CASES = [
    ("blocks-f43", "blocks", "ragged", F43),
    ("blocks-noimages", "blocks", "ragged", NOIMG),
    ("up2-f43", "up2", "ragged", F43),
    ("three-precond-gfu", "three", "ragged", F43),
    ("nocond", "nocond", "ragged", F43),
    ("c64-f43", "c64", "ragged", F43),
    ("c64-direct", "c64", "ragged", DIRECT),
    ("deep6-f43", "deep6", "ragged", F43),
    ("lin2-f43", "lin2", "ragged", F43),
    ("causal-blocks", "causal", "ragged", {}),
    ("speech-noimages", "speech", "ragged", NOIMG),
    ("voice-noimages", "voice", "ragged", NOIMG),
    ("deep12-noimages", "deep12", "deep", NOIMG),
    ("causal1-noimages", "causal1", "ragged", NOIMG),
    ("pqmf-direct", "pqmf", "ragged", DIRECT),
    ("subharm-direct", "subharm", "ragged", DIRECT),
    ("subharm-folded", "subharm_fold", "ragged", DIRECT),
    ("large-c64-f43", "c64", "large", F43),
]
# a handle without weight images runs every res/skip layer through conv1d (mbx_kernel_report), and the tail unfused
NOIMG_RESSKIP = {"conv1d"}
MUST_FOLD = {"subharm-folded"}       # the sub-harmonic channels go through the folded layer 0 (wn_gate0.hip)
_MAX_LAYERS = 64                     # MBX_MAX_WN_LAYERS


def expected_gate_kernels(dims, kwargs, fold_start):
    """The gate kernel of every layer (block-major) that csrc/mbx_forward.hip (run_gate_layer) picks.  Several blocks (run_wavenet_blocks): F(4,3)
    (launch_wn_gate_winograd4w, 256-row blocks; d > 16 as d / 16 interleaved sub-sequences) where the form is F(4,3), the
    padding SAME, C % 4 == 0, C >= 25 and a 256-row tile holds at most 56 conditioning rows; the direct form otherwise.  One
    block: these cases pin the direct form or hand over no weight images, so layer 0 is the folded first layer or direct."""
    L = dims.wn_layers
    if not dims.wn_multi:
        assert kwargs.get("conv_form") == "direct" or kwargs.get("weight_images") is False
        return ["folded_start" if fold_start else "direct"] + ["direct"] * (L - 1)
    cu = dims.cond_lin_upsampling
    f43 = (kwargs.get("conv_form") == "f43" and kwargs.get("weight_images", True) and dims.wn_padding == "SAME" and
           dims.wn_kernel_size == 3)
    out = []
    for g in block_geometry(dims):
        fits = f43 and g["C"] % 4 == 0 and (g["C"] + 7) // 8 >= 4
        for ll in range(L):
            d = dims.wn_dilation(ll)
            if fits and d > 16:
                out.append("f43_strided")
            elif fits and (256 + cu - 2) // cu + 2 <= 56:
                out.append("f43")
            else:
                out.append("direct")
    return out[:_MAX_LAYERS]


def block_runner_branches(dims, kwargs):
    """The branches of run_wavenet_blocks a case reaches (empty for a single-block model)."""
    if not dims.wn_multi:
        return set()
    geo = block_geometry(dims)
    images = kwargs.get("weight_images", True)
    kernels = expected_gate_kernels(dims, kwargs, False)
    br = {"start: wn_start_kernel"}
    if len(geo) > 1:
        br.add("start: conv1d")
    if any(kk.startswith("f43") for kk in kernels):
        br.add("gate: F(4,3)")
    if "direct" in kernels:
        br.add("gate: conv1d EPI_GATE")
    if images and any(g["C"] % 4 == 0 for g in geo):
        br.add("res/skip: packed wn_resskip")
    if not images or any(g["C"] % 4 for g in geo):
        br.add("res/skip: conv1d EPI_RESSKIP")
    br.add("last block with up" if geo[-1]["ups"] > 1 else "last block without up")
    if dims.wn_disable_conditioning:
        br.add("zeroed conditioning")
    if dims.wn_pre_cond_channels:
        br.add("pre-conditioning chain")
    return br


ALL_BRANCHES = {"start: wn_start_kernel", "start: conv1d", "gate: F(4,3)", "gate: conv1d EPI_GATE",
                "res/skip: packed wn_resskip", "res/skip: conv1d EPI_RESSKIP", "last block with up", "last block without up",
                "zeroed conditioning", "pre-conditioning chain"}


def _dims(geom):
    voice, over = GEOMETRIES[geom]
    return ModelDims(build_case(voice, over)[0])


def test_gpu_cases_reach_every_block_runner_branch():
    """(CPU) The cases together reach every branch of the block runner, use F(4,3), its strided form and the direct form,
    and every geometry is a valid model."""
    assert len({case[0] for case in CASES}) == len(CASES)
    reached, kernels = set(), set()
    for cid, geom, lkey, kwargs in CASES:
        assert geom in GEOMETRIES and lkey in LENGTHS
        dims = _dims(geom)
        reached |= block_runner_branches(dims, kwargs)
        if dims.wn_multi:
            kernels |= set(expected_gate_kernels(dims, kwargs, False))
    assert reached == ALL_BRANCHES, sorted(ALL_BRANCHES - reached)
    assert kernels == {"f43", "f43_strided", "direct"}
    # the rows of every block straddle the 128- and 256-row tiles, and a 1-frame item sits next to long ones
    for geom in {case[1] for case in CASES if case[2] == "ragged"}:
        for g in block_geometry(_dims(geom)):
            rows = [ll * g["spf"] for ll in RAGGED]
            for tile in (128, 256):
                assert any(rr < tile for rr in rows) and any(tile < rr < 2 * tile for rr in rows), (geom, g, tile)
    assert 1 in RAGGED and 1 in DEEP
    assert sum(LARGE) * block_geometry(_dims("c64"))[0]["spf"] >= 12288


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    if not _torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return _torch


def _run(torch, geom, lengths, kwargs, seed=907, fill=None):
    """One forward of the ragged batch; returns (engine, dims, mel, noise, audio)."""
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    voice, over = GEOMETRIES[geom]
    cfg, raw, wt = build_case(voice, over)
    dims = ModelDims(cfg)
    rpf = dims.wn_in_rows_per_frame
    mel, noise = synthetic_inputs(seed, len(lengths), max(lengths), steps_per_frame=rpf)
    if fill is not None:
        for ii, ll in enumerate(lengths):
            mel[ii, ll:] = fill
            noise[ii, ll * rpf:] = fill
    eng = MBExWNEngine(cfg, raw, wt, **kwargs)
    nf = torch.as_tensor(lengths, dtype=torch.int32).cuda()
    audio = eng.forward(torch.as_tensor(mel).cuda(), n_frames=nf, noise=torch.as_tensor(noise).cuda()).cpu().numpy()
    return eng, (cfg, raw, wt), dims, mel, noise, audio


def _stage_names(eng, dims):
    names = list(stage_layout(dims))
    if not dims.wn_multi and eng.conv_form_info()["fold_skip"]:
        names.remove("wn_skip")             # folded into the end convolution: no skip tensor
    return names


@pytest.mark.gpu
@pytest.mark.parametrize("cid,geom,lkey,kwargs", CASES, ids=[case[0] for case in CASES])
def test_wavenet_block_stages_match_the_oracle(torch, cid, geom, lkey, kwargs):
    lengths, items = LENGTHS[lkey]
    items = list(range(len(lengths))) if items is None else items
    eng, (cfg, raw, wt), dims, mel, noise, audio = _run(torch, geom, lengths, kwargs)
    B = len(lengths)
    info = eng.conv_form_info()
    ran = info["gate_kernels"]
    expected = expected_gate_kernels(dims, kwargs, info["fold_start"])
    assert ran == expected, f"{cid}: gate kernels {ran}, expected {expected}"
    if cid in MUST_FOLD:
        assert info["fold_start"], f"{cid}: layer 0 not folded"
    if kwargs == NOIMG:
        assert len(info["resskip_kernels"]) == len(ran) and set(info["resskip_kernels"]) == NOIMG_RESSKIP, \
            f"{cid}: res/skip kernels {info['resskip_kernels']}"
        assert (info["tail_kernel"], info["tail_folded"]) == ("unfused", False), f"{cid}: tail kernel {info['tail_kernel']}"
    if dims.wn_multi:
        # the block runner: the packed kernel where the block has its image and C % 4 == 0, conv1d otherwise; generic tail
        # (launch_wn_resskip: 128-row blocks from 3 x 768 of them up, counted as row tiles x items x 128-column tiles of the
        # layer's 2 C output columns, C for the last layer)
        want = []
        for g in block_geometry(dims):
            for ll in range(dims.wn_layers):
                cout = g["C"] * (1 if ll == dims.wn_layers - 1 else 2)
                blocks = (max(lengths) * g["spf"] + 127) // 128 * B * ((cout + 127) // 128)
                packed = "packed64" if blocks < 3 * 768 else "packed128"
                want.append(packed if kwargs.get("weight_images", True) and g["C"] % 4 == 0 else "conv1d")
        assert info["resskip_kernels"] == want[:_MAX_LAYERS], f"{cid}: res/skip kernels {info['resskip_kernels']}, expected {want}"
        assert info["tail_kernel"] == "unfused", f"{cid}: tail kernel {info['tail_kernel']}"
    layout = stage_layout(dims)
    names = _stage_names(eng, dims)
    got = engine_stages(eng, layout, names, B, items)
    pulse = eng.stage("pulse").cpu().numpy()
    pulse_ana = eng.stage("pulse_ana").cpu().numpy() if dims.pulse_pqmf else None
    eng.close()
    for ii, ll in enumerate(lengths):
        assert np.all(np.isfinite(audio[ii, :ll * 300])) and np.all(audio[ii, ll * 300:] == 0.0), f"{cid}: audio of item {ii}"
    om64, om32 = oracle_models(cfg, raw, wt)
    ref = BlocksReference(om64, om32, dims, pulse, noise, mel, lengths, items=items, pulse_ana=pulse_ana)
    rep = ref.compare(got, names=names)
    record = {"kernels": sorted(set(ran)), "n_gate_layers": len(ran), "resskip_kernels": sorted(set(info["resskip_kernels"])),
              "tail_kernel": info["tail_kernel"],
              **{kk: {"err": vv["err"], "tol": vv["tol"], "ratio": vv["err"] / vv["tol"], "port_err": vv["port_err"],
                      "ref_max": vv["ref_max"]} for kk, vv in rep.items()}}
    print(f"\nwavenet blocks {cid}: {summary(rep)}  kernels {sorted(set(ran))}")
    print("wavenet blocks record " + json.dumps({cid: record}))       # with -s: one JSON line per case
    assert_matches(rep)


@pytest.mark.gpu
def test_multi_block_wn_hidden_is_the_last_blocks(torch):
    """On a handle with several blocks, "wn_hidden" / "wn_skip" have the last block's rows and channels, "cond1" those of
    block 1, the gate kernels list blocks x layers entries, and the hidden state matches the oracle."""
    lengths = [9, 4]
    eng, (cfg, raw, wt), dims, mel, noise, _ = _run(torch, "c64", lengths, F43, seed=5)
    geo = block_geometry(dims)
    T = max(lengths)
    assert tuple(eng.stage("wn_hidden").shape) == (2, T * geo[-1]["spf"] * geo[-1]["C"])
    assert tuple(eng.stage("wn_skip").shape) == (2, T * geo[-1]["spf"] * geo[-1]["C"])
    assert tuple(eng.stage("cond1").shape) == (2, T * geo[1]["ccu"] * 2 * geo[1]["C"])
    with pytest.raises(ValueError):
        eng.stage("cond2")
    assert len(eng.conv_form_info()["gate_kernels"]) == len(geo) * dims.wn_layers
    layout = stage_layout(dims)
    got = engine_stages(eng, layout, ["wn_hidden"], 2, [0, 1])
    pulse = eng.stage("pulse").cpu().numpy()
    eng.close()
    om64, om32 = oracle_models(cfg, raw, wt)
    rep = BlocksReference(om64, om32, dims, pulse, noise, mel, lengths).compare(got, names=["wn_hidden"])
    print(f"\nwn_hidden of the last block: {summary(rep)}")
    assert_matches(rep)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,geom,kwargs", [("three-f43", "three", F43), ("pqmf-direct", "pqmf", DIRECT),
                                             ("blocks-noimages", "blocks", NOIMG)])
def test_padding_frames_are_never_read(torch, cid, geom, kwargs):
    """The same ragged batch three times, its padding frames of mel and noise at 0, 1e30 and NaN: the audio and every stage
    of the items' valid rows are bit-identical across the three, and the audio behind each item's end is exactly 0."""
    lengths = RAGGED
    B = len(lengths)
    runs = {}
    for fill in (0.0, 1e30, np.nan):
        eng, _, dims, _, _, audio = _run(torch, geom, lengths, kwargs, seed=911, fill=fill)
        layout = stage_layout(dims)
        names = _stage_names(eng, dims)
        st = engine_stages(eng, layout, names, B, range(B))
        st["pulse"] = {ii: row.reshape(-1, 1) for ii, row in enumerate(eng.stage("pulse").cpu().numpy().astype(np.float64))}
        layout = dict(layout, pulse=(0, dims.pulse_per_frame * (1 + dims.wt_subharm), 1))
        eng.close()
        runs[fill] = (audio, st)
    base_audio, base_st = runs[0.0]
    for fill in (1e30, np.nan):
        audio, st = runs[fill]
        for ii, ll in enumerate(lengths):
            assert np.array_equal(audio[ii, :ll * 300], base_audio[ii, :ll * 300]), f"{cid}: audio of item {ii}, padding {fill}"
            assert np.all(audio[ii, ll * 300:] == 0.0), f"{cid}: audio behind item {ii}'s end, padding {fill}"
            for name in st:
                n = ll * layout[name][1]
                a, b = st[name][ii][:n], base_st[name][ii][:n]
                bad = np.argwhere(a != b)
                assert bad.size == 0, f"{cid}: {name} of item {ii} ({ll} frames) differs with padding {fill}: first at row " \
                                      f"{bad[0][0]} channel {bad[0][1]}"
    for ii, ll in enumerate(lengths):
        assert np.all(np.isfinite(base_audio[ii, :ll * 300]))

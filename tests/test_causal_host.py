"""force_causal on the host: the sub-net pads of subnet.build_subnet against the pads the reference builds
(tests/golden/make_reference_causal.py records them), and ModelDims forcing the WaveNet's CAUSAL padding."""
import os

import numpy as np
import pytest

from helpers import build_case, load_golden
from mbexwn_vocoder_amd.config import ModelDims, canonical_config
from mbexwn_vocoder_amd.subnet import PAD_ZERO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_causal_f32.npz")

_SMALL = {"mbexwn_config:force_causal": True, "mbexwn_config:pp_mod_subnet:n_channels": 32,
          "mbexwn_config:pp_mod_subnet:n_layers": 3}
# the cases of tests/golden/make_reference_causal.py
CAUSAL_CASES = {
    "causal_canon": ("SPEECH", dict(_SMALL), 2, 23),
    "causal_grammar": ("SPEECH", dict(_SMALL, **{"mbexwn_config:pp_subnet": [[5, 32, 2], [3, 64, "L2"], ["L", 5]]}), 2, 23),
    "causal_valid": ("SPEECH", dict(_SMALL, **{"mbexwn_config:pp_subnet_use_valid_padding": True,
                                                "mbexwn_config:ps_subnet_use_valid_padding": True}), 2, 23),
}


def reference_conv_pads(table):
    """(front, back, type) per convolution of a recorded reference sub-net: the TFPad1d in front of a VALID convolution
    gives its pads and type, a convolution that pads itself (Keras SAME / CAUSAL) zero pads."""
    out, pending = [], None
    for kind, front, back, typ in table.tolist():
        if kind == 0:
            pending = (front, back, typ)
            continue
        if pending is not None:
            assert typ == 0, "a TFPad1d in front of a convolution that pads itself"
            out.append(pending)
        else:
            out.append((front, back, PAD_ZERO))
        pending = None
    assert pending is None
    return out


def engine_subnets(cfg):
    from mbexwn_vocoder_amd.engine import subnet_ops
    f0_ops, vtf_ops = subnet_ops(cfg)
    return {"pp": f0_ops, "ps": vtf_ops}


@pytest.mark.parametrize("case", sorted(CAUSAL_CASES))
def test_build_subnet_pads_equal_the_reference(case):
    """Every convolution of both sub-nets pads as the reference's force_causal model does (custom_pulsed_generator.py:53,
    74-138): (front, back) always, the padding type wherever a pad exists."""
    gold = load_golden(GOLDEN)
    voice, over, _, _ = CAUSAL_CASES[case]
    cfg = canonical_config(voice, **over)
    ops = engine_subnets(cfg)
    for sub in ("pp", "ps"):
        ref = reference_conv_pads(gold[f"{case}/pads/{sub}"])
        got = [(op["pad_l"], op["pad_r"], op["pad_mode"]) for op in ops[sub] if op["kind"] == "conv"]
        assert len(got) == len(ref), f"{case} {sub}: {len(got)} convolutions against the reference's {len(ref)}"
        for ii, (gg, rr) in enumerate(zip(got, ref)):
            assert gg[:2] == rr[:2], f"{case} {sub} layer {ii}: pads {gg[:2]}, reference {rr[:2]}"
            if rr[0] + rr[1] > 0:
                assert gg[2] == rr[2], f"{case} {sub} layer {ii}: pad type {gg[2]}, reference {rr[2]}"
            assert gg[1] == 0, f"{case} {sub} layer {ii}: a causal layer pads behind"


def test_causal_golden_cases_cover_every_pad_branch():
    """The three recorded cases hold a SYMMETRIC and an EDGE TFPad1d, a Keras-CAUSAL sub-pixel layer and a VALID layer."""
    gold = load_golden(GOLDEN)
    tabs = np.concatenate([gold[f"{case}/pads/{sub}"] for case in CAUSAL_CASES for sub in ("pp", "ps")])
    assert {(0, 1), (0, 2)} <= {(int(kk), int(tt)) for kk, _, _, tt in tabs}
    assert any(kk == 1 and tt == 2 and ff > 0 for kk, ff, _, tt in tabs)          # Keras CAUSAL, ks > 1
    assert any(kk == 1 and tt == 0 for kk, _, _, tt in tabs)                      # VALID behind a pad


def test_model_dims_force_causal_pads_the_wavenet_causally():
    """force_causal makes the WaveNet CAUSAL whatever pp_mod_subnet.padding says (reference :474-475)."""
    assert ModelDims(canonical_config("SPEECH")).wn_padding == "SAME"
    assert ModelDims(canonical_config("SPEECH", **{"mbexwn_config:force_causal": True})).wn_padding == "CAUSAL"
    over = {"mbexwn_config:force_causal": True, "mbexwn_config:pp_mod_subnet:padding": "SAME"}
    assert ModelDims(canonical_config("SPEECH", **over)).wn_padding == "CAUSAL"
    assert ModelDims(canonical_config("SPEECH", **{"mbexwn_config:force_causal": False})).wn_padding == "SAME"


def test_engine_tensor_table_of_a_causal_model_has_the_winograd_images():
    """A single-block force_causal model gets the F(2,3) / F(4,3) images and the folded start weights that the pinned
    causal forms run on (they do not depend on the padding)."""
    from mbexwn_vocoder_amd.packing import tensor_table
    cfg, raw, wt = build_case(*CAUSAL_CASES["causal_canon"][:2])
    tab = tensor_table(cfg, raw, wt)
    for ll in range(3):
        assert f"wn.conv1D_{ll}.wino2w" in tab and f"wn.conv1D_{ll}.wino4w" in tab
    assert "wn.conv1D_0.start_fold" in tab


class _HostEngine:
    """The engine surface StreamingSynthesizer reads at construction (configuration, no device work)."""

    def __init__(self, cfg):
        import torch
        self.config, self.dims, self.device = cfg, ModelDims(cfg), torch.device("cpu")

    def layer_state_info(self):
        return 0, 0, 0

    def conv_form_info(self):
        return {"split_f16_layers": 0, "split_f16_gate_layers": 0}


_WN = "mbexwn_config:pp_mod_subnet:"
STREAM_SMALL = {_WN + "n_channels": 32, _WN + "n_layers": 5}       # the streaming model of test_gpu_streaming.py


def test_causal_stream_margins_match_the_docstring_table():
    """streaming.stream_margins of the SMALL model: SAME (10, 11, 4), force_causal (15, 7, 7) = 87.5 ms of look-ahead, CAUSAL
    WaveNet padding only (12, 10, 4); the WaveNet reach splits into left / right, the front end and the conditioning chain
    reach to the left only under force_causal."""
    from mbexwn_vocoder_amd.streaming import (StreamingSynthesizer, cond_chain_reach, frontend_reach, stream_margins,
                                              wavenet_reach)
    want = {"same": ({}, (10, 11, 4, 6, 7, 2), (2, 2), (3, 4), (1, 1), 137.5),
            "force_causal": ({"mbexwn_config:force_causal": True}, (15, 7, 7, 8, 6, 1), (4, 1), (6, 1), (2, 0), 87.5),
            "wavenet_causal": ({_WN + "padding": "CAUSAL"}, (12, 10, 4, 8, 6, 1), (4, 1), (3, 4), (2, 0), 125.0)}
    for name, (over, margins, wn, fe, cond, ms) in want.items():
        cfg = canonical_config("SPEECH", **dict(STREAM_SMALL, **over))
        dims = ModelDims(cfg)
        assert stream_margins(dims, cfg) == margins, name
        assert wavenet_reach(dims) == wn and frontend_reach(dims, cfg) == fe and cond_chain_reach(dims) == cond, name
        syn = StreamingSynthesizer(_HostEngine(cfg), chunk_frames=8)
        assert abs(syn.lookahead_ms - ms) < 1e-9 and syn.wn_left == wn[0] and syn.wn_reach == wn[1], name
        # the stages behind the WaveNet (PQMF 1 frame, STFT 3 / 4 frames) reach 4 / 5 frames around the emitted ones; under
        # CAUSAL padding the carried rows start align - 1 + 4 - 5 = 6 frames in front (align = 8 frames: d = 16)
        assert (syn.sr_left, syn.sr_right) == ((4 if name == "same" else 6), 5), name
    assert want["force_causal"][1][1] < want["same"][1][1]

"""The multi-block WaveNet stage comparator (tests/wn_blocks_reference.py) sees what it claims to see, on the CPU: it accepts
the float32 port of the graph and rejects planted defects of the kind the block runner's launches can make -- block 1's
conditioning read a row late at an item's end, a partial channel tile of the last block rounded to fp16, the up-sampling
convolution reading the next item's first row at an item's end, a PQMF-analysis tap lost at an item's edge.  Each defect
is shown, in the same test, to move the audio by less than the end-to-end bar 1e-4 * max(1, |audio|).

Two ragged items of 13 and 26 frames.  "two": blocks [2, 1] with C = 32 / 24 (10 and 20 rows per frame: 130 / 260 and
260 / 520 rows, across the 128- and 256-row tiles at both rates); "three": blocks [2, 2, 1], C = 32 / 24 / 16, a
pre-conditioning layer and the gfu gate; "pqmf": the pulse-PQMF model of the golden case "pulsepqmf"."""
import numpy as np
import pytest

from helpers import GOLDEN_CASES, build_case
from mbexwn_vocoder_amd.config import ModelDims
from oracle import mbexwn_oracle as orc
from wn_blocks_reference import F_FLOOR, K_PORT, BlocksReference, failures, oracle_models, summary

_MB, _WN = "mbexwn_config:", "mbexwn_config:pp_mod_subnet:"
GEOMETRIES = {
    "two": ("SPEECH", {_MB + "pp_mod_subnet_upsampling_factors": [2, 1], _MB + "pp_mod_subnet_channel_factors": [1, 0.75],
                       _MB + "pulse_channels": 10, _WN + "cond_lin_upsampling": 5, _WN + "n_channels": 32, _WN + "n_layers": 3}),
    "three": ("SPEECH", {_MB + "pp_mod_subnet_upsampling_factors": [2, 2, 1],
                         _MB + "pp_mod_subnet_channel_factors": [1, 0.75, 0.5], _MB + "pulse_channels": 20,
                         _WN + "cond_lin_upsampling": 5, _WN + "n_channels": 32, _WN + "n_layers": 2,
                         _WN + "pre_cond_layer_channels": [24], _WN + "activation": "gfu"}),
    "pqmf": GOLDEN_CASES["pulsepqmf"][:2],
}
LENGTHS = [13, 26]
_CASES = {}


def case(name):
    """(cfg, raw, wt, dims, mel, noise, BlocksReference) of a geometry, built once."""
    if name not in _CASES:
        voice, over = GEOMETRIES[name]
        cfg, raw, wt = build_case(voice, over)
        dims = ModelDims(cfg)
        om64, om32 = oracle_models(cfg, raw, wt)
        rng = np.random.default_rng(31)
        T = max(LENGTHS)
        mel = orc.synthetic_mel(rng, len(LENGTHS), T)
        noise = rng.normal(size=(len(LENGTHS), T * dims.wn_in_rows_per_frame)).astype(np.float32)
        # the oracle's own oscillator output, as the engine's "pulse" stage holds it (float32)
        pulse = om64.wavetable(om64.generate_f0(mel.astype(np.float64))).astype(np.float32)
        _CASES[name] = (cfg, raw, wt, dims, mel, noise, BlocksReference(om64, om32, dims, pulse, noise, mel, LENGTHS))
    return _CASES[name]


def _fresh(name, dtype):
    cfg, raw, wt = case(name)[:3]
    return orc.OracleModel(cfg, raw, wt, dtype=dtype)


def _with_hook(om, hook):
    """om with hook(block, layer, hidden) planted into every forward (the audio path included)."""
    clean = om.wavenet_blocks
    om.wavenet_blocks = lambda x, mel, hook=None, return_blocks=False, _planted=hook: clean(x, mel, hook=_planted,
                                                                                             return_blocks=return_blocks)
    return om


def _audio_moved(name, plant):
    """max over the items of |audio(planted float64 oracle) - audio(float64 oracle)| and the end-to-end bar
    1e-4 * max(1, |audio|); plant(model, item) -> the model with the defect."""
    _, _, _, dims, mel, noise, ref = case(name)
    moved, bar = 0.0, 0.0
    for ii, ll in enumerate(LENGTHS):
        m, nz = mel[ii:ii + 1, :ll].astype(np.float64), noise[ii:ii + 1, :ll * dims.wn_in_rows_per_frame]
        clean = ref.om64.forward(m, nz)
        bad = plant(_fresh(name, np.float64), ii).forward(m, nz)
        moved = max(moved, float(np.abs(bad - clean).max()))
        bar = max(bar, 1e-4 * max(1.0, float(np.abs(clean).max())))
    return moved, bar


def _rejected(name, label, plant):
    """Plants the defect into the float32 port (every item) and the float64 oracle's audio path: the comparator must reject
    it while the audio stays inside the end-to-end bar.  Returns the comparator's report and its failure text."""
    ref = case(name)[-1]
    got = ref.port_result(models={ii: plant(_fresh(name, np.float32), ii) for ii in ref.items})
    rep = ref.compare(got, names=list(got))
    moved, bar = _audio_moved(name, plant)
    msg = failures(rep)
    print(f"\n{name}: defect {label}: audio moved {moved:.2e} (end-to-end bar 1e-4*max(1,|audio|) = {bar:.2e}); comparator: "
          f"{summary(rep)}\n{msg}")
    assert msg, f"{label}: the comparator accepted a planted defect"
    assert moved < bar, f"{label}: the audio bar sees this defect already ({moved:.2e} >= {bar:.2e})"
    return rep, msg


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_accepts_the_float32_port(name):
    ref = case(name)[-1]
    got = ref.port_result()
    rep = ref.compare(got, names=list(got))
    print(f"\n{name}: float32 port {summary(rep)}")
    assert not failures(rep), failures(rep)
    assert set(rep) >= {"cond", "wn_hidden", "wn_skip", "wn_out"} and ("pulse_ana" in rep) == (name == "pqmf")
    assert sum(kk.startswith("cond") for kk in rep) == len(ModelDims(case(name)[0]).wn_block_ups)
    # the bar is set by float32 rounding, not by the floor alone: the port's own error is of float32's order
    for rr in rep.values():
        assert 0.0 < rr["port_err"] <= 1e-5 * max(1.0, rr["ref_max"])
        assert rr["tol"] <= max(K_PORT * rr["port_err"], F_FLOOR * max(1.0, rr["ref_max"])) * (1 + 1e-12)


def test_rejects_late_conditioning_of_block1_at_an_items_end():
    """(a) Block 1's last conditioning row of every item moved 1e-4 of the way towards the row in front of it (a one-row-late
    read at an item's end; at full weight the audio moves by ~30x its bar, at 1e-4 it stays inside)."""
    def plant(om, ii):
        clean = om.conditioning_rows

        def rows(mel, prefix="wn.", rate_factor=1):
            cc = np.array(clean(mel, prefix, rate_factor))
            if prefix == "wn1.":
                cc[:, -1] += cc.dtype.type(1e-4) * (cc[:, -2] - cc[:, -1])
            return cc
        om.conditioning_rows = rows
        return om
    rep, msg = _rejected("two", "(a) block 1's last conditioning row 1e-4 of a row late", plant)
    w = rep["cond1"]["where"]
    assert not rep["cond1"]["ok"] and (w["block"], w["rows_to_end"]) == (1, 1), msg
    assert rep["cond"]["ok"], msg


def test_rejects_fp16_channels_of_the_24_channel_block():
    """(b) The last 8 channels of the 24-channel (last) block rounded to fp16 after its layer 0 (a kernel dropping the low
    half of a partial channel tile)."""
    def hook(bb, ll, h):
        if bb == 1 and ll == 0:
            h = h.copy()
            h[..., 16:24] = h[..., 16:24].astype(np.float16).astype(h.dtype)
        return h
    rep, msg = _rejected("two", "(b) channels 16..23 of block 1 in fp16 after layer 0", lambda om, ii: _with_hook(om, hook))
    w = rep["wn_hidden"]["where"]
    assert not rep["wn_hidden"]["ok"] and w["block"] == 1 and 16 <= w["channel"] < 24, msg


def _first_up0_row(name, ii):
    """The first input row of item ii's up0 convolution (block 0's output), float64."""
    ref = case(name)[-1]
    om = _fresh(name, np.float64)
    clean, seen = om.up_conv, {}

    def up(block, y, factor):
        if block == 0:
            seen["row"] = np.array(y[:, :1])
        return clean(block, y, factor)
    om.up_conv = up
    om.wavenet_blocks(ref.wavenet_input(ii), ref.mels[ii].astype(np.float64))
    return seen["row"]


def test_rejects_up0_reading_the_next_items_first_row():
    """(c) At the end of item 0 the up0 convolution reads 1 % of item 1's first row where its zero padding belongs (a ragged
    batch whose up-sampling launch does not stop at the item's own length; the whole row moves the audio by ~13x its bar)."""
    nxt = _first_up0_row("two", 1)

    def plant(om, ii):
        if ii != 0:
            return om
        clean = om.up_conv

        def up(block, y, factor):
            if block != 0:
                return clean(block, y, factor)
            ext = np.concatenate((y, (1e-2 * nxt).astype(y.dtype)), axis=1)
            return clean(block, ext, factor)[:, :y.shape[1] * factor]
        om.up_conv = up
        return om
    rep, msg = _rejected("two", "(c) up0 at item 0's end reads 1 % of item 1's first row", plant)
    w = rep["wn_hidden"]["where"]
    assert not rep["wn_hidden"]["ok"] and w["item"] == 0 and w["rows_to_end"] <= 16, msg


def test_rejects_a_dropped_analysis_tap_at_an_items_edge():
    """(d) The PQMF analysis of the pulse loses its outermost tap in the first row of every item (the tap that reaches
    furthest into the item from its start)."""
    def plant(om, ii):
        clean = om.pulse_analysis

        def ana(pulse):
            x = np.array(clean(pulse))
            pq = om.mb["pulse_channels_multi_band_config"]
            bank = orc.pqmf_analysis_bank(pq["subbands"], pq["taps"], pq["cutoff_ratio"], pq["beta"]).astype(om.dtype)
            taps = bank.shape[0] - 1
            x[:, 0, :] -= bank[taps][None, :] * np.asarray(pulse).astype(om.dtype)[:, taps // 2, None]
            return x
        om.pulse_analysis = ana
        return om
    rep, msg = _rejected("pqmf", "(d) outermost analysis tap of row 0 dropped", plant)
    w = rep["pulse_ana"]["where"]
    assert not rep["pulse_ana"]["ok"] and w["row"] == 0, msg

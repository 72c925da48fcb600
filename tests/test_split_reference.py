"""The split-half-precision WaveNet path as designed, on the CPU (tests/split_reference.py): the arithmetic of
csrc/wn_gate_f16.hip and csrc/wn_resskip_f16.hip -- fp16 hi / lo' operands taken from the packers' own images, main and cross
accumulators, the 2^11-scaled res/skip accumulator, the hidden state carried as fp16 planes -- emulated in numpy inside the
float32 port of the graph.

(a) The design holds the stage bar of tests/wn_reference.py (K = 8, F = 5e-7, unchanged) on its own: the two ragged items of
    test_wn_reference.py at the 3-layer channel counts where the kernels' tiles are ragged and on SPEECH (5 layers).  What a
    GPU stage case of test_gpu_wavenet_stages.py shows beyond these figures is the kernel, not the mode.
(b) Planted defects of the kind only this path can have, (i) .. (n) behind the defects (a) .. (h) of test_wn_reference.py, each
    at the smallest geometry that has the edge: every one breaks the bar at the named place, and (m) -- values in the plane
    padding -- changes nothing, which holds the packer to zero weights behind C."""
import numpy as np
import pytest

from helpers import build_case
from mbexwn_vocoder_amd import packing
from oracle import mbexwn_oracle as orc
from split_reference import SplitEmulation, unpack_gate_f16, unpack_resskip_f16
from test_wn_reference import LENGTHS, N_OUT, _cpu_excitation, _rs_case
from wn_reference import F_FLOOR, K_PORT, WaveNetReference, failures, oracle_models, wavenet_inputs

_WN = "mbexwn_config:pp_mod_subnet:"
_CASES = {}


def _case(C):
    """(reference, (cfg, raw, wt)) of the 3-layer model with C channels, or of SPEECH (5 layers, C = 320) for C = "speech"."""
    if C not in _CASES:
        if C == "speech":
            model = build_case("SPEECH", {})
            om64, om32 = oracle_models(*model)
            rng = np.random.default_rng(31)
            T = max(LENGTHS)
            mel = orc.synthetic_mel(rng, len(LENGTHS), T)
            noise = rng.normal(size=(len(LENGTHS), T * 20)).astype(np.float32)
            pulse = _cpu_excitation(om64, mel).astype(np.float32)
            ref = WaveNetReference(om64, om32, wavenet_inputs(om64, pulse, noise, LENGTHS, 20), mel, LENGTHS, 20)
        else:
            model = build_case("SPEECH", {_WN + "n_channels": C, _WN + "n_layers": 3})
            ref = _rs_case(C)[0]
        _CASES[C] = (ref, model)
    return _CASES[C]


def _emulate(C, defects=None):
    ref, model = _case(C)
    return ref, SplitEmulation(*model, defects=defects).result(ref)


def test_unpacked_images_are_the_split_weights():
    """The unpackers of split_reference.py invert the packers: hi = fp16(w) and lo' = fp16((w - hi) 2^11) element for element,
    zero outside the matrix (K = 340 + 16 rows: a partial last step; 370 and 2 x 68 columns: partial last pair and tile)."""
    rng = np.random.default_rng(5)
    w = (rng.normal(size=(1, 356, 370)) * 0.07).astype(np.float32)
    hi, lo = unpack_resskip_f16(packing.pack_resskip_f16_weights(w))
    assert hi.shape == lo.shape == (384, 384)
    want = np.zeros((384, 384), dtype=np.float32)
    want[:356, :370] = w[0]
    assert np.array_equal(hi, want.astype(np.float16))
    assert np.array_equal(lo, ((want - want.astype(np.float16).astype(np.float32)) * np.float32(2048)).astype(np.float16))
    C = 68
    wg = (rng.normal(size=(3, C, 2 * C)) * 0.05).astype(np.float32)
    g = unpack_gate_f16(packing.pack_gate_f16_weights(wg))
    assert g.shape == (2, 3, 96, 2, 3, 32)
    want = np.zeros((3, 96, 2, 96), dtype=np.float32)
    want[:, :C, 0, :C], want[:, :C, 1, :C] = wg[:, :, :C], wg[:, :, C:]
    assert np.array_equal(g[0].reshape(3, 96, 2, 96), want.astype(np.float16))
    assert np.array_equal(g[1].reshape(3, 96, 2, 96),
                          ((want - want.astype(np.float16).astype(np.float32)) * np.float32(2048)).astype(np.float16))


@pytest.mark.parametrize("C", [68, 292, 324, 340, 352, "speech"])
def test_the_split_design_holds_the_stage_bar(C):
    """(a) The emulated split path against the float64 oracle at the stage bar, K = 8 and F = 5e-7 as everywhere."""
    ref, got = _emulate(C)
    rep = ref.compare(got, k=K_PORT, f=F_FLOOR)
    print(f"\nsplit emulation C = {C}: " + "  ".join(f"{kk} {rr['err']:.2e}/{rr['tol']:.2e} = {rr['err'] / rr['tol']:.2f}"
                                                    for kk, rr in rep.items()))
    assert not failures(rep), failures(rep)
    # ... and it is not the float32 port again: the hidden state went through the planes
    clean = ref.port_result()
    assert any(not np.array_equal(got["wn_hidden"][ii, :ref.rows(ii)], clean["wn_hidden"][ii, :ref.rows(ii)]) for ii in ref.items)


def _defect(C, label, defects):
    ref, got = _emulate(C, defects)
    rep = ref.compare(got)
    print(f"\nC{C}: defect {label}: " + "  ".join(f"{kk} {rr['err']:.2e}/{rr['tol']:.2e}" for kk, rr in rep.items()))
    msg = failures(rep)
    assert msg, f"{label}: the comparator accepted a planted defect"
    return rep, msg


def test_rejects_a_lost_low_half_in_the_partial_k_step():
    """(i) C = 340: layer 1's res/skip contraction loses lo' of its activation in the last, partial K step (channels 320 .. 339):
    every output column of the layer is off, the hidden state first."""
    rep, msg = _defect(340, "(i) layer 1 res/skip without lo' of channels 320 .. 339", {"rs_act_lo_lost": (1, 320, 340)})
    assert not rep["wn_hidden"]["ok"] and not rep["wn_out"]["ok"], msg


def test_rejects_a_zero_low_weight_image_of_the_last_pair():
    """(j) C = 324: the lo' weight image of the last column pair (pair 11: columns 352, 353 of 354, the last two skip columns)
    is zero: "wn_out" is off in its columns 28 and 29 and nowhere else."""
    C = 324
    assert (C + N_OUT + 31) // 32 == 12 and C + N_OUT - 32 * 11 == 2
    rep, msg = _defect(C, "(j) lo' weights of column pair 11 zero", {"rs_w_lo_zero_pair": 11})
    assert not rep["wn_out"]["ok"] and rep["wn_hidden"]["ok"], msg
    assert rep["wn_out"]["where"]["channel"] in (28, 29), msg


def test_rejects_a_cross_accumulator_at_twice_its_weight():
    """(k) The gate's cross accumulator enters with 2^-10 instead of 2^-11 in one column tile (C = 68: tile 1 of 3, layer 1)."""
    rep, msg = _defect(68, "(k) cross accumulator of gate tile 1 times 2^-10", {"gate_cross_scale": (1, 1, 2.0 ** -10)})
    assert not rep["wn_hidden"]["ok"] and not rep["wn_out"]["ok"], msg


def test_rejects_the_last_gate_tile_on_its_neighbours_weights():
    """(l) C = 324, 11 column tiles, the last of 4 channels: it takes the weight images of tile 9 -- the wrong side of the wide
    kernel's min(ct, n_ct - 1) clamp."""
    C = 324
    n_ct = (C + 31) // 32
    assert n_ct == 11 and C - 32 * (n_ct - 1) == 4
    rep, msg = _defect(C, "(l) gate tile 10 with the weights of tile 9", {"gate_last_tile_from": n_ct - 2})
    assert not rep["wn_hidden"]["ok"] and not rep["wn_out"]["ok"], msg


def test_plane_padding_is_never_multiplied_into_a_result():
    """(m) C = 324: the plane columns 324 .. 327 hold 1.0 instead of 0.  The gate reads them (8-channel chunks that start below
    C); its weight image must be zero there, so nothing changes, bit for bit."""
    ref, got = _emulate(324, {"plane_padding": 1.0})
    _, clean = _emulate(324)
    for name in ("wn_out", "wn_hidden"):
        assert np.array_equal(got[name], clean[name], equal_nan=True), name
    assert not failures(ref.compare(got))
    g = unpack_gate_f16(packing.tensor_table(*_case(324)[1], split_f16=True)["wn.conv1D_1.gate_f16"])
    assert np.all(g[:, :, 324:] == 0) and np.any(g[:, :, 323] != 0)


def test_rejects_the_last_output_columns_shifted_by_the_clamp():
    """(n) C = 352, cout = 382, the widest launch: the last two output columns (380, 381: skip columns 28, 29) take the values of
    the columns 378, 379 -- the kernel's min(col, cout - 2) read as a shift."""
    C = 352
    assert C + N_OUT == 382
    rep, msg = _defect(C, "(n) columns 380, 381 from 378, 379", {"rs_last_pair_shifted": True})
    assert not rep["wn_out"]["ok"] and rep["wn_hidden"]["ok"], msg
    assert rep["wn_out"]["where"]["channel"] in (28, 29), msg

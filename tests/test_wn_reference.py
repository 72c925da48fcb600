"""The WaveNet stage comparator (tests/wn_reference.py) sees what it claims to see, on the CPU: it accepts the float32 port of
the graph and rejects each planted defect of the kind Winograd transforms, LDS staging and ragged-batch tile decoding produce
-- a lost low half of one channel tile, a row at a 256-row tile seam, the conditioning of one row read from its neighbour, one
item leaking into the next.  Two ragged items of 13 and 26 frames (260 / 520 rows: both cross the 256-row seam), SPEECH
(5 layers, C = 320) and the 12-layer model with dilations up to 2048.

The second half plants what the residual/skip and tail kernels can get wrong at the channel counts of
test_gpu_wavenet_stages.py (3 layers; C + n_out one column pair past a multiple of 32, the residual/skip seam inside a pair, a
last 16-channel block of 4 channels): a lost last column pair, two residual columns filled from the skip side of the seam, a
16-row tile written with its neighbour's rows, a tail without its last channel block.  The skip path is planted as the engine
holds it, folded into the end convolution: a layer's skip columns are its n_out-wide share of "wn_out"."""
import numpy as np
import pytest

from helpers import build_case
from oracle import mbexwn_oracle as orc
from wn_reference import F_FLOOR, K_PORT, WaveNetReference, failures, oracle_models, wavenet_inputs

GEOMETRIES = {
    "speech5": ("SPEECH", {}),
    "deep12": ("SPEECH", {"mbexwn_config:pp_mod_subnet:n_layers": 12}),
}
LENGTHS = [13, 26]
TILE = 32


def _cpu_excitation(om, mel):
    """The oracle's own excitation rows (B, T*20, pulse channels) for mel: a realistic WaveNet input on the CPU."""
    f0 = om.generate_f0(mel.astype(np.float64))
    pulse = om.wavetable(f0)
    return pulse.reshape(pulse.shape[0], -1, om.pulse_channels)


@pytest.fixture(scope="module", params=sorted(GEOMETRIES))
def case(request):
    voice, over = GEOMETRIES[request.param]
    cfg, raw, wt = build_case(voice, over)
    om64, om32 = oracle_models(cfg, raw, wt)
    rng = np.random.default_rng(31)
    T = max(LENGTHS)
    mel = orc.synthetic_mel(rng, len(LENGTHS), T)
    noise = rng.normal(size=(len(LENGTHS), T * 20)).astype(np.float32)
    pulse = _cpu_excitation(om64, mel).astype(np.float32)
    xs = wavenet_inputs(om64, pulse, noise, LENGTHS, 20)
    return request.param, WaveNetReference(om64, om32, xs, mel, LENGTHS, 20)


def _old_bar(ref, name="wn_out"):
    return 1e-4 * max(1.0, max(float(np.abs(ref.ref[ii][name]).max()) for ii in ref.items))


def _moved(ref, got, name="wn_out"):
    """How far a planted defect moved a tensor from the clean float32 port (max over the items' valid rows)."""
    clean = ref.port_result()
    return max(float(np.abs(got[name][ii, :ref.rows(ii)] - clean[name][ii, :ref.rows(ii)]).max()) for ii in ref.items)


def test_accepts_the_float32_port(case):
    name, ref = case
    rep = ref.compare(ref.port_result(), names=("wn_out", "wn_hidden", "wn_skip"))
    print(f"\n{name}: float32 port " + "  ".join(f"{kk} {rr['err']:.2e} (|ref| {rr['ref_max']:.3g}, tol {rr['tol']:.2e})"
                                               for kk, rr in rep.items()))
    assert not failures(rep), failures(rep)
    # the bar is set by float32 rounding, not by the floor alone: the port's own error is of float32's order
    for rr in rep.values():
        assert 0.0 < rr["port_err"] <= 1e-5 * max(1.0, rr["ref_max"])
        assert rr["tol"] <= max(K_PORT * rr["port_err"], F_FLOOR * max(1.0, rr["ref_max"])) * (1 + 1e-12)


def _fp16_tile(layer, tile):
    def hook(ll, h):
        if ll == layer:
            h = h.copy()
            sl = slice(tile * TILE, (tile + 1) * TILE)
            h[..., sl] = h[..., sl].astype(np.float16).astype(h.dtype)
        return h
    return hook


def _scale_row(layer, row, factor):
    def hook(ll, h):
        if ll == layer:
            h = h.copy()
            h[:, row] *= h.dtype.type(factor)
        return h
    return hook


def _report_defect(name, label, ref, got):
    rep = ref.compare(got)
    moved = _moved(ref, got)
    print(f"\n{name}: defect {label}: wn_out moved {moved:.2e} (the audio-level bar 1e-4*max(1,|ref|) = {_old_bar(ref):.1e}, "
          f"{_old_bar(ref) / moved:.0f}x the defect); comparator: " +
          "  ".join(f"{kk} {rr['err']:.2e}/{rr['tol']:.2e}" for kk, rr in rep.items()))
    msg = failures(rep)
    assert msg, f"{label}: the comparator accepted a planted defect"
    return rep, moved, msg


def test_rejects_fp16_tile_of_h(case):
    """(a) One 32-channel tile of h rounded to fp16 after layer 2 (a split-precision kernel dropping the lo' half of one tile)."""
    name, ref = case
    rep, moved, msg = _report_defect(name, "(a) fp16 tile of h after layer 2", ref, ref.port_result(hook=_fp16_tile(2, 3)))
    assert moved < _old_bar(ref)          # ... which the plain audio-level tolerance lets through
    assert not rep["wn_out"]["ok"], msg   # the output alone already shows it
    assert rep["wn_hidden"]["where"]["channel"] // TILE == 3, msg


def test_rejects_row_at_a_256_row_seam(case):
    """(b) One row at the 256-row tile seam scaled by (1 - 1e-4) after layer 1 (item 1, row 256)."""
    name, ref = case
    rep, moved, msg = _report_defect(name, "(b) row 256 scaled by 1-1e-4 after layer 1", ref,
                                     ref.port_result(hooks={1: _scale_row(1, 256, 1 - 1e-4)}))
    assert moved < _old_bar(ref)
    w = rep["wn_hidden"]["where"]
    assert (w["item"], w["row"], w["row%256"]) == (1, 256, 0), msg


def test_rejects_conditioning_from_the_neighbouring_row(case):
    """(c) The conditioning of one row inside a tile (row 300 of every item's 2C-wide conditioning) taken from row 301."""
    name, ref = case
    bad = orc.OracleModel(ref.om32.cfg, ref.om32.raw, ref.om32.wt, dtype=np.float32)
    clean = bad.conditioning

    def shifted(mel, prefix="wn.", rate_factor=1):
        cc = np.array(clean(mel, prefix, rate_factor))
        if cc.shape[1] > 301:
            cc[:, 300] = cc[:, 301]
        return cc

    bad.conditioning = shifted
    rep, _, msg = _report_defect(name, "(c) conditioning of row 300 from row 301", ref, ref.port_result(model=bad))
    w = rep["wn_hidden"]["where"]
    assert w["item"] == 1 and abs(w["row"] - 300) <= 2 ** 11, msg


def test_rejects_a_leak_between_items(case):
    """(d) Item 1's first row leaking 1e-4 of itself into item 0's last valid row (after layer 1)."""
    name, ref = case
    first = {}

    def record(ll, h):
        if ll == 1:
            first["row"] = np.array(h[:, 0])
        return h

    ref.port_result(hooks={1: record})
    n0 = ref.rows(0)

    def leak(ll, h):
        if ll == 1:
            h = h.copy()
            h[:, n0 - 1] += h.dtype.type(1e-4) * first["row"].astype(h.dtype)
        return h

    rep, _, msg = _report_defect(name, "(d) 1e-4 of item 1's row 0 into item 0's last row", ref, ref.port_result(hooks={0: leak}))
    w = rep["wn_hidden"]["where"]
    assert (w["item"], w["rows_to_end"]) == (0, 1), msg


# ---- what the residual/skip and tail kernels can get wrong ---------------------------------------------------------------
_RS_REFS = {}
N_OUT = 30


def _rs_case(C):
    """The two ragged items on SPEECH with 3 layers and C channels (cached)."""
    if C not in _RS_REFS:
        wn = "mbexwn_config:pp_mod_subnet:"
        cfg, raw, wt = build_case("SPEECH", {wn + "n_channels": C, wn + "n_layers": 3})
        om64, om32 = oracle_models(cfg, raw, wt)
        rng = np.random.default_rng(31)
        T = max(LENGTHS)
        mel = orc.synthetic_mel(rng, len(LENGTHS), T)
        noise = rng.normal(size=(len(LENGTHS), T * 20)).astype(np.float32)
        pulse = _cpu_excitation(om64, mel).astype(np.float32)
        xs = wavenet_inputs(om64, pulse, noise, LENGTHS, 20)
        ref = WaveNetReference(om64, om32, xs, mel, LENGTHS, 20)
        w_end = ref.om32.weight("wn.end")[0]
        w_end = np.asarray(w_end).reshape(-1, np.asarray(w_end).shape[-1])
        assert w_end.shape == (C, N_OUT) and w_end.dtype == np.float32
        _RS_REFS[C] = (ref, w_end)
    return _RS_REFS[C]


@pytest.mark.parametrize("C", [292, 324, 340, 68])
def test_accepts_the_float32_port_at_the_resskip_geometries(C):
    ref, _ = _rs_case(C)
    rep = ref.compare(ref.port_result(), names=("wn_out", "wn_hidden", "wn_skip"))
    assert not failures(rep), failures(rep)


@pytest.mark.parametrize("C", [292, 324])
def test_rejects_a_lost_last_column_pair(C):
    """(e) Layer 1's res/skip launch loses its last column pair, the columns >= 32 (np - 1) of its C + 30: at C = 292 (322
    columns, np = 11) and C = 324 (354, np = 12) that pair holds the last two of the layer's 30 skip columns and nothing else,
    so "wn_out" lacks the layer's share in its columns 28 and 29."""
    ref, w_end = _rs_case(C)
    assert (C + N_OUT) % 32 == 2
    skip1 = {}

    def taps(ii):
        def record(ll, r):
            if ll == 1:
                skip1[ii] = np.array(r[0, :, C:])
            return r
        return {"res_skip": record}

    ref.port_result(taps={ii: taps(ii) for ii in ref.items})
    got = {kk: np.array(vv) for kk, vv in ref.port_result().items()}
    for ii in ref.items:
        got["wn_out"][ii, :ref.rows(ii), 28:30] -= skip1[ii] @ w_end[:, 28:30]
    rep, _, msg = _report_defect(f"C{C}", "(e) layer 1 loses its last column pair", ref, got)
    assert not rep["wn_out"]["ok"] and rep["wn_hidden"]["ok"], msg
    assert rep["wn_out"]["where"]["channel"] in (28, 29), msg


def test_rejects_residual_columns_from_behind_the_seam():
    """(f) C = 340: the residual/skip seam lies inside column pair 10 (columns 320 .. 351).  Layer 1's last two residual columns
    take the values of its first two skip columns."""
    C = 340
    ref, w_end = _rs_case(C)

    def seam(ll, r):
        if ll == 1:
            r = r.copy()
            r[..., C - 2:C] = r[..., C:] @ w_end[:, :2]
        return r

    rep, _, msg = _report_defect(f"C{C}", "(f) residual columns 338, 339 from skip columns 0, 1", ref,
                                 ref.port_result(taps={ii: {"res_skip": seam} for ii in ref.items}))
    assert not rep["wn_hidden"]["ok"] and rep["wn_hidden"]["where"]["channel"] in (C - 2, C - 1), msg


def test_rejects_a_row_tile_from_the_tile_before():
    """(g) C = 324: layer 1's res/skip output of item 1 has the rows of the 16-row tile 240 .. 255 in its tile 256 .. 271 too."""
    ref, _ = _rs_case(324)

    def tile(ll, r):
        if ll == 1:
            r = r.copy()
            r[:, 256:272] = r[:, 240:256]
        return r

    rep, _, msg = _report_defect("C324", "(g) rows 256 .. 271 take the rows 240 .. 255", ref,
                                 ref.port_result(taps={1: {"res_skip": tile}}))
    w = rep["wn_hidden"]["where"]
    assert not rep["wn_hidden"]["ok"] and w["item"] == 1 and 256 <= w["row"] < 272, msg
    assert not rep["wn_out"]["ok"], msg


@pytest.mark.parametrize("C", [324, 68])
def test_rejects_a_tail_without_its_last_channel_block(C):
    """(h) The tail drops the last 16-channel block of its input, the last layer's gate output: 4 channels at C = 324 and C = 68."""
    ref, _ = _rs_case(C)
    first = (C - 1) // 16 * 16
    assert C - first == 4

    def drop(ll, a):
        if ll == 2:
            a = a.copy()
            a[..., first:] = 0
        return a

    rep, _, msg = _report_defect(f"C{C}", f"(h) the tail without channels {first} .. {C - 1}", ref,
                                 ref.port_result(taps={ii: {"gate_out": drop} for ii in ref.items}))
    assert not rep["wn_out"]["ok"] and rep["wn_hidden"]["ok"], msg

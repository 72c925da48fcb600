"""The F(4,3) gate blocks of two column tiles (wn_gate_winograd4q_kernel: 256 rows x 64 gate channels, a wave owns 16 groups x
128 weight columns) give the bits of the 256-row blocks of one column tile: canonical models on a ragged batch, the layers
the shape does not cover, the launch-size rule, and the ABI that reports and pins it (mbx_kernel_report_info.
gate_block_channels, mbx_config.tune_gate_shape 1 | 4)."""
import ctypes

import numpy as np
import pytest

from oracle import mbexwn_oracle as orc
from helpers import build_case, synthetic_inputs

E2E_TOL = 1e-4          # the bar of test_gpu_parity.test_f43_block_shapes_give_the_same_bits
LENGTHS = [240, 133, 7]  # 4 800 rows; 2 660 rows: ends inside a block; 140 rows: shorter than one block
_WN = "mbexwn_config:pp_mod_subnet:"
# launch-size rule of csrc/wn_plan.h (gate_shape_policy, WIDE_FROM_BLOCKS): 256-row blocks of one column tile a launch
# must have to take the blocks of two -- (batch, frames) of the smallest SPEECH launch of 800-frame items above it, one below
WIDE_FROM_BLOCKS = 5040
ABOVE, BELOW = (8, 800), (8, 787)      # 63 x 8 x 10 = 5 040 blocks | 62 x 8 x 10 = 4 960


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    assert _torch.cuda.is_available(), "GPU tests need an MI355X"
    return _torch


def _run(torch, model, mel, noise, lengths=None, **kw):
    """(audio, kernel_report, gate_form of the launch) of one forward of a fresh engine."""
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    cfg, raw, wt = model
    eng = MBExWNEngine(cfg, raw, wt, **kw)
    nf = None if lengths is None else torch.as_tensor(lengths, dtype=torch.int32).cuda()
    audio = eng.forward(torch.as_tensor(mel).cuda(), n_frames=nf, noise=torch.as_tensor(noise).cuda()).cpu().numpy()
    rep = eng.kernel_report()
    form = eng.gate_form(mel.shape[0], mel.shape[1])
    # the report with the struct size of a caller built before gate_block_channels existed: accepted, the field untouched
    from mbexwn_vocoder_amd import engine
    old = engine.mbx_kernel_report_info()
    old.struct_size = engine.mbx_kernel_report_info.gate_block_channels.offset
    for ll in range(engine.MBX_MAX_WN_LAYERS):
        old.gate_block_channels[ll] = -7
    assert eng._lib.mbx_kernel_report(eng._handle, ctypes.byref(old)) == 0
    assert old.tail_kernel != 0 and all(vv == -7 for vv in old.gate_block_channels)
    eng.close()
    return audio, rep, form


@pytest.mark.gpu
@pytest.mark.parametrize("voice", ["SPEECH", "VOICE"])
def test_two_tile_blocks_give_the_bits_of_the_256_row_blocks(torch, voice):
    """SPEECH (C = 320: ten column tiles, five pairs) and VOICE (C = 340: eleven tiles -- the odd last one, a partial tile,
    runs in 256-row blocks -- and a partial last K slice), ragged batch; the 133-frame item is held to the float64 oracle."""
    model = build_case(voice, {})
    mel, noise = synthetic_inputs(77, len(LENGTHS), max(LENGTHS))
    wide, rep_w, form_w = _run(torch, model, mel, noise, LENGTHS, conv_form="f43", tune={"gate_shape": 4})
    base, rep_b, form_b = _run(torch, model, mel, noise, LENGTHS, conv_form="f43", tune={"gate_shape": 1})
    assert rep_w["gate_kernels"][1:] == ["f43"] * 4 and rep_b["gate_kernels"][1:] == ["f43"] * 4
    assert rep_w["gate_block_channels"][1:] == [64] * 4 and rep_b["gate_block_channels"][1:] == [32] * 4
    assert rep_w["gate_block_channels"][0] == rep_b["gate_block_channels"][0] == 0        # the folded first layer
    assert form_w == form_b == "winograd_f43"
    bad = np.argwhere(wide != base)
    assert bad.size == 0, f"{voice}: the blocks of two column tiles differ from the 256-row blocks, first at {bad[0]}"
    cfg, raw, wt = model
    ref = orc.OracleModel(cfg, raw, wt).forward(mel[1:2, :133], noise[1:2, :133 * 20])[0]
    err = float(np.max(np.abs(wide[1, :133 * 300].astype(np.float64) - ref)))
    bar = E2E_TOL * max(1.0, float(np.max(np.abs(ref))))
    print(f"\n{voice} two-tile blocks, 133-frame item vs the float64 oracle: {err:.3e} (bar {bar:.3e})")
    assert err <= bar


@pytest.mark.gpu
def test_layers_the_shape_does_not_cover_fall_back_with_the_same_bits(torch):
    """Six layers (d = 1 .. 32): pinned to two column tiles, the layers with d <= 16 run them and the d = 32 layer the strided
    256-row blocks; the audio is that of the pinned 256-row run."""
    model = build_case("SPEECH", {_WN + "n_layers": 6})
    mel, noise = synthetic_inputs(78, 2, 133)
    wide, rep_w, _ = _run(torch, model, mel, noise, [133, 40], conv_form="f43", tune={"gate_shape": 4})
    base, rep_b, _ = _run(torch, model, mel, noise, [133, 40], conv_form="f43", tune={"gate_shape": 1})
    assert rep_w["gate_kernels"][1:] == ["f43"] * 4 + ["f43_strided"] and rep_w["gate_block_channels"][1:] == [64] * 4 + [32]
    assert rep_b["gate_kernels"][1:] == ["f43"] * 4 + ["f43_strided"] and rep_b["gate_block_channels"][1:] == [32] * 5
    assert np.array_equal(wide, base)


@pytest.mark.gpu
def test_force_causal_model_keeps_the_bits_under_the_pin(torch):
    """A force_causal model (causal WaveNet padding: the staged rows start d rows earlier) pinned to F(4,3): two column tiles
    against 256-row blocks, whichever kernel the launcher took; the report says which."""
    model = build_case("SPEECH", {"mbexwn_config:force_causal": True})
    mel, noise = synthetic_inputs(79, 2, 133)
    wide, rep_w, _ = _run(torch, model, mel, noise, [133, 40], conv_form="f43", tune={"gate_shape": 4})
    base, rep_b, _ = _run(torch, model, mel, noise, [133, 40], conv_form="f43", tune={"gate_shape": 1})
    print(f"\nforce_causal pinned to two column tiles: {rep_w['gate_kernels']} {rep_w['gate_block_channels']}")
    assert rep_b["gate_block_channels"][1:] == [32] * 4 and set(rep_w["gate_block_channels"][1:]) <= {32, 64}
    assert set(rep_w["gate_kernels"][1:]) == {"f43"}
    assert np.array_equal(wide, base)


@pytest.mark.gpu
def test_default_policy_takes_the_shape_by_launch_size(torch):
    """Under the default policy the launch-size rule picks the block shape; either way the audio is that of the pinned
    256-row blocks and the form is reported as winograd_f43."""
    model = build_case("SPEECH", {})
    tiles = 10
    for (batch, frames), want in ((ABOVE, 64), (BELOW, 32)):
        blocks = ((frames * 20 + 255) // 256) * batch * tiles
        assert (blocks >= WIDE_FROM_BLOCKS) == (want == 64)
        mel, noise = synthetic_inputs(80, batch, frames)
        got, rep, form = _run(torch, model, mel, noise, None, conv_form="f43")
        base, rep_b, _ = _run(torch, model, mel, noise, None, conv_form="f43", tune={"gate_shape": 1})
        assert form == "winograd_f43" and rep["gate_kernels"][1:] == ["f43"] * 4
        assert rep["gate_block_channels"][1:] == [want] * 4, (batch, frames, rep["gate_block_channels"])
        assert rep_b["gate_block_channels"][1:] == [32] * 4
        assert np.array_equal(got, base), (batch, frames)


def test_kernel_report_struct_sizes_and_gate_shape_range():
    """No GPU needed: mbx_kernel_report takes the struct size with and without gate_block_channels and refuses any other;
    mbx_create accepts tune_gate_shape 4 and refuses 5 (both before it touches the device)."""
    from mbexwn_vocoder_amd import engine
    lib = engine.load_library()
    err = lambda: lib.mbx_last_error().decode("utf-8", "replace")
    info = engine.mbx_kernel_report_info()
    assert engine.mbx_kernel_report_info.gate_block_channels.offset == ctypes.sizeof(engine.mbx_kernel_report_info) - 4 * engine.MBX_MAX_WN_LAYERS
    for size, known in ((ctypes.sizeof(info), True), (engine.mbx_kernel_report_info.gate_block_channels.offset, True),
                        (ctypes.sizeof(info) - 4, False), (0, False)):
        info.struct_size = size
        assert lib.mbx_kernel_report(None, ctypes.byref(info)) != 0
        assert ("struct_size" in err()) == (not known), (size, err())      # a known size gets as far as the null handle
    cfg, raw, wt = build_case("SPEECH", {})
    tensors = (engine.mbx_tensor * 1)()
    for shape, refused in ((4, False), (5, True)):
        cc, _ = engine.make_config(cfg, wt, tune={"gate_shape": shape})
        out = ctypes.c_void_p()
        assert lib.mbx_create(ctypes.byref(cc), tensors, 0, 0, ctypes.byref(out)) != 0        # (no tensors: never a handle)
        assert ("tune_" in err()) == refused, (shape, err())

"""The kernels of a forward are planned on the host before the first launch (csrc/wn_plan.h): mbx_plan answers what a
whole-item forward of a size would run without launching, and after such a forward the kernel report is that plan; with
the dynamic-LDS opt-ins done once at mbx_create, a forward holds no runtime call that a graph capture could not take."""
import numpy as np
import pytest

from helpers import GOLDEN_CASES, build_case, synthetic_inputs

pytestmark = pytest.mark.gpu

_WN = "mbexwn_config:pp_mod_subnet:"
F43 = {"conv_form": "f43"}
# (id, voice, overrides, engine arguments, the (batch, frames) sizes run on one handle)
CASES = [
    # the canonical C = 320 model: 30 rows-per-item tiles to 8 x 800 frames = 5 040 blocks (the two-tile shape of large launches)
    ("speech", "SPEECH", {}, {}, [(1, 30), (2, 240), (8, 800)]),
    *[(f"speech-shape{ss}", "SPEECH", {}, dict(F43, tune={"gate_shape": ss}), [(1, 30), (2, 240)]) for ss in (1, 2, 3, 4)],
    ("speech-split-f16", "SPEECH", {}, dict(F43, precision="split_f16"), [(1, 30), (2, 240)]),
    ("voice", "VOICE", {}, {}, [(2, 240)]),                                       # C = 340: a partial column tile, 12 pairs
    ("deep12", "SPEECH", {_WN + "n_layers": 12}, F43, [(1, 240)]),                # dilations up to 2048
    ("two-blocks", *GOLDEN_CASES["blocks"][:2], F43, [(2, 30)]),
]


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    assert _torch.cuda.is_available(), "GPU tests need an MI355X"
    return _torch


@pytest.mark.parametrize("cid,voice,overrides,kwargs,sizes", CASES, ids=[cc[0] for cc in CASES])
def test_plan_is_what_the_forward_reports(torch, cid, voice, overrides, kwargs, sizes):
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    cfg, raw, wt = build_case(voice, overrides)
    eng = MBExWNEngine(cfg, raw, wt, **kwargs)
    seen = set()
    for batch, frames in sizes:
        plan = eng.plan(batch, frames)                     # before the forward: nothing was launched for this size yet
        mel, noise = synthetic_inputs(41, batch, frames, steps_per_frame=eng.dims.wn_in_rows_per_frame)
        audio = eng.forward(torch.as_tensor(mel).cuda(), noise=torch.as_tensor(noise).cuda())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(audio).all())
        rep = eng.kernel_report()
        print(cid, batch, frames, rep)
        assert plan == rep, (cid, batch, frames)
        assert eng.plan(batch, frames) == rep
        assert len(rep["gate_kernels"]) == len(rep["gate_block_channels"]) >= 2 and "none" not in rep["gate_kernels"]
        seen |= set(rep["gate_kernels"])
    if cid == "speech":
        assert {"folded_start", "f43_psplit", "f43"} <= seen or {"folded_start", "f43_hsplit", "f43"} <= seen
        assert max(rep["gate_block_channels"]) == 64      # (8, 800): the blocks of two column tiles
    if cid == "speech-split-f16":
        assert eng.conv_form_info()["split_rejected"] or seen & {"split_f16", "split_f16_wide"}
    if cid == "deep12":
        assert seen & {"f43_strided", "f43_strided_psplit", "direct"}
    eng.close()


def test_forward_of_the_canonical_model_replays_from_a_graph(torch):
    """A forward inside a graph capture replays to the eager result: no runtime call is left on the launch path (the
    LDS-size attributes of the gate kernels are set at mbx_create), at the size of a single short utterance."""
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    cfg, raw, wt = build_case("SPEECH", {})
    eng = MBExWNEngine(cfg, raw, wt)
    mel, noise = synthetic_inputs(43, 1, 30)
    mel_d, noise_d = torch.as_tensor(mel).cuda(), torch.as_tensor(noise).cuda()
    out = torch.empty((1, 30 * eng.dims.hop_size), dtype=torch.float32, device="cuda")
    eager = eng.forward(mel_d, noise=noise_d).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.forward(mel_d, noise=noise_d, out=out)          # warm-up on the capture stream (workspace allocation)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.forward(mel_d, noise=noise_d, out=out)
    planned = eng.plan(1, 30)
    assert eng.kernel_report() == planned
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    mel2, noise2 = synthetic_inputs(44, 1, 30)
    mel_d.copy_(torch.as_tensor(mel2).cuda())
    noise_d.copy_(torch.as_tensor(noise2).cuda())
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eng.forward(mel_d, noise=noise_d))
    assert np.isfinite(out.cpu().numpy()).all()
    eng.close()

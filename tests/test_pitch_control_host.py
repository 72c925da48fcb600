"""Per-frame pitch control on the host side (no GPU): the three trailing fields of mbx_forward_options in the ctypes mirror,
and the control rows of the streaming driver -- they travel with their frames through the shared rows, reach the engine
only once a synthesizer has seen control, and malformed values are refused at push()."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mbexwn_vocoder_amd import engine
from mbexwn_vocoder_amd.config import ModelDims, canonical_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTROL = ("f0_frames", "f0_scale", "f0_item_mask")


def test_control_fields_match_c(tmp_path):
    """sizeof(mbx_forward_options) and the offsets of the new fields as gcc lays the header out, against the mirror; the new
    fields are the last ones, so the offset of f0_frames is the size the struct had before them (the second accepted
    struct_size)."""
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mbexwn.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %d\\n", sizeof(mbx_forward_options),'
                   ' offsetof(mbx_forward_options, fe_end_frames), offsetof(mbx_forward_options, f0_frames),'
                   ' offsetof(mbx_forward_options, f0_scale), offsetof(mbx_forward_options, f0_item_mask), MBX_ABI_VERSION);'
                   ' return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(vv) for vv in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    opt = engine.mbx_forward_options
    assert got[:5] == [ctypes.sizeof(opt), opt.fe_end_frames.offset, opt.f0_frames.offset, opt.f0_scale.offset,
                       opt.f0_item_mask.offset]
    assert got[5] == 11                                              # an extension inside ABI 11
    assert opt.fe_end_frames.offset < opt.f0_frames.offset < opt.f0_scale.offset < opt.f0_item_mask.offset
    assert ctypes.sizeof(opt) == opt.f0_item_mask.offset + ctypes.sizeof(ctypes.c_void_p)
    assert [name for name, _ in opt._fields_][-3:] == list(CONTROL)


class _PitchFakeEngine:
    """CPU test double of the engine surface the streaming driver uses (not the oracle, not a product path).  The audio of
    frame t is (sum(mel[t]) + noise[t * spf]) * scale[t] + f0[t] on every sample of the frame -- scale[t] = 1 without
    f0_scale, f0[t] = 0 for an item whose mask is 0 or without f0_frames -- so the streamed output is known in closed form
    and a control row that does not travel with its frame shows up.  Records which control keywords every call carried."""

    def __init__(self):
        import torch
        cfg = canonical_config("SPEECH")
        self.config, self.dims, self.device = cfg, ModelDims(cfg), torch.device("cpu")
        self.calls = []

    def layer_state_info(self):
        return 0, 0, 0

    def conv_form_info(self):
        return {"split_f16_layers": 0, "split_f16_gate_layers": 0}

    def forward(self, mel, n_frames=None, noise=None, stream_state=None, **kw):
        import torch
        self.calls.append(tuple(kk for kk in CONTROL if kk in kw))
        hop, spf = self.dims.hop_size, self.dims.steps_per_frame
        val = mel.sum(dim=2) + noise[:, ::spf]
        if kw.get("f0_scale") is not None:
            assert kw["f0_scale"].shape == val.shape and kw["f0_scale"].dtype == torch.float32
            val = val * kw["f0_scale"]
        if kw.get("f0_frames") is not None:
            assert kw["f0_frames"].shape == val.shape and kw["f0_frames"].dtype == torch.float32
            mask = kw.get("f0_item_mask")
            assert mask is None or (mask.dtype == torch.int32 and tuple(mask.shape) == (val.shape[0],))
            val = val + (kw["f0_frames"] if mask is None else kw["f0_frames"] * mask[:, None].to(torch.float32))
        return val.repeat_interleave(hop, dim=1), torch.zeros_like(stream_state)


def _stream_data(rng, frames):
    return (rng.normal(size=(frames, 80)).astype(np.float32), rng.normal(size=(frames * 20,)).astype(np.float32))


def test_control_rows_travel_with_their_frames():
    """Three streams -- 700 frames with a transposition contour, 45 frames with external F0 frames, 300 frames with neither
    -- pushed in irregular packets through rows that drop and grow: the streamed output is the closed form of the test
    double.  Tolerance: every value is below 1024 in magnitude (float32 spacing 6.1e-5), the 80-term sums of the double and
    of numpy differ by at most 2e-5 (the bound of test_shared_input_rows_drop_and_grow), doubled by the largest factor; one
    rounding each for the product and the sum, half a spacing each: 4e-5 + 2 * 3.1e-5 < 2e-4.  A control row that is one
    frame off changes a value by the step of the contour times ~400, or by tens of Hz."""
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    fake = _PitchFakeEngine()
    syn = StreamingSynthesizer(fake, chunk_frames=8)
    syn.use_graph = False
    rng = np.random.default_rng(0)
    lengths = {"a": 700, "b": 45, "c": 300}
    data = {sid: _stream_data(rng, ll) for sid, ll in lengths.items()}
    scale = {"a": rng.uniform(0.5, 2.0, size=700).astype(np.float32)}
    f0 = {"b": rng.uniform(80.0, 400.0, size=45).astype(np.float32)}
    got = {sid: [] for sid in lengths}
    pos = {sid: 0 for sid in lengths}

    def push(sid, nn):
        mel, noise = data[sid]
        lo, hi = pos[sid], pos[sid] + nn
        extra = {}
        if sid in scale:
            extra["transposition"] = scale[sid][lo:hi]
        if sid in f0:
            extra["f0"] = f0[sid][lo:hi]
        syn.push(sid, mel[lo:hi], noise[lo * 20:hi * 20], last=hi >= lengths[sid], **extra)
        pos[sid] = hi

    syn.open("a")
    syn.open("b", f0="frames")
    push("a", 300)                                                    # more than a row holds: the rows grow
    assert syn._in_cap >= 300 and syn._in_scale.shape[1] == syn._in_cap == syn._in_f0.shape[1]
    for tick in range(400):
        if tick == 3:
            syn.open("c")
        for sid in list(syn.streams):
            if pos[sid] < lengths[sid]:
                push(sid, min(int(rng.integers(1, 13)), lengths[sid] - pos[sid]))     # slower than the ticks consume
        for sid, audio in syn.tick().items():
            got[sid].append(audio)
        if len(syn.streams) == 3 and all(syn.finished(sid) for sid in lengths):
            break
    assert syn._in_cap == 512 and syn.streams["a"].base > 0          # old frames of "a" were dropped, with their control rows
    for sid, ll in lengths.items():
        mel, noise = data[sid]
        want = (mel.sum(axis=1) + noise[::20]) * scale.get(sid, np.float32(1.0)) + f0.get(sid, np.float32(0.0))
        out = np.concatenate(got[sid])
        assert out.shape == (ll * 300,)
        np.testing.assert_allclose(out, np.repeat(want.astype(np.float32), 300), rtol=0, atol=2e-4)


def test_control_arguments_appear_with_the_first_control_and_stay():
    """A synthesizer that never saw control calls forward without any of the new keywords (the launch sequence of a server
    that only resynthesises is unchanged); from the first controlled push on every call carries all three."""
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    rng = np.random.default_rng(1)
    mel, noise = _stream_data(rng, 120)

    def serve(syn, sid, lo, hi, **extra):
        for pp in range(lo, hi, 8):
            more = {kk: vv[pp:pp + 8] if np.ndim(vv) else vv for kk, vv in extra.items()}
            syn.push(sid, mel[pp:pp + 8], noise[pp * 20:(pp + 8) * 20], last=pp + 8 >= 120, **more)
            syn.tick()

    fake = _PitchFakeEngine()
    syn = StreamingSynthesizer(fake, chunk_frames=8)
    syn.open(0)
    serve(syn, 0, 0, 120, transposition=1.0)                          # a factor of 1 is no control
    assert len(fake.calls) >= 10 and set(fake.calls) == {()}
    fake = _PitchFakeEngine()
    syn = StreamingSynthesizer(fake, chunk_frames=8)
    syn.open(0)
    serve(syn, 0, 0, 64)
    before = len(fake.calls)
    assert before >= 4 and set(fake.calls) == {()}
    serve(syn, 0, 64, 96, transposition=np.full(120, 1.25, dtype=np.float32))
    serve(syn, 0, 96, 120)                                            # the flag is sticky
    assert len(fake.calls) > before + 3 and set(fake.calls[before:]) == {CONTROL}
    fake = _PitchFakeEngine()
    syn = StreamingSynthesizer(fake, chunk_frames=8)
    syn.open(0, f0="frames")                                          # a "frames" stream is control from its first tick
    serve(syn, 0, 0, 120, f0=np.full(120, 200.0, dtype=np.float32))
    assert len(fake.calls) >= 10 and set(fake.calls) == {CONTROL}


def test_push_refuses_malformed_control():
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    syn = StreamingSynthesizer(_PitchFakeEngine(), chunk_frames=8)
    syn.open("net")
    syn.open("frames", f0="frames")
    with pytest.raises(ValueError):
        syn.open("other", f0="pulses")
    rng = np.random.default_rng(2)
    mel, noise = _stream_data(rng, 4)
    good = np.full(4, 150.0, dtype=np.float32)
    for bad in (np.asarray([150.0, 0.0, 150.0, 150.0]), np.asarray([150.0, -1.0, 150.0, 150.0]),
                np.asarray([150.0, np.nan, 150.0, 150.0]), np.asarray([150.0, np.inf, 150.0, 150.0]), good[:3]):
        with pytest.raises(ValueError):
            syn.push("frames", mel, noise, f0=bad)
        with pytest.raises(ValueError):
            syn.push("frames", mel, noise, f0=good, transposition=bad / 150.0)
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError):
            syn.push("net", mel, noise, transposition=bad)
    with pytest.raises(ValueError):
        syn.push("net", mel, noise, f0=good)                          # f0 on a "net" stream
    with pytest.raises(ValueError):
        syn.push("frames", mel, noise)                                # a "frames" stream without f0
    assert syn.streams["net"].have == 0 and syn.streams["frames"].have == 0        # a refused push appends nothing
    syn.push("frames", mel, noise, f0=good, transposition=2.0)
    syn.push("net", mel, noise, transposition=np.full(4, 0.5))
    assert syn.streams["net"].have == 4 and syn.streams["frames"].have == 4

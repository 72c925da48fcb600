"""MBExWNEngine.forward on the host (no GPU, no library): which library entry point a combination of arguments takes
(engine.forward_entry_point) and which combinations are refused, against a table written out from the forward that had
one copy of the call per branch."""
import itertools
import re

import pytest
import torch

from mbexwn_vocoder_amd import engine
from mbexwn_vocoder_amd.config import ModelDims, canonical_config

B, T = 2, 12


class _HostEngine(engine.MBExWNEngine):
    """The engine without a library handle: enough for the argument checks of forward, on CPU tensors."""

    def __init__(self):
        self.config = canonical_config("SPEECH")
        self.dims, self.device, self._torch = ModelDims(self.config), torch.device("cpu"), torch


def _arguments(eng, state=False, active=False, control=None, f0=False, transposition=1.0, wavenet=False, carry=False,
               layers=False, frontend=False):
    """The arguments of _forward_options with well-formed tensors for everything that is asked for."""
    ints = lambda *shape: torch.zeros(shape, dtype=torch.int32)                                     # noqa: E731
    floats = lambda *shape: torch.ones(shape, dtype=torch.float32)                                  # noqa: E731
    control = control or ()
    return dict(
        B=B, T=T, stream_state=ints(B, 6) if state else None, state_out=None,
        active=(2, ints(B), 8) if active else None, wavenet=(4, ints(B), 6) if wavenet else None,
        carry=(floats(4, 180, eng.dims.subbands), ints(B, 5)) if carry else None,
        layers=(floats(4, 64), ints(B, 3), 0) if layers else None,
        frontend=(floats(4, 64, eng.frontend_frame_floats), ints(B), 0, 0) if frontend else None,
        f0=floats(B, T * eng.dims.pulse_per_frame) if f0 else None, transposition=transposition,
        f0_frames=floats(B, T) if "f0_frames" in control else None, f0_scale=floats(B, T) if "f0_scale" in control else None,
        f0_item_mask=ints(B) if "f0_item_mask" in control else None)


# (state, active, control, f0, transposition other than 1) -> entry point; the combinations that are missing are refused
ENTRY = {
    (False, False, False, False, False): "mbx_forward",
    (False, False, False, True, False): "mbx_forward_ex",
    (False, False, False, False, True): "mbx_forward_ex",
    (False, False, False, True, True): "mbx_forward_ex",
    (False, False, True, False, False): "mbx_forward_ex",
    (False, False, True, True, False): "mbx_forward_ex",          # f0 next to f0_scale; next to f0_frames it is refused
    (True, False, False, False, False): "mbx_forward_stream",
    (True, False, True, False, False): "mbx_forward_ex",
    (True, True, False, False, False): "mbx_forward_ex",
    (True, True, True, False, False): "mbx_forward_ex",
}
CONTROLS = (("f0_frames",), ("f0_scale",), ("f0_frames", "f0_scale"), ("f0_frames", "f0_item_mask"),
            ("f0_frames", "f0_scale", "f0_item_mask"))


def test_entry_point_table():
    """Every combination of the five flags: the pure chooser on the legal ones, and the checked path -- entry point, the
    options' transposition (1 in a stream, the given factor for whole items), the state tensors -- on all 32."""
    eng = _HostEngine()
    for flags in itertools.product((False, True), repeat=5):
        state, active, control, f0, transposed = flags
        factor = 1.5 if transposed else 1.0
        for rows in (CONTROLS if control else ((),)):
            args = _arguments(eng, state=state, active=active, control=rows, f0=f0, transposition=factor)
            if flags not in ENTRY or (f0 and "f0_frames" in rows):
                with pytest.raises(ValueError):
                    eng._forward_options(**args)
                continue
            assert engine.forward_entry_point(*flags) == ENTRY[flags], flags
            entry, opt, alive, state_in, state_out = eng._forward_options(**args)
            assert entry == ENTRY[flags], (flags, rows)
            assert (opt is not None) == (entry == "mbx_forward_ex")
            assert (state_in is not None) == (state_out is not None) == state
            if opt is not None:
                assert opt.struct_size == engine.ctypes.sizeof(engine.mbx_forward_options)
                assert opt.transposition == (1.0 if state else factor)
                assert (opt.state_in, opt.state_out) == ((state_in.data_ptr(), state_out.data_ptr()) if state else (None, None))
                assert bool(opt.f0) == f0 and bool(opt.active_frames) == active
                for name in ("f0_frames", "f0_scale", "f0_item_mask"):
                    assert bool(getattr(opt, name)) == (name in rows), (flags, rows, name)
                # whatever the options point at stays alive with them
                held = {tt.data_ptr() for tt in alive if tt is not None}
                assert {pp for pp in (opt.f0, opt.active_frames, opt.f0_frames, opt.f0_scale, opt.f0_item_mask) if pp} <= held


REFUSED = [
    ("active without state", dict(active=True), "pass stream_state as well"),
    ("wavenet without state", dict(wavenet=True), "pass stream_state as well"),
    ("carry without state", dict(carry=True), "pass stream_state as well"),
    ("layers without state", dict(layers=True), "pass stream_state as well"),
    ("wavenet without active", dict(state=True, wavenet=True), "pass active as well"),
    ("carry without active", dict(state=True, carry=True), "pass active as well"),
    ("layers without active", dict(state=True, layers=True), "pass active as well"),
    ("frontend without active", dict(state=True, frontend=True), "pass active as well"),
    ("f0 with state", dict(state=True, f0=True), "apply to whole items: not with stream_state"),
    ("transposition with state", dict(state=True, active=True, transposition=2.0), "apply to whole items: not with stream_state"),
    ("f0_frames with f0", dict(f0=True, control=("f0_frames",)), "exclude each other"),
    ("f0_item_mask without f0_frames", dict(control=("f0_scale", "f0_item_mask")), "f0_item_mask needs f0_frames"),
    ("control with transposition", dict(control=("f0_scale",), transposition=2.0), "need transposition == 1"),
    ("control with transposition in a stream", dict(state=True, control=("f0_frames",), transposition=0.5),
     "apply to whole items: not with stream_state"),               # the first of the two checks that both hold
    ("transposition not positive", dict(transposition=-1.0), "transposition must be positive"),
    ("frontend without carry", dict(state=True, active=True, frontend=True), "carry is required"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[cc[0] for cc in REFUSED])
def test_refused_combinations(case):
    _, asked, text = case
    eng = _HostEngine()
    with pytest.raises(ValueError, match=text):
        eng._forward_options(**_arguments(eng, **asked))


def _whole_items(eng):
    return _arguments(eng, f0=True)


def _window(eng):
    args = _arguments(eng, state=True, active=True, wavenet=True, carry=True, layers=True, frontend=True,
                      control=("f0_frames", "f0_scale", "f0_item_mask"))
    return dict(args, state_out=torch.zeros((B, 6), dtype=torch.int32))


# every tensor argument of _forward_options: (name, the call it belongs to, key in the arguments, index in that key's tuple or
# None, its message, whether it must be contiguous, whether a non-tensor is refused with the same message)
TENSORS = [
    ("stream_state", _window, "stream_state", None, "stream_state must be an int32 tensor of shape (batch, 6) on the", False, False),
    ("state_out", _window, "state_out", None, "state_out must be a contiguous int32 tensor of shape (batch, 6) on the", True, False),
    ("active[1]", _window, "active", 1, "active = (begin frame inside the window, int32 tensor of shape (batch,) on", False, False),
    ("wavenet[1]", _window, "wavenet", 1, "wavenet = (begin frame inside the active region, int32 tensor (batch,) on", False, False),
    ("carry store", _window, "carry", 0, "carry store must be a contiguous float32 tensor (slots, rows, subbands) on", True, False),
    ("carry descriptors", _window, "carry", 1, "carry descriptors must be an int32 tensor of shape (batch, 5) on", False, False),
    ("layer store", _window, "layers", 0, "layer store must be a contiguous float32 tensor (slots, floats) on", True, False),
    ("layer descriptors", _window, "layers", 1, "layer descriptors must be an int32 tensor of shape (batch, 3) on", False, False),
    ("front-end ring", _window, "frontend", 0, "front-end ring must be a contiguous float32 tensor (slots, ring frames, ", True, False),
    ("front-end positions", _window, "frontend", 1, "front-end positions must be an int32 tensor (batch,) on", False, False),
    ("f0", _whole_items, "f0", None, f"f0 must be a float32 tensor of shape ({B}, ", False, False),
    ("f0_frames", _window, "f0_frames", None, f"f0_frames must be a float32 tensor of shape ({B}, {T}) on", False, True),
    ("f0_scale", _window, "f0_scale", None, f"f0_scale must be a float32 tensor of shape ({B}, {T}) on", False, True),
    ("f0_item_mask", _window, "f0_item_mask", None, f"f0_item_mask must be an int32 tensor of shape ({B},) on", False, True),
]
BAD = {
    "dtype": lambda good: good.double(),
    "shape": lambda good: good.unsqueeze(0),                  # one dimension more: wrong for the fixed and the open shapes alike
    "view": lambda good: torch.zeros(tuple(good.shape[:-1]) + (2 * good.shape[-1],), dtype=good.dtype)[..., ::2],
    "non-tensor": lambda good: good.numpy(),
}
TENSOR_CASES = [(row, kind) for row in TENSORS for kind in BAD
                if kind in ("dtype", "shape") or (kind == "view" and row[5]) or (kind == "non-tensor" and row[6])]


@pytest.mark.parametrize("row,kind", TENSOR_CASES, ids=[f"{row[0]}-{kind}" for row, kind in TENSOR_CASES])
def test_tensor_arguments_are_refused_with_their_message(row, kind):
    """One tensor argument at a time with a wrong dtype, a wrong shape, a non-contiguous view where contiguity is demanded,
    a numpy array where a non-tensor is refused by name: ValueError with that argument's message; the call is fine without."""
    _, base, key, index, text, _, _ = row
    eng = _HostEngine()
    args = base(eng)
    eng._forward_options(**args)
    good = args[key] if index is None else args[key][index]
    bad = BAD[kind](good)
    if kind == "view":
        assert tuple(bad.shape) == tuple(good.shape) and bad.dtype == good.dtype and not bad.is_contiguous()
    args[key] = bad if index is None else args[key][:index] + (bad,) + args[key][index + 1:]
    with pytest.raises(ValueError, match=re.escape(text)):
        eng._forward_options(**args)


def test_window_arguments_reach_the_options():
    """A whole streaming window: every field of the options its arguments set, and the shapes that are refused."""
    eng = _HostEngine()
    args = _arguments(eng, state=True, active=True, wavenet=True, carry=True, layers=True, frontend=True,
                      control=("f0_frames", "f0_scale", "f0_item_mask"))
    args["layers"] = args["layers"][:2] + (160,)
    args["frontend"] = args["frontend"][:2] + (9, 3, 11)
    entry, opt, alive, _, _ = eng._forward_options(**args)
    assert entry == "mbx_forward_ex"
    assert (opt.active_begin, opt.active_max_frames, opt.wn_begin, opt.wn_max_frames) == (2, 8, 4, 6)
    assert (opt.sub_store, opt.sub_store_rows, opt.sub_carry) == (args["carry"][0].data_ptr(), 180, args["carry"][1].data_ptr())
    assert (opt.layer_store, opt.layer_store_floats, opt.layer_rows) == (args["layers"][0].data_ptr(), 64, 160)
    assert (opt.fe_store, opt.fe_ring_frames, opt.fe_new_frames, opt.fe_margin_frames, opt.fe_end_frames) == (
        args["frontend"][0].data_ptr(), 64, 9, 3, 11)
    assert {opt.active_frames, opt.wn_frames, opt.sub_carry, opt.layer_carry, opt.fe_pos} <= {tt.data_ptr() for tt in alive}
    for name, bad in (("active", (T, args["active"][1])), ("wavenet", (1, args["wavenet"][1])),
                      ("carry", (args["carry"][0], torch.zeros((B, 4), dtype=torch.int32))),
                      ("layers", (args["layers"][0], torch.zeros((B, 3), dtype=torch.int64), 0)),
                      ("stream_state", torch.zeros((B, 5), dtype=torch.int32))):
        with pytest.raises(ValueError):
            eng._forward_options(**dict(args, **{name: bad}))

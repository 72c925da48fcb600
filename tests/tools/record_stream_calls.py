#!/usr/bin/env python3
"""Recorded-call characterisation of the streaming driver, on the CPU: drives StreamingSynthesizer through its public
surface with a recording test double of the engine and writes every argument of every engine call, as integers and
sha256 digests, to tests/golden/stream_calls.json.  tests/test_stream_plan_host.py re-runs the scenarios and requires
equality with that file field by field, so a change of the driver that moves one window, region, descriptor or carried
state shows up without a GPU.

    python tests/tools/record_stream_calls.py            # rewrite the fixture (only when the driver's behaviour is
                                                         # meant to change)

Every input comes from closed-form integer formulas (no random generator)."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mbexwn_vocoder_amd.config import ModelDims, canonical_config  # noqa: E402
from mbexwn_vocoder_amd.streaming import StreamingSynthesizer, stream_margins  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "stream_calls.json")
CONTROL = ("f0_frames", "f0_scale", "f0_item_mask")
# the force_causal model of tests/test_causal_host.py (STREAM_SMALL + force_causal): causal branch of sr_left, unequal
# wn_left / wn_reach
_WN = "mbexwn_config:pp_mod_subnet:"
CAUSAL = {_WN + "n_channels": 32, _WN + "n_layers": 5, "mbexwn_config:force_causal": True}
LAYER_FLOATS, LAYER_MIN_ROWS, FRONTEND_FLOATS = 64, 48, 8
# frames a slowly fed stream receives per tick
PUSH_TABLE = (3, 11, 1, 7, 5, 12, 2, 9, 4, 6, 10, 8, 1, 5)


def _digest(tensor):
    return hashlib.sha256(np.ascontiguousarray(tensor.detach().numpy()).tobytes()).hexdigest()


def _ints(tensor):
    return [int(vv) for vv in tensor.reshape(-1).tolist()]


class RecordingEngine:
    """CPU test double of the engine surface the streaming driver uses (not the oracle, not a product path).  The audio
    of frame t is sum(mel[t]) + noise[t * spf] on every sample of the frame; the returned phase state differs from the
    one passed in (position + 1, recognisable floats), so a carried state is visible in the next call.  Every call is
    recorded in ``calls``."""
    frontend_carry_supported = True
    frontend_frame_floats = FRONTEND_FLOATS

    def __init__(self, cfg, layer_state=True):
        import torch
        self.config, self.dims, self.device = cfg, ModelDims(cfg), torch.device("cpu")
        reach = stream_margins(self.dims, cfg)[5] * self.dims.steps_per_frame
        self._layer_info = (LAYER_FLOATS, reach, LAYER_MIN_ROWS) if layer_state else (0, 0, 0)
        self.calls = []

    def layer_state_info(self):
        return self._layer_info

    def conv_form_info(self):
        return {"split_f16_layers": 0, "split_f16_gate_layers": 0}

    def forward(self, mel, n_frames=None, noise=None, stream_state=None, active=None, wavenet=None, carry=None,
                layers=None, frontend=None, **pitch):
        import torch
        B, T = int(mel.shape[0]), int(mel.shape[1])
        rec = {"B": B, "T": T, "n_frames": _ints(n_frames), "stream_state": _ints(stream_state),
               "mel": _digest(mel), "noise": _digest(noise)}
        for name, region in (("active", active), ("wavenet", wavenet)):
            rec[name] = None if region is None else [int(region[0]), _ints(region[1]), int(region[2])]
        rec["carry"] = None if carry is None else {"store": list(carry[0].shape), "desc": _ints(carry[1])}
        rec["layers"] = None if layers is None else {"store": list(layers[0].shape), "desc": _ints(layers[1]),
                                                     "rows": int(layers[2])}
        rec["frontend"] = None if frontend is None else {"store": list(frontend[0].shape), "pos": _ints(frontend[1]),
                                                         "rest": [int(vv) for vv in frontend[2:]]}
        rec["pitch"] = {kk: (_ints(vv) if vv.dtype == torch.int32 else [list(vv.shape), _digest(vv)])
                        for kk, vv in sorted(pitch.items())}
        self.calls.append(rec)
        hop, spf = self.dims.hop_size, self.dims.steps_per_frame
        val = mel.sum(dim=2) + noise[:, ::spf]
        state_out = stream_state.clone()
        marks = torch.arange(B, dtype=torch.float32) / 16 + len(self.calls)
        state_out[:, 0] = marks.view(torch.int32)
        state_out[:, 1] = (stream_state[:, 1].contiguous().view(torch.float32) + 0.5).view(torch.int32)
        state_out[:, 2] += 1
        return val.repeat_interleave(hop, dim=1), state_out


def _pattern(count, seed):
    """float32 values in [-1, 1) on a grid of 1/1024, from the flat index."""
    ii = np.arange(count, dtype=np.uint64) + np.uint64(seed * 7919)
    return (((ii * np.uint64(2654435761)) % np.uint64(2048)).astype(np.float32) / 1024 - 1).astype(np.float32)


def stream_data(dims, index, frames):
    """(mel (frames, channels), noise (frames * spf,), f0 (frames,) Hz) of the stream number ``index``."""
    mel = _pattern(frames * dims.mel_channels, 2 * index + 1).reshape(frames, dims.mel_channels)
    noise = _pattern(frames * dims.steps_per_frame, 2 * index + 2)
    f0 = (100 + (np.arange(frames) * 37 + index) % 200).astype(np.float32)
    return mel, noise, f0


def closed_form(dims, mel, noise):
    return np.repeat(mel.sum(axis=1) + noise[::dims.steps_per_frame], dims.hop_size)


# stream: (id, frames, tick it is opened at, frames pushed per tick: "all" at once, an int, or "table" = PUSH_TABLE)
_STREAMS = (("a", 190, 0, "all"), ("b", 120, 0, 16), ("c", 150, 0, "table"), ("d", 96, 4, 24))
_SHORT = (("a", 64, 0, "all"), ("b", 44, 0, 6), ("c", 50, 0, "table"), ("d", 30, 4, 8))
SCENARIOS = {
    "chunk8": {"chunk": 8, "streams": _STREAMS},
    # "d" joins one period of the schedule (5 ticks, 32 frames) behind "a" and "b": the same phase and alignment
    "schedule_80ms": {"chunk": (6, 6, 7, 6, 7),
                      "streams": (("a", 190, 0, "all"), ("b", 120, 0, 32), ("c", 150, 0, "table"), ("d", 96, 5, 32))},
    "chunk5": {"chunk": 5, "streams": _STREAMS},
    "chunk2": {"chunk": 2, "streams": _SHORT},
    "force_causal": {"chunk": 8, "streams": _STREAMS, "config": CAUSAL},
    # "q": plain; "r": its transposition leaves 1 at frame 72, pushed at tick 9 (the sticky flag flips there); "p": external
    # F0 frames, opened after that
    "pitch": {"chunk": 8, "streams": (("q", 150, 0, "all"), ("r", 110, 0, 8), ("p", 100, 11, 16)),
              "f0_frames": ("p",), "transposition_from": {"r": 72}},
    "chunk8_graph": {"chunk": 8, "streams": _STREAMS, "use_graph": True},
    "no_layer_state": {"chunk": 8, "streams": _STREAMS, "layer_state": False},
}


def run_scenario(name):
    """-> (record, {stream id: streamed audio}, {stream id: closed-form audio})."""
    sc = SCENARIOS[name]
    cfg = canonical_config("SPEECH", **sc.get("config", {}))
    eng = RecordingEngine(cfg, layer_state=sc.get("layer_state", True))
    dims = eng.dims
    syn = StreamingSynthesizer(eng, chunk_frames=sc["chunk"])
    syn.use_graph = bool(sc.get("use_graph", False))
    spf = dims.steps_per_frame
    data = {sid: stream_data(dims, ii, frames) for ii, (sid, frames, _, _) in enumerate(sc["streams"])}
    pos = {sid: 0 for sid in data}
    got = {sid: [] for sid in data}
    ticks = []
    for tick in range(1000):
        for ii, (sid, frames, open_tick, rate) in enumerate(sc["streams"]):
            if tick == open_tick:
                syn.open(sid, f0="frames" if sid in sc.get("f0_frames", ()) else "net")
            if tick < open_tick or pos[sid] >= frames:
                continue
            nn = frames if rate == "all" else PUSH_TABLE[(tick + 3 * ii) % len(PUSH_TABLE)] if rate == "table" else rate
            lo, hi = pos[sid], min(frames, pos[sid] + nn)
            mel, noise, f0 = data[sid]
            extra = {}
            if sid in sc.get("f0_frames", ()):
                extra["f0"] = f0[lo:hi]
            if sid in sc.get("transposition_from", {}):
                extra["transposition"] = np.where(np.arange(lo, hi) >= sc["transposition_from"][sid], 1.25, 1.0)
            syn.push(sid, mel[lo:hi], noise[lo * spf:hi * spf], last=hi >= frames, **extra)
            pos[sid] = hi
        before = len(eng.calls)
        out = syn.tick()
        for sid, audio in out.items():
            got[sid].append(audio)
        assert len(eng.calls) - before <= 1
        ticks.append({"ids": list(out), "lens": [int(len(vv)) for vv in out.values()],
                      "frames": int(syn.last_tick_frames), "active_frames": int(syn.last_tick_active_frames),
                      "wavenet_frames": int(syn.last_tick_wavenet_frames), "layer_rows": int(syn.last_tick_layer_rows),
                      "replayed": bool(syn.last_tick_replayed), "graph_ticks": int(syn.graph_ticks),
                      "use_graph": bool(syn.use_graph), "call": eng.calls[-1] if len(eng.calls) > before else None})
        if tick >= max(ss[2] for ss in sc["streams"]) and all(syn.finished(sid) for sid in data):
            break
    else:
        raise RuntimeError(f"{name}: the streams did not finish")
    audio = {sid: np.concatenate(got[sid]) for sid in data}
    want = {sid: closed_form(dims, mel, noise) for sid, (mel, noise, _) in data.items()}
    return {"ticks": ticks}, audio, want


def main():
    out = {}
    for name in SCENARIOS:
        out[name], _, _ = run_scenario(name)
        steady = sum(tt["layer_rows"] > 0 for tt in out[name]["ticks"])
        print(f"{name}: {len(out[name]['ticks'])} ticks, {steady} steady", file=sys.stderr)
    with open(FIXTURE if len(sys.argv) < 2 else sys.argv[1], "w") as fh:
        json.dump(out, fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()

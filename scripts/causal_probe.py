#!/usr/bin/env python3
"""Cost of force_causal against the SAME-padding model, on the canonical SPEECH model (C = 320, 5 layers).  GPU box:

    python scripts/causal_probe.py [OUT.json]

Uses only engine API that predates force_causal, so the same script times a tree without it (there it reports the SAME
model only: building a force_causal engine raises).

  * 16 x 10 s (800 frames) per forward, pinned to F(4,3) (and the causal model on its default form, which runs direct):
    the device time of every gate launch (mbx_profile_read_launches, HIP events around each launch), median per layer
    over STEPS forwards after a time-based warm-up;
  * 64 streams on the 80 ms schedule (6, 6, 7, 6, 7 frames), engines pinned to F(2,3) (the form streams run): device ms per
    steady tick (StreamingSynthesizer.time_device), median over whole periods after the graph captures.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = 25                 # profiled forwards per model (>= 20)
WARMUP_S = 2.0             # time-based warm-up of every engine before it is measured
SCHEDULE = (6, 6, 7, 6, 7)
MODELS = {"same": {}, "causal": {"mbexwn_config:force_causal": True}}


def build(overrides, **kw):
    from mbexwn_vocoder_amd.config import ModelDims, canonical_config
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    from mbexwn_vocoder_amd.tables import WaveTables
    from mbexwn_vocoder_amd.weights import synthetic_weights
    cfg = canonical_config("SPEECH", **overrides)
    dims = ModelDims(cfg)
    raw = synthetic_weights(cfg, seed=1234)
    wt = WaveTables(sample_rate=dims.pulse_rate, **cfg["mbexwn_config"]["wavetable_config"])
    return MBExWNEngine(cfg, raw, wt, **kw), dims


def inputs(torch, dims, batch, frames, seed=42):
    rng = np.random.default_rng(seed)
    mel = np.clip(np.log(np.exp(rng.normal(-5.0, 2.0, size=(batch, frames, 80))) + 1e-5), -11.5, 2.0).astype(np.float32)
    noise = rng.normal(size=(batch, frames * dims.steps_per_frame)).astype(np.float32)
    return torch.as_tensor(mel).cuda(), torch.as_tensor(noise).cuda()


def gate_layers(torch, overrides, conv_form, batch=16, frames=800):
    eng, dims = build(overrides, conv_form=conv_form)
    mel, noise = inputs(torch, dims, batch, frames)
    audio = torch.empty((batch, frames * dims.hop_size), dtype=torch.float32, device=mel.device)
    t_end = time.perf_counter() + WARMUP_S
    while time.perf_counter() < t_end:
        eng.forward(mel, noise=noise, out=audio)
        torch.cuda.synchronize()
    eng.profile_enable(True)
    eng.profile_read_launches("gate")
    eng.profile_read("gate0")
    per_step, first = [], []
    for _ in range(STEPS):
        eng.forward(mel, noise=noise, out=audio)
        torch.cuda.synchronize()
        per_step.append(eng.profile_read_launches("gate"))
        first.append(eng.profile_read("gate0")[0])
    eng.profile_enable(False)
    info = eng.conv_form_info()
    kernels = info["gate_kernels"]
    off = 1 if kernels[0] == "folded_start" else 0
    layers = []
    for ll in range(dims.wn_layers):
        ts = first if ll < off else [step[ll - off] for step in per_step if len(step) > ll - off]
        layers.append({"layer": ll, "dilation": dims.wn_dilation(ll), "kernel": kernels[ll],
                       "median_ms": round(float(np.median(ts)), 4)})
    eng.close()
    return {"conv_form": conv_form, "form": info["form"], "layers": layers}


def stream_ticks(torch, overrides, n_streams=64, periods=8):
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    eng, dims = build(overrides, conv_form="f23")
    syn = StreamingSynthesizer(eng, chunk_frames=SCHEDULE)
    syn.time_device = True
    lead = 6 * len(SCHEDULE)
    n_ticks = lead + periods * len(SCHEDULE)
    total = n_ticks * max(SCHEDULE) + syn.right + 8
    for sid in range(n_streams):
        syn.open(sid)
        rng = np.random.default_rng(1000 + sid)
        mel = np.clip(np.log(np.exp(rng.normal(-5.0, 2.0, size=(total, 80))) + 1e-5), -11.5, 2.0).astype(np.float32)
        syn.push(sid, mel, rng.normal(size=(total * dims.steps_per_frame,)).astype(np.float32))
    dev = []
    for tick in range(n_ticks):
        res = syn.tick()
        torch.cuda.synchronize()
        assert len(res) == n_streams
        if tick >= lead:
            dev.append(syn.last_tick_device_ms)
    out = {"streams": n_streams, "schedule": list(SCHEDULE), "lookahead_ms": syn.lookahead_ms,
           "margins": [syn.left, syn.right, syn.lead], "graph_ticks": syn.graph_ticks,
           "tick_device_ms_median": round(float(np.median(dev)), 4), "tick_device_ms_mean": round(float(np.mean(dev)), 4)}
    eng.close()
    return out


def main():
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    res = {"device": torch.cuda.get_device_name(0)}
    for name, over in MODELS.items():
        try:
            build(over)[0].close()
        except NotImplementedError as exc:          # a tree without force_causal
            res[name] = {"unsupported": str(exc)}
            continue
        res[name] = {"gate_f43": gate_layers(torch, over, "f43"), "stream_f23": stream_ticks(torch, over)}
        if name == "causal":
            res[name]["gate_auto"] = gate_layers(torch, over, "auto")
        print(name, json.dumps(res[name]), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()

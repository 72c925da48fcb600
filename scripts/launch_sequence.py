#!/usr/bin/env python3
"""The kernels a set of representative forwards launches, in dispatch order: the evidence that a change to the host side of
the C ABI (csrc/mbx_create.hip, mbx_forward.hip, mbx_api.hip) left every launch as it was.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/launch_sequence.py run
    python scripts/launch_sequence.py list OUT > profiles/launch_sequence.txt

`run` creates the handles below (their calibration forwards included) and runs one forward on each; `list` turns the
trace into one line per dispatch: kernel name (without its parameter list), grid size, workgroup size, LDS bytes.  Two
builds launch the same kernels iff their lists are equal (diff).  Seeded synthetic weights and inputs; no timing.
"""
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_WN = "mbexwn_config:pp_mod_subnet:"
BLOCKS2 = {"mbexwn_config:pp_mod_subnet_upsampling_factors": [2, 1], "mbexwn_config:pp_mod_subnet_channel_factors": [1, 0.5],
           "mbexwn_config:pulse_channels": 10, _WN + "cond_lin_upsampling": 5}
# (label, voice, config overrides, engine arguments, batch, frames)
CASES = [
    ("default 1 x 3 s", "SPEECH", {}, {}, 1, 240),
    ("default 16 x 10 s", "SING", {}, {}, 16, 800),
    ("conv_form f23", "SPEECH", {}, {"conv_form": "f23"}, 2, 240),
    ("conv_form direct", "SPEECH", {}, {"conv_form": "direct"}, 2, 240),
    ("batch_invariant", "SPEECH", {}, {"batch_invariant": True}, 2, 240),
    ("force_causal f23", "SPEECH", {"mbexwn_config:force_causal": True}, {"conv_form": "f23"}, 2, 240),
    ("two blocks", "SING", BLOCKS2, {}, 2, 240),
    ("split_f16", "SING", {}, {"precision": "split_f16"}, 2, 240),
    ("keep_skip keep_start", "SPEECH", {}, {"keep_skip": True, "keep_start": True}, 2, 240),
    ("12 layers d <= 2048, 1 x 3 s", "SPEECH", {_WN + "n_layers": 12}, {}, 1, 240),
]


def model(voice, overrides):
    from mbexwn_vocoder_amd.config import canonical_config
    from mbexwn_vocoder_amd.tables import WaveTables
    from mbexwn_vocoder_amd.config import ModelDims
    from mbexwn_vocoder_amd.weights import synthetic_weights
    cfg = canonical_config(voice, **overrides)
    dims = ModelDims(cfg)
    wt = WaveTables(sample_rate=dims.pulse_rate, **cfg["mbexwn_config"]["wavetable_config"])
    return cfg, synthetic_weights(cfg, seed=1234), wt, dims


def inputs(rng, batch, frames, rows_per_frame):
    mel = np.clip(np.log(np.exp(rng.normal(-5.0, 2.0, size=(batch, frames, 80))) + 1e-5), -11.5, 2.0).astype(np.float32)
    return mel, rng.normal(size=(batch, frames * rows_per_frame)).astype(np.float32)


def run():
    import torch
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    for label, voice, overrides, kw, batch, frames in CASES:
        cfg, raw, wt, dims = model(voice, overrides)
        eng = MBExWNEngine(cfg, raw, wt, **kw)
        mel, noise = inputs(np.random.default_rng(7), batch, frames, dims.wn_in_rows_per_frame)
        eng.forward(torch.as_tensor(mel).cuda(), noise=torch.as_tensor(noise).cuda())
        torch.cuda.synchronize()
        print(label, eng.gate_form(batch, frames), flush=True)
        eng.close()
    # eight ticks of four streams
    cfg, raw, wt, dims = model("SPEECH", {})
    eng = MBExWNEngine(cfg, raw, wt)
    syn = StreamingSynthesizer(eng, chunk_frames=8)
    for sid in range(4):
        syn.open(sid)
        mel, noise = inputs(np.random.default_rng(100 + sid), 1, 8 * 8 + syn.right + 16, dims.steps_per_frame)
        syn.push(sid, mel[0], noise[0])
    for _ in range(8):
        syn.tick()
        torch.cuda.synchronize()
    print("streams", eng.conv_form_info()["stream_form"], flush=True)


def listing(out_dir):
    files = sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True))
    if len(files) != 1:
        raise SystemExit(f"expected one kernel trace under {out_dir}, found {len(files)}")
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda rr: int(rr["Dispatch_Id"]))
    print("# kernel  grid  workgroup  lds_bytes   (scripts/launch_sequence.py; one line per dispatch, in dispatch order)")
    for rr in rows:
        name = rr["Kernel_Name"].split("(")[0].replace("void ", "")
        grid = "x".join(rr[f"Grid_Size_{ax}"] for ax in "XYZ")
        wg = "x".join(rr[f"Workgroup_Size_{ax}"] for ax in "XYZ")
        print(name, grid, wg, rr["LDS_Block_Size"])


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "list":
        listing(sys.argv[2])
    else:
        raise SystemExit(__doc__)

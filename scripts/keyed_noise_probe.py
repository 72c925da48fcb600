#!/usr/bin/env python3
"""The numbers of DESIGN.md section 6e (keyed noise) on one GPU, written as JSON (default: profiles/keyed_noise.json):

  float       max |z - ref| of mbxn_fill_normal over 2^20 values against noise.normals_reference, beside the numpy float32 port
  cost_us     device time of mbxn_fill_normal for 16 x 16 000 values (HIP events, 50 warm-up + 500 timed calls), torch.randn of
              the same shape and the 16 x 10 s forward in the same process
  throughput  transform_audio.py --batch 16 on 64 synthetic 10 s files (its own -v summary), and stream_transpose.py on four

    python scripts/keyed_noise_probe.py [OUT.json]
"""
import ctypes
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RESULT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "keyed_noise.json")
OUT = tempfile.mkdtemp(prefix="keyed_noise_probe_")
from mbexwn_vocoder_amd import engine, noise
from mbexwn_vocoder_amd.mel_inverter import MELInverter, create_synthetic_model_dir
res = {}
lib = engine.load_library()
dev = torch.device("cuda", 0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def fill(out, keys, counts, top):
    st = lib.mbxn_fill_normal(out.data_ptr(), out.shape[1], out.shape[0], keys.data_ptr(), None, counts.data_ptr(), top, stream())
    assert st == 0

# A. float ratio
nn = 1 << 20
key = noise.item_key("a.wav")
ref = noise.normals_reference(7, key, 0, nn)
port = float(np.max(np.abs(noise.normals_float32_port(7, key, 0, nn) - ref)))
out = torch.zeros((1, nn), device=dev)
keys = torch.as_tensor(np.array([[7, key]], dtype=np.uint64).view(np.int64)).to(dev)
fill(out, keys, torch.tensor([nn], dtype=torch.int32, device=dev), nn)
torch.cuda.synchronize()
got = out[0].cpu().numpy().astype(np.float64)
err = np.abs(got - ref)
bar = np.maximum(8 * port, 4e-6 * np.maximum(1, np.abs(ref)))
res["float"] = {"values": nn, "seed": 7, "item": "a.wav", "device_max_abs_err": float(err.max()), "float32_port_max_abs_err": port,
                "ratio_device_over_port": float(err.max() / port), "worst_err_over_bar": float(np.max(err / bar)),
                "bar": "max(8 x port error, 4e-6 max(1, |ref|))"}
print(res["float"], flush=True)

# B. cost
B, N = 16, 16000
out = torch.zeros((B, N), device=dev)
keys = torch.as_tensor(np.array([[7, 100 + b] for b in range(B)], dtype=np.uint64).view(np.int64)).to(dev)
counts = torch.full((B,), N, dtype=torch.int32, device=dev)

def timed(fn, warm=50, reps=500):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # microseconds

res["cost_us"] = {"shape": [B, N], "warmup": 50, "timed": 500,
                  "mbxn_fill_normal": timed(lambda: fill(out, keys, counts, N)),
                  "torch_randn": timed(lambda: torch.randn((B, N), device=dev, dtype=torch.float32))}
model = os.path.join(OUT, "_model_speech")
create_synthetic_model_dir(model, "SPEECH")
inv = MELInverter(model)
eng = inv.model
res["cost_us"]["engine_keyed_noise_with_upload"] = timed(lambda: eng.keyed_noise(7, list(range(B)), [N] * B), 10, 100)
mel = torch.as_tensor(np.random.default_rng(0).normal(-5, 2, size=(B, 800, 80)).astype(np.float32)).to(dev)
nz = eng.keyed_noise(7, list(range(B)), [N] * B)
res["cost_us"]["forward_16x10s"] = timed(lambda: eng.forward(mel, noise=nz), 3, 10)
res["cost_us"]["fill_over_forward"] = res["cost_us"]["mbxn_fill_normal"] / res["cost_us"]["forward_16x10s"]
print(res["cost_us"], flush=True)
del inv, eng, mel, nz
torch.cuda.empty_cache()

# C. throughput: 64 synthetic 10 s files
from scipy.io import wavfile
snd_dir = os.path.join(OUT, "_sounds")
os.makedirs(snd_dir, exist_ok=True)
files = []
for ii in range(64):
    rng = np.random.default_rng(ii)
    tt = np.arange(240000) / 24000.0
    xx = (0.3 * np.sin(2 * np.pi * (120 + ii) * tt) + 0.05 * rng.normal(size=tt.size)).astype(np.float32)
    files.append(os.path.join(snd_dir, f"utt{ii:02d}.wav"))
    wavfile.write(files[-1], 24000, xx)
tool = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin", "transform_audio.py")
t0 = time.perf_counter()
run = subprocess.run([sys.executable, tool, *files, "-o", os.path.join(OUT, "_syn"), "--model_id", model, "--batch", "16",
                      "--transposition", "1.25", "--noise-seed", "7", "-v", "-q", "-nt", "4"], capture_output=True, text=True, timeout=400)
wall = time.perf_counter() - t0
summary = [ll for ll in run.stderr.splitlines() if ll.startswith("transform_audio:")]
res["throughput"] = {"files": 64, "seconds_each": 10, "batch": 16, "threads": 4, "rc": run.returncode, "process_wall_s": wall,
                     "summary": summary[-1] if summary else run.stderr[-1500:]}
print(res["throughput"], flush=True)
if run.returncode == 0:
    live_tool = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin", "stream_transpose.py")
    t0 = time.perf_counter()
    rcs = []
    for ff in files[:4]:
        rr = subprocess.run([sys.executable, live_tool, ff, "-o", os.path.join(OUT, "_live", os.path.basename(ff)), "--model_id", model,
                             "--transposition", "1.25", "--noise-seed", "7", "-q"], capture_output=True, text=True, timeout=300)
        rcs.append(rr.returncode)
        if rr.returncode:
            print(rr.stderr[-1500:])
            break
    res["stream_transpose_4_files"] = {"rc": rcs, "wall_s": time.perf_counter() - t0}
    print(res["stream_transpose_4_files"], flush=True)
shutil.rmtree(OUT, ignore_errors=True)
with open(RESULT, "w") as fo:
    json.dump(res, fo, indent=1)

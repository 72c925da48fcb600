#!/usr/bin/env python3
"""What the F0 tracker costs on the device: one batch of 16 x 10 s of sound at 24 kHz, tracked by
mbxp_track_f0 on the frame grid of the mel analysis (hop 300, the defaults of f0track.params: window 1024, lags 24 .. 437)
next to mbx_mel_analysis on the same buffers in the same process, for scale.

The calls go through the library on preallocated buffers, alternating, each between two HIP events on the stream it runs on;
after a warm-up of both, the timed calls give the percentiles of the device time of a whole call.  Before anything is timed
some frames of the tracker's output are compared with the host definition bit for bit, so that the timed code is the code
that is right.  The cost model (terms, float operations, LDS bytes, and the two floors they give at the rates of the
micro-architecture notes) is computed from the shapes and printed with the times.  ``--lib PATH`` times another build of the
library (one process per build: run the script once per build, alternating, to compare two).  Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile

import numpy as np

# per compute unit and clock: four-byte LDS reads of a wave move 128 B; 4 SIMDs of 32 lanes make 128 float operations
LDS_B32_BYTES_PER_CLK_CU, VALU_OPS_PER_CLK_CU, CUS, CLOCK_HZ = 128, 128, 256, 2.4e9


def percentiles(values):
    return {"p50": float(np.percentile(values, 50)), "p10": float(np.percentile(values, 10)),
            "p90": float(np.percentile(values, 90)), "n": len(values)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--warmup", type=int, default=30, help="untimed calls of each leg")
    ap.add_argument("--iters", type=int, default=200, help="timed calls of each leg")
    ap.add_argument("--lib", default=None, help="time this build of the library instead of the tree's")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("f0_track_probe.py: no GPU available; a timing taken without one says nothing")
    from mbexwn_vocoder_amd import f0track, timemap
    from mbexwn_vocoder_amd.analysis import mel_analysis_tables
    from mbexwn_vocoder_amd.config import read_config
    from mbexwn_vocoder_amd.abi import _check, load_library
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    with tempfile.TemporaryDirectory() as tmp:
        cfg = read_config(config_file=os.path.join(create_synthetic_model_dir(os.path.join(tmp, "speech"), "SPEECH"),
                                                   "config.yaml"))["preprocess_config"]
    rate, hop, fft_size, n_mels = int(cfg["sample_rate"]), int(cfg["hop_size"]), int(cfg["fft_size"]), int(cfg["mel_channels"])
    win = int(cfg.get("win_size", fft_size))
    prm = f0track.params(rate)
    dev = torch.device("cuda", torch.cuda.current_device())
    B, N = args.items, int(round(args.seconds * rate))
    rng = np.random.default_rng(0)
    tt = np.arange(N) / rate
    host = np.stack([sum((0.3 / h) * np.sin(2 * np.pi * (110.0 + 7 * bb) * h * tt) for h in range(1, 6))
                     + 0.01 * rng.standard_normal(N) for bb in range(B)]).astype(np.float32)
    sound = torch.as_tensor(host).to(dev)
    n_dev = torch.full((B,), N, dtype=torch.int32, device=dev)
    tables = [torch.as_tensor(np.ascontiguousarray(tb)).to(dev) for tb in mel_analysis_tables(cfg)]
    eps = ctypes.c_float(float(np.finfo(np.float32).eps))
    lib = load_library()
    tracker = lib.mbxp_track_f0
    if args.lib:
        other = ctypes.CDLL(os.path.abspath(args.lib))
        tracker = other.mbxp_track_f0
        tracker.restype, tracker.argtypes = lib.mbxp_track_f0.restype, lib.mbxp_track_f0.argtypes
    stream = torch.cuda.current_stream(dev)
    cc = timemap.centres(N, hop, rate, None)
    frames = int(cc.size)
    c_dev = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(cc, (B, frames)))).to(dev)
    k_dev = torch.full((B,), frames, dtype=torch.int32, device=dev)
    mel = torch.zeros((B, frames, n_mels), dtype=torch.float32, device=dev)
    f0 = torch.zeros((B, frames), dtype=torch.float32, device=dev)
    per = torch.zeros((B, frames), dtype=torch.float32, device=dev)

    def analysis():
        _check(lib.mbx_mel_analysis(sound.data_ptr(), n_dev.data_ptr(), B, N, win, hop, fft_size, n_mels, tables[0].data_ptr(),
                                    tables[1].data_ptr(), tables[2].data_ptr(), tables[3].data_ptr(), tables[4].data_ptr(), eps,
                                    mel.data_ptr(), frames, stream.cuda_stream))

    def track():
        status = tracker(sound.data_ptr(), N, B, n_dev.data_ptr(), c_dev.data_ptr(), k_dev.data_ptr(), frames, rate,
                         prm["window"], prm["tau_min"], prm["tau_max"], ctypes.c_float(prm["threshold"]),
                         ctypes.c_float(prm["e_min"]), f0.data_ptr(), per.data_ptr(), stream.cuda_stream)
        if status != 0:
            raise RuntimeError(f"mbxp_track_f0 returned {status}")

    terms = B * frames * prm["window"] * prm["tau_max"]
    model = {"frames": B * frames, "terms": terms, "float_ops": 3 * terms, "lds_bytes_two_reads_per_term": 8 * terms,
             "lds_bytes_shared_first_window": 6 * terms}
    model["alu_floor_ms"] = 1e3 * model["float_ops"] / (VALU_OPS_PER_CLK_CU * CUS * CLOCK_HZ)
    model["lds_floor_ms_two_reads"] = 1e3 * model["lds_bytes_two_reads_per_term"] / (LDS_B32_BYTES_PER_CLK_CU * CUS * CLOCK_HZ)
    model["lds_floor_ms_shared"] = 1e3 * model["lds_bytes_shared_first_window"] / (LDS_B32_BYTES_PER_CLK_CU * CUS * CLOCK_HZ)
    result = {"device": torch.cuda.get_device_name(0), "library": args.lib or "tree", "items": B, "seconds": N / rate,
              "params": prm, "frames_per_item": frames, "cost_model": model, "warmup": args.warmup, "iters": args.iters}
    legs = [("mbx_mel_analysis", analysis), ("mbxp_track_f0", track)]
    with torch.cuda.device(dev):
        for _, fn in legs:
            fn()
        torch.cuda.synchronize()
        some = np.array([0, 1, 2, frames // 2, frames - 2, frames - 1])
        want = f0track.track_f0_host(host[B - 1], cc[some], prm)
        got = (f0[B - 1].cpu().numpy()[some], per[B - 1].cpu().numpy()[some])
        same = all(np.array_equal(gg.view(np.uint32), ww.view(np.uint32)) for gg, ww in zip(got, want))
        assert same, "the tracker's output differs from the host definition"
        result["bit_equal_to_host_on_sampled_frames"] = bool(same)
        result["voiced_share"] = float((f0 > 0).float().mean())
        times = {name: [] for name, _ in legs}
        for it in range(args.warmup + args.iters):
            for name, fn in legs:                            # alternating: both see the same state of the machine
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record(stream)
                fn()
                ev1.record(stream)
                ev1.synchronize()
                if it >= args.warmup:
                    times[name].append(ev0.elapsed_time(ev1))
        result["call_ms_device"] = {name: percentiles(vals) for name, vals in times.items()}
    print(json.dumps(result))


if __name__ == "__main__":
    main()

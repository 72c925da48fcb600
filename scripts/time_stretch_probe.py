#!/usr/bin/env python3
"""What the mel analysis at arbitrary frame positions costs on the device: one batch of 16 x 10 s of
sound at the canonical analysis geometry (1200 / 300 / 2048 / 80 at 24 kHz), analysed by mbx_mel_analysis (frames on
multiples of the hop) and by mbxw_mel_frames_at (frames where a table says) on the same buffers in the same process.

The calls go through the library on preallocated buffers, alternating -- the regular analysis, the new call with regular
centres (factor 1: the same grid and the same frame body), and the new call at factor 2 and factor 0.5 --, each between two
HIP events on the stream it runs on; after a warm-up of all of them, the timed calls give the percentiles of the device time
of a whole call.  Before anything is timed the factor-1 output is compared with the regular analysis bit for bit, so that the
timed code is the code that is right.  Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile

import numpy as np


def percentiles(values):
    return {"p50": float(np.percentile(values, 50)), "p10": float(np.percentile(values, 10)),
            "p90": float(np.percentile(values, 90)), "n": len(values)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--warmup", type=int, default=50, help="untimed calls of each leg")
    ap.add_argument("--iters", type=int, default=500, help="timed calls of each leg")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_stretch_probe.py: no GPU available; a timing taken without one says nothing")
    from mbexwn_vocoder_amd import timemap
    from mbexwn_vocoder_amd.analysis import mel_analysis_tables
    from mbexwn_vocoder_amd.config import read_config
    from mbexwn_vocoder_amd.abi import _check, load_library
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    with tempfile.TemporaryDirectory() as tmp:
        cfg = read_config(config_file=os.path.join(create_synthetic_model_dir(os.path.join(tmp, "speech"), "SPEECH"),
                                                   "config.yaml"))["preprocess_config"]
    rate, hop, fft_size, n_mels = int(cfg["sample_rate"]), int(cfg["hop_size"]), int(cfg["fft_size"]), int(cfg["mel_channels"])
    win = int(cfg.get("win_size", fft_size))
    dev = torch.device("cuda", torch.cuda.current_device())
    B, N = args.items, int(round(args.seconds * rate))
    rng = np.random.default_rng(0)
    tt = np.arange(N) / rate
    sound = np.stack([0.3 * np.sin(2 * np.pi * (110.0 + 7 * bb) * tt) + 0.05 * rng.standard_normal(N) for bb in range(B)])
    sound = torch.as_tensor(sound.astype(np.float32)).to(dev)
    n_dev = torch.full((B,), N, dtype=torch.int32, device=dev)
    tables = [torch.as_tensor(np.ascontiguousarray(tb)).to(dev) for tb in mel_analysis_tables(cfg)]
    eps = ctypes.c_float(float(np.finfo(np.float32).eps))
    lib = load_library()
    stream = torch.cuda.current_stream(dev)

    legs, outs = [], {}
    frames = N // hop + 1
    outs["mbx_mel_analysis"] = torch.zeros((B, frames, n_mels), dtype=torch.float32, device=dev)

    def regular(out=outs["mbx_mel_analysis"]):
        _check(lib.mbx_mel_analysis(sound.data_ptr(), n_dev.data_ptr(), B, N, win, hop, fft_size, n_mels, tables[0].data_ptr(),
                                    tables[1].data_ptr(), tables[2].data_ptr(), tables[3].data_ptr(), tables[4].data_ptr(), eps,
                                    out.data_ptr(), frames, stream.cuda_stream))
    legs.append(("mbx_mel_analysis", regular))
    counts = {"mbx_mel_analysis": frames}
    for factor in (1.0, 2.0, 0.5):
        cc = timemap.centres(N, hop, rate, factor)
        name = f"mbxw_mel_frames_at_factor_{factor:g}"
        counts[name] = int(cc.size)
        c_dev = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(cc, (B, cc.size)))).to(dev)
        k_dev = torch.full((B,), cc.size, dtype=torch.int32, device=dev)
        outs[name] = torch.zeros((B, cc.size, n_mels), dtype=torch.float32, device=dev)

        def warped(c_dev=c_dev, k_dev=k_dev, out=outs[name], frames=int(cc.size)):
            _check(lib.mbxw_mel_frames_at(sound.data_ptr(), N, B, n_dev.data_ptr(), c_dev.data_ptr(), k_dev.data_ptr(), frames,
                                          win, fft_size, n_mels, tables[0].data_ptr(), tables[1].data_ptr(), tables[2].data_ptr(),
                                          tables[3].data_ptr(), tables[4].data_ptr(), eps, out.data_ptr(), stream.cuda_stream))
        legs.append((name, warped))

    result = {"device": torch.cuda.get_device_name(0), "items": B, "seconds": N / rate, "geometry": [win, hop, fft_size, n_mels],
              "frames_per_item": counts, "warmup": args.warmup, "iters": args.iters}
    with torch.cuda.device(dev):
        for _, fn in legs:
            fn()
        torch.cuda.synchronize()
        same = torch.equal(outs["mbx_mel_analysis"].view(torch.int32), outs["mbxw_mel_frames_at_factor_1"].view(torch.int32))
        assert same, "factor 1 differs from the regular analysis"
        assert torch.equal(outs["mbxw_mel_frames_at_factor_2"][:, ::2].contiguous().view(torch.int32), outs["mbx_mel_analysis"].view(torch.int32))
        result["factor_1_bit_equal"] = bool(same)
        times = {name: [] for name, _ in legs}
        for it in range(args.warmup + args.iters):
            for name, fn in legs:                            # alternating: all see the same state of the machine
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

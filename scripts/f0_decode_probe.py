#!/usr/bin/env python3
"""What decoding the F0 contour costs on the device: the batch of f0_track_probe.py -- 16 x 10 s of
sound at 24 kHz, 801 frames each on the grid of the mel analysis, the defaults of f0track.params and f0decode.decode_params
-- through mbxc_f0_candidates and mbxc_decode_f0, next to mbxp_track_f0 on the same buffers in the same process as the
yardstick.

The calls go through the library on preallocated buffers, alternating, each between two HIP events on the stream it runs on;
after a warm-up of all three, the timed calls give the percentiles of the device time of a whole call.  Before anything is
timed, sampled frames of the candidate tables and the whole decoded contour of one item are compared with the host definition
bit for bit, so that the timed code is the code that is right.  The decode kernel is a chain of dependent steps, one per
frame, on one wave per item: its time is printed beside cycles per step x steps at the clock of the micro-architecture
notes, forward pass and walk back together.  Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

CLOCK_HZ = 2.4e9


def percentiles(values):
    return {"p50": float(np.percentile(values, 50)), "p10": float(np.percentile(values, 10)),
            "p90": float(np.percentile(values, 90)), "n": len(values)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--warmup", type=int, default=30, help="untimed calls of each leg")
    ap.add_argument("--iters", type=int, default=200, help="timed calls of each leg")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("f0_decode_probe.py: no GPU available; a timing taken without one says nothing")
    from mbexwn_vocoder_amd import f0decode, f0track, timemap
    from mbexwn_vocoder_amd.abi import _check, load_library
    rate, hop = 24000, 300
    prm, dec = f0track.params(rate), f0decode.decode_params()
    dev = torch.device("cuda", torch.cuda.current_device())
    B, N = args.items, int(round(args.seconds * rate))
    rng = np.random.default_rng(0)
    tt = np.arange(N) / rate
    host = np.stack([sum((0.3 / h) * np.sin(2 * np.pi * (110.0 + 7 * bb) * h * tt) for h in range(1, 6))
                     + 0.01 * rng.standard_normal(N) for bb in range(B)]).astype(np.float32)
    sound = torch.as_tensor(host).to(dev)
    n_dev = torch.full((B,), N, dtype=torch.int32, device=dev)
    lib = load_library()
    stream = torch.cuda.current_stream(dev)
    cc = timemap.centres(N, hop, rate, None)
    frames = int(cc.size)
    c_dev = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(cc, (B, frames)))).to(dev)
    k_dev = torch.full((B,), frames, dtype=torch.int32, device=dev)
    f0 = torch.zeros((B, frames), dtype=torch.float32, device=dev)
    per = torch.zeros((B, frames), dtype=torch.float32, device=dev)
    f0_v, per_v = torch.zeros_like(f0), torch.zeros_like(per)
    tabs = [torch.zeros((B, frames, 8), dtype=torch.float32, device=dev) for _ in range(3)]
    th = np.ascontiguousarray(dec["thresholds"], np.float32)
    ww = np.ascontiguousarray(dec["weights"], np.float32)
    fpp = ctypes.POINTER(ctypes.c_float)

    def track():
        _check(lib.mbxp_track_f0(sound.data_ptr(), N, B, n_dev.data_ptr(), c_dev.data_ptr(), k_dev.data_ptr(), frames, rate,
                                 prm["window"], prm["tau_min"], prm["tau_max"], ctypes.c_float(prm["threshold"]),
                                 ctypes.c_float(prm["e_min"]), f0.data_ptr(), per.data_ptr(), stream.cuda_stream))

    def candidates():
        _check(lib.mbxc_f0_candidates(sound.data_ptr(), N, B, n_dev.data_ptr(), c_dev.data_ptr(), k_dev.data_ptr(), frames, rate,
                                      prm["window"], prm["tau_min"], prm["tau_max"], ctypes.c_float(prm["e_min"]),
                                      th.ctypes.data_as(fpp), ww.ctypes.data_as(fpp), int(th.size), dec["n_cand"],
                                      tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), stream.cuda_stream))

    def decode():
        _check(lib.mbxc_decode_f0(tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), k_dev.data_ptr(), frames, B, rate,
                                  ctypes.c_float(dec["w_jump"]), ctypes.c_float(dec["w_switch"]), f0_v.data_ptr(), per_v.data_ptr(),
                                  stream.cuda_stream))

    result = {"device": torch.cuda.get_device_name(0), "items": B, "seconds": N / rate, "params": prm,
              "decode": {kk: (vv.tolist() if hasattr(vv, "tolist") else vv) for kk, vv in dec.items()},
              "frames_per_item": frames, "frames": B * frames, "warmup": args.warmup, "iters": args.iters}
    legs = [("mbxp_track_f0", track), ("mbxc_f0_candidates", candidates), ("mbxc_decode_f0", decode)]
    with torch.cuda.device(dev):
        for _, fn in legs:
            fn()
        torch.cuda.synchronize()
        some = np.array([0, 1, 2, frames // 2, frames - 2, frames - 1])
        halves = f0track.difference_host(host[B - 1], cc[some], prm)
        want = f0decode.candidates_host(*halves, prm, dec)
        got = [tb[B - 1].cpu().numpy() for tb in tabs]
        same = all(np.array_equal(gg[some].view(np.uint32), wt.view(np.uint32)) for gg, wt in zip(got, want))
        assert same, "the candidate tables differ from the host definition"
        want = f0decode.viterbi_host(*got, rate, dec)
        same = all(np.array_equal(gg[B - 1].cpu().numpy().view(np.uint32), wt.view(np.uint32)) for gg, wt in zip((f0_v, per_v), want))
        assert same, "the decoded contour differs from the host definition"
        result["bit_equal_to_host"] = {"candidate_frames_sampled": int(some.size), "decoded_frames": frames}
        result["voiced_share"] = {"greedy": float((f0 > 0).float().mean()), "viterbi": float((f0_v > 0).float().mean())}
        result["candidates_per_frame_mean"] = float((tabs[0][:, :, :7] > 0).float().sum(dim=2).mean())
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
    ms = result["call_ms_device"]
    result["candidates_over_tracker_p50"] = ms["mbxc_f0_candidates"]["p50"] / ms["mbxp_track_f0"]["p50"]
    # the chain: `frames` forward steps and as many steps of the walk back, on one wave per item, the items side by side
    result["decode_cycles_per_frame_at_2p4_ghz"] = ms["mbxc_decode_f0"]["p50"] * 1e-3 * CLOCK_HZ / frames
    print(json.dumps(result))


if __name__ == "__main__":
    main()

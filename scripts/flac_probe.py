#!/usr/bin/env python3
"""What compressing the FLAC output costs on the device ("Compressed FLAC"): one batch of 16 x 10 s of audio
synthesised by the canonical SPEECH geometry, encoded by mbx_encode_flac16 (VERBATIM frames) and by
mbxf_encode_flac16_fixed (fixed predictors and Rice codes) on the same buffers in the same process.

The two encoders are called through the library on preallocated buffers, alternating, each call between two HIP events on
the stream it runs on; after a warm-up of both, the timed calls give the percentiles of the device time of a whole call (for
the compressing encoder: the memset of max_abs, the plan launch, the scan launch and the encode launch).  The time of each of
its three kernels comes from a run of its own under ``rocprofv3 --kernel-trace --stats`` with ``--only fixed`` (the kernels
are flac_fixed_plan_kernel, flac_fixed_scan_kernel and flac_fixed_encode_kernel).

The byte ratio is the packed total over the VERBATIM frames' bytes, on the synthesised batch and, next to it, on a batch of a
39-harmonic 120 Hz tone under a little noise: the weights of the synthetic model are random, so that its audio is closer to
noise than speech is.  Prints one JSON line.
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
    ap.add_argument("--warmup", type=int, default=50, help="untimed calls of each encoder")
    ap.add_argument("--iters", type=int, default=500, help="timed calls of each encoder")
    ap.add_argument("--only", choices=["both", "fixed", "verbatim"], default="both", help="for a run under a profiler")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("flac_probe.py: no GPU available; a timing taken without one says nothing")
    from mbexwn_vocoder_amd import flac
    from mbexwn_vocoder_amd.abi import _check
    from mbexwn_vocoder_amd.mel_inverter import MELInverter, create_synthetic_model_dir
    with tempfile.TemporaryDirectory() as tmp:
        inv = MELInverter(create_synthetic_model_dir(os.path.join(tmp, "speech"), "SPEECH"))
    eng, dims = inv.model, inv.model.dims
    rate = int(dims.sample_rate)
    frames = int(round(args.seconds * rate / dims.hop_size))
    rng = np.random.default_rng(0)
    mel = np.clip(np.log(np.exp(rng.normal(-5.0, 2.0, size=(args.items, frames, dims.mel_channels))) + 1e-5), -11.5, 2.0)
    torch.manual_seed(0)
    noise = (torch.randn((args.items, frames * dims.wn_in_rows_per_frame), dtype=torch.float32, device=eng.device)
             if dims.noise_sigma else None)
    audio = eng.forward(torch.as_tensor(mel.astype(np.float32), device=eng.device), noise=noise).contiguous()
    B, stride = int(audio.shape[0]), int(audio.shape[1])
    counts = [stride] * B
    tt = np.arange(stride) / rate
    tone = sum(np.sin(2 * np.pi * 120 * kk * tt) / kk for kk in range(1, 40))
    tone = 0.5 * tone / np.max(np.abs(tone))
    tones = np.stack([tone + 0.002 * rng.standard_normal(stride) for _ in range(B)]).astype(np.float32)

    n_frames = sum(-(-nn // flac.BLOCK) for nn in counts)
    capacity = sum(flac.frames_bytes(nn) for nn in counts)
    tables = torch.as_tensor(flac.crc16_device_tables().view(np.int16)).to(eng.device)
    out = torch.empty(capacity, dtype=torch.uint8, device=eng.device)
    lengths = torch.empty(n_frames, dtype=torch.int32, device=eng.device)
    work = torch.empty(3 * n_frames + 1, dtype=torch.int64, device=eng.device)
    pcm = torch.empty((B, stride), dtype=torch.int16, device=eng.device)
    peak = torch.empty(B, dtype=torch.float32, device=eng.device)
    counts_c = (ctypes.c_int64 * B)(*counts)
    lib = eng._lib

    def verbatim(src):
        _check(lib.mbx_encode_flac16(src.data_ptr(), stride, B, counts_c, rate, tables.data_ptr(), out.data_ptr(), capacity,
                                     peak.data_ptr(), eng._stream()))

    def fixed(src):
        _check(lib.mbxf_encode_flac16_fixed(src.data_ptr(), stride, B, counts_c, rate, tables.data_ptr(), out.data_ptr(), capacity,
                                            lengths.data_ptr(), work.data_ptr(), pcm.data_ptr(), peak.data_ptr(), eng._stream()))

    result = {"device": torch.cuda.get_device_name(0), "items": B, "seconds": stride / rate, "frames": n_frames,
              "verbatim_bytes": capacity, "warmup": args.warmup, "iters": args.iters}
    with torch.cuda.device(eng.device):
        stream = torch.cuda.current_stream(eng.device)
        ratios = {}
        for name, src in (("synthesised", audio), ("harmonic_tone", torch.as_tensor(tones, device=eng.device))):
            fixed(src)
            torch.cuda.synchronize()
            used = int(lengths.cpu().numpy().astype(np.int64).sum())
            assert used == int(work[n_frames].item())
            ratios[name] = used / capacity
        result["compressed_share_of_verbatim_bytes"] = ratios
        # one item checked against the host writer, so that the timed code is the code that is right
        fixed(audio)
        torch.cuda.synchronize()
        first = lengths[:-(-stride // flac.BLOCK)].cpu().numpy().astype(np.int64)
        want = flac.fixed_frames(flac.to_pcm16(audio[0].cpu().numpy()), rate)
        assert out[:int(first.sum())].cpu().numpy().tobytes() == b"".join(want), "device frames differ from the host writer's"

        legs = [("verbatim", verbatim), ("fixed", fixed)] if args.only == "both" else [(args.only, dict(verbatim=verbatim, fixed=fixed)[args.only])]
        times = {name: [] for name, _ in legs}
        for it in range(args.warmup + args.iters):
            for name, fn in legs:                            # alternating: both see the same state of the machine
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record(stream)
                fn(audio)
                ev1.record(stream)
                ev1.synchronize()
                if it >= args.warmup:
                    times[name].append(ev0.elapsed_time(ev1))
        result["call_ms_device"] = {name: percentiles(vals) for name, vals in times.items()}
    print(json.dumps(result))


if __name__ == "__main__":
    main()

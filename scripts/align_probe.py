#!/usr/bin/env python3
"""What the timing alignment costs on the device: mbxg_local_cost and mbxg_align_path at a band of
80 frames on 16 items of 10 s (801 frames each side) and on one item of 5 min (24 001 frames), at the canonical analysis
geometry (hop 300 at 24 kHz, 80 mel channels), beside mbx_mel_analysis of the 16 x 10 s batch in the same process.

The source of every item is its guide read along a smooth random warp, plus noise: the paths wander inside the band as they
do for two takes of one line.  The calls go through the library on preallocated buffers, alternating, each between two HIP
events on the stream it runs on; after a warm-up the timed calls give the percentiles of the device time of a whole call.
Before anything is timed the cost table, the nodes, the count and the total of one item of each shape are compared with the
definition (align.py) bit for bit, so that the timed code is the code that is right.  Prints one JSON line.
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
    ap.add_argument("--band", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=20, help="untimed calls of each leg")
    ap.add_argument("--iters", type=int, default=200, help="timed calls of each leg")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("align_probe.py: no GPU available; a timing taken without one says nothing")
    from mbexwn_vocoder_amd import align
    from mbexwn_vocoder_amd.abi import _check, load_library
    from mbexwn_vocoder_amd.analysis import mel_analysis_tables
    from mbexwn_vocoder_amd.config import read_config
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    with tempfile.TemporaryDirectory() as tmp:
        cfg = read_config(config_file=os.path.join(create_synthetic_model_dir(os.path.join(tmp, "speech"), "SPEECH"),
                                                   "config.yaml"))["preprocess_config"]
    rate, hop, fft_size, n_mels = int(cfg["sample_rate"]), int(cfg["hop_size"]), int(cfg["fft_size"]), int(cfg["mel_channels"])
    win = int(cfg.get("win_size", fft_size))
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = load_library()
    stream = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(0)
    band = args.band
    legs, checks = [], {}

    def shape(tag, items, seconds):
        frames = int(round(seconds * rate)) // hop + 1
        guide = (rng.normal(size=(items, frames, n_mels)) * 2.0 - 5.0).astype(np.float32)
        source = np.empty_like(guide)
        for bb in range(items):                                  # a warp of up to half the band, a few seconds per swing
            tt = np.arange(frames)
            pos = tt + 0.5 * band * np.sin(2 * np.pi * tt / (400.0 + 37 * bb)) * np.sin(np.pi * tt / (frames - 1))
            source[bb] = guide[bb][np.clip(np.round(pos).astype(int), 0, frames - 1)]
        source += (rng.normal(size=source.shape) * 0.1).astype(np.float32)
        mel_a, mel_b = torch.as_tensor(guide).to(dev), torch.as_tensor(source).to(dev)
        counts = torch.full((items,), frames, dtype=torch.int32, device=dev)
        cost = torch.zeros((items, frames, 2 * band + 1), dtype=torch.int16, device=dev)
        nbytes = int(lib.mbxg_align_workspace_size(items, frames, band))
        work = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        nodes_i, nodes_j = (torch.zeros((items, frames), dtype=torch.int32, device=dev) for _ in range(2))
        count, total = (torch.zeros((items,), dtype=torch.int32, device=dev) for _ in range(2))

        def local_cost():
            _check(lib.mbxg_local_cost(mel_a.data_ptr(), mel_b.data_ptr(), counts.data_ptr(), counts.data_ptr(), items, frames,
                                       frames, n_mels, band, cost.data_ptr(), stream.cuda_stream))

        def path():
            _check(lib.mbxg_align_path(cost.data_ptr(), counts.data_ptr(), counts.data_ptr(), items, frames, band, work.data_ptr(),
                                       nbytes, nodes_i.data_ptr(), nodes_j.data_ptr(), count.data_ptr(), total.data_ptr(),
                                       stream.cuda_stream))
        # the same table under source lengths that no path can reach: every row of the recursion runs, nothing is walked
        # back -- the share of the row chain in the call
        far = torch.full((items,), min(2 * frames + 50, align.MAX_FRAMES), dtype=torch.int32, device=dev)
        junk_i, junk_j, junk_c, junk_t = (torch.zeros_like(tt) for tt in (nodes_i, nodes_j, count, total))

        def rows_only():
            _check(lib.mbxg_align_path(cost.data_ptr(), counts.data_ptr(), far.data_ptr(), items, frames, band, work.data_ptr(),
                                       nbytes, junk_i.data_ptr(), junk_j.data_ptr(), junk_c.data_ptr(), junk_t.data_ptr(),
                                       stream.cuda_stream))
        legs.extend([(f"mbxg_local_cost_{tag}", local_cost), (f"mbxg_align_path_{tag}", path),
                     (f"mbxg_align_path_{tag}_rows_only", rows_only)])
        local_cost()
        path()
        torch.cuda.synchronize()
        want_cost = align.local_cost_host(guide[0], source[0], band)
        want_nodes, want_total = align.path_host(want_cost, frames, band)
        got_cost = cost[0].cpu().numpy().view(np.uint16)
        nn = int(count[0])
        same = (np.array_equal(got_cost, want_cost) and nn == len(want_nodes) and int(total[0]) == want_total
                and np.array_equal(nodes_i[0, :nn].cpu().numpy(), want_nodes[:, 0])
                and np.array_equal(nodes_j[0, :nn].cpu().numpy(), want_nodes[:, 1]))
        assert same, f"{tag}: the kernels differ from the definition"
        rows_only()
        torch.cuda.synchronize()
        assert int(junk_c.abs().sum()) == 0 and bool((junk_t == -1).all()), f"{tag}: the unreachable lengths found a path"
        checks[tag] = {"frames": frames, "items": items, "nodes_item_0": nn, "bit_equal_to_definition": bool(same),
                       "cost_table_bytes": int(cost.numel() * 2), "workspace_bytes": nbytes}

    with torch.cuda.device(dev):
        shape("16x10s", 16, 10.0)
        shape("1x300s", 1, 300.0)
        # the regular analysis of 16 x 10 s, for scale
        B, N = 16, 10 * rate
        tt = np.arange(N) / rate
        sound = np.stack([0.3 * np.sin(2 * np.pi * (110.0 + 7 * bb) * tt) + 0.05 * rng.standard_normal(N) for bb in range(B)])
        sound = torch.as_tensor(sound.astype(np.float32)).to(dev)
        n_dev = torch.full((B,), N, dtype=torch.int32, device=dev)
        tables = [torch.as_tensor(np.ascontiguousarray(tb)).to(dev) for tb in mel_analysis_tables(cfg)]
        eps = ctypes.c_float(float(np.finfo(np.float32).eps))
        frames = N // hop + 1
        out = torch.zeros((B, frames, n_mels), dtype=torch.float32, device=dev)

        def regular():
            _check(lib.mbx_mel_analysis(sound.data_ptr(), n_dev.data_ptr(), B, N, win, hop, fft_size, n_mels, tables[0].data_ptr(),
                                        tables[1].data_ptr(), tables[2].data_ptr(), tables[3].data_ptr(), tables[4].data_ptr(), eps,
                                        out.data_ptr(), frames, stream.cuda_stream))
        legs.append(("mbx_mel_analysis_16x10s", regular))

        result = {"device": torch.cuda.get_device_name(0), "band_frames": band, "n_mels": n_mels, "shapes": checks,
                  "warmup": args.warmup, "iters": args.iters}
        times = {name: [] for name, _ in legs}
        for it in range(args.warmup + args.iters):
            for name, fn in legs:                                # alternating: all see the same state of the machine
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

#!/usr/bin/env python3
"""What the streaming F0 tracker adds to an analysis tick: 64 streams of the SPEECH analysis at the
80 ms schedule, every stream tracking (mbxl_ring_append + mbxl_mel_frames + mbxt_f0_frames) against none (the first two), by
the analyzer's own ``time_device`` probe: HIP events around the launches of a tick, the upload in front and the copy back
behind them outside.

Two legs in one process, each a fresh StreamingAnalyzer after its own warm-up.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def percentiles(values):
    return {"p50": float(np.percentile(values, 50)), "p10": float(np.percentile(values, 10)),
            "p90": float(np.percentile(values, 90)), "n": len(values)}


def leg(cfg, streams, warm_ticks, ticks, f0_params):
    from mbexwn_vocoder_amd.live import StreamingAnalyzer
    an = StreamingAnalyzer(cfg, slots=streams)
    an.time_device = True
    rate = int(round(cfg["sample_rate"]))
    per_tick = int(round(0.080 * rate))
    rng = np.random.default_rng(99)
    tt = np.arange(50 * per_tick) / rate
    sounds = [(0.3 * np.sin(2 * np.pi * (90.0 + 3 * sid) * tt) + 0.05 * rng.normal(size=tt.size)).astype(np.float32)
              for sid in range(streams)]
    for sid in range(streams):
        an.open(sid, f0_params=f0_params)
    device_ms, frames, pos = [], [], 0
    for tick in range(warm_ticks + ticks):
        for sid in range(streams):                                       # the sounds repeat: the streams never end
            an.push(sid, sounds[sid][pos:pos + per_tick])
        pos = (pos + per_tick) % sounds[0].size
        rows = an.tick()
        if tick >= warm_ticks:
            assert len(rows) == streams and len(an.last_f0) == (streams if f0_params else 0)
            device_ms.append(an.last_tick_device_ms)
            frames.append(sum(mm.shape[0] for mm in rows.values()) / streams)
    return {"launches_ms_device": percentiles(device_ms), "frames_per_stream_and_tick": float(np.mean(frames)),
            "ring_samples": an.ring_samples}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--warm-ticks", type=int, default=100)
    ap.add_argument("--ticks", type=int, default=300, help="timed steady ticks per leg")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("live_pitch_probe.py: no GPU available; a timing taken without one says nothing")
    from mbexwn_vocoder_amd import f0track
    from mbexwn_vocoder_amd.config import canonical_config
    cfg = canonical_config("SPEECH")["preprocess_config"]
    prm = f0track.params(int(round(cfg["sample_rate"])))
    out = {"streams": args.streams, "tick_ms": 80, "device": torch.cuda.get_device_name(0), "f0_params": prm}
    out["none_tracking"] = leg(cfg, args.streams, args.warm_ticks, args.ticks, None)
    out["all_tracking"] = leg(cfg, args.streams, args.warm_ticks, args.ticks, prm)
    out["difference_ms_p50"] = out["all_tracking"]["launches_ms_device"]["p50"] - out["none_tracking"]["launches_ms_device"]["p50"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()

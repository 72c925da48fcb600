#!/usr/bin/env python3
"""What the streaming F0 tracker and the fixed-lag decoder add to an analysis tick (DESIGN.md sections 6j and 6l): 64 streams of
the SPEECH analysis at the 80 ms schedule, every stream tracking (mbxl_ring_append + mbxl_mel_frames + mbxt_f0_frames) and
every stream decoding at ``--lag`` frames (mbxv_f0_candidate_frames + mbxv_decode_f0_frames in place of the last) against none
(the first two), by the analyzer's own ``time_device`` probe: HIP events around the launches of a tick, the upload in front
and the copy back behind them outside.

Three legs in one process, a StreamingAnalyzer each, ALTERNATING tick by tick behind a common warm-up.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def percentiles(values):
    return {"p50": float(np.percentile(values, 50)), "p10": float(np.percentile(values, 10)),
            "p90": float(np.percentile(values, 90)), "n": len(values)}


def legs(cfg, streams, warm_ticks, ticks, kinds):
    """``kinds``: {name: keywords of ``StreamingAnalyzer.open``}; every tick pushes 80 ms to every stream of every leg and
    ticks the legs one after the other."""
    from mbexwn_vocoder_amd.live import StreamingAnalyzer
    rate = int(round(cfg["sample_rate"]))
    per_tick = int(round(0.080 * rate))
    rng = np.random.default_rng(99)
    tt = np.arange(50 * per_tick) / rate
    sounds = [(0.3 * np.sin(2 * np.pi * (90.0 + 3 * sid) * tt) + 0.05 * rng.normal(size=tt.size)).astype(np.float32)
              for sid in range(streams)]
    analyzers = {}
    for name, kw in kinds.items():
        an = analyzers[name] = StreamingAnalyzer(cfg, slots=streams)
        an.time_device = True
        for sid in range(streams):
            an.open(sid, **kw)
    device_ms, frames, decided = ({name: [] for name in kinds} for _ in range(3))
    pos = 0
    for tick in range(warm_ticks + ticks):
        for name, an in analyzers.items():
            for sid in range(streams):                                   # the sounds repeat: the streams never end
                an.push(sid, sounds[sid][pos:pos + per_tick])
            rows = an.tick()
            if tick >= warm_ticks:
                assert len(rows) == streams and len(an.last_f0) == (streams if kinds[name] else 0)
                device_ms[name].append(an.last_tick_device_ms)
                frames[name].append(sum(mm.shape[0] for mm in rows.values()) / streams)
                decided[name].append(sum(pair[0].size for pair in an.last_f0.values()) / streams)
        pos = (pos + per_tick) % sounds[0].size
    return {name: {"launches_ms_device": percentiles(device_ms[name]), "frames_per_stream_and_tick": float(np.mean(frames[name])),
                   "f0_frames_per_stream_and_tick": float(np.mean(decided[name])), "ring_samples": an.ring_samples,
                   "device_allocations": an.device_allocations}
            for name, an in analyzers.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--warm-ticks", type=int, default=100)
    ap.add_argument("--ticks", type=int, default=300, help="timed steady ticks per leg")
    ap.add_argument("--lag", type=int, default=8, help="frames of look-ahead of the decoding leg")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("live_pitch_probe.py: no GPU available; a timing taken without one says nothing")
    from mbexwn_vocoder_amd import f0track
    from mbexwn_vocoder_amd.config import canonical_config
    cfg = canonical_config("SPEECH")["preprocess_config"]
    prm = f0track.params(int(round(cfg["sample_rate"])))
    out = {"streams": args.streams, "tick_ms": 80, "device": torch.cuda.get_device_name(0), "f0_params": prm, "lag": args.lag}
    out.update(legs(cfg, args.streams, args.warm_ticks, args.ticks,
                    {"none_tracking": {}, "all_tracking": {"f0_params": prm}, "all_decoding": {"f0_params": prm, "f0_lag": args.lag}}))
    none = out["none_tracking"]["launches_ms_device"]["p50"]
    out["difference_ms_p50"] = out["all_tracking"]["launches_ms_device"]["p50"] - none
    out["decoding_difference_ms_p50"] = out["all_decoding"]["launches_ms_device"]["p50"] - none
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What taking the pitch from the audio costs a file-to-file job: 16 sound files of 10 s at 24 kHz
through ``batched.run_audio_job`` -- the job of transform_audio.py -- on the synthetic canonical SPEECH model, with
``f0_source="net"`` and with ``f0_source="audio"``, stage by stage (the job's ``timings``: what its verbose line reports;
device stages between HIP events, host stages by the host clock).

One process: after one untimed job per source the two sources alternate ``--rounds`` times on the same files; the line gives
every round and the median per stage.  Prints one JSON line.

``--compare decode``: both legs take the pitch from the audio, one with the greedy pick of every frame
and one with the contour decoded over the file (``f0_decode=f0decode.decode_params()``), alternating in the same way.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--compare", default="source", choices=["source", "decode"],
                    help="source: f0_source net against audio; decode: audio with the greedy pick against the decoded contour")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("f0_source_probe.py: no GPU available; a timing taken without one says nothing")
    from scipy.io import wavfile
    from mbexwn_vocoder_amd import f0decode
    from mbexwn_vocoder_amd.batched import run_audio_job
    from mbexwn_vocoder_amd.mel_inverter import MELInverter, create_synthetic_model_dir
    rate, n = 24000, int(round(args.seconds * 24000))
    rng = np.random.default_rng(0)
    tt = np.arange(n) / rate
    with tempfile.TemporaryDirectory() as tmp:
        inv = MELInverter(create_synthetic_model_dir(os.path.join(tmp, "speech"), "SPEECH"))
        files = []
        for ii in range(args.files):
            snd = sum((0.3 / h) * np.sin(2 * np.pi * (110.0 + 7 * ii) * h * tt) for h in range(1, 6)) + 0.01 * rng.standard_normal(n)
            files.append(os.path.join(tmp, f"voice{ii:02d}.wav"))
            wavfile.write(files[-1], rate, snd.astype(np.float32))

        if args.compare == "source":
            legs = {"net": {"f0_source": "net"}, "audio": {"f0_source": "audio"}}
        else:
            legs = {"greedy": {"f0_source": "audio"}, "viterbi": {"f0_source": "audio", "f0_decode": f0decode.decode_params()}}

        def job(leg, tag):
            out = os.path.join(tmp, tag)
            os.makedirs(out, exist_ok=True)
            timings = {}
            skipped = run_audio_job(inv, files, out, "flac", noise_seed=0, batch=args.files, quiet=True, timings=timings, **legs[leg])
            assert skipped == []
            return {kk: float(vv) for kk, vv in sorted(timings.items())}

        for source in legs:
            job(source, "warm_" + source)
        rounds = {leg: [] for leg in legs}
        for rr in range(args.rounds):
            for source in legs:
                rounds[source].append(job(source, f"{source}_{rr}"))
    median = {source: {kk: float(np.median([rr[kk] for rr in rows])) for kk in rows[0]} for source, rows in rounds.items()}
    print(json.dumps({"device": torch.cuda.get_device_name(0), "files": args.files, "seconds": args.seconds, "unit": "s", "compare": args.compare,
                      "median": median, "rounds": rounds}))


if __name__ == "__main__":
    main()

"""Gate-kernel time per launch for the F(4,3) block shapes at several launch sizes (tune_gate_shape: 2 and 3 pin the shape
of launches below 4 x 768 full blocks, 1 and 4 the 256-row blocks of one column tile and of two column tiles at every launch
size).  Run on the GPU box:
    python scripts/experiments/gate_shapes.py                 every shape, one reading per size
    python scripts/experiments/gate_shapes.py --ab 1 4 -n 3   shapes 1 and 4 alternating in one process, n readings per size
                                                              at 1 / 2 / 4 / 8 / 16 x 800 frames, with their spread"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

SIZES = [(1, 80), (1, 160), (1, 240), (1, 320), (1, 400), (1, 480), (1, 560), (1, 640), (1, 800), (1, 1200), (2, 800), (4, 800), (8, 800),
         (16, 800)]
AB_SIZES = [(1, 800), (2, 800), (4, 800), (8, 800), (16, 800)]


def gate_us(eng, mel, noise, warmup=3, steps=10):
    """Mean time of one gate launch (layers behind the folded first one) from the HIP events of profile_read("gate")."""
    import torch
    for _ in range(warmup):
        eng.forward(mel, noise=noise)
    eng.profile_enable(True)
    for _ in range(steps):
        eng.forward(mel, noise=noise)
    torch.cuda.synchronize()
    ms, cnt = eng.profile_read("gate")
    eng.profile_enable(False)
    return ms / cnt * 1e3


def batch_of(dims, batch, frames):
    import torch
    rng = np.random.default_rng(1)
    mel_h, noise_h = bench.synthetic_batch(rng, batch, frames, dims.steps_per_frame)
    return torch.as_tensor(mel_h).cuda(), torch.as_tensor(noise_h).cuda()


def sweep():
    for shape in (1, 2, 3, 4, 0):         # 256-row, product-split, product-split half column tiles, two column tiles, the launch-size rule
        bench._ENGINES.clear()
        cfg, raw, wt, dims, eng = bench.build_engine("SPEECH", None, tune={"gate_shape": shape})
        row = []
        for batch, frames in SIZES:
            mel, noise = batch_of(dims, batch, frames)
            us = gate_us(eng, mel, noise)
            chans = max(eng.kernel_report()["gate_block_channels"])
            row.append(f"{batch}x{frames}: {us:7.1f} us ({eng.gate_form(batch, frames)[13:] or 'f43'}/{chans})")
        print(f"tune_gate_shape={shape}  " + "  ".join(row), flush=True)
        eng.close()


def ab(shapes, n):
    engines = []
    for shape in shapes:
        bench._ENGINES.clear()
        cfg, raw, wt, dims, eng = bench.build_engine("SPEECH", None, tune={"gate_shape": shape})
        engines.append(eng)
    for batch, frames in AB_SIZES:
        mel, noise = batch_of(dims, batch, frames)
        reads = [[] for _ in shapes]
        for _ in range(n):
            for ii, eng in enumerate(engines):
                reads[ii].append(gate_us(eng, mel, noise))
        parts = []
        for shape, eng, rr in zip(shapes, engines, reads):
            chans = max(eng.kernel_report()["gate_block_channels"])
            parts.append(f"shape {shape} ({chans} ch): " + " ".join(f"{v:7.1f}" for v in rr) + f"  mean {np.mean(rr):7.1f} spread {max(rr) - min(rr):5.1f}")
        gain = 1.0 - np.mean(reads[1]) / np.mean(reads[0])
        print(f"{batch}x{frames} us/launch  " + "  |  ".join(parts) + f"  |  second against first {-100 * gain:+.2f} %", flush=True)
    for eng in engines:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", type=int, nargs=2, metavar=("FIRST", "SECOND"), help="alternate two pinned shapes in one process")
    ap.add_argument("-n", type=int, default=3, help="readings per size and shape (--ab)")
    args = ap.parse_args()
    if args.ab:
        ab(args.ab, args.n)
    else:
        sweep()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the level stage costs on the device: one batch of 16 x 10 s of audio synthesised by the
canonical SPEECH geometry, then measured (mbxl_measure), given its gains (mbxl_gains) and multiplied (mbxl_apply, out of
place), with and without the 4x true peak, next to the forward it follows -- all in the same process.

The three legs alternate, each between two HIP events on the stream it runs on; after a warm-up of all, the timed calls give
the percentiles of the device time of a whole leg.  The level legs go through ``level.measure_device`` / ``gains_device`` /
``apply_device`` as the micro-batches call them (so they include their allocations; nothing is uploaded);
``measure_only`` is mbxl_measure alone, without the true peak.  ``limiter`` is the level stage with the look-ahead limiter
 as ``run_micro_batches`` runs it -- measure, gains without a ceiling, mbxd_limit, measure again -- at
per-item loudness targets ``--limiter-over`` dB above the one at which the static gain would touch the ceiling, and
``limit_only`` is mbxd_limit alone on the same gains (its kernels are limit_kernel and limit_stats_kernel);
``limit_only_heavy`` is the same 12 dB further up, where no tile takes the fast path.  The share of samples limited is reported.  The time of each kernel comes from a run of its own under
``rocprofv3 --kernel-trace --stats`` with ``--only level`` (the kernels are level_hops_kernel, level_peak_kernel,
level_gate_kernel, level_gains_kernel and level_apply_kernel).

``job``: what the event-timed legs cannot see -- whether the stage makes the HOST wait.  ``batched.run_micro_batches`` runs
``--job-batches`` micro-batches of the same shape without and with the stage (a loudness target and a ceiling), alternating;
per run the wall time up to the last batch's end, and per micro-batch the host time the generator takes to enqueue it, next
to the forward's device time: a host that had to wait for the stream in every batch would take a forward's time to enqueue one.

Item 0's measure is checked against the host definition first, so that the timed code is the code that is right.  Prints one
JSON line.
"""
import argparse
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
    ap.add_argument("--warmup", type=int, default=10, help="untimed rounds of every leg")
    ap.add_argument("--iters", type=int, default=50, help="timed rounds of every leg")
    ap.add_argument("--only", choices=["all", "level"], default="all", help="level: without the forward, for a run under a profiler")
    ap.add_argument("--limiter-over", type=float, default=3.0,
                    help="dB of loudness the limiter legs ask for beyond what the static ceiling allows")
    ap.add_argument("--job-batches", type=int, default=6, help="micro-batches of a job run (0: no job runs)")
    ap.add_argument("--job-runs", type=int, default=5, help="timed job runs of each kind, after one untimed")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("level_probe.py: no GPU available; a timing taken without one says nothing")
    from mbexwn_vocoder_amd import level, limiter
    from mbexwn_vocoder_amd.mel_inverter import MELInverter, create_synthetic_model_dir
    with tempfile.TemporaryDirectory() as tmp:
        inv = MELInverter(create_synthetic_model_dir(os.path.join(tmp, "speech"), "SPEECH"))
    eng, dims = inv.model, inv.model.dims
    rate = int(dims.sample_rate)
    frames = int(round(args.seconds * rate / dims.hop_size))
    rng = np.random.default_rng(0)
    mel = np.clip(np.log(np.exp(rng.normal(-5.0, 2.0, size=(args.items, frames, dims.mel_channels))) + 1e-5), -11.5, 2.0)
    mel = torch.as_tensor(mel.astype(np.float32), device=eng.device)
    torch.manual_seed(0)
    noise = (torch.randn((args.items, frames * dims.wn_in_rows_per_frame), dtype=torch.float32, device=eng.device)
             if dims.noise_sigma else None)
    audio = eng.forward(mel, noise=noise).contiguous().clone()
    B, stride = int(audio.shape[0]), int(audio.shape[1])
    counts = [stride] * B
    target, ceiling = level.target_power(-23.0), level.ceiling_linear(-1.0)

    got = level.measure_device(audio, counts, rate, true_peak=True).host()[0]
    want = level.measure_host(audio[0].cpu().numpy(), rate)
    assert got.power == want.power and got.count == want.count and got.sample_peak == want.sample_peak, "device measure differs"
    assert got.true_peak >= got.sample_peak

    def stage(true_peak):
        measure = level.measure_device(audio, counts, rate, true_peak=true_peak)
        gains = level.gains_device(measure, target, ceiling=ceiling, true_peak=true_peak)
        level.apply_device(audio, counts, gains, out=gained)

    gained = torch.empty_like(audio)
    h, hold = limiter.window(rate)
    # per item: the loudness at which its peak touches the ceiling, and --limiter-over dB more
    loud = [level.target_power(mm.lufs - 20.0 * np.log10(float(mm.sample_peak) / ceiling) + args.limiter_over)
            for mm in level.measure_device(audio, counts, rate).host(details=False)]
    loud_gains = level.gains_device(level.measure_device(audio, counts, rate), loud)
    heavy_gains = (loud_gains * 4.0).contiguous()

    def limited_stage():
        measure = level.measure_device(audio, counts, rate)
        gains = level.gains_device(measure, loud)
        out, _ = limiter.limit_device(audio, counts, gains, ceiling, h, hold, out=gained)
        level.measure_device(out, counts, rate)

    item0, stats0 = limiter.limit_device(audio[:1], counts[:1], loud_gains[:1].contiguous(), ceiling, h, hold)
    want0, want_stats = limiter.limit_host(audio[0].cpu().numpy(), loud_gains[0].item(), np.float32(ceiling), h, hold)
    assert np.array_equal(item0.cpu().numpy()[0].view(np.int32), want0.view(np.int32)), "device limiter differs"
    assert list(stats0.cpu().numpy()[0]) == list(want_stats.words())
    legs = [("forward", lambda: eng.forward(mel, noise=noise))] if args.only == "all" else []
    legs += [("level", lambda: stage(False)), ("level_true_peak", lambda: stage(True)),
             ("measure_only", lambda: level.measure_device(audio, counts, rate)), ("limiter", limited_stage),
             ("limit_only", lambda: limiter.limit_device(audio, counts, loud_gains, ceiling, h, hold, out=gained)),
             ("limit_only_heavy", lambda: limiter.limit_device(audio, counts, heavy_gains, ceiling, h, hold, out=gained))]
    result = {"device": torch.cuda.get_device_name(0), "items": B, "seconds": stride / rate, "rate": rate,
              "hops_per_item": stride // level.hop_samples(rate), "lufs_item0": got.lufs, "warmup": args.warmup, "iters": args.iters,
              "limiter": {"over_db": args.limiter_over, "h": h, "hold": hold, "limited_share_item0": want_stats.limited / stride,
                          "clamped_item0": want_stats.clamped, "reduction_db_item0": want_stats.reduction_db}}
    with torch.cuda.device(eng.device):
        stream = torch.cuda.current_stream(eng.device)
        times = {name: [] for name, _ in legs}
        for it in range(args.warmup + args.iters):
            for name, fn in legs:                            # alternating: every leg sees the same state of the machine
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record(stream)
                fn()
                ev1.record(stream)
                ev1.synchronize()
                if it >= args.warmup:
                    times[name].append(ev0.elapsed_time(ev1))
        result["leg_ms_device"] = {name: percentiles(vals) for name, vals in times.items()}
    if args.only == "all" and args.job_batches > 0:
        import time
        from mbexwn_vocoder_amd.batched import run_micro_batches
        from mbexwn_vocoder_amd.mel_inverter import KeyedNoise
        mels = [mel[bb].cpu().numpy() for bb in range(B)] * args.job_batches
        keyed = KeyedNoise(0, list(range(len(mels)))) if dims.noise_sigma else None
        control = level.level_control(-23.0, -1.0)
        limiting = level.level_control(loud * args.job_batches, -1.0, limiter=True)

        def job(ctl):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            enqueue, mark = [], t0
            for sb in run_micro_batches(eng, mels, keyed, max_batch=B, max_padded_frames=B * frames, flac=False,
                                        host_audio=True, level=ctl):
                now = time.perf_counter()
                enqueue.append((now - mark) * 1e3)
                mark = now
                last = sb
            last.wait()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, enqueue

        runs = {"plain": [], "level": [], "limiter": []}
        for it in range(1 + args.job_runs):
            for name, ctl in (("plain", None), ("level", control), ("limiter", limiting)):
                got_ms = job(ctl)
                if it:
                    runs[name].append(got_ms)
        result["job"] = {name: {"batches": args.job_batches, "wall_ms": percentiles([rr[0] for rr in vals]),
                                "host_enqueue_ms_per_batch": percentiles([ee for rr in vals for ee in rr[1][1:]])}
                         for name, vals in runs.items()}
    if "forward" in times:
        step = result["leg_ms_device"]["forward"]["p50"]
        result["share_of_step"] = {name: result["leg_ms_device"][name]["p50"] / step for name in ("level", "level_true_peak", "limiter", "limit_only", "limit_only_heavy")}
    print(json.dumps(result))


if __name__ == "__main__":
    main()

"""Host side of the batched / sharded CLI (mbexwn_vocoder_amd/batched.py): the noise replay gives every item the draw of
the one-at-a-time loop, the padded micro-batch puts it into the item's row, and the parent of a --gpus job plans without
importing torch -- no GPU needed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mbexwn_vocoder_amd.batched import replay_noise, stage_micro_batch
from mbexwn_vocoder_amd.sharding import lpt_partition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 3}


def sequential_draws(frames, rows, seed):
    """What the one-at-a-time loop draws: torch.randn((1, T_i * rows)) once per file, in file order."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn((1, tt * rows), generator=gen)[0] for tt in frames]


def test_noise_replay_gives_every_item_its_sequential_draw():
    import torch
    frames, rows = [7, 3, 12, 1, 9, 5, 12, 2], 20
    want = sequential_draws(frames, rows, 42)
    got = replay_noise(frames, rows, device="cpu", generator=torch.Generator().manual_seed(42))
    assert sorted(got) == list(range(len(frames)))
    assert all(torch.equal(got[ii], want[ii]) for ii in got)
    shards = lpt_partition(frames, 3)
    assert sorted(shards[0]) != list(range(min(shards[0]), max(shards[0]) + 1))      # a rank with non-contiguous files
    for mine in shards:
        got = replay_noise(frames, rows, keep=mine, device="cpu", generator=torch.Generator().manual_seed(42))
        assert sorted(got) == sorted(mine) and all(torch.equal(got[ii], want[ii]) for ii in mine)


def test_micro_batch_rows_hold_the_items_draws():
    import torch
    frames, rows = [5, 11, 2], 20
    rng = np.random.default_rng(0)
    mels = [rng.normal(size=(tt, 80)).astype(np.float32) for tt in frames]
    draws = sequential_draws(frames, rows, 7)
    mel, n_frames, noise = stage_micro_batch(mels, draws, rows, device="cpu")
    assert tuple(mel.shape) == (3, 11, 80) and n_frames.dtype == torch.int32 and n_frames.tolist() == frames
    assert tuple(noise.shape) == (3, 11 * rows)
    for jj, tt in enumerate(frames):
        assert np.array_equal(mel[jj, :tt].numpy(), mels[jj]) and not mel[jj, tt:].any()
        assert torch.equal(noise[jj, :tt * rows], draws[jj]) and not noise[jj, tt * rows:].any()


def mell_dict(frames, seed, hoplen=300):
    rng = np.random.default_rng(seed)
    return {"nfft": 2048, "hoplen": hoplen, "winlen": 1200, "nmels": 80, "sr": 24000, "fmin": 0.0, "fmax": 12000.0,
            "lin_spec_offset": 1e-5, "lin_spec_scale": 1, "log_spec_offset": 0.0, "log_spec_scale": 1, "time_axis": 1,
            "mell": rng.normal(-5, 2, size=(80, frames)).astype(np.float32)}


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    from mbexwn_vocoder_amd.fileio import save_var
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    root = tmp_path_factory.mktemp("job")
    model = create_synthetic_model_dir(str(root / "model"), "SPEECH", **SMALL)
    files = []
    for ii, (frames, hop) in enumerate([(23, 300), (7, 300), (41, 256), (15, 300), (30, 300)]):
        files.append(str(root / f"utt{ii}.mell"))
        save_var(files[-1], mell_dict(frames, ii, hop))
    return model, files


def test_gpus_parent_plans_without_torch(job):
    """The parent of `resynth_mel.py --gpus N` counts the GPUs from the visibility variables and partitions the files by
    their frames after scale_mel (a .mell with another hop is resampled) -- without importing torch."""
    model, files = job
    code = ("import json, sys; sys.path.insert(0, sys.argv[1]);"
            "from mbexwn_vocoder_amd.batched import plan_ranks;"
            "plan = plan_ranks(sys.argv[2], sys.argv[3:], 2);"
            "print(json.dumps({'plan': plan, 'torch': 'torch' in sys.modules}))")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0,1,2", ROCR_VISIBLE_DEVICES="0")
    res = subprocess.run([sys.executable, "-c", code, ROOT, model, *files], env=env, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["torch"] is False
    from mbexwn_vocoder_amd.fileio import load_var
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    inv = MELInverter.host_only(model)
    frames = [int(inv.scale_mel(load_var(ff)).shape[1]) for ff in files]
    assert frames[2] != 41                                   # the resampled one
    assert out["plan"] == {"devices": 1, "frames": frames, "shards": lpt_partition(frames, 2)}


def test_visible_gpu_count_reads_the_visibility_variables(monkeypatch):
    from mbexwn_vocoder_amd.sharding import visible_gpu_count
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0,1,2,3")
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0,1")
    monkeypatch.delenv("CUDA_VISIBLE_DEVICES", raising=False)
    assert visible_gpu_count() == 2
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "")
    assert visible_gpu_count() == 0


@pytest.mark.timeout(300)
def test_gpus_parent_fails_when_a_rank_fails_and_on_a_missing_file(job, tmp_path):
    """Without a GPU every rank exits with an error: the parent must exit non-zero (it polls its children).  A missing
    .mell fails the parent's plan before any rank starts."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gpu_batched_cli.py runs the ranks")
    model, files = job
    cli = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin", "resynth_mel.py")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0,1")
    res = subprocess.run([sys.executable, cli, model, "-i", *files, "-o", str(tmp_path / "a"), "--gpus", "2", "-q"],
                         env=env, capture_output=True, text=True, timeout=280)
    assert res.returncode != 0 and "no GPU available" in res.stderr
    res = subprocess.run([sys.executable, cli, model, "-i", *files, str(tmp_path / "missing.mell"), "-o", str(tmp_path / "b"),
                          "--gpus", "2", "-q"], env=env, capture_output=True, text=True, timeout=280)
    assert res.returncode != 0 and "missing.mell" in res.stderr and "no GPU available" not in res.stderr
    assert not os.path.exists(tmp_path / "b")

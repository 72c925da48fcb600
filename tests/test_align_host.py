"""The definition of the timing alignment (mbexwn_vocoder_amd/align.py) on the CPU: the recursion and
its tie rules on hand-computed tables and against a plain triple loop, the properties of the cost, the refusals, the
recovery of a known warp, and the way to the host analysis and to generate_mel.py --host."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import align_cases
from mbexwn_vocoder_amd import align, timemap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 3}


def path_of(q_full, band):
    q_full = np.asarray(q_full)
    nodes, cost = align.path_host(align.band_table(q_full, band), q_full.shape[1], band)
    return [tuple(int(vv) for vv in row) for row in nodes], cost


def plain_dtw(q_full, band):
    """The recursion as three nested loops over the full table: an independent statement of align.py's docstring."""
    n_a, n_b = q_full.shape
    cc = [(ii * (n_b - 1) + (n_a - 1) // 2) // max(n_a - 1, 1) for ii in range(n_a)]
    dist, back = {(0, 0): int(q_full[0, 0])}, {}
    for ii in range(1, n_a):
        for jj in range(n_b):
            if abs(jj - cc[ii]) > band:
                continue
            best = None
            for di, dj in ((1, 1), (1, 2), (2, 1)):
                prev = (ii - di, jj - dj)
                if prev in dist and (best is None or dist[prev] < dist[best]):
                    best = prev
            if best is not None:
                dist[ii, jj], back[ii, jj] = dist[best] + int(q_full[ii, jj]), best
    node = (n_a - 1, n_b - 1)
    if node not in dist or abs(n_b - 1 - cc[-1]) > band:
        return [], -1
    nodes = [node]
    while nodes[-1] != (0, 0):
        nodes.append(back[nodes[-1]])
    return nodes[::-1], dist[node]


# ------------------------------------------------------------------------------------------------------------------------
# the path
# ------------------------------------------------------------------------------------------------------------------------
def test_hand_computed_tables():
    # 3 x 3: two (1, 1) steps are the only way; the cost is the diagonal's
    assert path_of([[2, 9, 9], [9, 3, 9], [9, 9, 4]], 2) == ([(0, 0), (1, 1), (2, 2)], 9)
    # 4 x 6: one (1, 1) and two (1, 2) steps in any order -- three paths; the cheap cells pick (1, 2), (1, 2), (1, 1)
    qq = np.full((4, 6), 9)
    qq[0, 0] = qq[1, 2] = qq[2, 4] = qq[3, 5] = 1
    qq[1, 1] = qq[2, 3] = 5
    assert path_of(qq, 2) == ([(0, 0), (1, 2), (2, 4), (3, 5)], 4)
    qq[2, 4], qq[2, 3] = 7, 2                                   # ... and now (1, 2), (1, 1), (1, 2)
    assert path_of(qq, 2) == ([(0, 0), (1, 2), (2, 3), (3, 5)], 5)
    qq[1, 2], qq[1, 1] = 8, 1                                   # ... and (1, 1), (1, 2), (1, 2)
    assert path_of(qq, 1) == ([(0, 0), (1, 1), (2, 3), (3, 5)], 5)
    # one frame each: the node (0, 0)
    assert path_of([[7]], 1) == ([(0, 0)], 7)
    # a (2, 1) step and a (1, 2) step on their own
    assert path_of([[1, 9], [9, 9], [9, 2]], 1) == ([(0, 0), (2, 1)], 3)
    assert path_of([[1, 9, 9], [9, 9, 2]], 1) == ([(0, 0), (1, 2)], 3)


def test_tie_rules():
    # 4 x 6 of ones: all three paths cost 4.  At (3, 5) D(2, 4) = D(2, 3) = 3: the (1, 1) predecessor is first and wins
    assert path_of(np.ones((4, 6), dtype=int), 2) == ([(0, 0), (1, 2), (2, 4), (3, 5)], 4)
    # 4 x 4 of ones: the diagonal has 4 nodes, (1, 2) + (2, 1) and (2, 1) + (1, 2) have 3.  At (3, 3): D(2, 2) = 3, then
    # D(2, 1) = 2 through step (1, 2) takes over, and D(1, 2) = 2 through (2, 1) is not smaller: the earlier one stays
    assert path_of(np.ones((4, 4), dtype=int), 3) == ([(0, 0), (2, 1), (3, 3)], 3)
    # equal totals through different cells: (1, 1) before (1, 2) before (2, 1)
    qq = np.array([[1, 9, 9, 9], [9, 9, 2, 9], [9, 2, 1, 9], [9, 9, 9, 1]])
    # D(2, 2) = 1 + 9 + 1 = 11 (diagonal), D(2, 1) = 1 + 2 = 3, D(1, 2) = 1 + 2 = 3: the tie of 3 goes to step (1, 2)
    assert path_of(qq, 3) == ([(0, 0), (2, 1), (3, 3)], 4)


def test_unreachable_ends_and_a_band_that_cuts_the_path():
    for shape in ((2, 4), (4, 2), (1, 2), (2, 1), (5, 11), (11, 5)):         # no sum of the three steps joins the corners
        assert path_of(np.ones(shape, dtype=int), max(shape)) == ([], -1)
    assert path_of(np.ones((5, 9), dtype=int), 9)[1] == 5                   # slope exactly 2: four (1, 2) steps
    assert path_of(np.ones((9, 5), dtype=int), 9)[1] == 5
    # 7 x 7, a free path that leaves the diagonal by two frames at (2, 4)
    free = [(0, 0), (1, 2), (2, 4), (4, 5), (6, 6)]
    qq = np.full((7, 7), 10)
    for node in free:
        qq[node] = 0
    assert path_of(qq, 2) == (free, 0)
    # a band of one frame cuts (2, 4) off; the only way over the other free cells passes (3, 3)
    assert path_of(qq, 1) == ([(0, 0), (1, 2), (3, 3), (4, 5), (6, 6)], 10)
    # with the band too narrow for the end cell itself there is no path: Ta = 1 puts c(0) = 0, the end is (0, 3)
    assert path_of(np.ones((1, 4), dtype=int), 1) == ([], -1)


@pytest.mark.parametrize("seed", range(6))
def test_the_recursion_equals_a_plain_triple_loop(seed):
    rng = np.random.default_rng(seed)
    for _ in range(25):
        n_a = int(rng.integers(1, 14))
        n_b = int(rng.integers(max(1, n_a // 2), 2 * n_a + 1))
        band = int(rng.integers(1, 6))
        qq = rng.integers(0, 4, size=(n_a, n_b))                 # few values: many ties
        want = plain_dtw(qq, band)
        assert path_of(qq, band) == want, (n_a, n_b, band)


def test_band_table_and_centres_of_a_path():
    qq = np.arange(12).reshape(3, 4)
    table = align.band_table(qq, 1)                             # c = (3 i + 1) // 2 = 0, 2, 3
    assert align.band_centres(3, 4).tolist() == [0, 2, 3]
    assert table.dtype == np.uint16 and table.tolist() == [[align.NO_CELL, 0, 1], [5, 6, 7], [10, 11, align.NO_CELL]]
    # (1, 1), (2, 1), (1, 2): frame 2 is skipped and gets the mean of its neighbours, everything is clipped to n
    nodes = [(0, 0), (1, 1), (3, 2), (4, 4)]
    assert align.centres_from_path(nodes, 300, 2000).tolist() == [0, 300, 450, 600, 1200]
    assert align.centres_from_path(nodes, 300, 1000).tolist() == [0, 300, 450, 600, 1000]
    assert align.centres_from_path(nodes, 301, 10 ** 6).tolist() == [0, 301, (3 * 301) // 2, 602, 1204]
    assert align.centres_from_path(nodes, 300, 2000).dtype == np.int64
    for bad in ([], [(0, 1), (1, 2)], [(0, 0), (1, 3)], [(0, 0), (2, 2)]):
        with pytest.raises(ValueError):
            align.centres_from_path(bad, 300, 2000)


# ------------------------------------------------------------------------------------------------------------------------
# the cost
# ------------------------------------------------------------------------------------------------------------------------
def test_the_sum_has_the_stated_order_and_the_cost_its_quantum():
    rng = np.random.default_rng(3)
    for m in (1, 2, 3, 4, 5, 7, 80):
        xx = (rng.normal(size=(5, m)) * 10.0 ** rng.integers(-3, 4, size=(5, m))).astype(np.float32)
        want = np.zeros(5, dtype=np.float32)
        for row in range(5):
            part = [np.float32(0)] * 4
            for mm in range(m):
                part[mm % 4] = np.float32(part[mm % 4] + xx[row, mm])
            want[row] = np.float32(np.float32(part[0] + part[1]) + np.float32(part[2] + part[3]))
        assert np.array_equal(align.sum4_host(xx), want), m
    aa = rng.normal(size=(6, 7)).astype(np.float32)
    bb = rng.normal(size=(9, 7)).astype(np.float32)
    table = align.local_cost_host(aa, bb, 2)
    fa, fb = align.features_host(aa), align.features_host(bb)
    cc = align.band_centres(6, 9)
    for ii in range(6):
        for oo in range(5):
            jj = int(cc[ii]) - 2 + oo
            if not 0 <= jj < 9:
                assert table[ii, oo] == align.NO_CELL
                continue
            dd = align.sum4_host(np.abs(fa[ii] - fb[jj])[None])[0]
            assert table[ii, oo] == int(np.rint(min(dd, np.float32(2048)) * np.float32(8)))
    # the clamp: rows that differ by 1e30 cost 16384, and so does a NaN
    aa[0], bb[0, 0] = 1e30 * np.sign(rng.normal(size=7)), np.nan
    table = align.local_cost_host(aa, bb, 2)
    assert table[0, 2] == table[0, 3] == table[1, 0] == align.Q_MAX == 16384


def test_self_alignment_is_the_diagonal_and_level_does_not_matter():
    rng = np.random.default_rng(5)
    mel = (rng.normal(size=(40, 80)) * 2 - 5).astype(np.float32)
    nodes, cost = align.align_host(mel, mel, 4)
    assert nodes.dtype == np.int32 and nodes.tolist() == [[ii, ii] for ii in range(40)]
    diagonal = align.local_cost_host(mel, mel, 4)[:, 4].astype(np.int64)
    assert cost == int(diagonal.sum()) == 0
    # against another sequence the cost of the diagonal is what a path along it sums
    other = (mel + rng.normal(size=mel.shape) * 0.01).astype(np.float32)
    nodes, cost = align.align_host(mel, other, 4)
    table = align.local_cost_host(mel, other, 4).astype(np.int64)
    cc = align.band_centres(40, 40)
    assert cost == int(sum(table[ii, jj - cc[ii] + 4] for ii, jj in nodes)) > 0
    # a source at a quarter of the level: log-mel - log 4 in every channel
    guide = (rng.normal(size=(33, 80)) * 2 - 5).astype(np.float32)
    source = guide[np.sort(rng.integers(0, 33, size=45))] + (rng.normal(size=(45, 80)) * 0.05).astype(np.float32)
    quiet = (source + np.float32(np.log(0.25))).astype(np.float32)
    loud_nodes, _ = align.align_host(guide, source, 12)
    quiet_nodes, _ = align.align_host(guide, quiet, 12)
    assert len(loud_nodes) > 0 and np.array_equal(loud_nodes, quiet_nodes)


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    one = np.zeros((1, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="65535"):
        align.check_sizes(65536, 10, 4)
    with pytest.raises(ValueError, match="65535"):
        align.local_cost_host(one, np.zeros((65536, 4), dtype=np.float32), 4)
    assert align.check_sizes(65535, 65535, 511) == (65535, 65535, 511)
    for band in (0, -1, 512, 1.5):
        with pytest.raises(ValueError, match="band"):
            align.align_host(one, one, band)
    for empty in (np.zeros((0, 4), dtype=np.float32), np.zeros((3, 0), dtype=np.float32)):
        with pytest.raises(ValueError):
            align.align_host(empty, one, 1)
        with pytest.raises(ValueError):
            align.align_host(one, empty, 1)
    with pytest.raises(ValueError, match="mel channels"):
        align.align_host(one, np.zeros((1, 5), dtype=np.float32), 1)
    for seconds in (0, -1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="band"):
            align.band_frames(seconds, 24000, 300)
    assert align.band_frames(1.0, 24000, 300) == 80 and align.band_frames(1e-6, 24000, 300) == 1
    with pytest.raises(ValueError, match="511"):
        align.band_frames(7.0, 24000, 300)


def test_explicit_centres_are_a_third_kind_of_time_map():
    good = timemap.Centres([0, 0, 300, 450, 1000])
    assert timemap.centres(1000, 300, 24000, good).tolist() == [0, 0, 300, 450, 1000]
    assert timemap.centres(1000, 300, 24000, good).dtype == np.int64 and timemap.frame_count(1000, 300, 24000, good) == 5
    assert not timemap.is_factor(good) and timemap.per_item(good, 2) == [good, good]
    with pytest.raises(ValueError, match="non-decreasing"):
        timemap.centres(1000, 300, 24000, timemap.Centres([0, 300, 299]))
    with pytest.raises(ValueError, match=r"within \[0, 1000\]"):
        timemap.centres(1000, 300, 24000, timemap.Centres([0, 300, 1001]))
    with pytest.raises(ValueError, match=r"within \[0, 1000\]"):
        timemap.centres(1000, 300, 24000, timemap.Centres([-1, 300]))
    with pytest.raises(ValueError, match="limit"):                # 2^24 - 1 rows at 4 rows per frame
        timemap.centres(10, 300, 24000, timemap.Centres(np.zeros((1 << 22), dtype=np.int64)), rows_per_frame=4)
    for bad in ([], [[0, 1]], [0.0, 1.0], 3):
        with pytest.raises(ValueError, match="1-D integer"):
            timemap.Centres(bad)
    with pytest.raises(ValueError, match=r"\(m, 2\)"):             # a bare 1-D list stays what it was: no map
        timemap.centres(1000, 300, 24000, [0, 300, 600])


def load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(BIN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("tool", ["transform_audio", "generate_mel"])
def test_the_parsers_refuse_the_combinations_with_status_2(tool, capsys):
    parser = load_tool(tool).make_parser()
    base = ["a.wav", "-o", "out"]
    args = parser.parse_args(base)
    assert (args.align_to, args.align_to_dir, args.align_band) == (None, None, 1.0)
    args = parser.parse_args(base + ["--align-to", "g.wav", "--align-band", "0.5"])
    assert (args.align_to, args.align_to_dir, args.align_band) == ("g.wav", None, 0.5)
    assert parser.parse_args(base + ["--align-to-dir", "guides"]).align_to_dir == "guides"
    assert parser.parse_args(base + ["--time-stretch", "1.5"]).time_stretch == 1.5
    bad = [["--align-to", "g.wav", "--time-stretch", "1.5"], ["--align-to-dir", "d", "--time-stretch", "0.5"],
           ["--align-to", "g.wav", "--align-to-dir", "d"]]
    bad += [["--align-to", "g.wav", "--align-band", vv] for vv in ("0", "-1", "nan", "inf", "x")]
    if tool == "transform_audio":
        bad += [["--align-to", "g.wav", "--time-stretch-file", "list.txt"], ["--align-to-dir", "d", "--time-stretch-file", "l"]]
    for extra in bad:
        with pytest.raises(SystemExit) as exc:
            parser.parse_args(base + extra)
        assert exc.value.code == 2, extra
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------------------------
# a known warp is recovered
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sine_mels():
    from mbexwn_vocoder_amd.analysis import compute_log_mel
    guide, source = align_cases.sine_case()
    return tuple(compute_log_mel(ss[np.newaxis], align_cases.PRE, dtype=np.float32)[0][0] for ss in (guide, source))


def test_a_known_warp_is_recovered(sine_mels):
    """The guide is the source's score at w(t) = t + 0.25 sin(2 pi t / 4), 641 frames each.  At W = 40 the path's source
    time may differ from w by at most 4 frames and by 1 frame on average (the definition measures 1.8 and 0.53 on this
    sound)."""
    mel_a, mel_b = sine_mels
    assert mel_a.shape == mel_b.shape == (641, 80)
    nodes, cost = align.align_host(mel_a, mel_b, 40)
    worst, mean = align_cases.warp_error(nodes)
    print(f"sine warp at W = 40: {len(nodes)} nodes, cost {cost}, max {worst:.3f} frames, mean {mean:.3f} frames")
    assert tuple(nodes[0]) == (0, 0) and tuple(nodes[-1]) == (640, 640)
    assert worst <= 4.0 and mean <= 1.0
    # the map is far from the diagonal: the diagonal itself would miss by 20 frames
    assert align_cases.warp_error(np.stack((np.arange(641), np.arange(641)), axis=1))[0] > 19.0


# ------------------------------------------------------------------------------------------------------------------------
# end to end on the host
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    return create_synthetic_model_dir(str(tmp_path_factory.mktemp("model") / "speech_small"), "SPEECH", **SMALL)


@pytest.fixture(scope="module")
def pre(model_dir):
    from mbexwn_vocoder_amd.config import read_config
    return read_config(os.path.join(model_dir, "config.yaml"))["preprocess_config"]


def short_case():
    """2 s of the sine case: a guide of 2 s and a source cut 0.1 s shorter (the ends still hold the same syllables)."""
    guide, source = align_cases.sine_case()
    return np.array(guide[:48000]), np.array(source[:48000 - 2400])


def test_generate_mels_on_the_host_follows_the_guide(pre):
    from mbexwn_vocoder_amd.analysis import compute_log_mel, compute_log_mel_at, generate_mels
    guide, source = short_case()
    other = np.array(align_cases.sine_case()[1][5000:20000])
    notes = {}
    dicts = generate_mels([source, other], [24000, 24000], pre, on_device=False, guides=[guide, None], guide_rates=[24000, None],
                          align_band_s=0.5, align_out=notes)
    mel_a = compute_log_mel(guide[np.newaxis], pre, dtype=np.float32)[0][0]
    mel_b = compute_log_mel(source[np.newaxis], pre, dtype=np.float32)[0][0]
    nodes, cost = align.align_host(mel_a, mel_b, align.band_frames(0.5, 24000, 300))
    centres = align.centres_from_path(nodes, 300, source.size)
    assert centres.shape == (mel_a.shape[0],) == (161,) and np.all(np.diff(centres) >= 0)
    want = compute_log_mel_at(source[np.newaxis], centres, pre, dtype=np.float32)[0][0]
    assert dicts[0]["mell"].shape == (80, 161) and np.array_equal(dicts[0]["mell"], want.T)
    assert np.array_equal(dicts[1]["mell"], compute_log_mel(other[np.newaxis], pre, dtype=np.float32)[0][0].T)
    assert sorted(notes) == [0] and notes[0]["nodes"] == len(nodes) and notes[0]["cost"] == cost
    assert notes[0]["mean_cost"] == cost / 8.0 / len(nodes) and 0 < notes[0]["max_offset_ms"] <= 500.0
    # no guide at all: the call of before
    plain = generate_mels([source, other], [24000, 24000], pre, on_device=False, guides=[None, None], guide_rates=[None, None])
    assert np.array_equal(plain[0]["mell"], mel_b.T) and np.array_equal(plain[1]["mell"], dicts[1]["mell"])
    # a source three times as long as its guide cannot be aligned: raised, or noted where a dict is given
    with pytest.raises(align.AlignError, match="161 frames.*41 frames|41 frames.*161 frames"):
        generate_mels([guide], [24000], pre, on_device=False, guides=[guide[:12000]], guide_rates=[24000])
    notes = {}
    dicts = generate_mels([guide, other], [24000, 24000], pre, on_device=False, guides=[guide[:12000], None],
                          guide_rates=[24000, None], align_out=notes)
    assert dicts[0] is None and "error" in notes[0] and "band of 80 frames" in notes[0]["error"] and dicts[1] is not None
    with pytest.raises(ValueError, match="guide and a time map"):
        generate_mels([source], [24000], pre, on_device=False, guides=[guide], guide_rates=[24000], time_maps=[1.5])


def test_generate_mel_tool_writes_the_aligned_file(pre, model_dir, tmp_path):
    from scipy.io import wavfile
    from mbexwn_vocoder_amd.analysis import generate_mels
    from mbexwn_vocoder_amd.fileio import load_var
    guide, source = short_case()
    wavfile.write(str(tmp_path / "guide.wav"), 24000, guide)
    wavfile.write(str(tmp_path / "take.wav"), 24000, source)
    wavfile.write(str(tmp_path / "long.wav"), 24000, np.concatenate([guide] * 3))
    cli = os.path.join(BIN, "generate_mel.py")
    out = str(tmp_path / "out")
    res = subprocess.run([sys.executable, cli, str(tmp_path / "take.wav"), "-o", out, "--model_id", model_dir, "--host",
                          "--align-to", str(tmp_path / "guide.wav"), "--align-band", "0.5", "-v"], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "mean cost per node" in res.stderr and "largest offset from the diagonal" in res.stderr
    want = generate_mels([source], [24000], pre, on_device=False, guides=[guide], guide_rates=[24000], align_band_s=0.5)[0]
    got = load_var(os.path.join(out, "take.mell"))
    assert got["mell"].shape == (80, 161) and np.array_equal(got["mell"], want["mell"])
    # a file that cannot be aligned is reported and skipped, the other is written, the exit status is 1
    out2 = str(tmp_path / "out2")
    res = subprocess.run([sys.executable, cli, str(tmp_path / "long.wav"), str(tmp_path / "take.wav"), "-o", out2, "--model_id",
                          model_dir, "--host", "--align-to", str(tmp_path / "guide.wav"), "--align-band", "0.5"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 1 and "skipped" in res.stderr and "long.wav" in res.stderr and "cannot be aligned" in res.stderr
    assert os.listdir(out2) == ["take.mell"]

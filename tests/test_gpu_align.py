"""The timing alignment on the GPU: mbxg_local_cost and mbxg_align_path (csrc/mel_align.hip) against their definitions
align.local_cost_host and align.path_host, bit for bit -- no tolerance: the float32 sums have one order on both sides and
everything behind the quantised cost is integer --, their memory contract (outputs and workspace between guard bands, nothing
written behind an item's counts), their refusals, and the way through generate_mels and transform_audio.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import align_cases
from guarded import Guarded
from helpers import build_case
from mbexwn_vocoder_amd import align, analysis

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")
# one frame, the smallest with a step, both directions of (1, 2) and (2, 1), odd sizes, a whole wave, one more, a long one
SHAPES = [(1, 1), (2, 2), (2, 3), (3, 2), (7, 13), (13, 7), (64, 64), (65, 127), (300, 257)]
BANDS = [1, 2, 31, 32, 33]       # 63, 65 and 67 cells: one fewer and one more than a wave; plus W = Tb, wider than the item
LOG_EPS = float(np.log(np.finfo(np.float32).eps))


@pytest.fixture(scope="module")
def torch():
    import torch as tt
    return tt


def dev(torch, arr):
    return torch.as_tensor(np.ascontiguousarray(arr)).cuda()


def bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float32).view(np.uint32)


def random_mel(rng, frames, mels, special=True):
    """A log-mel like the analysis makes, with -- where there is room -- a row on the log(eps) floor and rows of +-1e30
    (costs beyond the clamp at 2048)."""
    mel = (rng.normal(size=(frames, mels)) * 2.0 - 5.0).astype(np.float32)
    if special and frames >= 5:
        mel[1] = LOG_EPS
        mel[frames // 2] = np.where(rng.random(mels) < 0.5, -1e30, 1e30).astype(np.float32)
        mel[frames - 2, ::2] = 1e30
    return mel


class Call:
    """One raw call of mbxg_local_cost and one of mbxg_align_path on a ragged batch: every output and the workspace between
    guard bands, pre-filled."""

    def __init__(self, torch, mels_a, mels_b, band, fill="nan", counts_a=None, counts_b=None):
        from mbexwn_vocoder_amd.abi import load_library
        self.torch, self.lib, self.band = torch, load_library(), int(band)
        self.batch, self.mels = len(mels_a), int(mels_a[0].shape[1])
        self.max_a, self.max_b = max(mm.shape[0] for mm in mels_a), max(mm.shape[0] for mm in mels_b)
        host_a = np.full((self.batch, self.max_a, self.mels), np.nan, dtype=np.float32)    # padding a kernel must not use
        host_b = np.full((self.batch, self.max_b, self.mels), np.nan, dtype=np.float32)
        for bb in range(self.batch):
            host_a[bb, :mels_a[bb].shape[0]] = mels_a[bb]
            host_b[bb, :mels_b[bb].shape[0]] = mels_b[bb]
        self.mel_a, self.mel_b = dev(torch, host_a), dev(torch, host_b)
        self.n_a = dev(torch, np.asarray([mm.shape[0] for mm in mels_a] if counts_a is None else counts_a, np.int32))
        self.n_b = dev(torch, np.asarray([mm.shape[0] for mm in mels_b] if counts_b is None else counts_b, np.int32))
        self.nb = 2 * self.band + 1
        self.work_bytes = int(self.lib.mbxg_align_workspace_size(self.batch, self.max_a, self.band))
        self.cost = Guarded("cost", 2 * self.batch * self.max_a * self.nb, fill, device="cuda")
        self.work = Guarded("workspace", self.work_bytes, fill, device="cuda")
        self.nodes_i = Guarded("nodes_i", 4 * self.batch * self.max_a, fill, device="cuda")
        self.nodes_j = Guarded("nodes_j", 4 * self.batch * self.max_a, fill, device="cuda")
        self.count = Guarded("count", 4 * self.batch, fill, device="cuda")
        self.total = Guarded("total", 4 * self.batch, fill, device="cuda")
        self.outputs = [self.cost, self.nodes_i, self.nodes_j, self.count, self.total]

    def run_cost(self, **kw):
        args = dict(mel_a=self.mel_a.data_ptr(), mel_b=self.mel_b.data_ptr(), n_frames_a=self.n_a.data_ptr(),
                    n_frames_b=self.n_b.data_ptr(), batch=self.batch, max_frames_a=self.max_a, max_frames_b=self.max_b,
                    n_mels=self.mels, band=self.band, cost=self.cost.ptr)
        args.update(kw)
        status = self.lib.mbxg_local_cost(args["mel_a"], args["mel_b"], args["n_frames_a"], args["n_frames_b"], args["batch"],
                                          args["max_frames_a"], args["max_frames_b"], args["n_mels"], args["band"], args["cost"],
                                          None)
        self.torch.cuda.synchronize()
        return status

    def run_path(self, **kw):
        args = dict(cost=self.cost.ptr, n_frames_a=self.n_a.data_ptr(), n_frames_b=self.n_b.data_ptr(), batch=self.batch,
                    max_frames_a=self.max_a, band=self.band, workspace=self.work.ptr, workspace_bytes=self.work_bytes,
                    nodes_i=self.nodes_i.ptr, nodes_j=self.nodes_j.ptr, count=self.count.ptr, total=self.total.ptr)
        args.update(kw)
        status = self.lib.mbxg_align_path(args["cost"], args["n_frames_a"], args["n_frames_b"], args["batch"],
                                          args["max_frames_a"], args["band"], args["workspace"], args["workspace_bytes"],
                                          args["nodes_i"], args["nodes_j"], args["count"], args["total"], None)
        self.torch.cuda.synchronize()
        return status

    def table(self):
        return self.cost.view(self.torch.int16, self.batch, self.max_a, self.nb).cpu().numpy().view(np.uint16)

    def ints(self, buf, *shape):
        return buf.view(self.torch.int32, *shape).cpu().numpy()

    def untouched(self, buffers=None):
        return all(gg.payload_untouched() for gg in (self.outputs if buffers is None else buffers))

    def check(self):
        for gg in self.outputs + [self.work]:
            gg.check()


def assert_equals_definition(call, mels_a, mels_b, fill="nan"):
    """Both kernels' results against align.py, item by item; behind an item's counts the fill is still there."""
    from guarded import fill_word
    assert call.run_cost() == 0, call.lib.mbx_last_error()
    got = call.table()
    word = np.asarray([fill_word(fill)], dtype="<i4")
    half = word.view(np.uint16)
    for bb, (aa, cc) in enumerate(zip(mels_a, mels_b)):
        want = align.local_cost_host(aa, cc, call.band)
        assert np.array_equal(got[bb, :aa.shape[0]], want), (bb, aa.shape, cc.shape, call.band)
        rest = got[bb, aa.shape[0]:].reshape(-1)
        if rest.size:                                            # rows behind the item: the fill's halves, in its phase
            flat0 = (bb * call.max_a + aa.shape[0]) * call.nb
            assert np.array_equal(rest, half[(flat0 + np.arange(rest.size)) % 2]), bb
    assert call.run_path() == 0, call.lib.mbx_last_error()
    nodes_i, nodes_j = call.ints(call.nodes_i, call.batch, call.max_a), call.ints(call.nodes_j, call.batch, call.max_a)
    count, total = call.ints(call.count, call.batch), call.ints(call.total, call.batch)
    for bb, (aa, cc) in enumerate(zip(mels_a, mels_b)):
        nodes, cost = align.path_host(got[bb, :aa.shape[0]], cc.shape[0], call.band)
        assert count[bb] == len(nodes) and total[bb] == cost, (bb, aa.shape, cc.shape, call.band, count[bb], total[bb], cost)
        assert np.array_equal(nodes_i[bb, :count[bb]], nodes[:, 0]) and np.array_equal(nodes_j[bb, :count[bb]], nodes[:, 1]), bb
        assert np.all(nodes_i[bb, count[bb]:] == word[0]) and np.all(nodes_j[bb, count[bb]:] == word[0]), bb
    call.check()
    return count, total


# ------------------------------------------------------------------------------------------------------------------------
# bit equality with the definition
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mels", [1, 7, 80])
def test_both_kernels_equal_the_definition_bit_for_bit(torch, mels):
    rng = np.random.default_rng(100 + mels)
    mels_a = [random_mel(rng, ta, mels) for ta, _ in SHAPES]
    mels_b = [random_mel(rng, tb, mels) for _, tb in SHAPES]
    # a pair that does align well: the source is the guide, locally repeated and thinned, plus a little noise
    pick = np.clip(np.round(np.arange(257) * 299 / 256 + 6 * np.sin(np.arange(257) / 20)).astype(int), 0, 299)
    mels_b[-1] = (mels_a[-1][np.sort(pick)] + rng.normal(size=(257, mels)).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    aligned = 0
    for band in BANDS:                                           # all nine shapes in one ragged batch
        count, _ = assert_equals_definition(Call(torch, mels_a, mels_b, band), mels_a, mels_b)
        aligned += int(np.count_nonzero(count))
        assert count[0] == 1 and count[1] == 2                   # (1, 1) and (2, 2) always have their path
    for (ta, tb), aa, cc in zip(SHAPES, mels_a, mels_b):          # W = Tb: a band wider than the item
        count, _ = assert_equals_definition(Call(torch, [aa], [cc], tb), [aa], [cc])
        assert (count[0] > 0) == (ta == 1 == tb or (ta > 1 and tb > 1 and 0.5 <= (tb - 1) / (ta - 1) <= 2.0)), (ta, tb)
    assert aligned >= 5 * 4


def test_the_clamp_and_the_floor_rows_are_hit(torch):
    """What the special rows are for: a cost table with 16384 (beyond the clamp), 0 (floor against floor) and values between."""
    rng = np.random.default_rng(7)
    aa, cc = random_mel(rng, 64, 80), random_mel(rng, 64, 80)
    call = Call(torch, [aa], [cc], 33)
    assert call.run_cost() == 0
    table = call.table()[0]
    assert np.array_equal(table, align.local_cost_host(aa, cc, 33))
    inside = table[table != align.NO_CELL]
    assert inside.max() == 16384 and inside.min() == 0 and np.count_nonzero((inside > 0) & (inside < 16384)) > 1000
    assert np.count_nonzero(table == align.NO_CELL) > 0          # band columns outside the item


def test_a_ragged_batch_with_an_item_that_cannot_be_aligned(torch):
    rng = np.random.default_rng(9)
    shapes = [(40, 33), (64, 64), (5, 14), (65, 127), (1, 1)]    # (5, 14): more than twice as long -- no path
    base = random_mel(rng, 130, 80, special=False)
    mels_a = [base[:ta].copy() for ta, _ in shapes]
    mels_b = [(base[np.round(np.linspace(0, ta - 1, tb)).astype(int)]
               + rng.normal(size=(tb, 80)).astype(np.float32) * np.float32(0.1)).astype(np.float32) for ta, tb in shapes]
    for fill in ("nan", "huge", "zero"):
        count, total = assert_equals_definition(Call(torch, mels_a, mels_b, 20, fill=fill), mels_a, mels_b, fill=fill)
        assert count[2] == 0 and total[2] == -1 and np.all(count[[0, 1, 3, 4]] > 0) and np.all(total[[0, 1, 3, 4]] >= 0)
    # the same through the package's wrappers, and items whose counts say "no frames"
    n_a = dev(torch, np.asarray([40, 0, 5, 65, 1], np.int32))
    n_b = dev(torch, np.asarray([33, 64, 14, 0, 1], np.int32))
    pad_a, pad_b = np.zeros((5, 65, 80), np.float32), np.zeros((5, 127, 80), np.float32)
    for bb in range(5):
        pad_a[bb, :shapes[bb][0]], pad_b[bb, :shapes[bb][1]] = mels_a[bb], mels_b[bb]
    nodes_i, nodes_j, count, total = (tt.cpu().numpy() for tt in align.align_device(dev(torch, pad_a), n_a, dev(torch, pad_b), n_b, 20))
    assert count.tolist()[1:4] == [0, 0, 0] and total.tolist()[1:4] == [-1, -1, -1]
    for bb in (0, 4):
        nodes, cost = align.align_host(mels_a[bb], mels_b[bb], 20)
        assert count[bb] == len(nodes) and total[bb] == cost
        assert np.array_equal(nodes_i[bb, :count[bb]], nodes[:, 0]) and np.array_equal(nodes_j[bb, :count[bb]], nodes[:, 1])


# ------------------------------------------------------------------------------------------------------------------------
# the memory contract
# ------------------------------------------------------------------------------------------------------------------------
def test_workspace_size_is_exact_and_refusals_leave_the_outputs_untouched(torch):
    rng = np.random.default_rng(21)
    mels_a = [random_mel(rng, 30, 7), random_mel(rng, 11, 7)]
    mels_b = [random_mel(rng, 25, 7), random_mel(rng, 16, 7)]
    call = Call(torch, mels_a, mels_b, 6, fill="huge")
    lib = call.lib

    def why():
        return lib.mbx_last_error().decode()

    # the size function: one byte per band cell rounded up to 4, and 4 bytes per guide frame; 0 for what the call refuses
    assert call.work_bytes == (2 * 30 * 13 + 3) // 4 * 4 + 4 * 2 * 30
    assert lib.mbxg_align_workspace_size(3, 5, 1) == (3 * 5 * 3 + 3) // 4 * 4 + 4 * 3 * 5 == 108
    assert lib.mbxg_align_workspace_size(65535, 65535, 511) == (65535 * 65535 * 1023 + 3) // 4 * 4 + 4 * 65535 * 65535
    for bad in ((-1, 5, 1), (65536, 5, 1), (1, 0, 1), (1, 65536, 1), (1, 5, 0), (1, 5, 512)):
        assert lib.mbxg_align_workspace_size(*bad) == 0, bad
    assert lib.mbxg_align_workspace_size(0, 5, 1) == 0

    cases = [({name: None}, "null") for name in ("mel_a", "mel_b", "n_frames_a", "n_frames_b", "cost")]
    cases += [({"batch": -1}, "batch"), ({"batch": 65536}, "batch"), ({"max_frames_a": 0}, "max_frames_a"),
              ({"max_frames_b": 0}, "max_frames_b"), ({"max_frames_a": 65536}, "65535"), ({"max_frames_b": 65536}, "65535"),
              ({"n_mels": 0}, "n_mels"), ({"n_mels": 241}, "n_mels"), ({"band": 0}, "band"), ({"band": -3}, "band"),
              ({"band": 512}, "band")]
    for kw, what in cases:
        assert call.run_cost(**kw) == 1, kw                      # MBX_ERR_INVALID_ARGUMENT
        assert why().startswith("local cost:") and what in why(), (kw, why())
        assert call.untouched(), kw
        call.check()
    assert call.run_cost(batch=0) == 0 and call.untouched()      # nothing to do
    assert call.run_cost() == 0 and not call.cost.payload_untouched() and call.untouched(call.outputs[1:])

    cases = [({name: None}, "null") for name in ("cost", "n_frames_a", "n_frames_b", "workspace", "nodes_i", "nodes_j", "count",
                                                 "total")]
    cases += [({"batch": -1}, "batch"), ({"batch": 65536}, "batch"), ({"max_frames_a": 0}, "max_frames_a"),
              ({"max_frames_a": 65536}, "65535"), ({"band": 0}, "band"), ({"band": 512}, "band"),
              ({"workspace_bytes": call.work_bytes - 1}, "workspace"), ({"workspace_bytes": 0}, "workspace"),
              ({"band": 7}, "workspace"),                        # a wider band needs more than this workspace
              ({"workspace": call.work.ptr + 1}, "aligned")]
    for kw, what in cases:
        assert call.run_path(**kw) == 1, kw
        assert why().startswith("align path:") and what in why(), (kw, why())
        assert call.untouched(call.outputs[1:]) and call.work.payload_untouched(), kw
        call.check()
    assert call.run_path(batch=0) == 0 and call.untouched(call.outputs[1:]) and call.work.payload_untouched()
    # and the same buffers do run, the workspace of exactly the stated size between its guards
    assert call.run_path() == 0 and not call.count.payload_untouched()
    call.check()
    want = [align.align_host(aa, cc, 6) for aa, cc in zip(mels_a, mels_b)]
    assert call.ints(call.count, 2).tolist() == [len(nodes) for nodes, _ in want]
    assert call.ints(call.total, 2).tolist() == [cost for _, cost in want]
    # items without frames write their count and total, and nothing else
    empty = Call(torch, mels_a, mels_b, 6, fill="nan", counts_a=[0, 11], counts_b=[25, 0])
    assert empty.run_cost() == 0 and empty.run_path() == 0
    assert empty.ints(empty.count, 2).tolist() == [0, 0] and empty.ints(empty.total, 2).tolist() == [-1, -1]
    assert empty.nodes_i.payload_untouched() and empty.nodes_j.payload_untouched()
    assert empty.cost.payload_untouched()                        # no guide rows, no source rows: no table
    empty.check()


# ------------------------------------------------------------------------------------------------------------------------
# through the package: the synthetic canonical model, batch_invariant kernels
# ------------------------------------------------------------------------------------------------------------------------
def run_script(name, args):
    return subprocess.run([sys.executable, os.path.join(BIN, name + ".py"), *args], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from mbexwn_vocoder_amd.config import dump_config
    from mbexwn_vocoder_amd.weights import save_weights
    cfg, raw, _ = build_case("SPEECH", {})
    path = str(tmp_path_factory.mktemp("model") / "speech")
    os.makedirs(path)
    dump_config(os.path.join(path, "config.yaml"), cfg)
    save_weights(os.path.join(path, "weights.npz"), raw)
    return path


@pytest.fixture(scope="module")
def inv(model_dir):
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    return MELInverter(model_dir, batch_invariant=True)


def device_mel_at(torch, sound, centres, pre):
    mel, _ = analysis.compute_log_mel_device_at(dev(torch, sound[np.newaxis]), dev(torch, np.asarray([sound.size], np.int32)),
                                                dev(torch, np.asarray(centres, np.int64)[np.newaxis]),
                                                dev(torch, np.asarray([len(centres)], np.int32)), pre)
    return mel[0].cpu().numpy()


def test_generate_mels_recovers_the_sine_warp_on_the_device(torch, inv):
    """The case of tests/test_align_host.py through generate_mels(on_device=True): the centres are the definition's on the
    device's own mels, the rows carry the bits of compute_log_mel_device_at on them, the warp is recovered within the same
    caps (max 4 frames, mean 1 frame at W = 40), and the neighbour without a guide keeps its regular bits."""
    pre = inv.preprocess_config
    guide, source = (np.array(ss) for ss in align_cases.sine_case())
    other = source[10000:40000].copy()
    regular = analysis.generate_mels([guide, source, other], [24000] * 3, pre)
    mel_a, mel_b = regular[0]["mell"].T, regular[1]["mell"].T
    assert mel_a.shape == mel_b.shape == (641, 80)
    nodes, cost = align.align_host(mel_a, mel_b, 40)
    worst, mean = align_cases.warp_error(nodes)
    print(f"sine warp on the device's mels at W = 40: {len(nodes)} nodes, cost {cost}, max {worst:.3f}, mean {mean:.3f} frames")
    assert worst <= 4.0 and mean <= 1.0
    centres = align.centres_from_path(nodes, 300, source.size)
    notes = {}
    dicts = analysis.generate_mels([source, other], [24000, 24000], pre, guides=[guide, None], guide_rates=[24000, None],
                                   align_band_s=0.5, align_out=notes)
    assert notes[0]["nodes"] == len(nodes) and notes[0]["cost"] == cost and sorted(notes) == [0]
    assert dicts[0]["mell"].shape == (80, 641)
    assert np.array_equal(bits(dicts[0]["mell"].T), bits(device_mel_at(torch, source, centres, pre)))
    assert np.array_equal(bits(dicts[1]["mell"]), bits(regular[2]["mell"]))
    # one item at a time gives the same bits; an item that cannot be aligned is noted and leaves None
    alone = analysis.generate_mels([source], [24000], pre, batch=1, guides=[guide], guide_rates=[24000], align_band_s=0.5)
    assert np.array_equal(bits(alone[0]["mell"]), bits(dicts[0]["mell"]))
    notes = {}
    dicts = analysis.generate_mels([source, other], [24000, 24000], pre, guides=[guide[:48000], None], guide_rates=[24000, None],
                                   align_out=notes)
    assert dicts[0] is None and "cannot be aligned" in notes[0]["error"] and np.array_equal(bits(dicts[1]["mell"]), bits(regular[2]["mell"]))
    with pytest.raises(align.AlignError):
        analysis.generate_mels([source], [24000], pre, guides=[guide[:48000]], guide_rates=[24000])


@pytest.fixture(scope="module")
def short_files(tmp_path_factory):
    """The guide's first 1.5 s -- 1.677 s of the score --, two takes of that much score (at score time: 40 200 samples; 1.6 s
    long), and a bystander a quarter of the guide's length."""
    from scipy.io import wavfile
    root = tmp_path_factory.mktemp("takes")
    guide, source = (np.array(ss) for ss in align_cases.sine_case())
    tt = np.arange(int(1.6 * 24000)) / 24000
    takes = {"take_a.wav": (source[:40200], 24000), "take_b.wav": (align_cases.render(tt * 1.677 / 1.6, noise_seed=3), 24000),
             "other.wav": (source[50000:60000], 24000), "guide.wav": (guide[:36000], 24000)}
    for name, (snd, rate) in takes.items():
        wavfile.write(str(root / name), rate, snd.astype(np.float32))
    return str(root), takes


@pytest.mark.timeout(600)
def test_cli_align_to_writes_the_guides_length_in_any_batch(model_dir, short_files, tmp_path):
    from mbexwn_vocoder_amd.audioio import read_audio
    root, takes = short_files
    files = [os.path.join(root, "take_a.wav"), os.path.join(root, "take_b.wav")]
    common = ["--model_id", model_dir, "--align-to", os.path.join(root, "guide.wav"), "--align-band", "0.5", "--batch-invariant",
              "--noise-seed", "5", "-v"]
    outs = []
    for batch in ("2", "1"):
        outs.append(str(tmp_path / f"batch{batch}"))
        res = run_script("transform_audio", [*files, "-o", outs[-1], "--batch", batch, *common])
        assert res.returncode == 0, res.stderr[-3000:]
        assert res.stderr.count("mean cost per node") == 2 and "largest offset from the diagonal" in res.stderr
    want = (36000 // 300 + 1) * 300                              # the guide's frames times the hop
    for name in ("syn_take_a.flac", "syn_take_b.flac"):
        one, two = (open(os.path.join(oo, name), "rb").read() for oo in outs)
        assert one == two, name
        audio, rate = read_audio(os.path.join(outs[0], name))
        assert rate == 24000 and audio.size == want, (name, audio.size)
    res = run_script("transform_audio", [*files, "-o", str(tmp_path / "x"), "--model_id", model_dir, "--align-to", "g.wav",
                                         "--time-stretch", "1.2"])
    assert res.returncode == 2 and "not combinable" in res.stderr


def test_a_job_without_guides_keeps_its_bytes_beside_a_guided_neighbour(inv, short_files, tmp_path, monkeypatch):
    """run_audio_job with and without a guided neighbour: the file without a guide has the same bytes, a job without any
    guide makes none of the two launches, and the guided file has its guide's sample count."""
    from mbexwn_vocoder_amd.abi import load_library
    from mbexwn_vocoder_amd.audioio import read_audio
    from mbexwn_vocoder_amd.batched import run_audio_job
    root, _ = short_files
    files = [os.path.join(root, "other.wav"), os.path.join(root, "take_a.wav")]
    lib, calls = load_library(), []
    for symbol in ("mbxg_local_cost", "mbxg_align_path"):
        def spy(*args, _real=getattr(lib, symbol), _name=symbol):
            calls.append(_name)
            return _real(*args)
        monkeypatch.setattr(lib, symbol, spy)
    plain, nones, mixed = str(tmp_path / "plain"), str(tmp_path / "nones"), str(tmp_path / "mixed")
    for out in (plain, nones, mixed):
        os.makedirs(out)
    assert run_audio_job(inv, files, plain, "flac", noise_seed=5, quiet=True) == [] and calls == []
    assert run_audio_job(inv, files, nones, "flac", noise_seed=5, quiet=True, guides=[None, None]) == [] and calls == []
    skipped = run_audio_job(inv, files, mixed, "flac", noise_seed=5, quiet=True, guides=[None, os.path.join(root, "guide.wav")],
                            align_band_s=0.5)
    assert skipped == [] and calls == ["mbxg_local_cost", "mbxg_align_path"]
    for other in (nones, mixed):
        assert open(os.path.join(plain, "syn_other.flac"), "rb").read() == open(os.path.join(other, "syn_other.flac"), "rb").read()
    assert read_audio(os.path.join(mixed, "syn_take_a.flac"))[0].size == 121 * 300
    assert read_audio(os.path.join(plain, "syn_take_a.flac"))[0].size == (40200 // 300 + 1) * 300
    # a file that cannot be aligned is reported and skipped, the other is written
    again = str(tmp_path / "again")
    os.makedirs(again)
    skipped = run_audio_job(inv, files, again, "flac", noise_seed=5, quiet=True, guides=[os.path.join(root, "guide.wav"), None])
    assert [name for name, _ in skipped] == [files[0]] and "cannot be aligned" in skipped[0][1]
    assert os.listdir(again) == ["syn_take_a.flac"]

"""The shared layers under the file tools, on the host: the control rows of ``run_micro_batches``, the argv a ``--gpus`` parent
builds from its own parser, and the arrays-in pipeline below ``MELInverter.transform_audio`` and ``batched.run_audio_job``."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")


# ------------------------------------------------------------------------------------------------------------------------
# the control rows of run_micro_batches
# ------------------------------------------------------------------------------------------------------------------------
class _RecordingEngine:
    """Records the keyword arguments of every forward; the audio is zeros."""
    device = "cpu"
    dims = SimpleNamespace(sample_rate=24000, wn_in_rows_per_frame=4, hop_size=8)

    def __init__(self):
        self.calls = []

    def forward(self, mel, n_frames=None, noise=None, **control):
        import torch
        self.calls.append((n_frames.tolist(), control))
        return torch.zeros((mel.shape[0], mel.shape[1] * self.dims.hop_size))


class _Event:
    def __init__(self, enable_timing=False):
        pass

    def record(self, stream=None):
        pass


LENGTHS = (3, 5, 5, 2)


def control_rows(monkeypatch, **kw):
    """The (n_frames, control) of every forward of four mels of 3, 5, 5 and 2 frames in micro-batches of two."""
    import torch
    from mbexwn_vocoder_amd.batched import run_micro_batches
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: None)
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    engine = _RecordingEngine()
    mels = [np.zeros((tt, 80), np.float32) for tt in LENGTHS]
    batches = list(run_micro_batches(engine, mels, None, max_batch=2, host_audio=False, **kw))
    assert sorted(ii for sb in batches for ii in sb.indices) == [0, 1, 2, 3] and all(len(sb.indices) == 2 for sb in batches)
    assert [nn for nn, _ in engine.calls] == [[LENGTHS[ii] for ii in sb.indices] for sb in batches]
    return [(sb.indices, control) for sb, (_, control) in zip(batches, engine.calls)]


def padded(rows, dtype=np.float32):
    """Rows of unequal length as one array, each continued with its last value."""
    out = np.ones((len(rows), max(len(rr) for rr in rows)), dtype=dtype)
    for jj, rr in enumerate(rows):
        out[jj, :len(rr)], out[jj, len(rr):] = rr, rr[-1]
    return out


def ramp(ii, base):
    return (base + 0.01 * np.arange(LENGTHS[ii])).astype(np.float32)


def test_control_rows_of_every_combination(monkeypatch):
    import torch
    ones = [np.ones(tt, np.float32) for tt in LENGTHS]
    for indices, control in control_rows(monkeypatch):
        assert control == {}
    # transpositions: f0_scale in every micro-batch, ones for the item with None, the padding repeats the last factor
    rows = [ramp(0, 1.5), None, ramp(2, 0.5), ramp(3, 2.0)]
    for indices, control in control_rows(monkeypatch, transpositions=rows):
        assert sorted(control) == ["f0_scale"] and control["f0_scale"].dtype == torch.float32
        assert np.array_equal(control["f0_scale"].numpy(), padded([ones[ii] if rows[ii] is None else rows[ii] for ii in indices]))
    # formants all 1: no key; one item other than 1: the key in its micro-batch only
    for indices, control in control_rows(monkeypatch, formants=ones):
        assert control == {}
    shifts = [None, None, None, ramp(3, 1.2)]
    seen = 0
    for indices, control in control_rows(monkeypatch, formants=shifts):
        if 3 not in indices:
            assert control == {}
            continue
        seen += 1
        assert sorted(control) == ["formant"]
        assert np.array_equal(control["formant"].numpy(), padded([ones[ii] if shifts[ii] is None else shifts[ii] for ii in indices]))
    assert seen == 1
    # f0s mixed with None: padded with the last value, the mask int32; a micro-batch without contour runs without the keys
    f0s = [ramp(0, 100.0), None, None, None]
    keyed = 0
    for indices, control in control_rows(monkeypatch, f0s=f0s):
        if all(f0s[ii] is None for ii in indices):
            assert control == {}
            continue
        keyed += 1
        assert sorted(control) == ["f0_frames", "f0_item_mask"]
        assert np.array_equal(control["f0_frames"].numpy(), padded([ones[ii] if f0s[ii] is None else f0s[ii] for ii in indices]))
        assert control["f0_item_mask"].dtype == torch.int32
        assert control["f0_item_mask"].tolist() == [int(f0s[ii] is not None) for ii in indices]
    assert keyed == 1
    # all three together
    for indices, control in control_rows(monkeypatch, transpositions=rows, formants=shifts, f0s=f0s):
        want = {"f0_scale"} | ({"formant"} if 3 in indices else set())
        want |= {"f0_frames", "f0_item_mask"} if any(f0s[ii] is not None for ii in indices) else set()
        assert set(control) == want
        assert np.array_equal(control["f0_scale"].numpy(), padded([ones[ii] if rows[ii] is None else rows[ii] for ii in indices]))
        if "formant" in control:
            assert np.array_equal(control["formant"].numpy(), padded([ones[ii] if shifts[ii] is None else shifts[ii] for ii in indices]))
        if "f0_frames" in control:
            assert np.array_equal(control["f0_frames"].numpy(), padded([ones[ii] if f0s[ii] is None else f0s[ii] for ii in indices]))
            assert control["f0_item_mask"].tolist() == [int(f0s[ii] is not None) for ii in indices]


@pytest.mark.parametrize("name", ["transpositions", "formants", "f0s"])
def test_a_row_of_the_wrong_shape_is_refused_by_argument_and_item(monkeypatch, name):
    rows = [None, None, np.full(4, 110.0, np.float32), None]              # item 2 has 5 frames
    with pytest.raises(ValueError, match=rf"{name}\[2\].*5"):
        control_rows(monkeypatch, **{name: rows})


# ------------------------------------------------------------------------------------------------------------------------
# the argv of a rank
# ------------------------------------------------------------------------------------------------------------------------
def load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(BIN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def words_of(action):
    """A command-line value for the option that differs from its default, from the action alone."""
    if action.nargs == 0:
        return []
    if action.choices:
        return [next(cc for cc in action.choices if cc != action.default)]
    if action.nargs == "+":
        return ["one.x", "two.x"]
    for text in ("3", "1.75", "word"):
        try:
            value = action.type(text) if action.type else text
        except Exception:        # noqa: BLE001 -- whatever this type refuses: the next word
            continue
        if value != action.default:
            return [text]
    raise AssertionError(f"no value found for {action.option_strings}")


# options that exclude each other at parse time: every line leaves one side out
WITHOUT = {"transform_audio": [("align_to", "align_to_dir"), ("time_stretch", "time_stretch_file", "align_to_dir"),
                               ("time_stretch", "time_stretch_file", "align_to")],
           "resynth_mel": [()]}


@pytest.mark.parametrize("tool", ["transform_audio", "resynth_mel"])
def test_rank_argv_round_trip(tool):
    from mbexwn_vocoder_amd.cli import rank_argv
    parser = load_tool(tool).make_parser()
    options = [aa for aa in parser._actions if aa.option_strings and aa.dest != "help"]
    positional = [aa for aa in parser._actions if not aa.option_strings]
    front = [ww for aa in positional for ww in (["a.x", "b.x"] if aa.nargs == "+" else ["model"])]
    required = [ww for aa in options if aa.required for ww in [aa.option_strings[0], *words_of(aa)]]
    lines = [front + required]
    covered = set()
    for without in WITHOUT[tool]:
        lines.append(front + [ww for aa in options if aa.dest not in without for ww in [aa.option_strings[0], *words_of(aa)]])
        covered |= {aa.dest for aa in options} - set(without)
    assert covered == {aa.dest for aa in options}                   # every option, a future one included, is set in some line
    for without, line in zip([None] + WITHOUT[tool], lines):
        parent = vars(parser.parse_args(line))
        if without is not None:                                     # the line does set what it names
            assert all(parent[aa.dest] != aa.default for aa in options if aa.dest not in without)
        files = [ww for aa in positional for ww in (parent[aa.dest] if aa.nargs == "+" else [parent[aa.dest]])]
        argv = rank_argv(parser, parent, files)
        assert all(isinstance(ww, str) for ww in argv)
        rank = vars(parser.parse_args(argv))
        for name in set(parent) - {"gpus", "rank", "job"}:
            assert rank[name] == parent[name], (name, argv)
        assert (rank["gpus"], rank["rank"], rank["job"]) == (1, None, None)


# ------------------------------------------------------------------------------------------------------------------------
# the pipeline under transform_audio and run_audio_job, on the host
# ------------------------------------------------------------------------------------------------------------------------
def voice(seconds, rate, f0, seed):
    tt = np.arange(int(seconds * rate)) / rate
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 3.0 * tt) ** 2
    noise = np.random.default_rng(seed).standard_normal(tt.size)
    return (0.3 * env * (np.sin(2 * np.pi * f0 * tt) + 0.5 * np.sin(4 * np.pi * f0 * tt)) + 0.01 * noise).astype(np.float32)


def test_the_pipeline_is_generate_mels_scale_mel_and_fill_by_hand(tmp_path):
    from mbexwn_vocoder_amd import f0decode, f0track
    from mbexwn_vocoder_amd.analysis import generate_mels
    from mbexwn_vocoder_amd.batched import analyse_for_synthesis
    from mbexwn_vocoder_amd.config import ModelDims, read_config
    from mbexwn_vocoder_amd.mel_inverter import MELInverter, create_synthetic_model_dir
    model = create_synthetic_model_dir(str(tmp_path / "model"), "SPEECH")
    inv = MELInverter.host_only(model)
    rows = ModelDims(read_config(os.path.join(model, "config.yaml"))).steps_per_frame
    sounds, rates = [voice(0.5, 24000, 140.0, 1), voice(0.5, 16000, 210.0, 2)], [24000, 16000]
    guide = voice(0.6, 24000, 140.0, 3)
    decode = f0decode.decode_params()
    options = dict(time_maps=[None, 1.5], guides=[guide, None], guide_rates=[24000, None], align_band_s=0.25)
    got = analyse_for_synthesis(inv, sounds, rates, f0_source="audio", f0_decode=decode, f0_fill="hold", on_device=False,
                                rows_per_frame=rows, who="test", **options)
    tracked, notes = [], {}
    dicts = generate_mels(sounds, rates, inv.preprocess_config, on_device=False, rows_per_frame=rows, f0_out=tracked,
                          f0_params=f0track.params(24000), f0_decode=decode, align_out=notes, **options)
    assert [dd["mell"].shape[1] for dd in dicts] == [49, 61]              # the guide's frames; 1.5 times 41 frames
    for ii in range(2):
        assert np.array_equal(got.scaled[ii], inv.scale_mel(dicts[ii])) and got.scaled[ii].dtype == np.float32
        assert np.array_equal(got.contours[ii], f0track.fill_tracked(tracked[ii][0], "hold", 150.0))
        assert np.array_equal(got.tracked[ii][0], tracked[ii][0]) and np.array_equal(got.tracked[ii][1], tracked[ii][1])
    assert got.notes == notes and sorted(notes) == [0]
    # an item that cannot be aligned leaves the mels, the contours, the pairs and its note together; the other stays
    options["guides"] = [voice(0.1, 24000, 140.0, 4), None]
    got = analyse_for_synthesis(inv, sounds, rates, f0_source="audio", f0_decode=decode, f0_fill="hold", on_device=False,
                                rows_per_frame=rows, who="test", **options)
    assert got.scaled[0] is None and got.contours[0] is None and got.tracked[0] is None and "error" in got.notes[0]
    assert np.array_equal(got.scaled[1], inv.scale_mel(dicts[1])) and np.array_equal(got.tracked[1][0], tracked[1][0])
    # the pitch options are checked once, under the caller's name
    for bad, what in ((dict(f0_source="file"), "test: f0_source"), (dict(f0_decode=decode), "test: f0_decode"),
                      (dict(f0_fill="hold"), "test: f0_fill")):
        with pytest.raises(ValueError, match=what):
            analyse_for_synthesis(inv, sounds, rates, on_device=False, rows_per_frame=rows, who="test", **bad)

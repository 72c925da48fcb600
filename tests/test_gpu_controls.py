"""The per-frame controls where they meet: pitch (mbx_forward_options.f0_frames / f0_scale / f0_item_mask) and formant
(mbxe_forward: env_factor) in ONE call.  Offline: a ragged batch with a mixed item mask -- one launch group then runs the F0-net
for some items on the rows as they came and the VTF and conditioning chains on the warped rows -- on the SMALL model, its
force_causal and RMS-normalising variants and the two-block geometry, under the default convolution form and under F(2,3),
against envelope.warp_envelope_host (bits), the float64 oracle composed in tests/control_reference.py (the end-to-end bar), the
two-step route (bits) and the single items (bits).  Streams: every combination of control rows side by side, the two switches of
the stage layout at different ticks of one run under graph replay, a causal and a normalising model -- all against the offline
forward of the item alone, bit for bit."""
import functools

import numpy as np
import pytest

import control_reference as cref
import test_gpu_parity as parity
import test_gpu_wavenet_blocks as tblk
from helpers import build_case, synthetic_inputs
from mbexwn_vocoder_amd.envelope import channel_centres, warp_envelope_host

pytestmark = pytest.mark.gpu

_MB = "mbexwn_config:"
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 5}
MODELS = {
    "small": ("SPEECH", SMALL),
    "causal": ("SPEECH", dict(SMALL, **{_MB + "force_causal": True})),
    "normmel": ("SPEECH", dict(SMALL, **{_MB + "normalize_rms_from_mell": True, _MB + "normalize_rms_num_smooth_iters": 1})),
    "blocks": tblk.GEOMETRIES["blocks"],
}
FORMS = {"default": {}, "f23": {"conv_form": "f23"}}
N_FRAMES = (21, 8, 1)              # as in tests/test_gpu_pitch_control.py: several blocks of pulse samples, a short item, one frame
MASK = (1, 0, 1)                   # item 1 keeps the F0-net: it runs on the unwarped rows beside the chains on the warped ones
F0_BAR = 1e-3                      # Hz: what tests/test_gpu_configs.py holds an F0-net contour to
CASES = [(model, form) for model in MODELS for form in FORMS]

_ENGINES = {}


def _dev(array):
    import torch
    return torch.as_tensor(np.ascontiguousarray(array)).cuda()


def bits(array):
    return np.ascontiguousarray(array, dtype=np.float32).view(np.uint32)


def _engine(model, form):
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    if (model, form) not in _ENGINES:
        _ENGINES[model, form] = MBExWNEngine(*build_case(*MODELS[model]), **FORMS[form])
    return _ENGINES[model, form]


def _chain_stage(eng):
    """The rows the mel-rate chains read, of the last forward: the input, or the stage "mel_norm" of a normalising model"""
    return eng.stage("mel_norm").cpu().numpy() if eng.normalizes_rms else None


@functools.lru_cache(maxsize=None)
def _run(model, form):
    """One model under one form: the inputs, the forward with the pitch control only, the combined forward and its stages."""
    eng = _engine(model, form)
    d = eng.dims
    B, T = len(N_FRAMES), max(N_FRAMES)
    mel, noise = synthetic_inputs(8100, B, T, steps_per_frame=d.wn_in_rows_per_frame)
    rng = np.random.default_rng(8101)
    frames = rng.uniform(80.0, 400.0, size=(B, T)).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, size=(B, T)).astype(np.float32)
    phi = cref.formant_rows(rng, B, T)
    phi[:, 0] = (1.3, 0.75, 1.4)                                      # (the one-frame item: never the copy alone)
    dev = {"mel": _dev(mel), "noise": _dev(noise), "n_frames": _dev(np.asarray(N_FRAMES, dtype=np.int32)), "frames": _dev(frames),
           "scale": _dev(scale), "mask": _dev(np.asarray(MASK, dtype=np.int32)), "phi": _dev(phi)}
    base = dict(n_frames=dev["n_frames"], noise=dev["noise"])
    pitch = dict(f0_frames=dev["frames"], f0_scale=dev["scale"], f0_item_mask=dev["mask"])
    out = {"mel": mel, "noise": noise, "frames": frames, "scale": scale, "phi": phi, "dev": dev, "base": base, "pitch": pitch}
    out["pitch_audio"] = eng.forward(dev["mel"], **base, **pitch).cpu().numpy()
    out["pitch_f0"] = eng.stage("f0").cpu().numpy()
    out["audio"] = eng.forward(dev["mel"], formant=dev["phi"], **base, **pitch).cpu().numpy()
    out["f0_dev"] = eng.stage("f0")
    out["f0"] = out["f0_dev"].cpu().numpy()
    out["mel_env"] = eng.stage("mel_env").cpu().numpy().reshape(B, T, -1)
    chain = _chain_stage(eng)
    out["chain_rows"] = mel if chain is None else chain.reshape(B, T, -1)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(model, item, contour_bytes):
    """The oracle's audio of one item of _run at its own length on a contour (the bytes of a float32 row): shared by the forms,
    whose contours are the same F0-net's.  The warped rows are warp_envelope_host -- whose bits the stage "mel_env" has -- of
    the item's own rows; for the normalising model of the rows the oracle's own normalisation gives, so that the engine's
    normalisation is inside the comparison."""
    cfg, raw, wt = build_case(*MODELS[model])
    run = _run(model, "default")
    nn = N_FRAMES[item]
    rpf = _engine(model, "default").dims.wn_in_rows_per_frame
    mel = run["mel"][item:item + 1, :nn]
    rows, _ = cref.chain_rows(cfg, mel)
    warped = warp_envelope_host(rows, run["phi"][item:item + 1, :nn], channel_centres(cfg["preprocess_config"]))
    contour = np.frombuffer(contour_bytes, dtype=np.float32)[None]
    return cref.controlled_oracle_audio(cfg, raw, wt, mel, run["noise"][item:item + 1, :nn * rpf], contour, env_rows=warped)[0]


@pytest.mark.parametrize("model,form", CASES, ids=[f"{mm}-{ff}" for mm, ff in CASES])
def test_pitch_keeps_its_bits_and_the_chains_read_the_warped_rows(model, form):
    """Stage "f0" of the combined call is that of the call without the formant shift, bit for bit, the masked-out item (whose
    F0-net shares its launches with chains that read other rows) included; stage "mel_env" is warp_envelope_host of the rows the
    chains read -- the stage "mel_norm" of the normalising model --, rows at or behind n_frames copies."""
    eng, run = _engine(model, form), _run(model, form)
    assert np.array_equal(bits(run["f0"]), bits(run["pitch_f0"]))
    assert not np.array_equal(run["audio"], run["pitch_audio"])                       # the shift does something
    centres = channel_centres(eng.config["preprocess_config"])
    want = warp_envelope_host(run["chain_rows"], run["phi"], centres, n_frames=N_FRAMES)
    assert np.array_equal(bits(run["mel_env"]), bits(want))
    for bb, nn in enumerate(N_FRAMES):
        assert np.array_equal(bits(run["mel_env"][bb, nn:]), bits(run["chain_rows"][bb, nn:])), bb
        assert not np.array_equal(run["mel_env"][bb, :nn], run["chain_rows"][bb, :nn]), bb
    if eng.normalizes_rms:
        assert not np.array_equal(run["chain_rows"], run["mel"])


@pytest.mark.parametrize("model,form", CASES, ids=[f"{mm}-{ff}" for mm, ff in CASES])
def test_audio_against_the_oracle(model, form):
    """Every item's audio at its own length within parity.E2E_TOL * max(1, |ref|) of controlled_oracle_audio on the float32
    warped rows and the stage's contour; the contour of the masked-out item within 1e-3 Hz of the one the oracle builds itself
    from the unwarped rows and the interpolated scale."""
    eng, run = _engine(model, form), _run(model, form)
    d = eng.dims
    hop, ppf = d.hop_size, d.pulse_per_frame
    cfg, raw, wt = build_case(*MODELS[model])
    for bb, nn in enumerate(N_FRAMES):
        ref = _oracle(model, bb, run["f0"][bb, :nn * ppf].tobytes())
        err = float(np.max(np.abs(run["audio"][bb, :nn * hop].astype(np.float64) - ref)))
        bar = parity.E2E_TOL * max(1.0, float(np.max(np.abs(ref))))
        print(f"\ncontrols {model}-{form}: item {bb} ({nn} frames) max |audio - oracle| {err:.3e}, bar {bar:.3e}")
        assert err <= bar, f"item {bb}: {err} > {bar}"
    for bb, (nn, take) in enumerate(zip(N_FRAMES, MASK)):
        if take:
            continue
        own = cref.oracle_contour(cfg, raw, wt, run["mel"][bb:bb + 1, :nn], run["scale"][bb:bb + 1, :nn])[0]
        err = float(np.max(np.abs(run["f0"][bb, :nn * ppf].astype(np.float64) - own)))
        print(f"controls {model}-{form}: item {bb} (keeps the F0-net) max |f0 - oracle's contour| {err:.3e} Hz, bar {F0_BAR:.1e}")
        assert err <= F0_BAR, f"item {bb}: contour {err} Hz from the oracle's"


@pytest.mark.parametrize("model,form", CASES, ids=[f"{mm}-{ff}" for mm, ff in CASES])
def test_two_step_route(model, form):
    """forward(mel = the warped rows, f0 = the stage's contour) equals the combined call bit for bit at every item's own length.
    The normalising model would normalise the warped rows again: its second step runs on the same weights without the
    normalisation, and is compared in front of the gain -- conditioning rows, cepstrum and excitation."""
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    eng, run = _engine(model, form), _run(model, form)
    d = eng.dims
    warped = _dev(run["mel_env"])
    if not eng.normalizes_rms:
        audio = eng.forward(warped, f0=run["f0_dev"], **run["base"]).cpu().numpy()
        for bb, nn in enumerate(N_FRAMES):
            assert np.array_equal(bits(audio[bb, :nn * d.hop_size]), bits(run["audio"][bb, :nn * d.hop_size])), bb
        return
    names = ("cond", "cepstrum", "excitation")
    eng.forward(run["dev"]["mel"], formant=run["dev"]["phi"], **run["base"], **run["pitch"])
    got = {name: eng.stage(name).cpu().numpy() for name in names}
    voice, over = MODELS[model]
    plain_over = {kk: vv for kk, vv in over.items() if "normalize_rms" not in kk}
    cfg, raw, wt = build_case(voice, over)
    twin = MBExWNEngine(build_case(voice, plain_over)[0], raw, wt, **FORMS[form])
    assert not twin.normalizes_rms
    twin.forward(warped, f0=run["f0_dev"], **run["base"])
    T = max(N_FRAMES)
    for name in names:
        ref = twin.stage(name).cpu().numpy()
        per = ref.shape[1] // T
        assert got[name].shape == ref.shape
        for bb, nn in enumerate(N_FRAMES):
            assert np.array_equal(bits(got[name][bb, :nn * per]), bits(ref[bb, :nn * per])), (name, bb)


@pytest.mark.parametrize("model,form", CASES, ids=[f"{mm}-{ff}" for mm, ff in CASES])
def test_neutral_controls_change_no_bit(model, form):
    """Formant all 1, scale all 1 and mask all 0 (the frames are given and taken by nobody): the plain forward, and the stage
    "mel_env" is a copy of the rows the chains read."""
    eng, run = _engine(model, form), _run(model, form)
    B, T = run["phi"].shape
    plain = eng.forward(run["dev"]["mel"], **run["base"]).cpu().numpy()
    plain_f0 = eng.stage("f0").cpu().numpy()
    ones = _dev(np.ones((B, T), dtype=np.float32))
    audio = eng.forward(run["dev"]["mel"], f0_frames=run["dev"]["frames"], f0_scale=ones,
                        f0_item_mask=_dev(np.zeros(B, dtype=np.int32)), formant=ones, **run["base"]).cpu().numpy()
    assert np.array_equal(bits(audio), bits(plain))
    assert np.array_equal(bits(eng.stage("f0").cpu().numpy()), bits(plain_f0))
    assert np.array_equal(bits(eng.stage("mel_env").cpu().numpy().reshape(B, T, -1)), bits(run["chain_rows"]))


@pytest.mark.parametrize("model", list(MODELS))
def test_items_alone_equal_their_slice_of_the_batch(model):
    """Under F(2,3): every item alone, with its own rows at its own length, equals its slice of the batch bit for bit."""
    eng, run = _engine(model, "f23"), _run(model, "f23")
    d = eng.dims
    rpf = d.wn_in_rows_per_frame
    for bb, nn in enumerate(N_FRAMES):
        one = slice(bb, bb + 1)
        audio = eng.forward(_dev(run["mel"][one, :nn]), noise=_dev(run["noise"][one, :nn * rpf]),
                            f0_frames=_dev(run["frames"][one, :nn]), f0_scale=_dev(run["scale"][one, :nn]),
                            f0_item_mask=_dev(np.asarray(MASK[one], dtype=np.int32)), formant=_dev(run["phi"][one, :nn])).cpu().numpy()
        assert np.array_equal(bits(audio[0]), bits(run["audio"][bb, :nn * d.hop_size])), f"item {bb}"
        assert np.array_equal(bits(eng.stage("f0").cpu().numpy()[0]), bits(run["f0"][bb, :nn * d.pulse_per_frame])), f"item {bb}"


# ------------------------------------------------------------------------------------------------------------------------
# streams: against the offline forward of the item alone with its own rows, on an engine pinned to F(2,3)
# ------------------------------------------------------------------------------------------------------------------------
def _vibrato(frames, step_at=None):
    """Transposition contour: vibrato of +-6 %, and a step to 1.5 from frame step_at on."""
    tt = np.arange(frames)
    contour = 1.0 + 0.06 * np.sin(2.0 * np.pi * tt / 9.0)
    if step_at is not None:
        contour[step_at:] *= 1.5
    return contour.astype(np.float32)


def _offline(eng, stream):
    """One item alone through the offline forward with its control rows (none: the plain forward)."""
    mel, noise, f0, scale, formant = stream
    extra = {name: _dev(rows[None]) for name, rows in (("f0_frames", f0), ("f0_scale", scale), ("formant", formant))
             if rows is not None}
    return eng.forward(_dev(mel[None]), noise=_dev(noise[None]), **extra).cpu().numpy()[0]


def _stream_set(lengths, seed, control):
    """control: {sid: (has f0 frames, transposition rows or None, formant rows or None)}"""
    rng = np.random.default_rng(seed)
    streams = {}
    for sid, ll in enumerate(lengths):
        mel, noise = synthetic_inputs(seed + 1 + sid, 1, ll)
        has_f0, scale, formant = control.get(sid, (False, None, None))
        f0 = rng.uniform(80.0, 400.0, size=ll).astype(np.float32) if has_f0 else None
        streams[sid] = (mel[0], noise[0], f0, scale, formant)
    return streams


def _formant(seed, frames):
    return cref.formant_rows(np.random.default_rng(seed), 1, frames)[0]


@pytest.mark.parametrize("chunk", [8, (6, 6, 7, 6, 7)], ids=["8", "80ms_schedule"])
def test_streams_side_by_side(chunk):
    """Transposition contour and formant; F0 frames, transposition and formant; formant only; no control -- four streams of
    97, 40, 8 and 23 frames in irregular packets of 1 to 12 frames, steady and whole-region ticks."""
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    streams = _stream_set([97, 40, 8, 23], 8200, {0: (False, _vibrato(97, 50), _formant(8210, 97)),
                                                  1: (True, _vibrato(40), _formant(8211, 40)),
                                                  2: (False, None, _formant(8212, 8))})
    off = _engine("small", "f23")
    offline = {sid: _offline(off, stream) for sid, stream in streams.items()}
    for sid in (0, 1, 2):                                               # every control does something
        mel, noise, f0, scale, formant = streams[sid]
        assert not np.array_equal(offline[sid], _offline(off, (mel, noise, f0, scale, None))), sid
    assert not np.array_equal(offline[0], _offline(off, streams[0][:3] + (None, streams[0][4])))
    syn = StreamingSynthesizer(_engine("small", "default"), chunk_frames=chunk)
    rng = np.random.default_rng(0)
    got, kinds, _ = cref.serve(syn, streams, lambda sid: int(rng.integers(1, 13)))
    assert kinds == {False, True}          # ticks with the per-layer WaveNet state carried, and whole-region ticks
    assert syn._control and syn._formant
    for sid in streams:
        assert got[sid].shape == offline[sid].shape
        assert np.array_equal(bits(got[sid]), bits(offline[sid])), f"stream {sid} differs from the offline synthesis"


def test_two_late_switches_under_graph_replay():
    """Three streams of 140 frames in packets of 8, no control at first.  Stream 2's formant leaves 1 at frame 64 (the ninth
    packet), stream 0's transposition leaves 1 at frame 96 (the thirteenth).  Each switch changes the stage layout of a tick:
    the steady run is left, that tick runs launch by launch, the graphs are captured anew.  Replayed ticks in front of the
    first switch, between the two and behind the second; graph-on equals graph-off equals offline."""
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    phi = np.ones(140, dtype=np.float32)
    phi[64:] = _formant(8310, 140 - 64)
    phi[64] = 1.3
    scale = np.ones(140, dtype=np.float32)
    scale[96:] = _vibrato(140 - 96) * np.float32(1.25)
    streams = _stream_set([140, 140, 140], 8300, {0: (False, scale, None), 2: (False, None, phi)})
    off = _engine("small", "f23")
    offline = {sid: _offline(off, stream) for sid, stream in streams.items()}
    seen = {}

    def run(use_graph):
        syn = StreamingSynthesizer(_engine("small", "default"), chunk_frames=8)
        syn.use_graph = use_graph
        assert not syn._control and not syn._formant
        count = {sid: 0 for sid in streams}

        def packets(sid):
            # (called once per push: the flags as they stand when stream 0's packet of a tick is pushed)
            if sid == 0:
                seen.setdefault(use_graph, []).append((count[0], syn._formant, syn._control))
            count[sid] += 1
            return 8

        got, _, replayed = cref.serve(syn, streams, packets, max_ticks=60)
        assert syn._formant and syn._control
        return got, syn.graph_ticks, replayed

    plain, n_plain, _ = run(False)
    graphed, n_graph, replayed = run(True)
    assert n_plain == 0 and replayed.count(True) == n_graph
    # stream 0 is pushed first in a tick: in front of packet 9 nothing is set, in front of packet 13 the formant alone
    flags = {packet: (formant, control) for packet, formant, control in seen[True]}
    assert flags[8] == (False, False) and flags[9] == (True, False) and flags[12] == (True, False) and flags[13] == (True, True)
    print(f"\ntwo switches: replayed per tick {['-' if rr is None else int(rr) for rr in replayed]}")
    assert True in replayed[:8] and replayed[8] is False, replayed
    assert True in replayed[9:12] and replayed[12] is False, replayed
    assert True in replayed[13:], replayed
    for sid in streams:
        assert np.array_equal(bits(graphed[sid]), bits(plain[sid])), f"stream {sid}: graph replay differs from the launch-by-launch ticks"
        assert np.array_equal(bits(graphed[sid]), bits(offline[sid])), f"stream {sid} differs from the offline synthesis"


def test_causal_model_stream_with_every_control():
    """force_causal SMALL pinned to F(2,3): one 40-frame stream with F0 frames, a transposition contour and a formant shift
    equals the same engine offline."""
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    eng = _engine("causal", "f23")
    assert eng.dims.wn_padding == "CAUSAL"
    streams = _stream_set([40], 8400, {0: (True, _vibrato(40, 20), _formant(8410, 40))})
    offline = _offline(eng, streams[0])
    assert not np.array_equal(offline, _offline(eng, streams[0][:4] + (None,)))
    syn = StreamingSynthesizer(eng, chunk_frames=8)
    assert syn.fe_carry and syn.layer_carry               # the front end comes from its ring, the layers carry their state
    rng = np.random.default_rng(1)
    got, _, _ = cref.serve(syn, streams, lambda sid: int(rng.integers(1, 13)))
    assert syn._formant and syn._control
    assert np.array_equal(bits(got[0]), bits(offline))


def test_normalising_model_stream_with_a_formant_shift():
    """RMS-normalising SMALL pinned to F(2,3): one 40-frame stream with a formant shift only.  A normalising model does not
    carry its front end in the ring (engine.frontend_carry_supported): every tick normalises its whole window and warps the
    normalised rows behind that, and the audio is still that of the whole-utterance run.  (The stream whose windows do come
    from the front-end ring while all three controls act is the causal one above.)"""
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    eng = _engine("normmel", "f23")
    assert eng.normalizes_rms
    streams = _stream_set([40], 8500, {0: (False, None, _formant(8510, 40))})
    offline = _offline(eng, streams[0])
    assert not np.array_equal(offline, _offline(eng, streams[0][:4] + (None,)))
    syn = StreamingSynthesizer(eng, chunk_frames=8)
    assert not syn.fe_carry
    rng = np.random.default_rng(2)
    got, _, _ = cref.serve(syn, streams, lambda sid: int(rng.integers(1, 13)))
    assert syn._formant and not syn._control
    assert np.array_equal(bits(got[0]), bits(offline))

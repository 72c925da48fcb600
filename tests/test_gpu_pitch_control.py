"""Per-frame F0 and transposition control on the device (mbx_forward_options.f0_frames / f0_scale / f0_item_mask): the
contour against mbx_lin_interp, the audio against the pulse-rate option and the float64 oracle, streams -- launch by launch
and as replayed graphs, SAME and causal padding -- against the offline forward, and the refusals."""
import ctypes

import numpy as np
import pytest

from helpers import build_case, synthetic_inputs

pytestmark = pytest.mark.gpu

SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 5}
PPF = 100                          # pulse samples per mel frame of the canonical configuration
N_FRAMES = (21, 8, 1)              # ragged batch: more than one block of pulse samples, a short item, the one-frame clamp
MASK = (1, 0, 1)


@pytest.fixture(scope="module")
def case():
    return build_case("SPEECH", SMALL)


@pytest.fixture(scope="module")
def engine(case):
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    return MBExWNEngine(*case)


@pytest.fixture(scope="module")
def offline_f23_engine(case):
    """Pinned to the convolution form the streams run (tests/test_gpu_streaming.py)."""
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    return MBExWNEngine(*case, conv_form="f23")


def _dev(array):
    import torch
    return torch.as_tensor(np.ascontiguousarray(array)).cuda()


@pytest.fixture(scope="module")
def ragged(engine):
    """The ragged batch of cases 1 and 2, run once: inputs, control rows, the "f0" stage and the audio of the controlled
    forward, the "f0" stage of the plain one."""
    assert engine.dims.pulse_per_frame == PPF
    T = max(N_FRAMES)
    mel, noise = synthetic_inputs(900, len(N_FRAMES), T)
    rng = np.random.default_rng(901)
    frames = rng.uniform(80.0, 400.0, size=(len(N_FRAMES), T)).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, size=(len(N_FRAMES), T)).astype(np.float32)
    dev = {"mel": _dev(mel), "noise": _dev(noise), "n_frames": _dev(np.asarray(N_FRAMES, dtype=np.int32)),
           "frames": _dev(frames), "scale": _dev(scale), "mask": _dev(np.asarray(MASK, dtype=np.int32))}
    engine.forward(dev["mel"], n_frames=dev["n_frames"], noise=dev["noise"])
    plain_f0 = engine.stage("f0").cpu().numpy()
    audio = engine.forward(dev["mel"], n_frames=dev["n_frames"], noise=dev["noise"], f0_frames=dev["frames"],
                           f0_scale=dev["scale"], f0_item_mask=dev["mask"]).cpu().numpy()
    f0_dev = engine.stage("f0")
    return {"mel": mel, "noise": noise, "frames": frames, "scale": scale, "dev": dev, "plain_f0": plain_f0, "audio": audio,
            "f0_dev": f0_dev, "f0": f0_dev.cpu().numpy()}


def _lin_interp(engine, row):
    """mbx_lin_interp of one item's values at the item's own length: (n,) -> (n * PPF,)"""
    return engine.lin_interp(_dev(row.astype(np.float32)[None, :, None]), PPF).cpu().numpy()[0, :, 0]


def test_contour(engine, ragged):
    """Stage "f0" of the controlled forward, bit for bit: LI(frames) * LI(scale) for the items that take the frames, the
    F0-net's contour * LI(scale) for the one that does not -- both interpolations by mbx_lin_interp at the item's own
    length, multiplied in float32 on the host.  The one-frame item interpolates towards itself."""
    for bb, (nn, take) in enumerate(zip(N_FRAMES, MASK)):
        li_s = _lin_interp(engine, ragged["scale"][bb, :nn])
        base = _lin_interp(engine, ragged["frames"][bb, :nn]) if take else ragged["plain_f0"][bb, :nn * PPF]
        want = base.astype(np.float32) * li_s.astype(np.float32)
        got = ragged["f0"][bb, :nn * PPF]
        assert want.dtype == np.float32 and np.array_equal(got, want), f"item {bb}: {np.max(np.abs(got - want))}"
    # the clamp: with one frame both neighbours are that frame, and the weights of a sample sum to 1 in float32
    one = np.float32(ragged["frames"][2, 0])
    li_one = _lin_interp(engine, ragged["frames"][2, :1])
    assert np.max(np.abs(li_one - one)) <= np.spacing(one)
    assert np.array_equal(ragged["f0"][2, :PPF], li_one * _lin_interp(engine, ragged["scale"][2, :1]))
    # without a mask every item takes the frames, and the F0-net does not run: same contour for the masked items
    engine.forward(ragged["dev"]["mel"], n_frames=ragged["dev"]["n_frames"], noise=ragged["dev"]["noise"],
                   f0_frames=ragged["dev"]["frames"], f0_scale=ragged["dev"]["scale"])
    all_frames = engine.stage("f0").cpu().numpy()
    for bb, nn in enumerate(N_FRAMES):
        want = _lin_interp(engine, ragged["frames"][bb, :nn]) * _lin_interp(engine, ragged["scale"][bb, :nn])
        assert np.array_equal(all_frames[bb, :nn * PPF], want)


def _oracle_audio(cfg, raw, wt, mel, noise, f0):
    """The float64 oracle's audio of one item (1, T hop) on a given pulse-rate contour: excitation from the contour, the
    STFT-domain envelope filter of the contour's lifter selection (the SMALL model has no RMS normalisation)."""
    from oracle import mbexwn_oracle as orc
    om = orc.OracleModel(cfg, raw, wt)
    T = mel.shape[1]
    mel64 = np.asarray(mel).astype(om.dtype)
    contour = np.asarray(f0, dtype=np.float32).astype(np.float64)
    exc = om.generate_excitation(mel64, contour, noise)
    out_len = contour.shape[1] * int(om.sample_rate // om.pulse_rate)
    return om.istft(om.stft(exc, T) * om.generate_specenv(mel64, contour), out_len)[:, :T * om.hop]


def test_audio_equals_the_pulse_rate_option_and_the_oracle(case, engine, ragged):
    """The frame-rate control is the same function as the pulse-rate option: feeding the controlled forward's own "f0"
    stage back as mbx_forward_options.f0 gives the same audio bit for bit, and that audio is within the suite's end-to-end
    bar 1e-4 * max(1, |ref|) of the float64 oracle run on that contour, item by item at its own length."""
    dev = ragged["dev"]
    again = engine.forward(dev["mel"], n_frames=dev["n_frames"], noise=dev["noise"], f0=ragged["f0_dev"]).cpu().numpy()
    hop = engine.dims.hop_size
    for bb, nn in enumerate(N_FRAMES):
        assert np.array_equal(ragged["audio"][bb, :nn * hop], again[bb, :nn * hop]), f"item {bb}"
    assert np.array_equal(ragged["audio"], again)
    cfg, raw, wt = case
    for bb, nn in enumerate(N_FRAMES):
        ref = _oracle_audio(cfg, raw, wt, ragged["mel"][bb:bb + 1, :nn], ragged["noise"][bb:bb + 1, :nn * 20],
                            ragged["f0"][bb:bb + 1, :nn * PPF])[0]
        err = float(np.max(np.abs(ragged["audio"][bb, :nn * hop] - ref)))
        bar = 1e-4 * max(1.0, float(np.max(np.abs(ref))))
        print(f"item {bb} ({nn} frames): max |audio - oracle| {err:.3e}, bar {bar:.3e}")
        assert err <= bar, f"item {bb}: {err} > {bar}"


def _vibrato(frames, step_at=None):
    """Transposition contour: vibrato of +-6 %, and a step to 1.5 from frame step_at on."""
    tt = np.arange(frames)
    contour = 1.0 + 0.06 * np.sin(2.0 * np.pi * tt / 9.0)
    if step_at is not None:
        contour[step_at:] *= 1.5
    return contour.astype(np.float32)


def _offline(eng, mel, noise, f0=None, scale=None):
    """One item alone through the offline forward with its control rows (none: the plain forward)."""
    extra = {}
    if f0 is not None:
        extra["f0_frames"] = _dev(f0[None])
    if scale is not None:
        extra["f0_scale"] = _dev(scale[None])
    return eng.forward(_dev(mel), noise=_dev(noise), **extra).cpu().numpy()[0]


def _serve(syn, streams, packets, max_ticks=400, join_late=None):
    """Push every stream's frames in packets and tick until all are finished.  streams: {sid: (mel (T, 80), noise, f0 rows
    or None, transposition rows or None)}; packets(sid) -> frames of the next packet; join_late: {sid: first tick}."""
    got = {sid: [] for sid in streams}
    pos = {sid: 0 for sid in streams}
    opened, kinds, replayed = set(), set(), []
    for tick in range(max_ticks):
        for sid, (mel, noise, f0, scale) in streams.items():
            if join_late and tick < join_late.get(sid, 0):
                continue
            if sid not in opened:
                syn.open(sid, f0="net" if f0 is None else "frames")
                opened.add(sid)
            lo = pos[sid]
            if lo < mel.shape[0]:
                hi = min(lo + packets(sid), mel.shape[0])
                syn.push(sid, mel[lo:hi], noise[lo * 20:hi * 20], last=hi == mel.shape[0],
                         f0=None if f0 is None else f0[lo:hi], transposition=None if scale is None else scale[lo:hi])
                pos[sid] = hi
        out = syn.tick()
        if out:
            kinds.add(syn.last_tick_layer_rows > 0)
        replayed.append(syn.last_tick_replayed if out else None)
        for sid, audio in out.items():
            got[sid].append(np.array(audio))
        if len(opened) == len(streams) and all(syn.finished(sid) for sid in streams):
            break
    return {sid: np.concatenate(vv) for sid, vv in got.items()}, kinds, replayed


def _stream_set(lengths, seed, control):
    """control: {sid: (has f0 frames, transposition contour or None)}"""
    rng = np.random.default_rng(seed)
    streams = {}
    for sid, ll in enumerate(lengths):
        mel, noise = synthetic_inputs(seed + 1 + sid, 1, ll)
        has_f0, scale = control.get(sid, (False, None))
        f0 = rng.uniform(80.0, 400.0, size=ll).astype(np.float32) if has_f0 else None
        streams[sid] = (mel[0], noise[0], f0, scale)
    return streams


@pytest.mark.parametrize("chunk", [8, (6, 6, 7, 6, 7)], ids=["8", "80ms_schedule"])
def test_streams_equal_offline(engine, offline_f23_engine, chunk):
    """A transposition contour (vibrato and a step), external frames times a contour, external frames only and no control,
    side by side in irregular packets: every stream is bit-equal to the offline forward of that item alone with its own
    control rows (none for the stream without control: the factor 1 it gets in the batch changes no bit)."""
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    lengths = [97, 40, 8, 23]
    streams = _stream_set(lengths, 1000, {0: (False, _vibrato(97, 50)), 1: (True, _vibrato(40)), 2: (True, None)})
    offline = {sid: _offline(offline_f23_engine, mel[None], noise[None], f0, scale)
               for sid, (mel, noise, f0, scale) in streams.items()}
    plain = _offline(offline_f23_engine, streams[0][0][None], streams[0][1][None])
    assert not np.array_equal(plain, offline[0])                     # the control does something
    syn = StreamingSynthesizer(engine, chunk_frames=chunk)
    rng = np.random.default_rng(0)
    got, kinds, _ = _serve(syn, streams, lambda sid: int(rng.integers(1, 13)))
    assert kinds == {False, True}          # ticks with the per-layer WaveNet state carried, and whole-region ticks
    for sid in streams:
        assert got[sid].shape == offline[sid].shape
        assert np.array_equal(got[sid], offline[sid]), f"stream {sid} differs from the offline synthesis"


@pytest.mark.parametrize("from_start", [True, False], ids=["controlled_from_the_start", "first_control_at_frame_64"])
def test_graph_replay(engine, offline_f23_engine, from_start):
    """The set-up of test_steady_ticks_replay_a_graph_and_stay_bit_equal with control: the replayed graphs upload the
    control rows of the whole windows with the tick's other inputs.  Stream 2's transposition leaves 1 at frame 64 only: the
    frames its windows share with earlier ticks come from the front-end ring, which therefore must hold the unscaled
    contour.  With no other control before that, the steady run recorded without the control arguments is left there and
    captured anew."""
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    late = np.ones(93, dtype=np.float32)
    late[64:] = _vibrato(93 - 64) * np.float32(1.25)
    control = {2: (False, late)}
    if from_start:
        control.update({0: (False, _vibrato(140, 50)), 1: (True, _vibrato(140))})
    # (first control at frame 64: three streams from the first tick on, so that steady ticks are replayed before it)
    streams = _stream_set([140, 140, 93, 140] if from_start else [140, 140, 93], 2000, control)
    offline = {sid: _offline(offline_f23_engine, mel[None], noise[None], f0, scale)
               for sid, (mel, noise, f0, scale) in streams.items()}

    def run(use_graph):
        syn = StreamingSynthesizer(engine, chunk_frames=8)
        syn.use_graph = use_graph
        got, _, replayed = _serve(syn, streams, lambda sid: 8, max_ticks=60, join_late={3: 4} if from_start else None)
        return got, syn.graph_ticks, replayed

    plain, n_plain, _ = run(False)
    graphed, n_graph, replayed = run(True)
    assert n_plain == 0 and n_graph >= 6
    assert replayed.count(True) == n_graph
    if not from_start:
        # frame 64 arrives with the ninth packet: replayed ticks in front of it, that tick launch by launch (the run
        # recorded without the control arguments was left), replayed ticks again behind it
        assert True in replayed[:8] and replayed[8] is False and True in replayed[9:]
    for sid in streams:
        assert np.array_equal(graphed[sid], plain[sid]), f"stream {sid}: graph replay differs from the launch-by-launch ticks"
        assert np.array_equal(graphed[sid], offline[sid]), f"stream {sid} differs from the offline synthesis"


def test_causal_model_stream():
    """force_causal SMALL model pinned to F(2,3): one 40-frame stream with a transposition contour equals the same engine
    offline."""
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    eng = MBExWNEngine(*build_case("SPEECH", dict(SMALL, **{"mbexwn_config:force_causal": True})), conv_form="f23")
    streams = _stream_set([40], 3000, {0: (False, _vibrato(40, 20))})
    mel, noise, f0, scale = streams[0]
    offline = _offline(eng, mel[None], noise[None], f0, scale)
    assert not np.array_equal(offline, _offline(eng, mel[None], noise[None]))
    syn = StreamingSynthesizer(eng, chunk_frames=8)
    rng = np.random.default_rng(1)
    got, _, _ = _serve(syn, streams, lambda sid: int(rng.integers(1, 13)))
    assert np.array_equal(got[0], offline)


def test_refusals(engine, ragged):
    import torch
    from mbexwn_vocoder_amd.engine import mbx_forward_options
    dev = ragged["dev"]
    base = {"n_frames": dev["n_frames"], "noise": dev["noise"]}
    B, T = ragged["frames"].shape
    with pytest.raises(ValueError):
        engine.forward(dev["mel"], f0=ragged["f0_dev"], f0_frames=dev["frames"], **base)
    with pytest.raises(ValueError):
        engine.forward(dev["mel"], transposition=1.5, f0_scale=dev["scale"], **base)
    with pytest.raises(ValueError):
        engine.forward(dev["mel"], transposition=1.5, f0_frames=dev["frames"], **base)
    with pytest.raises(ValueError):
        engine.forward(dev["mel"], f0_item_mask=dev["mask"], **base)                          # a mask without frames
    with pytest.raises(ValueError):
        engine.forward(dev["mel"], f0_frames=dev["frames"][:, :-1], **base)                   # wrong shape
    with pytest.raises(ValueError):
        engine.forward(dev["mel"], f0_scale=dev["scale"].reshape(-1), **base)
    with pytest.raises(ValueError):
        engine.forward(dev["mel"], f0_frames=dev["frames"].double(), **base)                  # wrong dtype
    with pytest.raises(ValueError):
        engine.forward(dev["mel"], f0_frames=dev["frames"], f0_item_mask=dev["mask"].long(), **base)
    with pytest.raises(ValueError):
        engine.forward(dev["mel"], f0_frames=dev["frames"], f0_item_mask=dev["mask"][:2], **base)
    with pytest.raises(ValueError):
        engine.forward(dev["mel"], f0_scale=dev["scale"].cpu(), **base)                       # wrong device
    with pytest.raises(ValueError):
        engine.forward(dev["mel"], f0_frames=ragged["frames"], **base)                        # not a tensor
    # the C ABI itself: the rules of mbx_forward_ex and its two struct sizes
    out = torch.empty((B, T * engine.dims.hop_size), dtype=torch.float32, device="cuda")
    ws, need = engine._get_workspace(B, T)

    def call(opt):
        return engine._lib.mbx_forward_ex(engine._handle, dev["mel"].data_ptr(), dev["n_frames"].data_ptr(), B, T,
                                          dev["noise"].data_ptr(), out.data_ptr(), ws.data_ptr(), need, ctypes.byref(opt),
                                          engine._stream())

    def options(size=ctypes.sizeof(mbx_forward_options), **fields):
        opt = mbx_forward_options()
        opt.struct_size, opt.transposition = size, 1.0
        for kk, vv in fields.items():
            setattr(opt, kk, vv)
        return opt

    invalid = 1                                                      # MBX_ERR_INVALID_ARGUMENT
    frames_p, scale_p, mask_p = dev["frames"].data_ptr(), dev["scale"].data_ptr(), dev["mask"].data_ptr()
    assert call(options(f0=ragged["f0_dev"].data_ptr(), f0_frames=frames_p)) == invalid
    assert call(options(transposition=1.5, f0_scale=scale_p)) == invalid
    assert call(options(transposition=1.5, f0_frames=frames_p)) == invalid
    assert call(options(f0_item_mask=mask_p)) == invalid
    old_size = mbx_forward_options.f0_frames.offset
    assert call(options(size=old_size + 4)) == invalid and call(options(size=0)) == invalid
    assert call(options(size=ctypes.sizeof(mbx_forward_options) + 8)) == invalid
    # the old size: the three fields are not read (a mask without frames would be refused otherwise), the plain forward runs
    assert call(options(size=old_size, f0_item_mask=mask_p)) == 0
    torch.cuda.synchronize()
    plain = engine.forward(dev["mel"], **base)
    assert torch.equal(out, plain)
    assert call(options(f0_frames=frames_p, f0_scale=scale_p, f0_item_mask=mask_p)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ragged["audio"])


def test_synth_from_mel_takes_the_control(tmp_path):
    """MELInverter.synth_from_mel(f0=, transposition=): a scalar transposition is the transposition_factor of
    infer_components (same bits), per-frame values go through f0_frames / f0_scale; malformed values are refused."""
    import torch
    from mbexwn_vocoder_amd.mel_inverter import MELInverter, create_synthetic_model_dir
    small3 = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 3}
    inv = MELInverter(create_synthetic_model_dir(str(tmp_path / "speech_small"), "SPEECH", **small3))
    T = 19
    mell, noise = synthetic_inputs(4000, 1, T)
    plain = inv.synth_from_mel(mell, noise=noise)
    assert np.array_equal(plain, inv.synth_from_mel(mell, noise=noise, transposition=1.0))
    shifted = inv.synth_from_mel(mell, noise=noise, transposition=1.5)
    inv.model.infer_components(mell, synth_length=T * inv.hop_size, transposition_factor=1.5, noise=noise)
    assert shifted.shape == plain.shape and np.array_equal(shifted, inv.model.last_audio.cpu().numpy().ravel())
    assert not np.array_equal(shifted, plain)
    rng = np.random.default_rng(4001)
    f0 = rng.uniform(80.0, 400.0, size=T).astype(np.float32)
    scale = _vibrato(T, 10)
    for kw, extra in (({"f0": f0}, {"f0_frames": _dev(f0[None])}),
                      ({"transposition": scale}, {"f0_scale": _dev(scale[None])}),
                      ({"f0": f0, "transposition": scale}, {"f0_frames": _dev(f0[None]), "f0_scale": _dev(scale[None])}),
                      ({"f0": f0, "transposition": 1.25},
                       {"f0_frames": _dev(f0[None]), "f0_scale": torch.full((1, T), 1.25, device="cuda")})):
        want = inv.model.forward(_dev(mell), noise=_dev(noise), **extra).cpu().numpy().ravel()
        assert np.array_equal(inv.synth_from_mel(mell, noise=noise, **kw), want), sorted(kw)
    for kw in ({"f0": f0[:-1]}, {"transposition": scale[:-1]}, {"f0": 200.0}, {"f0": -f0}, {"transposition": 0.0},
               {"transposition": np.where(np.arange(T) == 3, np.nan, scale)}):
        with pytest.raises(ValueError):
            inv.synth_from_mel(mell, noise=noise, **kw)


def test_ring_keeps_the_unscaled_contour(engine):
    """The control runs behind the front-end ring (the set-up of test_frontend_ring_equals_whole_window_and_checks_its_
    arguments): with a transposition the ring's F0 lane holds the F0-net's own contour while the window's contour is the
    scaled one; with f0_frames and no mask the F0-net does not run and the lane is not written at all."""
    import torch
    from mbexwn_vocoder_amd.streaming import pack_state
    assert engine.frontend_carry_supported
    B, T, ring_frames, sentinel = 2, 40, 64, 7.0
    mel, noise = synthetic_inputs(61, B, T)
    mel_d, noise_d = _dev(mel), _dev(noise)
    st = torch.as_tensor(np.stack([pack_state(0.0, 0.0, 0, 4 * 100, -1)] * B)).cuda()
    act = torch.full((B,), T - 12, dtype=torch.int32, device="cuda")
    store = torch.zeros((4, 8, 15), dtype=torch.float32, device="cuda")
    slots, pos = (2, 1), (10, 50)                                             # (one ring position wraps)
    desc = torch.tensor([[ss, 0, 0, 0, 0] for ss in slots], dtype=torch.int32, device="cuda")
    pos_d = torch.tensor(pos, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(62)
    frames = rng.uniform(80.0, 400.0, size=(B, T)).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, size=(B, T)).astype(np.float32)

    def run(**control):
        ring = torch.full((4, ring_frames, engine.frontend_frame_floats), sentinel, dtype=torch.float32, device="cuda")
        engine.forward(mel_d, noise=noise_d, stream_state=st, active=(8, act, T - 12), carry=(store, desc),
                       frontend=(ring, pos_d, 0, 0), **control)
        lanes = np.stack([ring[ss, [(pp + ff) % ring_frames for ff in range(T)]].cpu().numpy() for ss, pp in zip(slots, pos)])
        return engine.stage("f0").cpu().numpy(), lanes                        # lanes: (B, T, floats per frame)

    plain_f0, plain_lanes = run()
    assert np.array_equal(plain_lanes[:, :, -PPF:].reshape(B, -1), plain_f0) and not np.any(plain_lanes == sentinel)
    scaled_f0, scaled_lanes = run(f0_scale=_dev(scale))
    assert np.array_equal(scaled_lanes, plain_lanes)                         # the ring does not see the control
    want = np.stack([plain_f0[bb] * _lin_interp(engine, scale[bb]) for bb in range(B)])
    assert np.array_equal(scaled_f0, want) and not np.array_equal(scaled_f0, plain_f0)
    frames_f0, frames_lanes = run(f0_frames=_dev(frames))
    assert np.array_equal(frames_f0, np.stack([_lin_interp(engine, frames[bb]) for bb in range(B)]))
    assert np.all(frames_lanes[:, :, -PPF:] == sentinel)                      # the F0 lane: neither computed nor stored
    assert np.array_equal(frames_lanes[:, :, :-PPF], plain_lanes[:, :, :-PPF])
    masked_f0, masked_lanes = run(f0_frames=_dev(frames), f0_item_mask=_dev(np.asarray([0, 1], dtype=np.int32)))
    assert np.array_equal(masked_lanes, plain_lanes)                         # with a mask the net runs for every item
    assert np.array_equal(masked_f0[0], plain_f0[0]) and np.array_equal(masked_f0[1], frames_f0[1])

"""Formant shift on the device (include/mbexwn_envelope.h: mbxe_warp_envelope; mbx_forward_options.env_factor; DESIGN.md
section 6g): the kernel against its numpy restatement bit for bit, its memory contract and refusals, the forward -- the warped
rows reach the VTF and conditioning chains, the F0 chain keeps its bits --, streams against the offline forward, the tool."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from guarded import Guarded
from helpers import GOLDEN_CASES, build_case, synthetic_inputs
from mbexwn_vocoder_amd.envelope import channel_centres, warp_envelope_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 5}
SMALL3 = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 3}
NORM = dict(SMALL3, **{"mbexwn_config:normalize_rms_from_mell": True, "mbexwn_config:normalize_rms_num_smooth_iters": 1})
FACTORS = np.asarray([1.0, 0.5, 0.8, 1.25, 2.0, 1.0 + 2.0 ** -23], dtype=np.float32)
# (mel_channels, fmin, fmax): the canonical analysis, a narrow one, an odd small one, the smallest table
TABLES = {80: (0.0, 12000.0), 20: (50.0, 4000.0), 7: (0.0, 12000.0), 2: (0.0, 12000.0)}
# (batch, frames, n_frames): one element, one block that is not full, several blocks with a short and an empty item
SHAPES = [(1, 1, (1,)), (1, 2, (2,)), (3, 37, (37, 5, 0))]


def _dev(array):
    import torch
    return torch.as_tensor(np.ascontiguousarray(array)).cuda()


def bits(array):
    return np.ascontiguousarray(array, dtype=np.float32).view(np.uint32)


def _centres(n_mels):
    fmin, fmax = TABLES[n_mels]
    return channel_centres({"mel_channels": n_mels, "fmin": fmin, "fmax": fmax, "sample_rate": 24000})


class Call:
    """One raw call of mbxe_warp_envelope on a window of a longer buffer: item stride = frames * n_mels + 24 floats, the
    output between guard bands and pre-filled, so that what the call leaves alone keeps the fill."""

    def __init__(self, n_mels, batch, frames, counts, seed, fill="nan"):
        import torch
        from mbexwn_vocoder_amd.engine import load_library
        self.torch, self.lib = torch, load_library()
        self.n, self.batch, self.frames, self.stride = n_mels, batch, frames, frames * n_mels + 24
        rng = np.random.default_rng(seed)
        self.mel = np.clip(rng.normal(-5.0, 2.0, size=(batch, self.stride)), -11.5, 2.0).astype(np.float32)
        self.mel[0, 0] = -0.0
        self.factors = FACTORS[rng.integers(0, len(FACTORS), size=(batch, frames))]
        self.factors[:, 0] = FACTORS[1 + seed % 5]                        # (one frame: never the copy alone)
        self.counts = np.asarray(counts, dtype=np.int32)
        self.centres = _centres(n_mels)
        self.dev = {"mel": _dev(self.mel), "factors": _dev(self.factors), "counts": _dev(self.counts), "centres": _dev(self.centres)}
        self.out = Guarded("out", 4 * ((batch - 1) * self.stride + frames * n_mels), fill, device="cuda")

    def run(self, **kw):
        args = dict(mel=self.dev["mel"].data_ptr(), stride=self.stride, batch=self.batch, n_frames=self.dev["counts"].data_ptr(),
                    max_frames=self.frames, n_mels=self.n, centres=self.dev["centres"].data_ptr(),
                    factors=self.dev["factors"].data_ptr(), out=self.out.ptr)
        args.update(kw)
        status = self.lib.mbxe_warp_envelope(args["mel"], args["stride"], args["batch"], args["n_frames"], args["max_frames"],
                                             args["n_mels"], args["centres"], args["factors"], args["out"], None)
        self.torch.cuda.synchronize()
        return status

    def rows(self, array):
        """(batch, frames, n) of a flat (batch-strided) buffer"""
        flat = np.zeros(self.batch * self.stride, dtype=array.dtype)
        flat[:array.size] = array.reshape(-1)
        return flat.reshape(self.batch, self.stride)[:, :self.frames * self.n].reshape(self.batch, self.frames, self.n)

    def want(self):
        return warp_envelope_host(self.rows(self.mel), self.factors, self.centres, n_frames=self.counts)


@pytest.mark.parametrize("n_mels", sorted(TABLES))
def test_kernel_equals_the_host_restatement(n_mels):
    """mbxe_warp_envelope against envelope.warp_envelope_host, bit for bit, per-frame factors mixed from FACTORS; rows behind
    n_frames are copies; the guard bands around out and the floats between the items' windows keep the fill."""
    for seed, (batch, frames, counts) in enumerate(SHAPES):
        call = Call(n_mels, batch, frames, counts, seed=100 * n_mels + seed)
        assert call.run() == 0, call.lib.mbx_last_error()
        call.out.check()
        raw = call.out.view(call.torch.float32).cpu().numpy()
        got, want = call.rows(raw), call.want()
        assert np.array_equal(bits(got), bits(want)), (n_mels, batch, frames, float(np.nanmax(np.abs(got - want))))
        mel_rows = call.rows(call.mel)
        for bb, nn in enumerate(counts):
            assert np.array_equal(bits(got[bb, nn:]), bits(mel_rows[bb, nn:]))          # behind the item's end: copies
        gaps = np.zeros(call.batch * call.stride, dtype=np.int32)
        gaps[:raw.size] = raw.view(np.int32)
        assert np.all(gaps.reshape(batch, call.stride)[:-1, frames * n_mels:] == -1) or batch == 1     # between the windows: the fill
    # n_frames NULL: every item has max_frames frames
    call = Call(n_mels, 2, 5, (5, 5), seed=7)
    assert call.run(n_frames=None) == 0
    assert np.array_equal(bits(call.rows(call.out.view(call.torch.float32).cpu().numpy())), bits(call.want()))


def test_warp_envelope_device_needs_no_engine():
    """envelope.warp_envelope_device on its own (the library and a centre table, no model): a batch view with a batch stride of
    its own -- passed as it is, the row-stride path --, the factors 0.8, 1 and 1.25, a short item: the bits of
    warp_envelope_host."""
    from mbexwn_vocoder_amd.envelope import device_centres, warp_envelope_device
    batch, frames, n, counts = 2, 3, 80, (3, 1)
    analysis = {"mel_channels": n, "fmin": TABLES[n][0], "fmax": TABLES[n][1], "sample_rate": 24000}
    rng = np.random.default_rng(8)
    wide = np.clip(rng.normal(-5.0, 2.0, size=(batch, frames + 2, n)), -11.5, 2.0).astype(np.float32)
    factors = np.asarray([[0.8, 1.0, 1.25], [1.25, 0.8, 1.0]], dtype=np.float32)
    view = _dev(wide)[:, :frames]
    assert not view.is_contiguous() and view.stride(0) == (frames + 2) * n
    centres = device_centres(analysis, view.device)
    assert centres is device_centres(dict(analysis), view.device)                    # uploaded once
    got = warp_envelope_device(view, _dev(factors), centres, _dev(np.asarray(counts, dtype=np.int32)))
    assert got.stride() == view.stride()                       # (the call has one item stride for mel and out)
    got = got.cpu().numpy()
    want = warp_envelope_host(wide[:, :frames], factors, channel_centres(analysis), n_frames=counts)
    assert got.shape == (batch, frames, n) and np.array_equal(bits(got), bits(want))
    assert not np.array_equal(got[0, 0], wide[0, 0]) and np.array_equal(bits(got[1, 1:]), bits(wide[1, 1:frames]))


def test_kernel_refusals_leave_the_output_untouched():
    call = Call(80, 2, 6, (6, 3), seed=3, fill="huge")

    def why():
        return call.lib.mbx_last_error().decode()

    cases = [({name: None}, "null") for name in ("mel", "centres", "factors", "out")]
    cases += [({"n_mels": 1}, "n_mels"), ({"n_mels": 0}, "n_mels"), ({"max_frames": 0}, "max_frames"), ({"batch": -1}, "batch"),
              ({"batch": 65536}, "batch"), ({"stride": 6 * 80 - 1}, "stride"), ({"out": call.dev["mel"].data_ptr()}, "alias"),
              ({"out": call.dev["mel"].data_ptr() + 4 * 80}, "alias")]
    for kw, what in cases:
        assert call.run(**kw) == 1, kw                                   # MBX_ERR_INVALID_ARGUMENT
        assert why().startswith("warp envelope:") and what in why(), (kw, why())
        assert call.out.payload_untouched(), kw
        call.out.check()
    assert np.array_equal(call.dev["mel"].cpu().numpy(), call.mel)       # (the aliased calls wrote nothing either)
    assert call.run(batch=0) == 0 and call.out.payload_untouched()       # nothing to do
    assert call.run() == 0 and not call.out.payload_untouched()          # and the same buffers do run


# ------------------------------------------------------------------------------------------------------------------------
# the forward
# ------------------------------------------------------------------------------------------------------------------------
B, T, N_FRAMES = 2, 40, (40, 23)


def _factor_rows(seed, batch, frames):
    """Per-frame factors: a slow sweep between 0.8 and 1.25 with frames of exactly 1 and the extremes mixed in"""
    rng = np.random.default_rng(seed)
    rows = (1.0 + 0.22 * np.sin(2.0 * np.pi * (np.arange(frames)[None, :] / 17.0 + rng.uniform(size=(batch, 1))))).astype(np.float32)
    pick = rng.integers(0, 4 * len(FACTORS), size=(batch, frames))
    return np.where(pick < len(FACTORS), FACTORS[pick % len(FACTORS)], rows).astype(np.float32)


def _engine(case, **kw):
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    return MBExWNEngine(*case, conv_form="f23", batch_invariant=True, **kw)


@pytest.fixture(scope="module")
def case():
    return build_case("SPEECH", SMALL)


@pytest.fixture(scope="module")
def engine(case):
    return _engine(case)


@pytest.fixture(scope="module")
def runs(engine):
    """The forwards of the plain model, each run once: without a factor, with per-frame factors, with factors of 1."""
    mel, noise = synthetic_inputs(7100, B, T)
    phi = _factor_rows(7101, B, T)
    dev = {"mel": _dev(mel), "noise": _dev(noise), "n_frames": _dev(np.asarray(N_FRAMES, dtype=np.int32)), "phi": _dev(phi)}
    base = dict(n_frames=dev["n_frames"], noise=dev["noise"])
    out = {"mel": mel, "noise": noise, "phi": phi, "dev": dev, "base": base}
    out["plain"] = engine.forward(dev["mel"], **base).cpu().numpy()
    out["plain_f0"] = engine.stage("f0")
    out["plain_stages"] = {name: engine.stage(name).cpu().numpy() for name in ("cond", "cepstrum")}
    with pytest.raises(ValueError, match="unknown stage"):
        engine.stage("mel_env")                                          # published for calls with a factor only
    out["audio"] = engine.forward(dev["mel"], formant=dev["phi"], **base).cpu().numpy()
    out["stages"] = {name: engine.stage(name).cpu().numpy() for name in ("mel_env", "f0", "cond", "cepstrum")}
    out["ones"] = engine.forward(dev["mel"], formant=_dev(np.ones((B, T), dtype=np.float32)), **base).cpu().numpy()
    out["ones_env"] = engine.stage("mel_env").cpu().numpy()
    return out


def test_forward_warps_the_envelope_chains_and_keeps_the_pitch(engine, runs):
    centres = channel_centres(engine.config["preprocess_config"])
    want = warp_envelope_host(runs["mel"], runs["phi"], centres, n_frames=N_FRAMES)
    assert np.array_equal(bits(runs["stages"]["mel_env"]), bits(want.reshape(B, -1)))
    assert np.array_equal(bits(runs["stages"]["f0"]), bits(runs["plain_f0"].cpu().numpy()))       # the F0 chain: not one bit
    for name in ("cond", "cepstrum"):
        assert not np.array_equal(runs["stages"][name], runs["plain_stages"][name]), name         # the other chains moved
    assert not np.array_equal(runs["audio"], runs["plain"])
    # a factor of 1 on every frame: the rows are copies, the audio has the bits of the call without a factor
    assert np.array_equal(bits(runs["ones_env"]), bits(runs["mel"].reshape(B, -1)))
    assert np.array_equal(bits(runs["ones"]), bits(runs["plain"]))
    # and the same bits through the stand-alone binding
    alone = engine.warp_envelope(runs["dev"]["mel"], runs["dev"]["phi"], runs["dev"]["n_frames"]).cpu().numpy()
    assert np.array_equal(bits(alone), bits(want))


def test_forward_equals_a_plain_forward_of_the_host_warped_mel(engine, runs):
    """No RMS normalisation: the audio is, bit for bit, that of a plain forward of the host-warped mel which is given the
    first call's F0 contour from outside (the F0-net then does not run: the mel-rate launches group two chains, not three)."""
    centres = channel_centres(engine.config["preprocess_config"])
    warped = warp_envelope_host(runs["mel"], runs["phi"], centres, n_frames=N_FRAMES)
    audio = engine.forward(_dev(warped), f0=runs["plain_f0"], **runs["base"]).cpu().numpy()
    for name in ("cond", "cepstrum"):
        assert np.array_equal(bits(engine.stage(name).cpu().numpy()), bits(runs["stages"][name])), name
    hop = engine.dims.hop_size
    for bb, nn in enumerate(N_FRAMES):
        assert np.array_equal(bits(audio[bb, :nn * hop]), bits(runs["audio"][bb, :nn * hop])), bb


def test_forward_refusals(engine, runs):
    import torch
    from mbexwn_vocoder_amd.engine import mbx_forward_options
    dev, base = runs["dev"], runs["base"]
    for bad in (dev["phi"][:, :-1], dev["phi"].reshape(-1), dev["phi"].double(), dev["phi"].cpu(), runs["phi"]):
        with pytest.raises(ValueError, match="formant"):
            engine.forward(dev["mel"], formant=bad, **base)
    # the C entry point itself: mbxe_forward = the arguments of mbx_forward_ex (options may be NULL) and the three pointers
    out = torch.empty((B, T * engine.dims.hop_size), dtype=torch.float32, device="cuda")
    ws, need = engine._get_workspace(B, T)
    scratch = torch.empty((B, T, 80), dtype=torch.float32, device="cuda")
    centres = engine._envelope_centres()

    def call(opt=None, env_factor=None, env_centres=None, env_mel=None):
        status = engine._lib.mbxe_forward(engine._handle, dev["mel"].data_ptr(), dev["n_frames"].data_ptr(), B, T,
                                          dev["noise"].data_ptr(), out.data_ptr(), ws.data_ptr(), need,
                                          ctypes.byref(opt) if opt is not None else None, env_factor, env_centres, env_mel,
                                          engine._stream())
        torch.cuda.synchronize()
        return status

    def options(size=ctypes.sizeof(mbx_forward_options)):
        opt = mbx_forward_options()
        opt.struct_size, opt.transposition = size, 1.0
        return opt

    all3 = dict(env_factor=dev["phi"].data_ptr(), env_centres=centres.data_ptr(), env_mel=scratch.data_ptr())
    for name in all3:                                                     # all three or none
        assert call(**{kk: vv for kk, vv in all3.items() if kk != name}) == 1, name
        assert "go together" in engine._lib.mbx_last_error().decode()
    assert call(**dict(all3, env_mel=dev["mel"].data_ptr())) == 1 and "alias" in engine._lib.mbx_last_error().decode()
    # the struct sizes are those of mbx_forward_ex, and with all three NULL the call is that call
    old = mbx_forward_options.f0_frames.offset
    assert call(options(size=old + 4), **all3) == 1 and call(options(size=ctypes.sizeof(mbx_forward_options) + 8)) == 1
    for opt in (None, options(), options(size=old)):
        assert call(opt) == 0
        assert np.array_equal(bits(out.cpu().numpy()), bits(runs["plain"]))
        assert call(opt, **all3) == 0
        assert np.array_equal(bits(out.cpu().numpy()), bits(runs["audio"]))


def test_rms_normalised_model_warps_the_normalised_mel():
    """With RMS normalisation the warp acts on the normalised mel: "mel_env" is the host restatement of the stage "mel_norm",
    and the conditioning rows and the cepstrum are those of a model without normalisation fed with that warped mel."""
    cfg, raw, wt = build_case("SPEECH", NORM)
    eng = _engine((cfg, raw, wt))
    assert eng.normalizes_rms
    mel, noise = synthetic_inputs(7200, B, T)
    phi = _factor_rows(7201, B, T)
    counts = _dev(np.asarray(N_FRAMES, dtype=np.int32))
    eng.forward(_dev(mel), n_frames=counts, noise=_dev(noise), formant=_dev(phi))
    got = {name: eng.stage(name).cpu().numpy() for name in ("mel_norm", "mel_env", "cond", "cepstrum")}
    want = warp_envelope_host(got["mel_norm"].reshape(B, T, -1), phi, channel_centres(cfg["preprocess_config"]), n_frames=N_FRAMES)
    assert np.array_equal(bits(got["mel_env"]), bits(want.reshape(B, -1)))
    assert not np.array_equal(got["mel_norm"], mel.reshape(B, -1))
    plain_cfg = build_case("SPEECH", SMALL3)[0]
    plain = _engine((plain_cfg, raw, wt))
    plain.forward(_dev(want), n_frames=counts, noise=_dev(noise))
    nf = np.asarray(N_FRAMES)
    for name in ("cond", "cepstrum"):
        ref, have = plain.stage(name).cpu().numpy(), got[name]
        per = ref.shape[1] // T
        for bb in range(B):
            assert np.array_equal(bits(have[bb, :nf[bb] * per]), bits(ref[bb, :nf[bb] * per])), (name, bb)


def test_later_blocks_follow_the_warped_rows():
    """Several WaveNet blocks: the conditioning chains of the blocks behind the first one read the warped rows too."""
    voice, over, _, _ = GOLDEN_CASES["blocks"]
    case = build_case(voice, over)
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    eng = MBExWNEngine(*case)
    frames = 12
    mel, noise = synthetic_inputs(7300, 2, frames, steps_per_frame=eng.dims.wn_in_rows_per_frame)
    phi = _factor_rows(7301, 2, frames)
    counts = (frames, 7)
    base = dict(n_frames=_dev(np.asarray(counts, dtype=np.int32)), noise=_dev(noise))
    eng.forward(_dev(mel), **base)
    unwarped = eng.stage("cond1").cpu().numpy()
    audio = eng.forward(_dev(mel), formant=_dev(phi), **base).cpu().numpy()
    got = {name: eng.stage(name).cpu().numpy() for name in ("mel_env", "cond", "cond1")}
    f0 = eng.stage("f0")
    warped = warp_envelope_host(mel, phi, channel_centres(case[0]["preprocess_config"]), n_frames=counts)
    assert np.array_equal(bits(got["mel_env"]), bits(warped.reshape(2, -1)))
    ref_audio = eng.forward(_dev(warped), f0=f0, **base).cpu().numpy()
    for name in ("cond", "cond1"):
        ref = eng.stage(name).cpu().numpy()
        per = ref.shape[1] // frames
        for bb, nn in enumerate(counts):
            assert np.array_equal(bits(got[name][bb, :nn * per]), bits(ref[bb, :nn * per])), (name, bb)
    assert not np.array_equal(got["cond1"], unwarped)
    hop = eng.dims.hop_size
    for bb, nn in enumerate(counts):
        assert np.array_equal(bits(audio[bb, :nn * hop]), bits(ref_audio[bb, :nn * hop])), bb


# ------------------------------------------------------------------------------------------------------------------------
# streams
# ------------------------------------------------------------------------------------------------------------------------
SCHEDULE = (6, 6, 7, 6, 7)


def _serve(syn, streams, packet, max_ticks=80):
    """Push every stream's frames in packets of `packet` and tick until all are finished.  streams: {sid: (mel (T, 80),
    noise, factor rows or None)}.  Returns the audio per stream and, per tick that emitted, whether it was a replayed graph."""
    got, pos, replayed = {sid: [] for sid in streams}, {sid: 0 for sid in streams}, []
    for sid in streams:
        syn.open(sid)
    for _ in range(max_ticks):
        for sid, (mel, noise, phi) in streams.items():
            lo = pos[sid]
            if lo < mel.shape[0]:
                hi = min(lo + packet, mel.shape[0])
                extra = {} if phi is None else {"formant": phi[lo:hi]}
                syn.push(sid, mel[lo:hi], noise[lo * 20:hi * 20], last=hi == mel.shape[0], **extra)
                pos[sid] = hi
        out = syn.tick()
        if out:
            replayed.append(syn.last_tick_replayed)
        for sid, audio in out.items():
            got[sid].append(np.array(audio))
        if all(syn.finished(sid) for sid in streams):
            break
    return {sid: np.concatenate(vv) for sid, vv in got.items()}, replayed


def test_streams_equal_the_offline_forward(engine):
    """Two streams through the 80 ms schedule (6, 6, 7, 6, 7), long enough for every phase to be recorded and then replayed
    as a graph: the one with per-frame factors -- they change inside every tick -- equals the offline forward(formant=) of
    its utterance bit for bit, the one without equals its plain forward, the bits it has in a synthesizer of its own."""
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    frames = 4 * sum(SCHEDULE) + 12
    streams = {}
    for sid in range(2):
        mel, noise = synthetic_inputs(7400 + sid, 1, frames)
        streams[sid] = (mel[0], noise[0], _factor_rows(7410, 1, frames)[0] if sid == 0 else None)
    assert len(np.unique(streams[0][2][:6])) > 2
    offline = {sid: engine.forward(_dev(mel[None]), noise=_dev(noise[None]),
                                   **({} if phi is None else {"formant": _dev(phi[None])})).cpu().numpy()[0]
               for sid, (mel, noise, phi) in streams.items()}
    assert not np.array_equal(offline[0], engine.forward(_dev(streams[0][0][None]), noise=_dev(streams[0][1][None])).cpu().numpy()[0])
    syn = StreamingSynthesizer(engine, chunk_frames=SCHEDULE)
    got, replayed = _serve(syn, streams, 8)
    assert syn.graph_ticks > 0 and replayed.count(True) == syn.graph_ticks and False in replayed
    for sid in streams:
        assert got[sid].shape == offline[sid].shape
        assert np.array_equal(bits(got[sid]), bits(offline[sid])), f"stream {sid} differs from the offline synthesis"
    alone = StreamingSynthesizer(engine, chunk_frames=SCHEDULE)
    solo, _ = _serve(alone, {1: streams[1]}, 8)
    assert not alone._formant and np.array_equal(bits(solo[1]), bits(got[1]))


# ------------------------------------------------------------------------------------------------------------------------
# live streams and the tool, on a small model
# ------------------------------------------------------------------------------------------------------------------------
SEED = 11
SOUNDS = [("alto.wav", 7200, 24000), ("basso.wav", 13230, 44100)]          # 0.3 s each


def _sound(seed, n, rate):
    rng = np.random.default_rng(seed)
    tt = np.arange(n) / float(rate)
    return (0.3 * np.sin(2 * np.pi * 170.0 * tt) + 0.05 * rng.normal(size=n)).astype(np.float32)


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    return create_synthetic_model_dir(str(tmp_path_factory.mktemp("model") / "speech_small"), "SPEECH", **SMALL)


def test_live_stream_equals_transform_audio(model_dir):
    """LiveResynthesizer.push_audio(formant=1.3) in 80 ms pushes equals MELInverter.transform_audio(formant=[1.3]) of the
    same sound under the same keyed noise, for a sound at the model rate and a resampled one; and the factor does something."""
    import importlib.util
    from mbexwn_vocoder_amd.live import LiveResynthesizer, keyed_noise_fn
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    spec = importlib.util.spec_from_file_location("stream_transpose", os.path.join(ROOT, "mbexwn_vocoder_amd", "bin", "stream_transpose.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    inv = MELInverter(model_dir, conv_form="f23")
    sounds = [_sound(40 + ii, nn, rate) for ii, (_, nn, rate) in enumerate(SOUNDS)]
    names, rates = [ss[0] for ss in SOUNDS], [ss[2] for ss in SOUNDS]
    want = inv.transform_audio(sounds, rates, names, noise_seed=SEED, formant=[1.3, 1.3])
    plain = inv.transform_audio(sounds, rates, names, noise_seed=SEED)
    ones = inv.transform_audio(sounds, rates, names, noise_seed=SEED, formant=[1.0, np.ones(want[1].size // inv.hop_size)])
    live = LiveResynthesizer(inv)
    fn = keyed_noise_fn(inv.model, SEED)
    for snd, name, rate, ref, base, one in zip(sounds, names, rates, want, plain, ones):
        got = tool.stream_file(live, snd, int(round(0.08 * rate)), 1.0, stream_id=name, noise_fn=fn,
                               sample_rate=None if rate == 24000 else rate, formant=1.3)
        assert got.shape == ref.shape and np.array_equal(bits(got), bits(ref)), name
        assert not np.array_equal(ref, base) and np.array_equal(bits(one), bits(base)), name
    # it composes with the transposition: the two-step route with both rows
    from mbexwn_vocoder_amd.analysis import generate_mels
    from mbexwn_vocoder_amd.noise import item_key
    both = inv.transform_audio(sounds[:1], rates[:1], names[:1], noise_seed=SEED, transposition=1.25, formant=[0.8])[0]
    scaled = inv.scale_mel(generate_mels(sounds[:1], rates[:1], inv.preprocess_config, on_device=True)[0])
    rows = np.full(scaled.shape[1], 1.25, dtype=np.float32)
    two_step = inv.synth_from_mel(scaled, noise_seed=SEED, noise_key=item_key(names[0]), transposition=rows, formant=0.8)
    assert np.array_equal(bits(both), bits(two_step))


@pytest.mark.timeout(600)
def test_tool_writes_the_same_files_in_any_batch_and_order(model_dir, tmp_path):
    """transform_audio.py --formant-shift 1.2 --batch-invariant on two short wav files: each output is independent of the batch
    size and the argument order, differs from the --formant-shift 1 output, and that one is the output without the flag."""
    from scipy.io import wavfile
    files = []
    for ii, (name, nn, rate) in enumerate(SOUNDS):
        files.append(str(tmp_path / name))
        wavfile.write(files[-1], rate, _sound(40 + ii, nn, rate))
    common = ["--model_id", model_dir, "--batch-invariant", "--noise-seed", str(SEED), "-q"]
    runs = {}
    for tag, order, extra in (("shift_b2", files, ["--formant-shift", "1.2", "--batch", "2"]),
                              ("shift_b1", files[::-1], ["--formant-shift", "1.2", "--batch", "1"]),
                              ("one", files, ["--formant-shift", "1", "--batch", "2"]), ("none", files, ["--batch", "2"])):
        # (the four jobs side by side: most of a job's time is its start)
        runs[tag] = subprocess.Popen([sys.executable, os.path.join(ROOT, "mbexwn_vocoder_amd", "bin", "transform_audio.py"), *order,
                                      "-o", str(tmp_path / tag), *common, *extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                     text=True)
    outs = {}
    for tag, proc in runs.items():
        _, err = proc.communicate(timeout=600)
        assert proc.returncode == 0, err[-3000:]
        out = str(tmp_path / tag)
        outs[tag] = {nn: open(os.path.join(out, nn), "rb").read() for nn in sorted(os.listdir(out))}
    assert sorted(outs["shift_b2"]) == ["syn_alto.flac", "syn_basso.flac"]
    assert outs["shift_b1"] == outs["shift_b2"] and outs["one"] == outs["none"]
    for name in outs["none"]:
        assert outs["shift_b2"][name] != outs["none"][name], name

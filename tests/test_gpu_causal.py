"""force_causal models and the causal Winograd gate kernels on the device.

* the three force_causal golden cases of tests/golden/make_reference_causal.py (the reference's own graph, run with
  tf.float32 := float64) at the end-to-end bar 1e-4 * max(1, max|ref|) of test_gpu_configs.py, for the audio, the F0
  contour and the excitation, on the default form and pinned to F(2,3) and F(4,3);
* the "causal" geometry of test_gpu_wavenet_stages.py (SPEECH, WaveNet padding CAUSAL) pinned to F(2,3) / F(4,3), stage
  by stage against the float64 oracle at that file's tolerance; per layer the gate kernel is the one the SAME model runs
  under the same pin, except the layers with d > 16 (no causal strided kernel): those run the direct form;
* the padding contract (padding frames at 0, 1e30, NaN give bit-identical valid rows) for the pinned causal forms;
* streams of the causal SMALL model (force_causal, and CAUSAL WaveNet padding only) bit-equal to the offline F(2,3) run,
  with and without the per-layer state, graph replays and the front-end ring; a direct-form causal engine's streams;
* a pinned causal forward and a causal stream between guard bands (tests/guarded.py);
* streams of a multi-block causal model stay refused.
"""
import os

import numpy as np
import pytest

import test_gpu_memory_contract as tmc
import test_gpu_wavenet_stages as twn
from helpers import build_case, load_golden
from test_causal_host import CAUSAL_CASES
from wn_reference import assert_matches, engine_stages, summary

pytestmark = pytest.mark.gpu

E2E_TOL = 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WINOGRAD = {"folded_start", "f23", "f43", "f43_psplit", "f43_hsplit"}
_WN = "mbexwn_config:pp_mod_subnet:"
DEEP12_CAUSAL = ("SPEECH", {_WN + "n_layers": 12, _WN + "padding": "CAUSAL"})
DEEP12_SAME = ("SPEECH", {_WN + "n_layers": 12})


def _tol(ref, rel=E2E_TOL):
    return rel * max(1.0, float(np.max(np.abs(ref))))


def _maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    assert _torch.cuda.is_available(), "GPU tests need an MI355X"
    return _torch


def _engine(model, **kwargs):
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    cfg, raw, wt = build_case(*model)
    return MBExWNEngine(cfg, raw, wt, **kwargs), cfg, raw, wt


def _gate_kernels(eng):
    return list(eng.conv_form_info()["gate_kernels"])


# ------------------------------------------------------------------------------------------------------------------------
# 1. the reference's force_causal graph
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["auto", "f23", "f43"])
@pytest.mark.parametrize("case", sorted(CAUSAL_CASES))
def test_force_causal_goldens(torch, case, form):
    """Audio, F0 contour and excitation of a force_causal model against the reference's float64 run (and its float32 run),
    at the end-to-end bar.  The default form keeps the direct gate kernel on every layer; a pinned form runs its Winograd
    kernels with the start convolution folded into layer 0."""
    g64 = load_golden(os.path.join(GOLDEN, "reference_causal_f64.npz"))
    g32 = load_golden(os.path.join(GOLDEN, "reference_causal_f32.npz"))
    voice, over, _, _ = CAUSAL_CASES[case]
    eng, cfg, raw, wt = _engine((voice, over), conv_form=form)
    mel, noise = g32[f"{case}/mell"], g32[f"{case}/noise"]
    got = eng.forward(torch.as_tensor(mel).cuda(), noise=torch.as_tensor(noise).cuda()).cpu().numpy()
    out = {"audio": got, "f0": eng.stage("f0").cpu().numpy(), "excitation": eng.stage("excitation").cpu().numpy()}
    kernels = _gate_kernels(eng)
    eng.close()
    for name, arr in out.items():
        for tag, gold in (("f64", g64), ("f32", g32)):
            ref = gold[f"{case}/{name}"]
            err, bar = _maxdiff(arr, ref), _tol(ref)
            print(f"\ncausal golden {case} [{form}] {name} vs reference {tag}: {err:.3e} (bar {bar:.3e})")
            assert err <= bar, f"{case} [{form}]: {name} is {err:.3e} from the reference's {tag} run (bar {bar:.3e})"
    if form == "auto":
        assert set(kernels) == {"direct"}, kernels
    else:
        assert kernels[0] == "folded_start" and set(kernels) <= WINOGRAD and "direct" not in kernels, kernels


def test_causal_subnets_large_launch_same_bits(torch):
    """The force_causal sub-nets (front pads only, SYMMETRIC) through the large-launch kernels of the mel-rate group launch
    (16 x 800 frames: the LDS-staged mel tile, the 32 x 32 float64 tile of the F0-net) give the bits of the small-launch
    kernels that run the same items one at a time: F0 contour and cepstrum of the first, a middle and the last item."""
    from helpers import synthetic_inputs
    eng = _engine(("SPEECH", {"mbexwn_config:force_causal": True}), conv_form="direct")[0]
    B, T = 16, 800
    mel, noise = synthetic_inputs(31, B, T)
    eng.forward(torch.as_tensor(mel).cuda(), noise=torch.as_tensor(noise).cuda())
    big = {name: eng.stage(name).cpu().numpy() for name in ("f0", "cepstrum")}
    for ii in (0, 7, B - 1):
        eng.forward(torch.as_tensor(mel[ii:ii + 1]).cuda(), noise=torch.as_tensor(noise[ii:ii + 1]).cuda())
        for name, arr in big.items():
            one = eng.stage(name).cpu().numpy()[0]
            bad = np.argwhere(one != arr[ii])
            assert bad.size == 0, f"{name} of item {ii}: the large launch differs from the single item, first at {bad[0]}"
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 2. stage by stage against the float64 oracle
# ------------------------------------------------------------------------------------------------------------------------
STAGE_CASES = [
    # (id, causal model, SAME twin, lengths, pin)
    ("causal-f23", twn.GEOMETRIES["causal"], twn.GEOMETRIES["speech"], "ragged", "f23"),
    ("causal-f43", twn.GEOMETRIES["causal"], twn.GEOMETRIES["speech"], "ragged", "f43"),
    ("causal-large-f23", twn.GEOMETRIES["causal"], twn.GEOMETRIES["speech"], "large", "f23"),
    ("causal-large-f43", twn.GEOMETRIES["causal"], twn.GEOMETRIES["speech"], "large", "f43"),
    ("deep12-causal-f43", DEEP12_CAUSAL, DEEP12_SAME, "deep", "f43"),
]


def _twin_kernels(torch, model, lkey, pin):
    """The gate kernels the SAME-padding model runs under the same pin on the same batch."""
    lengths, _ = twn.LENGTHS[lkey]
    mel, noise = twn._inputs(lengths)
    eng = _engine(model, conv_form=pin)[0]
    eng.forward(torch.as_tensor(mel).cuda(), n_frames=torch.as_tensor(lengths, dtype=torch.int32).cuda(),
                noise=torch.as_tensor(noise).cuda())
    out = _gate_kernels(eng)
    eng.close()
    return out


def _expected_kernels(dims, same_kernels):
    return [kk if dims.wn_dilation(ll) <= 16 else "direct" for ll, kk in enumerate(same_kernels)]


@pytest.mark.parametrize("cid,model,twin,lkey,pin", STAGE_CASES, ids=[case[0] for case in STAGE_CASES])
def test_causal_wavenet_stages_match_the_oracle(torch, cid, model, twin, lkey, pin):
    """"wn_out" and "wn_hidden" of every checked item against the float64 oracle's causal WaveNet at the tolerance of
    test_gpu_wavenet_stages.py; per layer the SAME model's gate kernel for the same pin (d > 16: direct)."""
    lengths, items = twn.LENGTHS[lkey]
    B, T = len(lengths), max(lengths)
    mel, noise = twn._inputs(lengths)
    eng, cfg, raw, wt = _engine(model, conv_form=pin)
    assert eng.dims.wn_padding == "CAUSAL"
    rpf = eng.dims.wn_in_rows_per_frame
    nf = torch.as_tensor(lengths, dtype=torch.int32).cuda()
    audio = eng.forward(torch.as_tensor(mel).cuda(), n_frames=nf, noise=torch.as_tensor(noise).cuda()).cpu().numpy()
    ran = _gate_kernels(eng)
    names = ["wn_out", "wn_hidden"]
    got = engine_stages(eng, names, B, T, items=items)
    pulse = eng.stage("pulse").cpu().numpy().reshape(B, T * rpf, -1)
    dims = eng.dims
    eng.close()
    want = _expected_kernels(dims, _twin_kernels(torch, twin, lkey, pin))
    print(f"\ncausal stages {cid}: gate kernels {ran} (SAME twin, d > 16 direct: {want})")
    assert ran == want, f"{cid}: gate kernels {ran}, expected {want}"
    for ii, ll in enumerate(lengths):
        assert np.all(np.isfinite(audio[ii, :ll * 300])) and np.all(audio[ii, ll * 300:] == 0.0), f"{cid}: audio of item {ii}"
    ref = twn._reference(cid, lkey, cfg, raw, wt, mel, noise, pulse)
    rep = ref.compare(got, names=names)
    print(f"causal stages {cid}: {summary(rep)}")
    assert_matches(rep)


# ------------------------------------------------------------------------------------------------------------------------
# 3. the padding contract
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pin", ["f23", "f43"])
def test_causal_padding_frames_are_never_read(torch, pin):
    """The ragged batch of test_padding_frames_are_never_read with its padding frames of mel and noise at 0, 1e30 and NaN,
    through the causal model pinned to a Winograd form: audio and WaveNet stages of the valid rows bit-identical."""
    eng, cfg, _, _ = _engine(twn.GEOMETRIES["causal"], conv_form=pin)
    lengths = twn.RAGGED
    B, T = len(lengths), max(lengths)
    mel, noise = twn._inputs(lengths, seed=911)
    nf = torch.as_tensor(lengths, dtype=torch.int32).cuda()
    runs = {}
    for fill in (0.0, 1e30, np.nan):
        m, n = mel.copy(), noise.copy()
        for ii, ll in enumerate(lengths):
            m[ii, ll:] = fill
            n[ii, ll * 20:] = fill
        audio = eng.forward(torch.as_tensor(m).cuda(), n_frames=nf, noise=torch.as_tensor(n).cuda()).cpu().numpy()
        st = engine_stages(eng, ["wn_out", "wn_hidden"], B, T)
        runs[fill] = (audio, st, _gate_kernels(eng))
    dims = eng.dims
    eng.close()
    want = _expected_kernels(dims, _twin_kernels(torch, twn.GEOMETRIES["speech"], "ragged", pin))
    base_audio, base_st, base_k = runs[0.0]
    for fill in (0.0, 1e30, np.nan):
        assert runs[fill][2] == want, f"{pin}: gate kernels {runs[fill][2]}, expected {want}"
    for fill in (1e30, np.nan):
        audio, st, _ = runs[fill]
        for ii, ll in enumerate(lengths):
            assert np.array_equal(audio[ii, :ll * 300], base_audio[ii, :ll * 300]), f"{pin}: audio of item {ii}, padding {fill}"
            assert np.all(audio[ii, ll * 300:] == 0.0), f"{pin}: audio behind item {ii}'s end, padding {fill}"
            for name in st:
                a, b = st[name][ii, :ll * 20], base_st[name][ii, :ll * 20]
                bad = np.argwhere(a != b)
                assert bad.size == 0, f"{pin}: {name} of item {ii} differs with padding {fill}: first at {bad[0]}"
    for ii, ll in enumerate(lengths):
        assert np.all(np.isfinite(base_audio[ii, :ll * 300]))


# ------------------------------------------------------------------------------------------------------------------------
# 4. streams
# ------------------------------------------------------------------------------------------------------------------------
SMALL = {_WN + "n_channels": 32, _WN + "n_layers": 5}          # the streaming model of test_gpu_streaming.py
STREAM_MODELS = {"force_causal": ("SPEECH", dict(SMALL, **{"mbexwn_config:force_causal": True})),
                 "wavenet_causal": ("SPEECH", dict(SMALL, **{_WN + "padding": "CAUSAL"}))}
STREAM_LENGTHS = [140, 140, 23, 8]      # two long streams in step (steady ticks, graph replays), a short one, one chunk


def _stream(syn, lengths, seed, before_ticks=None):
    """Open, push whole (last=True) and tick to the end: ({stream: audio}, kinds of tick (True: per-layer state carried))."""
    for sid in range(len(lengths)):
        syn.open(sid)
    if before_ticks is not None:
        before_ticks(syn)
    from helpers import synthetic_inputs
    inputs = {sid: synthetic_inputs(seed + sid, 1, ll) for sid, ll in enumerate(lengths)}
    for sid, (mel, noise) in inputs.items():
        syn.push(sid, mel[0], noise[0], last=True)
    got, kinds = {sid: [] for sid in inputs}, set()
    for _ in range(400):
        out = syn.tick()
        if out:
            kinds.add(syn.last_tick_layer_rows > 0)
        for sid, audio in out.items():
            got[sid].append(np.array(audio, copy=True))
        if all(syn.finished(sid) for sid in inputs):
            break
    return {sid: np.concatenate(vv) for sid, vv in got.items()}, kinds, inputs


def _offline(torch, eng, inputs):
    return {sid: eng.forward(torch.as_tensor(mel).cuda(), noise=torch.as_tensor(noise).cuda()).cpu().numpy()[0]
            for sid, (mel, noise) in inputs.items()}


@pytest.mark.parametrize("chunk", [8, 5, 2, (6, 6, 7, 6, 7)], ids=["8", "5", "2", "80ms_schedule"])
@pytest.mark.parametrize("model", sorted(STREAM_MODELS))
def test_causal_streams_equal_the_offline_f23_run(torch, model, chunk):
    """Streams of the causal SMALL model on an engine pinned to F(2,3) (the form streams run): bit-equal to the offline
    synthesis of the same engine, ticks with and without the per-layer WaveNet state, and on the schedules whose period
    is a whole number of alignment steps, graph replays with the front end carried in its ring."""
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    eng = _engine(STREAM_MODELS[model], conv_form="f23")[0]
    assert eng.dims.wn_padding == "CAUSAL" and eng.conv_form_info()["stream_form"] == "f23"
    syn = StreamingSynthesizer(eng, chunk_frames=chunk)
    assert syn.layer_carry
    got, kinds, inputs = _stream(syn, STREAM_LENGTHS, 700)
    offline = _offline(torch, eng, inputs)
    print(f"\ncausal streams {model} chunk {chunk}: look-ahead {syn.lookahead_ms} ms, margins ({syn.left}, {syn.right}, "
          f"{syn.lead}), {syn.graph_ticks} graph ticks, front-end ring {syn.fe_carry}")
    eng.close()
    assert kinds == {False, True}, kinds
    if chunk in (8, (6, 6, 7, 6, 7)):
        assert syn.fe_carry and syn.graph_ticks > 0, (syn.fe_carry, syn.graph_ticks)
    for sid, ref in offline.items():
        assert got[sid].shape == ref.shape, f"stream {sid}"
        where = np.argwhere(got[sid] != ref)
        assert where.size == 0, f"{model} chunk {chunk}: stream {sid} differs from the offline run, first at sample {where[0][0]}"


def test_direct_form_causal_streams_equal_their_own_offline_run(torch):
    """A causal engine on the default form runs direct: its streams carry no per-layer state and are bit-equal to its own
    offline synthesis."""
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    eng = _engine(STREAM_MODELS["force_causal"])[0]
    assert eng.conv_form_info()["form"] == "direct" and eng.layer_state_info()[0] == 0
    syn = StreamingSynthesizer(eng, chunk_frames=8)
    assert not syn.layer_carry
    got, kinds, inputs = _stream(syn, [61, 23], 77)
    offline = _offline(torch, eng, inputs)
    assert _gate_kernels(eng) == ["direct"] * eng.dims.wn_layers
    eng.close()
    assert kinds == {False}
    for sid, ref in offline.items():
        assert np.array_equal(got[sid], ref), f"stream {sid}"


def test_causal_stream_stays_inside_its_stores(torch):
    """The 80 ms schedule on the force_causal SMALL model pinned to F(2,3), its three stores (carried sub-bands, per-layer
    state with the causal slot layout, front-end ring) between NaN guard bands: every guard untouched, the audio bit-equal
    to the offline run."""
    from guarded import GuardSet
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    eng = _engine(STREAM_MODELS["force_causal"], conv_form="f23")[0]
    floats, reach, min_rows = eng.layer_state_info()
    assert (reach, min_rows) == (20, 32) and floats == sum(2 * d * 32 for d in (2, 4, 8, 16))
    syn = StreamingSynthesizer(eng, chunk_frames=(6, 6, 7, 6, 7))
    gs = GuardSet("nan", eng.device)

    def guard_stores(syn):
        for attr in ("_store", "_layer_store", "_fe_store"):
            old = getattr(syn, attr)
            assert old is not None, attr
            buf = gs.new(attr, old.numel() * 4, data=old)
            setattr(syn, attr, buf.view(torch.float32, *old.shape))
    got, kinds, inputs = _stream(syn, STREAM_LENGTHS, 900, before_ticks=guard_stores)
    torch.cuda.synchronize()
    gs.check()
    offline = _offline(torch, eng, inputs)
    eng.close()
    assert kinds == {False, True} and syn.graph_ticks > 0
    for sid, ref in offline.items():
        assert np.array_equal(got[sid], ref), f"stream {sid}"


# ------------------------------------------------------------------------------------------------------------------------
# 5. guard bands
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pin", ["f23", "f43"])
def test_pinned_causal_forward_stays_inside_its_buffers(torch, pin):
    """The pinned causal forward of the ragged batch on guarded buffers (test_gpu_memory_contract.py's _run_forward) under
    the three fills: every guard untouched, the poisoned runs bit-identical to the zero run, the gate kernels those of the
    SAME model."""
    case = (f"causal-guarded-{pin}", twn.GEOMETRIES["causal"], twn.RAGGED, None, {"conv_form": pin}, {}, "wn")
    runs = {fill: tmc._run_forward(torch, case, fill) for fill in tmc.FILLS}
    eng = tmc._engine(case[0], case[1], case[4])[0]
    ran = _gate_kernels(eng)
    want = _expected_kernels(eng.dims, _twin_kernels(torch, twn.GEOMETRIES["speech"], "ragged", pin))
    assert ran == want, f"{pin}: gate kernels {ran}, expected {want}"
    base_audio, base_stages = runs["zero"]
    for fill in ("nan", "huge"):
        audio, stages = runs[fill]
        for ii, ll in enumerate(case[2]):
            assert tmc._first_difference(audio[ii, :ll * 300], base_audio[ii, :ll * 300]) is None, f"{pin} [{fill}]: item {ii}"
            assert np.all(audio[ii, ll * 300:] == 0.0)
        for name in stages:
            for ii, (a, b) in enumerate(zip(stages[name], base_stages[name])):
                assert tmc._first_difference(a, b) is None, f"{pin} [{fill}]: {name} of item {ii}"


# ------------------------------------------------------------------------------------------------------------------------
# 6. what stays refused
# ------------------------------------------------------------------------------------------------------------------------
def test_multi_block_causal_streams_stay_refused(torch):
    """A causal model with several WaveNet blocks runs whole items only: its streams raise."""
    from helpers import synthetic_inputs
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    # two blocks at the sub-band rate (the noise of a stream then has the rows of the first block)
    model = ("SPEECH", {_WN + "n_channels": 32, _WN + "n_layers": 3, _WN + "padding": "CAUSAL",
                        "mbexwn_config:pp_mod_subnet_upsampling_factors": [1, 1],
                        "mbexwn_config:pp_mod_subnet_channel_factors": [1, 1]})
    eng = _engine(model, conv_form="f23")[0]
    assert eng.dims.wn_multi and eng.dims.wn_padding == "CAUSAL"
    mel, noise = synthetic_inputs(5, 1, 24, steps_per_frame=eng.dims.steps_per_frame)
    syn = StreamingSynthesizer(eng, chunk_frames=8)
    syn.open(0)
    with pytest.raises(NotImplementedError):
        syn.push(0, mel[0], noise[0], last=True)
        for _ in range(4):
            syn.tick()

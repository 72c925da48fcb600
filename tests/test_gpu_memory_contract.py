"""The memory contract of the C ABI (include/mbexwn.h: "the caller owns all buffers"): no entry point writes outside the bytes
it was given, reads its inputs outside their stated extent, or depends on what its scratch memory held before.

Every buffer of every call sits between two 4 MiB guard bands (tests/guarded.py) and has exactly the byte size the header
states -- the workspace ``mbx_workspace_size(handle, B, T)``, passed on as ``workspace_bytes`` unchanged.  The whole
allocation (guards, scratch and outputs) is filled before the call, once with zeros, once with 0xFF (NaN in every float
format: survives a multiply by zero) and once with float32 1e30 (finite: survives the clamps that swallow a NaN); then

* every guard of every buffer, inputs included, is untouched under all three fills;
* the audio and every stage are bit-identical across the three fills over each item's own valid range, and the audio behind
  an item's own length is zero;
* the ``zero`` run's audio is within the end-to-end bar of tests/test_gpu_parity.py (E2E_TOL) of the float64 oracle, so that
  three equal wrong answers cannot pass.  That is the only tolerance in this file: everything else is equality.

The forward cases are those of test_gpu_wavenet_stages.py, test_gpu_wavenet_blocks.py and test_gpu_backend_stages.py,
selected by id with their ragged length lists, plus batch shapes those tables do not have, plus the per-frame controls
together (CONTROLS: the control rows are guarded inputs whose entries behind an item's length hold the fill, and env_mel of
mbxe_forward -- scratch of the caller -- is a guarded, filled buffer of exactly its stated size).  The one int32 region of the
workspace ("ceps_index") is filled with a valid lifter row instead of the poison (a stale read still changes bits, and
cannot address outside the lifter table); integer inputs are never poisoned.  The stand-alone entry points are called through
the library with raw pointers and held bit for bit to the engine's own wrappers, which the parity tests hold to the oracle.

No test here makes a kernel overrun, shrinks a buffer that a launch sees, or hands a bad pointer to a launch: the refusals
are host-side checks in front of every launch, and the detector's own test only tells the checker that a payload is shorter
than it is."""
import ctypes
import itertools

import numpy as np
import pytest

import backend_reference as bref
import control_reference as cref
import test_gpu_backend_stages as tbe
import test_gpu_parity as parity
import test_gpu_wavenet_blocks as tblk
import test_gpu_wavenet_stages as twn
import wn_blocks_reference as wnb
import wn_reference as wnr
from guarded import FILLS, Guarded, GuardSet, fill_word
from helpers import build_case, synthetic_inputs
from mbexwn_vocoder_amd import flac
from mbexwn_vocoder_amd.envelope import channel_centres, warp_envelope_host
from oracle import mbexwn_oracle as orc

E2E_TOL = parity.E2E_TOL

# ------------------------------------------------------------------------------------------------------------------------
# forward cases: (id, model (voice, overrides), lengths, items held to the oracle or None = all, engine arguments, forward
# arguments, stage cutter)
# ------------------------------------------------------------------------------------------------------------------------
WN_IDS = ["c12-f43", "c36-f43", "speech-direct", "speech-f23", "speech-f43", "speech-f43-invariant", "speech-f43-hsplit",
          "speech-rs-nowave", "speech-rs-split2", "lin5-f43", "groups2-f43", "causal-auto", "speech-keep-skip", "speech-split",
          "speech-split-f32h",
          "voice-f43", "deep12-f43", "deep12-f43-invariant", "deep12-split", "large-f43", "large-split",
          # C + n_out one column pair past a multiple of 32: a last pair of two valid columns under the wide and the wave kernel
          "c292-invariant", "c324-rs-split2",
          # the F(4,3) blocks of two column tiles: a partial tile inside a pair, a pair beside an odd one-tile launch, one pair
          "c292-two-tile", "c68-two-tile", "c36-two-tile"]
# every multi-block geometry once (the mb_* regions are the last ones carved, next to the end of the workspace), the handle
# without weight images (res/skip through conv1d), and the pulse-PQMF and sub-harmonic inputs
BLOCK_IDS = ["blocks-f43", "blocks-noimages", "up2-f43", "three-precond-gfu", "nocond", "c64-f43", "deep6-f43", "lin2-f43",
             "causal-blocks", "subharm-folded", "pqmf-direct", "large-c64-f43"]
BACKEND_IDS = ["psoff", "subgain", "nopqmf", "mixed_b", "normmel", "bands12_fold4", "bands30_out60", "sr16k_hop200", "hop400",
               "ceps400_energy", "voice", "speech-f0-sweep", "speech-transpose-0.4", "speech-large"]
LARGE_IDS = {"large-f43", "large-split", "large-c64-f43", "speech-large"}
F43 = {"conv_form": "f43"}
# shapes the tables do not have, on the SPEECH geometry of test_gpu_wavenet_stages.py: one item of one frame; the last item
# the longest and the last item one frame (the last item's rows end at the buffer's end); the float32 F0-net
EXTRA = [
    ("one-frame", "speech", [1], F43),
    ("last-longest", "speech", [7, 1, 26, 52], F43),
    ("last-one-frame", "speech", [52, 13, 1], F43),
    ("f0net-f32", "speech", twn.RAGGED, dict(F43, f0_accumulate="f32")),
]
# The per-frame controls together (mbx_forward_options.f0_frames / f0_scale / f0_item_mask, env_factor of mbxe_forward), on the
# small SPEECH model of the control tests (tests/test_gpu_controls.py), its RMS-normalising variant and the causal two-block
# geometry: every control row is a guarded input of exactly its byte size whose entries at or behind an item's n_frames hold
# the fill, and env_mel -- "scratch of the caller" -- is a guarded, filled buffer of exactly batch x max_frames x mel floats.
_SMALL5 = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 5}
_NORM5 = dict(_SMALL5, **{"mbexwn_config:normalize_rms_from_mell": True, "mbexwn_config:normalize_rms_num_smooth_iters": 1})
CONTROL_KEYS = ("f0_frames", "f0_scale", "f0_item_mask", "formant")
ALL_CONTROLS = {"f0_frames": "rows", "f0_scale": "rows", "f0_item_mask": "alternate", "formant": "rows"}
CONTROLS = [
    ("backend-speech-controls", ("SPEECH", _SMALL5), tbe.RAGGED, {}, ALL_CONTROLS, "backend"),
    ("backend-normmel-formant", ("SPEECH", _NORM5), tbe.RAGGED, {}, {"formant": "rows"}, "backend"),
    ("causal-blocks-controls", tblk.GEOMETRIES["causal"], tblk.RAGGED, {}, ALL_CONTROLS, "blocks"),
]


def _forward_cases():
    out = []
    wn_cases = {case[0]: case for case in twn.CASES}
    for cid in WN_IDS:
        _, geom, lkey, kwargs, _ = wn_cases[cid]
        lengths, items = twn.LENGTHS[lkey]
        out.append((cid, twn.GEOMETRIES[geom], lengths, items, kwargs, {}, "wn"))
    for cid, geom, lengths, kwargs in EXTRA:
        out.append((cid, twn.GEOMETRIES[geom], lengths, None, kwargs, {}, "wn"))
    blk_cases = {case[0]: case for case in tblk.CASES}
    for cid in BLOCK_IDS:
        _, geom, lkey, kwargs = blk_cases[cid]
        lengths, items = tblk.LENGTHS[lkey]
        out.append((cid, tblk.GEOMETRIES[geom], lengths, items, kwargs, {}, "blocks"))
    be_cases = {case[0]: case for case in tbe.CASES}
    for cid in BACKEND_IDS:
        _, geom, lengths, fw = be_cases[cid]
        out.append(("backend-" + cid, tbe.GEOMETRIES[geom], lengths, tbe.LARGE_CHECK if lengths is tbe.LARGE else None, {}, fw,
                    "backend"))
    out.append(("backend-pulsepqmf", tblk.GEOMETRIES["pqmf"], tbe.RAGGED, None, {}, {}, "backend"))
    for cid, model, lengths, kwargs, fw, cutter in CONTROLS:
        out.append((cid, model, lengths, None, kwargs, fw, cutter))
    small = [case for case in out if case[0].replace("backend-", "") not in LARGE_IDS]
    return small + [case for case in out if case[0].replace("backend-", "") in LARGE_IDS]      # the large launches last


FORWARD_CASES = _forward_cases()
FORWARD = {case[0]: case for case in FORWARD_CASES}

# ------------------------------------------------------------------------------------------------------------------------
# stand-alone entry points: {symbol: [(case id, arguments)]}
# ------------------------------------------------------------------------------------------------------------------------
_PAD = {"CONSTANT": 0, "SYMMETRIC": 1, "EDGE": 2}


def _table(fn):
    return [mm for mm in fn.pytestmark if mm.name == "parametrize"][0].args[1]


def _conv_cases():
    """(id, cin, cout, ks, dil, mode, rows, prelu, batch) from the tables of the parity tests: the rows with ``cout`` of
    1, 7, 15, 36, 132, 240 and ``rows`` of 1, 3, 5, 129, 801, the dilated case with rows < dil, one large launch per family."""
    f32, f64 = [], []
    for cin, cout, ks, dil, mode, rows, prelu in _table(parity.test_conv1d):
        if cout in (1, 15, 240) or rows in (1, 3, 5, 129) or (dil, rows) in ((2048, 1200), (1024, 7000)):
            f32.append((f"{cin}x{cout}k{ks}d{dil}r{rows}", cin, cout, ks, dil, mode, rows, prelu, 2))
    for ks, cin, cout, mode, rows in _table(parity.test_mel_tile_large_launch_same_bits):
        if cout in (36, 132, 240) or rows == 801:
            f32.append((f"{cin}x{cout}k{ks}r{rows}b16", cin, cout, ks, 1, mode, rows, True, 16))
    for cin, cout, ks, mode, rows, prelu in _table(parity.test_conv1d_f64_accumulation):
        if cout in (1, 7, 20) or rows in (1, 5):
            f64.append((f"{cin}x{cout}k{ks}r{rows}", cin, cout, ks, 1, mode, rows, prelu, 2))
        if (cin, cout, rows) == (128, 128, 240):
            f64.append((f"{cin}x{cout}k{ks}r{rows}b52", cin, cout, ks, 1, mode, rows, prelu, 52))    # 12 480 rows: 32 x 32 tiles
    return f32, f64


CONV_F32, CONV_F64 = _conv_cases()
FLAC_LENGTHS = [1, 4095, 4096, 4097, 128 * 4096 + 1]


def _flac_residues(order):
    ends = np.cumsum([flac.frames_bytes(nn) for nn in order])
    return {int(ee) % 16 for ee in ends}


# the order that puts item boundaries at the most residues mod 16 (the kernel writes the 16-byte words a frame shares with
# its neighbour byte by byte), the first such order in lexicographic order of the positions
FLAC_ORDER = list(max(itertools.permutations(FLAC_LENGTHS), key=lambda oo: len(_flac_residues(oo))))
WINDOW_SCHEDULE = [(6, 29, 6), (6, 29, 6), (7, 28, 7), (6, 29, 6), (7, 28, 7)]     # (shift, keep, new) at 35 frames: 80 ms
STANDALONE = {
    "mbx_conv1d": [(cc[0], cc[1:]) for cc in CONV_F32],
    "mbx_conv1d_f64acc": [(cc[0], cc[1:]) for cc in CONV_F64],
    "mbx_lin_interp": [(f"{rows}x{ch}up{up}", (rows, ch, up)) for rows, ch, up in _table(parity.test_lin_interp)],
    "mbx_wavetable": [(f"n{nn}", (nn,)) for nn in (1, 999, 1000, 1001, 12345)],
    "mbx_pqmf_synthesis": [(f"steps{nn}", (nn,)) for nn in (1, 63, 64, 65, 333)],
    "mbx_stft_filter": [(f"frames{nn}", (nn,)) for nn in (1, 3, 4, 5, 11)],
    "mbx_mel_analysis": [("ragged-exact", ([3001, 900, 5000, 301],))],     # 301 < win / 2: reflected three times
    "mbx_norm_mel": [("ragged-one-frame", ([13, 1, 26, 7],))],
    "mbx_encode_flac16": [("boundaries", (FLAC_ORDER,))],
    "mbx_window_advance": [("step8", (35, 8)), ("step-is-window", (35, 35))],
    "mbx_window_update": [("shift0", (35, [(0, 20, 9)])), ("keep0", (35, [(11, 0, 9)])), ("new-is-window", (35, [(0, 0, 35)])),
                          ("schedule-66767", (35, WINDOW_SCHEDULE))],
    "mbx_emit_rows": [("rows-end", (3, 777, 677, 100))],
}
# exported symbols that take an output pointer and have no stand-alone case, and why
EXEMPT = {
    "mbx_forward": "the forward cases of this file",
    "mbx_forward_ex": "the forward cases with an external F0 / transposition, the refusals and the streaming run",
    "mbx_forward_stream": "the refusals here; the streaming run drives it through streaming.py",
    "mbx_calibrate": "runs mbx_forward on its workspace argument and allocates its own audio; the refusals are held here",
    "mbx_create": "writes a host handle pointer only",
    "mbx_conv_form": "fills a host struct",
    "mbx_kernel_report": "fills a host struct",
    "mbx_plan": "fills a host struct, launches nothing",
    "mbx_layer_state_info": "writes three host integers",
    "mbx_stage": "hands out pointers into the workspace of the last forward, writes no device memory",
    "mbx_profile_read": "host scalars",
    "mbx_profile_read_launches": "host array of the caller's capacity, bench.py's own instrument",
    "mbx_clock_probe": "bench.py's own instrument: one wave writing four words",
}
# the symbols whose prototype (include/mbexwn.h) takes a device or host output pointer
_OUTPUT_ARGS = ("mbx_handle **", "*info", "float *audio", "float *y", "float *pulse", "float *out", "uint8_t *out", "float *mel_out",
                "float *mel_window", "float *host_out", "void *workspace", "*device_ptr", "*total_ms", "*launch_ms", "*device_out4",
                "*floats_per_slot")


def _prototypes():
    import c_headers
    return {name: plist for name, _, plist in c_headers.prototypes(c_headers.read_code("mbexwn.h"))}


def test_cases_cover_every_kernel_branch_and_export():
    """(CPU) The selected ids exist in the imported tables and still declare every gate kernel, every branch of the block
    runner and every branch of the back end; every exported symbol that takes an output pointer has a stand-alone case or a
    commented exemption, so a new export without a case fails the suite."""
    from mbexwn_vocoder_amd.config import ModelDims
    from mbexwn_vocoder_amd.engine import EXPORTED_SYMBOLS, GATE_KERNEL_NAMES
    wn_cases = {case[0]: case for case in twn.CASES}
    blk_cases = {case[0]: case for case in tblk.CASES}
    be_cases = {case[0]: case for case in tbe.CASES}
    assert set(WN_IDS) <= set(wn_cases) and set(BLOCK_IDS) <= set(blk_cases) and set(BACKEND_IDS) <= set(be_cases)
    assert len({case[0] for case in FORWARD_CASES}) == len(FORWARD_CASES)
    assert sum(cid.startswith("speech-rs-split") for cid in WN_IDS) >= 1
    declared = set().union(*(wn_cases[cid][4] for cid in WN_IDS))
    assert declared == set(GATE_KERNEL_NAMES.values()) - {"none"}, sorted(set(GATE_KERNEL_NAMES.values()) - declared)
    reached, multi = set(), set()
    for cid in BLOCK_IDS:
        dims = ModelDims(build_case(*tblk.GEOMETRIES[blk_cases[cid][1]])[0])
        reached |= tblk.block_runner_branches(dims, blk_cases[cid][3])
        if dims.wn_multi:
            multi.add(blk_cases[cid][1])
    assert reached == tblk.ALL_BRANCHES, sorted(tblk.ALL_BRANCHES - reached)
    every_multi = {geom for geom in tblk.GEOMETRIES if ModelDims(build_case(*tblk.GEOMETRIES[geom])[0]).wn_multi}
    assert multi == every_multi, sorted(every_multi - multi)
    geoms = {be_cases[cid][1] for cid in BACKEND_IDS}
    for geom, want in tbe.EXPECTED.items():
        cfg = build_case(*tbe.GEOMETRIES[geom])[0]
        kind = bref.backend_kind(ModelDims(cfg), cfg)
        assert any({kk: bref.backend_kind(ModelDims(build_case(*tbe.GEOMETRIES[gg])[0]), build_case(*tbe.GEOMETRIES[gg])[0])[kk]
                    for kk in want} == {kk: kind[kk] for kk in want} for gg in geoms), f"no case takes the branches of {geom}: {want}"
    # the batch shapes of EXTRA
    shapes = {cid: lengths for cid, _, lengths, _ in EXTRA}
    assert shapes["one-frame"] == [1] and shapes["last-longest"][-1] == max(shapes["last-longest"]) and shapes["last-one-frame"][-1] == 1
    # stand-alone coverage of the exports
    protos = _prototypes()
    assert set(EXPORTED_SYMBOLS) <= set(protos), sorted(set(EXPORTED_SYMBOLS) - set(protos))
    with_output = {sym for sym in EXPORTED_SYMBOLS if any(arg in protos[sym] for arg in _OUTPUT_ARGS)}
    assert {"mbx_conv1d", "mbx_emit_rows", "mbx_encode_flac16", "mbx_forward", "mbx_create", "mbx_stage"} <= with_output
    assert with_output - {"mbx_forward", "mbx_forward_ex", "mbx_forward_stream", "mbx_calibrate"} >= set(STANDALONE)
    missing = with_output - set(STANDALONE) - set(EXEMPT)
    assert not missing, f"exported symbols with an output pointer and neither a case nor an exemption: {sorted(missing)}"
    assert not set(STANDALONE) & set(EXEMPT)
    # every other export has no output pointer at all
    assert set(EXPORTED_SYMBOLS) - with_output <= {"mbx_last_error", "mbx_destroy", "mbx_workspace_size", "mbx_profile_enable"}
    # the edge shapes of the convolutions, the FLAC boundaries
    assert {cc[2] for cc in CONV_F32} >= {1, 15, 36, 132, 240} and {cc[2] for cc in CONV_F64} >= {1, 7}
    assert {cc[6] for cc in CONV_F32} >= {1, 3, 5, 129, 801} and any(cc[6] < cc[4] for cc in CONV_F32)
    assert any(cc[6] * cc[8] >= 12288 for cc in CONV_F32) and any(cc[6] * cc[8] >= 12288 for cc in CONV_F64)
    assert sorted(FLAC_ORDER) == sorted(FLAC_LENGTHS)
    assert all(len(_flac_residues(oo)) <= len(_flac_residues(FLAC_ORDER)) for oo in itertools.permutations(FLAC_LENGTHS))


# ------------------------------------------------------------------------------------------------------------------------
# GPU side
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    if not _torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return _torch


_ENGINES, _RUNS, _CEPS_REGION = {}, {}, {}


def _engine(key, model, kwargs):
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    if key not in _ENGINES:
        cfg, raw, wt = build_case(*model)
        with twn.tensor_table_of(key):
            _ENGINES[key] = (MBExWNEngine(cfg, raw, wt, **kwargs), cfg, raw, wt)
    return _ENGINES[key]


def _bits(arr):
    arr = np.ascontiguousarray(arr)
    return arr.view({4: np.uint32, 8: np.uint64}[arr.dtype.itemsize]) if arr.dtype.kind == "f" else arr


def _first_difference(a, b):
    bad = np.argwhere(_bits(a) != _bits(b))
    return None if bad.size == 0 else tuple(int(vv) for vv in bad[0])


def _ceps_region(torch, eng, B, T):
    """(byte offset into the workspace, int32 words) of the lifter rows, the one integer region of the workspace: located
    with mbx_stage after a warm-up forward of the same handle, batch and max_frames on a zero-filled guarded workspace."""
    key = (id(eng), B, T)
    if key not in _CEPS_REGION:
        d = eng.dims
        gs = GuardSet("zero", eng.device)
        ws = gs.new("workspace", eng.workspace_bytes(B, T))
        eng._workspace = ws.payload
        mel, noise = synthetic_inputs(1, B, T, steps_per_frame=d.wn_in_rows_per_frame)
        eng.forward(torch.as_tensor(mel).cuda(), noise=torch.as_tensor(noise).cuda() if d.noise_sigma else None)
        torch.cuda.synchronize()
        gs.check()
        ptr, cnt, stride = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        assert eng._lib.mbx_stage(eng._handle, b"ceps_index", ctypes.byref(ptr), ctypes.byref(cnt), ctypes.byref(stride)) == 0
        offset = ptr.value - ws.ptr
        assert offset % 256 == 0 and 0 <= offset and offset + 4 * B * stride.value <= ws.nbytes and cnt.value == T
        _CEPS_REGION[key] = (offset, B * stride.value)
        eng._workspace = None
    return _CEPS_REGION[key]


def _guarded_workspace(torch, gs, eng, B, T, nbytes=None):
    """The workspace between its guards, filled, with a valid lifter row in its integer region: 0 under ``zero``, the last row
    of the table under the poisons."""
    offset, words = _ceps_region(torch, eng, B, T)
    ws = gs.new("workspace", eng.workspace_bytes(B, T) if nbytes is None else nbytes)
    row = 0 if gs.fill == "zero" else bref.N_LIFTER_ROWS - 1
    ws.payload[offset:offset + 4 * words].view(torch.int32).fill_(row)
    return ws


def _case_inputs(case, dims):
    cid, _, lengths, _, _, fw, _ = case
    B, T = len(lengths), max(lengths)
    mel, noise = synthetic_inputs(907, B, T, steps_per_frame=dims.wn_in_rows_per_frame)
    fw = dict(fw)
    if fw.get("f0") == "sweep":
        fw["f0"] = tbe.sweep_contour(lengths, dims.pulse_per_frame)
    if any(kk in fw for kk in CONTROL_KEYS):
        rng = np.random.default_rng(908)
        rows = {"f0_frames": rng.uniform(80.0, 400.0, size=(B, T)).astype(np.float32),
                "f0_scale": rng.uniform(0.5, 2.0, size=(B, T)).astype(np.float32),
                "f0_item_mask": (np.arange(B) % 2 == 0).astype(np.int32),          # mixed: the F0-net runs for the odd items
                "formant": cref.formant_rows(rng, B, T)}
        rows["formant"][:, 0] = np.float32(1.3)                                      # (a one-frame item is warped too)
        fw.update({kk: rows[kk] for kk in CONTROL_KEYS if kk in fw})
    return mel, (noise if dims.noise_sigma else None), fw


def _stages(torch, eng, cfg, case):
    """{stage: [the item's own valid rows, per checked item]} of the last forward, cut with the helpers of the stage tests."""
    cid, _, lengths, items, kwargs, _, cutter = case
    d = eng.dims
    B, T = len(lengths), max(lengths)
    items = list(range(B)) if items is None else list(items)
    out = {}
    if cutter == "wn":
        names = ["wn_out"] + (["wn_skip"] if kwargs.get("keep_skip") else [])
        planes = True
        try:
            eng.stage("wn_hidden_planes")
        except ValueError:
            planes = False
        names.append("wn_hidden_planes" if planes else "wn_hidden")     # planes: the float32 hidden state is not written
        got = wnr.engine_stages(eng, [nn for nn in names if nn != "wn_hidden_planes"], B, T, items=items)
        rpf = d.wn_in_rows_per_frame
        for name, per_item in got.items():
            out[name] = [per_item[ii][:lengths[ii] * rpf] for ii in items]
        if planes:
            words = eng.stage("wn_hidden_planes").view(torch.int32).view(B, T * rpf, -1)
            out["wn_hidden_planes"] = [words[ii, :lengths[ii] * rpf].cpu().numpy() for ii in items]
        out["pulse"] = [eng.stage("pulse")[ii].cpu().numpy()[:lengths[ii] * d.pulse_per_frame * (1 + d.wt_subharm)] for ii in items]
    elif cutter == "blocks":
        layout = wnb.stage_layout(d)
        names = tblk._stage_names(eng, d)
        got = wnb.engine_stages(eng, layout, names, B, items)
        for name in names:
            out[name] = [got[name][ii][:lengths[ii] * layout[name][1]] for ii in items]
    else:
        per_frame = {"mel_in": 1, "cepstrum": 1, "ceps_index": 1, "subbands": d.steps_per_frame, "excitation": d.hop_size,
                     "frames": 1, "f0": d.pulse_per_frame, "wn_out": d.steps_per_frame}
        got = bref.engine_backend_stages(eng, B, T)
        for name, arr in got.items():
            out[name] = [arr[ii, :lengths[ii] * per_frame[name]] for ii in items]
    if "formant" in case[5]:
        env = eng.stage("mel_env").cpu().numpy().reshape(B, T, d.mel_channels)
        out["mel_env"] = [env[ii, :lengths[ii]] for ii in items]
    return out


def _run_forward(torch, case, fill):
    """One guarded forward of a case under a fill: (audio (B, T hop) numpy, stages)."""
    cid, model, lengths, items, kwargs, _, _ = case
    eng, cfg, raw, wt = _engine(cid, model, kwargs)
    d = eng.dims
    B, T = len(lengths), max(lengths)
    mel, noise, fw = _case_inputs(case, d)
    gs = GuardSet(fill, eng.device)
    ws = _guarded_workspace(torch, gs, eng, B, T)
    mel_g = gs.put("mel", mel)
    noise_g = gs.put("noise", noise) if noise is not None else None
    nf_g = gs.put("n_frames", np.asarray(lengths, dtype=np.int32))
    audio_g = gs.new("audio", B * T * d.hop_size * 4)
    dev = {}
    if "f0" in fw:
        dev["f0"] = gs.put("f0", fw["f0"]).view(torch.float32, B, T * d.pulse_per_frame)
    if "transposition" in fw:
        dev["transposition"] = fw["transposition"]
    for key in CONTROL_KEYS:
        if key not in fw:
            continue
        if key == "f0_item_mask":
            dev[key] = gs.put(key, fw[key]).view(torch.int32)
            continue
        dev[key] = gs.put(key, fw[key]).view(torch.float32, B, T)
        for ii, ll in enumerate(lengths):                 # entries at or behind an item's n_frames: the fill again
            dev[key][ii, ll:].view(torch.int32).fill_(fill_word(fill))
    env_before = eng._env_mel
    if "formant" in fw:
        eng._env_mel = gs.new("env_mel", B * T * d.mel_channels * 4).view(torch.float32)
    eng._workspace = ws.payload
    try:
        out = eng.forward(mel_g.view(torch.float32, B, T, d.mel_channels), n_frames=nf_g.view(torch.int32),
                          noise=noise_g.view(torch.float32, B, -1) if noise_g is not None else None,
                          out=audio_g.view(torch.float32, B, T * d.hop_size), **dev)
        torch.cuda.synchronize()
        assert out.data_ptr() == audio_g.ptr and eng._workspace.data_ptr() == ws.ptr
        gs.check()
        audio = out.cpu().numpy()
        stages = _stages(torch, eng, cfg, case)
    finally:
        eng._workspace = None
        eng._env_mel = env_before
    return audio, stages


def _oracle_audio(cfg, raw, wt, mel, noise, f0=None, transposition=1.0, controls=None):
    """The float64 oracle's audio of one item (1, T hop): OracleModel.forward, with the RMS normalisation of a normalising
    model in front and its gain behind, and with the contour given or transposed as mbx_forward_options does.  controls: the
    item's per-frame rows {f0_frames, f0_scale, formant: (1, T); f0_item_mask: 0 or 1}, any subset: the contour is built on the
    host as the header defines it -- LI(f0_frames) for an item that takes the frames, the oracle's own F0-net on the unwarped
    rows otherwise, times LI(f0_scale) -- and the chains read the rows warped by envelope.warp_envelope_host
    (tests/control_reference.py: controlled_oracle_audio)."""
    if controls:
        ppf = int(orc.OracleModel(cfg, raw, wt).pulse_per_frame)
        scale = controls.get("f0_scale")
        if "f0_frames" in controls and controls.get("f0_item_mask", 1):
            contour = orc.lin_interp(controls["f0_frames"].astype(np.float64)[:, :, None], ppf)[:, :, 0]
            if scale is not None:
                # (one float32 multiply of the two float32 interpolations, as the header states it)
                li = orc.lin_interp(scale.astype(np.float64)[:, :, None], ppf)[:, :, 0]
                contour = contour.astype(np.float32) * li.astype(np.float32)
        else:
            contour = cref.oracle_contour(cfg, raw, wt, mel, scale)
        env = None
        if "formant" in controls:
            env = warp_envelope_host(cref.chain_rows(cfg, mel)[0], controls["formant"], channel_centres(cfg["preprocess_config"]))
        return cref.controlled_oracle_audio(cfg, raw, wt, mel, noise, contour, env_rows=env)
    om = orc.OracleModel(cfg, raw, wt)
    T = mel.shape[1]
    gain = None
    if cfg["mbexwn_config"].get("normalize_rms_from_mell", False):
        mel, gain = orc.normalize_inputs_by_rms(mel, cfg, T * om.hop)
        mel = mel.astype(np.float32)
    if f0 is None and transposition == 1.0:
        audio = om.forward(mel, noise)
    else:
        mel64 = np.asarray(mel).astype(om.dtype)
        contour = om.generate_f0(mel64) if f0 is None else np.asarray(f0, dtype=np.float64)
        contour = (contour.astype(np.float32) * np.float32(transposition)).astype(np.float64)
        exc = om.generate_excitation(mel64, contour, noise)
        if om.mb.get("ps_off", False) or not om.mb.get("ps_use_stft", True):
            audio = exc[:, :T * om.hop]
        else:
            out_len = contour.shape[1] * int(om.sample_rate // om.pulse_rate)
            audio = om.istft(om.stft(exc, T) * om.generate_specenv(mel64, contour), out_len)[:, :T * om.hop]
    return audio if gain is None else audio * gain


def _get_run(torch, case, fill):
    key = (case[0], fill)
    if key not in _RUNS:
        _RUNS[key] = _run_forward(torch, case, fill)
    return _RUNS[key]


_FORWARD_PARAMS = [(fill, case[0]) for large in (False, True) for fill in FILLS for case in FORWARD_CASES
                   if (case[0].replace("backend-", "") in LARGE_IDS) == large]


@pytest.mark.gpu
@pytest.mark.parametrize("fill,cid", _FORWARD_PARAMS, ids=[f"{fill}-{cid}" for fill, cid in _FORWARD_PARAMS])
def test_forward_stays_inside_its_buffers_and_ignores_stale_scratch(torch, fill, cid):
    """One forward case under one fill: every guard untouched (inside _run_forward), the audio behind every item's own length
    zero; under ``zero`` the audio within E2E_TOL of the float64 oracle, under ``nan`` and ``huge`` the audio and every stage
    bit-identical to the ``zero`` run over every item's own valid range."""
    case = FORWARD[cid]
    _, model, lengths, items, kwargs, _, _ = case
    audio, stages = _get_run(torch, case, fill)
    eng, cfg, raw, wt = _engine(cid, model, kwargs)
    d = eng.dims
    hop = d.hop_size
    checked = list(range(len(lengths))) if items is None else list(items)
    for ii, ll in enumerate(lengths):
        assert np.all(_bits(audio[ii, ll * hop:]) == 0) or np.all(audio[ii, ll * hop:] == 0.0), \
            f"{cid} [{fill}]: audio behind item {ii}'s own length ({ll} frames) is not zero"
        assert np.all(np.isfinite(audio[ii, :ll * hop])), f"{cid} [{fill}]: audio of item {ii} is not finite"
    if fill == "zero":
        mel, noise, fw = _case_inputs(case, d)
        rpf = d.wn_in_rows_per_frame
        for ii in checked:
            ll = lengths[ii]
            ref = _oracle_audio(cfg, raw, wt, mel[ii:ii + 1, :ll], None if noise is None else noise[ii:ii + 1, :ll * rpf],
                                f0=fw["f0"][ii:ii + 1, :ll * d.pulse_per_frame] if "f0" in fw else None,
                                transposition=fw.get("transposition", 1.0),
                                controls={kk: int(fw[kk][ii]) if kk == "f0_item_mask" else fw[kk][ii:ii + 1, :ll]
                                          for kk in CONTROL_KEYS if kk in fw})[0]
            err = float(np.max(np.abs(audio[ii, :ll * hop].astype(np.float64) - ref)))
            bar = E2E_TOL * max(1.0, float(np.max(np.abs(ref))))
            print(f"\nmemory contract {cid}: item {ii} ({ll} frames) max|audio - oracle| {err:.3e} (bar {bar:.3e})")
            assert err <= bar, f"{cid}: audio of item {ii} is {err:.3e} from the oracle (bar {bar:.3e})"
        return
    base_audio, base_stages = _get_run(torch, case, "zero")
    for ii, ll in enumerate(lengths):
        where = _first_difference(audio[ii, :ll * hop], base_audio[ii, :ll * hop])
        assert where is None, f"{cid}: audio of item {ii} ({ll} frames) depends on the scratch content ({fill} against zero): " \
                              f"first at sample {where[0]}"
    assert set(stages) == set(base_stages)
    for name in stages:
        for ii, a, b in zip(checked, stages[name], base_stages[name]):
            where = _first_difference(a, b)
            assert where is None, f"{cid}: {name} of item {ii} ({lengths[ii]} frames) depends on the scratch content ({fill} " \
                                  f"against zero): first at {where}"


@pytest.mark.gpu
def test_workspace_reused_across_layouts(torch):
    """How the engine really runs: on one guarded workspace sized for the larger of the two, a VOICE forward in split half
    precision, then -- without refilling -- a SPEECH float32 forward of another batch shape, bit-identical to the same forward
    on a zero-filled workspace."""
    first = ("reuse-voice-split", twn.GEOMETRIES["voice"], twn.RAGGED, None, dict(F43, precision="split_f16"), {}, "wn")
    second = FORWARD["last-one-frame"]
    eng1 = _engine(first[0], first[1], first[4])[0]
    eng2, cfg2 = _engine(second[0], second[1], second[4])[:2]
    B1, T1, B2, T2 = len(first[2]), max(first[2]), len(second[2]), max(second[2])
    need = max(eng1.workspace_bytes(B1, T1), eng2.workspace_bytes(B2, T2))
    _ceps_region(torch, eng2, B2, T2)
    gs = GuardSet("nan", eng1.device)
    ws = _guarded_workspace(torch, gs, eng1, B1, T1, nbytes=need)
    try:
        audios = []
        for eng, case, B, T in ((eng1, first, B1, T1), (eng2, second, B2, T2)):
            d = eng.dims
            mel, noise, _ = _case_inputs(case, d)
            eng._workspace = ws.payload
            audio_g = gs.new("audio", B * T * d.hop_size * 4)
            out = eng.forward(gs.put("mel", mel).view(torch.float32, B, T, d.mel_channels),
                              n_frames=gs.put("n_frames", np.asarray(case[2], dtype=np.int32)).view(torch.int32),
                              noise=gs.put("noise", noise).view(torch.float32, B, -1), out=audio_g.view(torch.float32, B, -1))
            torch.cuda.synchronize()
            assert eng._workspace.data_ptr() == ws.ptr
            gs.check()
            audios.append(out.cpu().numpy())
        stages = _stages(torch, eng2, cfg2, second)
    finally:
        eng1._workspace = eng2._workspace = None
    assert np.all(np.isfinite(audios[0][1, :twn.RAGGED[1] * 300]))
    base_audio, base_stages = _get_run(torch, second, "zero")
    for ii, ll in enumerate(second[2]):
        where = _first_difference(audios[1][ii, :ll * 300], base_audio[ii, :ll * 300])
        assert where is None, f"audio of item {ii} depends on the previous forward's leftovers: first at sample {where[0]}"
        assert np.all(audios[1][ii, ll * 300:] == 0.0)
    for name in stages:
        for ii, (a, b) in enumerate(zip(stages[name], base_stages[name])):
            assert _first_difference(a, b) is None, f"{name} of item {ii} depends on the previous forward's leftovers"


# ------------------------------------------------------------------------------------------------------------------------
# stand-alone entry points
# ------------------------------------------------------------------------------------------------------------------------
def _small_engine():
    return _engine("standalone-small", parity.SMALL, {})[0]


def _status(eng, status):
    assert status == 0, f"status {status}: {eng._lib.mbx_last_error().decode()}"


def _conv_data(cid, cin, cout, ks, dil, mode, rows, prelu, B):
    rng = np.random.default_rng(cin * 1000 + cout + rows)
    x = rng.normal(size=(B, rows, cin)).astype(np.float32)
    w = (rng.normal(size=(ks, cin, cout)) / np.sqrt(ks * cin)).astype(np.float32)
    b = rng.normal(size=(cout,)).astype(np.float32)
    alpha = rng.uniform(0.05, 0.4, size=(cout,)).astype(np.float32) if prelu else None
    total = (ks - 1) * dil
    pl = total // 2 if mode == "CONSTANT" else (ks - 1) // 2 + ((ks - 1) % 2)
    return x, w, b, alpha, pl


def _call_conv(torch, f64, args, fill):
    eng = _small_engine()
    cin, cout, ks, dil, mode, rows, prelu, B = args
    x, w, b, alpha, pl = _conv_data(None, *args)
    gs = GuardSet(fill, eng.device)
    xg, wg, bg = gs.put("x", x), gs.put("w", w), gs.put("b", b)
    ag = gs.put("alpha", alpha) if prelu else None
    yg = gs.new("y", B * rows * cout * 4)
    fn = eng._lib.mbx_conv1d_f64acc if f64 else eng._lib.mbx_conv1d
    _status(eng, fn(eng._handle, xg.ptr, B, rows, cin, wg.ptr, bg.ptr, ag.ptr if ag else None, ks, cout, dil, pl, _PAD[mode], yg.ptr,
                    eng._stream()))
    torch.cuda.synchronize()

    def want():
        dv = lambda arr: torch.as_tensor(arr).cuda()      # noqa: E731
        return {"y": eng.conv1d(dv(x), dv(w), dv(b), dv(alpha) if prelu else None, dilation=dil, pad_l=pl, pad_mode=_PAD[mode],
                                f64_accumulate=f64).cpu().numpy().reshape(-1)}
    return gs, {"y": yg.view(torch.float32).cpu().numpy()}, want


def _call_lin_interp(torch, args, fill):
    eng = _small_engine()
    rows, ch, up = args
    x = np.random.default_rng(rows).normal(size=(2, rows, ch)).astype(np.float32)
    gs = GuardSet(fill, eng.device)
    xg, yg = gs.put("x", x), gs.new("y", 2 * rows * up * ch * 4)
    _status(eng, eng._lib.mbx_lin_interp(eng._handle, xg.ptr, 2, rows, ch, up, yg.ptr, eng._stream()))
    torch.cuda.synchronize()
    return gs, {"y": yg.view(torch.float32).cpu().numpy()}, \
        lambda: {"y": eng.lin_interp(torch.as_tensor(x).cuda(), up).cpu().numpy().reshape(-1)}


def _call_wavetable(torch, args, fill):
    eng = _small_engine()
    (n,) = args
    B, nch = 2, 1 + eng.dims.wt_subharm
    f0 = np.random.default_rng(n).uniform(60.0, 500.0, size=(B, n)).astype(np.float32)
    gs = GuardSet(fill, eng.device)
    fg, pg, hg = gs.put("f0", f0), gs.new("pulse", B * n * nch * 4), gs.new("phase", B * n * 4)
    sg = gs.new("scratch", B * (n + n // 1000 + 3) * 4)
    _status(eng, eng._lib.mbx_wavetable(eng._handle, fg.ptr, B, n, pg.ptr, hg.ptr, sg.ptr, eng._stream()))
    torch.cuda.synchronize()

    def want():
        pulse, phase = eng.wavetable(torch.as_tensor(f0).cuda())
        return {"pulse": pulse.cpu().numpy().reshape(-1), "phase": phase.cpu().numpy().reshape(-1)}
    return gs, {"pulse": pg.view(torch.float32).cpu().numpy(), "phase": hg.view(torch.float32).cpu().numpy()}, want


def _call_pqmf(torch, args, fill):
    eng = _small_engine()
    (steps,) = args
    M = eng.dims.subbands
    x = np.random.default_rng(steps).normal(size=(2, steps, M)).astype(np.float32)
    gs = GuardSet(fill, eng.device)
    xg, yg = gs.put("x", x), gs.new("y", 2 * steps * M * 4)
    _status(eng, eng._lib.mbx_pqmf_synthesis(eng._handle, xg.ptr, 2, steps, yg.ptr, eng._stream()))
    torch.cuda.synchronize()
    return gs, {"y": yg.view(torch.float32).cpu().numpy()}, \
        lambda: {"y": eng.pqmf_synthesis(torch.as_tensor(x).cuda()).cpu().numpy().reshape(-1)}


def _call_stft_filter(torch, args, fill):
    eng = _small_engine()
    (frames,) = args
    d = eng.dims
    rng = np.random.default_rng(frames)
    exc = rng.normal(size=(2, frames * d.hop_size)).astype(np.float32)
    ceps = (0.1 * rng.normal(size=(2, frames, d.n_ceps))).astype(np.float32)
    index = rng.integers(0, bref.N_LIFTER_ROWS, size=(2, frames)).astype(np.int32)
    gs = GuardSet(fill, eng.device)
    eg, cg, ig = gs.put("excitation", exc), gs.put("cepstrum", ceps), gs.put("ceps_index", index)
    ag, sg = gs.new("audio", 2 * frames * d.hop_size * 4), gs.new("scratch", 2 * frames * d.stft_win * 4)
    _status(eng, eng._lib.mbx_stft_filter(eng._handle, eg.ptr, cg.ptr, ig.ptr, 2, frames, ag.ptr, sg.ptr, eng._stream()))
    torch.cuda.synchronize()
    return gs, {"audio": ag.view(torch.float32).cpu().numpy()}, \
        lambda: {"audio": eng.stft_filter(torch.as_tensor(exc).cuda(), torch.as_tensor(ceps).cuda(),
                                          torch.as_tensor(index).cuda()).cpu().numpy().reshape(-1)}


def _call_mel_analysis(torch, args, fill):
    """Ragged n_samples whose longest item fills max_samples exactly, max_frames exactly max_samples / hop + 1; the rows
    behind an item's own frames are not written (analysis.compute_log_mel_device), so the comparison is cut to them."""
    from mbexwn_vocoder_amd import analysis
    from mbexwn_vocoder_amd.config import canonical_config
    eng = _small_engine()
    (counts,) = args
    cfg = canonical_config("SPEECH")["preprocess_config"]
    win, hop, fft, n_mels = int(cfg.get("win_size", cfg["fft_size"])), int(cfg["hop_size"]), int(cfg["fft_size"]), int(cfg["mel_channels"])
    B, N = len(counts), max(counts)
    frames = N // hop + 1
    sound = (0.3 * np.random.default_rng(N).normal(size=(B, N))).astype(np.float32)
    basis = analysis.mel_basis_slaney(cfg["sample_rate"], fft, n_mels, cfg["fmin"], cfg["fmax"], dtype=np.float32)
    nz = basis != 0
    lo = np.where(nz.any(axis=1), nz.argmax(axis=1), 1).astype(np.int32)
    hi = np.where(nz.any(axis=1), basis.shape[1] - 1 - nz[:, ::-1].argmax(axis=1), 0).astype(np.int32)
    ang = -2.0 * np.pi * np.arange(fft // 2) / fft
    gs = GuardSet(fill, eng.device)
    sg, ng = gs.put("audio", sound), gs.put("n_samples", np.asarray(counts, dtype=np.int32))
    tabs = [gs.put(name, arr) for name, arr in (("window", analysis.hann_symmetric(win).astype(np.float32)),
                                                ("twiddle", np.stack((np.cos(ang), np.sin(ang)), axis=1).astype(np.float32)),
                                                ("basis", basis), ("bin_lo", lo), ("bin_hi", hi))]
    og = gs.new("out", B * frames * n_mels * 4)
    with torch.cuda.device(eng.device):
        _status(eng, eng._lib.mbx_mel_analysis(sg.ptr, ng.ptr, B, N, win, hop, fft, n_mels, *(tt.ptr for tt in tabs),
                                               ctypes.c_float(float(np.finfo(np.float32).eps)), og.ptr, frames,
                                               torch.cuda.current_stream(eng.device).cuda_stream))
    torch.cuda.synchronize()
    cut = lambda arr: np.concatenate([arr.reshape(B, frames, n_mels)[ii, :nn // hop + 1].reshape(-1) for ii, nn in enumerate(counts)])  # noqa: E731

    def want():
        out, _ = analysis.compute_log_mel_device(torch.as_tensor(sound).cuda(), cfg, torch.as_tensor(counts, dtype=torch.int32).cuda())
        return {"out": cut(out.cpu().numpy())}
    return gs, {"out": cut(og.view(torch.float32).cpu().numpy())}, want


def _call_norm_mel(torch, args, fill):
    eng = _engine("standalone-normmel", tbe.GEOMETRIES["normmel"], {})[0]
    (lengths,) = args
    d = eng.dims
    B, T, hop = len(lengths), max(lengths), d.hop_size
    mel, _ = synthetic_inputs(5, B, T)
    gs = GuardSet(fill, eng.device)
    mg, ng = gs.put("mel", mel), gs.put("n_frames", np.asarray(lengths, dtype=np.int32))
    og, gg, sg = gs.new("mel_out", mel.nbytes), gs.new("gain", B * T * hop * 4), gs.new("scratch", 2 * B * T * 4)
    _status(eng, eng._lib.mbx_norm_mel(eng._handle, mg.ptr, ng.ptr, B, T, og.ptr, gg.ptr, sg.ptr, eng._stream()))
    torch.cuda.synchronize()

    def cut(mel_out, gain):
        return {"mel_out": np.concatenate([mel_out.reshape(B, T, -1)[ii, :ll].reshape(-1) for ii, ll in enumerate(lengths)]),
                "gain": np.concatenate([gain.reshape(B, T * hop)[ii, :ll * hop] for ii, ll in enumerate(lengths)])}

    def want():
        out, gain = eng.norm_mel_stage(torch.as_tensor(mel).cuda(), torch.as_tensor(lengths, dtype=torch.int32).cuda())
        return cut(out.cpu().numpy(), gain.cpu().numpy())
    return gs, cut(og.view(torch.float32).cpu().numpy(), gg.view(torch.float32).cpu().numpy()), want


def _call_encode_flac(torch, args, fill):
    """out_bytes exactly the frames of the items; the guard behind the last frame and the guard behind max_abs are the ones
    that matter (the kernel writes the 16-byte words a frame shares with its neighbour byte by byte)."""
    eng = _small_engine()
    (counts,) = args
    B, stride = len(counts), max(counts)
    rate = int(eng.dims.sample_rate)
    audio = np.clip(0.5 * np.random.default_rng(11).standard_normal((B, stride)), -1.3, 1.3).astype(np.float32)
    total = sum(flac.frames_bytes(nn) for nn in counts)
    gs = GuardSet(fill, eng.device)
    ag = gs.put("audio", audio)
    tg = gs.put("crc_tables", flac.crc16_device_tables())
    og, mg = gs.new("out", total), gs.new("max_abs", B * 4)
    counts_c = (ctypes.c_int64 * B)(*counts)
    with torch.cuda.device(eng.device):
        _status(eng, eng._lib.mbx_encode_flac16(ag.ptr, stride, B, counts_c, rate, tg.ptr, og.ptr, total, mg.ptr, eng._stream()))
    torch.cuda.synchronize()

    def want():
        res = eng.encode_flac16(torch.as_tensor(audio).cuda(), counts)
        return {"out": np.concatenate([res.frames(bb) for bb in range(B)]), "max_abs": np.asarray(res.max_abs)}
    return gs, {"out": og.payload.cpu().numpy(), "max_abs": mg.view(torch.float32).cpu().numpy()}, want


def _window_data(eng, T, news, seed):
    d = eng.dims
    rng = np.random.default_rng(seed)
    B = 3
    mel = rng.normal(size=(B, T, d.mel_channels)).astype(np.float32)
    noise = rng.normal(size=(B, T * d.steps_per_frame)).astype(np.float32)
    new = [(rng.normal(size=(B, nn, d.mel_channels)).astype(np.float32),
            rng.normal(size=(B, nn * d.steps_per_frame)).astype(np.float32)) for nn in news]
    return B, mel, noise, new


def _call_window_advance(torch, args, fill):
    eng = _small_engine()
    T, step = args
    B, mel, noise, new = _window_data(eng, T, [step], 3)
    gs = GuardSet(fill, eng.device)
    mg, ng = gs.put("mel_window", mel), gs.put("noise_window", noise)
    mn, nn = gs.put("mel_new", new[0][0]), gs.put("noise_new", new[0][1])
    _status(eng, eng._lib.mbx_window_advance(eng._handle, mg.ptr, mn.ptr, ng.ptr, nn.ptr, B, T, step, eng._stream()))
    torch.cuda.synchronize()

    def want():
        md, nd = torch.as_tensor(mel).cuda(), torch.as_tensor(noise).cuda()
        eng.window_advance(md, torch.as_tensor(new[0][0]).cuda(), nd, torch.as_tensor(new[0][1]).cuda())
        return {"mel_window": md.cpu().numpy().reshape(-1), "noise_window": nd.cpu().numpy().reshape(-1)}
    return gs, {"mel_window": mg.view(torch.float32).cpu().numpy(), "noise_window": ng.view(torch.float32).cpu().numpy()}, want


def _call_window_update(torch, args, fill):
    eng = _small_engine()
    T, ticks = args
    B, mel, noise, new = _window_data(eng, T, [tt[2] for tt in ticks], 4)
    gs = GuardSet(fill, eng.device)
    mg, ng = gs.put("mel_window", mel), gs.put("noise_window", noise)
    for (shift, keep, count), (mel_new, noise_new) in zip(ticks, new):
        mn, nn = gs.put("mel_new", mel_new), gs.put("noise_new", noise_new)
        _status(eng, eng._lib.mbx_window_update(eng._handle, mg.ptr, mn.ptr, ng.ptr, nn.ptr, B, T, shift, keep, count, eng._stream()))
    torch.cuda.synchronize()

    def want():
        md, nd = torch.as_tensor(mel).cuda(), torch.as_tensor(noise).cuda()
        for (shift, keep, _), (mel_new, noise_new) in zip(ticks, new):
            eng.window_update(md, torch.as_tensor(mel_new).cuda(), nd, torch.as_tensor(noise_new).cuda(), shift, keep)
        return {"mel_window": md.cpu().numpy().reshape(-1), "noise_window": nd.cpu().numpy().reshape(-1)}
    return gs, {"mel_window": mg.view(torch.float32).cpu().numpy(), "noise_window": ng.view(torch.float32).cpu().numpy()}, want


def _call_emit_rows(torch, args, fill):
    """first + count at the row's end; the pinned host buffer is guarded like the device ones."""
    eng = _small_engine()
    B, n, first, count = args
    assert first + count == n
    audio = np.random.default_rng(9).normal(size=(B, n)).astype(np.float32)
    gs = GuardSet(fill, eng.device)
    ag = gs.put("audio", audio)
    hg = Guarded("host_out", B * count * 4, fill, pinned=True)
    gs.buffers.append(hg)
    _status(eng, eng._lib.mbx_emit_rows(eng._handle, ag.ptr, n, B, first, count, hg.ptr, eng._stream()))
    torch.cuda.synchronize()

    def want():
        host = torch.empty((B, count), dtype=torch.float32).pin_memory()
        eng.emit_rows(torch.as_tensor(audio).cuda(), first, count, host)
        torch.cuda.synchronize()
        return {"host_out": host.numpy().reshape(-1).copy()}
    return gs, {"host_out": hg.view(torch.float32).numpy().copy()}, want


_CALLS = {
    "mbx_conv1d": lambda torch, args, fill: _call_conv(torch, False, args, fill),
    "mbx_conv1d_f64acc": lambda torch, args, fill: _call_conv(torch, True, args, fill),
    "mbx_lin_interp": _call_lin_interp, "mbx_wavetable": _call_wavetable, "mbx_pqmf_synthesis": _call_pqmf,
    "mbx_stft_filter": _call_stft_filter, "mbx_mel_analysis": _call_mel_analysis, "mbx_norm_mel": _call_norm_mel,
    "mbx_encode_flac16": _call_encode_flac, "mbx_window_advance": _call_window_advance, "mbx_window_update": _call_window_update,
    "mbx_emit_rows": _call_emit_rows,
}
_STANDALONE_PARAMS = [(sym, cid, args) for sym, cases in STANDALONE.items() for cid, args in cases]


@pytest.mark.gpu
@pytest.mark.parametrize("symbol,cid,args", _STANDALONE_PARAMS, ids=[f"{sym}-{cid}" for sym, cid, _ in _STANDALONE_PARAMS])
def test_entry_point_stays_inside_its_buffers(torch, symbol, cid, args):
    """A stand-alone entry point with guarded inputs and outputs of exactly the stated sizes under the three fills: no guard
    is touched, the outputs are bit-identical across the fills and equal to what the engine's own wrapper returns."""
    results = {}
    want = None
    for fill in FILLS:
        gs, outputs, wrapper = _CALLS[symbol](torch, args, fill)
        gs.check()
        results[fill] = outputs
        if want is None:
            want = wrapper()
    for fill in FILLS:
        assert set(results[fill]) == set(want)
        for name, arr in results[fill].items():
            assert arr.shape == want[name].shape, f"{symbol} {cid} [{fill}]: {name} has {arr.shape}, the wrapper's {want[name].shape}"
            where = _first_difference(arr, want[name])
            assert where is None, f"{symbol} {cid} [{fill}]: {name} differs from the wrapper's result, first at {where}"
            assert _first_difference(arr, results["zero"][name]) is None, f"{symbol} {cid}: {name} depends on the fill ({fill})"


@pytest.mark.gpu
def test_the_detector_reports_a_row_it_is_told_is_guard(torch):
    """mbx_conv1d (batch 1) with a perfectly valid output buffer, while the checker is told that the payload is one output row
    shorter than it is: the kernel's legitimate last row counts as guard and must be reported on the ``behind`` side from
    offset 0 with cout x 4 changed bytes.  Integer-valued operands make the outputs small whole numbers, none of whose bytes is
    the 0xFF of the fill.  Everything stays inside one allocation."""
    eng = _small_engine()
    rows, cin, cout = 5, 4, 7
    x = np.arange(1, rows * cin + 1, dtype=np.float32).reshape(1, rows, cin) % 5 + 1
    w = (np.arange(cin * cout, dtype=np.float32).reshape(1, cin, cout) % 3 + 1)
    want = x[0] @ w[0]
    assert not np.any(want.astype(np.float32).view(np.uint8) == 0xFF) and np.all(want > 0)
    gs = GuardSet("nan", eng.device)
    xg, wg, yg = gs.put("x", x), gs.put("w", w), gs.new("y", rows * cout * 4)
    _status(eng, eng._lib.mbx_conv1d(eng._handle, xg.ptr, 1, rows, cin, wg.ptr, None, None, 1, cout, 1, 0, 0, yg.ptr, eng._stream()))
    torch.cuda.synchronize()
    gs.check()                                                      # told the truth, the checker finds nothing
    assert np.array_equal(yg.view(torch.float32, rows, cout).cpu().numpy(), want)
    assert yg.hits(payload_bytes=(rows - 1) * cout * 4) == [{"name": "y", "side": "behind", "first": 0, "last": cout * 4 - 1,
                                                             "count": cout * 4, "fill": "nan"}]


# ------------------------------------------------------------------------------------------------------------------------
# host-side refusals: nothing is launched, nothing is written
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["mbx_forward", "mbx_forward_ex", "mbx_forward_stream", "mbx_calibrate", "mbxe_forward"])
@pytest.mark.parametrize("fill", FILLS)
def test_short_or_misaligned_workspace_is_refused_before_any_launch(torch, fill, entry):
    """workspace_bytes one less than mbx_workspace_size -> MBX_ERR_WORKSPACE; a workspace pointer at +128 bytes ->
    MBX_ERR_INVALID_ARGUMENT (check_forward_args of csrc/mbx_forward.hip checks both in front of the first launch, and mbx_calibrate's
    first forward is refused the same way); every byte of audio, workspace and guards is still the fill."""
    from mbexwn_vocoder_amd.engine import mbx_forward_options
    eng = _small_engine()
    lib, d = eng._lib, eng.dims
    B, T = 2, 9
    need = eng.workspace_bytes(B, T)
    assert need == int(lib.mbx_workspace_size(eng._handle, B, T)) and need > 256
    mel, noise = synthetic_inputs(3, B, T)
    gs = GuardSet(fill, eng.device)
    ws, audio = gs.new("workspace", need), gs.new("audio", B * T * d.hop_size * 4)
    mel_g, noise_g = gs.put("mel", mel), gs.put("noise", noise)
    state = gs.put("state_in", np.zeros((B, 6), dtype=np.int32))
    state_out = gs.new("state_out", B * 6 * 4)
    # mbxe_forward with all three env arguments given: the factors, the centre table, the caller's scratch of the warped rows
    env_factor = gs.put("env_factor", np.full((B, T), 1.25, dtype=np.float32))
    env_mel = gs.new("env_mel", B * T * d.mel_channels * 4)
    centres = eng._envelope_centres()
    opt = mbx_forward_options()
    opt.struct_size = ctypes.sizeof(mbx_forward_options)
    opt.transposition = 1.0

    def call(ptr, nbytes):
        if entry == "mbx_forward":
            return lib.mbx_forward(eng._handle, mel_g.ptr, None, B, T, noise_g.ptr, audio.ptr, ptr, nbytes, eng._stream())
        if entry == "mbx_forward_ex":
            return lib.mbx_forward_ex(eng._handle, mel_g.ptr, None, B, T, noise_g.ptr, audio.ptr, ptr, nbytes, ctypes.byref(opt),
                                      eng._stream())
        if entry == "mbx_forward_stream":
            return lib.mbx_forward_stream(eng._handle, mel_g.ptr, None, B, T, noise_g.ptr, audio.ptr, ptr, nbytes, state.ptr,
                                          state_out.ptr, eng._stream())
        if entry == "mbxe_forward":
            return lib.mbxe_forward(eng._handle, mel_g.ptr, None, B, T, noise_g.ptr, audio.ptr, ptr, nbytes, ctypes.byref(opt),
                                    env_factor.ptr, centres.data_ptr(), env_mel.ptr, eng._stream())
        return lib.mbx_calibrate(eng._handle, mel_g.ptr, None, B, T, noise_g.ptr, ptr, nbytes, eng._stream())

    before = eng.conv_form_info()
    assert call(ws.ptr, need - 1) == 3, lib.mbx_last_error().decode()                  # MBX_ERR_WORKSPACE
    assert "workspace too small" in lib.mbx_last_error().decode()
    assert call(ws.ptr + 128, need - 128) == 1, lib.mbx_last_error().decode()          # MBX_ERR_INVALID_ARGUMENT
    assert "256-byte aligned" in lib.mbx_last_error().decode()
    torch.cuda.synchronize()
    gs.check()
    assert ws.payload_untouched() and audio.payload_untouched() and state_out.payload_untouched() and env_mel.payload_untouched()
    assert eng.conv_form_info()["form"] == before["form"]


# ------------------------------------------------------------------------------------------------------------------------
# streaming: nothing is carried in the workspace between ticks
# ------------------------------------------------------------------------------------------------------------------------
def _streams_carry_nothing(torch, controlled):
    """The 80 ms schedule (6 / 6 / 7 / 6 / 7 frames) on a handful of streams of the small streaming model, the engine's
    workspace refilled with NaN between the ticks (an ordinary memset between graph replays): bit-equal to the undisturbed
    run.  The header names no state that lives in the workspace; what a stream carries lives in the caller's stores.
    controlled: stream 0 is pushed with a formant shift and a transposition, both changing from frame to frame, and the
    engine's scratch of the warped rows (env_mel of mbxe_forward) is refilled with the workspace."""
    import test_gpu_streaming as tstream
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    lengths = [140, 140, 93, 140, 8]       # long streams in step (steady ticks replay a graph), one that ends early, a short one

    def run(poison):
        cfg, raw, wt = build_case("SPEECH", tstream.SMALL)
        eng = MBExWNEngine(cfg, raw, wt)
        syn = StreamingSynthesizer(eng, chunk_frames=(6, 6, 7, 6, 7))
        pending = {}
        for sid, ll in enumerate(lengths):
            mel, noise = synthetic_inputs(100 + sid, 1, ll)
            pending[sid] = (mel[0], noise[0], 0)
            syn.open(sid)
        rng = np.random.default_rng(99)
        formant = cref.formant_rows(rng, 1, lengths[0])[0]
        scale = rng.uniform(0.5, 2.0, size=lengths[0]).astype(np.float32)
        got = {sid: [] for sid in pending}
        for _ in range(400):
            for sid, (mel, noise, pos) in pending.items():
                if pos < mel.shape[0]:
                    end = min(pos + 8, mel.shape[0])
                    extra = {"formant": formant[pos:end], "transposition": scale[pos:end]} if controlled and sid == 0 else {}
                    syn.push(sid, mel[pos:end], noise[pos * 20:end * 20], last=end == mel.shape[0], **extra)
                    pending[sid] = (mel, noise, end)
            if poison and eng._env_mel is not None:
                eng._env_mel.view(torch.uint8).fill_(0xFF)
            if poison and eng._workspace is not None:
                eng._workspace.fill_(0xFF)
                # the integer region of the last tick's layout (the layout of a steady tick and of every graph replay) gets a
                # valid lifter row, as everywhere in this file
                ptr, cnt, stride = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
                if eng._lib.mbx_stage(eng._handle, b"ceps_index", ctypes.byref(ptr), ctypes.byref(cnt), ctypes.byref(stride)) == 0:
                    offset, nbytes = ptr.value - eng._workspace.data_ptr(), 4 * eng._last_shape[0] * stride.value
                    if 0 <= offset and offset + nbytes <= eng._workspace.numel():
                        eng._workspace[offset:offset + nbytes].view(torch.int32).fill_(bref.N_LIFTER_ROWS - 1)
            for sid, audio in syn.tick().items():
                got[sid].append(np.array(audio, copy=True))
            if all(syn.finished(sid) for sid in pending):
                break
        torch.cuda.synchronize()
        assert (syn._formant, syn._control) == (controlled, controlled) and (eng._env_mel is not None) == controlled
        eng.close()
        return {sid: np.concatenate(vv) for sid, vv in got.items()}, syn.graph_ticks

    plain, plain_graph_ticks = run(False)
    poisoned, graph_ticks = run(True)
    print(f"\nstreams: {graph_ticks} ticks served by a graph replay ({plain_graph_ticks} in the undisturbed run)")
    assert graph_ticks == plain_graph_ticks
    for sid, ll in enumerate(lengths):
        assert plain[sid].shape == (ll * 300,) and np.all(np.isfinite(plain[sid]))
        where = _first_difference(poisoned[sid], plain[sid])
        assert where is None, f"stream {sid}: the audio depends on what the workspace held between ticks, first at sample {where[0]}"


@pytest.mark.gpu
def test_streams_carry_nothing_in_the_workspace(torch):
    _streams_carry_nothing(torch, False)


@pytest.mark.gpu
def test_controlled_streams_carry_nothing_in_the_workspace(torch):
    """The same run with one stream pushed with ``formant`` and ``transposition``: the ticks go through mbxe_forward with the
    control rows of their whole windows, and neither the workspace nor the scratch of the warped rows carries anything."""
    _streams_carry_nothing(torch, True)

"""The C-ABI library builds on a CPU-only host and the binding lists what include/mbexwn.h declares; the policy fields of
mbx_config and the kernel-code names (no compute calls here).  The exports, every parameter and the layout of every
structure: test_abi_headers.py."""
import ctypes
import os
import re

import pytest

import c_headers
from mbexwn_vocoder_amd import abi, engine
from mbexwn_vocoder_amd.build import LIB_PATH, build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mbexwn.h")


def test_library_exports_every_declared_symbol():
    """(that the library exports each of them, and each function of the other headers: test_abi_headers.py)"""
    build_library()
    assert os.path.exists(LIB_PATH)
    names = [name for name, _, _ in c_headers.prototypes(c_headers.read_code("mbexwn.h"))]
    assert "mbx_forward" in names and "mbx_create" in names and len(names) >= 12
    assert engine.EXPORTED_SYMBOLS == abi.symbols("mbexwn.h") == names
    assert engine.AUDIO_SYMBOLS == abi.symbols("mbexwn_audio.h")         # the two lists the build hook reads


def test_policy_fields_and_experiment_variables(monkeypatch, capsys):
    """The library reads no environment variable: the policy is mbx_config fields, which the Python host fills from its
    arguments -- or, for the experiment scripts, from the MBX_* variables, naming them on stderr."""
    from helpers import build_case
    cfg, raw, wt = build_case("SPEECH", {})
    for kk in ("MBX_WINOGRAD", "MBX_FOLD_SKIP", "MBX_FOLD_START", "MBX_WG_SMALL", "MBX_RV_TILES", "MBX_RV_SPLIT", "MBX_EXPERIMENT"):
        monkeypatch.delenv(kk, raising=False)
    cc, _ = engine.make_config(cfg, wt)
    assert (cc.wn_conv_form, cc.batch_invariant, cc.wn_keep_skip, cc.wn_keep_start, cc.tune_gate_shape) == (0, 0, 0, 0, 0)
    assert capsys.readouterr().err == ""
    cc, _ = engine.make_config(cfg, wt, conv_form="f23", batch_invariant=True, keep_start=True, tune={"resskip_split": 2})
    assert (cc.wn_conv_form, cc.batch_invariant, cc.wn_keep_start, cc.tune_resskip_split) == (2, 1, 1, 2)
    monkeypatch.setenv("MBX_WINOGRAD", "44")
    monkeypatch.setenv("MBX_FOLD_START", "0")
    monkeypatch.setenv("MBX_WG_SMALL", "1")
    monkeypatch.delenv("MBX_EXPERIMENT", raising=False)
    cc, _ = engine.make_config(cfg, wt)                                # without the opt-in the variables are ignored, loudly
    assert (cc.wn_conv_form, cc.batch_invariant, cc.wn_keep_start, cc.tune_gate_shape) == (0, 0, 0, 0)
    assert "ignoring MBX_WINOGRAD=44" in capsys.readouterr().err
    monkeypatch.setenv("MBX_EXPERIMENT", "1")
    cc, _ = engine.make_config(cfg, wt)
    assert (cc.wn_conv_form, cc.batch_invariant, cc.wn_keep_start, cc.tune_gate_shape) == (3, 1, 1, 2)
    assert "MBX_WINOGRAD=44" in capsys.readouterr().err
    cc, _ = engine.make_config(cfg, wt, conv_form="direct")           # an explicit argument wins over the variable
    assert cc.wn_conv_form == 1
    with pytest.raises(ValueError):
        engine.make_config(cfg, wt, conv_form="f63")
    csrc = os.path.join(ROOT, "mbexwn_vocoder_amd", "csrc")
    sources = sorted(os.listdir(csrc))
    assert {"mbx_api.hip", "mbx_create.hip", "mbx_forward.hip", "mbx_handle.h"} <= set(sources)
    for name in sources:
        assert "getenv" not in open(os.path.join(csrc, name)).read(), name


def test_make_config_and_tensor_table():
    from helpers import build_case
    cfg, raw, wt = build_case("VOICE", {})
    cconf, dims = engine.make_config(cfg, wt)
    assert cconf.struct_size == ctypes.sizeof(engine.mbx_config) and cconf.wn_channels == 340
    assert [cconf.wn_dilations[ii] for ii in range(5)] == [1, 2, 4, 8, 16]
    assert cconf.n_f0_ops == 9 and cconf.n_vtf_ops == 5   # 3x(conv,prelu) + final conv + lin + act ; 2x(conv,prelu) + final conv
    assert cconf.f0_ops[0].name == b"PulsPar_Layer_0" and cconf.f0_ops[8].act == 1
    tensors = engine.tensor_table(cfg, raw, wt)
    assert tensors["wn.conv1D_0.w"].shape == (3, 340, 680) and tensors["table.pqmf_syn"].shape == (121, 15)
    assert tensors["wn.res_skip_4.w"].shape == (1, 340, 340) and tensors["table.wavetables"].shape == (513, 15)
    assert all(vv.dtype.name == "float32" and vv.flags["C_CONTIGUOUS"] for vv in tensors.values())


def test_engine_refuses_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from helpers import build_case
    cfg, raw, wt = build_case("SPEECH", {})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.MBExWNEngine(cfg, raw, wt)


def test_gate_kernel_codes_match_the_header():
    """mbx_conv_form_info.gate_kernel[] (ABI 10; the version literal follows MBX_ABI_VERSION): the MBX_GATE_K_* codes of include/mbexwn.h and the names engine.py reports."""
    import re
    from mbexwn_vocoder_amd import engine
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mbexwn.h")).read()
    codes = {name: int(val) for name, val in re.findall(r"#define MBX_GATE_K_(\w+) (\d+)", header)}
    assert sorted(codes.values()) == sorted(engine.GATE_KERNEL_NAMES)
    want = {"NONE": "none", "DIRECT": "direct", "F23": "f23", "F43": "f43", "F43_PSPLIT": "f43_psplit", "F43_HSPLIT": "f43_hsplit",
            "F43_STRIDED": "f43_strided", "F43_STRIDED_PSPLIT": "f43_strided_psplit", "FOLDED_START": "folded_start",
            "SPLIT_F16": "split_f16", "SPLIT_F16_WIDE": "split_f16_wide", "SPLIT_F16_F32H": "split_f16_f32h"}
    assert {engine.GATE_KERNEL_NAMES[vv]: kk for kk, vv in codes.items()} == {vv: kk for kk, vv in want.items()}
    assert int(re.search(r"#define MBX_ABI_VERSION (\d+)", header).group(1)) == engine.MBX_ABI_VERSION == 11
    # bench.py's executed-FLOP factors know every kernel that multiplies
    import bench
    assert set(bench.GATE_EXECUTED) == set(engine.GATE_KERNEL_NAMES.values()) - {"none", "folded_start", "split_f16", "split_f16_wide",
                                                                                     "split_f16_f32h"}


def test_resskip_and_tail_kernel_codes_match_the_header():
    """mbx_kernel_report (ABI 11): the MBX_RESSKIP_K_* and MBX_TAIL_K_* codes of include/mbexwn.h and the names engine.py reports;
    every code's comment names its kernel."""
    header = open(HEADER).read()
    for prefix, names, want in (
            ("RESSKIP", engine.RESSKIP_KERNEL_NAMES,
             {"NONE": "none", "CONV1D": "conv1d", "PACKED64": "packed64", "PACKED128": "packed128", "WIDE11_RES10": "wide11_res10",
              "WIDE11": "wide11", "WIDE6X2": "wide6x2", "WAVE11": "wave11", "WAVE12": "wave12", "WAVE6X2": "wave6x2",
              "WAVE4X3": "wave4x3", "SPLIT_F16": "split_f16"}),
            ("TAIL", engine.TAIL_KERNEL_NAMES,
             {"NONE": "none", "UNFUSED": "unfused", "TAIL2_NJ4": "tail2_nj4", "TAIL2_NJ8": "tail2_nj8", "TAIL2_NJ12": "tail2_nj12",
              "TAIL2_NJ20": "tail2_nj20", "TAIL2_NJ22": "tail2_nj22", "TAIL": "tail"})):
        defs = re.findall(rf"#define MBX_{prefix}_K_(\w+) (\d+)[ \t]*(/\*.*?\*/)?", header)
        codes = {name: int(val) for name, val, _ in defs}
        assert sorted(codes.values()) == sorted(names) == list(range(len(names)))
        assert {names[vv]: kk for kk, vv in codes.items()} == {vv: kk for kk, vv in want.items()}
        for name, _, comment in defs:
            assert name == "NONE" or "kernel" in comment or "conv" in comment, f"MBX_{prefix}_K_{name}: no kernel named"
    templ = dict(re.findall(r"#define MBX_RESSKIP_K_(\w+) \d+\s*/\* (\w+(?:<[\d,]+>)?)", header))
    assert templ["PACKED64"] == "wn_resskip_kernel<1,2>" and templ["PACKED128"] == "wn_resskip_kernel<2,3>"
    assert templ["WIDE11_RES10"] == "wn_resskip_wide_kernel<11,1,10>" and templ["WIDE11"] == "wn_resskip_wide_kernel<11,1,0>"
    assert templ["WIDE6X2"] == "wn_resskip_wide_kernel<6,2,0>" and templ["WAVE11"] == "wn_resskip_wave_kernel<11,3>"
    assert templ["WAVE12"] == "wn_resskip_wave_kernel<12,3>" and templ["WAVE6X2"] == "wn_resskip_wave_kernel<6,4>"
    assert templ["WAVE4X3"] == "wn_resskip_wave_kernel<4,4>"
    info = engine.mbx_kernel_report_info()
    assert len(info.resskip_kernel) == engine.MBX_MAX_WN_LAYERS

"""The gate plan of the stage cases without a GPU: tests/tools/wn_plan_stage_cases.cpp, a stand-alone host program on
csrc/wn_plan.h, is given the mbx_config fields and the launch size of every case of test_gpu_wavenet_stages.CASES and prints
each layer's kernel / shape / block_channels / cr / vs_arg; instantiations() maps such a row and the model's gate activation
to the kernel instantiations launch_wn_gate_winograd4w launches for it (csrc/wn_winograd4w.hip)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mbexwn_vocoder_amd", "csrc")
TOOLS = os.path.join(ROOT, "tests", "tools")
SOURCE = os.path.join(TOOLS, "wn_plan_stage_cases.cpp")
LAUNCHER = os.path.join(CSRC, "wn_winograd4w.hip")
K_F43, K_PSPLIT, K_HSPLIT, K_STRIDED, K_STRIDED_PSPLIT = 3, 4, 5, 6, 7         # MBX_GATE_K_* of the F(4,3) kernels


def case_line(cid, geometry, lengths, kwargs, no_start_f16=False):
    """The input line of a stage case: the fields of the mbx_config the engine would create it with (make_config)."""
    from helpers import canonical_config, wavetables_for
    from mbexwn_vocoder_amd.engine import make_config
    voice, over = geometry
    cc, dims = make_config(canonical_config(voice, **over), wavetables_for(voice), **kwargs)
    assert not dims.wn_multi and dims.wn_in_rows_per_frame == cc.steps_per_frame
    fields = [cc.wn_channels, cc.wn_out_channels, 15, cc.wn_layers, cc.cond_lin_upsampling, cc.wn_kernel_size, cc.wn_causal,
              cc.wn_gate_activation, cc.pulse_channels * (1 + cc.wt_subharm_channels), cc.wn_conv_form, cc.batch_invariant,
              cc.wn_keep_skip, cc.wn_keep_start, cc.tune_gate_shape, cc.tune_resskip_wave_tiles, cc.tune_resskip_split,
              cc.wn_precision, int(no_start_f16), len(lengths), max(lengths), cc.steps_per_frame, cc.cond_conv_upsampling,
              *(cc.wn_dilations[ll] for ll in range(cc.wn_layers))]
    return " ".join([cid, *(str(int(ff)) for ff in fields)]), int(cc.wn_channels), int(cc.wn_gate_activation)


def build(tmp, name="wn_plan_stage_cases", extra=("-O1",)):
    exe = os.path.join(str(tmp), name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC, SOURCE, "-o", exe], check=True)
    return exe


def run(exe, lines):
    """{case id: [(kernel, shape, block_channels, cr, vs_arg) per layer]} of the input lines."""
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(lines)
    rows = {}
    for line in out:
        parts = [pp.strip() for pp in line.split("|")]
        assert parts[1] == "st=0", line
        rows[parts[0]] = [tuple(int(vv) for vv in gg.split("/")) for gg in parts[2][2:].split()]
    return rows


def stage_case_lines(twn):
    """(lines, {case id: (C, gate activation code)}) of every case of test_gpu_wavenet_stages (the module `twn`)."""
    lines, model = [], {}
    for cid, geom, lkey, kwargs, _ in twn.CASES:
        line, C, act = case_line(cid, twn.GEOMETRIES[geom], twn.LENGTHS[lkey][0], kwargs, cid in twn.NO_START_F16)
        lines.append(line)
        model[cid] = (C, act)
    return lines, model


def instantiations(row, C, act):
    """The kernels launch_wn_gate_winograd4w launches for one layer's plan row, as it spells them."""
    kernel, shape, _, cr, vs_arg = row
    ga = "0" if act == 0 else "-1"
    if kernel not in (K_F43, K_PSPLIT, K_HSPLIT, K_STRIDED, K_STRIDED_PSPLIT):
        return set()
    if shape == 3:
        # pairs of column tiles; an odd last tile goes to a launch of the one-tile kernel (CR = 28)
        odd = {f"wn_gate_winograd4w_kernel<28,{ga}>"} if ((C + 31) // 32) % 2 else set()
        return {f"wn_gate_winograd4q_kernel<{ga}>"} | odd
    if shape == 2:
        return {f"wn_gate_winograd4h_kernel<{ga}>"}
    if vs_arg:
        return {f"wn_gate_winograd4p_kernel<{ga},1>" if shape == 1 else f"wn_gate_winograd4w_kernel<28,{ga},{vs_arg}>"}
    return {f"wn_gate_winograd4p_kernel<{ga}>" if shape == 1 else f"wn_gate_winograd4w_kernel<{cr},{ga}>"}


def launcher_instantiations():
    """Every instantiation a hipLaunchKernelGGL line of csrc/wn_winograd4w.hip names, blanks removed."""
    text = open(LAUNCHER).read()
    found = re.findall(r"hipLaunchKernelGGL\(\(?\s*(wn_gate_winograd4\w_kernel<[^>]*>)", text)
    assert len(found) == text.count("hipLaunchKernelGGL")
    return {ff.replace(" ", "") for ff in found}

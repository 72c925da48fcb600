// Prints the gate plan of the stage cases of tests/test_gpu_wavenet_stages.py: a stand-alone host program on the planner
// header alone (tests/test_wn_stage_plan_host.py builds and runs it, once more under the address and undefined-behaviour
// sanitizers).  One case per line of standard input, the fields of mbx_config and of the launch that selection looks at:
//   name C n_out M L cond_up ks causal gate_act pulse_channels conv_form batch_invariant keep_skip keep_start
//   tune_gate_shape tune_resskip_wave_tiles tune_resskip_split split_f16 no_start_f16 B frames steps_per_frame cond_conv_up
//   dilation[0] .. dilation[L - 1]
// The policy is derived from them as mbx_create does for a handle with every weight image (no_start_f16: but layer 0's split
// res/skip image) on a device that grants every dynamic-LDS size, the geometry as mbx_plan does for a whole-item forward.
// One line out per case: name | st=<status> | g=<kernel/shape/block_channels/cr/vs_arg per layer>.
#include "wn_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string name;
        int C, n_out, M, L, cond_up, ks, causal, gate_act, pulse_channels, form, batch_invariant, keep_skip, keep_start;
        int tune_gate_shape, wave_tiles, resskip_split, split, no_start_f16, B, frames, spf, cond_conv_up;
        in >> name >> C >> n_out >> M >> L >> cond_up >> ks >> causal >> gate_act >> pulse_channels >> form >> batch_invariant >>
            keep_skip >> keep_start >> tune_gate_shape >> wave_tiles >> resskip_split >> split >> no_start_f16 >> B >> frames >>
            spf >> cond_conv_up;
        if (!in || L < 1 || L > MBX_MAX_WN_LAYERS) {
            std::fprintf(stderr, "bad case line: %s\n", line.c_str());
            return 2;
        }
        mbx::WnPolicy p;
        p.C = C, p.n_out = n_out, p.M = M, p.L = L, p.cond_up = cond_up, p.ks = ks, p.causal = causal, p.gate_act = gate_act;
        p.pulse_channels = pulse_channels;
        for (int l = 0; l < L; ++l) {
            in >> p.dil[l];
            p.img[l] = 127;
        }
        if (!in) {
            std::fprintf(stderr, "bad case line: %s\n", line.c_str());
            return 2;
        }
        if (no_start_f16) p.img[0] &= (unsigned char)~mbx::WN_IMG_F16;
        p.end_packed = true;
        p.lds_ok = mbx::WN_LDS_GATE_F16 | mbx::WN_LDS_GATE_F16W | mbx::WN_LDS_F43Q;
        // mbx_create: the folds, the split precision, the tuning knobs and the form, in its order
        const bool pinned = form == MBX_CONV_F23 || form == MBX_CONV_F43;
        p.fold_skip = !keep_skip && n_out <= 32 && M <= 16;
        p.fold_start = p.fold_skip && (!causal || pinned) && !keep_start && ks == 3 && mbx::wn_gate0_fits(C, pulse_channels, p.dil[0], cond_up);
        p.split_f16 = split != 0;
        p.split_f16_gate = p.split_f16 && p.fold_start && !causal && ks == 3;
        p.gate_small_shape = tune_gate_shape - 1;
        if (wave_tiles) p.resskip_wave_tiles = std::max(0, wave_tiles);
        p.resskip_split = resskip_split;
        // (every image is there: MBX_CONV_AUTO takes F(4,3) where its calibration lets it; causal padding needs a pinned form)
        const bool wino_ok = ks == 3 && (!causal || pinned);
        const int f = form == MBX_CONV_AUTO ? MBX_CONV_F43 : form;
        p.winograd = !wino_ok ? 0 : f == MBX_CONV_F43 ? 4 : f == MBX_CONV_F23 ? 2 : 0;
        p.winograd4_always = p.winograd == 4 && batch_invariant != 0;
        const bool split_ok = p.fold_skip && L >= 3 && C + n_out <= 384 && gate_act != MBX_GATE_GLU;
        mbx::WnGeometry geo;
        geo.B = B;
        geo.nsteps = (long long)frames * spf;
        geo.cond_bstride = (long long)frames * 2 * C * cond_conv_up;
        for (int l = 0; l < L; ++l) {
            geo.gate[l] = mbx::WnSpan{(int)geo.nsteps, 0, 0, 0};
            geo.res_rows[l] = (int)geo.nsteps;
        }
        const mbx::WnPlan plan = mbx::wn_plan(p, geo);
        const int status = split && !split_ok ? (int)MBX_ERR_INVALID_ARGUMENT : (int)plan.status;
        std::printf("%s | st=%d", name.c_str(), status);
        if (status == 0) {
            std::printf(" | g=");
            for (int l = 0; l < plan.n_layers; ++l) {
                const mbx::GateChoice &k = plan.gate[l];
                std::printf("%s%d/%d/%d/%d/%d", l ? " " : "", k.kernel, k.shape, k.block_channels, k.cr, k.vs_arg);
            }
        }
        std::printf("\n");
    }
    return 0;
}

// Prints the plan of every case of wn_plan_cases.h: a stand-alone host program on the planner header alone
// (tests/test_wn_plan_host.py builds and runs it, once more under the address and undefined-behaviour sanitizers).
#include "wn_plan.h"

#include "wn_plan_cases.h"

int main() {
    using namespace plan_cases;
    for (const Case &c : make_cases()) {
        mbx::WnPolicy p;
        p.winograd = c.winograd;
        p.winograd4_always = c.winograd == 4 && c.always;
        p.gate_small_shape = c.tune_gate_shape - 1;
        p.resskip_wave_tiles = c.wave_tiles;
        p.resskip_split = c.resskip_split;
        p.split_f16 = c.split >= 1;
        p.split_f16_gate = c.split >= 2;
        p.fold_skip = c.fold_skip;
        p.fold_start = c.fold_start;
        p.lds_ok = c.lds;
        p.C = c.C, p.n_out = c.n_out, p.M = c.M, p.L = c.L, p.cond_up = c.cond_up, p.ks = c.ks, p.causal = c.causal;
        p.gate_act = c.gate_act, p.pulse_channels = c.pulse_channels, p.end_packed = c.end_packed;
        mbx::WnGeometry geo;
        geo.B = c.B;
        geo.nsteps = c.rows;
        geo.cond_bstride = cond_bstride(c);
        geo.streamed = c.streamed, geo.active = c.active, geo.layer_state = c.layered != 0;
        for (int l = 0; l < c.L; ++l) {
            p.dil[l] = c.dil[l];
            p.img[l] = (unsigned char)layer_img(c, l);
            const Span s = gate_span(c, l);
            geo.gate[l] = mbx::WnSpan{s.max_rows, s.cphase, s.out0, s.out_rows};
            geo.res_rows[l] = res_rows(c, l);
        }
        const mbx::WnPlan plan = mbx::wn_plan(p, geo);
        Row r;
        r.status = plan.status;
        r.n = plan.n_layers;
        for (int l = 0; l < c.L; ++l) {
            r.gate[l] = plan.gate[l].kernel;
            r.shape[l] = plan.gate[l].shape;
            r.chan[l] = plan.gate[l].block_channels;
            r.cr[l] = plan.gate[l].cr;
            r.vs[l] = plan.gate[l].vs_arg;
            r.res[l] = plan.resskip[l];
        }
        r.tail = plan.tail, r.tail_folded = plan.tail_folded, r.planes_only = plan.planes_only;
        print_row(c, r);
    }
    return 0;
}

// The cases of tests/test_wn_plan_host.py and the text of a row: which kernel the host-side planner of
// mbexwn_vocoder_amd/csrc/wn_plan.h chooses for every WaveNet layer of a launch.  Plain C++, no project header: the
// table was also printed from a throw-away program holding the selection code of the commit before the planner, which
// is how tests/golden/wn_plan_expected.txt was made.
#pragma once
#include <cstdio>
#include <string>
#include <vector>

namespace plan_cases {

constexpr int MAX_L = 8;
// image bits as WN_IMG_* of wn_plan.h
enum { I_W4 = 1, I_W2 = 2, I_FOLD = 4, I_WIDE = 8, I_WAVE = 16, I_F16 = 32, I_PACKED = 64, I_ALL = 127 };
enum { LDS_F16 = 1, LDS_F16W = 2, LDS_Q = 4, LDS_ALL = 7 };

struct Case {
    std::string name;
    int C = 320, n_out = 30, M = 15, L = 5;
    int dil[MAX_L] = {1, 2, 4, 8, 16, 1, 1, 1};
    int cond_up = 20, ks = 3, causal = 0, gate_act = 0, pulse_channels = 6;
    int winograd = 4, always = 0, tune_gate_shape = 0, resskip_split = 0;
    long long wave_tiles = 2048;
    int split = 0;                  // 0: float32 | 1: split res/skip layers | 2: and split gates
    int fold_skip = 1, fold_start = 1, end_packed = 1;
    unsigned lds = LDS_ALL;
    unsigned img = I_ALL, img0_clear = 0;       // every layer's images; bits cleared on layer 0
    int B = 1, rows = 4800;         // items, sub-band rows per item
    int cond_conv_up = 1;
    int streamed = 0, active = 0, layered = 0;  // layered: per-layer spans of `layered` new rows (a steady streaming tick)
};

struct Span { int max_rows, cphase, out0, out_rows; };

inline Span gate_span(const Case &c, int l) {
    if (!c.layered) return Span{c.rows, 0, 0, 0};
    const int d = c.dil[l];
    if (l == 0) return Span{c.layered + 4 * d + 2 * c.cond_up, 0, 0, c.layered};
    return Span{c.layered + 6 * d + 2 * c.cond_up, (3 * l) % c.cond_up, 2 * d, c.layered};
}
inline int res_rows(const Case &c, int) { return c.layered ? c.layered : c.rows; }
inline unsigned layer_img(const Case &c, int l) { return l == 0 ? c.img & ~c.img0_clear : c.img; }
inline long long cond_bstride(const Case &c) { return (long long)(c.rows / 20 > 0 ? c.rows / 20 : 1) * 2 * c.C * c.cond_conv_up; }

struct Row {
    int status = 0, n = 0;
    int gate[MAX_L] = {}, shape[MAX_L] = {}, chan[MAX_L] = {}, cr[MAX_L] = {}, vs[MAX_L] = {}, res[MAX_L] = {};
    int tail = 0, tail_folded = 0, planes_only = 0;
};

inline void print_row(const Case &c, const Row &r) {
    std::printf("%s | st=%d", c.name.c_str(), r.status);
    if (r.status == 0) {
        std::printf(" | g=");
        for (int l = 0; l < r.n; ++l) {
            if (r.chan[l]) std::printf("%s%d/%d/%d/%d/%d", l ? " " : "", r.gate[l], r.shape[l], r.chan[l], r.cr[l], r.vs[l]);
            else std::printf("%s%d", l ? " " : "", r.gate[l]);
        }
        std::printf(" | r=");
        for (int l = 0; l < r.n; ++l) std::printf("%s%d", l ? " " : "", r.res[l]);
        std::printf(" | tail=%d/%d | po=%d", r.tail, r.tail_folded, r.planes_only);
    }
    std::printf("\n");
}

inline std::vector<Case> make_cases() {
    std::vector<Case> out;
    auto add = [&](Case c, const std::string &name) {
        c.name = name;
        out.push_back(c);
    };
    auto tag = [](const char *k, long long v) { return std::string(k) + std::to_string(v); };
    const int Cs[] = {64, 320, 340, 512}, rows[] = {600, 4800, 16000}, Bs[] = {1, 2, 8, 16};
    // channels x rows per item x batch: full_blocks = 1024, WIDE_FROM_BLOCKS = 5040 and the half_blocks 256 window are crossed
    for (int C : Cs)
        for (int r : rows)
            for (int B : Bs) {
                Case c;
                c.C = C, c.rows = r, c.B = B;
                add(c, "size-" + tag("C", C) + tag("-r", r) + tag("-B", B));
            }
    // dilations 1, 16, 64, 2048 (600 rows: sub-sequences of at most 128 rows at d = 2048, the VS == 2 blocks)
    for (int r : rows)
        for (int B : {1, 8})
            for (int t = 0; t <= 4; ++t)
                for (int always = 0; always < 2; ++always) {
                    Case c;
                    c.rows = r, c.B = B, c.tune_gate_shape = t, c.always = always;
                    const int d[] = {1, 1, 16, 64, 2048, 32, 256};
                    c.L = 7;
                    for (int l = 0; l < 7; ++l) c.dil[l] = d[l];
                    add(c, "deep" + tag("-r", r) + tag("-B", B) + tag("-tune", t) + tag("-inv", always));
                }
    // mbx_config.tune_gate_shape 0-4 and batch_invariant at every size
    for (int C : {320, 340})
        for (int r : rows)
            for (int B : {1, 2, 16})
                for (int t = 0; t <= 4; ++t)
                    for (int always = 0; always < 2; ++always) {
                        Case c;
                        c.C = C, c.rows = r, c.B = B, c.tune_gate_shape = t, c.always = always;
                        add(c, "tune" + tag("-C", C) + tag("-r", r) + tag("-B", B) + tag("-t", t) + tag("-inv", always));
                    }
    // conditioning up-sampling 4, 5, 9, 10: nothing / the CR = 56 blocks / ... / the CR = 28 and the product-split blocks
    for (int cu : {4, 5, 9, 10, 20, 64, 65})
        for (int B : {1, 16})
            for (int t : {0, 2, 3, 4})
                for (int w : {4, 2}) {
                    Case c;
                    c.cond_up = cu, c.B = B, c.tune_gate_shape = t, c.winograd = w;
                    add(c, "cond" + tag("-up", cu) + tag("-B", B) + tag("-t", t) + tag("-w", w));
                }
    // streamed calls and per-layer spans run F(2,3); without its images a per-layer span has no kernel
    for (int w : {0, 2, 4})
        for (int lay : {0, 40})
            for (unsigned img : {(unsigned)I_ALL, (unsigned)(I_ALL & ~I_W2)})
                for (int B : {1, 64}) {
                    Case c;
                    c.winograd = w, c.streamed = 1, c.active = 1, c.layered = lay, c.img = img, c.B = B, c.rows = 700;
                    add(c, "stream" + tag("-w", w) + tag("-lay", lay) + tag("-img", img) + tag("-B", B));
                }
    // causal padding (single block under a pinned Winograd form)
    for (int w : {0, 2, 4})
        for (int r : {600, 16000})
            for (int fs = 0; fs < 2; ++fs) {
                Case c;
                c.causal = 1, c.winograd = w, c.rows = r, c.fold_start = fs;
                add(c, "causal" + tag("-w", w) + tag("-r", r) + tag("-fs", fs));
            }
    // res/skip: the wave-tile bound at, below and above the launch's tile count (4800 rows = 300 tiles), the pinned cuts,
    // np = ceil((C + n_out) / 32) = 10, 11 (C below and at 320), 12, 13, missing images, batch_invariant, F(2,3)
    for (long long wt : {0LL, 299LL, 300LL, 301LL})
        for (int sp = 0; sp <= 3; ++sp) {
            Case c;
            c.wave_tiles = wt, c.resskip_split = sp;
            add(c, "wave" + tag("-tiles", wt) + tag("-split", sp));
        }
    for (int C : {288, 300, 320, 340, 384, 24, 20})
        for (int r : rows)
            for (int B : {1, 16})
                for (int w : {2, 4})
                    for (unsigned clear : {0u, (unsigned)I_WIDE, (unsigned)I_WAVE, (unsigned)(I_WIDE | I_WAVE)}) {
                        Case c;
                        c.C = C, c.rows = r, c.B = B, c.winograd = w, c.img = I_ALL & ~clear;
                        add(c, "np" + tag("-C", C) + tag("-r", r) + tag("-B", B) + tag("-w", w) + tag("-noimg", clear));
                    }
    for (int r : rows)
        for (int B : {1, 16}) {
            Case c;
            c.rows = r, c.B = B, c.always = 1;
            add(c, "resinv" + tag("-r", r) + tag("-B", B));
        }
    // the un-folded graph: packed or generic res/skip layers, the tail on the skip tensor or two convolutions
    for (int C : {64, 320})
        for (int r : {600, 16000})
            for (int B : {1, 16})
                for (unsigned img : {(unsigned)I_ALL, (unsigned)(I_W4 | I_W2), 0u})
                    for (int nout : {30, 60}) {
                        Case c;
                        c.C = C, c.rows = r, c.B = B, c.img = img, c.n_out = nout, c.fold_skip = 0, c.fold_start = 0, c.end_packed = img == (unsigned)I_ALL;
                        add(c, "unfolded" + tag("-C", C) + tag("-r", r) + tag("-B", B) + tag("-img", img) + tag("-nout", nout));
                    }
    for (int C : {8, 16, 64, 128, 192, 320, 352, 356}) {
        Case c;
        c.C = C;
        add(c, "tail" + tag("-C", C));
    }
    // an odd column-tile count under the blocks of two column tiles (C = 340: 11 tiles), and too few tiles for them
    for (int C : {32, 64, 96, 340, 352})
        for (unsigned lds : {(unsigned)LDS_ALL, (unsigned)(LDS_ALL & ~LDS_Q)}) {
            Case c;
            c.C = C, c.tune_gate_shape = 4, c.lds = lds;
            add(c, "twotile" + tag("-C", C) + tag("-lds", lds));
        }
    // split half precision: gates with and without planes in front, every LDS opt-in bit cleared, cond_up = 9, glu
    for (int split : {1, 2})
        for (int r : {600, 16000})
            for (int B : {1, 16})
                for (unsigned clear0 : {0u, (unsigned)I_F16})
                    for (unsigned lds : {(unsigned)LDS_ALL, (unsigned)(LDS_ALL & ~LDS_F16), (unsigned)(LDS_ALL & ~LDS_F16W), (unsigned)(LDS_ALL & ~LDS_Q)})
                        for (int cu : {9, 20}) {
                            Case c;
                            c.split = split, c.rows = r, c.B = B, c.img0_clear = clear0, c.lds = lds, c.cond_up = cu;
                            add(c, "split" + tag("-s", split) + tag("-r", r) + tag("-B", B) + tag("-no0", clear0) + tag("-lds", lds) + tag("-up", cu));
                        }
    for (int active = 0; active < 2; ++active)
        for (int deep = 0; deep < 2; ++deep) {
            Case c;
            c.split = 2, c.active = active;
            if (deep) c.dil[3] = 32;
            add(c, "splitx" + tag("-active", active) + tag("-deep", deep));
        }
    return out;
}

}  // namespace plan_cases

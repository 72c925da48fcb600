"""The WaveNet kernels stage by stage against the float64 oracle at float32-rounding tolerance (tests/wn_reference.py).

Every case runs a ragged batch through the engine, asserts which gate, residual/skip and tail kernels ran
(mbx_conv_form_info.gate_kernel, mbx_kernel_report) and holds
"wn_out", "wn_hidden" and (with keep_skip) "wn_skip" to the oracle's WaveNet fed the engine's own excitation rows, over every
item's valid rows, at tol = max(K * float32-port error, F * max(1, |ref|)).  The lengths straddle the 128- and 256-row tiles
(20 rows per frame) and an item of one frame is shorter than every dilation >= 32; the ragged order puts short items next
to long ones, so that one item leaking into its neighbour shows.  The end-to-end tests hold the audio to 1e-4: a lost low
half of one channel tile, a row off at a tile seam or a leak between items passes that bar (test_wn_reference.py) and not
this one.  A failure names the worst item, row and channel and the row's place in its 256- and 128-row tiles.

The res/skip convolution runs one of eleven kernel instantiations (or conv1d) and the tail one of six (or two generic
convolutions); which one follows from C + n_out, C, the launch size and the policy (resskip_shape_policy and the launchers).
The 3-layer geometries "c<C>" put every instantiation at the channel counts where its tiles are ragged: C + 30 one column
pair past a multiple of 32 (C = 292, 324: the last pair holds two valid columns), the residual/skip seam inside a pair
(C = 324, 340) and on a pair boundary (C = 352), a last 16-channel block of 4 channels in the tail (C = 68, 132, 196, 324), the
first C behind the wave, wide and wn_tail2 kernels (C = 356) and five 128-column tiles (C = 512).

The split-half-precision path (precision="split_f16": wn_gate_f16.hip, wn_resskip_f16.hip) is a second implementation of both
contractions with three gate kernels (the planes kernel, the large-launch kernel over pairs of column tiles, the kernel that
splits a float32 hidden state itself) and a res/skip kernel; the "*-split" cases put each at the channel counts where ITS tiles
are ragged (C % 32 != 0 under an odd tile count, C % 8 == 4: plane padding, C + 30 = 382, C <= 162), on the model variants, in
the mixed mode under float32 gates, and hold it to the same bar; what the mode's arithmetic alone costs is in
test_split_reference.py.

The F(4,3) blocks of two column tiles (wn_gate_winograd4q_kernel, the gate of the large launches) promise the bits of the
one-tile blocks.  The "*-two-tile" cases pin them on the ragged batch (tune gate_shape 4 holds at every launch size) at the
channel counts where THEIR tiles are ragged (TWO_TILE_C: a partial tile inside a pair, one pair only, an odd last tile in the
one-tile kernel, the shortest K loop, both parities of the stage the conditioning rows land in) and on the model variants,
hold them to the oracle, and compare their stages bit for bit with a run pinned to the one-tile blocks.  Which instantiation
of the F(4,3) kernels a case launches follows from its plan row (kernel, block shape, conditioning rows, sub-sequences per
block) and the gate activation; test_wn_stage_plan_host.py derives it on the host for every case here and holds the union to
the launcher's list, and every case asserts that the plan is what ran.

The padding contract of include/mbexwn.h ("every boundary op honours the item's own length") is held bit for bit: the same
ragged batch with its padding frames of mel and noise at 0, 1e30 and NaN."""
import contextlib
import json

import numpy as np
import pytest

from helpers import build_case, synthetic_inputs
from wn_reference import WaveNetReference, assert_matches, engine_stages, oracle_models, summary, wavenet_inputs

# ragged lengths in frames: 20 - 1040 rows around the 128- / 256-row tiles, short next to long
RAGGED = [26, 1, 52, 7, 13, 51, 6, 25, 12]
# the 12-layer model (dilations 1 .. 2048): items shorter and longer than the deepest layers reach (110 frames = 2200 rows)
DEEP = [13, 110, 1, 52, 7]
# one launch of 16 items of 400 - 700 frames: the large-launch kernel shapes (256-row F(4,3), wn_resskip_wide, wn_gate_f16w);
# the oracle checks the longest, the shortest and one in the middle
LARGE = [560, 400, 700, 420, 640, 460, 520, 680, 440, 600, 480, 620, 500, 660, 540, 580]
LARGE_CHECK = [LARGE.index(max(LARGE)), LARGE.index(min(LARGE)), LARGE.index(560)]
# C = 512, one launch of 77 row tiles x 6 items x 5 column tiles = 2 310 128-row blocks: the packed res/skip kernel's 128-row
# shape starts at 2 304
LARGE6 = [490, 3, 260, 77, 411, 128]
LARGE6_CHECK = [LARGE6.index(max(LARGE6)), LARGE6.index(min(LARGE6)), LARGE6.index(260)]
# C = 68 under the large-launch split gate kernel (wn_gate_f16w_kernel: 4 x 256 blocks of 256 rows x a PAIR of column tiles): 3
# column tiles = 2 pairs, so 512 row tiles: 8 items x 65 (the oracle at C = 68 is cheap: three items, about a second)
LARGE8 = [820, 3, 411, 77, 640, 128, 260, 700]
LARGE8_CHECK = [0, 1, 2]
# the shortest set that takes wn_gate_f16w_kernel at C = 340 (6 pairs): 8 items x 22 row tiles = 176 -> 1056 blocks >= 1024
WIDE8 = [280, 1, 52, 7, 13, 201, 6, 25]
LENGTHS = {"ragged": (RAGGED, None), "deep": (DEEP, None), "large": (LARGE, LARGE_CHECK), "large6": (LARGE6, LARGE6_CHECK),
           "large8": (LARGE8, LARGE8_CHECK)}


def split_gate_blocks(C, lengths, wide=True):
    """Blocks of a split gate launch as launch_wn_gate_f16 counts them (row tiles of 256 rows rounded up to the 8 XCDs x column
    tiles, or pairs of them): the wide kernel runs from 4 * 256 pair blocks."""
    tiles = ((max(lengths) * 20 + 255) // 256) * len(lengths)
    nt = (C + 31) // 32
    return 8 * ((tiles + 7) // 8) * ((nt + 1) // 2 if wide else nt)

_WN = "mbexwn_config:pp_mod_subnet:"
GEOMETRIES = {
    "speech": ("SPEECH", {}),                                                   # C = 320, 5 layers, d <= 16
    "voice": ("VOICE", {}),                                                     # C = 340: a partial 32-channel tile
    "deep12": ("SPEECH", {_WN + "n_layers": 12}),                               # d <= 2048: strided F(4,3), direct fall-back
    "c36": ("SPEECH", {_WN + "n_channels": 36, _WN + "n_layers": 3}),
    "c12": ("SPEECH", {_WN + "n_channels": 12, _WN + "n_layers": 3}),           # too narrow for the Winograd kernels; wn_tail_kernel
    "l3": ("SPEECH", {_WN + "n_layers": 3}),
    "lin5": ("SPEECH", {_WN + "cond_lin_upsampling": 5}),                       # layer 0 not folded (conditioning rows)
    "lin20": ("SPEECH", {_WN + "cond_lin_upsampling": 20}),
    "gfu": ("SPEECH", {_WN + "activation": "gfu"}),
    "gsu": ("SPEECH", {_WN + "activation": "gsu"}),
    "glu": ("SPEECH", {_WN + "activation": "glu"}),
    "groups2": ("SPEECH", {_WN + "n_ch_groups": 2}),
    "causal": ("SPEECH", {_WN + "padding": "CAUSAL"}),
    # the channel counts of the res/skip and tail instantiations, 3 layers each
    **{f"c{C}": ("SPEECH", {_WN + "n_channels": C, _WN + "n_layers": 3})
       for C in (64, 68, 128, 132, 192, 196, 292, 300, 316, 324, 340, 352, 356, 512)},
    # gfu at C = 64 (the oracle is about 25 times cheaper than at C = 320): cond_up = 5 takes the 256-row blocks of 56
    # conditioning rows; nine layers reach d = 256, whose 16 sub-sequences of a 52-frame item have 65 rows
    "lin5-c64-gfu": ("SPEECH", {_WN + "n_channels": 64, _WN + "n_layers": 3, _WN + "cond_lin_upsampling": 5, _WN + "activation": "gfu"}),
    "deep9-c64-gfu": ("SPEECH", {_WN + "n_channels": 64, _WN + "n_layers": 9, _WN + "activation": "gfu"}),
}

F43 = {"conv_form": "f43"}
INVARIANT = {"conv_form": "f43", "batch_invariant": True}
FS, PS, HS = "folded_start", "f43_psplit", "f43_hsplit"
SP, SPW, SPF = "split_f16", "split_f16_wide", "split_f16_f32h"
SPLIT = dict(F43, precision="split_f16")
# the F(4,3) blocks of two column tiles (wn_gate_winograd4q_kernel), pinned: gate_shape_policy honours the pin at every launch
# size for d <= 16
TWO = dict(F43, tune={"gate_shape": 4})
# channel counts of the 3-layer two-tile cases: {C: column tiles}.  36: one pair, its second tile holds 4 channels, nk8 = 5
# with a partial last slice; 64: one full pair, nk8 even; 68: one pair, then an odd partial tile in the one-tile kernel,
# nk8 = 9; 132: two pairs, then an odd partial tile; 292: a partial tile (4 channels) inside the last pair, nk8 = 37; 324: an
# odd partial tile; 352: an odd full tile, nk8 = 44; 356: a partial tile inside the last pair, nk8 = 45
TWO_TILE_C = {36: 2, 64: 2, 68: 3, 132: 5, 292: 10, 324: 11, 352: 11, 356: 12}
TWO_TILE_VARIANTS = ("speech", "voice", "gfu", "gsu", "glu", "groups2", "lin20", "causal")


def _split(ss):
    return dict(F43, tune={"resskip_split": ss})


# (id, geometry, lengths, engine arguments, the gate kernels the forward must run)
CASES = [
    # the forms on SPEECH (9 items, 1040 rows: 450 256-row blocks -> the product-split shape under the default policy)
    ("speech-direct", "speech", "ragged", {"conv_form": "direct"}, {FS, "direct"}),
    ("speech-f23", "speech", "ragged", {"conv_form": "f23"}, {FS, "f23"}),
    ("speech-f43", "speech", "ragged", F43, {FS, PS}),
    ("speech-f43-invariant", "speech", "ragged", {"conv_form": "f43", "batch_invariant": True}, {FS, "f43"}),
    ("speech-auto", "speech", "ragged", {"conv_form": "auto"}, {FS, PS}),
    # the F(4,3) block shapes pinned (tune_gate_shape 1 | 2 | 3: 256-row, product-split, product-split half column tiles)
    ("speech-f43-256row", "speech", "ragged", dict(F43, tune={"gate_shape": 1}), {FS, "f43"}),
    ("speech-f43-psplit", "speech", "ragged", dict(F43, tune={"gate_shape": 2}), {FS, PS}),
    ("speech-f43-hsplit", "speech", "ragged", dict(F43, tune={"gate_shape": 3}), {FS, "f43_hsplit"}),
    # the res/skip variants: the wave-tiled kernel's three column splits, and the plain kernel (wave tiles off)
    ("speech-rs-split1", "speech", "ragged", dict(F43, tune={"resskip_split": 1}), {FS, PS}),
    ("speech-rs-split2", "speech", "ragged", dict(F43, tune={"resskip_split": 2}), {FS, PS}),
    ("speech-rs-split3", "speech", "ragged", dict(F43, tune={"resskip_split": 3}), {FS, PS}),
    ("speech-rs-nowave", "speech", "ragged", dict(F43, tune={"resskip_wave_tiles": -1}), {FS, PS}),
    # geometries
    ("voice-f43", "voice", "ragged", F43, {FS, PS}),
    ("voice-f43-256row", "voice", "ragged", dict(F43, tune={"gate_shape": 1}), {FS, "f43"}),
    ("deep12-f43", "deep12", "deep", F43, {FS, PS, "f43_strided_psplit", "direct"}),
    # batch_invariant keeps F(4,3) at every dilation (no direct fall-back); the strided block shape still follows the cost
    # rule (both shapes give the same bits)
    ("deep12-f43-invariant", "deep12", "deep", {"conv_form": "f43", "batch_invariant": True},
     {FS, "f43", "f43_strided", "f43_strided_psplit"}),
    ("c36-f43", "c36", "ragged", F43, {FS, "f43_hsplit"}),
    ("c12-f43", "c12", "ragged", F43, {FS, "direct"}),
    ("lin5-f43", "lin5", "ragged", F43, {"f43"}),
    ("lin20-f43", "lin20", "ragged", F43, {FS, PS}),
    ("gfu-f43", "gfu", "ragged", F43, {FS, PS}),
    ("gsu-f43", "gsu", "ragged", F43, {FS, PS}),
    ("glu-f43", "glu", "ragged", F43, {FS, PS}),
    ("groups2-f43", "groups2", "ragged", F43, {FS, PS}),
    ("causal-auto", "causal", "ragged", {"conv_form": "auto"}, {"direct"}),
    ("speech-keep-skip", "speech", "ragged", dict(F43, keep_skip=True), {PS}),
    ("speech-keep-start", "speech", "ragged", dict(F43, keep_start=True), {PS}),
    # split half precision, held to the same bar; SPEECH and the 3-layer model take the plane-only hidden state, the 12-layer
    # model does not (dilations above 16 run the float32 gate kernels)
    ("speech-split", "speech", "ragged", dict(F43, precision="split_f16"), {FS, "split_f16"}),
    ("l3-split", "l3", "ragged", dict(F43, precision="split_f16"), {FS, "split_f16"}),
    ("deep12-split", "deep12", "deep", dict(F43, precision="split_f16"), {FS, "split_f16", "f43_strided_psplit", "direct"}),
    # large launches
    ("large-f43", "speech", "large", F43, {FS, "f43"}),
    ("large-split", "speech", "large", dict(F43, precision="split_f16"), {FS, SPW}),
    # ---- split half precision at every channel edge (3 layers) and model variant; small launches: the planes kernel ----
    # C % 32 != 0 (a partial last column tile and K step), C % 8 == 4 (plane padding), C + 30 = 382 (the largest res/skip
    # launch), C <= 162 (the second column-half block of the res/skip kernel stores little or nothing)
    *[(f"c{C}-split", f"c{C}", "ragged", SPLIT, {FS, SP}) for C in (340, 324, 292, 352, 68, 132, 36)],
    ("voice-split", "voice", "ragged", SPLIT, {FS, SP}),
    ("gfu-split", "gfu", "ragged", SPLIT, {FS, SP}),
    ("gsu-split", "gsu", "ragged", SPLIT, {FS, SP}),
    ("groups2-split", "groups2", "ragged", SPLIT, {FS, SP}),
    ("lin20-split", "lin20", "ragged", SPLIT, {FS, SP}),
    # a tensor table without wn.res_skip_0.fold_start_f16: layer 0's res/skip runs in float32 and leaves no planes, layer 1's
    # gate splits the float32 hidden state itself (wn_gate_f16_kernel<false>)
    ("speech-split-f32h", "speech", "ragged", SPLIT, {FS, SPF, SP}),
    # mixed mode: split res/skip layers under float32 gates, no planes.  A kept start convolution leaves layer 0's res/skip to
    # the float32 policy (L - 2 split layers); causal padding under a pinned form folds the start, so layer 0 takes its split
    # image as well (L - 1), and only the gates stay float32
    ("speech-keep-start-split", "speech", "ragged", dict(SPLIT, keep_start=True), {PS}),
    ("causal-f43-split", "causal", "ragged", SPLIT, {FS, PS}),
    # large launches: wn_gate_f16w_kernel with an odd number of column tiles (the last pair's second tile does not exist)
    ("large6-c340-split", "c340", "large6", SPLIT, {FS, SPW}),
    ("large6-c324-split", "c324", "large6", SPLIT, {FS, SPW}),
    ("large6-speech-split", "speech", "large6", SPLIT, {FS, SPW}),
    ("large8-c68-split", "c68", "large8", SPLIT, {FS, SPW}),
    # ---- the res/skip and tail instantiations (3 layers) ----
    # wide kernel (batch_invariant): 11 pairs with C < 320 -> <11,1,0>; 12 pairs -> <6,2,0>
    *[(f"c{C}-invariant", f"c{C}", "ragged", INVARIANT, {FS, "f43"}) for C in (292, 300, 316, 324, 340, 352)],
    # wave kernel, its column split pinned: 12 pairs -> <12,3>, <6,4>, <4,4>; 11 pairs cut unevenly (6 + 5, 4 + 4 + 3)
    *[(f"c{C}-rs-split{ss}", f"c{C}", "ragged", _split(ss), {FS, PS}) for C in (340, 324) for ss in (1, 2, 3)],
    *[(f"c300-rs-split{ss}", "c300", "ragged", _split(ss), {FS, PS}) for ss in (2, 3)],
    # packed kernel, 64-row shape: one, two, four and five 128-column tiles
    ("c64-f43", "c64", "ragged", F43, {FS, HS}),
    ("c128-f43", "c128", "ragged", F43, {FS, PS}),
    ("c356-f43", "c356", "ragged", F43, {FS, PS}),
    ("c512-f43", "c512", "ragged", F43, {FS, PS}),
    # ... and its 128-row shape
    ("large6-c512-f43", "c512", "large6", F43, {FS, "f43"}),
    # tail: a last 16-channel block of 4 channels under NJ = 8, 12 and 20, and NJ = 12 filled
    ("c68-f43", "c68", "ragged", F43, {FS, HS}),
    ("c132-f43", "c132", "ragged", F43, {FS, PS}),
    ("c192-f43", "c192", "ragged", F43, {FS, PS}),
    ("c196-f43", "c196", "ragged", F43, {FS, PS}),
    # ---- the blocks of two column tiles at the stages: channel edges (3 layers) and model variants ----
    *[(f"c{C}-two-tile", f"c{C}", "ragged", TWO, {FS, "f43"}) for C in TWO_TILE_C],
    # causal padding under a pinned form folds the start convolution; the gate layers pad 2 d (sh = d in the kernel)
    *[(f"{gg}-two-tile", gg, "ragged", TWO, {FS, "f43"}) for gg in TWO_TILE_VARIANTS],
    # a kept start convolution: layer 0 runs the gate kernel at d = 1
    ("speech-keep-start-two-tile", "speech", "ragged", dict(TWO, keep_start=True), {"f43"}),
    # cond_up = 5 needs 53 conditioning rows, the two-tile blocks hold 28: wn_gate_winograd4w_select refuses the shape and the
    # plan falls back to the one-tile 256-row blocks with CR = 56 (layer 0 is not folded: wn_gate0 holds 32 rows)
    ("lin5-two-tile-refused", "lin5", "ragged", TWO, {"f43"}),
    # ---- the <-1> instantiations (gfu, gsu, glu) of the other F(4,3) kernels ----
    ("gfu-f43-256row", "gfu", "ragged", dict(F43, tune={"gate_shape": 1}), {FS, "f43"}),            # 4w<28,-1>
    ("gfu-f43-hsplit", "gfu", "ragged", dict(F43, tune={"gate_shape": 3}), {FS, HS}),               # 4h<-1>
    ("lin5-c64-gfu-f43", "lin5-c64-gfu", "ragged", F43, {"f43"}),                                   # 4w<56,-1>
    # d = 32, 64: 4p<-1,1> under both policies; d = 128, 256: the direct form under the default policy (F(4,3) costs 144
    # block units against 0.9 x 146.25) and, batch_invariant, 4w<28,-1,1> (130 rows per sub-sequence) and 4w<28,-1,2> (65)
    ("deep9-c64-gfu-f43", "deep9-c64-gfu", "ragged", F43, {FS, HS, "f43_strided_psplit", "direct"}),
    ("deep9-c64-gfu-invariant", "deep9-c64-gfu", "ragged", INVARIANT, {FS, "f43", "f43_strided_psplit", "f43_strided"}),
]
# the cases that run the blocks of two column tiles: each is run once more pinned to the one-tile 256-row blocks, for the bits
TWO_TILE = [f"c{C}-two-tile" for C in TWO_TILE_C] + [f"{gg}-two-tile" for gg in TWO_TILE_VARIANTS] + ["speech-keep-start-two-tile"]
PLANES_ONLY = {"speech-split", "l3-split", "large-split", "voice-split", "gfu-split", "gsu-split", "groups2-split", "lin20-split",
               "large6-c340-split", "large6-c324-split", "large6-speech-split", "large8-c68-split",
               *(f"c{C}-split" for C in (340, 324, 292, 352, 68, 132, 36))}
# the cases built from a tensor table without layer 0's split res/skip image
NO_START_F16 = {"speech-split-f32h"}
# split res/skip layers whose layer 0 runs a float32 kernel: {case id: that kernel}; split_f16_layers is L - 2 there, L - 1 elsewhere
F32_LAYER0 = {"speech-split-f32h": "wave4x3", "speech-keep-start-split": "wave4x3"}

# {case id: (the res/skip kernels its forward must run, its tail kernel)} (engine.RESSKIP_KERNEL_NAMES / TAIL_KERNEL_NAMES).  A
# model with the skip path folded launches L - 1 res/skip layers; the tail kernel takes the last layer's share.
W43, P64 = "wave4x3", "packed64"
NJ4, NJ8, NJ12, NJ20, NJ22 = "tail2_nj4", "tail2_nj8", "tail2_nj12", "tail2_nj20", "tail2_nj22"
KERNELS = {
    # SPEECH, 9 ragged items: 585 wave tiles, the fill score picks three column splits; a pinned direct form and the wave
    # tiles switched off leave the packed kernel; batch_invariant and large launches take the wide one
    "speech-direct": ({P64}, NJ20), "speech-f23": ({W43}, NJ20), "speech-f43": ({W43}, NJ20),
    "speech-f43-invariant": ({"wide11_res10"}, NJ20), "speech-auto": ({W43}, NJ20),
    "speech-f43-256row": ({W43}, NJ20), "speech-f43-psplit": ({W43}, NJ20), "speech-f43-hsplit": ({W43}, NJ20),
    "speech-rs-split1": ({"wave11"}, NJ20), "speech-rs-split2": ({"wave6x2"}, NJ20), "speech-rs-split3": ({W43}, NJ20),
    "speech-rs-nowave": ({P64}, NJ20),
    "voice-f43": ({W43}, NJ22), "voice-f43-256row": ({W43}, NJ22),
    # 5 items of up to 2 200 rows: 690 wave tiles, all columns per wave
    "deep12-f43": ({"wave11"}, NJ20), "deep12-f43-invariant": ({"wide11_res10"}, NJ20),
    "c36-f43": ({P64}, NJ4), "c12-f43": ({P64}, "tail"),
    "lin5-f43": ({W43}, NJ20), "lin20-f43": ({W43}, NJ20), "gfu-f43": ({W43}, NJ20), "gsu-f43": ({W43}, NJ20),
    "glu-f43": ({W43}, NJ20), "groups2-f43": ({W43}, NJ20), "causal-auto": ({P64}, NJ20),
    "speech-keep-skip": ({P64}, NJ20), "speech-keep-start": ({W43}, NJ20),
    "speech-split": ({"split_f16"}, NJ20), "l3-split": ({"split_f16"}, NJ20), "deep12-split": ({"split_f16"}, NJ20),
    "large-f43": ({"wide11_res10"}, NJ20), "large-split": ({"split_f16"}, NJ20),
    "c340-split": ({SP}, NJ22), "c324-split": ({SP}, NJ22), "c292-split": ({SP}, NJ20), "c352-split": ({SP}, NJ22),
    "c68-split": ({SP}, NJ8), "c132-split": ({SP}, NJ12), "c36-split": ({SP}, NJ4), "voice-split": ({SP}, NJ22),
    "gfu-split": ({SP}, NJ20), "gsu-split": ({SP}, NJ20), "groups2-split": ({SP}, NJ20), "lin20-split": ({SP}, NJ20),
    "speech-split-f32h": ({W43, SP}, NJ20), "speech-keep-start-split": ({W43, SP}, NJ20), "causal-f43-split": ({SP}, NJ20),
    "large6-c340-split": ({SP}, NJ22), "large6-c324-split": ({SP}, NJ22), "large6-speech-split": ({SP}, NJ20),
    "large8-c68-split": ({SP}, NJ8),
    "c292-invariant": ({"wide11"}, NJ20), "c300-invariant": ({"wide11"}, NJ20), "c316-invariant": ({"wide11"}, NJ20),
    "c324-invariant": ({"wide6x2"}, NJ22), "c340-invariant": ({"wide6x2"}, NJ22), "c352-invariant": ({"wide6x2"}, NJ22),
    "c340-rs-split1": ({"wave12"}, NJ22), "c340-rs-split2": ({"wave6x2"}, NJ22), "c340-rs-split3": ({W43}, NJ22),
    "c324-rs-split1": ({"wave12"}, NJ22), "c324-rs-split2": ({"wave6x2"}, NJ22), "c324-rs-split3": ({W43}, NJ22),
    "c300-rs-split2": ({"wave6x2"}, NJ20), "c300-rs-split3": ({W43}, NJ20),
    "c64-f43": ({P64}, NJ4), "c128-f43": ({P64}, NJ8), "c356-f43": ({P64}, "tail"), "c512-f43": ({P64}, "tail"),
    "large6-c512-f43": ({"packed128"}, "tail"),
    "c68-f43": ({P64}, NJ8), "c132-f43": ({P64}, NJ12), "c192-f43": ({P64}, NJ12), "c196-f43": ({P64}, NJ20),
    # the gate's block shape does not enter the res/skip and tail selection: np = ceil((C + 30) / 32) of 11 or 12 takes the
    # wave-tiled kernel (585 tiles: three column splits), every other one the packed kernel; nj = ceil(8 ceil(C / 8) / 16)
    "c36-two-tile": ({P64}, NJ4), "c64-two-tile": ({P64}, NJ4), "c68-two-tile": ({P64}, NJ8), "c132-two-tile": ({P64}, NJ12),
    "c292-two-tile": ({W43}, NJ20), "c324-two-tile": ({W43}, NJ22), "c352-two-tile": ({W43}, NJ22), "c356-two-tile": ({P64}, "tail"),
    "speech-two-tile": ({W43}, NJ20), "voice-two-tile": ({W43}, NJ22), "gfu-two-tile": ({W43}, NJ20), "gsu-two-tile": ({W43}, NJ20),
    "glu-two-tile": ({W43}, NJ20), "groups2-two-tile": ({W43}, NJ20), "lin20-two-tile": ({W43}, NJ20), "causal-two-tile": ({W43}, NJ20),
    "speech-keep-start-two-tile": ({W43}, NJ20), "lin5-two-tile-refused": ({W43}, NJ20),
    "gfu-f43-256row": ({W43}, NJ20), "gfu-f43-hsplit": ({W43}, NJ20), "lin5-c64-gfu-f43": ({P64}, NJ4),
    "deep9-c64-gfu-f43": ({P64}, NJ4), "deep9-c64-gfu-invariant": ({P64}, NJ4),
}
# {case id: gate channels per F(4,3) block and layer} (kernel_report()["gate_block_channels"]; wn_gate_winograd4w_select: 64 two
# column tiles, 32 one, 16 half a tile, 0 no F(4,3) block: the folded layer 0, the direct form)
BLOCK_CHANNELS = {
    "large-f43": [0, 64, 64, 64, 64],          # 55 row tiles x 16 items x 10 column tiles = 8 800 blocks >= WIDE_FROM_BLOCKS
    **{f"c{C}-two-tile": [0, 64, 64] for C in TWO_TILE_C},
    **{f"{gg}-two-tile": [0, 64, 64, 64, 64] for gg in TWO_TILE_VARIANTS},
    "speech-keep-start-two-tile": [64] * 5, "lin5-two-tile-refused": [32] * 5,
    "gfu-f43-256row": [0, 32, 32, 32, 32], "gfu-f43-hsplit": [0, 16, 16, 16, 16], "lin5-c64-gfu-f43": [32, 32, 32],
    "deep9-c64-gfu-f43": [0, 16, 16, 16, 16, 32, 32, 0, 0], "deep9-c64-gfu-invariant": [0] + [32] * 8,
}
# the cases whose skip path is not folded (a skip tensor is kept): every layer launches a res/skip convolution, the tail reads
# the skip tensor
UNFOLDED = {"speech-keep-skip"}
_REFS = {}


@contextlib.contextmanager
def tensor_table_of(cid):
    """The tensor table a case's engine is created from: for the cases of NO_START_F16 the host leaves out layer 0's split
    res/skip image (a legal table: the C ABI runs that layer in float32), for every other case the engine's own."""
    from mbexwn_vocoder_amd import packing as packing_module
    fold_start = packing_module.fold_start_weights

    def without_the_split_image(*args, **kw):
        out = fold_start(*args, **kw)
        assert out.pop("wn.res_skip_0.fold_start_f16", None) is not None
        return out

    if cid in NO_START_F16:
        packing_module.fold_start_weights = without_the_split_image
    try:
        yield
    finally:
        packing_module.fold_start_weights = fold_start


def test_gpu_cases_cover_every_gate_kernel():
    """(CPU) Every gate kernel the library reports is expected by at least one stage case: a new kernel without a case here
    fails the suite."""
    from mbexwn_vocoder_amd.engine import GATE_KERNEL_NAMES
    declared = set().union(*(case[4] for case in CASES))
    assert declared <= set(GATE_KERNEL_NAMES.values())
    assert declared == set(GATE_KERNEL_NAMES.values()) - {"none"}
    assert len({case[0] for case in CASES}) == len(CASES)
    for case in CASES:
        assert case[1] in GEOMETRIES and case[2] in LENGTHS


def test_gpu_cases_cover_every_resskip_and_tail_kernel():
    """(CPU) Every res/skip and tail kernel the library reports is expected by a stage case here, but for the two generic
    fall-backs, which the cases without weight images (test_gpu_wavenet_blocks.py: conv1d) and with 60 output channels
    (test_gpu_backend_stages.py: the unfused tail) expect: a new instantiation without a case fails the suite."""
    import test_gpu_backend_stages as tbe
    import test_gpu_wavenet_blocks as tblk
    from mbexwn_vocoder_amd.engine import RESSKIP_KERNEL_NAMES, TAIL_KERNEL_NAMES
    assert set(KERNELS) == {case[0] for case in CASES}
    resskip = set().union(*(kk[0] for kk in KERNELS.values()))
    tails = {kk[1] for kk in KERNELS.values()}
    assert any(case[3] == tblk.NOIMG for case in tblk.CASES) and tblk.NOIMG_RESSKIP == {"conv1d"}
    assert tbe.TAIL_KERNELS["bands30_out60"] == "unfused" and any(case[1] == "bands30_out60" for case in tbe.CASES)
    assert resskip | tblk.NOIMG_RESSKIP == set(RESSKIP_KERNEL_NAMES.values()) - {"none"}
    assert tails | {tbe.TAIL_KERNELS["bands30_out60"]} == set(TAIL_KERNEL_NAMES.values()) - {"none"}
    assert UNFOLDED <= set(KERNELS)
    # the edges the channel counts are there for
    chans = {int(case[1][1:]): case[0] for case in CASES if case[1][1:].isdigit()}
    assert {C for C in chans if (C + 30) % 32 == 2} >= {292, 324} and {C for C in chans if C % 16 == 4} >= {68, 132, 196, 324}
    lengths, items = LENGTHS["large6"]
    # launch_wn_resskip: 128-row blocks from three rounds of 768 resident blocks up (row tiles x items x 128-column tiles)
    assert ((max(lengths) * 20 + 127) // 128) * len(lengths) * ((512 + 30 + 127) // 128) >= 3 * 768
    assert sorted(lengths[ii] for ii in items) == [min(lengths), 260, max(lengths)]


def test_gpu_split_cases_cover_the_channel_edges_and_launch_sizes():
    """(CPU) The split-precision cases stand at the channel counts where wn_gate_f16.hip and wn_resskip_f16.hip take another
    branch, and the launch arithmetic of launch_wn_gate_f16 puts each case on the kernel it expects."""
    split = {case[0]: case for case in CASES if case[3].get("precision") == "split_f16"}
    chan = {"speech": 320, "l3": 320, "deep12": 320, "voice": 340, "gfu": 320, "gsu": 320, "groups2": 320, "lin20": 320, "causal": 320}
    chan.update({gg: int(gg[1:]) for gg in GEOMETRIES if gg[1:].isdigit()})
    small = {chan[case[1]] for case in split.values() if SP in case[4] and SPW not in case[4]}
    wide = {chan[case[1]] for case in split.values() if SPW in case[4]}
    # a partial last column tile under an odd tile count, in the wide kernel: its last pair has one tile only
    assert {C for C in wide if C % 32 and ((C + 31) // 32) % 2} >= {340, 324, 68}
    assert {C for C in small if C % 32} >= {340, 324, 292, 68, 132, 36}
    # plane padding between C and ceil8(C), read by the next gate as 8-channel chunks
    assert {C for C in small if C % 8 == 4} >= {292, 324, 340, 68, 132, 36} and {C for C in wide if C % 8 == 4} >= {340, 324, 68}
    # the widest res/skip launch the kernel accepts (C + 30 = 382: the clamp of the last column pair), two valid columns in it
    assert {C for C in small if C + 30 == 382} == {352} and {C for C in small if (C + 30) % 32 == 2} >= {292, 324}
    # the second column-half block (pairs 6 .. 11) lies behind cout: nothing, or plane padding only, to store
    assert {C for C in small | wide if C <= 162} >= {36, 68, 132}
    # cond_up: 10 sits exactly at the gate kernels' 28 conditioning rows; 20 is the other value a model can have
    assert "lin20-split" in split and GEOMETRIES["lin20"][1][_WN + "cond_lin_upsampling"] == 20
    # launch_wn_gate_f16: the wide kernel from 4 * 256 blocks of column-tile PAIRS, the planes kernel below
    for cid, case in split.items():
        lengths = LENGTHS[case[2]][0]
        if SPW in case[4]:
            assert SP not in case[4] and split_gate_blocks(chan[case[1]], lengths) >= 4 * 256, cid
        elif SP in case[4]:
            assert split_gate_blocks(chan[case[1]], lengths) < 4 * 256, cid
    assert split_gate_blocks(340, LARGE6) == 1440 and split_gate_blocks(324, LARGE6) == 1440 and split_gate_blocks(320, LARGE6) == 1200
    assert split_gate_blocks(68, LARGE8) == 1040
    assert split_gate_blocks(340, WIDE8) == 1056 and split_gate_blocks(340, [ll if ll != max(WIDE8) else ll - 26 for ll in WIDE8]) < 1024
    assert split_gate_blocks(340, RAGGED) < 1024
    # every split case that leaves planes is a plane-only one unless a layer is out of the split gate's reach; the mixed mode has none
    assert PLANES_ONLY <= set(split) and NO_START_F16 <= set(split) and set(F32_LAYER0) <= set(split)
    assert not PLANES_ONLY & (set(F32_LAYER0) | {"causal-f43-split", "deep12-split"})


def test_gpu_two_tile_cases_cover_the_channel_edges_and_variants():
    """(CPU) The cases pinned to the blocks of two column tiles stand at the channel counts where wn_gate_winograd4q_kernel
    and its launcher take another branch, and on every model variant that changes a path through the blocks."""
    two = {case[0]: case for case in CASES if case[3].get("tune", {}).get("gate_shape") == 4}
    assert set(TWO_TILE) == set(two) - {"lin5-two-tile-refused"} and len(set(TWO_TILE)) == len(TWO_TILE)
    assert all(64 in BLOCK_CHANNELS[cid] and set(BLOCK_CHANNELS[cid]) <= {0, 64} for cid in TWO_TILE)
    assert set(BLOCK_CHANNELS["lin5-two-tile-refused"]) == {32} and set(BLOCK_CHANNELS) <= {case[0] for case in CASES}
    chans = {int(case[1][1:]) for case in two.values() if case[1][1:].isdigit()}
    tiles, nk8 = (lambda C: (C + 31) // 32), (lambda C: (C + 7) // 8)
    assert chans == set(TWO_TILE_C) and all(tiles(C) == TWO_TILE_C[C] for C in chans)
    # a partial tile INSIDE a pair (an even tile count with C % 32 != 0): the zero page of issue_cond, the bias guard and ch_ok
    assert {C for C in chans if tiles(C) % 2 == 0 and C % 32} >= {36, 292, 356}
    # one pair only (q.n_tiles == 1), with and without an odd tile behind it; several pairs
    assert {C for C in chans if tiles(C) // 2 == 1} >= {36, 64, 68} and {C for C in chans if tiles(C) // 2 > 1} >= {132, 292}
    # the odd last tile in the one-tile kernel (ConvArgs::tile0), partial and full
    assert {C for C in chans if tiles(C) % 2 and C % 32} >= {68, 132, 324} and {C for C in chans if tiles(C) % 2 and C % 32 == 0} >= {352}
    # the K loop: the conditioning rows land in stage (nk8 - 1) & 1, so both parities; the smallest loop a model with two
    # column tiles has (C = 36: nk8 = 5, against the two stages of the prologue); a partial last slice (C % 8 == 4)
    assert {C for C in chans if nk8(C) % 2 == 0} >= {64, 352} and {C for C in chans if nk8(C) % 2} >= {36, 68, 292, 356}
    assert min(nk8(C) for C in chans) == nk8(36) == 5 and all(nk8(C) < 5 or tiles(C) < 2 for C in range(4, 36, 4))
    assert {C for C in chans if C % 8 == 4} >= {36, 68, 292, 356}
    # the variants: every gate activation (<0> and <-1>), an odd tile count on a 5-layer model, channel groups, both
    # conditioning up-samplings the shape takes, causal padding, a kept start convolution
    acts = {GEOMETRIES[case[1]][1].get(_WN + "activation", "gtu") for case in two.values()}
    assert acts == {"gtu", "gfu", "gsu", "glu"}
    ups = {GEOMETRIES[case[1]][1].get(_WN + "cond_lin_upsampling", 10) for cid, case in two.items() if cid in TWO_TILE}
    assert ups == {10, 20} and GEOMETRIES["lin5"][1][_WN + "cond_lin_upsampling"] == 5
    assert {"voice-two-tile", "groups2-two-tile", "causal-two-tile", "speech-keep-start-two-tile"} <= set(TWO_TILE)
    assert two["speech-keep-start-two-tile"][3].get("keep_start") and GEOMETRIES["causal"][1][_WN + "padding"] == "CAUSAL"
    # every two-tile case runs on the ragged batch: the oracle's stages are shared with the cases of the same geometry
    assert all(case[2] == "ragged" for case in two.values())
    # the large launch takes the shape by the size rule (gate_shape_policy: WIDE_FROM_BLOCKS = 5040)
    lengths = LENGTHS["large"][0]
    assert ((max(lengths) * 20 + 255) // 256) * len(lengths) * tiles(320) == 8800 >= 5040 and BLOCK_CHANNELS["large-f43"][1:] == [64] * 4


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    if not _torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return _torch


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """{case id: plan rows} of tests/tools/wn_plan_stage_cases.cpp for every stage case (built and run once)."""
    import sys
    import wn_stage_plan
    lines, _ = wn_stage_plan.stage_case_lines(sys.modules[__name__])
    return wn_stage_plan.run(wn_stage_plan.build(tmp_path_factory.mktemp("wn_stage_plan")), lines)


def _inputs(lengths, seed=907):
    T = max(lengths)
    mel, noise = synthetic_inputs(seed, len(lengths), T)
    return mel, noise


def _reference(geom, lkey, cfg, raw, wt, mel, noise, pulse):
    """The oracle's WaveNet stages for the checked items, cached per geometry, batch and excitation bits (the forms share
    one F0-net and oscillator, so their engines feed the WaveNet the same rows)."""
    lengths, items = LENGTHS[lkey]
    key = (geom, lkey, hash(pulse.tobytes()))
    if key not in _REFS:
        om64, om32 = oracle_models(cfg, raw, wt)
        xs = wavenet_inputs(om64, pulse, noise, lengths, 20)
        _REFS[key] = WaveNetReference(om64, om32, xs, mel, lengths, 20, items=items)
    return _REFS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("cid,geom,lkey,kwargs,kernels", CASES, ids=[case[0] for case in CASES])
def test_wavenet_stages_match_the_oracle(torch, planned, cid, geom, lkey, kwargs, kernels):
    from mbexwn_vocoder_amd.engine import GATE_KERNEL_NAMES, MBExWNEngine
    voice, over = GEOMETRIES[geom]
    cfg, raw, wt = build_case(voice, over)
    lengths, items = LENGTHS[lkey]
    B, T = len(lengths), max(lengths)
    mel, noise = _inputs(lengths)
    with tensor_table_of(cid):
        eng = MBExWNEngine(cfg, raw, wt, **kwargs)
    rpf = eng.dims.wn_in_rows_per_frame
    assert rpf == 20
    nf = torch.as_tensor(lengths, dtype=torch.int32).cuda()
    audio = eng.forward(torch.as_tensor(mel).cuda(), n_frames=nf, noise=torch.as_tensor(noise).cuda()).cpu().numpy()
    info = eng.conv_form_info()
    ran = info["gate_kernels"]
    assert len(ran) == eng.dims.wn_layers and set(ran) == kernels, f"{cid}: gate kernels {ran}, expected {sorted(kernels)}"
    if cid in BLOCK_CHANNELS:
        assert info["gate_block_channels"] == BLOCK_CHANNELS[cid], f"{cid}: gate block channels {info['gate_block_channels']}"
    # the forward ran what the library plans for this size (test_gpu_plan.py), and what the stand-alone program on wn_plan.h
    # prints for the case: the instantiations of test_wn_stage_plan_host.py are those of this run
    assert eng.plan(B, T) == eng.kernel_report(), f"{cid}: plan {eng.plan(B, T)}, report {eng.kernel_report()}"
    assert [GATE_KERNEL_NAMES[row[0]] for row in planned[cid]] == ran and [row[2] for row in planned[cid]] == info["gate_block_channels"], \
        f"{cid}: the host program plans {planned[cid]}, the forward ran {ran} {info['gate_block_channels']}"
    resskip, tail = KERNELS[cid]
    ran_rs, ran_tail = info["resskip_kernels"], info["tail_kernel"]
    assert info["fold_skip"] == (cid not in UNFOLDED), f"{cid}: fold_skip {info['fold_skip']}"
    assert len(ran_rs) == eng.dims.wn_layers - (1 if info["fold_skip"] else 0) and set(ran_rs) == resskip, \
        f"{cid}: res/skip kernels {ran_rs}, expected {sorted(resskip)}"
    assert (ran_tail, info["tail_folded"]) == (tail, info["fold_skip"]), f"{cid}: tail kernel {ran_tail}, expected {tail}"
    if kwargs.get("precision") == "split_f16":
        # layers 0 .. L - 2 run the split res/skip kernel; layer 0 runs a float32 one where its rows have no split image
        assert not info["split_rejected"] and info["split_f16_layers"] == eng.dims.wn_layers - (2 if cid in F32_LAYER0 else 1), info
        assert ran_rs[1:] == [SP] * (len(ran_rs) - 1) and ran_rs[0] == F32_LAYER0.get(cid, SP), f"{cid}: res/skip kernels {ran_rs}"
        assert ran[0] in (FS, PS) and SP not in ran[:1], f"{cid}: gate kernels {ran}"
        if SPF in kernels:
            assert ran[1] == SPF and set(ran[2:]) == {SP}, f"{cid}: gate kernels {ran}"
        if SPW in kernels:
            assert set(ran[1:]) == {SPW}, f"{cid}: gate kernels {ran}"
    names = ["wn_out", "wn_hidden"] + (["wn_skip"] if kwargs.get("keep_skip") else [])
    got = engine_stages(eng, names, B, T, items=items)
    planes = True
    try:
        eng.stage("wn_hidden_planes")
    except ValueError:
        planes = False
    assert planes == (cid in PLANES_ONLY), f"{cid}: plane-only hidden state {planes}"
    pulse = eng.stage("pulse").cpu().numpy().reshape(B, T * rpf, -1)
    eng.close()
    for ii, ll in enumerate(lengths):
        assert np.all(np.isfinite(audio[ii, :ll * 300])) and np.all(audio[ii, ll * 300:] == 0.0), f"{cid}: audio of item {ii}"
    ref = _reference(geom, lkey, cfg, raw, wt, mel, noise, pulse)
    rep = ref.compare(got, names=names)
    record = {"kernels": ran, "resskip_kernels": ran_rs, "tail_kernel": ran_tail,
              **{kk: {"err": vv["err"], "tol": vv["tol"], "port_err": vv["port_err"],
                      "ref_max": vv["ref_max"]} for kk, vv in rep.items()}}
    print(f"\nwavenet stages {cid}: {summary(rep)}  kernels {ran}  res/skip {ran_rs}  tail {ran_tail}")
    print("wavenet stages record " + json.dumps({cid: record}))       # with -s: one JSON line per case
    assert_matches(rep)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", TWO_TILE)
def test_two_tile_blocks_give_the_bits_of_the_one_tile_blocks_at_the_stages(torch, cid):
    """wn_gate_winograd4q_kernel's contract -- every accumulator chain, the output combination and the epilogue are those of the
    other shapes -- held where it is stated: "wn_out" and "wn_hidden" of every two-tile case are bit-identical, over every
    item's valid rows, to those of the same model pinned to the 256-row blocks of one column tile."""
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    _, geom, lkey, kwargs, _ = next(case for case in CASES if case[0] == cid)
    cfg, raw, wt = build_case(*GEOMETRIES[geom])
    lengths, _ = LENGTHS[lkey]
    B, T = len(lengths), max(lengths)
    mel, noise = _inputs(lengths)
    nf = torch.as_tensor(lengths, dtype=torch.int32).cuda()
    got = {}
    for shape in (4, 1):
        eng = MBExWNEngine(cfg, raw, wt, **dict(kwargs, tune={"gate_shape": shape}))
        eng.forward(torch.as_tensor(mel).cuda(), n_frames=nf, noise=torch.as_tensor(noise).cuda())
        rep = eng.kernel_report()
        want = [cc // 2 if shape == 1 else cc for cc in BLOCK_CHANNELS[cid]]
        assert rep["gate_block_channels"] == want, f"{cid}: gate_shape {shape} ran {rep['gate_kernels']} {rep['gate_block_channels']}"
        got[shape] = engine_stages(eng, ["wn_out", "wn_hidden"], B, T)
        eng.close()
    for name in ("wn_out", "wn_hidden"):
        for ii, ll in enumerate(lengths):
            a, b = got[4][name][ii, :ll * 20], got[1][name][ii, :ll * 20]
            assert np.all(np.isfinite(b)), f"{cid}: {name} of item {ii}"
            bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))      # (float32 values widened exactly)
            assert bad.size == 0, f"{cid}: {name} of item {ii} ({ll} frames) differs between the blocks of two column tiles and of " \
                                  f"one: {len(bad)} values, first at row {bad[0][0]} channel {bad[0][1]}: " \
                                  f"{a[tuple(bad[0])]!r} against {b[tuple(bad[0])]!r}"


# forms of the padding test on the blocks of two column tiles: {form: geometry}.  C = 292: the clamped conditioning and halo
# sources sit beside a tile whose missing channels read the zero page; C = 68: the pair launch and the one-tile launch write the
# same rows of `out`
TWO_TILE_PADDING = {"f43-two-tile": "speech", "f43-two-tile-c292": "c292", "f43-two-tile-c68": "c68"}


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["f43", "direct", "split_f16", "split_f16-c340", "split_f16-c340-wide", *TWO_TILE_PADDING])
def test_padding_frames_are_never_read(torch, form):
    """The same ragged batch three times, its padding frames of mel and noise at 0, 1e30 and NaN: the audio and every WaveNet
    stage of the items' valid rows are bit-identical across the three, and the audio behind each item's end is exactly 0.
    split_f16-c340: a partial last column tile, K step and plane chunk under the planes kernel and, with the shortest batch that
    reaches it (WIDE8), under wn_gate_f16w_kernel, whose halo rows and missing twelfth column tile are clamped sources: a
    clamped source that is not masked shows as the neighbour's NaN.  f43-two-tile*: the F(4,3) blocks of two column tiles
    (TWO_TILE_PADDING)."""
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    cfg, raw, wt = build_case(*GEOMETRIES[TWO_TILE_PADDING[form] if form in TWO_TILE_PADDING else "c340" if "c340" in form else "speech"])
    kwargs = {"conv_form": "f43", "precision": "split_f16"} if form.startswith("split_f16") else TWO if form in TWO_TILE_PADDING else {"conv_form": form}
    eng = MBExWNEngine(cfg, raw, wt, **kwargs)
    lengths = WIDE8 if form.endswith("-wide") else RAGGED
    B, T = len(lengths), max(lengths)
    mel, noise = _inputs(lengths, seed=911)
    nf = torch.as_tensor(lengths, dtype=torch.int32).cuda()
    runs = {}
    for fill in (0.0, 1e30, np.nan):
        m, n = mel.copy(), noise.copy()
        for ii, ll in enumerate(lengths):
            m[ii, ll:] = fill
            n[ii, ll * 20:] = fill
        audio = eng.forward(torch.as_tensor(m).cuda(), n_frames=nf, noise=torch.as_tensor(n).cuda()).cpu().numpy()
        st = engine_stages(eng, ["wn_out", "wn_hidden"], B, T)
        st["pulse"] = eng.stage("pulse").cpu().numpy().reshape(B, T * 20, -1)
        runs[fill] = (audio, st)
        if form.startswith("split_f16"):
            ran = eng.conv_form_info()["gate_kernels"]
            assert set(ran[1:]) == {SPW if form.endswith("-wide") else SP}, f"{form}: gate kernels {ran}"
        if form in TWO_TILE_PADDING:
            rep = eng.kernel_report()
            assert rep["gate_block_channels"] == [0] + [64] * (eng.dims.wn_layers - 1), f"{form}: {rep}"
    eng.close()
    base_audio, base_st = runs[0.0]
    for fill in (1e30, np.nan):
        audio, st = runs[fill]
        for ii, ll in enumerate(lengths):
            assert np.array_equal(audio[ii, :ll * 300], base_audio[ii, :ll * 300]), f"{form}: audio of item {ii}, padding {fill}"
            assert np.all(audio[ii, ll * 300:] == 0.0), f"{form}: audio behind item {ii}'s end, padding {fill}"
            for name in st:
                a, b = st[name][ii, :ll * 20], base_st[name][ii, :ll * 20]
                bad = np.argwhere(a != b)
                assert bad.size == 0, f"{form}: {name} of item {ii} ({ll} frames) differs with padding {fill}: first at row " \
                                      f"{bad[0][0]} channel {bad[0][1]}"
    for ii, ll in enumerate(lengths):
        assert np.all(np.isfinite(base_audio[ii, :ll * 300]))


_BLOCKS2 = {"mbexwn_config:pp_mod_subnet_upsampling_factors": [2, 1], "mbexwn_config:pp_mod_subnet_channel_factors": [1, 0.5],
            "mbexwn_config:pulse_channels": 10, _WN + "cond_lin_upsampling": 5, _WN + "n_channels": 32, _WN + "n_layers": 3}


@pytest.mark.gpu
@pytest.mark.parametrize("what,over,kwargs", [
    ("several WaveNet blocks", _BLOCKS2, {}),
    ("keep_skip", {_WN + "n_channels": 36, _WN + "n_layers": 3}, {"keep_skip": True}),
    ("C + n_out > 384", {_WN + "n_channels": 356, _WN + "n_layers": 3}, {}),
    ("two layers", {_WN + "n_channels": 36, _WN + "n_layers": 2}, {}),
], ids=["blocks", "keep-skip", "c356", "two-layers"])
def test_split_f16_refusals(torch, what, over, kwargs):
    """What the split precision does not cover is refused at creation with the C ABI's argument error and its message (no
    forward): a model of several WaveNet blocks, a kept skip tensor, C + n_out > 384 and fewer than three layers.  (glu:
    test_gpu_forms.py.)"""
    from mbexwn_vocoder_amd.engine import MBExWNEngine
    cfg, raw, wt = build_case("SPEECH", over)
    with pytest.raises(ValueError, match="wn_precision = split f16 needs the folded skip path, >= 3 layers, C \\+ n_out <= 384"):
        MBExWNEngine(cfg, raw, wt, conv_form="f43", precision="split_f16", **kwargs)

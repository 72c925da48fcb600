// mbx_create / mbx_destroy / mbx_workspace_size: validation of the configuration, upload of the tensors, their resolution into
// the records the launch sequence reads (mbx_handle.h), and the decisions that are fixed for the life of a handle (folded
// skip path / start convolution, split precision, form of the dilated convolution).
#include "mbx_handle.h"

using namespace mbx_host;

namespace {

const DevTensor *find(const mbx_handle *h, const std::string &name) {
    auto it = h->tensors.find(name);
    return it == h->tensors.end() ? nullptr : &it->second;
}

// floats per mel frame needed by the widest intermediate of a sub-net, and its time factor
mbx_status analyse_subnet(const mbx_subnet_op *ops, int n_ops, int cin, long long *per_frame, int *factor,
                          int *cout) {
    long long fac = 1, chan = cin, widest = cin;
    for (int i = 0; i < n_ops; ++i) {
        const mbx_subnet_op &op = ops[i];
        if (op.kind == MBX_OP_CONV) {
            if (op.cin != chan) return fail(MBX_ERR_INVALID_ARGUMENT, std::string("sub-net op ") + op.name + ": cin mismatch");
            if (op.up < 1 || op.cout % op.up) return fail(MBX_ERR_INVALID_ARGUMENT, "sub-pixel factor must divide cout");
            widest = std::max(widest, fac * op.cout);
            chan = op.cout / op.up;
            fac *= op.up;
        } else if (op.kind == MBX_OP_LIN) {
            fac *= op.up;
            widest = std::max(widest, fac * chan);
        }
    }
    *per_frame = widest;
    *factor = (int)fac;
    *cout = (int)chan;
    return MBX_OK;
}

// ---- tensor resolution: every name of the launch sequence is built and looked up here, once per handle, and every shape
// or size an optional weight image must have to be used is written here and nowhere else
const DevTensor *image_or_null(const mbx_handle *hd, const std::string &name, long long count) {
    const DevTensor *t = find(hd, name);
    return t && t->count == count ? t : nullptr;
}

const DevTensor *image_or_null(const mbx_handle *hd, const std::string &name, long long s0, long long s1, long long s2) {
    const DevTensor *t = find(hd, name);
    return t && t->ndim == 3 && t->shape[0] == s0 && t->shape[1] == s1 && t->shape[2] == s2 ? t : nullptr;
}

std::vector<SubnetOpTensors> resolve_subnet(const mbx_handle *hd, const mbx_subnet_op *ops, int n_ops) {
    std::vector<SubnetOpTensors> out(n_ops);
    for (int i = 0; i < n_ops; ++i) {
        const mbx_subnet_op &op = ops[i];
        const std::string name = op.name;
        if (op.kind == MBX_OP_CONV) {
            out[i].w = find(hd, name + ".w");
            out[i].b = find(hd, name + ".b");
            const DevTensor *t = image_or_null(hd, name + ".w64", 2LL * op.ks * op.cin * op.cout);
            if (t && !(reinterpret_cast<uintptr_t>(t->ptr) & 7)) out[i].w64 = reinterpret_cast<const double *>(t->ptr);
        } else if (op.kind == MBX_OP_PRELU) {
            out[i].alpha = find(hd, name + ".alpha");
        }
    }
    return out;
}

// the images of the folded res/skip layer `name` whose rows have cin channels (C, or C + 16 with the start convolution folded in)
FoldImages resolve_fold(const mbx_handle *hd, const std::string &name, int cin, int C, int n_out) {
    FoldImages im;
    im.fold = image_or_null(hd, name, (long long)((C + n_out + 127) / 128) * ((cin + 15) / 16) * 2048);
    im.wide = image_or_null(hd, name + "_wide", (cin + 7) / 8, (C + n_out + 31) / 32, 256);
    im.wave = image_or_null(hd, name + "_wave", (cin + 15) / 16, 12, 512);
    im.f16 = image_or_null(hd, name + "_f16", (long long)((cin + 31) / 32) * 12 * 1024);
    return im;
}

void resolve_tensors(mbx_handle *hd) {
    const mbx_config &c = hd->cfg;
    const int L = c.wn_layers, n_out = c.wn_out_channels;
    HandleTensors &tab = hd->tab;
    tab.post_w = find(hd, "post.w");
    tab.post_b = find(hd, "post.b");
    tab.wavetables = find(hd, "table.wavetables");
    tab.pulse_ana = find(hd, "table.pulse_ana");
    tab.hann = find(hd, "table.hann");
    tab.inv_win = find(hd, "table.inv_win");
    tab.ceps_windows = find(hd, "table.ceps_windows");
    tab.ceps_log10f0 = find(hd, "table.ceps_log10f0");
    tab.f0_smooth = find(hd, "table.f0_smooth");
    tab.nm_inv_enorm = find(hd, "table.nm_inv_enorm");
    tab.nm_pinv = find(hd, "table.nm_pinv");
    tab.nm_gwin = find(hd, "table.nm_gwin");
    tab.nm_smooth_win = find(hd, "table.nm_smooth_win");
    tab.f0 = resolve_subnet(hd, c.f0_ops, c.n_f0_ops);
    tab.vtf = resolve_subnet(hd, c.vtf_ops, c.n_vtf_ops);
    hd->wn.resize(std::max<size_t>(1, hd->blocks.size()));
    for (size_t b = 0; b < hd->wn.size(); ++b) {
        WnBlockTensors &bt = hd->wn[b];
        const bool multi = !hd->blocks.empty();
        const std::string p = multi ? hd->blocks[b].prefix : "wn.";
        const int C = multi ? hd->blocks[b].C : c.wn_channels;
        const std::vector<mbx_subnet_op> &cond_ops = multi ? hd->blocks[b].cond_ops : hd->cond_ops;
        bt.cond = resolve_subnet(hd, cond_ops.data(), (int)cond_ops.size());
        bt.start_w = find(hd, p + "start.w");
        bt.start_b = find(hd, p + "start.b");
        bt.end_w = find(hd, p + "end.w");
        bt.end_b = find(hd, p + "end.b");
        bt.end_packed = image_or_null(hd, p + "end.packed", (long long)((C + 7) / 8) * 256);
        bt.tail_fold = image_or_null(hd, p + "tail.fold", (long long)((C + 7) / 8) * 256);
        bt.tail_fold_b = image_or_null(hd, p + "tail.fold_b", n_out);
        bt.up_w = find(hd, "up" + std::to_string(b) + ".w");
        bt.up_b = find(hd, "up" + std::to_string(b) + ".b");
        bt.layer.resize(L);
        for (int l = 0; l < L; ++l) {
            WnLayerTensors &t = bt.layer[l];
            const std::string g = p + "conv1D_" + std::to_string(l), r = p + "res_skip_" + std::to_string(l);
            const int cout_l = l == L - 1 ? C : 2 * C;
            t.w = find(hd, g + ".w");
            t.b = find(hd, g + ".b");
            t.wino4w = image_or_null(hd, g + ".wino4w", (C + 31) / 32, (C + 7) / 8, 3072);
            t.wino2w = image_or_null(hd, g + ".wino2w", (C + 31) / 32, (C + 7) / 8, 2048);
            t.gate_f16 = image_or_null(hd, g + ".gate_f16", (long long)((C + 31) / 32) * ((C + 31) / 32) * 6144);
            t.start_fold = image_or_null(hd, g + ".start_fold", (long long)((C + 31) / 32) * 1536);
            t.res_w = find(hd, r + ".w");
            t.res_b = find(hd, r + ".b");
            t.packed = image_or_null(hd, r + ".packed", (cout_l + 127) / 128, (C + 15) / 16, 2048);
            t.fold_b = image_or_null(hd, r + ".fold_b", C + n_out);
            t.plain = resolve_fold(hd, r + ".fold", C, C, n_out);
            t.start = resolve_fold(hd, r + ".fold_start", C + 16, C, n_out);
            t.run = t.plain;      // (layer 0 under fold_start: mbx_create switches it to t.start)
        }
    }
}

// The whole F0-net in float64 (weights, hidden layers, head): its op list is (conv [prelu | leaky])* head, every layer has
// its float64 weights "<layer>.w64" and rows of whole float4 / double4 groups.  Other shapes of the grammar keep float32
// weights and hidden layers and accumulate in float64 (ConvArgs::precise alone).
bool f0_chain_is_full64(const mbx_handle *hd) {
    const mbx_config &c = hd->cfg;
    if (c.f0_accumulate != MBX_F0_ACC_F64 || c.n_f0_ops < 3) return false;
    int k = 0;
    while (k < c.n_f0_ops) {
        const mbx_subnet_op &op = c.f0_ops[k];
        if (op.kind != MBX_OP_CONV || op.up != 1 || op.cin % 4 || !hd->tab.f0[k].w64) return false;
        if (is_f0_head(c.f0_ops, c.n_f0_ops, k)) return k > 0;
        if (op.cout % 4) return false;
        ++k;
        if (k < c.n_f0_ops && (c.f0_ops[k].kind == MBX_OP_PRELU || c.f0_ops[k].kind == MBX_OP_LEAKY)) ++k;
    }
    return false;
}

}  // namespace

namespace mbx_host {

// ---- form of the dilated convolution -----------------------------------------------------------------------------------
// A Winograd form is available when the host supplied its weight images for every layer that runs a gate kernel and the
// kernel size is 3 (layers whose dilation does not fit the kernels fall back per layer).  CAUSAL padding runs the same
// kernels on a window shifted by d rows, on a single block whose configuration pins a Winograd form: MBX_CONV_AUTO and the
// block runner keep the direct form there.
bool form_available(const mbx_handle *hd, int form) {
    const mbx_config &c = hd->cfg;
    if (form == MBX_CONV_DIRECT) return true;
    if (form != MBX_CONV_F23 && form != MBX_CONV_F43) return false;
    if (c.wn_kernel_size != 3) return false;
    if (c.wn_causal && (!hd->blocks.empty() || (c.wn_conv_form != MBX_CONV_F23 && c.wn_conv_form != MBX_CONV_F43))) return false;
    const bool f43 = form == MBX_CONV_F43;
    auto images = [&](const WnBlockTensors &bt, int l0) {
        if (l0 >= c.wn_layers) return false;
        for (int l = l0; l < c.wn_layers; ++l)
            if (!(f43 ? bt.layer[l].wino4w : bt.layer[l].wino2w)) return false;
        return true;
    };
    if (!hd->blocks.empty()) {
        if (!f43) return false;             // the block runner knows the F(4,3) and the direct form
        for (const WnBlockTensors &bt : hd->wn)
            if (!images(bt, 0)) return false;
        return true;
    }
    return images(hd->wn[0], hd->pol.fold_start ? 1 : 0);
}

void set_form(mbx_handle *hd, int form) {
    hd->pol.winograd = form == MBX_CONV_F43 ? 4 : form == MBX_CONV_F23 ? 2 : 0;
    // causal padding without a pinned Winograd form, or in the block runner: the direct form (generic kernel)
    if (hd->cfg.wn_causal && !form_available(hd, form)) hd->pol.winograd = 0;
    hd->pol.winograd4_always = hd->pol.winograd == 4 && hd->cfg.batch_invariant != 0;
}

int current_form(const mbx_handle *hd) {
    return hd->pol.winograd == 4 ? MBX_CONV_F43 : hd->pol.winograd == 2 ? MBX_CONV_F23 : MBX_CONV_DIRECT;
}

}  // namespace mbx_host

extern "C" {

mbx_status mbx_create(const mbx_config *config, const mbx_tensor *tensors, int32_t n_tensors, int32_t device,
                      mbx_handle **out) {
    if (!config || !tensors || !out) return fail(MBX_ERR_INVALID_ARGUMENT, "null argument");
    if (config->struct_size != (int32_t)sizeof(mbx_config) || config->abi_version != MBX_ABI_VERSION)
        return fail(MBX_ERR_INVALID_ARGUMENT, "mbx_config ABI mismatch (struct_size / abi_version)");
    const mbx_config &c = *config;
    if (c.wn_layers < 1 || c.wn_layers > MBX_MAX_WN_LAYERS) return fail(MBX_ERR_INVALID_ARGUMENT, "wn_layers out of range");
    if (c.n_f0_ops < 1 || c.n_f0_ops > MBX_MAX_SUBNET_OPS || c.n_vtf_ops < (c.ps_off ? 0 : 1) || c.n_vtf_ops > MBX_MAX_SUBNET_OPS ||
        (c.ps_off && c.n_vtf_ops != 0))
        return fail(MBX_ERR_INVALID_ARGUMENT, "sub-net op count out of range (ps_off: no VTF-net)");
    if (c.wn_channels % 4 || c.wn_kernel_size % 2 != 1) return fail(MBX_ERR_INVALID_ARGUMENT, "wn_channels must be a multiple of 4, kernel size odd");
    if (c.fft_size > 2048 || (c.fft_size & (c.fft_size - 1)) || c.stft_win > c.fft_size || c.stft_win != 4 * c.hop_size)
        return fail(MBX_ERR_UNSUPPORTED, "STFT geometry: need power-of-two fft_size <= 2048 and win == 4*hop");
    if (c.hop_size % c.subbands || c.steps_per_frame * c.subbands != c.hop_size)
        return fail(MBX_ERR_INVALID_ARGUMENT, "hop_size must be steps_per_frame * subbands");
    // rows per frame of the first WaveNet block: the sub-band rate divided by the in-block upsampling factors
    int spf0 = c.steps_per_frame;
    if (c.n_wn_blocks > MBX_MAX_WN_BLOCKS || c.n_wn_blocks < 0) return fail(MBX_ERR_INVALID_ARGUMENT, "n_wn_blocks out of range");
    if (c.n_wn_blocks >= 1) {
        if (c.wn_block_channels[0] != c.wn_channels) return fail(MBX_ERR_INVALID_ARGUMENT, "wn_block_channels[0] must be wn_channels");
        for (int b = 0; b < c.n_wn_blocks; ++b) {
            if (c.wn_block_ups[b] < 1 || c.wn_block_channels[b] < 4 || c.wn_block_channels[b] % 4 || spf0 % c.wn_block_ups[b])
                return fail(MBX_ERR_INVALID_ARGUMENT, "WaveNet blocks: channels must be multiples of 4, upsampling factors must divide steps_per_frame");
            spf0 /= c.wn_block_ups[b];
        }
    }
    if (spf0 * c.pulse_channels != c.pulse_per_frame)
        return fail(MBX_ERR_INVALID_ARGUMENT, "pulse_per_frame must be (rows per frame of the first WaveNet block) * pulse_channels");
    if ((spf0 % c.cond_lin_upsampling) || spf0 / c.cond_lin_upsampling != c.cond_conv_upsampling)
        return fail(MBX_ERR_INVALID_ARGUMENT, "conditioning rates do not reach the WaveNet rate");
    if (c.wt_subharm_channels < 0 || c.wt_subharm_channels > 8) return fail(MBX_ERR_INVALID_ARGUMENT, "wt_subharm_channels out of range");
    if (c.wn_in_channels != c.pulse_channels * (1 + c.wt_subharm_channels) + (c.noise_sigma != 0.f ? 1 : 0))
        return fail(MBX_ERR_INVALID_ARGUMENT, "wn_in_channels must be pulse_channels * (1 + wt_subharm_channels) (+1 with noise)");
    if (c.ps_subband_gain && (c.n_ceps != c.subbands || c.ps_off || c.n_ceps_windows))
        return fail(MBX_ERR_INVALID_ARGUMENT, "ps_subband_gain: the VTF-net ends in one gain per sub-band (n_ceps == subbands), no lifter, not ps_off");
    if (c.pqmf_taps % 2) return fail(MBX_ERR_INVALID_ARGUMENT, "PQMF taps must be even");
    if (c.pulse_pqmf_taps < 0 || c.pulse_pqmf_taps % 2 || (c.pulse_pqmf_taps > 0 && c.wt_subharm_channels))
        return fail(MBX_ERR_INVALID_ARGUMENT, "pulse_pqmf_taps must be even and >= 0, and excludes wt_subharm_channels");
    if (c.phase_chunk < 1 || c.phase_chunk > 1024) return fail(MBX_ERR_INVALID_ARGUMENT, "phase_chunk must be in [1, 1024]");
    if (c.wn_gate_activation < MBX_GATE_GTU || c.wn_gate_activation > MBX_GATE_GLU)
        return fail(MBX_ERR_INVALID_ARGUMENT, "wn_gate_activation must be MBX_GATE_GTU, MBX_GATE_GFU, MBX_GATE_GSU or MBX_GATE_GLU");
    if (c.n_precond < 0 || c.n_precond > MBX_MAX_PRECOND) return fail(MBX_ERR_INVALID_ARGUMENT, "n_precond out of range");
    for (int i = 0; i < c.n_precond; ++i)
        if (c.precond_channels[i] < 1) return fail(MBX_ERR_INVALID_ARGUMENT, "precond_channels must be positive");
    if (c.tune_gate_shape < 0 || c.tune_gate_shape > 4 || c.tune_resskip_split < 0 || c.tune_resskip_split > 3 ||
        c.tune_resskip_wave_tiles < -1 || c.calib_fraction < 0.f || c.calib_fraction > 1.f)
        return fail(MBX_ERR_INVALID_ARGUMENT, "tune_* / calib_fraction out of range");

    mbx_handle *hd = new mbx_handle();
    hd->cfg = c;
    hd->device = device;
    auto bail = [&](mbx_status st) {
        mbx_destroy(hd);
        return st;
    };
    DeviceGuard guard(device);
    if (!guard.ok) {
        delete hd;
        return fail(MBX_ERR_HIP, "hipSetDevice: cannot select device " + std::to_string(device));
    }
    hipError_t e = hipSuccess;

    // interpolation factors in use
    std::vector<int> ups = {c.cond_lin_upsampling};
    if (c.ps_subband_gain) ups.push_back(c.hop_size);     // the sub-band gains are interpolated by hop_size
    ups.push_back(c.pulse_per_frame);                     // per-frame pitch control (mbx_forward_options.f0_frames / f0_scale)
    for (int i = 0; i < c.n_f0_ops; ++i)
        if (c.f0_ops[i].kind == MBX_OP_LIN) ups.push_back(c.f0_ops[i].up);
    for (int i = 0; i < c.n_vtf_ops; ++i)
        if (c.vtf_ops[i].kind == MBX_OP_LIN) ups.push_back(c.vtf_ops[i].up);

    // polyphase table of the PQMF synthesis bank
    const mbx_tensor *syn = nullptr;
    size_t total = 0;
    for (int i = 0; i < n_tensors; ++i) {
        long long cnt = 1;
        if (tensors[i].ndim < 1 || tensors[i].ndim > 4 || !tensors[i].data || !tensors[i].name)
            return bail(fail(MBX_ERR_INVALID_ARGUMENT, "malformed tensor entry"));
        for (int d = 0; d < tensors[i].ndim; ++d) cnt *= tensors[i].shape[d];
        total += align_up((size_t)cnt * sizeof(float), 256);
        if (std::strcmp(tensors[i].name, "table.pqmf_syn") == 0) syn = &tensors[i];
    }
    if (!syn || syn->ndim != 2 || syn->shape[0] != c.pqmf_taps + 1 || syn->shape[1] != c.subbands)
        return bail(fail(MBX_ERR_INVALID_ARGUMENT, "table.pqmf_syn must be (taps+1, subbands)"));
    const int M = c.subbands, half = c.pqmf_taps / 2;
    hd->poly_dm_min = -((half + M - 1) / M);
    const int dm_max = (half + M - 1) / M;
    hd->poly_ndm = dm_max - hd->poly_dm_min + 1;
    std::vector<float> poly((size_t)M * hd->poly_ndm * M, 0.f);
    for (int p = 0; p < M; ++p)
        for (int i = 0; i < hd->poly_ndm; ++i) {
            const int j = (hd->poly_dm_min + i) * M + half - p;
            if (j >= 0 && j <= c.pqmf_taps)
                for (int k = 0; k < M; ++k) poly[((size_t)p * hd->poly_ndm + i) * M + k] = syn->data[(size_t)j * M + k];
        }
    const int poly_k = hd->poly_ndm * M, poly_kpad = (poly_k + 3) / 4 * 4;
    std::vector<float> poly_t(M <= 16 ? (size_t)poly_kpad * 16 : 0, 0.f);
    if (M <= 16)
        for (int p = 0; p < M; ++p)
            for (int i = 0; i < poly_k; ++i) poly_t[(size_t)i * 16 + p] = poly[(size_t)p * poly_k + i];
    std::vector<float> tw((size_t)c.fft_size);
    for (int k = 0; k < c.fft_size / 2; ++k) {
        const double ang = -2.0 * M_PI * (double)k / (double)c.fft_size;
        tw[2 * k] = (float)std::cos(ang);
        tw[2 * k + 1] = (float)std::sin(ang);
    }
    total += align_up(poly.size() * sizeof(float), 256) + align_up(poly_t.size() * sizeof(float), 256) +
             align_up(tw.size() * sizeof(float), 256) + 256;
    for (int u : ups) total += 2 * align_up((size_t)u * sizeof(float), 256);

    e = hipMalloc(reinterpret_cast<void **>(&hd->arena), total);
    if (e != hipSuccess) return bail(fail(MBX_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e)));
    hd->arena_bytes = total;
    size_t off = 0;
    auto upload = [&](const float *src, size_t count) -> float * {
        float *dst = reinterpret_cast<float *>(hd->arena + off);
        off += align_up(count * sizeof(float), 256);
        hipError_t ee = hipMemcpy(dst, src, count * sizeof(float), hipMemcpyHostToDevice);
        return ee == hipSuccess ? dst : nullptr;
    };
    for (int i = 0; i < n_tensors; ++i) {
        DevTensor t;
        t.ndim = tensors[i].ndim;
        t.count = 1;
        for (int d = 0; d < t.ndim; ++d) {
            t.shape[d] = tensors[i].shape[d];
            t.count *= t.shape[d];
        }
        t.ptr = upload(tensors[i].data, (size_t)t.count);
        if (!t.ptr) return bail(fail(MBX_ERR_HIP, "hipMemcpy of a tensor failed"));
        hd->tensors[tensors[i].name] = t;
    }
    hd->poly = upload(poly.data(), poly.size());
    if (!poly_t.empty()) hd->poly_t = upload(poly_t.data(), poly_t.size());
    hd->twiddle = upload(tw.data(), tw.size());
    {
        std::vector<float> zz(64, 0.f);
        hd->zeros = upload(zz.data(), zz.size());
    }
    if (!hd->poly || !hd->twiddle || !hd->zeros) return bail(fail(MBX_ERR_HIP, "hipMemcpy of a table failed"));
    for (int u : ups) {
        if (hd->lerp.count(u)) continue;
        std::vector<float> w0(u), w1(u);
        for (int j = 0; j < u; ++j) {   // float32 of the float64 ratios (reference support_layers.py:19-27)
            w0[j] = (float)((double)(u - j) / (double)u);
            w1[j] = (float)((double)j / (double)u);
        }
        float *d0 = upload(w0.data(), u), *d1 = upload(w1.data(), u);
        if (!d0 || !d1) return bail(fail(MBX_ERR_HIP, "hipMemcpy of a table failed"));
        hd->lerp[u] = {d0, d1};
    }

    // required tensors
    std::vector<std::string> need = {"table.hann", "table.inv_win", "table.wavetables", "wn.start.w", "wn.start.b",
                                     "wn.end.w", "wn.end.b", "post.w", "post.b"};
    // conditioning chain (reference custom_AE_layers.py:190-227,283-289): pre-conditioning convolutions, then the
    // conditioning layer; all with kernel size cond_kernel_size and zero SAME padding, no activation in between
    auto cond_chain = [&](const std::string &prefix, int channels, int ccu, std::vector<mbx_subnet_op> &ops) {
        if (c.wn_disable_conditioning) return;
        int chan = c.mel_channels;
        auto add = [&](const std::string &nm, int cout) {
            mbx_subnet_op op{};
            op.kind = MBX_OP_CONV;
            op.ks = c.cond_kernel_size;
            op.cin = chan;
            op.cout = cout;
            op.pad_l = c.wn_causal ? c.cond_kernel_size - 1 : (c.cond_kernel_size - 1) / 2;
            op.pad_r = c.cond_kernel_size - 1 - op.pad_l;
            op.pad_mode = MBX_PAD_ZERO;
            op.up = 1;
            std::snprintf(op.name, MBX_NAME_LEN, "%s", nm.c_str());
            ops.push_back(op);
            need.push_back(nm + ".w");
            need.push_back(nm + ".b");
            chan = cout;
        };
        for (int i = 0; i < c.n_precond; ++i) {
            add(prefix + "precond_" + std::to_string(i), c.precond_channels[i]);
            hd->cond_buf_per_frame = std::max<long long>(hd->cond_buf_per_frame, c.precond_channels[i]);
        }
        add(prefix + "cond", 2 * channels * ccu);
    };
    cond_chain("wn.", c.wn_channels, c.cond_conv_upsampling, hd->cond_ops);
    // several WaveNet blocks (reference custom_pulsed_generator.py:456-488): every block has its own start / conditioning
    // / layer / end tensors; the up-sampling convolution "up<b>" sits behind block b
    if (c.n_wn_blocks >= 1) {
        int spf = spf0;
        for (int b = 0; b < c.n_wn_blocks; ++b) {
            mbx_handle::WnBlock blk;
            blk.C = c.wn_block_channels[b];
            blk.ups = c.wn_block_ups[b];
            blk.spf = spf;
            if (spf % c.cond_lin_upsampling) return bail(fail(MBX_ERR_INVALID_ARGUMENT, "a WaveNet block's rate is not a multiple of cond_lin_upsampling"));
            blk.ccu = spf / c.cond_lin_upsampling;
            blk.prefix = b == 0 ? "wn." : "wn" + std::to_string(b) + ".";
            if (b == 0) blk.cond_ops = hd->cond_ops;
            else cond_chain(blk.prefix, blk.C, blk.ccu, blk.cond_ops);
            hd->mb_hc_per_frame = std::max<long long>(hd->mb_hc_per_frame, (long long)spf * blk.C);
            if (b >= 1) {
                need.push_back(blk.prefix + "start.w");
                need.push_back(blk.prefix + "start.b");
                need.push_back(blk.prefix + "end.w");
                need.push_back(blk.prefix + "end.b");
                for (int l = 0; l < c.wn_layers; ++l)
                    for (const char *nm : {"conv1D_", "res_skip_"}) {
                        need.push_back(blk.prefix + nm + std::to_string(l) + ".w");
                        need.push_back(blk.prefix + nm + std::to_string(l) + ".b");
                    }
            }
            if (blk.ups > 1) {
                need.push_back("up" + std::to_string(b) + ".w");
                need.push_back("up" + std::to_string(b) + ".b");
            }
            spf *= blk.ups;
            hd->blocks.push_back(blk);
        }
    }
    if (c.nm_iters > 0) {
        if (c.nm_smooth_win < c.hop_size || c.nm_smooth_win % 2 || !(c.nm_rms_norm_fact > 0.f))
            return bail(fail(MBX_ERR_INVALID_ARGUMENT, "RMS normalisation: bad smoothing window / norm factor"));
        need.push_back("table.nm_inv_enorm");
        need.push_back("table.nm_gwin");
        need.push_back("table.nm_smooth_win");
        if (c.nm_use_pinv) {
            if (c.mel_channels > 256 || !(c.nm_win_norm > 0.f))
                return bail(fail(MBX_ERR_INVALID_ARGUMENT, "normalize_use_pinv: at most 256 mel channels, nm_win_norm > 0"));
            need.push_back("table.nm_pinv");
        }
    }
    if (c.pulse_pqmf_taps > 0) need.push_back("table.pulse_ana");
    if (c.n_ceps_windows) {
        need.push_back("table.ceps_windows");
        need.push_back("table.ceps_log10f0");
        need.push_back("table.f0_smooth");
    }
    for (int l = 0; l < c.wn_layers; ++l) {
        need.push_back("wn.conv1D_" + std::to_string(l) + ".w");
        need.push_back("wn.conv1D_" + std::to_string(l) + ".b");
        need.push_back("wn.res_skip_" + std::to_string(l) + ".w");
        need.push_back("wn.res_skip_" + std::to_string(l) + ".b");
    }
    for (const auto &nm : need)
        if (!find(hd, nm)) return bail(fail(MBX_ERR_INVALID_ARGUMENT, "missing tensor " + nm));
    auto expect = [&](const std::string &nm, long long count) {
        const DevTensor *t = find(hd, nm);
        return t && t->count == count;
    };
    const int C = c.wn_channels;
    bool ok = expect("wn.start.w", (long long)c.wn_in_channels * C) &&
              expect("wn.end.w", (long long)C * c.wn_out_channels) && expect("post.w", (long long)c.wn_out_channels * M) &&
              expect("table.hann", c.stft_win) && expect("table.inv_win", c.stft_win) &&
              expect("table.wavetables", (long long)(c.wt_n_period + 1) * c.wt_n_tables);
    for (const mbx_subnet_op &op : hd->cond_ops)
        ok = ok && expect(std::string(op.name) + ".w", (long long)op.ks * op.cin * op.cout) && expect(std::string(op.name) + ".b", op.cout);
    for (size_t b = 0; b < hd->blocks.size(); ++b) {
        const auto &blk = hd->blocks[b];
        const long long Cb = blk.C;
        if (b >= 1) {
            for (const mbx_subnet_op &op : blk.cond_ops)
                ok = ok && expect(std::string(op.name) + ".w", (long long)op.ks * op.cin * op.cout) && expect(std::string(op.name) + ".b", op.cout);
            ok = ok && expect(blk.prefix + "start.w", (long long)c.wn_out_channels * Cb) && expect(blk.prefix + "end.w", Cb * c.wn_out_channels);
            for (int l = 0; l < c.wn_layers && ok; ++l)
                ok = expect(blk.prefix + "conv1D_" + std::to_string(l) + ".w", (long long)c.wn_kernel_size * Cb * 2 * Cb) &&
                     expect(blk.prefix + "res_skip_" + std::to_string(l) + ".w", Cb * (l < c.wn_layers - 1 ? 2 * Cb : Cb));
        }
        if (blk.ups > 1)
            ok = ok && expect("up" + std::to_string(b) + ".w", 3LL * c.wn_out_channels * c.wn_out_channels * blk.ups);
    }
    for (int l = 0; l < c.wn_layers && ok; ++l) {
        ok = expect("wn.conv1D_" + std::to_string(l) + ".w", (long long)c.wn_kernel_size * C * 2 * C) &&
             expect("wn.res_skip_" + std::to_string(l) + ".w", (long long)C * (l < c.wn_layers - 1 ? 2 * C : C));
    }
    if (c.pulse_pqmf_taps > 0) ok = ok && expect("table.pulse_ana", (long long)(c.pulse_pqmf_taps + 1) * c.pulse_channels);
    if (c.n_ceps_windows)
        ok = ok && expect("table.ceps_windows", (long long)c.n_ceps_windows * c.n_ceps) &&
             expect("table.f0_smooth", 2 * c.hop_size + 1);
    if (c.nm_iters > 0)
        ok = ok && expect("table.nm_inv_enorm", c.mel_channels) && expect("table.nm_gwin", c.stft_win) &&
             expect("table.nm_smooth_win", c.nm_smooth_win) &&
             (!c.nm_use_pinv || expect("table.nm_pinv", (long long)c.mel_channels * (c.fft_size / 2 + 1)));
    if (!ok) return bail(fail(MBX_ERR_INVALID_ARGUMENT, "a tensor has the wrong number of elements"));
    resolve_tensors(hd);

    long long pf0 = 0, pvtf = 0;
    int f0_out = 0, vtf_out = 0;
    mbx_status st = analyse_subnet(c.f0_ops, c.n_f0_ops, c.mel_channels, &pf0, &hd->f0_time_factor, &f0_out);
    if (st != MBX_OK) return bail(st);
    if (!c.ps_off) {
        st = analyse_subnet(c.vtf_ops, c.n_vtf_ops, c.mel_channels, &pvtf, &hd->vtf_time_factor, &vtf_out);
        if (st != MBX_OK) return bail(st);
    }
    if (hd->f0_time_factor < c.pulse_per_frame || f0_out != 1)
        return bail(fail(MBX_ERR_INVALID_ARGUMENT, "F0 sub-net must end with 1 channel at >= pulse_per_frame samples per frame"));
    if (!c.ps_off && (hd->vtf_time_factor != 1 || vtf_out != c.n_ceps))
        return bail(fail(MBX_ERR_INVALID_ARGUMENT, "VTF sub-net must end with n_ceps channels at the mel frame rate"));
    hd->subnet_buf_per_frame = std::max(pf0, pvtf);
    if (c.f0_accumulate != MBX_F0_ACC_F64 && c.f0_accumulate != MBX_F0_ACC_F32)
        return bail(fail(MBX_ERR_INVALID_ARGUMENT, "f0_accumulate must be MBX_F0_ACC_F64 or MBX_F0_ACC_F32"));
    hd->f0_full64 = f0_chain_is_full64(hd);
    if (c.wn_conv_form < MBX_CONV_AUTO || c.wn_conv_form > MBX_CONV_F43)
        return bail(fail(MBX_ERR_INVALID_ARGUMENT, "wn_conv_form must be MBX_CONV_AUTO, _DIRECT, _F23 or _F43"));
    {
        // skip path folded into the end convolution when the host supplied the folded tensors (wn_keep_skip: keep
        // the skip tensor, e.g. to look at the "wn_skip" stage)
        std::vector<WnLayerTensors> &lt = hd->wn[0].layer;
        bool have = !c.wn_keep_skip && c.wn_out_channels <= 32 && M <= 16;
        for (int l = 0; l + 1 < c.wn_layers && have; ++l) have = lt[l].plain.fold && lt[l].fold_b;
        have = have && hd->wn[0].tail_fold && hd->wn[0].tail_fold_b;
        if (c.n_wn_blocks >= 1) have = false;      // several blocks: generic kernels (run_wavenet_blocks)
        // causal padding folds the start only under a pinned Winograd form: MBX_CONV_AUTO keeps the kernels it always ran
        const bool pinned = c.wn_conv_form == MBX_CONV_F23 || c.wn_conv_form == MBX_CONV_F43;
        const bool fold_pad = !c.wn_causal || pinned;
        hd->pol.fold_skip = have;
        // start convolution folded into layer 0 (wn_gate0.hip); wn_keep_start keeps the h0 tensor and the full layer
        bool have0 = have && fold_pad && !c.wn_keep_start && c.wn_kernel_size == 3 &&
                     mbx::wn_gate0_fits(C, c.pulse_channels * (1 + c.wt_subharm_channels), c.wn_dilations[0], c.cond_lin_upsampling) &&
                     lt[0].start_fold;
        if (have0 && c.wn_layers > 1) have0 = lt[0].start.fold != nullptr;
        hd->pol.fold_start = have0;
        if (have0) lt[0].run = lt[0].start;
    }
    if (c.wn_precision != MBX_PRECISION_F32 && c.wn_precision != MBX_PRECISION_SPLIT_F16)
        return bail(fail(MBX_ERR_INVALID_ARGUMENT, "wn_precision must be MBX_PRECISION_F32 or MBX_PRECISION_SPLIT_F16"));
    if (c.wn_precision == MBX_PRECISION_SPLIT_F16) {
        // opt-in experiment: folded res/skip layers 1 .. L-2 on the 16-bit matrix pipe (wn_resskip_f16.hip)
        if (c.wn_gate_activation == MBX_GATE_GLU)
            return bail(fail(MBX_ERR_UNSUPPORTED, "wn_precision = split f16 needs a bounded gate (not glu)"));
        bool have16 = hd->pol.fold_skip && c.wn_layers >= 3 && C + c.wn_out_channels <= 384;
        for (int l = 1; l + 1 < c.wn_layers && have16; ++l) have16 = hd->wn[0].layer[l].plain.f16 != nullptr;
        if (!have16)
            return bail(fail(MBX_ERR_INVALID_ARGUMENT, "wn_precision = split f16 needs the folded skip path, >= 3 layers, C + n_out <= 384 "
                                                        "and the wn.res_skip_<l>.fold_f16 images"));
        hd->pol.split_f16 = true;
        // ... and the gate layers behind the folded first one (wn_gate_f16.hip), where the host supplied their images
        hd->pol.split_f16_gate = hd->pol.fold_start && !c.wn_causal && c.wn_kernel_size == 3;
        for (int l = 1; l < c.wn_layers && hd->pol.split_f16_gate; ++l) hd->pol.split_f16_gate = hd->wn[0].layer[l].gate_f16 != nullptr;
    }
    {
        // what kernel selection depends on besides the form (wn_plan.h): the single block's shape, the images the host supplied
        // for its layers, and the dynamic-LDS sizes this device grants (asked for once, here, under the device guard)
        mbx::WnPolicy &p = hd->pol;
        p.C = C;
        p.n_out = c.wn_out_channels;
        p.M = M;
        p.L = c.wn_layers;
        p.cond_up = c.cond_lin_upsampling;
        p.ks = c.wn_kernel_size;
        p.causal = c.wn_causal;
        p.gate_act = c.wn_gate_activation;
        p.pulse_channels = c.pulse_channels * (1 + c.wt_subharm_channels);
        for (int l = 0; l < c.wn_layers; ++l) {
            p.dil[l] = c.wn_dilations[l];
            p.img[l] = (unsigned char)layer_images(hd->wn[0].layer[l]);
        }
        p.end_packed = hd->wn[0].end_packed != nullptr;
        p.lds_ok = mbx::wn_gate_f16_lds_opt_in() | mbx::wn_gate_winograd4q_lds_opt_in();
        hd->pol.gate_small_shape = c.tune_gate_shape - 1;
        if (c.tune_resskip_wave_tiles) hd->pol.resskip_wave_tiles = std::max(0, c.tune_resskip_wave_tiles);
        hd->pol.resskip_split = c.tune_resskip_split;
        // form of the dilated convolution: a Winograd form needs its weight images (for every layer that runs the gate
        // kernels), SAME padding and kernel size 3; a handle without them runs the direct form whatever was asked for
        const bool can43 = form_available(hd, MBX_CONV_F43), can23 = form_available(hd, MBX_CONV_F23);
        int form = c.wn_conv_form;
        const bool autoform = form == MBX_CONV_AUTO;
        if (autoform) form = can43 ? MBX_CONV_F43 : can23 ? MBX_CONV_F23 : MBX_CONV_DIRECT;
        if (form == MBX_CONV_F43 && !can43) form = can23 ? MBX_CONV_F23 : MBX_CONV_DIRECT;
        if (form == MBX_CONV_F23 && !can23) form = MBX_CONV_DIRECT;
        set_form(hd, form);
        if ((autoform && form != MBX_CONV_DIRECT) || hd->pol.split_f16) {
            // MBX_CONV_AUTO: the Winograd forms must earn their place on this handle's own weights -- and so must the opt-in
            // split precision, whatever the form (an overflow of fp16's range by the hidden state shows here as well)
            st = calibrate_on_synthetic_mel(hd, autoform && form != MBX_CONV_DIRECT);
            if (st != MBX_OK) return bail(st);
        }
    }
    *out = hd;
    return MBX_OK;
}

mbx_status mbx_destroy(mbx_handle *handle) {
    if (!handle) return MBX_OK;
    if (handle->arena) (void)hipFree(handle->arena);
    for (auto &pool : handle->ev_pool)
        for (auto &pr : pool) {
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
    delete handle;
    return MBX_OK;
}

size_t mbx_workspace_size(const mbx_handle *handle, int32_t batch, int32_t max_frames) {
    if (!handle || batch <= 0 || max_frames <= 0) return 0;
    return carve(handle, nullptr, batch, max_frames).total;
}

}  // extern "C"

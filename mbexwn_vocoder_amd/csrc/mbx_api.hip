// C ABI of the engine handle (include/mbexwn.h): the extern "C" surface apart from mbx_create / mbx_destroy /
// mbx_workspace_size (mbx_create.hip) and the entry points that take no handle (mbx_stages.hip) -- the forward entry points
// (their launch sequence: mbx_forward.hip; mbxe_forward of include/mbexwn_envelope.h is one of them), the calibration of the
// convolution form, the stage and profile readers, the stand-alone operator entry points and the window helpers.
// Nothing in here allocates, frees or synchronises after mbx_create apart from the calibration: every call only enqueues
// kernels on the caller's stream, so a forward pass can be captured into a hipGraph by the caller.
#include "mbx_handle.h"
#include "../../include/mbexwn_envelope.h"

using namespace mbx_host;

static const char *const kProfNames[PROF_KINDS] = {"gate", "res_skip", "frontend", "wavetable", "start", "tail", "pqmf",
                                                   "stft_filter", "overlap_add", "norm_mel", "gate0", "res_skip_f16"};

// One calibration: the same input through the direct form, F(4,3) and F(2,3); the fastest form whose audio differs from
// the direct form's by at most calib_fraction of the parity budget 1e-4 * max(1, |audio|) is adopted.  The difference
// between two float32 forms measures the rounding of the less exact one (F(4,3): ~5x the direct form's, growing with the
// amplitude of the residual stream).  Synchronises.
// forms: compare the convolution forms and adopt the fastest one within the threshold (MBX_CONV_AUTO at mbx_create,
// mbx_calibrate); false: only the split-precision check of a handle whose form the configuration pins
static mbx_status calibrate_run(mbx_handle *hd, const float *mel, const int32_t *n_frames, int B, int T, const float *noise,
                                void *workspace, size_t workspace_bytes, hipStream_t stream, int kind, bool forms = true) {
    const size_t n = (size_t)B * T * hd->cfg.hop_size;
    float *audio_dev = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&audio_dev), n * sizeof(float)));
    std::vector<float> ref(n), got(n);
    const bool was_profiling = hd->profiling;
    hd->profiling = false;
    const int form_before = current_form(hd);
    // the opt-in split precision is measured like a form: every reference and form run below is float32; the handle's
    // configuration in split precision is then held to the same threshold against the float32 direct form
    const bool split_req = hd->pol.split_f16, split_gate_req = hd->pol.split_f16_gate;
    hd->pol.split_f16 = hd->pol.split_f16_gate = false;
    auto run = [&](int form, std::vector<float> &host) -> mbx_status {
        set_form(hd, form);
        mbx_status st = forward_impl(hd, mel, n_frames, B, T, noise, audio_dev, workspace, workspace_bytes, stream);
        if (st != MBX_OK) return st;
        if (hipMemcpyAsync(host.data(), audio_dev, n * sizeof(float), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            return fail(MBX_ERR_HIP, "calibration: reading the audio back failed");
        return MBX_OK;
    };
    auto done = [&](mbx_status st) {
        (void)hipFree(audio_dev);
        hd->profiling = was_profiling;
        // the calibration forwards filled the stage table with pointers into their own (temporary, or by now overwritten)
        // workspace and strides of the calibration batch: mbx_stage answers "unknown stage" until the caller's next forward
        hd->stages.clear();
        hd->last_plan = mbx::WnPlan();
        if (st != MBX_OK) {
            set_form(hd, form_before);
            hd->pol.split_f16 = split_req;
            hd->pol.split_f16_gate = split_gate_req;
        }
        return st;
    };
    mbx_status st = run(MBX_CONV_DIRECT, ref);
    if (st != MBX_OK) return done(st);
    float ref_max = 0.f;
    bool finite = true;
    for (float v : ref) {
        if (!std::isfinite(v)) finite = false;
        ref_max = std::max(ref_max, std::fabs(v));
    }
    const float frac = hd->cfg.calib_fraction > 0.f ? hd->cfg.calib_fraction : 0.25f;
    const float threshold = frac * 1e-4f * std::max(1.f, ref_max);
    float err[2] = {-1.f, -1.f};
    const int form_list[2] = {MBX_CONV_F43, MBX_CONV_F23};
    for (int k = 0; k < 2 && forms; ++k) {
        if (!form_available(hd, form_list[k])) continue;
        st = run(form_list[k], got);
        if (st != MBX_OK) return done(st);
        float e = 0.f;
        for (size_t i = 0; i < n; ++i) {
            const float d = std::fabs(got[i] - ref[i]);
            e = std::isfinite(d) ? std::max(e, d) : INFINITY;
        }
        err[k] = e;
    }
    int form = forms ? MBX_CONV_DIRECT : form_before;
    if (forms && finite && err[0] >= 0.f && err[0] <= threshold) form = MBX_CONV_F43;
    else if (forms && finite && err[1] >= 0.f && err[1] <= threshold) form = MBX_CONV_F23;
    set_form(hd, form);
    if (forms) {
        hd->calibrated = kind;
        hd->calib_err43 = err[0];
        hd->calib_err23 = err[1];
    }
    hd->calib_ref = ref_max;
    hd->calib_threshold = threshold;
    if (split_req) {
        // the handle as it will run (its form, split precision on) against the float32 direct form
        hd->pol.split_f16 = true;
        hd->pol.split_f16_gate = split_gate_req;
        st = run(form, got);
        if (st != MBX_OK) return done(st);
        float e = 0.f;
        for (size_t i = 0; i < n; ++i) {
            const float d = std::fabs(got[i] - ref[i]);
            e = std::isfinite(d) ? std::max(e, d) : INFINITY;
        }
        hd->calib_err_split = e;
        // (the split precision rides on the form's own error: its budget is what the threshold leaves)
        hd->split_rejected = !(finite && e <= threshold);
        if (hd->split_rejected) hd->pol.split_f16 = hd->pol.split_f16_gate = false;
    }
    return done(MBX_OK);
}

// MBX_CONV_AUTO at mbx_create: two items of 40 frames of seeded synthetic log-mel input -- one with independent values
// of the level statistics the models are fed with (N(-5, 2^2) log amplitudes, clipped like scale_mel's output), one a
// smooth loud sweep that drives the conditioning towards the saturated side of the gates -- and a seeded noise draw.
// What is measured is this handle's own weights on plausible input, not the user's data: mbx_calibrate does that.
mbx_status mbx_host::calibrate_on_synthetic_mel(mbx_handle *hd, bool forms) {
    const mbx_config &c = hd->cfg;
    const int B = 2, T = 40;
    uint64_t rs = 0x9E3779B97F4A7C15ull;
    auto uni = [&]() {                       // xorshift64*: (0, 1]
        rs ^= rs >> 12;
        rs ^= rs << 25;
        rs ^= rs >> 27;
        return (double)(((rs * 0x2545F4914F6CDD1Dull) >> 11) + 1) / 9007199254740992.0;
    };
    auto gauss = [&]() { return std::sqrt(-2.0 * std::log(uni())) * std::cos(2.0 * M_PI * uni()); };
    std::vector<float> mel((size_t)B * T * c.mel_channels), noise((size_t)B * T * c.steps_per_frame);
    for (int t = 0; t < T; ++t)
        for (int m = 0; m < c.mel_channels; ++m) {
            const double v0 = std::log(std::exp(-5.0 + 2.0 * gauss()) + 1e-5);
            const double v1 = -3.0 + 4.0 * std::sin(0.21 * t + 0.08 * m) + 1.5 * std::cos(0.045 * m * (1 + t % 7)) + 0.3 * gauss();
            mel[((size_t)0 * T + t) * c.mel_channels + m] = (float)std::min(2.0, std::max(-11.5, v0));
            mel[((size_t)1 * T + t) * c.mel_channels + m] = (float)std::min(2.0, std::max(-11.5, v1));
        }
    for (float &v : noise) v = (float)gauss();
    const size_t ws_bytes = mbx_workspace_size(hd, B, T);
    float *mel_dev = nullptr, *noise_dev = nullptr;
    void *ws = nullptr;
    auto release = [&](mbx_status st) {
        if (mel_dev) (void)hipFree(mel_dev);
        if (noise_dev) (void)hipFree(noise_dev);
        if (ws) (void)hipFree(ws);
        return st;
    };
    if (hipMalloc(reinterpret_cast<void **>(&mel_dev), mel.size() * sizeof(float)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&noise_dev), noise.size() * sizeof(float)) != hipSuccess ||
        hipMalloc(&ws, ws_bytes) != hipSuccess ||
        hipMemcpy(mel_dev, mel.data(), mel.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(noise_dev, noise.data(), noise.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return release(fail(MBX_ERR_HIP, "calibration: device allocation / upload failed"));
    return release(calibrate_run(hd, mel_dev, nullptr, B, T, c.noise_sigma != 0.f ? noise_dev : nullptr, ws, ws_bytes, nullptr, 1, forms));
}

// mbx_conv1d and, precise, mbx_conv1d_f64acc: the way the launch sequence issues its mel-rate convolutions (large launches
// take the LDS-staged tile kernel)
static mbx_status conv1d_entry(mbx_handle *hd, const float *x, int32_t batch, int32_t n_rows, int32_t cin, const float *w,
                               const float *b, const float *alpha, int32_t ks, int32_t cout, int32_t dilation, int32_t pad_l,
                               int32_t pad_mode, float *y, void *hip_stream, bool precise) {
    if (!hd || !x || !w || !y || batch <= 0 || n_rows <= 0 || cin <= 0 || cout <= 0 || ks <= 0 || dilation <= 0)
        return fail(MBX_ERR_INVALID_ARGUMENT, "bad argument");
    if (pad_mode < MBX_PAD_ZERO || pad_mode > MBX_PAD_EDGE) return fail(MBX_ERR_INVALID_ARGUMENT, "bad pad_mode");
    if (precise && (cin % 4 || (reinterpret_cast<uintptr_t>(x) & 15)))
        return fail(MBX_ERR_UNSUPPORTED, "the float64-accumulating convolution needs cin % 4 == 0 and a 16-byte aligned input");
    DeviceGuard guard(hd->device);
    DevTensor wt, bt;
    wt.ptr = const_cast<float *>(w);
    bt.ptr = const_cast<float *>(b);
    mbx::ConvArgs a = conv_args(x, (long long)n_rows * cin, cin, nullptr, 1, n_rows, batch, &wt, b ? &bt : nullptr, ks,
                                cin, cout, dilation, pad_l, pad_mode, y, (long long)n_rows * cout, cout);
    a.alpha = alpha;
    a.precise = precise ? 1 : 0;
    if (!precise) a.zeros = hd->zeros;
    mbx::launch_conv1d_group(&a, 1, static_cast<hipStream_t>(hip_stream));
    return launch_status();
}

extern "C" {

const char *mbx_last_error(void) { return g_last_error.c_str(); }

mbx_status mbx_layer_state_info(const mbx_handle *hd, int32_t *floats_per_slot, int32_t *reach_rows, int32_t *min_rows) {
    if (!hd) return fail(MBX_ERR_INVALID_ARGUMENT, "null handle");
    const LayerGeom g = layer_geom(hd);
    if (floats_per_slot) *floats_per_slot = g.floats;
    if (reach_rows) *reach_rows = g.reach_rows;
    if (min_rows) *min_rows = g.min_rows;
    return MBX_OK;
}

mbx_status mbx_calibrate(mbx_handle *hd, const float *mel, const int32_t *n_frames, int32_t batch, int32_t max_frames,
                         const float *noise, void *workspace, size_t workspace_bytes, void *hip_stream) {
    if (!hd || !mel || !workspace) return fail(MBX_ERR_INVALID_ARGUMENT, "null argument");
    if (batch <= 0 || max_frames <= 0) return fail(MBX_ERR_INVALID_ARGUMENT, "batch and max_frames must be positive");
    DeviceGuard guard(hd->device);
    if (!guard.ok) return fail(MBX_ERR_HIP, "cannot select the handle's device");
    return calibrate_run(hd, mel, n_frames, batch, max_frames, noise, workspace, workspace_bytes,
                         static_cast<hipStream_t>(hip_stream), 2);
}

mbx_status mbx_conv_form(const mbx_handle *hd, mbx_conv_form_info *info) {
    if (!hd || !info || info->struct_size != (int32_t)sizeof(mbx_conv_form_info))
        return fail(MBX_ERR_INVALID_ARGUMENT, "mbx_conv_form_info ABI mismatch (struct_size)");
    info->requested = hd->cfg.wn_conv_form;
    info->form = current_form(hd);
    info->stream_form = hd->pol.winograd != 0 && form_available(hd, MBX_CONV_F23) ? MBX_CONV_F23 : MBX_CONV_DIRECT;
    info->calibrated = hd->calibrated;
    info->batch_invariant = (hd->pol.winograd != 4 || hd->pol.winograd4_always) ? 1 : 0;
    info->fold_skip = hd->pol.fold_skip;
    info->fold_start = hd->pol.fold_start;
    info->split_f16_layers = 0;
    for (int l = 0; hd->pol.split_f16 && l + 1 < hd->cfg.wn_layers; ++l)
        info->split_f16_layers += hd->wn[0].layer[l].run.f16 != nullptr;
    info->split_f16_gate_layers = hd->pol.split_f16_gate ? std::max(0, hd->cfg.wn_layers - 1) : 0;
    info->err_split = hd->calib_err_split;
    info->split_rejected = hd->split_rejected;
    info->err_f43 = hd->calib_err43;
    info->err_f23 = hd->calib_err23;
    info->ref_max = hd->calib_ref;
    info->threshold = hd->calib_threshold;
    info->f0_float64_chain = hd->f0_full64 ? 1 : 0;
    const mbx::WnPlan &plan = hd->last_plan;
    info->n_gate_layers = plan.n_layers;
    for (int l = 0; l < MBX_MAX_WN_LAYERS; ++l) info->gate_kernel[l] = l < plan.n_layers ? plan.gate[l].kernel : MBX_GATE_K_NONE;
    return MBX_OK;
}

mbx_status mbx_kernel_report(const mbx_handle *hd, mbx_kernel_report_info *info) {
    // (a caller built before gate_block_channels existed passes the size up to that field)
    const bool whole = info && info->struct_size == (int32_t)sizeof(mbx_kernel_report_info);
    if (!info || !(whole || info->struct_size == (int32_t)offsetof(mbx_kernel_report_info, gate_block_channels)))
        return fail(MBX_ERR_INVALID_ARGUMENT, "mbx_kernel_report_info ABI mismatch (struct_size)");
    if (!hd) return fail(MBX_ERR_INVALID_ARGUMENT, "mbx_kernel_report: null handle");
    const mbx::WnPlan &plan = hd->last_plan;
    info->n_resskip_layers = plan.n_layers;
    for (int l = 0; l < MBX_MAX_WN_LAYERS; ++l) info->resskip_kernel[l] = l < plan.n_layers ? plan.resskip[l] : MBX_RESSKIP_K_NONE;
    info->tail_kernel = plan.n_layers ? plan.tail : MBX_TAIL_K_NONE;
    info->tail_folded = plan.n_layers ? plan.tail_folded : 0;
    for (int l = 0; whole && l < MBX_MAX_WN_LAYERS; ++l)
        info->gate_block_channels[l] = l < plan.n_layers ? plan.gate[l].block_channels : 0;
    return MBX_OK;
}

mbx_status mbx_plan(const mbx_handle *hd, int32_t batch, int32_t max_frames, mbx_plan_info *info) {
    if (!info || info->struct_size != (int32_t)sizeof(mbx_plan_info)) return fail(MBX_ERR_INVALID_ARGUMENT, "mbx_plan_info ABI mismatch (struct_size)");
    if (!hd) return fail(MBX_ERR_INVALID_ARGUMENT, "mbx_plan: null handle");
    if (batch <= 0 || max_frames <= 0) return fail(MBX_ERR_INVALID_ARGUMENT, "batch and max_frames must be positive");
    if ((long long)max_frames * hd->cfg.steps_per_frame >= (1LL << 24))
        return fail(MBX_ERR_UNSUPPORTED, "an item may have at most 2^24 - 1 sub-band rows (split longer recordings)");
    const mbx::WnPlan plan = plan_whole_items(hd, batch, max_frames);
    if (plan.status != MBX_OK) return fail(plan.status, plan.error);
    info->n_layers = plan.n_layers;
    for (int l = 0; l < MBX_MAX_WN_LAYERS; ++l) {
        const bool in = l < plan.n_layers;
        info->gate_kernel[l] = in ? plan.gate[l].kernel : MBX_GATE_K_NONE;
        info->gate_kernel_f32[l] = in ? plan.gate_f32[l] : MBX_GATE_K_NONE;
        info->gate_block_channels[l] = in ? plan.gate[l].block_channels : 0;
        info->resskip_kernel[l] = in ? plan.resskip[l] : MBX_RESSKIP_K_NONE;
    }
    info->tail_kernel = plan.tail;
    info->tail_folded = plan.tail_folded;
    info->planes_only = plan.planes_only ? 1 : 0;
    return MBX_OK;
}

mbx_status mbx_forward(mbx_handle *hd, const float *mel, const int32_t *n_frames, int32_t batch, int32_t max_frames,
                       const float *noise, float *audio, void *workspace, size_t workspace_bytes, void *hip_stream) {
    return forward_impl(hd, mel, n_frames, batch, max_frames, noise, audio, workspace, workspace_bytes, hip_stream);
}

mbx_status mbx_forward_stream(mbx_handle *hd, const float *mel, const int32_t *n_frames, int32_t batch,
                              int32_t max_frames, const float *noise, float *audio, void *workspace,
                              size_t workspace_bytes, const mbx_stream_state *state_in, mbx_stream_state *state_out,
                              void *hip_stream) {
    static_assert(sizeof(mbx_stream_state) == sizeof(mbx::StreamState), "stream state layout");
    if (!state_in) return fail(MBX_ERR_INVALID_ARGUMENT, "state_in is required (use mbx_forward for whole utterances)");
    ForwardExtras ex;
    ex.st_in = reinterpret_cast<const mbx::StreamState *>(state_in);
    ex.st_out = reinterpret_cast<mbx::StreamState *>(state_out);
    return forward_impl(hd, mel, n_frames, batch, max_frames, noise, audio, workspace, workspace_bytes, hip_stream, ex);
}

// mbx_forward_ex and mbxe_forward (include/mbexwn_envelope.h): the options (null: none) and the formant shift (all three or none)
static mbx_status forward_with_options(mbx_handle *hd, const float *mel, const int32_t *n_frames, int32_t batch, int32_t max_frames,
                                       const float *noise, float *audio, void *workspace, size_t workspace_bytes,
                                       const mbx_forward_options *options, const float *env_factor, const float *env_centres,
                                       float *env_mel, void *hip_stream) {
    if ((env_factor != nullptr) != (env_centres != nullptr) || (env_factor != nullptr) != (env_mel != nullptr))
        return fail(MBX_ERR_INVALID_ARGUMENT, "env_factor, env_centres and env_mel go together (all three or none)");
    ForwardExtras ex;
    ex.env_factor = env_factor;
    ex.env_centres = env_centres;
    ex.env_mel = env_mel;
    if (!options) return forward_impl(hd, mel, n_frames, batch, max_frames, noise, audio, workspace, workspace_bytes, hip_stream, ex);
    // two sizes: the whole struct, or the struct as it was before the per-frame pitch control (f0_frames, f0_scale,
    // f0_item_mask are then not read: all NULL)
    const bool has_control = options->struct_size == (int32_t)sizeof(mbx_forward_options);
    if (!has_control && options->struct_size != (int32_t)offsetof(mbx_forward_options, f0_frames))
        return fail(MBX_ERR_INVALID_ARGUMENT, "mbx_forward_options ABI mismatch (struct_size)");
    if (!(options->transposition > 0.f)) return fail(MBX_ERR_INVALID_ARGUMENT, "transposition must be positive");
    const float *f0_frames = has_control ? options->f0_frames : nullptr, *f0_scale = has_control ? options->f0_scale : nullptr;
    const int32_t *f0_item_mask = has_control ? options->f0_item_mask : nullptr;
    if (f0_frames && options->f0)
        return fail(MBX_ERR_INVALID_ARGUMENT, "f0_frames (per mel frame) and f0 (per pulse sample) exclude each other");
    if ((f0_frames || f0_scale) && options->transposition != 1.f)
        return fail(MBX_ERR_INVALID_ARGUMENT, "f0_frames / f0_scale need transposition == 1 (put the factor into f0_scale)");
    if (f0_item_mask && !f0_frames) return fail(MBX_ERR_INVALID_ARGUMENT, "f0_item_mask needs f0_frames");
    if ((!options->layer_carry && options->layer_rows != 0) || options->layer_rows < 0)
        return fail(MBX_ERR_INVALID_ARGUMENT, "layer_rows must be >= 0 and needs layer_carry");
    const LayerOpts lay{options->layer_store, options->layer_store_floats, options->layer_carry, options->layer_rows};
    ex.st_in = reinterpret_cast<const mbx::StreamState *>(options->state_in);
    ex.st_out = reinterpret_cast<mbx::StreamState *>(options->state_out);
    ex.f0_in = options->f0;
    ex.transposition = options->transposition;
    ex.f0_frames = f0_frames;
    ex.f0_scale = f0_scale;
    ex.f0_item_mask = f0_item_mask;
    ex.active_begin = options->active_begin;
    ex.active_frames = options->active_frames;
    ex.wn_begin = options->wn_begin;
    ex.wn_frames = options->wn_frames;
    ex.sub_store = options->sub_store;
    ex.sub_store_rows = options->sub_store_rows;
    ex.sub_carry = options->sub_carry;
    ex.active_max_frames = options->active_max_frames;
    ex.wn_max_frames = options->wn_max_frames;
    ex.lay = options->layer_carry ? &lay : nullptr;
    ex.fe_store = options->fe_store;
    ex.fe_ring_frames = options->fe_ring_frames;
    ex.fe_pos = options->fe_pos;
    ex.fe_new_frames = options->fe_new_frames;
    ex.fe_margin_frames = options->fe_margin_frames;
    ex.fe_end_frames = options->fe_end_frames;
    return forward_impl(hd, mel, n_frames, batch, max_frames, noise, audio, workspace, workspace_bytes, hip_stream, ex);
}

mbx_status mbx_forward_ex(mbx_handle *hd, const float *mel, const int32_t *n_frames, int32_t batch, int32_t max_frames,
                          const float *noise, float *audio, void *workspace, size_t workspace_bytes,
                          const mbx_forward_options *options, void *hip_stream) {
    if (!options) return fail(MBX_ERR_INVALID_ARGUMENT, "mbx_forward_options ABI mismatch (struct_size)");
    return forward_with_options(hd, mel, n_frames, batch, max_frames, noise, audio, workspace, workspace_bytes, options, nullptr,
                                nullptr, nullptr, hip_stream);
}

mbx_status mbxe_forward(mbx_handle *hd, const float *mel, const int32_t *n_frames, int32_t batch, int32_t max_frames,
                        const float *noise, float *audio, void *workspace, size_t workspace_bytes,
                        const mbx_forward_options *options, const float *env_factor, const float *env_centres, float *env_mel,
                        void *hip_stream) {
    return forward_with_options(hd, mel, n_frames, batch, max_frames, noise, audio, workspace, workspace_bytes, options, env_factor,
                                env_centres, env_mel, hip_stream);
}

mbx_status mbx_window_advance(mbx_handle *hd, float *mel_window, const float *mel_new, float *noise_window,
                              const float *noise_new, int32_t batch, int32_t frames, int32_t step_frames, void *hip_stream) {
    if (!hd || !mel_window || !mel_new || (noise_window != nullptr) != (noise_new != nullptr))
        return fail(MBX_ERR_INVALID_ARGUMENT, "null argument (noise_window and noise_new go together)");
    DeviceGuard guard(hd->device);
    if (!guard.ok) return fail(MBX_ERR_HIP, "cannot select the handle's device");
    if (!mbx::launch_window_advance(mel_window, mel_new, noise_window, noise_new, batch, frames, step_frames,
                                    hd->cfg.mel_channels, hd->cfg.steps_per_frame, static_cast<hipStream_t>(hip_stream)))
        return fail(MBX_ERR_INVALID_ARGUMENT, "window advance: need 0 < step_frames <= frames and a window of at most 64 KB per item");
    return launch_status();
}

mbx_status mbx_clock_probe(mbx_handle *hd, uint64_t *device_out4, int64_t real_ticks, void *hip_stream) {
    if (!hd || !device_out4 || real_ticks <= 0 || real_ticks > 100000000LL)
        return fail(MBX_ERR_INVALID_ARGUMENT, "clock probe: need a device buffer of 4 x uint64 and 0 < real_ticks <= 1e8 (1 s)");
    DeviceGuard guard(hd->device);
    if (!guard.ok) return fail(MBX_ERR_HIP, "cannot select the handle's device");
    mbx::launch_clock_probe(reinterpret_cast<unsigned long long *>(device_out4), (unsigned long long)real_ticks,
                            static_cast<hipStream_t>(hip_stream));
    return launch_status();
}

mbx_status mbx_window_update(mbx_handle *hd, float *mel_window, const float *mel_new, float *noise_window,
                             const float *noise_new, int32_t batch, int32_t window_frames, int32_t shift_frames,
                             int32_t keep_frames, int32_t new_frames, void *hip_stream) {
    if (!hd || !mel_window || !mel_new || (noise_window != nullptr) != (noise_new != nullptr))
        return fail(MBX_ERR_INVALID_ARGUMENT, "null argument (noise_window and noise_new go together)");
    DeviceGuard guard(hd->device);
    if (!guard.ok) return fail(MBX_ERR_HIP, "cannot select the handle's device");
    if (!mbx::launch_window_update(mel_window, mel_new, noise_window, noise_new, batch, window_frames, shift_frames, keep_frames,
                                   new_frames, hd->cfg.mel_channels, hd->cfg.steps_per_frame, static_cast<hipStream_t>(hip_stream)))
        return fail(MBX_ERR_INVALID_ARGUMENT, "window update: need shift + keep <= window, keep + new <= window and at most 64 KB kept per item");
    return launch_status();
}

mbx_status mbx_emit_rows(mbx_handle *hd, const float *audio, int64_t row_floats, int32_t batch, int64_t first, int64_t count,
                         float *host_out, void *hip_stream) {
    if (!hd || !audio || !host_out || batch <= 0 || count <= 0 || first < 0 || first + count > row_floats)
        return fail(MBX_ERR_INVALID_ARGUMENT, "emit rows: need 0 <= first, first + count <= row_floats");
    DeviceGuard guard(hd->device);
    if (!guard.ok) return fail(MBX_ERR_HIP, "cannot select the handle's device");
    HIP_TRY(hipMemcpy2DAsync(host_out, (size_t)count * sizeof(float), audio + first, (size_t)row_floats * sizeof(float),
                             (size_t)count * sizeof(float), (size_t)batch, hipMemcpyDeviceToHost, static_cast<hipStream_t>(hip_stream)));
    return MBX_OK;
}

mbx_status mbx_profile_enable(mbx_handle *handle, int32_t enabled) {
    if (!handle) return fail(MBX_ERR_INVALID_ARGUMENT, "null argument");
    handle->profiling = enabled != 0;
    return MBX_OK;
}

mbx_status mbx_profile_read(mbx_handle *handle, const char *kernel, double *total_ms, int64_t *launches) {
    if (!handle || !kernel || !total_ms || !launches) return fail(MBX_ERR_INVALID_ARGUMENT, "null argument");
    int kind = -1;
    for (int k = 0; k < PROF_KINDS; ++k)
        if (std::strcmp(kernel, kProfNames[k]) == 0) kind = k;
    if (kind < 0) return fail(MBX_ERR_INVALID_ARGUMENT, std::string("unknown profile stage ") + kernel);
    double sum = 0.0;
    for (size_t i = 0; i < handle->ev_used[kind]; ++i) {
        auto &pr = handle->ev_pool[kind][i];
        HIP_TRY(hipEventSynchronize(pr.second));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
        sum += ms;
    }
    *total_ms = sum;
    *launches = (int64_t)handle->ev_used[kind];
    handle->ev_used[kind] = 0;
    return MBX_OK;
}

mbx_status mbx_profile_read_launches(mbx_handle *handle, const char *kernel, float *launch_ms, int64_t capacity,
                                     int64_t *launches) {
    if (!handle || !kernel || !launches || (capacity > 0 && !launch_ms) || capacity < 0)
        return fail(MBX_ERR_INVALID_ARGUMENT, "null argument");
    int kind = -1;
    for (int k = 0; k < PROF_KINDS; ++k)
        if (std::strcmp(kernel, kProfNames[k]) == 0) kind = k;
    if (kind < 0) return fail(MBX_ERR_INVALID_ARGUMENT, std::string("unknown profile stage ") + kernel);
    for (size_t i = 0; i < handle->ev_used[kind]; ++i) {
        auto &pr = handle->ev_pool[kind][i];
        HIP_TRY(hipEventSynchronize(pr.second));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
        if ((int64_t)i < capacity) launch_ms[i] = ms;
    }
    *launches = (int64_t)handle->ev_used[kind];
    handle->ev_used[kind] = 0;
    return MBX_OK;
}

mbx_status mbx_stage(const mbx_handle *handle, const char *name, const void **device_ptr, int64_t *count,
                     int64_t *stride) {
    if (!handle || !name || !device_ptr || !count || !stride) return fail(MBX_ERR_INVALID_ARGUMENT, "null argument");
    auto it = handle->stages.find(name);
    if (it == handle->stages.end()) return fail(MBX_ERR_INVALID_ARGUMENT, std::string("unknown stage ") + name);
    *device_ptr = it->second.ptr;
    *count = it->second.count;
    *stride = it->second.stride;
    return MBX_OK;
}

mbx_status mbx_pqmf_synthesis(mbx_handle *hd, const float *x, int32_t batch, int32_t n_steps, float *y,
                              void *hip_stream) {
    if (!hd || !x || !y || batch <= 0 || n_steps <= 0) return fail(MBX_ERR_INVALID_ARGUMENT, "bad argument");
    DeviceGuard guard(hd->device);
    const int M = hd->cfg.subbands;
    mbx::launch_pqmf(x, (long long)n_steps * M, nullptr, 1, n_steps, batch, M, hd->poly, hd->poly_t, hd->poly_ndm,
                     hd->poly_dm_min, y, (long long)n_steps * M, static_cast<hipStream_t>(hip_stream));
    return launch_status();
}

mbx_status mbx_conv1d(mbx_handle *hd, const float *x, int32_t batch, int32_t n_rows, int32_t cin, const float *w,
                      const float *b, const float *alpha, int32_t ks, int32_t cout, int32_t dilation, int32_t pad_l,
                      int32_t pad_mode, float *y, void *hip_stream) {
    return conv1d_entry(hd, x, batch, n_rows, cin, w, b, alpha, ks, cout, dilation, pad_l, pad_mode, y, hip_stream, false);
}

mbx_status mbx_conv1d_f64acc(mbx_handle *hd, const float *x, int32_t batch, int32_t n_rows, int32_t cin, const float *w,
                             const float *b, const float *alpha, int32_t ks, int32_t cout, int32_t dilation, int32_t pad_l,
                             int32_t pad_mode, float *y, void *hip_stream) {
    return conv1d_entry(hd, x, batch, n_rows, cin, w, b, alpha, ks, cout, dilation, pad_l, pad_mode, y, hip_stream, true);
}

mbx_status mbx_lin_interp(mbx_handle *hd, const float *x, int32_t batch, int32_t n_rows, int32_t channels, int32_t up,
                          float *y, void *hip_stream) {
    if (!hd || !x || !y || batch <= 0 || n_rows <= 0 || channels <= 0) return fail(MBX_ERR_INVALID_ARGUMENT, "bad argument");
    DeviceGuard guard(hd->device);
    auto it = hd->lerp.find(up);
    if (it == hd->lerp.end()) return fail(MBX_ERR_INVALID_ARGUMENT, "interpolation factor not part of this model");
    mbx::launch_lin_interp(x, (long long)n_rows * channels, nullptr, 1, n_rows, batch, channels, up, it->second.first,
                           it->second.second, MBX_ACT_LINEAR, 1.f, 0.f, y, (long long)n_rows * up * channels,
                           static_cast<hipStream_t>(hip_stream));
    return launch_status();
}

mbx_status mbx_wavetable(mbx_handle *hd, const float *f0, int32_t batch, int32_t n, float *pulse, float *phase,
                         float *scratch, void *hip_stream) {
    if (!hd || !f0 || !pulse || !scratch || batch <= 0 || n <= 0) return fail(MBX_ERR_INVALID_ARGUMENT, "bad argument");
    DeviceGuard guard(hd->device);
    float *cum = scratch;
    float *chunk_last = scratch + (size_t)batch * n;
    mbx::launch_wavetable(wavetable_consts(hd), f0, n, nullptr, 1, n, batch, pulse, phase, cum, chunk_last, nullptr,
                          nullptr, static_cast<hipStream_t>(hip_stream));
    return launch_status();
}

mbx_status mbx_norm_mel(mbx_handle *hd, const float *mel, const int32_t *n_frames, int32_t batch, int32_t frames,
                        float *mel_out, float *gain, float *scratch, void *hip_stream) {
    if (!hd || !mel || !mel_out || !scratch || batch <= 0 || frames <= 0)
        return fail(MBX_ERR_INVALID_ARGUMENT, "bad argument");
    if (hd->cfg.nm_iters <= 0) return fail(MBX_ERR_INVALID_ARGUMENT, "this model has no RMS normalisation (nm_iters == 0)");
    DeviceGuard guard(hd->device);
    const mbx_config &c = hd->cfg;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    mbx::NormMelConsts k = norm_mel_consts(hd);
    const float *src = mbx::launch_norm_mel(k, mel, (long long)frames * c.mel_channels, n_frames, frames, batch, scratch,
                                            scratch + (size_t)batch * frames, mel_out, stream);
    if (gain)
        mbx::launch_norm_mel_gain(k, src, n_frames, frames, batch, gain, (long long)frames * c.hop_size, true, stream);
    return launch_status();
}

mbx_status mbx_stft_filter(mbx_handle *hd, const float *excitation, const float *cepstrum, const int32_t *ceps_index,
                           int32_t batch, int32_t frames, float *audio, float *scratch, void *hip_stream) {
    if (!hd || !excitation || !cepstrum || !audio || !scratch || batch <= 0 || frames <= 0)
        return fail(MBX_ERR_INVALID_ARGUMENT, "bad argument");
    DeviceGuard guard(hd->device);
    const mbx_config &c = hd->cfg;
    mbx::StftConsts sc = stft_consts(hd);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    mbx::launch_stft_filter(sc, excitation, (long long)frames * c.hop_size, cepstrum, (long long)frames * c.n_ceps,
                            c.n_ceps_windows ? ceps_index : nullptr, nullptr, 0, nullptr, nullptr, frames, batch, scratch,
                            stream);
    mbx::launch_overlap_add(sc, scratch, nullptr, frames, frames, batch, audio, (long long)frames * c.hop_size, stream);
    return launch_status();
}

}  // extern "C"

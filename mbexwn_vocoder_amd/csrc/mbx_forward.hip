// The launch sequence of one forward pass (mbx_forward, mbx_forward_stream, mbx_forward_ex and the calibration runs), as the
// stages of DESIGN.md section 1: forward_impl at the end of this file is their table of contents.
//
// The sequence restates the inference branch of MBExWN.call
// (reference MBExWN_NVoc/vocoder/model/custom_pulsed_generator.py:556-771) driven the way
// PaNWaveNet.infer drives it (reference MBExWN_NVoc/vocoder/model/wavegen_1d.py:483-526).
// Nothing in here allocates device memory, frees or synchronises: every call only enqueues kernels on the caller's stream,
// so a forward pass can be captured into a hipGraph by the caller.  Nothing in here builds a tensor name either: the
// tensors were resolved into the handle's records at mbx_create.
#include <optional>

#include "mbx_handle.h"

using namespace mbx_host;

namespace {
// Executes a sub-net op list (reference custom_pulsed_generator.py:38-148 flattened by the host).
// in (B, T, cin) -> final (B, T*factor, cout); optional affine y*scale+offset applied after the last op.
// Resumable: next_conv() launches the element-wise ops up to the next convolution and hands that convolution back
// un-launched, so that the caller can put the convolutions of independent sub-nets into one launch
// (launch_conv1d_group); the caller launches it before calling next_conv() again.
struct SubnetRun {
    mbx_handle *hd;
    const mbx_subnet_op *ops;
    const SubnetOpTensors *tens;   // the ops' tensors (resolved at mbx_create)
    int n_ops;
    const int *n_frames;
    int B, T;
    float *buf0, *buf1, *final_out;
    float scale, offset;
    hipStream_t stream;
    const float *cur;
    int chan, rpf = 1, pp = 0, last_writer = -1, i = 0;
    long long cur_bstride;
    long long stride_frames = 0;   // > 0: frames between batch items of the input and of the final output (a sub-window of a
                                   // longer window is being computed: mbx_forward_options.fe_new_frames); 0: T
    bool affine_done, finished = false;
    bool precise = false;          // the F0-net under mbx_config.f0_accumulate == MBX_F0_ACC_F64: float64 accumulation in its
                                   // convolutions (ConvArgs::precise) and its head -- final 1x1 convolution to one channel,
                                   // interpolation, final activation, affine map -- as one float64 kernel
    double *buf64_0 = nullptr, *buf64_1 = nullptr;   // ... with float64 weights and hidden layers (mbx_handle::f0_full64)
    const double *cur64 = nullptr;                   // the current tensor when it is a float64 one (cur is null then)
    mbx_status status = MBX_OK;
    void window_stride(long long frames, int cin) {
        stride_frames = frames;
        cur_bstride = frames * cin;
    }

    SubnetRun(mbx_handle *hd_, const mbx_subnet_op *ops_, const SubnetOpTensors *tens_, int n_ops_, const float *in, int cin, const int *n_frames_,
              int B_, int T_, float *buf0_, float *buf1_, float *final_out_, bool affine, float scale_, float offset_,
              hipStream_t stream_)
        : hd(hd_), ops(ops_), tens(tens_), n_ops(n_ops_), n_frames(n_frames_), B(B_), T(T_), buf0(buf0_), buf1(buf1_),
          final_out(final_out_), scale(scale_), offset(offset_), stream(stream_), cur(in), chan(cin),
          cur_bstride((long long)T_ * cin), affine_done(!affine) {
        // index of the last op that launches a kernel writing a new buffer
        for (int k = 0; k < n_ops; ++k)
            if (ops[k].kind == MBX_OP_CONV || ops[k].kind == MBX_OP_LIN) last_writer = k;
    }
    bool stop(mbx_status st) {
        status = st;
        finished = true;
        return false;
    }
    bool next_conv(mbx::ConvArgs &pending) {
        if (finished) return false;
        for (; i < n_ops; ++i) {
            const mbx_subnet_op &op = ops[i];
            if (op.kind == MBX_OP_CONV) {
                const DevTensor *w = tens[i].w, *bias = tens[i].b;
                if (!w || !bias) return stop(fail(MBX_ERR_INVALID_ARGUMENT, std::string("missing tensor ") + op.name + ".w/.b"));
                // float64 head: [conv 1x1 -> 1 channel] [lin] ([act]) at the end of the list
                const int n_tail = n_ops - i;
                if (precise && is_f0_head(ops, n_ops, i)) {
                    const mbx_subnet_op &lin = ops[i + 1];
                    auto it = hd->lerp.find(lin.up);
                    if (it == hd->lerp.end()) return stop(fail(MBX_ERR_INVALID_ARGUMENT, "interpolation table missing"));
                    const long long out_bstride = (stride_frames ? stride_frames : (long long)T) * rpf * lin.up;
                    mbx::launch_f0_head(cur, cur64, cur_bstride, op.cin, n_frames, rpf, T * rpf, B, w->ptr,
                                        buf64_0 ? tens[i].w64 : nullptr, bias->ptr, lin.up,
                                        it->second.first, it->second.second, n_tail == 3 ? ops[i + 2].act : MBX_ACT_LINEAR,
                                        affine_done ? 1.f : scale, affine_done ? 0.f : offset, final_out, out_bstride, stream);
                    cur64 = nullptr;
                    affine_done = true;
                    cur = final_out;
                    chan = 1;
                    rpf *= lin.up;
                    cur_bstride = out_bstride;
                    i = n_ops;
                    break;
                }
                float *out = (i == last_writer) ? final_out : (pp ? buf1 : buf0);
                pp ^= 1;
                const long long out_bstride = ((i == last_writer && stride_frames) ? stride_frames : (long long)T) * rpf * op.cout;
                mbx::ConvArgs a = conv_args(cur, cur_bstride, chan, n_frames, rpf, T * rpf, B, w, bias, op.ks, op.cin,
                                            op.cout, 1, op.pad_l, op.pad_mode, out, out_bstride, op.cout);
                a.precise = precise ? 1 : 0;
                a.zeros = hd->zeros;
                if (buf64_0) {             // full-float64 chain (the op list was checked at mbx_create: f0_chain_is_full64)
                    double *out64 = (pp ^ 1) ? buf64_1 : buf64_0;       // (pp was toggled above)
                    a.w64 = tens[i].w64;
                    a.x64 = cur64;
                    a.out64 = out64;
                    if (cur64) a.x = nullptr;
                    a.out = nullptr;
                    cur64 = out64;
                    out = nullptr;
                }
                if (i + 1 < n_ops && ops[i + 1].kind == MBX_OP_PRELU && op.up == 1) {
                    const DevTensor *al = tens[i + 1].alpha;
                    if (!al) return stop(fail(MBX_ERR_INVALID_ARGUMENT, std::string("missing tensor ") + ops[i + 1].name + ".alpha"));
                    a.alpha = al->ptr;
                    ++i;
                } else if (i + 1 < n_ops && ops[i + 1].kind == MBX_OP_LEAKY) {
                    a.use_leaky = 1;
                    a.leaky = ops[i + 1].alpha;
                    ++i;
                }
                cur = out;
                chan = op.cout / op.up;
                rpf *= op.up;
                cur_bstride = out_bstride;
                ++i;
                pending = a;
                return true;
            } else if (op.kind == MBX_OP_LIN) {
                auto it = hd->lerp.find(op.up);
                if (it == hd->lerp.end()) return stop(fail(MBX_ERR_INVALID_ARGUMENT, "interpolation table missing"));
                float *out = (i == last_writer) ? final_out : (pp ? buf1 : buf0);
                pp ^= 1;
                int act = MBX_ACT_LINEAR;
                float sc = 1.f, of = 0.f;
                int consumed = 0;
                if (i + 1 < n_ops && ops[i + 1].kind == MBX_OP_ACT) {
                    act = ops[i + 1].act;
                    consumed = 1;
                }
                if (i + consumed == n_ops - 1 && !affine_done) {
                    sc = scale;
                    of = offset;
                    affine_done = true;
                }
                const long long out_bstride = ((i == last_writer && stride_frames) ? stride_frames : (long long)T) * rpf * op.up * chan;
                mbx::launch_lin_interp(cur, cur_bstride, n_frames, rpf, T * rpf, B, chan, op.up, it->second.first,
                                       it->second.second, act, sc, of, out, out_bstride, stream);
                i += consumed;
                cur = out;
                rpf *= op.up;
                cur_bstride = out_bstride;
            } else if (op.kind == MBX_OP_PRELU || op.kind == MBX_OP_LEAKY) {
                const DevTensor *al = tens[i].alpha;
                if (op.kind == MBX_OP_PRELU && !al) return stop(fail(MBX_ERR_INVALID_ARGUMENT, "missing PReLU slopes"));
                mbx::launch_prelu(const_cast<float *>(cur), cur_bstride, n_frames, rpf, T * rpf, B, chan,
                                  al ? al->ptr : nullptr, op.alpha, stream);
            } else if (op.kind == MBX_OP_ACT) {
                float sc = 1.f, of = 0.f;
                if (i == n_ops - 1 && !affine_done) {
                    sc = scale;
                    of = offset;
                    affine_done = true;
                }
                mbx::launch_activation(cur, cur_bstride, n_frames, rpf, T * rpf, B, chan, op.act, sc, of,
                                       const_cast<float *>(cur), cur_bstride, stream);
            } else {
                return stop(fail(MBX_ERR_INVALID_ARGUMENT, "unknown sub-net op kind"));
            }
        }
        if (!affine_done)
            mbx::launch_activation(cur, cur_bstride, n_frames, rpf, T * rpf, B, chan, MBX_ACT_LINEAR, scale, offset,
                                   const_cast<float *>(cur), cur_bstride, stream);
        if (cur != final_out) return stop(fail(MBX_ERR_INVALID_ARGUMENT, "sub-net without a convolution"));
        finished = true;
        return false;
    }
};

// A span = the rows of the window one launch treats as the item: first row, per-item row counts (nf[b] * rpf, or
// max_rows for every item when nf is null), conditioning-rate phase of the first row.  Whole-region runs use one span
// for every launch; a steady streaming tick (layer state carried, mbx_forward_options.layer_rows) one per layer.
// out0 / out_rows: the rows of a gate span that are consumed (the others are the layer's reach: inputs only)
struct Span { long long row0; const int32_t *nf; int rpf, max_rows, cphase, out0, out_rows; };

// One forward pass: the call's arguments, what check_forward_args derives from them, and what a stage leaves for a later one.
struct ForwardCtx {
    mbx_handle *hd;
    const mbx_config &c;
    const ForwardExtras &ex;
    std::optional<DeviceGuard> guard;
    Workspace w{};
    int B, T;
    hipStream_t stream;
    const float *mel;              // (run_norm_mel: the normalised / the aligned copy from there on)
    const float *mel_env = nullptr; // run_envelope: the rows the VTF and conditioning chains read (mel itself without a formant shift)
    const int32_t *n_frames;
    const float *noise;
    float *audio;
    long long npulse, nsteps;      // pulse samples / sub-band rows of the window
    int cond_cout;                 // conditioning floats per mel frame
    // mel-rate front end carried between the ticks of a stream (mbx_forward_options.fe_store): fe_frames > 0 = only the
    // last fe_frames frames of the window are computed, the frames in front of them come from the ring
    int fe_frames = 0, fe_end = 0;
    // active region (streaming windows, mbx_forward_options): behind the excitation every stage sees the frames
    // [active_begin, active_begin + active_frames[b]) of the window as the item.  All buffers are (batch, frames * k)
    // with the batch stride of the whole window, so a region is a row offset into every buffer plus per-item row counts.
    long long act0 = 0, wn0 = 0;   // (the WaveNet may have a region of its own inside the active one: wn_begin / wn_frames)
    const int32_t *n_frames_act = nullptr, *n_frames_wn = nullptr;
    int wn_rows = 0, act_frames_max = 0;       // upper bounds of the rows / frames an item can have in its region
    // single block: the spans of its launches (plan_layer_spans)
    bool carry_layers = false, layered = false;
    LayerGeom geo{};
    Span gate_sp[MBX_MAX_WN_LAYERS], res_sp[MBX_MAX_WN_LAYERS], tail_sp;
    // left by the stages
    const float *nm_gain_src = nullptr;        // run_norm_mel: the gain run_backend multiplies onto the audio
    const float *pulse_wn = nullptr;           // run_excitation: the excitation rows the WaveNet reads
    mbx::WnPlan plan;                          // check_forward_args: the kernel of every WaveNet launch (wn_plan.h)

    ForwardCtx(mbx_handle *hd_, const ForwardExtras &ex_, const float *mel_, const int32_t *n_frames_, int B_, int T_,
               const float *noise_, float *audio_, void *hip_stream)
        : hd(hd_), c(hd_->cfg), ex(ex_), B(B_), T(T_), stream(static_cast<hipStream_t>(hip_stream)), mel(mel_),
          n_frames(n_frames_), noise(noise_), audio(audio_), npulse((long long)T_ * hd_->cfg.pulse_per_frame),
          nsteps((long long)T_ * hd_->cfg.steps_per_frame), cond_cout(2 * hd_->cfg.wn_channels * hd_->cfg.cond_conv_upsampling) {}
    bool streamed() const { return ex.st_in || ex.st_out; }
};

// ---- argument builders ------------------------------------------------------------------------------------------------

mbx::WnSpan wn_span(const Span &sp) { return mbx::WnSpan{sp.max_rows, sp.cphase, sp.out0, sp.out_rows}; }

// Gate layer of a block with C channels on the span sp: h, a are (B, rows, C) with the batch stride bstride, cond the
// block's conditioning rows (B, rows / cond_up, 2 C).  Dimensions and strides: wn_gate_dims, which the plan was made from
mbx::ConvArgs gate_args(mbx_handle *hd, const WnLayerTensors &t, int C, int d, const float *h, float *a, long long bstride,
                        const Span &sp, int B, const float *cond, long long cond_bstride) {
    const mbx_config &c = hd->cfg;
    mbx::ConvArgs g = mbx::wn_gate_dims(hd->pol, C, d, bstride, wn_span(sp), B, cond_bstride);
    g.x = h + sp.row0 * C;
    g.n_frames = sp.nf;
    g.rows_per_frame = sp.rpf;
    g.w = t.w->ptr;
    g.bias = t.b ? t.b->ptr : nullptr;
    g.out = a + sp.row0 * C;
    const auto &lerp = hd->lerp[c.cond_lin_upsampling];
    g.cond = cond + (sp.row0 / c.cond_lin_upsampling) * (2 * C);
    g.lerp_w0 = lerp.first;
    g.lerp_w1 = lerp.second;
    g.zeros = hd->zeros;
    return g;
}

// Layer 0 with the start convolution folded in (wn_gate0.hip): rows, conditioning and bias of the gate's ConvArgs, the
// excitation instead of the hidden state, rows of ldo floats out
mbx::Gate0Args gate0_args(const ForwardCtx &cx, const mbx::ConvArgs &g, const WnLayerTensors &t, long long row0) {
    const mbx_config &c = cx.c;
    const int nsub1 = 1 + c.wt_subharm_channels;              // floats per excitation sample (pulse + sub-harmonic sinusoids)
    mbx::Gate0Args g0 = mbx::wn_gate0_dims(cx.hd->pol, g, cx.nsteps);
    g0.pulse = cx.pulse_wn + row0 * (c.pulse_per_frame / c.steps_per_frame * nsub1);
    g0.pulse_bstride = cx.npulse * nsub1;
    g0.noise = c.noise_sigma != 0.f ? cx.noise + row0 : nullptr;
    g0.noise_bstride = cx.nsteps;
    g0.sigma = c.noise_sigma;
    g0.n_frames = g.n_frames;
    g0.rows_per_frame = g.rows_per_frame;
    g0.w = t.start_fold->ptr;
    g0.bias = g.bias;
    g0.cond = g.cond;
    g0.lerp_w0 = g.lerp_w0;
    g0.lerp_w1 = g.lerp_w1;
    g0.out = cx.w.a + row0 * g0.ldo;
    return g0;
}

// per-layer state of a stream: the rows layer l reads from in front of its own come from the item's slot, the rows the
// next tick will read go there (layer_carry_kernel)
mbx::LayerCarryArgs layer_carry_args(const ForwardCtx &cx, int l) {
    const LayerGeom &geo = cx.geo;
    const int C = cx.c.wn_channels, n_out = cx.c.wn_out_channels;
    mbx::LayerCarryArgs lc{};
    lc.h = cx.w.h;
    lc.h_bstride = cx.nsteps * C;
    lc.C = C;
    lc.acc = cx.w.wn_out;
    lc.acc_bstride = cx.nsteps * n_out;
    lc.n_out = n_out;
    lc.store = cx.ex.lay->store;
    lc.slot_stride = geo.floats;
    lc.layer_off = geo.off[l];
    lc.desc = cx.ex.lay->carry;
    lc.inject = cx.layered;
    lc.base_off = geo.c[l] - geo.reach_rows;
    lc.h_before = geo.r[l];
    lc.h_rows = geo.r[l] + geo.step[l];
    lc.acc_rows = geo.step[l];
    return lc;
}

// res/skip layer with a skip tensor (un-folded single block, block runner): a, h, skip are (B, rows, C)
mbx::ConvArgs resskip_args(mbx_handle *hd, const WnLayerTensors &t, int C, int l, const float *a, float *h, float *skip,
                           long long bstride, const Span &sp, int B) {
    mbx::ConvArgs r = mbx::wn_resskip_dims(C, l == 0, l == hd->cfg.wn_layers - 1, bstride, sp.max_rows, B);
    r.x = a + sp.row0 * C;
    r.n_frames = sp.nf;
    r.rows_per_frame = sp.rpf;
    r.w = t.res_w->ptr;
    r.bias = t.res_b ? t.res_b->ptr : nullptr;
    r.zeros = hd->zeros;
    r.h = h + sp.row0 * C;
    r.skip = skip + sp.row0 * C;
    return r;
}

// res/skip layer l < L - 1 with the skip path folded into the end convolution (wn_resskip_fold_dims): a (B, rows, C, or C + 16
// under ext) -> h (B, rows, C) and the n_out-wide output accumulator
mbx::ConvArgs resskip_fold_args(const ForwardCtx &cx, const WnLayerTensors &t, int l, bool ext, const Span &sp) {
    const int C = cx.c.wn_channels, n_out = cx.c.wn_out_channels;
    mbx::ConvArgs r = mbx::wn_resskip_fold_dims(cx.hd->pol, l == 0, ext, cx.nsteps, sp.max_rows, cx.B);
    r.x = cx.w.a + sp.row0 * r.cin;
    r.n_frames = sp.nf;
    r.rows_per_frame = sp.rpf;
    r.w = t.run.fold->ptr;
    r.bias = t.fold_b ? t.fold_b->ptr : nullptr;
    r.zeros = cx.hd->zeros;
    r.h = cx.w.h + sp.row0 * C;
    r.skip = cx.w.wn_out + sp.row0 * n_out;
    return r;
}

// ---- stages -----------------------------------------------------------------------------------------------------------

mbx_status plan_layer_spans(ForwardCtx &cx);
mbx::WnGeometry wn_geometry(const ForwardCtx &cx);
mbx::WnPlan plan_blocks(const mbx_handle *hd, int B, int T);

// The formant shift of the call (mbxe_forward: env_factor): the whole window of the mel the chains read -> env_mel
mbx::EnvelopeArgs envelope_args(const ForwardCtx &cx) {
    mbx::EnvelopeArgs a{};
    a.mel = cx.mel;
    a.bstride = (long long)cx.T * cx.c.mel_channels;
    a.batch = cx.B;
    a.n_frames = cx.n_frames;
    a.max_frames = cx.T;
    a.n_mels = cx.c.mel_channels;
    a.centres = cx.ex.env_centres;
    a.factors = cx.ex.env_factor;
    a.out = cx.ex.env_mel;
    return a;
}

// Every check that needs no launch, in front of the first launch; carves the workspace and derives the regions.
mbx_status check_forward_args(ForwardCtx &cx, void *workspace, size_t workspace_bytes) {
    mbx_handle *hd = cx.hd;
    const mbx_config &c = cx.c;
    const ForwardExtras &ex = cx.ex;
    const int T = cx.T;
    const bool fe_on = ex.fe_store != nullptr;
    cx.fe_end = ex.fe_end_frames > 0 ? ex.fe_end_frames : T;      // frames of the items of a steady tick
    if (fe_on) {
        if (!ex.fe_pos || !ex.sub_carry || ex.fe_ring_frames < T || ex.fe_new_frames < 0 || ex.fe_margin_frames < 0 ||
            cx.fe_end > T || ex.fe_new_frames + ex.fe_margin_frames > cx.fe_end)
            return fail(MBX_ERR_INVALID_ARGUMENT, "fe_store needs fe_pos, sub_carry (slots), fe_ring_frames >= max_frames, "
                                                  "fe_end_frames <= max_frames and fe_new_frames + fe_margin_frames <= fe_end_frames");
        if (c.nm_iters > 0 || hd->f0_time_factor > c.pulse_per_frame || ex.f0_in)
            return fail(MBX_ERR_UNSUPPORTED, "the front end cannot be carried for this model / call (RMS normalisation, an F0-net "
                                             "that runs above the pulse rate, an external F0 contour)");
        if ((2 * c.wn_channels * c.cond_conv_upsampling) % 4 || c.n_ceps % 4 || c.pulse_per_frame % 4)
            return fail(MBX_ERR_UNSUPPORTED, "the front end ring needs per-frame sizes that are multiples of 4 floats");
        if (ex.fe_new_frames > 0) cx.fe_frames = ex.fe_new_frames + ex.fe_margin_frames;
    }
    if (cx.B <= 0 || T <= 0) return fail(MBX_ERR_INVALID_ARGUMENT, "batch and max_frames must be positive");
    // row and sample indices inside the kernels are 32-bit ints (offsets are 64-bit or block relative): 2^24 sub-band
    // rows per item = 2.9 h of audio at the canonical 1.6 kHz is the tested side of that
    if ((long long)T * c.steps_per_frame >= (1LL << 24))
        return fail(MBX_ERR_UNSUPPORTED, "an item may have at most 2^24 - 1 sub-band rows (split longer recordings)");
    if (!hd->blocks.empty() && (ex.active_frames || ex.st_in || ex.st_out || ex.sub_carry || ex.lay || fe_on))
        return fail(MBX_ERR_UNSUPPORTED, "a model with several WaveNet blocks runs whole items only (no stream windows / state)");
    cx.guard.emplace(hd->device);
    if (!cx.guard->ok) return fail(MBX_ERR_HIP, "cannot select the handle's device");
    if (c.noise_sigma != 0.f && !cx.noise) return fail(MBX_ERR_INVALID_ARGUMENT, "noise is required when noise_sigma != 0");
    if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0) return fail(MBX_ERR_INVALID_ARGUMENT, "workspace must be 256-byte aligned");
    if (ex.active_begin < 0 || ex.active_begin >= T || (ex.active_begin > 0 && !ex.active_frames))
        return fail(MBX_ERR_INVALID_ARGUMENT, "active_begin must lie inside the window and needs active_frames");
    if (ex.wn_frames && (!ex.active_frames || ex.wn_begin < ex.active_begin || ex.wn_begin >= T))
        return fail(MBX_ERR_INVALID_ARGUMENT, "wn_frames needs active_frames and wn_begin inside the active region");
    if ((ex.sub_store != nullptr) != (ex.sub_carry != nullptr) || (ex.sub_store && ex.sub_store_rows <= 0))
        return fail(MBX_ERR_INVALID_ARGUMENT, "sub_store, sub_store_rows and sub_carry go together");
    if (ex.env_factor)
        if (const char *why = mbx::check_envelope(envelope_args(cx)))
            return fail(MBX_ERR_INVALID_ARGUMENT, std::string("formant shift (env_factor / env_centres / env_mel): ") + why);
    cx.w = carve(hd, static_cast<char *>(workspace), cx.B, T);
    if (cx.w.total > workspace_bytes) return fail(MBX_ERR_WORKSPACE, "workspace too small, see mbx_workspace_size");

    cx.n_frames_act = ex.active_frames ? ex.active_frames : cx.n_frames;   // PQMF, STFT filter, overlap-add
    cx.act0 = ex.active_frames ? ex.active_begin : 0;
    cx.wn0 = ex.active_frames ? (ex.wn_frames ? ex.wn_begin : ex.active_begin) : 0;
    cx.n_frames_wn = ex.active_frames ? (ex.wn_frames ? ex.wn_frames : ex.active_frames) : cx.n_frames;
    // the launchers size their grids (and pick block shapes) from the bounds; batch strides stay those of the whole window
    int wn_frames_max = T - (int)cx.wn0;
    const int wn_bound = ex.wn_frames ? ex.wn_max_frames : ex.active_max_frames;
    if (ex.active_frames && wn_bound > 0) wn_frames_max = std::min(wn_frames_max, wn_bound);
    cx.wn_rows = wn_frames_max * c.steps_per_frame;
    cx.act_frames_max = T - (int)cx.act0;
    if (ex.active_frames && ex.active_max_frames > 0) cx.act_frames_max = std::min(cx.act_frames_max, ex.active_max_frames);

    const bool windowed = ex.active_frames || ex.st_in || ex.st_out;
    if (c.pulse_pqmf_taps > 0 && windowed) return fail(MBX_ERR_UNSUPPORTED, "pulse_channels_use_pqmf models run whole items only");
    if (hd->blocks.empty()) {
        const mbx_status st = plan_layer_spans(cx);
        if (st != MBX_OK) return st;
        // the kernel of every WaveNet launch, and "does not fit" in front of the first launch
        cx.plan = mbx::wn_plan(hd->pol, wn_geometry(cx));
        if (cx.plan.status != MBX_OK) return fail(cx.plan.status, cx.plan.error);
        if (c.pulse_per_frame % c.steps_per_frame != 0)
            return fail(MBX_ERR_INVALID_ARGUMENT, "pulse_per_frame must be a multiple of steps_per_frame");
    }
    if (c.ps_subband_gain && windowed) return fail(MBX_ERR_UNSUPPORTED, "ps_use_stft: false models run whole items only");
    if (!hd->blocks.empty()) cx.plan = plan_blocks(hd, cx.B, T);
    return MBX_OK;
}

// The spans of the single block's launches: the WaveNet's region for every launch, or one span per layer where a stream
// carries layer state and runs its new rows only (mbx_forward_options.layer_rows).  Host arithmetic only.
mbx_status plan_layer_spans(ForwardCtx &cx) {
    mbx_handle *hd = cx.hd;
    const mbx_config &c = cx.c;
    const LayerOpts *lay = cx.ex.lay;
    const int L = c.wn_layers, spf = c.steps_per_frame, cond_up = c.cond_lin_upsampling;
    const Span region{cx.wn0 * spf, cx.n_frames_wn, spf, cx.wn_rows, 0, 0, 0};
    for (int l = 0; l < L; ++l) cx.gate_sp[l] = cx.res_sp[l] = region;
    cx.tail_sp = region;
    cx.carry_layers = lay && lay->carry;
    cx.layered = cx.carry_layers && lay->rows > 0;
    if (cx.carry_layers) {
        cx.geo = layer_geom(hd);
        if (!cx.geo.floats) return fail(MBX_ERR_UNSUPPORTED, "this handle cannot carry layer state (mbx_layer_state_info)");
        if (!lay->store || lay->floats != cx.geo.floats)
            return fail(MBX_ERR_INVALID_ARGUMENT, "layer_store / layer_store_floats do not match mbx_layer_state_info");
    }
    if (!cx.layered) return MBX_OK;
    // every item: state stored up to row E - N, region end E; layer l runs on [s_l, s_l + N), s_l = E - N - reach + c_l
    const LayerGeom &geo = cx.geo;
    const int N = lay->rows;
    if (!cx.ex.wn_frames || cx.ex.wn_max_frames <= 0 || N < geo.min_rows)
        return fail(MBX_ERR_INVALID_ARGUMENT, "layer_rows needs wn_frames, wn_max_frames and at least min_rows rows");
    const long long E = (long long)(cx.ex.wn_begin + cx.ex.wn_max_frames) * spf;
    if (E > cx.nsteps || E - N - geo.reach_rows != (long long)cx.ex.wn_begin * spf)
        return fail(MBX_ERR_INVALID_ARGUMENT, "layer_rows: wn_begin must be the frame of the first new sub-band row");
    for (int l = 0; l < L; ++l) {
        const long long s = E - N - geo.reach_rows + geo.c[l], e = s + N;
        const int align = l == 0 ? cond_up : 2 * c.wn_dilations[l];      // Winograd F(2,3) pairs rows t, t+d in blocks of 2d
        const long long A = ((s - geo.r[l]) / align) * align;
        if (s - geo.r[l] < 0) return fail(MBX_ERR_INVALID_ARGUMENT, "layer_rows: the window does not reach far enough back");
        const int phase = (int)(A % cond_up);
        // rows of the launch: up to the layer's reach behind the last new row, and far enough that the conditioning
        // row behind the last new row is not the item's last one (which is where the interpolation clamps)
        const long long n1 = e + geo.ahead[l] - A;
        const long long n2 = (long long)cond_up * ((e - 1 - A + phase) / cond_up + 2) - phase;
        const long long need = std::max(n1, n2);
        if (A + need > cx.nsteps) return fail(MBX_ERR_INVALID_ARGUMENT, "layer_rows: the region ends too close to the window end");
        // only the rows [s, e) are consumed (res_sp): the gate kernel computes the aligned blocks of output pairs that hold them
        const long long o0 = ((s - A) / align) * align;
        cx.gate_sp[l] = Span{A, nullptr, 1, (int)need, phase, (int)o0, (int)(e - A - o0)};
        cx.res_sp[l] = Span{s, nullptr, 1, N, 0, 0, 0};
    }
    cx.tail_sp = cx.res_sp[L - 1];
    return MBX_OK;
}

// ---- optional RMS normalisation of the mel input (reference wavegen_1d.py:493-495, 638-769); the matching gain
// is multiplied onto the audio at the end (reference wavegen_1d.py:506-507)
mbx_status run_norm_mel(ForwardCtx &cx) {
    mbx_handle *hd = cx.hd;
    const mbx_config &c = cx.c;
    const Workspace &w = cx.w;
    if (c.nm_iters > 0) {
        // (streaming windows: the smoothing treats the window edges as item edges, so the frames within the smoothing's
        // reach of a window edge differ from the whole-utterance run -- the caller's margins cover that reach,
        // streaming.py::norm_reach)
        ScopedEvents ev(hd, PROF_NORM_MEL, cx.stream);
        cx.nm_gain_src = mbx::launch_norm_mel(norm_mel_consts(hd), cx.mel, (long long)cx.T * c.mel_channels, cx.n_frames, cx.T, cx.B,
                                              w.nm_a, w.nm_b, w.mel_norm, cx.stream);
        cx.mel = w.mel_norm;
    }
    // the float64 F0 chain reads the mel rows as 16-byte pieces: a caller's mel that starts in the middle of one (a view
    // into a larger buffer) is copied into the workspace first, so that the same handle and the same mel give the same
    // bits however the call was made
    if (hd->f0_full64 && c.nm_iters == 0 && (reinterpret_cast<uintptr_t>(cx.mel) & 15) != 0 && c.mel_channels % 4 == 0) {
        if (hipMemcpyAsync(w.mel_norm, cx.mel, (size_t)cx.B * cx.T * c.mel_channels * sizeof(float), hipMemcpyDeviceToDevice, cx.stream) != hipSuccess)
            return fail(MBX_ERR_HIP, "hipMemcpyAsync of a misaligned mel failed");
        cx.mel = w.mel_norm;
    }
    return MBX_OK;
}

// ---- formant shift (no counterpart in the reference): the chains that describe the spectral envelope
// read the mel rows warped along the frequency axis, the F0 chain keeps cx.mel
void run_envelope(ForwardCtx &cx) {
    cx.mel_env = cx.mel;
    if (!cx.ex.env_factor) return;
    ScopedEvents ev(cx.hd, PROF_FRONTEND, cx.stream);
    mbx::launch_envelope(envelope_args(cx), cx.stream);
    cx.mel_env = cx.ex.env_mel;
}

// ---- conditioning conv (reference custom_AE_layers.py:214-227,287), VTF-net -> cepstrum (reference
// custom_pulsed_generator.py:793-800) and F0-net (reference :773-791) are independent chains on the mel input:
// the n-th convolution of each goes into one launch (launch_conv1d_group; matters at small batch, where the
// mel-rate convolutions are latency-bound).  Then the extra blocks' conditioning chains, the external F0 contour or the
// transposition, the front end's ring, and behind it the per-frame pitch control (f0_control_kernel).
mbx_status run_frontend(ForwardCtx &cx) {
    mbx_handle *hd = cx.hd;
    const mbx_config &c = cx.c;
    const Workspace &w = cx.w;
    const ForwardExtras &ex = cx.ex;
    const int B = cx.B, T = cx.T, fe_frames = cx.fe_frames, fe_end = cx.fe_end, cond_cout = cx.cond_cout;
    const long long npulse = cx.npulse;
    const float *mel = cx.mel, *f0_in = ex.f0_in;
    // per-frame pitch control: every item takes its contour from f0_frames (no mask) = the F0-net does not run
    const bool no_f0_net = ex.f0_frames && !ex.f0_item_mask;
    hipStream_t stream = cx.stream;
    {
        ScopedEvents ev(hd, PROF_FRONTEND, stream);
        // a carried front end computes the frames [fe_end - fe_frames, fe_end) of every item only (all items then have
        // fe_end frames: a steady tick); batch strides stay those of the window
        const int Tf = fe_frames ? fe_frames : T;
        const long long f_off = fe_frames ? fe_end - Tf : 0;
        const int32_t *nf_fe = fe_frames ? nullptr : cx.n_frames;
        const float *mel_fe = mel + f_off * c.mel_channels;                 // the F0 chain's rows
        const float *env_fe = cx.mel_env + f_off * c.mel_channels;          // the VTF and conditioning chains' rows
        SubnetRun cond(hd, hd->cond_ops.data(), hd->wn[0].cond.data(), (int)hd->cond_ops.size(), env_fe, c.mel_channels, nf_fe, B, Tf,
                       w.sub4, w.sub5, w.cond + f_off * cond_cout, false, 1.f, 0.f, stream);
        if (hd->cond_ops.empty()) {   // disable_conditioning: cond_layers = zeros (reference custom_AE_layers.py:293-294)
            cond.finished = true;
            if (hipMemsetAsync(w.cond, 0, (size_t)B * T * cond_cout * sizeof(float), stream) != hipSuccess)
                return fail(MBX_ERR_HIP, "hipMemsetAsync of the conditioning rows failed");
        }
        SubnetRun vtf(hd, c.vtf_ops, hd->tab.vtf.data(), c.n_vtf_ops, env_fe, c.mel_channels, nf_fe, B, Tf, w.sub2, w.sub3,
                      w.ceps + f_off * c.n_ceps, false, 1.f, 0.f, stream);
        const bool f0_wide = hd->f0_time_factor > c.pulse_per_frame;
        SubnetRun f0(hd, c.f0_ops, hd->tab.f0.data(), c.n_f0_ops, mel_fe, c.mel_channels, nf_fe, B, Tf, w.sub0, w.sub1,
                     f0_wide ? w.f0_wide : w.f0 + f_off * c.pulse_per_frame, true, c.f0_max - c.f0_min, c.f0_min, stream);
        f0.precise = c.f0_accumulate == MBX_F0_ACC_F64;
        // (a misaligned mel was copied into the workspace by run_norm_mel; mel_channels % 4 != 0 keeps the float32 hidden layers)
        if (hd->f0_full64 && (reinterpret_cast<uintptr_t>(mel_fe) & 15) == 0 && c.mel_channels % 4 == 0) {
            f0.buf64_0 = w.f0h0;
            f0.buf64_1 = w.f0h1;
        }
        if (c.ps_off) vtf.finished = true;             // no VTF-net (the cepstrum buffer stays unused)
        if (fe_frames) {
            vtf.window_stride(T, c.mel_channels);
            f0.window_stride(T, c.mel_channels);
            cond.window_stride(T, c.mel_channels);
        }
        if (f0_in || no_f0_net) f0.finished = true;
        for (;;) {
            mbx::ConvArgs group[3];
            int n = 0;
            if (f0.next_conv(group[n])) ++n;
            if (vtf.next_conv(group[n])) ++n;
            if (cond.next_conv(group[n])) ++n;
            if (!n) break;
            mbx::launch_conv1d_group(group, n, stream);
        }
        if (vtf.status != MBX_OK) return vtf.status;
        if (f0.status != MBX_OK) return f0.status;
        if (cond.status != MBX_OK) return cond.status;
        // the conditioning chains of the WaveNet blocks behind the first one (each block has its own layer)
        for (size_t bk = 1; bk < hd->blocks.size(); ++bk) {
            const auto &blk = hd->blocks[bk];
            const size_t floats = (size_t)B * T * blk.ccu * 2 * blk.C;
            if (blk.cond_ops.empty()) {
                if (hipMemsetAsync(w.mb_cond[bk], 0, floats * sizeof(float), stream) != hipSuccess)
                    return fail(MBX_ERR_HIP, "hipMemsetAsync of the conditioning rows failed");
                continue;
            }
            SubnetRun cb(hd, blk.cond_ops.data(), hd->wn[bk].cond.data(), (int)blk.cond_ops.size(), cx.mel_env, c.mel_channels, cx.n_frames, B, T,
                         w.sub4, w.sub5, w.mb_cond[bk], false, 1.f, 0.f, stream);
            mbx::ConvArgs one;
            while (cb.next_conv(one)) mbx::launch_conv1d_group(&one, 1, stream);
            if (cb.status != MBX_OK) return cb.status;
        }
        if (f0_wide && !f0_in && !no_f0_net)   // pulse_frequency[:, :T * pulse_per_frame] (reference custom_pulsed_generator.py:787)
            mbx::launch_activation(w.f0_wide, (long long)T * hd->f0_time_factor, cx.n_frames, c.pulse_per_frame, (int)npulse,
                                   B, 1, MBX_ACT_LINEAR, 1.f, 0.f, w.f0, npulse, stream);
    }
    if (f0_in)   // externally supplied contour (reference wavegen_1d.py:546-550)
        mbx::launch_activation(f0_in, npulse, cx.n_frames, c.pulse_per_frame, (int)npulse, B, 1, MBX_ACT_LINEAR, ex.transposition,
                               0.f, w.f0, npulse, stream);
    else if (ex.transposition != 1.f)
        mbx::launch_activation(w.f0, npulse, cx.n_frames, c.pulse_per_frame, (int)npulse, B, 1, MBX_ACT_LINEAR,
                               ex.transposition, 0.f, w.f0, npulse, stream);
    if (ex.fe_store) {
        // frames in front of the new ones come from the ring (they were computed, exactly, by earlier ticks); the new
        // ones (fe_new_frames == 0: the whole window) go there for the ticks to come
        ScopedEvents ev(hd, PROF_FRONTEND, stream);
        mbx::FrontendCarryArgs fc{};
        fc.cond = w.cond;
        fc.ceps = w.ceps;
        fc.f0 = w.f0;
        fc.cond_floats = cond_cout;
        fc.ceps_floats = c.n_ceps;
        fc.f0_floats = c.pulse_per_frame;
        fc.frames = T;
        fc.n_frames = cx.n_frames;
        fc.store = ex.fe_store;
        fc.ring_frames = ex.fe_ring_frames;
        fc.pos = ex.fe_pos;
        fc.slot_desc = ex.sub_carry;
        fc.first_new = fe_frames ? fe_end - ex.fe_new_frames : 0;
        fc.skip_f0 = no_f0_net ? 1 : 0;
        mbx::launch_frontend_carry(fc, B, stream);
    }
    if (ex.f0_frames || ex.f0_scale) {
        // per-frame pitch control, in place and behind the ring: the ring keeps the F0-net's own contour, and the control
        // rows of the whole window are applied in every call, so a frame's ring entry never depends on a control value
        auto it = hd->lerp.find(c.pulse_per_frame);
        if (it == hd->lerp.end()) return fail(MBX_ERR_INVALID_ARGUMENT, "interpolation table missing (pulse_per_frame)");
        ScopedEvents ev(hd, PROF_FRONTEND, stream);
        mbx::launch_f0_control(ex.f0_frames, ex.f0_scale, ex.f0_item_mask, cx.n_frames, T, B, c.pulse_per_frame, it->second.first,
                               it->second.second, w.f0, stream);
    }
    return MBX_OK;
}

// ---- wavetable excitation (reference custom_pulsed_generator.py:889), and the PQMF analysis of the pulse signal instead of
// folding consecutive samples (reference :892-895)
void run_excitation(ForwardCtx &cx) {
    mbx_handle *hd = cx.hd;
    const mbx_config &c = cx.c;
    const Workspace &w = cx.w;
    {
        ScopedEvents ev(hd, PROF_WAVETABLE, cx.stream);
        mbx::launch_wavetable(wavetable_consts(hd), w.f0, cx.npulse, cx.n_frames, c.pulse_per_frame, (int)cx.npulse, cx.B, w.pulse,
                              nullptr, w.cum, w.chunk_last, cx.ex.st_in, cx.ex.st_out, cx.stream);
    }
    cx.pulse_wn = w.pulse;
    if (c.pulse_pqmf_taps > 0) {
        ScopedEvents ev(hd, PROF_WAVETABLE, cx.stream);
        mbx::launch_pulse_analysis(w.pulse, cx.npulse, cx.n_frames, c.pulse_per_frame, (int)cx.npulse, cx.B, hd->tab.pulse_ana->ptr,
                                   c.pulse_pqmf_taps, c.pulse_channels, w.pulse_ana, cx.stream);
        cx.pulse_wn = w.pulse_ana;               // what the WaveNet reads; the stage "pulse" stays the oscillator's output
    }
}

// The launch geometry the single block's plan is made from (wn_plan.h): the spans of plan_layer_spans and the kind of call
mbx::WnGeometry wn_geometry(const ForwardCtx &cx) {
    mbx::WnGeometry geo;
    geo.B = cx.B;
    geo.nsteps = cx.nsteps;
    geo.cond_bstride = (long long)cx.T * cx.cond_cout;
    geo.streamed = cx.streamed();
    geo.active = cx.ex.active_frames != nullptr;
    geo.layer_state = cx.ex.lay != nullptr;
    for (int l = 0; l < cx.c.wn_layers; ++l) {
        geo.gate[l] = wn_span(cx.gate_sp[l]);
        geo.res_rows[l] = cx.res_sp[l].max_rows;
    }
    return geo;
}

// Layer l of block b of the block runner, whole items of T frames: F(4,3) in the 256-row shape at every size where the
// host supplied the block's weight image and the layer fits (SAME padding, k = 3, power-of-two dilation), the direct form
// otherwise; the packed res/skip kernel or the generic one
struct BlockLayerPlan { mbx::GateChoice gate; int resskip; };
BlockLayerPlan plan_block_layer(const mbx_handle *hd, size_t b, int l, int B, int T) {
    const auto &blk = hd->blocks[b];
    const int C = blk.C, L = hd->cfg.wn_layers;
    const long long rows = (long long)T * blk.spf;
    const unsigned img = layer_images(hd->wn[b].layer[l]);
    const mbx::ConvArgs g = mbx::wn_gate_dims(hd->pol, C, hd->cfg.wn_dilations[l], rows * C, mbx::WnSpan{(int)rows, 0, 0, 0}, B,
                                              (long long)T * blk.ccu * 2 * C);
    BlockLayerPlan lp;
    lp.gate = mbx::wn_plan_gate(hd->pol, img, g, (long long)T * hd->cfg.steps_per_frame, false, true, false, nullptr);
    bool planes;
    lp.resskip = mbx::wn_plan_resskip(hd->pol, img, mbx::wn_resskip_dims(C, l == 0, l == L - 1, rows * C, (int)rows, B),
                                      (long long)T * hd->cfg.steps_per_frame, false, false, false, &planes);
    return lp;
}

// The report of a model with several blocks (mbx_conv_form_info.gate_kernel, mbx_kernel_report_info): block-major, entry
// b * L + l, as many as MBX_MAX_WN_LAYERS holds; every block's end convolution and the post-net are generic convolutions
mbx::WnPlan plan_blocks(const mbx_handle *hd, int B, int T) {
    mbx::WnPlan plan;
    const int L = hd->cfg.wn_layers;
    plan.n_layers = std::min<int>((int)hd->blocks.size() * L, MBX_MAX_WN_LAYERS);
    for (int slot = 0; slot < plan.n_layers; ++slot) {
        const BlockLayerPlan lp = plan_block_layer(hd, slot / L, slot % L, B, T);
        plan.gate[slot] = lp.gate;
        plan.gate_f32[slot] = lp.gate.kernel;
        plan.resskip[slot] = lp.resskip;
    }
    plan.tail = MBX_TAIL_K_UNFUSED;
    return plan;
}

// Gate of one layer (dilated convolution + conditioning + gate) with the kernel the plan chose.  carry: the layer's stream
// state moves first (null: none)
mbx_status run_gate_layer(ForwardCtx &cx, const mbx::ConvArgs &g, const WnLayerTensors &t, const mbx::GateChoice &k,
                          const mbx::LayerCarryArgs *carry) {
    mbx_handle *hd = cx.hd;
    hipStream_t stream = cx.stream;
    ScopedEvents ev(hd, PROF_GATE, stream);
    if (carry) mbx::launch_layer_carry(*carry, g.batch, stream);
    mbx::ConvArgs a = g;
    const char *err = nullptr;
    switch (k.kernel) {
    case MBX_GATE_K_SPLIT_F16:
    case MBX_GATE_K_SPLIT_F16_WIDE:                 // the res/skip layer in front left h as fp16 planes
        a.h_split = cx.w.h16;
        mbx::wn_planes_dims(a, g.channels, cx.nsteps);
        [[fallthrough]];
    case MBX_GATE_K_SPLIT_F16_F32H:
        a.w = t.gate_f16->ptr;
        err = mbx::launch_wn_gate_f16(a, k.kernel, stream);
        break;
    case MBX_GATE_K_F43:
    case MBX_GATE_K_F43_PSPLIT:
    case MBX_GATE_K_F43_HSPLIT:
    case MBX_GATE_K_F43_STRIDED:
    case MBX_GATE_K_F43_STRIDED_PSPLIT:
        a.w = t.wino4w->ptr;
        err = mbx::launch_wn_gate_winograd4w(a, k, stream);
        break;
    case MBX_GATE_K_F23:
        a.w = t.wino2w->ptr;
        err = mbx::launch_wn_gate_winograd2w(a, stream);
        break;
    case MBX_GATE_K_DIRECT:
        mbx::launch_conv1d(g, mbx::EPI_GATE, stream);
        break;
    default:
        err = "gate layer without a planned kernel";
    }
    return err ? fail(MBX_ERR_INVALID_ARGUMENT, err) : MBX_OK;
}

// res/skip of one layer with the kernel the plan chose (folded layers: im is the layer's image set, rows of C + 16 channels
// under ext; layers with a skip tensor: im null, r.w the plain weights).  planes_out: a split launch also writes h as fp16 planes
mbx_status run_resskip_layer(ForwardCtx &cx, const mbx::ConvArgs &r, const WnLayerTensors &t, const FoldImages *im, bool ext,
                             int kernel, bool planes_out) {
    mbx_handle *hd = cx.hd;
    hipStream_t stream = cx.stream;
    ScopedEvents ev(hd, (hd->pol.split_f16 && (!ext || im->f16)) ? PROF_RES_SKIP_F16 : PROF_RES_SKIP, stream);
    mbx::ConvArgs a = r;
    const char *err = nullptr;
    switch (kernel) {
    case MBX_RESSKIP_K_SPLIT_F16:
        a.w = im->f16->ptr;
        a.gate_act = cx.c.wn_gate_activation;
        if (planes_out) {                           // the next layer's gate reads the new hidden state as fp16 planes
            a.h_split = cx.w.h16;
            mbx::wn_planes_dims(a, r.channels, cx.nsteps);
            a.h_planes_only = cx.plan.planes_only ? 1 : 0;
        }
        err = mbx::launch_wn_resskip_f16(a, stream);
        break;
    case MBX_RESSKIP_K_WIDE11_RES10:
    case MBX_RESSKIP_K_WIDE11:
    case MBX_RESSKIP_K_WIDE6X2:
        a.w = im->wide->ptr;
        err = mbx::launch_wn_resskip_wide(a, kernel, stream);
        break;
    case MBX_RESSKIP_K_WAVE11:
    case MBX_RESSKIP_K_WAVE12:
    case MBX_RESSKIP_K_WAVE6X2:
    case MBX_RESSKIP_K_WAVE4X3:
        a.w = im->wave->ptr;
        a.tune_split = hd->pol.resskip_split;
        err = mbx::launch_wn_resskip_wave(a, kernel, stream);
        break;
    case MBX_RESSKIP_K_PACKED64:
    case MBX_RESSKIP_K_PACKED128:                   // host-packed weights (folded layers: the image r was built with)
        a.w = (im ? im->fold : t.packed)->ptr;
        err = mbx::launch_wn_resskip(a, kernel, stream);
        break;
    case MBX_RESSKIP_K_CONV1D:
        mbx::launch_conv1d(r, mbx::EPI_RESSKIP, stream);
        break;
    default:
        err = "res/skip layer without a planned kernel";
    }
    return err ? fail(MBX_ERR_INVALID_ARGUMENT, err) : MBX_OK;
}

// End of the single block: the last layer's share of the folded skip path, or the end convolution on the skip tensor; then
// the post-net 1x1 into the sub-band rows (one kernel where the plan found the images and the shapes fit)
mbx_status run_tail(ForwardCtx &cx) {
    mbx_handle *hd = cx.hd;
    const mbx_config &c = cx.c;
    const Workspace &w = cx.w;
    const WnBlockTensors &bt = hd->wn[0];
    const int B = cx.B, C = c.wn_channels, L = c.wn_layers, M = c.subbands, n_out = c.wn_out_channels;
    const long long nsteps = cx.nsteps;
    hipStream_t stream = cx.stream;
    ScopedEvents ev(hd, PROF_TAIL, stream);
    const DevTensor *wpn = hd->tab.post_w, *bpn = hd->tab.post_b, *be = bt.end_b;
    const Span &ts = cx.tail_sp;
    float *acc_t = w.wn_out + ts.row0 * n_out, *sub_t = w.sub + ts.row0 * M, *skip_t = w.skip + ts.row0 * C;
    const char *err = nullptr;
    if (cx.plan.tail == MBX_TAIL_K_UNFUSED) {
        mbx::ConvArgs a = conv_args(skip_t, nsteps * C, C, ts.nf, ts.rpf, ts.max_rows, B, bt.end_w, be, 1, C,
                                    n_out, 1, 0, MBX_PAD_ZERO, acc_t, nsteps * n_out, n_out);
        mbx::launch_conv1d(a, mbx::EPI_LINEAR, stream);
        // post-net 1x1 (reference custom_pulsed_generator.py:490-493,913-914)
        mbx::ConvArgs pn = conv_args(acc_t, nsteps * n_out, n_out, ts.nf, ts.rpf, ts.max_rows, B, wpn, bpn, 1, n_out, M, 1, 0,
                                     MBX_PAD_ZERO, sub_t, nsteps * M, M);
        mbx::launch_conv1d(pn, mbx::EPI_LINEAR, stream);
    } else if (hd->pol.fold_skip) {
        err = mbx::launch_wn_tail(cx.plan.tail, w.a + ts.row0 * C, nsteps * C, ts.nf, ts.rpf, ts.max_rows, B, C, bt.tail_fold->ptr,
                                  bt.tail_fold_b->ptr, n_out, wpn->ptr, bpn ? bpn->ptr : nullptr, M, L > 1 ? acc_t : nullptr,
                                  acc_t, nsteps * n_out, sub_t, nsteps * M, stream);
    } else {
        err = mbx::launch_wn_tail(cx.plan.tail, skip_t, nsteps * C, ts.nf, ts.rpf, ts.max_rows, B, C, bt.end_packed->ptr,
                                  be ? be->ptr : nullptr, n_out, wpn->ptr, bpn ? bpn->ptr : nullptr, M, nullptr,
                                  acc_t, nsteps * n_out, sub_t, nsteps * M, stream);
    }
    return err ? fail(MBX_ERR_INVALID_ARGUMENT, err) : MBX_OK;
}

// ---- WaveNet (reference custom_AE_layers.py:273-346), one block: the measured path.  Which kernel runs every layer was
// planned in check_forward_args (cx.plan); this only builds the arguments and launches.
mbx_status run_wavenet(ForwardCtx &cx) {
    mbx_handle *hd = cx.hd;
    const mbx_config &c = cx.c;
    const Workspace &w = cx.w;
    const WnBlockTensors &bt = hd->wn[0];
    const mbx::WnPlan &plan = cx.plan;
    const bool fold_start = hd->pol.fold_start, fold = hd->pol.fold_skip;
    const int B = cx.B, C = c.wn_channels, L = c.wn_layers;
    const long long nsteps = cx.nsteps;
    hipStream_t stream = cx.stream;
    hd->last_plan = plan;
    if (!fold_start) {
        ScopedEvents ev(hd, PROF_START, stream);
        const Span &sp = cx.gate_sp[0];                       // (the region: a handle that carries layer state folds the start)
        const int nsub1 = 1 + c.wt_subharm_channels;              // floats per excitation sample (pulse + sub-harmonic sinusoids)
        const int ppr = c.pulse_per_frame / c.steps_per_frame * nsub1;           // excitation floats per WaveNet row
        mbx::launch_wn_start(cx.pulse_wn + sp.row0 * ppr, cx.npulse * nsub1, c.noise_sigma != 0.f ? cx.noise + sp.row0 : nullptr, nsteps, c.noise_sigma,
                             sp.nf, sp.rpf, sp.max_rows, B, c.pulse_channels * nsub1, bt.start_w->ptr,
                             bt.start_b->ptr, C, w.h + sp.row0 * C, nsteps * C, stream);
    }
    for (int l = 0; l < L; ++l) {
        const WnLayerTensors &t = bt.layer[l];
        const Span &gs = cx.gate_sp[l], &rs = cx.res_sp[l];
        const mbx::ConvArgs g = gate_args(hd, t, C, c.wn_dilations[l], w.h, w.a, nsteps * C, gs, B, w.cond, (long long)cx.T * cx.cond_cout);
        mbx_status st = MBX_OK;
        if (plan.gate[l].kernel == MBX_GATE_K_FOLDED_START) {
            // start convolution folded into the layer: a K = 24 contraction of the excitation (wn_gate0.hip)
            ScopedEvents ev(hd, PROF_GATE0, stream);
            if (const char *err = mbx::launch_wn_gate0(gate0_args(cx, g, t, gs.row0), stream)) st = fail(MBX_ERR_INVALID_ARGUMENT, err);
        } else {
            const bool carry = cx.carry_layers && l >= 1;
            const mbx::LayerCarryArgs lc = carry ? layer_carry_args(cx, l) : mbx::LayerCarryArgs{};
            st = run_gate_layer(cx, g, t, plan.gate[l], carry ? &lc : nullptr);
        }
        if (st != MBX_OK) return st;
        if (!fold)
            st = run_resskip_layer(cx, resskip_args(hd, t, C, l, w.a, w.h, w.skip, nsteps * C, rs, B), t, nullptr, false, plan.resskip[l], false);
        else if (l < L - 1)                                   // (the tail kernel adds the last layer's share)
            st = run_resskip_layer(cx, resskip_fold_args(cx, t, l, l == 0 && fold_start, rs), t, &t.run, l == 0 && fold_start, plan.resskip[l],
                                   plan.planes_out[l]);
        if (st != MBX_OK) return st;
    }
    return run_tail(cx);
}

// Several WaveNet blocks with in-block upsampling (reference custom_pulsed_generator.py:456-488, 908-914;
// custom_AE_layers.py:273-346, 574-582), on the generic kernels: block b = start convolution (block 0: fold + noise
// channel + start, wn_start_kernel) -> L x (dilated convolution + conditioning + gate, res/skip) -> end convolution ->
// sub-pixel convolution "up<b>" (depth -> time).  The last block's output goes through the post-net into the sub-band
// rows.  Whole items only (no stream regions).
mbx_status run_wavenet_blocks(ForwardCtx &cx) {
    mbx_handle *hd = cx.hd;
    const mbx_config &c = cx.c;
    const Workspace &w = cx.w;
    const int B = cx.B, T = cx.T;
    const int32_t *n_frames = cx.n_frames;
    hipStream_t stream = cx.stream;
    const int L = c.wn_layers, n_out = c.wn_out_channels, M = c.subbands;
    const int nsub1 = 1 + c.wt_subharm_channels;
    const float *x_in = nullptr;                 // output of the previous block (B, rows, n_out)
    hd->last_plan = cx.plan;                     // (plan_blocks: the report of as many layers as MBX_MAX_WN_LAYERS holds)
    for (size_t b = 0; b < hd->blocks.size(); ++b) {
        const auto &blk = hd->blocks[b];
        const WnBlockTensors &bt = hd->wn[b];
        const int C = blk.C, spf = blk.spf;
        const long long rows = (long long)T * spf;
        const Span sp{0, n_frames, spf, (int)rows, 0, 0, 0};
        const bool last_block = b + 1 == hd->blocks.size();
        const float *cond = b == 0 ? w.cond : w.mb_cond[b];
        if (b == 0) {
            ScopedEvents ev(hd, PROF_START, stream);
            mbx::launch_wn_start(cx.pulse_wn, cx.npulse * nsub1, c.noise_sigma != 0.f ? cx.noise : nullptr, rows, c.noise_sigma, n_frames, spf,
                                 (int)rows, B, c.pulse_channels * nsub1, bt.start_w->ptr, bt.start_b->ptr, C, w.mb_h, rows * C, stream);
        } else {
            mbx::ConvArgs a = conv_args(x_in, rows * n_out, n_out, n_frames, spf, (int)rows, B, bt.start_w, bt.start_b, 1, n_out, C, 1, 0,
                                        MBX_PAD_ZERO, w.mb_h, rows * C, C);
            mbx::launch_conv1d(a, mbx::EPI_LINEAR, stream);
        }
        for (int l = 0; l < L; ++l) {
            const WnLayerTensors &t = bt.layer[l];
            const BlockLayerPlan lp = plan_block_layer(hd, b, l, B, T);
            const mbx::ConvArgs g = gate_args(hd, t, C, c.wn_dilations[l], w.mb_h, w.mb_a, rows * C, sp, B, cond, (long long)T * blk.ccu * 2 * C);
            mbx_status st = run_gate_layer(cx, g, t, lp.gate, nullptr);
            if (st != MBX_OK) return st;
            st = run_resskip_layer(cx, resskip_args(hd, t, C, l, w.mb_a, w.mb_h, w.mb_skip, rows * C, sp, B), t, nullptr, false, lp.resskip, false);
            if (st != MBX_OK) return st;
        }
        // end convolution (reference custom_AE_layers.py:337-340); the last block's output is the stage "wn_out" unless an
        // up-sampling convolution follows it
        ScopedEvents ev(hd, PROF_TAIL, stream);
        float *y = (last_block && blk.ups == 1) ? w.wn_out : w.mb_y0;
        mbx::ConvArgs e = conv_args(w.mb_skip, rows * C, C, n_frames, spf, (int)rows, B, bt.end_w, bt.end_b, 1, C, n_out, 1, 0,
                                    MBX_PAD_ZERO, y, rows * n_out, n_out);
        mbx::launch_conv1d(e, mbx::EPI_LINEAR, stream);
        x_in = y;
        if (blk.ups > 1) {
            // Conv1DUpDownSample (reference conv_layers.py:177-261): k = 3 convolution to n_out * ups channels, zero SAME
            // padding, then depth -> time: row r of the input becomes rows ups r .. ups r + ups - 1 (a reshape in memory)
            float *yu = last_block ? w.wn_out : w.mb_y1;
            mbx::ConvArgs u = conv_args(y, rows * n_out, n_out, n_frames, spf, (int)rows, B, bt.up_w, bt.up_b, 3,
                                        n_out, n_out * blk.ups, 1, c.wn_causal ? 2 : 1, MBX_PAD_ZERO, yu, rows * n_out * blk.ups, n_out * blk.ups);
            mbx::launch_conv1d(u, mbx::EPI_LINEAR, stream);
            x_in = yu;
        }
    }
    // post-net 1x1 (reference custom_pulsed_generator.py:490-493,913-914) at the sub-band rate
    mbx::ConvArgs pn = conv_args(x_in, cx.nsteps * n_out, n_out, n_frames, c.steps_per_frame, (int)cx.nsteps, B, hd->tab.post_w,
                                 hd->tab.post_b, 1, n_out, M, 1, 0, MBX_PAD_ZERO, w.sub, cx.nsteps * M, M);
    mbx::launch_conv1d(pn, mbx::EPI_LINEAR, stream);
    return MBX_OK;
}

// Behind the WaveNet: sub-band gains, the sub-band rows a stream carries, PQMF synthesis (or the reshape), the STFT-domain
// filter with overlap-add (or the plain copy), the gain of the RMS normalisation.  These stages see the active region
// (which contains the WaveNet's) as the item.
mbx_status run_backend(ForwardCtx &cx) {
    mbx_handle *hd = cx.hd;
    const mbx_config &c = cx.c;
    const Workspace &w = cx.w;
    const ForwardExtras &ex = cx.ex;
    const int B = cx.B, T = cx.T, M = c.subbands, act_frames_max = cx.act_frames_max;
    const long long nsteps = cx.nsteps, act0 = cx.act0;
    const int32_t *n_frames_act = cx.n_frames_act;
    hipStream_t stream = cx.stream;
    // ---- sub-band gains instead of the STFT-domain filter (ps_use_stft: false; reference :857-884, 670, 916-917)
    if (c.ps_subband_gain) {
        auto lh = hd->lerp[c.hop_size];
        mbx::launch_subband_gain(w.sub, nsteps * M, w.ceps, (long long)T * c.n_ceps, cx.n_frames, T, c.steps_per_frame, B, M, c.hop_size,
                                 lh.first, lh.second, c.spect_preserve_energy, stream);
    }
    // ---- sub-band rows carried between the ticks of a stream: rows in front of the WaveNet region come from the
    // caller's store (computed by the previous tick), the rows the next tick will need go there
    if (ex.sub_carry) {
        mbx::launch_sub_carry(w.sub, nsteps * M, ex.sub_store, (long long)ex.sub_store_rows * M, ex.sub_carry, B, ex.sub_store_rows,
                              M, 0, stream);
        mbx::launch_sub_carry(w.sub, nsteps * M, ex.sub_store, (long long)ex.sub_store_rows * M, ex.sub_carry, B, ex.sub_store_rows,
                              M, 1, stream);
    }
    float *sub_act = w.sub + act0 * c.steps_per_frame * M;
    float *exc_act = w.exc + act0 * c.hop_size;
    float *ceps_act = w.ceps + act0 * c.n_ceps;
    float *f0_act = w.f0 + act0 * c.pulse_per_frame;
    int *cidx_act = w.ceps_index + act0;
    float *frames_act = w.frames + act0 * c.stft_win;
    float *audio_act = cx.audio + act0 * c.hop_size;
    // ---- PQMF synthesis (reference :920-921)
    {
        ScopedEvents ev(hd, PROF_PQMF, stream);
        if (c.no_pqmf)   // pp_mod_subnet_use_pqmf: false -- source_signal = reshape(x, (B, rows * M)) (reference :922-923)
            mbx::launch_activation(sub_act, nsteps * M, n_frames_act, c.hop_size, act_frames_max * c.hop_size, B, 1, MBX_ACT_LINEAR,
                                   1.f, 0.f, exc_act, (long long)T * c.hop_size, stream);
        else
            mbx::launch_pqmf(sub_act, nsteps * M, n_frames_act, c.steps_per_frame, act_frames_max * c.steps_per_frame, B, M, hd->poly, hd->poly_t, hd->poly_ndm,
                             hd->poly_dm_min, exc_act, (long long)T * c.hop_size, stream);
    }
    if (c.ps_off || c.ps_subband_gain) {
        // ps_off / sub-band gains: signal = generate_excitation(...) (reference :663-672); samples behind an item's own length are zero
        ScopedEvents ev(hd, PROF_OVERLAP_ADD, stream);
        if (hipMemsetAsync(cx.audio, 0, (size_t)B * T * c.hop_size * sizeof(float), stream) != hipSuccess)
            return fail(MBX_ERR_HIP, "hipMemsetAsync of the audio failed");
        mbx::launch_activation(exc_act, (long long)T * c.hop_size, n_frames_act, c.hop_size, act_frames_max * c.hop_size, B, 1,
                               MBX_ACT_LINEAR, 1.f, 0.f, audio_act, (long long)T * c.hop_size, stream);
    } else {
        // ---- STFT-domain filtering with the spectral envelope (reference :681-724, 801-855)
        // (the lifter row of a frame is selected from the F0 contour inside the kernel, reference :507-525)
        const mbx::StftConsts sc = stft_consts(hd);
        {
            ScopedEvents ev(hd, PROF_STFT_FILTER, stream);
            mbx::launch_stft_filter(sc, exc_act, (long long)T * c.hop_size, ceps_act, (long long)T * c.n_ceps, nullptr,
                                    c.n_ceps_windows ? f0_act : nullptr, cx.npulse, c.n_ceps_windows ? cidx_act : nullptr,
                                    n_frames_act, T, B, frames_act, stream);
        }
        {
            ScopedEvents ev(hd, PROF_OVERLAP_ADD, stream);
            mbx::launch_overlap_add(sc, frames_act, n_frames_act, T, T - (int)act0, B, audio_act, (long long)T * c.hop_size, stream);
        }
    }
    if (cx.nm_gain_src) {
        ScopedEvents ev(hd, PROF_NORM_MEL, stream);
        mbx::launch_norm_mel_gain(norm_mel_consts(hd), cx.nm_gain_src, cx.n_frames, T, B, cx.audio, (long long)T * c.hop_size,
                                  false, stream);
    }
    return MBX_OK;
}

// The stage table (mbx_stage): pointers into the whole window of this call's workspace
void publish_stages(ForwardCtx &cx) {
    mbx_handle *hd = cx.hd;
    const mbx_config &c = cx.c;
    const Workspace &w = cx.w;
    const int T = cx.T, C = c.wn_channels, M = c.subbands;
    const long long npulse = cx.npulse, nsteps = cx.nsteps;
    auto &sg = hd->stages;
    if (cx.nm_gain_src) sg["mel_norm"] = {w.mel_norm, (long long)T * c.mel_channels, (long long)T * c.mel_channels};
    else sg.erase("mel_norm");
    if (cx.ex.env_factor) sg["mel_env"] = {cx.ex.env_mel, (long long)T * c.mel_channels, (long long)T * c.mel_channels};
    else sg.erase("mel_env");
    sg["f0"] = {w.f0, npulse, npulse};
    sg["pulse"] = {w.pulse, npulse * (1 + c.wt_subharm_channels), npulse * (1 + c.wt_subharm_channels)};
    sg["cond"] = {w.cond, (long long)T * cx.cond_cout, (long long)T * cx.cond_cout};
    if (cx.plan.planes_only) {
        // split precision with the planes as the hidden state: the float32 tensor was not written; per row [C8 hi halves | C8 lo'
        // halves] = C8 float32 words (engine.py::stage rebuilds hi + 2^-11 lo' from it)
        sg.erase("wn_hidden");
        sg["wn_hidden_planes"] = {w.h16, nsteps * (long long)((C + 7) / 8 * 8), nsteps * (long long)((C + 7) / 8 * 8)};
    } else {
        sg.erase("wn_hidden_planes");
        sg["wn_hidden"] = {w.h, nsteps * C, nsteps * C};
    }
    if (!hd->pol.fold_skip) sg["wn_skip"] = {w.skip, nsteps * C, nsteps * C};
    else sg.erase("wn_skip");
    if (!hd->blocks.empty()) {
        // several blocks (run_wavenet_blocks): the hidden state and the skip sum of the last block, at its own rate
        const auto &lb = hd->blocks.back();
        const long long hc = (long long)T * lb.spf * lb.C;
        sg["wn_hidden"] = {w.mb_h, hc, hc};
        sg["wn_skip"] = {w.mb_skip, hc, hc};
    }
    static const char *const kCondNames[] = {"cond", "cond1", "cond2", "cond3"};
    static_assert(sizeof(kCondNames) / sizeof(kCondNames[0]) == MBX_MAX_WN_BLOCKS, "one stage name per WaveNet block");
    for (int b = 1; b < MBX_MAX_WN_BLOCKS; ++b) {
        // the conditioning rows of block b >= 1, laid out like "cond" (zeros with disable_conditioning)
        if (b < (int)hd->blocks.size()) {
            const long long cc = (long long)T * hd->blocks[b].ccu * 2 * hd->blocks[b].C;
            sg[kCondNames[b]] = {w.mb_cond[b], cc, cc};
        } else {
            sg.erase(kCondNames[b]);
        }
    }
    if (c.pulse_pqmf_taps > 0) sg["pulse_ana"] = {w.pulse_ana, npulse, npulse};
    else sg.erase("pulse_ana");
    sg["wn_out"] = {w.wn_out, nsteps * c.wn_out_channels, nsteps * c.wn_out_channels};
    sg["subbands"] = {w.sub, nsteps * M, nsteps * M};
    sg["excitation"] = {w.exc, (long long)T * c.hop_size, (long long)T * c.hop_size};
    sg["cepstrum"] = {w.ceps, (long long)T * c.n_ceps, (long long)T * c.n_ceps};
    sg["ceps_index"] = {w.ceps_index, (long long)T, (long long)T};
    sg["frames"] = {w.frames, (long long)T * c.stft_win, (long long)T * c.stft_win};
}

}  // namespace

namespace mbx_host {

LayerGeom layer_geom(const mbx_handle *hd) {
    LayerGeom g{};
    const mbx_config &c = hd->cfg;
    const int L = c.wn_layers, C = c.wn_channels;
    // needs the folded graph (no separate start / skip tensors to carry) and the F(2,3) gate kernel (per-layer regions
    // start between conditioning rows: ConvArgs::cond_phase)
    if (!hd->pol.fold_skip || !hd->pol.fold_start || !hd->pol.winograd || c.wn_kernel_size != 3 || L < 2) return g;
    for (int l = 1; l < L; ++l) {
        const int d = c.wn_dilations[l];
        if (!hd->wn[0].layer[l].wino2w || d > 16 || (d & (d - 1)) != 0) return g;
    }
    const bool causal = c.wn_causal != 0;
    for (int l = 0; l < L; ++l) {
        g.r[l] = c.wn_dilations[l] * (c.wn_kernel_size - 1) / (causal ? 1 : 2);
        g.ahead[l] = causal ? 0 : g.r[l];
        g.step[l] = causal ? 0 : (g.r[l] + 1) & ~1;
    }
    g.c[L - 1] = 0;
    for (int l = L - 2; l >= 0; --l) g.c[l] = g.c[l + 1] + g.step[l + 1];
    const int spf = c.steps_per_frame;
    // (+ cond_lin_upsampling - 1: a whole-region run interpolates the conditioning of its last rows towards the clamped
    // last conditioning row; that error spreads backwards through the layers behind, streaming.py::stream_margins --
    // under CAUSAL padding it stays where it is)
    const int spread = causal ? 0 : g.c[0] + g.r[0];
    g.reach_rows = (spread + c.cond_lin_upsampling - 1 + spf - 1) / spf * spf;
    long long off = 0;
    for (int l = 1; l < L; ++l) {
        g.off[l] = off;
        off += (long long)(g.r[l] + g.step[l]) * C + (long long)g.step[l] * c.wn_out_channels;
        g.min_rows = std::max(g.min_rows, g.r[l] + g.step[l]);
    }
    g.floats = (int)off;
    return g;
}

// What a whole-item mbx_forward of (batch, max_frames) would run (mbx_plan): check_forward_args' planning without a workspace
mbx::WnPlan plan_whole_items(const mbx_handle *hd, int batch, int max_frames) {
    if (!hd->blocks.empty()) return plan_blocks(hd, batch, max_frames);
    const mbx_config &c = hd->cfg;
    mbx::WnGeometry geo;
    geo.B = batch;
    geo.nsteps = (long long)max_frames * c.steps_per_frame;
    geo.cond_bstride = (long long)max_frames * 2 * c.wn_channels * c.cond_conv_upsampling;
    for (int l = 0; l < c.wn_layers; ++l) {
        geo.gate[l] = mbx::WnSpan{(int)geo.nsteps, 0, 0, 0};
        geo.res_rows[l] = (int)geo.nsteps;
    }
    return mbx::wn_plan(hd->pol, geo);
}

// One forward pass, in the order of DESIGN.md section 1.  Only enqueues kernels on the caller's stream.
mbx_status forward_impl(mbx_handle *hd, const float *mel, const int32_t *n_frames, int32_t batch, int32_t max_frames,
                        const float *noise, float *audio, void *workspace, size_t workspace_bytes, void *hip_stream,
                        const ForwardExtras &ex) {
    if (!hd || !mel || !audio || !workspace) return fail(MBX_ERR_INVALID_ARGUMENT, "null argument");
    ForwardCtx cx(hd, ex, mel, n_frames, batch, max_frames, noise, audio, hip_stream);
    mbx_status st = check_forward_args(cx, workspace, workspace_bytes);
    if (st == MBX_OK) st = run_norm_mel(cx);
    if (st == MBX_OK) {
        run_envelope(cx);
        st = run_frontend(cx);
    }
    if (st != MBX_OK) return st;
    run_excitation(cx);
    st = hd->blocks.empty() ? run_wavenet(cx) : run_wavenet_blocks(cx);
    if (st == MBX_OK) st = run_backend(cx);
    if (st != MBX_OK) return st;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MBX_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    publish_stages(cx);
    return MBX_OK;
}

}  // namespace mbx_host

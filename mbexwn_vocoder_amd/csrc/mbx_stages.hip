// C ABI of the stages that take no engine handle: mbx_mel_analysis and mbx_encode_flac16 of include/mbexwn.h and the entry
// points of the thirteen headers beside it (mbxa_ resampler, mbxl_ / mbxr_ / mbxo_ live rings, mbxf_ FLAC, mbxn_ noise, mbxw_ mel
// warp, mbxe_warp_envelope, mbxp_ tracker, mbxc_ decoder, mbxt_ streaming tracker, mbxv_ streaming decoder, mbxg_ alignment; mbxe_forward takes a handle and is in
// mbx_api.hip).  Each one copies
// its arguments into the kernel's struct, lets check_* (beside the kernel) refuse them, enqueues on the caller's stream and
// reports the launch error.  A new entry point: prototype in its header, a row in abi.py's TABLE, the body here.
#include "mbx_handle.h"
#include "../../include/mbexwn_audio.h"
#include "../../include/mbexwn_live.h"
#include "../../include/mbexwn_live_resample.h"
#include "../../include/mbexwn_live_out.h"
#include "../../include/mbexwn_flac.h"
#include "../../include/mbexwn_noise.h"
#include "../../include/mbexwn_warp.h"
#include "../../include/mbexwn_pitch.h"
#include "../../include/mbexwn_contour.h"
#include "../../include/mbexwn_envelope.h"
#include "../../include/mbexwn_live_pitch.h"
#include "../../include/mbexwn_live_contour.h"
#include "../../include/mbexwn_align.h"

static_assert(MBXG_MAX_FRAMES == mbx::ALIGN_MAX_FRAMES && MBXG_MAX_BAND == mbx::ALIGN_MAX_BAND && MBXG_MAX_MELS == mbx::ALIGN_MAX_MELS,
              "mbexwn_align.h states the limits of mel_align.hip");
static_assert(MBXN_FILL_TILE == mbx::NOISE_TILE, "mbexwn_noise.h states the tile of noise_keyed.hip");
static_assert(MBXA_RESAMPLE_TILE == mbx::RS_TILE, "mbexwn_audio.h states the tile of resample_poly.hip");

using namespace mbx_host;

// what check_* said, behind the stage's name
static mbx_status refuse(const char *stage, const char *why) {
    return fail(MBX_ERR_INVALID_ARGUMENT, std::string(stage) + ": " + why);
}

extern "C" {

mbx_status mbx_mel_analysis(const float *audio, const int32_t *n_samples, int32_t batch, int32_t max_samples,
                            int32_t win, int32_t hop, int32_t fft_size, int32_t n_mels, const float *window,
                            const float *twiddle, const float *basis, const int32_t *bin_lo, const int32_t *bin_hi,
                            float eps, float *out, int32_t max_frames, void *hip_stream) {
    mbx::MelAnalysisArgs a{};
    a.audio = audio;
    a.audio_bstride = max_samples;
    a.n_samples = n_samples;
    a.max_samples = max_samples;
    a.batch = batch;
    a.win = win;
    a.hop = hop;
    a.fft_size = fft_size;
    a.n_mels = n_mels;
    a.window = window;
    a.twiddle = twiddle;
    a.basis = basis;
    a.bin_lo = bin_lo;
    a.bin_hi = bin_hi;
    a.eps = eps;
    a.out = out;
    a.max_frames = max_frames;
    if (!mbx::launch_mel_analysis(a, static_cast<hipStream_t>(hip_stream)))
        return fail(MBX_ERR_INVALID_ARGUMENT, "mel analysis: sizes do not fit the kernel (fft_size a power of two <= 2048, "
                                              "win <= fft_size, max_samples > win/2, max_frames >= max_samples/hop + 1)");
    return launch_status("kernel launch: ");
}

mbx_status mbxa_resample_poly(const float *audio, const int32_t *n_samples, int32_t batch, int32_t max_samples, int32_t up,
                              int32_t down, const float *taps, int32_t n_taps, float *out, int32_t max_out, void *hip_stream) {
    mbx::ResampleArgs a{};
    a.audio = audio;
    a.n_samples = n_samples;
    a.batch = batch;
    a.max_samples = max_samples;
    a.up = up;
    a.down = down;
    a.taps = taps;
    a.n_taps = n_taps;
    a.out = out;
    a.max_out = max_out;
    if (const char *why = mbx::check_resample_poly(a)) return refuse("resample poly", why);
    mbx::launch_resample_poly(a, static_cast<hipStream_t>(hip_stream));
    return launch_status("kernel launch: ");
}

mbx_status mbxl_ring_append(const float *packed, int64_t packed_samples, const int64_t *desc, int32_t n_streams,
                            int32_t max_count, float *rings, int32_t n_slots, int32_t ring_samples, void *hip_stream) {
    mbx::RingAppendArgs a{};
    a.packed = packed;
    a.packed_samples = packed_samples;
    a.desc = reinterpret_cast<const long long *>(desc);
    a.n_streams = n_streams;
    a.max_count = max_count;
    a.rings = {rings, n_slots, ring_samples};
    if (const char *why = mbx::check_ring_append(a)) return refuse("ring append", why);
    mbx::launch_ring_append(a, static_cast<hipStream_t>(hip_stream));
    return launch_status("kernel launch: ");
}

mbx_status mbxl_mel_frames(const float *rings, int32_t n_slots, int32_t ring_samples, const int64_t *desc, int32_t n_streams,
                           int32_t max_new_frames, int32_t win, int32_t hop, int32_t fft_size, int32_t n_mels,
                           const float *window, const float *twiddle, const float *basis, const int32_t *bin_lo,
                           const int32_t *bin_hi, float eps, float *out, void *hip_stream) {
    mbx::MelStreamArgs a{};
    a.rings = {rings, n_slots, ring_samples};
    a.desc = reinterpret_cast<const long long *>(desc);
    a.n_streams = n_streams;
    a.max_new_frames = max_new_frames;
    a.win = win;
    a.hop = hop;
    a.fft_size = fft_size;
    a.n_mels = n_mels;
    a.window = window;
    a.twiddle = twiddle;
    a.basis = basis;
    a.bin_lo = bin_lo;
    a.bin_hi = bin_hi;
    a.eps = eps;
    a.out = out;
    if (const char *why = mbx::check_mel_stream(a)) return refuse("mel frames", why);
    mbx::launch_mel_stream(a, static_cast<hipStream_t>(hip_stream));
    return launch_status("kernel launch: ");
}

mbx_status mbxr_resample_rings(const float *in_rings, int32_t n_in_slots, int32_t in_ring_samples, const int64_t *desc,
                               int32_t n_rows, int32_t max_new_out, int32_t up, int32_t down, const float *taps, int32_t n_taps,
                               float *out_rings, int32_t n_out_slots, int32_t out_ring_samples, void *hip_stream) {
    mbx::ResampleStreamArgs a{};
    a.in_rings = {in_rings, n_in_slots, in_ring_samples};
    a.desc = reinterpret_cast<const long long *>(desc);
    a.n_rows = n_rows;
    a.max_new_out = max_new_out;
    a.up = up;
    a.down = down;
    a.taps = taps;
    a.n_taps = n_taps;
    a.out_rings = {out_rings, n_out_slots, out_ring_samples};
    if (const char *why = mbx::check_resample_stream(a)) return refuse("resample rings", why);
    mbx::launch_resample_stream(a, static_cast<hipStream_t>(hip_stream));
    return launch_status("kernel launch: ");
}

mbx_status mbxo_resample_emit(const float *in_rings, int32_t n_in_slots, int32_t in_ring_samples, const int64_t *desc,
                              int32_t n_rows, int32_t max_new_out, int32_t up, int32_t down, const float *taps, int32_t n_taps,
                              float *out, int64_t out_floats, void *hip_stream) {
    mbx::ResampleEmitArgs a{};
    a.in_rings = {in_rings, n_in_slots, in_ring_samples};
    a.desc = reinterpret_cast<const long long *>(desc);
    a.n_rows = n_rows;
    a.max_new_out = max_new_out;
    a.up = up;
    a.down = down;
    a.taps = taps;
    a.n_taps = n_taps;
    a.out = out;
    a.out_floats = out_floats;
    if (const char *why = mbx::check_resample_emit(a)) return refuse("resample emit", why);
    mbx::launch_resample_emit(a, static_cast<hipStream_t>(hip_stream));
    return launch_status("kernel launch: ");
}

mbx_status mbx_encode_flac16(const float *audio, int64_t stride, int32_t batch, const int64_t *n_samples, int32_t sample_rate,
                             const uint16_t *crc_tables, uint8_t *out, int64_t out_bytes, float *max_abs, void *hip_stream) {
    if (const char *why = mbx::check_flac_frames(audio, stride, batch, n_samples, sample_rate, crc_tables, out, out_bytes,
                                                 max_abs))
        return refuse("encode flac16", why);
    if (batch == 0) return MBX_OK;
    const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipMemsetAsync(max_abs, 0, (size_t)batch * sizeof(float), stream));
    mbx::launch_flac_frames(audio, stride, batch, n_samples, sample_rate, crc_tables, out, max_abs, stream);
    return launch_status("kernel launch: ");
}

mbx_status mbxf_encode_flac16_fixed(const float *audio, int64_t stride, int32_t batch, const int64_t *n_samples,
                                    int32_t sample_rate, const uint16_t *crc_tables, uint8_t *out, int64_t out_bytes,
                                    int32_t *frame_bytes, int64_t *workspace, int16_t *pcm_out, float *max_abs, void *hip_stream) {
    if (const char *why = mbx::check_flac_fixed(audio, stride, batch, n_samples, sample_rate, crc_tables, out, out_bytes,
                                                frame_bytes, workspace, max_abs))
        return refuse("encode flac16 fixed", why);
    if (batch == 0) return MBX_OK;
    const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipMemsetAsync(max_abs, 0, (size_t)batch * sizeof(float), stream));
    mbx::launch_flac_fixed(audio, stride, batch, n_samples, sample_rate, crc_tables, out, frame_bytes, workspace, pcm_out,
                           max_abs, stream);
    return launch_status("kernel launch: ");
}

mbx_status mbxn_fill_normal(float *out, int64_t stride, int32_t batch, const uint64_t *keys, const int64_t *first_step,
                            const int32_t *counts, int32_t max_count, void *hip_stream) {
    mbx::NoiseArgs a{};
    a.out = out;
    a.stride = stride;
    a.batch = batch;
    a.keys = keys;
    a.first_step = first_step;
    a.counts = counts;
    a.max_count = max_count;
    if (const char *why = mbx::check_fill_normal(a)) return refuse("fill normal", why);
    if (batch == 0 || max_count == 0) return MBX_OK;
    mbx::launch_fill_normal(a, static_cast<hipStream_t>(hip_stream));
    return launch_status("kernel launch: ");
}

mbx_status mbxw_mel_frames_at(const float *audio, int64_t stride, int32_t batch, const int32_t *n_samples,
                              const int64_t *centres, const int32_t *n_frames, int32_t max_frames, int32_t win,
                              int32_t fft_size, int32_t n_mels, const float *window, const float *twiddle, const float *basis,
                              const int32_t *bin_lo, const int32_t *bin_hi, float eps, float *out, void *hip_stream) {
    mbx::MelWarpArgs a{};
    a.audio = audio;
    a.stride = stride;
    a.batch = batch;
    a.n_samples = n_samples;
    a.centres = centres;
    a.n_frames = n_frames;
    a.max_frames = max_frames;
    a.win = win;
    a.fft_size = fft_size;
    a.n_mels = n_mels;
    a.window = window;
    a.twiddle = twiddle;
    a.basis = basis;
    a.bin_lo = bin_lo;
    a.bin_hi = bin_hi;
    a.eps = eps;
    a.out = out;
    if (const char *why = mbx::check_mel_warp(a)) return refuse("mel frames at", why);
    if (batch == 0) return MBX_OK;
    mbx::launch_mel_warp(a, static_cast<hipStream_t>(hip_stream));
    return launch_status("kernel launch: ");
}

mbx_status mbxe_warp_envelope(const float *mel, int64_t row_stride_items, int32_t batch, const int32_t *n_frames,
                              int32_t max_frames, int32_t n_mels, const float *centres, const float *factors, float *out,
                              void *hip_stream) {
    mbx::EnvelopeArgs a{};
    a.mel = mel;
    a.bstride = row_stride_items;
    a.batch = batch;
    a.n_frames = n_frames;
    a.max_frames = max_frames;
    a.n_mels = n_mels;
    a.centres = centres;
    a.factors = factors;
    a.out = out;
    if (const char *why = mbx::check_envelope(a)) return refuse("warp envelope", why);
    if (batch == 0) return MBX_OK;
    mbx::launch_envelope(a, static_cast<hipStream_t>(hip_stream));
    return launch_status("kernel launch: ");
}

mbx_status mbxp_track_f0(const float *audio, int64_t stride, int32_t batch, const int32_t *n_samples,
                         const int64_t *centres, const int32_t *n_frames, int32_t max_frames, int32_t sample_rate,
                         int32_t window, int32_t tau_min, int32_t tau_max, float threshold, float e_min, float *f0,
                         float *periodicity, void *hip_stream) {
    mbx::PitchArgs a{};
    a.audio = audio;
    a.stride = stride;
    a.batch = batch;
    a.n_samples = n_samples;
    a.centres = centres;
    a.n_frames = n_frames;
    a.max_frames = max_frames;
    a.sample_rate = sample_rate;
    a.window = window;
    a.tau_min = tau_min;
    a.tau_max = tau_max;
    a.threshold = threshold;
    a.e_min = e_min;
    a.f0 = f0;
    a.periodicity = periodicity;
    if (const char *why = mbx::check_track_f0(a)) return refuse("track f0", why);
    if (batch == 0) return MBX_OK;
    mbx::launch_track_f0(a, static_cast<hipStream_t>(hip_stream));
    return launch_status("kernel launch: ");
}

mbx_status mbxc_f0_candidates(const float *audio, int64_t stride, int32_t batch, const int32_t *n_samples,
                              const int64_t *centres, const int32_t *n_frames, int32_t max_frames, int32_t sample_rate,
                              int32_t window, int32_t tau_min, int32_t tau_max, float e_min, const float *thresholds,
                              const float *weights, int32_t n_thresholds, int32_t n_cand, float *period, float *cost,
                              float *dprime, void *hip_stream) {
    mbx::CandidateArgs a{};
    a.frame.audio = audio;
    a.frame.stride = stride;
    a.frame.batch = batch;
    a.frame.n_samples = n_samples;
    a.frame.centres = centres;
    a.frame.n_frames = n_frames;
    a.frame.max_frames = max_frames;
    a.frame.sample_rate = sample_rate;
    a.frame.window = window;
    a.frame.tau_min = tau_min;
    a.frame.tau_max = tau_max;
    a.frame.e_min = e_min;
    a.n_thresholds = n_thresholds;
    a.n_cand = n_cand;
    a.period = period;
    a.cost = cost;
    a.dprime = dprime;
    if (const char *why = mbx::fill_f0_candidates(a, thresholds, weights)) return refuse("f0 candidates", why);
    if (batch == 0) return MBX_OK;
    mbx::launch_f0_candidates(a, static_cast<hipStream_t>(hip_stream));
    return launch_status("kernel launch: ");
}

mbx_status mbxc_decode_f0(const float *period, const float *cost, const float *dprime, const int32_t *n_frames,
                          int32_t max_frames, int32_t batch, int32_t sample_rate, float w_jump, float w_switch, float *f0,
                          float *periodicity, void *hip_stream) {
    mbx::DecodeArgs a{};
    a.period = period;
    a.cost = cost;
    a.dprime = dprime;
    a.n_frames = n_frames;
    a.max_frames = max_frames;
    a.batch = batch;
    a.sample_rate = sample_rate;
    a.w_jump = w_jump;
    a.w_switch = w_switch;
    a.f0 = f0;
    a.periodicity = periodicity;
    if (const char *why = mbx::check_decode_f0(a)) return refuse("decode f0", why);
    if (batch == 0) return MBX_OK;
    mbx::launch_decode_f0(a, static_cast<hipStream_t>(hip_stream));
    return launch_status("kernel launch: ");
}

mbx_status mbxt_f0_frames(const float *rings, int32_t n_slots, int32_t ring_samples, const int64_t *desc, int32_t n_streams,
                          int32_t max_new_frames, int32_t hop, int32_t sample_rate, int32_t window, int32_t tau_min,
                          int32_t tau_max, float threshold, float e_min, float *f0, float *periodicity, void *hip_stream) {
    mbx::PitchStreamArgs a{};
    a.rings = {rings, n_slots, ring_samples};
    a.desc = reinterpret_cast<const long long *>(desc);
    a.n_streams = n_streams;
    a.max_new_frames = max_new_frames;
    a.hop = hop;
    a.sample_rate = sample_rate;
    a.window = window;
    a.tau_min = tau_min;
    a.tau_max = tau_max;
    a.threshold = threshold;
    a.e_min = e_min;
    a.f0 = f0;
    a.periodicity = periodicity;
    if (const char *why = mbx::check_f0_stream(a)) return refuse("f0 frames", why);
    mbx::launch_f0_stream(a, static_cast<hipStream_t>(hip_stream));
    return launch_status("kernel launch: ");
}

mbx_status mbxv_f0_candidate_frames(const float *rings, int32_t n_slots, int32_t ring_samples, const int64_t *desc,
                                    int32_t n_streams, int32_t max_new_frames, int32_t hop, int32_t sample_rate, int32_t window,
                                    int32_t tau_min, int32_t tau_max, float e_min, const float *thresholds, const float *weights,
                                    int32_t n_thresholds, int32_t n_cand, float *period, float *cost, float *dprime,
                                    void *hip_stream) {
    mbx::CandidateStreamArgs a{};
    a.ring.rings = {rings, n_slots, ring_samples};
    a.ring.desc = reinterpret_cast<const long long *>(desc);
    a.ring.n_streams = n_streams;
    a.ring.max_new_frames = max_new_frames;
    a.ring.hop = hop;
    a.ring.sample_rate = sample_rate;
    a.ring.window = window;
    a.ring.tau_min = tau_min;
    a.ring.tau_max = tau_max;
    a.ring.e_min = e_min;
    a.n_thresholds = n_thresholds;
    a.n_cand = n_cand;
    a.period = period;
    a.cost = cost;
    a.dprime = dprime;
    if (const char *why = mbx::fill_f0_stream_candidates(a, thresholds, weights)) return refuse("f0 candidate frames", why);
    if (n_streams == 0 || max_new_frames == 0) return MBX_OK;
    mbx::launch_f0_stream_candidates(a, static_cast<hipStream_t>(hip_stream));
    return launch_status("kernel launch: ");
}

size_t mbxv_lag_state_words(void) { return mbx::F0_LAG_STATE_WORDS; }

mbx_status mbxv_decode_f0_frames(const float *period, const float *cost, const float *dprime, const int64_t *desc,
                                 int32_t n_streams, int32_t max_new_frames, int32_t hop, void *state, int32_t n_slots,
                                 int32_t lag, int32_t sample_rate, float w_jump, float w_switch, float *f0, float *periodicity,
                                 int32_t max_out, void *hip_stream) {
    mbx::LagDecodeArgs a{};
    a.period = period;
    a.cost = cost;
    a.dprime = dprime;
    a.desc = reinterpret_cast<const long long *>(desc);
    a.n_streams = n_streams;
    a.max_new_frames = max_new_frames;
    a.hop = hop;
    a.state = static_cast<unsigned *>(state);
    a.n_slots = n_slots;
    a.lag = lag;
    a.sample_rate = sample_rate;
    a.w_jump = w_jump;
    a.w_switch = w_switch;
    a.f0 = f0;
    a.periodicity = periodicity;
    a.max_out = max_out;
    if (const char *why = mbx::check_lag_decode(a)) return refuse("decode f0 frames", why);
    if (n_streams == 0) return MBX_OK;
    mbx::launch_lag_decode(a, static_cast<hipStream_t>(hip_stream));
    return launch_status("kernel launch: ");
}

mbx_status mbxg_local_cost(const float *mel_a, const float *mel_b, const int32_t *n_frames_a, const int32_t *n_frames_b,
                           int32_t batch, int32_t max_frames_a, int32_t max_frames_b, int32_t n_mels, int32_t band,
                           uint16_t *cost, void *hip_stream) {
    mbx::AlignCostArgs a{};
    a.mel_a = mel_a;
    a.mel_b = mel_b;
    a.n_frames_a = n_frames_a;
    a.n_frames_b = n_frames_b;
    a.batch = batch;
    a.max_frames_a = max_frames_a;
    a.max_frames_b = max_frames_b;
    a.n_mels = n_mels;
    a.band = band;
    a.cost = cost;
    if (const char *why = mbx::check_align_cost(a)) return refuse("local cost", why);
    if (batch == 0) return MBX_OK;
    mbx::launch_align_cost(a, static_cast<hipStream_t>(hip_stream));
    return launch_status("kernel launch: ");
}

size_t mbxg_align_workspace_size(int32_t batch, int32_t max_frames_a, int32_t band) {
    if (batch < 0 || batch > 65535 || max_frames_a < 1 || max_frames_a > mbx::ALIGN_MAX_FRAMES || band < 1 ||
        band > mbx::ALIGN_MAX_BAND)
        return 0;
    return mbx::align_workspace_bytes(batch, max_frames_a, band);
}

mbx_status mbxg_align_path(const uint16_t *cost, const int32_t *n_frames_a, const int32_t *n_frames_b, int32_t batch,
                           int32_t max_frames_a, int32_t band, uint8_t *workspace, size_t workspace_bytes, int32_t *nodes_i,
                           int32_t *nodes_j, int32_t *count, int32_t *total, void *hip_stream) {
    mbx::AlignPathArgs a{};
    a.cost = cost;
    a.n_frames_a = n_frames_a;
    a.n_frames_b = n_frames_b;
    a.batch = batch;
    a.max_frames_a = max_frames_a;
    a.band = band;
    a.workspace = workspace;
    a.workspace_bytes = workspace_bytes;
    a.nodes_i = nodes_i;
    a.nodes_j = nodes_j;
    a.count = count;
    a.total = total;
    if (const char *why = mbx::check_align_path(a)) return refuse("align path", why);
    if (batch == 0) return MBX_OK;
    mbx::launch_align_path(a, static_cast<hipStream_t>(hip_stream));
    return launch_status("kernel launch: ");
}

}  // extern "C"

// Streaming F0 tracker (include/mbexwn_live_pitch.h: mbxt_f0_frames): the tracker of f0_track.hip for
// sounds that are still arriving, on the rings of the streaming mel analysis (mel_stream.hip).
//
// Frame t of a stream has centre c = t * hop (clamped to [0, n_total] once the length is known) and holds
//   y[i] = x[c - L/2 + i], 0 outside the sound,   L = W + tau_max,
// read by absolute index through ring[s & (ring_samples - 1)].  Everything behind the load of the frame is f0_frame.h's, the
// functions the offline kernel calls: only the fetch of a sample differs (ring instead of the item's row), so a frame carries
// the bits mbxp_track_f0 gives at centre t * hop on the stream's whole sound.  "Outside" is decided from the index alone and
// never touches the ring: a reused slot may hold another stream's NaN.  While a stream is open its length is unknown
// (n_total < 0): only the start is an edge, and the host asks for no frame that reads past the newest sample.
//
// One 256-thread block per (stream, new frame), plain vector code.  A descriptor that names a slot outside the ring store
// is skipped: a wrong entry must not address outside the caller's buffers.
//
// Host and device must give the same bits: f0_frame.h switches contraction off, and it stays off for this file.
#include <algorithm>
#include <cmath>

#include "f0_frame.h"
#include "mbx_kernels.h"

#pragma clang fp contract(off)

namespace mbx {

__global__ __launch_bounds__(F0_THREADS) void f0_stream_kernel(PitchStreamArgs p) {
    extern __shared__ __attribute__((aligned(16))) float f0_smem[];
    __shared__ float s_energy;
    const StreamRow row{p.desc + 4LL * blockIdx.y};
    if (!row.has_frame(blockIdx.x, p.rings)) return;
    const long long n_total = row.n_total();
    const int W = p.window, TM = p.tau_max, L = W + TM;
    long long c = (row.first() + blockIdx.x) * p.hop;
    if (n_total >= 0) c = min(c, n_total);
    const int bad = f0_frame_load(F0RingFetch(p.rings.row(row.slot()), p.rings.ring_samples, n_total, c, L), L, f0_smem);
    f0_frame_dprime(W, TM, f0_smem, &s_energy);
    if (threadIdx.x >= 64) return;
    float f0, per;
    f0_frame_pick(f0_smem + L, p.tau_min, TM, p.threshold, p.e_min, s_energy, p.sample_rate, bad, f0, per);
    if (threadIdx.x != 0) return;
    const long long o = (long long)blockIdx.y * p.max_new_frames + blockIdx.x;
    p.f0[o] = f0;
    p.periodicity[o] = per;
}

const char *check_f0_stream(const PitchStreamArgs &a) {
    if (!a.rings.data || !a.desc || !a.f0 || !a.periodicity) return "NULL pointer";
    if (!row_count_fits(a.n_streams)) return "n_streams must lie in [0, 65535]";
    if (a.max_new_frames < 0) return "max_new_frames must not be negative";
    if (a.hop < 1) return "hop must be at least 1";
    PitchArgs f{};                                          // the offline tracker's checks of the arguments the two share
    f.audio = a.rings.data;
    f.n_samples = f.n_frames = reinterpret_cast<const int32_t *>(a.desc);
    f.centres = reinterpret_cast<const int64_t *>(a.desc);
    f.f0 = a.f0;
    f.periodicity = a.periodicity;
    f.stride = f.max_frames = 1;
    f.sample_rate = a.sample_rate;
    f.window = a.window;
    f.tau_min = a.tau_min;
    f.tau_max = a.tau_max;
    f.threshold = a.threshold;
    f.e_min = a.e_min;
    if (const char *why = check_track_f0(f)) return why;
    if (ring_store_ok(a.rings, a.window + a.tau_max)) return nullptr;
    return "n_slots must be at least 1 and ring_samples a power of two, at least window + tau_max";
}

void launch_f0_stream(const PitchStreamArgs &a, hipStream_t stream) {
    if (a.n_streams == 0 || a.max_new_frames == 0) return;
    const size_t smem = (size_t)(a.window + 2 * a.tau_max + 1) * sizeof(float);
    hipLaunchKernelGGL(f0_stream_kernel, dim3(a.max_new_frames, a.n_streams), dim3(F0_THREADS), smem, stream, a);
}

}  // namespace mbx

// What the kernels of the live stages share around their own arithmetic (mel_stream.hip, f0_stream.hip, f0_lag.hip,
// resample_stream.hip, limiter.hip): the view of a ring store, the two descriptor rows with the guards their readers share,
// and the host checks of a store and of a row count.
//
// A ring store holds n_slots rings of ring_samples samples, a power of two: sample s of the stream in slot `slot` is at
// row(slot)[s & mask()].  A descriptor row that fails a guard is skipped and writes nothing: a wrong entry must not address
// outside the caller's buffers.  The guards a stage has of its own (an overflow bound that depends on its filter or its
// window, the clip of a count to the ring) stay with the stage.
#pragma once

namespace mbx {

inline bool power_of_two(int v) { return v > 0 && (v & (v - 1)) == 0; }

// the rows of a descriptor table are the y dimension of a grid
inline bool row_count_fits(int n) { return n >= 0 && n <= 65535; }

template <class T>
struct RingStoreOf {
    T *data;                      // (n_slots, ring_samples)
    int n_slots, ring_samples;    // ring_samples a power of two
    __device__ bool has(long long slot) const { return slot >= 0 && slot < n_slots; }
    __device__ T *row(long long slot) const { return data + slot * ring_samples; }
    __device__ long long mask() const { return ring_samples - 1; }
};
using RingStore = RingStoreOf<const float>;       // a store a kernel reads
using RingStoreOut = RingStoreOf<float>;          // ... and one it writes

// the host's check of a store: a pointer, at least one slot, rings of a power of two of at least `at_least` samples
template <class T>
bool ring_store_ok(const RingStoreOf<T> &s, int at_least = 1) {
    return s.data && s.n_slots >= 1 && power_of_two(s.ring_samples) && s.ring_samples >= at_least;
}

// a row of a frame table: (n_streams, 4) slot, first_frame, n_frames, n_total (< 0: the stream is still open).  A word is
// read where it is used, the guard's in its order: the kernels did so, and reading all four in front of the guard costs
// f0_stream_candidates_kernel 24 SGPRs and a wave of occupancy
struct StreamRow {
    const long long *d;
    __device__ long long slot() const { return d[0]; }
    __device__ long long first() const { return d[1]; }
    __device__ long long n() const { return d[2]; }
    __device__ long long n_total() const { return d[3]; }
    // frame `i` of the row is one to compute from `store`
    __device__ bool has_frame(long long i, const RingStore &store) const { return i < n() && store.has(slot()) && first() >= 0; }
};

// a row of an emit table: (n_rows, 6) slot, first_out, n_new, n_total (< 0: still open), out_offset and a word of the stage's
struct EmitRow {
    long long slot, first_out, n_new, n_total, out_offset, word5;
    static __device__ EmitRow of(const long long *d) { return {d[0], d[1], d[2], d[3], d[4], d[5]}; }
    // the row reads a ring of `store` and its n_new outputs fit the packed buffer of out_floats floats
    __device__ bool fits(const RingStore &store, long long out_floats) const {
        return store.has(slot) && first_out >= 0 && out_offset >= 0 && out_offset <= out_floats && n_new <= out_floats - out_offset;
    }
};

}  // namespace mbx

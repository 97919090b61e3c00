// The frame <-> timestamp bins of hirest_dataset.py:12-68 as device functions, shared by csrc/eval.hip (batched conversions) and
// csrc/cascade.hip (the seams of the end-to-end cascade).  Double precision, numpy's operation order; compile the including file
// with -ffp-contract=off so that no product is fused into an add.
#pragma once
#include "common.h"

namespace {

// hirest_dataset.py:12-68: bins = np.linspace(0, int(duration) - 1, n).  numpy builds it as arange(n) * step with
// step = (stop - start) / (n - 1) in double and overwrites the last element with `stop`; the bin value is recomputed
// here on demand (one multiply) instead of materialising n doubles per conversion as the reference does.
struct Bins {
    int64_t n; double stop, step;
    __device__ __forceinline__ double at(int64_t i) const { return (i == n - 1 && n > 1) ? stop : (n > 1 ? (double)i * step : 0.0); }
};
__device__ __forceinline__ bool make_bins(double duration, int32_t n_frames, Bins& b) {
    const int64_t d = (int64_t)duration;                       // Python int(): truncation toward zero
    b.n = n_frames < 0 ? d : n_frames;                         // n_frames < 0: one frame per second
    b.stop = (double)(d - 1);
    b.step = b.n > 1 ? b.stop / (double)(b.n - 1) : 0.0;
    return d >= 1 && b.n >= 1;                                 // shorter than one second: the reference's bins are empty / decreasing
}

// int(bins[f]) with numpy's negative indexing; INT64_MIN where the reference raises IndexError
__device__ __forceinline__ int64_t bins_frame_to_timestamp(const Bins& b, int64_t f) {
    if (f < 0) f += b.n;
    return (f < 0 || f >= b.n) ? INT64_MIN : (int64_t)b.at(f);
}

// min(np.digitize(x, bins, right=True), n - 1): the number of bins strictly below x, capped
__device__ __forceinline__ int64_t bins_timestamp_to_frame(const Bins& b, double x) {
    if (x != x) return b.n - 1;                                // NaN sorts after every bin
    int64_t k = 0;
    if (b.step > 0.0 && x > 0.0) {                             // first guess from the spacing, then settle on the exact bin values
        const double g = ceil(x / b.step);
        k = g >= (double)b.n ? b.n : (int64_t)g;
    }
    while (k > 0 && !(b.at(k - 1) < x)) --k;
    while (k < b.n && b.at(k) < x) ++k;
    return k < b.n - 1 ? k : b.n - 1;
}

}  // namespace

// Whisper's audio front end (hirest_amd/whisper.py): everything in front of the encoder's first block.
//
//   hirest_log_mel      waveform -> log-mel spectrogram, as whisper/audio.py::log_mel_spectrogram defines it (reflect-centred 400-point
//                       frames at hop 160, periodic Hann window, power spectrum over 201 bins, mel filter bank, log10, clamp at the call's
//                       maximum - 8, (x + 4) / 4).  The DFT and the mel sum are accumulated in double (plain fma chains, a 400-entry
//                       twiddle table indexed by (k j) mod 400) and rounded to fp32 at the log (the clamp and the affine map are exact in double on those
//                       logs and round once more at the store): an fp32 sum of 400 products has lost
//                       most of its digits exactly where the log is steepest, near the clamp floor.  Three launches: frames -> log10 mel
//                       + one maximum per block, the maxima -> one, clamp + normalise.  A maximum does not depend on the order it is
//                       taken in, so two runs give the same bits (no float atomics anywhere).
//   hirest_mel_to_rows  [B, n_mels, T] -> channel-last rows [B, T + 2, n_mels] with one zero row before and after each clip (the
//                       convolutions' padding): a 32x32 transpose through LDS, whole lines on both sides.  On that layout both
//                       convolutions of the stem are hirest_gemm_f32 products over an OVERLAPPING view of the rows (row m of the A
//                       operand starts stride * C floats after row m - 1 and is 3 C long), so no im2col copy exists.
#include "common.h"

namespace {

constexpr int NFFT = 400, HOP = 160, NBIN = NFFT / 2 + 1;
constexpr int FPB = 8;            // frames per block: one twiddle read feeds 16 fmas

// tables: cos(2 pi i / 400) [400] | sin(2 pi i / 400) [400] | periodic Hann window [400], doubles computed on the host
__global__ __launch_bounds__(256) void log_mel_kernel(const float* __restrict__ audio, int64_t n, int64_t total, int frames,
                                                      const float* __restrict__ filt, int n_mels, const double* __restrict__ tables,
                                                      float* __restrict__ out, float* __restrict__ blockmax) {
    __shared__ __attribute__((aligned(16))) double tw[NFFT][2];
    __shared__ double xs[FPB][NFFT];          // the windowed frames
    __shared__ double pw[FPB][NBIN];          // their power spectra
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f0 = blockIdx.x * FPB;
    for (int i = tid; i < NFFT; i += 256) { tw[i][0] = tables[i]; tw[i][1] = tables[NFFT + i]; }
    for (int e = tid; e < FPB * NFFT; e += 256) {
        const int f = e / NFFT, j = e - f * NFFT;
        double v = 0.0;
        if (f0 + f < frames) {
            int64_t i = (int64_t)(f0 + f) * HOP + j - NFFT / 2;     // position in the signal of n samples + padding zeros ...
            if (i < 0) i = -i;                                      // ... reflected about its first and last sample (total > 200)
            if (i >= total) i = 2 * (total - 1) - i;
            i = i < 0 ? 0 : i;
            if (i < n) v = (double)audio[i] * tables[2 * NFFT + j];
        }
        xs[f][j] = v;
    }
    __syncthreads();
    // lane = bin k: X[k] = sum_j x[j] (cos, sin)(2 pi k j / 400), the angle's index advanced by k mod 400 per sample.  The frame reads are
    // broadcasts; the twiddle read is the one per-lane LDS access of a step.
    if (tid < NBIN) {
        const int k = tid;
        double re[FPB], im[FPB];
#pragma unroll
        for (int f = 0; f < FPB; ++f) { re[f] = 0.0; im[f] = 0.0; }
        int idx = 0;
        for (int j = 0; j < NFFT; ++j) {
            const double c = tw[idx][0], s = tw[idx][1];
#pragma unroll
            for (int f = 0; f < FPB; ++f) {
                const double x = xs[f][j];
                re[f] = fma(x, c, re[f]);
                im[f] = fma(x, s, im[f]);
            }
            idx += k;
            idx = idx >= NFFT ? idx - NFFT : idx;
        }
#pragma unroll
        for (int f = 0; f < FPB; ++f) pw[f][k] = fma(re[f], re[f], im[f] * im[f]);
    }
    __syncthreads();
    // mel sums: thread -> (mel m, frame f), the frames of one m on consecutive lanes (one 32-B piece of the output row)
    float mx = -INFINITY;
    for (int o = tid; o < n_mels * FPB; o += 256) {
        const int m = o / FPB, f = o - m * FPB;
        const float* w = filt + (int64_t)m * NBIN;
        double acc = 0.0;
        for (int k = 0; k < NBIN; ++k) acc = fma((double)w[k], pw[f][k], acc);
        const float v = (float)log10(fmax(acc, 1e-10));
        if (f0 + f < frames) {
            out[(int64_t)m * frames + f0 + f] = v;
            mx = fmaxf(mx, v);
        }
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    if (tid == 0) blockmax[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void log_mel_max_kernel(const float* __restrict__ blockmax, int nblocks, float* __restrict__ gmax) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    float mx = -INFINITY;
    for (int i = tid; i < nblocks; i += 256) mx = fmaxf(mx, blockmax[i]);
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) *gmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// audio.py: log_spec = maximum(log_spec, log_spec.max() - 8.0); (log_spec + 4.0) / 4.0 — on the fp32 logs, in double (both steps are then
// exact), rounded once more at the store
__global__ __launch_bounds__(256) void log_mel_norm_kernel(float* __restrict__ out, int64_t count, const float* __restrict__ gmax) {
    const double floor_ = (double)*gmax - 8.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256)
        out[i] = (float)((fmax((double)out[i], floor_) + 4.0) * 0.25);
}

__global__ __launch_bounds__(256) void mel_to_rows_kernel(const float* __restrict__ mel, float* __restrict__ rows, int n_mels, int T) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int t0 = blockIdx.x * 32, m0 = blockIdx.y * 32, b = blockIdx.z;
    const float* src = mel + (int64_t)b * n_mels * T;
    float* dst = rows + (int64_t)b * (T + 2) * n_mels;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + ty + 8 * r, t = t0 + tx;
        if (m < n_mels && t < T) tile[ty + 8 * r][tx] = src[(int64_t)m * T + t];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int t = t0 + ty + 8 * r, m = m0 + tx;
        if (t < T && m < n_mels) dst[(int64_t)(t + 1) * n_mels + m] = tile[tx][ty + 8 * r];
    }
    if (blockIdx.x == 0 && ty < 2 && m0 + tx < n_mels) dst[(int64_t)(ty == 0 ? 0 : T + 1) * n_mels + m0 + tx] = 0.f;
}

inline int64_t log_mel_frames(int64_t n, int64_t padding) { return (n + padding) / HOP; }

}  // namespace

extern "C" size_t hirest_log_mel_workspace_bytes(int64_t n, int64_t padding) {
    if (n <= 0 || padding < 0 || n + padding <= NFFT / 2) return 0;
    const int64_t blocks = (log_mel_frames(n, padding) + FPB - 1) / FPB;
    return (size_t)(blocks + 1) * sizeof(float);
}

extern "C" int hirest_log_mel(const float* audio, int64_t n, int64_t padding, const float* filters, int32_t n_mels, const double* tables,
                              float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!audio || !filters || !tables || !out || !workspace || n <= 0 || padding < 0 || n_mels <= 0) return HIREST_E_BADARG;
    const int64_t total = n + padding, frames = log_mel_frames(n, padding);
    if (total <= NFFT / 2 || frames < 1 || frames > (int64_t)1 << 30 || n_mels > 1024) return HIREST_E_SHAPE;    // reflect padding needs > 200 samples
    if (workspace_bytes < hirest_log_mel_workspace_bytes(n, padding)) return HIREST_E_WORKSPACE;
    const int blocks = (int)((frames + FPB - 1) / FPB);
    float* blockmax = static_cast<float*>(workspace);
    float* gmax = blockmax + blocks;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(log_mel_kernel, dim3(blocks), dim3(256), 0, s, audio, n, total, (int)frames, filters, (int)n_mels, tables, out, blockmax);
    hipLaunchKernelGGL(log_mel_max_kernel, dim3(1), dim3(256), 0, s, blockmax, blocks, gmax);
    const int64_t count = frames * n_mels;
    const int64_t g = (count + 255) / 256;
    hipLaunchKernelGGL(log_mel_norm_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, s, out, count, gmax);
    return hirest_launch_status();
}

extern "C" int hirest_mel_to_rows(const float* mel, float* rows, int32_t B, int32_t n_mels, int32_t T, void* stream) {
    if (!mel || !rows || B <= 0 || n_mels <= 0 || T <= 0) return HIREST_E_BADARG;
    if (B > 65535 || (n_mels + 31) / 32 > 65535) return HIREST_E_SHAPE;
    hipLaunchKernelGGL(mel_to_rows_kernel, dim3((T + 31) / 32, (n_mels + 31) / 32, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), mel, rows,
                       (int)n_mels, (int)T);
    return hirest_launch_status();
}

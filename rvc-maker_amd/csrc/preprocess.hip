// Dataset preprocessing (main/inference/preprocess.py:129-185) in f64 on the device: the 5th-order
// high-pass over whole files (scipy.signal.lfilter), the slicer's frame RMS (get_rms), the peak
// normalisation (_normalize_audio) and the band-limited resample to 16 kHz (scipy.signal.resample_poly,
// the stand-in for soxr that rvc_amd.audio_io.resample uses on the host).
//
// lfilter: the chunked transposed-direct-form-II recurrence of filtfilt.hip (see its header for why
// chunks are chained by warm-up from a zero state and not by a matrix power, and for the LDS staging).
// What differs here:
//   * no zi: lanes whose window reaches n = 0 run on zero input from a zero state up to there, which
//     leaves the state exactly zero, so they are scipy's own recurrence from its own start;
//   * scipy's operation order with every product and sum rounded separately (no fused multiply-add):
//     those lanes are therefore bit-identical to scipy, and the others differ only by the rounding
//     noise a restart excites (the same size as the ba form's own noise) and the truncated warm-up;
//   * the warm-up length is an argument.  filtfilt.hip's 3584 is sized for 16 kHz; the same 48 Hz
//     Butterworth at 48 kHz needs 11383 samples for its impulse response to fall below 1e-12
//     (DESIGN.md), so the host measures the decay of the filter it is given (rvc_lfilter64_warmup).
#include "rvc_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int NS = 5;  // filter order
constexpr int LC = RVC_LFILTER_CHUNK;
constexpr int PB = RVC_LFILTER_TILE;
constexpr int RS = PB + 1;  // LDS row stride (elements)
static_assert(RVC_LFILTER_WAVE == 64 * LC && LC % PB == 0 && RVC_LFILTER_WARM_CAP % PB == 0, "lfilter geometry");

struct LfiltParams {
    double b[NS + 1], a[NS + 1];
    int N, warm;
};

// scipy's DOUBLE_filt, expression for expression
__device__ __forceinline__ double step(const LfiltParams& p, double* z, double xn) {
    const double yn = z[0] + p.b[0] * xn;
#pragma unroll
    for (int i = 0; i < NS - 1; ++i) z[i] = z[i + 1] + xn * p.b[i + 1] - yn * p.a[i + 1];
    z[NS - 1] = xn * p.b[NS] - yn * p.a[NS];
    return yn;
}

// lane r of block blk owns outputs [lo, lo + LC), lo = (blk*64 + r)*LC, and runs the recurrence from
// n = lo - warm.  A wave marches its 64 lanes through time in lockstep: each PB-step tile of inputs
// (64 rows x PB samples) is read with coalesced row loads into LDS one tile ahead, and the outputs leave
// through an LDS tile as coalesced row stores.
template <typename V>
__global__ __launch_bounds__(64) void lfilter_kernel(LfiltParams p, const V* x, double* y) {
    __shared__ V tin[64 * RS];
    __shared__ double tout[64 * RS];
    const int lane = threadIdx.x;
    const int blo = blockIdx.x * 64 * LC;  // first output of the block
    const int lo = blo + lane * LC;
    const int warm = p.warm;
    double z[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) z[i] = 0.0;
    // staging slot: element i of a tile load covers row 2i + (lane >> 5), column lane & 31
    const int srow = lane >> 5, scol = lane & 31;
    V raw[PB];
    auto gload = [&](int t0) {
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const int n = blo + (2 * i + srow) * LC - warm + t0 + scol;
            raw[i] = x[n < 0 ? 0 : (n >= p.N ? p.N - 1 : n)];  // clamped: values outside [0, N) are not used
        }
    };
    auto sstore = [&]() {
#pragma unroll
        for (int i = 0; i < PB; ++i) tin[(2 * i + srow) * RS + scol] = raw[i];
    };
    const int steps = warm + LC;
    gload(0);
    sstore();
    __syncthreads();
    for (int t0 = 0; t0 < steps; t0 += PB) {
        const bool more = t0 + PB < steps;
        if (more) gload(t0 + PB);
        const bool out_phase = t0 >= warm;
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const int n = lo - warm + t0 + j;
            const double xn = n < 0 ? 0.0 : (double)tin[lane * RS + j];  // before the start: zero input, zero state
            const double yn = step(p, z, xn);
            if (out_phase) tout[lane * RS + j] = yn;
        }
        __syncthreads();
        if (out_phase) {  // coalesced row stores of the tile's outputs
#pragma unroll
            for (int i = 0; i < PB; ++i) {
                const int row = 2 * i + srow;
                const int n = blo + row * LC + (t0 - warm) + scol;
                if (n < p.N) y[n] = tout[row * RS + scol];
            }
        }
        if (more) sstore();
        __syncthreads();
    }
}

// get_rms: one wave per frame.  Lane l sums the squares of samples l, l + 64, ... of the frame in that order,
// then the 64 partial sums meet in a butterfly whose every level adds the same pairs: a fixed order.
template <typename V>
__global__ __launch_bounds__(256) void frame_rms_kernel(const V* x, int64_t N, int frame, int hop, int64_t nframes,
                                                        double* out) {
    const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= nframes) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const int64_t base = f * hop - frame / 2;
    double acc = 0.0;
    for (int i = lane; i < frame; i += 64) {
        const int64_t j = base + i;
        const double v = (j >= 0 && j < N) ? (double)x[j] : 0.0;
        acc += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) out[f] = sqrt(acc / (double)frame);
}

// max|x| as the bit pattern of a non-negative double: the patterns order as the values do, and a NaN's
// pattern is above every number's, so a NaN reaches the cell as numpy's max would return it.
__global__ __launch_bounds__(256) void peak_abs_kernel(const double* x, int64_t N, unsigned long long* cell) {
    unsigned long long m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        const unsigned long long v = (unsigned long long)__double_as_longlong(fabs(x[i]));
        m = v > m ? v : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_xor(m, o, 64);
        m = v > m ? v : m;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(cell, m);
}

// (audio / tmp_max * (MAX_AMPLITUDE * ALPHA)) + (1 - ALPHA) * audio, numpy's order, each step rounded
__global__ __launch_bounds__(256) void peak_mix_kernel(const double* x, int64_t N, double gain, double rest,
                                                       const unsigned long long* cell, double* y) {
    const double peak = __longlong_as_double((long long)*cell);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        const double v = x[i];
        y[i] = (v / peak * gain) + rest * v;
    }
}

// scipy.signal.upfirdn(h, x, up, down)[n_pre_remove : n_pre_remove + out_len] of one chunk per blockIdx.y:
// output k of the full convolution reads phase t = (k down) % up at input position q = (k down) / up and sums
// x[q - hpp + 1 .. q] * h[t + (hpp - 1 - j) up] oldest sample first, as _upfirdn_apply does; samples outside
// the chunk's own [0, in_len) are zeros.
template <typename V>
__global__ __launch_bounds__(256) void resample_poly_kernel(const V* x, const double* h, int h_len, int up, int down,
                                                            int hpp, int n_pre_remove, const int64_t* seg,
                                                            double* y64, float* y32) {
    const int64_t* s = seg + 4 * (int64_t)blockIdx.y;
    const int64_t in_off = s[0], in_len = s[1], out_off = s[2], out_len = s[3];
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= out_len) return;
    const int64_t pos = (m + n_pre_remove) * down;
    const int t = (int)(pos % up);
    const int64_t q = pos / up;
    const V* xs = x + in_off;
    double acc = 0.0;
    for (int j = 0; j < hpp; ++j) {
        const int64_t xi = q - hpp + 1 + j;
        const int hi = t + (hpp - 1 - j) * up;
        if (xi >= 0 && xi < in_len && hi < h_len) acc += (double)xs[xi] * h[hi];
    }
    y64[out_off + m] = acc;
    y32[out_off + m] = (float)acc;
}
}  // namespace

// The first multiple of the staging tile past the last sample at which |impulse response| >= 1e-12,
// measured by running the recurrence itself on a unit impulse; -1 when the response has not settled below
// that within RVC_LFILTER_WARM_CAP samples (checked over four times the cap) or a[0] == 0.
extern "C" int64_t rvc_lfilter64_warmup(const double* b, const double* a) {
    if (!b || !a || a[0] == 0.0 || !(a[0] == a[0])) return -1;
    double bn[NS + 1], an[NS + 1], z[NS] = {0, 0, 0, 0, 0};
    for (int i = 0; i <= NS; ++i) {
        bn[i] = b[i] / a[0];
        an[i] = a[i] / a[0];
    }
    int64_t last = -1;
    for (int64_t n = 0; n < 4 * (int64_t)RVC_LFILTER_WARM_CAP; ++n) {
        const double xn = n == 0 ? 1.0 : 0.0;
        const double yn = z[0] + bn[0] * xn;
        for (int i = 0; i < NS - 1; ++i) z[i] = z[i + 1] + xn * bn[i + 1] - yn * an[i + 1];
        z[NS - 1] = xn * bn[NS] - yn * an[NS];
        if (!(fabs(yn) < 1e-12)) last = n;  // NaN counts as not settled
    }
    const int64_t warm = ((last + 1) / PB + 1) * PB;
    return warm <= RVC_LFILTER_WARM_CAP ? warm : -1;
}

extern "C" int64_t rvc_lfilter64_work_bytes(int64_t N, int64_t warm) {
    if (N <= 0 || warm <= 0 || warm % PB || warm > RVC_LFILTER_WARM_CAP) return -1;
    return 0;  // every lane keeps its state in registers and its tiles in LDS
}

extern "C" int rvc_lfilter64(const void* x, int x_is_f64, int64_t N, const double* b, const double* a, int64_t warm,
                             void* work, int64_t work_bytes, double* y, rvc_stream_t stream) {
    RVC_CHECK_ARG(x && b && a && y, "lfilter64: null pointer");
    RVC_CHECK_ARG(N > 0, "lfilter64: N=%lld must be positive", (long long)N);
    RVC_CHECK_ARG(warm > 0 && warm % PB == 0 && warm <= RVC_LFILTER_WARM_CAP,
                  "lfilter64: warm-up %lld must be a positive multiple of %d up to %d (a filter that needs more is "
                  "not supported)", (long long)warm, PB, RVC_LFILTER_WARM_CAP);
    RVC_CHECK_ARG(N + RVC_LFILTER_WAVE + RVC_LFILTER_WARM_CAP < (1ll << 31), "lfilter64: N=%lld too long",
                  (long long)N);
    RVC_CHECK_ARG(a[0] != 0.0, "lfilter64: a[0] is zero");
    RVC_CHECK_ARG(work_bytes >= 0, "lfilter64: negative work_bytes");
    LfiltParams p;
    for (int i = 0; i <= NS; ++i) {  // scipy normalises by a[0] before it filters
        p.b[i] = b[i] / a[0];
        p.a[i] = a[i] / a[0];
    }
    p.N = (int)N;
    p.warm = (int)warm;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cdiv(N, RVC_LFILTER_WAVE));
    if (x_is_f64)
        hipLaunchKernelGGL(lfilter_kernel<double>, grid, dim3(64), 0, s, p, (const double*)x, y);
    else
        hipLaunchKernelGGL(lfilter_kernel<float>, grid, dim3(64), 0, s, p, (const float*)x, y);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int64_t rvc_frame_rms64_len(int64_t N, int64_t frame, int64_t hop) {
    if (N <= 0 || frame <= 0 || hop <= 0) return -1;
    return (N + 2 * (frame / 2) - frame) / hop + 1;
}

extern "C" int rvc_frame_rms64(const void* x, int x_is_f64, int64_t N, int64_t frame, int64_t hop, double* out,
                               rvc_stream_t stream) {
    RVC_CHECK_ARG(x && out, "frame_rms64: null pointer");
    RVC_CHECK_ARG(N > 0 && frame > 0 && hop > 0, "frame_rms64: N=%lld frame=%lld hop=%lld must be positive",
                  (long long)N, (long long)frame, (long long)hop);
    RVC_CHECK_ARG(frame < (1ll << 30) && hop < (1ll << 30), "frame_rms64: frame=%lld hop=%lld too large",
                  (long long)frame, (long long)hop);
    RVC_CHECK_ARG(N + 2 * (frame / 2) >= frame, "frame_rms64: N=%lld is shorter than an odd frame's padding allows",
                  (long long)N);
    const int64_t nframes = rvc_frame_rms64_len(N, frame, hop);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cdiv(nframes, 4));
    if (x_is_f64)
        hipLaunchKernelGGL(frame_rms_kernel<double>, grid, dim3(256), 0, s, (const double*)x, N, (int)frame, (int)hop,
                           nframes, out);
    else
        hipLaunchKernelGGL(frame_rms_kernel<float>, grid, dim3(256), 0, s, (const float*)x, N, (int)frame, (int)hop,
                           nframes, out);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_peak_mix64(const double* x, int64_t N, double gain, double rest, double* peak, double* y,
                              rvc_stream_t stream) {
    RVC_CHECK_ARG(x && peak && y, "peak_mix64: null pointer");
    RVC_CHECK_ARG(N > 0, "peak_mix64: N=%lld must be positive", (long long)N);
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = cdiv(N, 256) < 1024u ? cdiv(N, 256) : 1024u;
    RVC_HIP(hipMemsetAsync(peak, 0, sizeof(double), s));
    hipLaunchKernelGGL(peak_abs_kernel, dim3(blocks), dim3(256), 0, s, x, N, (unsigned long long*)peak);
    hipLaunchKernelGGL(peak_mix_kernel, dim3(blocks), dim3(256), 0, s, x, N, gain, rest,
                       (const unsigned long long*)peak, y);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_resample_poly64(const void* x, int x_is_f64, int64_t n_in, const double* h, int64_t h_len, int up,
                                   int down, int64_t n_pre_remove, const int64_t* seg_host, const int64_t* seg_dev,
                                   int64_t nseg, double* y64, float* y32, int64_t n_out, rvc_stream_t stream) {
    RVC_CHECK_ARG(x && h && seg_host && seg_dev && y64 && y32, "resample_poly64: null pointer");
    RVC_CHECK_ARG(n_in > 0 && n_out > 0 && nseg > 0 && nseg <= 65535,
                  "resample_poly64: n_in=%lld n_out=%lld nseg=%lld out of range", (long long)n_in, (long long)n_out,
                  (long long)nseg);
    RVC_CHECK_ARG(up > 0 && down > 0 && up < (1 << 15) && down < (1 << 15), "resample_poly64: up=%d down=%d", up, down);
    RVC_CHECK_ARG(h_len > 0 && h_len < (1ll << 24) && n_pre_remove >= 0 && n_pre_remove < (1ll << 24),
                  "resample_poly64: h_len=%lld n_pre_remove=%lld out of range", (long long)h_len,
                  (long long)n_pre_remove);
    int64_t longest = 0;
    for (int64_t i = 0; i < nseg; ++i) {
        const int64_t in_off = seg_host[4 * i], in_len = seg_host[4 * i + 1];
        const int64_t out_off = seg_host[4 * i + 2], out_len = seg_host[4 * i + 3];
        RVC_CHECK_ARG(in_off >= 0 && in_len > 0 && in_len <= n_in && in_off <= n_in - in_len,
                      "resample_poly64: chunk %lld reads [%lld, +%lld) of %lld samples", (long long)i, (long long)in_off,
                      (long long)in_len, (long long)n_in);
        RVC_CHECK_ARG(in_len < (1ll << 40) && out_len == (in_len * up + down - 1) / down,
                      "resample_poly64: chunk %lld: out_len=%lld is not ceil(%lld * %d / %d)", (long long)i,
                      (long long)out_len, (long long)in_len, up, down);
        RVC_CHECK_ARG(out_off >= 0 && out_len <= n_out && out_off <= n_out - out_len,
                      "resample_poly64: chunk %lld writes [%lld, +%lld) of %lld samples", (long long)i,
                      (long long)out_off, (long long)out_len, (long long)n_out);
        longest = out_len > longest ? out_len : longest;
    }
    const int hpp = (int)((h_len + up - 1) / up);  // taps per phase
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cdiv(longest, 256), (unsigned)nseg);
    if (x_is_f64)
        hipLaunchKernelGGL(resample_poly_kernel<double>, grid, dim3(256), 0, s, (const double*)x, h, (int)h_len, up,
                           down, hpp, (int)n_pre_remove, seg_dev, y64, y32);
    else
        hipLaunchKernelGGL(resample_poly_kernel<float>, grid, dim3(256), 0, s, (const float*)x, h, (int)h_len, up,
                           down, hpp, (int)n_pre_remove, seg_dev, y64, y32);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

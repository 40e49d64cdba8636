// Formant shifting (main/library/algorithm/stftpitchshift.py, the StftPitchShift(1024, 32, 16000)
// .shiftpitch(audio, factors=1, quefrency, distortion) that load_audio runs for formant_shifting,
// main/library/utils.py:104-108) in f64 on the device.
//
// The reference is a phase vocoder at factor 1: every frame is split into magnitude and instantaneous
// frequency, the magnitude's cepstral envelope is taken off, resampled along frequency by `distortion`
// and put back, and the frames are resynthesised from the magnitudes and the running sum of the phase
// increments.  M = (n - n_fft) / hop + 1 frames, no centre padding, everything between the f32 input and
// the f32 output in f64:
//   1. fm_analysis   frame x window -> radix-2 FFT in LDS (/ n_fft) -> |X| and arg X, [M][nbin]        (stft, encode)
//   2. fm_spectral   frequency from arg[m] - arg[m-1] (NumPy's floored-modulo wrap); lifter as two cosine
//                    products nbin -> q+1 -> nbin (only cepstral coefficients 0..q survive, weights 1, 2..2, 1
//                    on both sides); not-normal mask; |X| / envelope; the envelope resampled by `distortion`;
//                    frequency mask; |X| * envelope -> magnitude in place, phase increment [M][nbin]
//                                                                                  (lifter, resample, shiftpitch, decode)
//   3. fm_phase      running sum of the increments over frames, one thread per bin walking the frames in order
//                    (the reference's own summation order), in place                                     (decode)
//   4. fm_synthesis  Hermitian spectrum |X| e^{j phase} (DC and Nyquist zeroed) -> inverse FFT in LDS -> x synthesis
//                    window -> frames [M][n_fft]                                                          (istft)
//   5. fm_ola        gather: each output sample sums its <= n_fft / hop frames in frame order (no atomics) -> f32;
//                    samples past the last frame are exactly 0
// No contraction in the spectral stage: its wrap and its frequency mask are decisions.
#include <float.h>

#include "rvc_common.h"
#include "fft_lds.h"

namespace {

constexpr int NFFT_MAX = 2048;
constexpr int NBIN_MAX = NFFT_MAX / 2 + 1;
constexpr int PH_UNROLL = 32;  // frames whose increments one fm_phase thread has in flight

struct FmParams {
    const float* x;
    int64_t n, M;
    int nfft, hop, nbin, logn, q, sr;
    int resample, rs_count;  // distortion != 1; bins the resampled envelope writes: min(nbin, int(nbin * distortion))
    double rs_ratio;         // nbin / int(nbin * distortion)
    const double* win;
    const double* swin;
    double* arg;  // [M][nbin]
    double* mag;  // [M][nbin]
    double* dl;   // [M][nbin] phase increment, then phase
    double* fr;   // [M][nfft]
    float* out;
};

__global__ __launch_bounds__(256) void fm_analysis_kernel(FmParams p) {
    __shared__ double2 a[NFFT_MAX];
    const int64_t m = blockIdx.x;
    const float* xr = p.x + m * p.hop;
    for (int i = threadIdx.x; i < p.nfft; i += blockDim.x)
        a[bitrev(i, p.logn)] = make_double2((double)xr[i] * p.win[i], 0.0);
    __syncthreads();
    fft_lds(a, p.nfft, p.logn);
    const double inv = 1.0 / (double)p.nfft;  // rfft(norm="forward"); a power of two
    for (int k = threadIdx.x; k < p.nbin; k += blockDim.x) {
        const double re = a[k].x * inv;
        const double im = (k == 0 || k == p.nbin - 1) ? 0.0 : a[k].y * inv;  // a real transform's DC / Nyquist
        p.mag[m * p.nbin + k] = hypot(re, im);
        p.arg[m * p.nbin + k] = atan2(im, re);
    }
}

// (x + pi) % (2 pi) - pi with NumPy's floored modulo (npy_divmod): the result of % takes the divisor's sign
__device__ __forceinline__ double wrap_pi(double x) {
#pragma clang fp contract(off)
    const double two_pi = 2.0 * M_PI;
    double r = fmod(x + M_PI, two_pi);
    if (r != 0.0) {
        if (r < 0.0) r += two_pi;
    } else {
        r = 0.0;
    }
    return r - M_PI;
}

// isinf | isnan | abs < DBL_MIN (shiftpitch's isnotnormal)
__device__ __forceinline__ bool not_normal(double v) { return !(isfinite(v) && fabs(v) >= DBL_MIN); }

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void fm_spectral_kernel(FmParams p) {
#pragma clang fp contract(off)
    __shared__ double s_mag[NBIN_MAX], s_frq[NBIN_MAX], s_lg[NBIN_MAX], s_env[NBIN_MAX], s_cep[NBIN_MAX];
    __shared__ double s_cos[NFFT_MAX];
    const int N = p.nfft, nb = p.nbin, q = p.q;
    const int64_t m = blockIdx.x;
    const double* am = p.arg + m * nb;
    double* mg = p.mag + m * nb;
    double* dl = p.dl + m * nb;
    const double freqinc = (double)p.sr / (double)N;
    const double phaseinc = 2.0 * M_PI * (double)p.hop / (double)N;
    const double nyq = (double)p.sr / 2.0;

    for (int i = threadIdx.x; i < nb; i += blockDim.x) {
        const double di = (double)i;
        const double delta = am[i] - (m > 0 ? am[i - nb] : 0.0);
        const double v = mg[i];
        s_mag[i] = v;
        s_frq[i] = (di + wrap_pi(delta - di * phaseinc) / phaseinc) * freqinc;
        if (q) s_lg[i] = log10(v);
    }
    if (q) {
        for (int j = threadIdx.x; j < N; j += blockDim.x) s_cos[j] = cospi(2.0 * (double)j / (double)N);
        __syncthreads();
        // cepstrum c[n] = irfft(log10 |X|, norm="forward")[n], n = 0..q: a wave per coefficient
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int n = wave; n <= q; n += 4) {
            double acc = 0.0;
            for (int k = lane; k < nb; k += 64) {
                const double h = (k == 0 || k == nb - 1) ? 1.0 : 2.0;
                acc += h * s_lg[k] * s_cos[(k * n) & (N - 1)];
            }
            acc = wave_sum64(acc);
            if (lane == 0) s_cep[n] = (n == 0 || n == q) ? acc : 2.0 * acc;  // lowpass: c[1:q] *= 2, c[q+1:] = 0
        }
        __syncthreads();
        // envelope = 10 ** Re rfft(lowpassed cepstrum, norm="forward")
        for (int k = threadIdx.x; k < nb; k += blockDim.x) {
            double acc = 0.0;
            for (int n = 0; n <= q; ++n) acc += s_cep[n] * s_cos[(k * n) & (N - 1)];
            s_env[k] = pow(10.0, acc / (double)N);
        }
        __syncthreads();
        if (p.resample) {  // envelopes[mask] = 0 before resample() reads its neighbours
            for (int k = threadIdx.x; k < nb; k += blockDim.x) s_lg[k] = not_normal(s_env[k]) ? 0.0 : s_env[k];
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < nb; i += blockDim.x) {
        const double di = (double)i;
        const double f = s_frq[i];
        double v = s_mag[i];
        double e = 1.0;
        bool masked = false;
        if (q) {
            e = s_env[i];
            masked = not_normal(e);
            v = masked ? 0.0 : v / e;
            if (p.resample) {  // resample(envelope, distortion): linear, only source bins j < nbin - 1 are written
                e = 0.0;
                if (i < p.rs_count) {
                    const double k = di * p.rs_ratio;
                    const double jt = trunc(k);
                    const int j = (int)jt;
                    const double w = k - jt;
                    if (j < nb - 1) e = w * s_lg[j + 1] + (1.0 - w) * s_lg[j];
                }
                masked = not_normal(e);
            }
        }
        if (f <= 0.0 || f >= nyq) v = 0.0;
        if (q) {
            v = v * e;
            if (masked) v = 0.0;
        }
        mg[i] = v;
        dl[i] = (di + (f - di * freqinc) / freqinc) * phaseinc;
    }
}

// phase[m][i] = sum of the increments of frames 0..m, added in frame order
__global__ __launch_bounds__(64) void fm_phase_kernel(FmParams p) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= p.nbin) return;
    double* d = p.dl + i;
    double acc = 0.0;
    int64_t m = 0;
    for (; m + PH_UNROLL <= p.M; m += PH_UNROLL) {  // a batch of loads in flight, then the sums in order
        double v[PH_UNROLL];
#pragma unroll
        for (int u = 0; u < PH_UNROLL; ++u) v[u] = d[(m + u) * p.nbin];
#pragma unroll
        for (int u = 0; u < PH_UNROLL; ++u) {
            acc += v[u];
            d[(m + u) * p.nbin] = acc;
        }
    }
    for (; m < p.M; ++m) {
        acc += d[m * p.nbin];
        d[m * p.nbin] = acc;
    }
}

__global__ __launch_bounds__(256) void fm_synthesis_kernel(FmParams p) {
    __shared__ double2 a[NFFT_MAX];
    const int N = p.nfft;
    const int64_t m = blockIdx.x;
    const double* mg = p.mag + m * p.nbin;
    const double* ph = p.dl + m * p.nbin;
    // irfft(Z) = Re fft(conj Z) over the Hermitian extension; frames[:, 0] = frames[:, -1] = 0
    for (int k = threadIdx.x; k < N / 2; k += blockDim.x) {
        if (k == 0) {
            a[bitrev(0, p.logn)] = make_double2(0.0, 0.0);
            a[bitrev(N / 2, p.logn)] = make_double2(0.0, 0.0);
            continue;
        }
        double sn, cs;
        sincos(ph[k], &sn, &cs);
        const double v = mg[k];
        a[bitrev(k, p.logn)] = make_double2(v * cs, -(v * sn));
        a[bitrev(N - k, p.logn)] = make_double2(v * cs, v * sn);
    }
    __syncthreads();
    fft_lds(a, N, p.logn);
    double* fr = p.fr + m * N;
    for (int i = threadIdx.x; i < N; i += blockDim.x) fr[i] = a[i].x * p.swin[i];
}

__global__ __launch_bounds__(256) void fm_ola_kernel(FmParams p) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= p.n) return;
    int64_t fa = (o - p.nfft + p.hop) / p.hop;  // first frame with o - fa hop < nfft
    if (fa < 0) fa = 0;
    int64_t fb = o / p.hop;
    if (fb > p.M - 1) fb = p.M - 1;
    double acc = 0.0;
    for (int64_t f = fa; f <= fb; ++f) acc += p.fr[f * p.nfft + (o - f * p.hop)];
    p.out[o] = (float)acc;
}

int plan(int64_t n, const rvc_formant_args* a, FmParams& p) {
    RVC_CHECK_ARG(a, "formant: null arguments");
    RVC_CHECK_ARG(a->n_fft >= 64 && a->n_fft <= NFFT_MAX && (a->n_fft & (a->n_fft - 1)) == 0,
                  "formant: n_fft must be a power of two in [64, %d]", NFFT_MAX);
    RVC_CHECK_ARG(a->hop >= 1 && a->hop <= a->n_fft && a->sample_rate > 0, "formant: bad hop / sample rate");
    RVC_CHECK_ARG(n >= a->n_fft, "formant: %lld samples are shorter than one frame of %d", (long long)n, a->n_fft);
    RVC_CHECK_ARG(a->quefrency_samples >= 0 && a->quefrency_samples <= a->n_fft / 2,
                  "formant: quefrency of %d samples outside 0..%d", a->quefrency_samples, a->n_fft / 2);
    RVC_CHECK_ARG(isfinite(a->distortion) && a->distortion > 0.0, "formant: distortion must be finite and positive");
    p.n = n;
    p.nfft = a->n_fft;
    p.hop = a->hop;
    p.nbin = a->n_fft / 2 + 1;
    p.logn = 0;
    while ((1 << p.logn) < p.nfft) ++p.logn;
    p.M = (n - p.nfft) / p.hop + 1;
    RVC_CHECK_ARG(p.M < (1LL << 31) - 1, "formant: signal too long");
    p.q = a->quefrency_samples;
    p.sr = a->sample_rate;
    p.resample = p.q != 0 && a->distortion != 1.0;
    const double md = trunc((double)p.nbin * a->distortion);  // resample(): m = int(n * factor)
    RVC_CHECK_ARG(md >= 1.0, "formant: distortion %g leaves no envelope bin", a->distortion);
    p.rs_ratio = (double)p.nbin / md;
    p.rs_count = md < (double)p.nbin ? (int)md : p.nbin;
    p.win = a->window;
    p.swin = a->synth_window;
    return RVC_OK;
}

}  // namespace

extern "C" int64_t rvc_formant_work_bytes(int64_t n, const rvc_formant_args* a) {
    FmParams p;
    if (plan(n, a, p) != RVC_OK) return -1;
    return p.M * (3 * (int64_t)p.nbin + p.nfft) * 8;
}

extern "C" int rvc_formant_shift(const float* x, int64_t n, const rvc_formant_args* a, void* work, int64_t work_bytes,
                                 float* out, rvc_stream_t stream) {
    RVC_CHECK_ARG(x && out && a && a->window && a->synth_window, "formant: null pointer");
    FmParams p;
    const int rc = plan(n, a, p);
    if (rc != RVC_OK) return rc;
    const int64_t need = rvc_formant_work_bytes(n, a);
    RVC_CHECK_ARG(work && work_bytes >= need, "formant: work needs %lld B", (long long)need);
    const int64_t cells = p.M * p.nbin;
    p.x = x;
    p.arg = (double*)work;
    p.mag = p.arg + cells;
    p.dl = p.mag + cells;
    p.fr = p.dl + cells;
    p.out = out;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fm_analysis_kernel, dim3((unsigned)p.M), dim3(256), 0, s, p);
    RVC_HIP(hipGetLastError());
    hipLaunchKernelGGL(fm_spectral_kernel, dim3((unsigned)p.M), dim3(256), 0, s, p);
    RVC_HIP(hipGetLastError());
    hipLaunchKernelGGL(fm_phase_kernel, dim3(cdiv(p.nbin, 64)), dim3(64), 0, s, p);
    RVC_HIP(hipGetLastError());
    hipLaunchKernelGGL(fm_synthesis_kernel, dim3((unsigned)p.M), dim3(256), 0, s, p);
    RVC_HIP(hipGetLastError());
    hipLaunchKernelGGL(fm_ola_kernel, dim3(cdiv(p.n, 256)), dim3(256), 0, s, p);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

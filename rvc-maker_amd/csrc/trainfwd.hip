// The training forward's pieces the inference path lacks (main/inference/train.py): the linear spectrogram of
// spectrogram_torch (:700-706), the fused mel projection + log of spec_to_mel_torch (:708-713), and the two
// discriminator-free generator losses -- F.l1_loss on the sliced mel (:845, :865) and kl_loss (:317-325).
// The posterior encoder, the flow forward and the decoder run on the conv engine (rvc_amd/train_forward.py).
#include "fft_lds.h"
#include "reduce64.h"

namespace {

constexpr int MEL_ROWS = 4;                          // basis rows per thread of mel_log_kernel

// ------------------------------------------------------------------ spectrogram (train.py:700-706)
// One block per (frame, signal): the reflect-padded frame times the window (the reference's f32 torch.hann_window,
// uploaded once; its f64 run multiplies by the same f32 values) into LDS in bit-reversed order (2048 complex f64
// points are 32 KB), an f64 FFT, sqrt(re^2 + im^2 + 1e-6) rounded to f32 at the store.
// Frame f starts at sample f * hop - pad of the signal, pad = (nfft - hop) / 2 < N: one reflection reaches every
// index (the host checks pad < N).
__global__ __launch_bounds__(256) void spectrogram_kernel(const float* __restrict__ x, const float* __restrict__ win,
                                                          float* __restrict__ spec, int64_t N, int64_t F, int nfft,
                                                          int logn, int hop, int pad) {
    __shared__ double2 a[2048];
    const int64_t f = blockIdx.x, b = blockIdx.y;
    const float* xb = x + b * N;
    for (int j = threadIdx.x; j < nfft; j += blockDim.x) {
        int64_t s = f * hop + j - pad;
        s = s < 0 ? -s : s;
        s = s >= N ? 2 * (N - 1) - s : s;
        a[bitrev(j, logn)] = make_double2((double)xb[s] * (double)win[j], 0.0);
    }
    __syncthreads();
    fft_lds(a, nfft, logn);
    const int K = nfft / 2 + 1;
    float* sb = spec + b * K * F;
    for (int k = threadIdx.x; k < K; k += blockDim.x)
        sb[(int64_t)k * F + f] = (float)sqrt(a[k].x * a[k].x + a[k].y * a[k].y + 1e-6);
}

// ------------------------------------------------------------------ mel + log (train.py:708-713)
// mel[m][f] = log(max(sum_k basis[m][k] * spec[k][f], 1e-5)): a wave per (64 frames, MEL_ROWS rows, signal), the
// lanes over the frames (spec rows are read coalesced, each value feeding MEL_ROWS rows), the basis rows at
// wave-uniform addresses.  k runs in order in f64, so the product never leaves the registers before the log and the
// result is rounded once.
__global__ __launch_bounds__(64) void mel_log_kernel(const float* __restrict__ spec, const float* __restrict__ basis,
                                                     float* __restrict__ mel, int M, int K, int64_t F) {
    const int64_t f = (int64_t)blockIdx.x * 64 + threadIdx.x, b = blockIdx.z;
    const int m0 = blockIdx.y * MEL_ROWS;
    const int64_t fc = f < F ? f : F - 1;  // idle lanes read a valid column and store nothing
    const float* sb = spec + b * K * F + fc;
    const float* br[MEL_ROWS];
#pragma unroll
    for (int r = 0; r < MEL_ROWS; ++r) br[r] = basis + (int64_t)(m0 + r < M ? m0 + r : M - 1) * K;
    double acc[MEL_ROWS] = {};
    for (int k = 0; k < K; ++k) {
        const double v = (double)sb[(int64_t)k * F];
#pragma unroll
        for (int r = 0; r < MEL_ROWS; ++r) acc[r] = fma((double)br[r][k], v, acc[r]);
    }
    if (f >= F) return;
#pragma unroll
    for (int r = 0; r < MEL_ROWS; ++r)
        if (m0 + r < M) mel[(b * M + m0 + r) * F + f] = (float)log(fmax(acc[r], 1e-5));
}

// ------------------------------------------------------------------ the two losses: fixed two-stage sums
// reduce64.h's stage 1 over the n terms, then one wave adds the RED_BLOCKS partials by the same tree and divides.  f64
// throughout, one rounding to f32; no atomics, so two runs give the same bits.
__global__ __launch_bounds__(64) void reduce_stage2(const double* __restrict__ part, double denom,
                                                    float* __restrict__ out) {
    static_assert(RED_BLOCKS == 64, "stage 2 is one wave over the partials");
    const double s = wave_sum64(part[threadIdx.x]);
    if (threadIdx.x == 0) out[0] = (float)(s / denom);
}

// F.l1_loss(slice_segments(mel, ids, S), y_hat_mel): term i = (b, m, s) of [B][M][S].  A start outside [0, T - S]
// reads nothing and makes the result NaN.
__global__ __launch_bounds__(256) void slice_l1_kernel(const float* __restrict__ mel, const int64_t* __restrict__ ids,
                                                       const float* __restrict__ yhat, int64_t B, int64_t M, int64_t T,
                                                       int64_t S, double* __restrict__ part) {
    reduce_stage1(B * M * S, part, [&](int64_t i) -> double {
        const int64_t s = i % S, m = (i / S) % M, b = i / (S * M);
        const int64_t st = ids[b];
        if (st < 0 || st > T - S) return (double)NAN;
        return fabs((double)mel[(b * M + m) * T + st + s] - (double)yhat[i]);
    });
}

// kl_loss (train.py:317-325) at an all-ones mask: logs_p - logs_q - 0.5 + 0.5 (z_p - m_p)^2 exp(-2 logs_p), summed
// over [B][C][T] and divided by B * T (the sum of the mask)
__global__ __launch_bounds__(256) void kl_kernel(const float* __restrict__ zp, const float* __restrict__ logs_q,
                                                 const float* __restrict__ m_p, const float* __restrict__ logs_p,
                                                 int64_t C, int64_t T, int64_t q_bs, int64_t p_bs, int64_t n,
                                                 double* __restrict__ part) {
    reduce_stage1(n, part, [&](int64_t i) -> double {
        const int64_t b = i / (C * T), r = i - b * C * T;
        const double lp = (double)logs_p[b * p_bs + r], d = (double)zp[i] - (double)m_p[b * p_bs + r];
        return lp - (double)logs_q[b * q_bs + r] - 0.5 + 0.5 * d * d * exp(-2.0 * lp);
    });
}

}  // namespace

extern "C" int64_t rvc_spectrogram_frames(int64_t N, int nfft, int hop) {
    if (N <= 0 || hop <= 0 || nfft < hop || ((nfft - hop) & 1)) return -1;
    const int64_t pad = (nfft - hop) / 2;
    if (pad >= N || N + 2 * pad < nfft) return -1;
    return (N + 2 * pad - nfft) / hop + 1;
}

extern "C" int rvc_spectrogram(const float* x, const float* win, float* spec, int64_t B, int64_t N, int64_t F,
                               int nfft, int hop, rvc_stream_t stream) {
    RVC_CHECK_ARG(x && win && spec && B > 0 && B <= 65535, "spectrogram: null pointer or bad batch");
    RVC_CHECK_ARG(nfft == 1024 || nfft == 2048, "spectrogram: n_fft must be 1024 or 2048 (got %d)", nfft);
    const int64_t want = rvc_spectrogram_frames(N, nfft, hop);
    RVC_CHECK_ARG(want > 0, "spectrogram: %lld samples do not hold the reflect pad of (n_fft - hop) / 2 (n_fft %d, "
                  "hop %d, n_fft - hop even)", (long long)N, nfft, hop);
    RVC_CHECK_ARG(F == want && F <= 0x7fffffff, "spectrogram: F = %lld, expected %lld", (long long)F, (long long)want);
    hipLaunchKernelGGL(spectrogram_kernel, dim3((unsigned)F, (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, win,
                       spec, N, F, nfft, nfft == 1024 ? 10 : 11, hop, (nfft - hop) / 2);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_mel_log(const float* spec, const float* basis, float* mel, int64_t B, int64_t M, int64_t K, int64_t F,
                           rvc_stream_t stream) {
    RVC_CHECK_ARG(spec && basis && mel, "mel_log: null pointer");
    RVC_CHECK_ARG(B > 0 && B <= 65535 && M > 0 && M <= 4096 && K > 0 && K <= 65536 && F > 0 && F <= (1 << 30),
                  "mel_log: bad shape");
    hipLaunchKernelGGL(mel_log_kernel, dim3(cdiv(F, 64), cdiv(M, MEL_ROWS), (unsigned)B), dim3(64), 0,
                       (hipStream_t)stream, spec, basis, mel, (int)M, (int)K, F);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int64_t rvc_trainfwd_work_bytes(void) { return (int64_t)RED_BLOCKS * sizeof(double); }

extern "C" int rvc_slice_l1(const float* mel, const int64_t* ids, const float* yhat_mel, int64_t B, int64_t M, int64_t T,
                            int64_t S, void* work, int64_t work_bytes, float* out, rvc_stream_t stream) {
    RVC_CHECK_ARG(mel && ids && yhat_mel && work && out, "slice_l1: null pointer");
    RVC_CHECK_ARG(B > 0 && M > 0 && S > 0 && T >= S && B * M * T <= ((int64_t)1 << 40), "slice_l1: bad shape");
    RVC_CHECK_ARG(work_bytes >= rvc_trainfwd_work_bytes(), "slice_l1: work buffer too small");
    hipLaunchKernelGGL(slice_l1_kernel, dim3(RED_BLOCKS), dim3(256), 0, (hipStream_t)stream, mel, ids, yhat_mel, B, M, T,
                       S, (double*)work);
    hipLaunchKernelGGL(reduce_stage2, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)work,
                       (double)(B * M * S), out);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_kl_loss(const float* z_p, const float* logs_q, const float* m_p, const float* logs_p, int64_t B,
                           int64_t C, int64_t T, int64_t q_bstride, int64_t p_bstride, void* work, int64_t work_bytes,
                           float* out, rvc_stream_t stream) {
    RVC_CHECK_ARG(z_p && logs_q && m_p && logs_p && work && out, "kl_loss: null pointer");
    RVC_CHECK_ARG(B > 0 && C > 0 && T > 0 && B * C * T <= ((int64_t)1 << 40), "kl_loss: bad shape");
    RVC_CHECK_ARG((q_bstride == 0 || q_bstride >= C * T) && (p_bstride == 0 || p_bstride >= C * T),
                  "kl_loss: a batch stride shorter than C * T");
    RVC_CHECK_ARG(work_bytes >= rvc_trainfwd_work_bytes(), "kl_loss: work buffer too small");
    hipLaunchKernelGGL(kl_kernel, dim3(RED_BLOCKS), dim3(256), 0, (hipStream_t)stream, z_p, logs_q, m_p, logs_p, C, T,
                       q_bstride ? q_bstride : C * T, p_bstride ? p_bstride : C * T, B * C * T, (double*)work);
    hipLaunchKernelGGL(reduce_stage2, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)work, (double)(B * T),
                       out);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

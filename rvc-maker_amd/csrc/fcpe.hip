// fcpe f0 (VC.get_f0_fcpe, convert.py:239-246): the pieces of the conv-only CFNaiveMelPE
// (main/library/predictors/FCPE.py) that the conv engine and rvc_layernorm_cf do not cover -- the mel
// front end, GroupNorm + LeakyReLU, the Conformer block's fused GLU / depthwise conv / SiLU, the local-argmax
// decoder and the f0 post-processing.  include/rvc_amd.h lists the launch order.
#include "fft_lds.h"

namespace {

constexpr int NFFT = RVC_FCPE_NFFT, HOP = RVC_FCPE_HOP, NMEL = RVC_FCPE_MELS, NBIN = NFFT / 2 + 1;
constexpr int PADL = (NFFT - HOP) / 2;  // 432 on both sides (FCPE.py:862-863 for n > 592)

RVC_DEV double wave_sum64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------ mel (FCPE.py:838-876, 898-913)
// One block per (frame, signal): the reflect-padded frame times the periodic Hann window into LDS in
// bit-reversed order, an f64 FFT, sqrt(re^2 + im^2 + 1e-9), then the 128 x 513 basis product (a wave per 32
// rows, lanes over the bins) and log(max(., 1e-5)), rounded to f32 at the store.
__global__ __launch_bounds__(256) void fcpe_mel_kernel(const float* __restrict__ x, const float* __restrict__ basis,
                                                       float* __restrict__ mel, int64_t N, int64_t T) {
    __shared__ double2 a[NFFT];
    __shared__ double mag[NBIN];
    const int64_t f = blockIdx.x, b = blockIdx.y;
    const int64_t fr = f < T - 1 ? f : T - 2;  // Wav2MelModule repeats the last frame (FCPE.py:910)
    const float* xb = x + b * N;
    for (int j = threadIdx.x; j < NFFT; j += blockDim.x) {
        int64_t s = fr * HOP + j - PADL;
        s = s < 0 ? -s : s;
        s = s >= N ? 2 * (N - 1) - s : s;
        const double w = 0.5 - 0.5 * cospi(2.0 * (double)j / (double)NFFT);
        a[bitrev(j, 10)] = make_double2((double)xb[s] * w, 0.0);
    }
    __syncthreads();
    fft_lds(a, NFFT, 10);
    for (int k = threadIdx.x; k < NBIN; k += blockDim.x) mag[k] = sqrt(a[k].x * a[k].x + a[k].y * a[k].y + 1e-9);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = wave * (NMEL / 4); r < (wave + 1) * (NMEL / 4); ++r) {
        double s = 0.0;
        for (int k = lane; k < NBIN; k += 64) s += (double)basis[r * NBIN + k] * mag[k];
        s = wave_sum64(s);
        if (lane == 0) mel[(b * NMEL + r) * T + f] = (float)log(fmax(s, 1e-5));
    }
}

// ------------------------------------------------------------------ GroupNorm + LeakyReLU (FCPE.py:422)
constexpr int GN_CHUNKS = 64;

// partial f64 sum and sum of squares of chunk blockIdx.x of group blockIdx.y (a group is contiguous: Cg * T)
__global__ __launch_bounds__(256) void gn_partial_kernel(const float* __restrict__ x, int64_t n, double* __restrict__ part) {
    __shared__ double ss[4], sq[4];
    const int64_t len = (n + GN_CHUNKS - 1) / GN_CHUNKS;
    const int64_t i0 = blockIdx.x * len, i1 = i0 + len < n ? i0 + len : n;
    const float* xg = x + blockIdx.y * n;
    double s = 0.0, q = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        const double v = (double)xg[i];
        s += v;
        q += v * v;
    }
    s = wave_sum64(s);
    q = wave_sum64(q);
    if ((threadIdx.x & 63) == 0) {
        ss[threadIdx.x >> 6] = s;
        sq[threadIdx.x >> 6] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* p = part + ((int64_t)blockIdx.y * GN_CHUNKS + blockIdx.x) * 2;
        p[0] = (ss[0] + ss[1]) + (ss[2] + ss[3]);
        p[1] = (sq[0] + sq[1]) + (sq[2] + sq[3]);
    }
}

__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ y, int64_t n,
                                                       int64_t T, int64_t Cg, int G, double eps, float slope,
                                                       const double* __restrict__ part) {
    __shared__ double stat[2];
    const int64_t bg = blockIdx.y;
    if (threadIdx.x < 64) {  // the group's 64 partials, summed in one fixed order by every block
        const double* p = part + (bg * GN_CHUNKS + threadIdx.x) * 2;
        const double s = wave_sum64(p[0]), q = wave_sum64(p[1]);
        if (threadIdx.x == 0) {
            const double mean = s / (double)n;
            const double var = fmax(q / (double)n - mean * mean, 0.0);
            stat[0] = mean;
            stat[1] = 1.0 / sqrt(var + eps);
        }
    }
    __syncthreads();
    const double mean = stat[0], rstd = stat[1];
    const int64_t c0 = (bg % G) * Cg;
    const int64_t base = (int64_t)blockIdx.x * 2048;
    for (int64_t i = base + threadIdx.x; i < base + 2048 && i < n; i += blockDim.x) {
        const int64_t c = c0 + i / T;
        const float v = (float)(((double)x[bg * n + i] - mean) * rstd * (double)gamma[c] + (double)beta[c]);
        y[bg * n + i] = v >= 0.f ? v : v * slope;
    }
}

// ------------------------------------------------------------------ GLU -> depthwise conv -> SiLU (FCPE.py:550)
// One block per (time tile, channel, batch element): the tile and its K - 1 halo are staged into LDS as
// u = a * sigmoid(g) (the GLU, once per element; zero outside [0, T): the conv's padding), then every thread
// computes one output from K LDS taps.  HBM is read once (plus the halo) and written once.
constexpr int DW_TILE = RVC_GLU_DW_TILE, DW_KMAX = 31;

__global__ __launch_bounds__(DW_TILE) void glu_dwconv_silu_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                  const float* __restrict__ bias, float* __restrict__ y,
                                                                  int64_t H, int64_t T, int K) {
    __shared__ float u[DW_TILE + DW_KMAX - 1];
    __shared__ float sw[DW_KMAX];
    const int64_t h = blockIdx.y, b = blockIdx.z;
    const int64_t t0 = (int64_t)blockIdx.x * DW_TILE;
    const int pad = K / 2;
    const float* xa = x + (b * 2 * H + h) * T;
    const float* xg = xa + H * T;
    for (int j = threadIdx.x; j < DW_TILE + K - 1; j += DW_TILE) {
        const int64_t t = t0 + j - pad;
        float v = 0.f;
        if (t >= 0 && t < T) v = xa[t] * (1.f / (1.f + expf(-xg[t])));
        u[j] = v;
    }
    if (threadIdx.x < K) sw[threadIdx.x] = w[h * K + threadIdx.x];
    __syncthreads();
    const int64_t t = t0 + threadIdx.x;
    if (t >= T) return;
    float acc = bias[h];
    for (int k = 0; k < K; ++k) acc = fmaf(sw[k], u[threadIdx.x + k], acc);
    y[(b * H + h) * T + t] = acc * (1.f / (1.f + expf(-acc)));
}

// ------------------------------------------------------------------ decode (FCPE.py:451-468, 479-480, 751-756)
// A block decodes DEC_F frames: DEC_S threads per frame each scan a contiguous slice of the bins (frames along the
// lanes, so every load is a run of consecutive frames), and the slices' maxima are merged in bin order.
constexpr int DEC_F = 32, DEC_S = 8;

__global__ __launch_bounds__(DEC_F * DEC_S) void fcpe_decode_kernel(const float* __restrict__ lat,
                                                                    const float* __restrict__ cent, float* __restrict__ f0,
                                                                    int64_t C, int64_t T, float thr, float f0_min,
                                                                    float f0_max) {
#pragma clang fp contract(off)
    __shared__ float s_val[DEC_S][DEC_F];
    __shared__ int s_idx[DEC_S][DEC_F];
    const int fl = threadIdx.x % DEC_F, sl = threadIdx.x / DEC_F;
    const int64_t t = (int64_t)blockIdx.x * DEC_F + fl, b = blockIdx.y;
    const int64_t tc = t < T ? t : T - 1;  // lanes past the end scan the last frame and store nothing
    const float* y = lat + b * C * T + tc;
    const int64_t per = (C + DEC_S - 1) / DEC_S;
    const int64_t c0 = sl * per, c1 = c0 + per < C ? c0 + per : C;
    float best = -INFINITY;
    int bi = -1;
    for (int64_t c = c0; c < c1; ++c) {  // torch.max: the first index of the largest value
        const float v = y[c * T];
        if (v > best || bi < 0) {
            best = v;
            bi = (int)c;
        }
    }
    s_val[sl][fl] = best;
    s_idx[sl][fl] = bi;
    __syncthreads();
    if (sl != 0 || t >= T) return;
    float conf = s_val[0][fl];
    int64_t am = s_idx[0][fl];
    for (int s = 1; s < DEC_S; ++s)
        if (s_idx[s][fl] >= 0 && s_val[s][fl] > conf) {
            conf = s_val[s][fl];
            am = s_idx[s][fl];
        }
    float num = 0.f, den = 0.f;
    for (int d = -4; d <= 4; ++d) {
        int64_t c = am + d;
        c = c < 0 ? 0 : (c > C - 1 ? C - 1 : c);
        const float v = y[c * T];
        num += cent[c] * v;
        den += v;
    }
    float f = 0.f;
    if (conf > thr) f = 10.f * exp2f((num / den) / 1200.f);  // masked frames: 2^-inf = 0
    if (f < f0_min) f = 0.f;
    if (f > f0_max) f = f0_max;
    f0[b * T + t] = f;
}

// ------------------------------------------------------------------ post (FCPE.py:757-759, 975-1000)
constexpr int PT = 1024;

__global__ __launch_bounds__(PT) void fcpe_post_kernel(const float* __restrict__ f0, int T, int P, int hop, int sr,
                                                       float* __restrict__ g, int* __restrict__ prev,
                                                       int* __restrict__ next, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ int s_last[PT], s_first[PT], s_cnt[PT];
    const int tid = threadIdx.x;
    // F.interpolate(where(f0 == 0, nan, f0), size=P, mode="linear") then nan -> 0, as torch's CPU kernel computes it
    // in f32: a copy when the sizes agree, else source index fma(scale, i + 0.5, -0.5) clamped at 0 and
    // fma(w0, x0, w1 * x1), so a NaN neighbour under a zero weight still makes the frame unvoiced
    const float scale = (float)T / (float)P;
    for (int i = tid; i < P; i += PT) {
        float r;
        if (P == T) {
            r = f0[i];
        } else {
            float src = fmaf(scale, (float)i + 0.5f, -0.5f);
            src = src < 0.f ? 0.f : src;
            int i0 = (int)src;
            i0 = i0 < T - 1 ? i0 : T - 1;
            const int i1 = i0 + 1 < T - 1 ? i0 + 1 : T - 1;
            float lam = src - (float)i0;
            lam = fminf(fmaxf(lam, 0.f), 1.f);
            const float x0 = f0[i0], x1 = f0[i1];
            r = (x0 == 0.f || x1 == 0.f) ? 0.f : fmaf(1.f - lam, x0, lam * x1);
        }
        g[i] = r;
    }
    __syncthreads();
    // voiced flags scanned over the block: every thread owns a run of frames
    const int chunk = (P + PT - 1) / PT;
    const int c0 = min(tid * chunk, P), c1 = min(c0 + chunk, P);
    int last = -1, first = P, cnt = 0;
    for (int i = c0; i < c1; ++i)
        if (g[i] != 0.f) {
            last = i;
            first = first == P ? i : first;
            ++cnt;
        }
    s_last[tid] = last;
    s_first[tid] = first;
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < PT; off <<= 1) {
        const int a = tid >= off ? s_last[tid - off] : -1;
        const int f = tid + off < PT ? s_first[tid + off] : P;
        const int c = tid >= off ? s_cnt[tid - off] : 0;
        __syncthreads();
        s_last[tid] = max(s_last[tid], a);
        s_first[tid] = min(s_first[tid], f);
        s_cnt[tid] += c;
        __syncthreads();
    }
    const int nv = s_cnt[PT - 1], vfirst = s_first[0], vlast = s_last[PT - 1];
    int l = tid > 0 ? s_last[tid - 1] : -1;
    for (int i = c0; i < c1; ++i) {
        l = g[i] != 0.f ? i : l;
        prev[i] = l;  // the last voiced frame <= i, or -1
    }
    int nx = tid + 1 < PT ? s_first[tid + 1] : P;
    for (int i = c1 - 1; i >= c0; --i) {
        nx = g[i] != 0.f ? i : nx;
        next[i] = nx;  // the first voiced frame >= i, or P
    }
    __syncthreads();
    if (nv <= 1) {  // compute_f0's all-zero return, post_process's single-value return
        const double v = nv == 1 ? (double)g[vfirst] : 0.0;
        for (int i = tid; i < P; i += PT) out[i] = v;
        return;
    }
    // np.interp(arange(P) * hop / sr, hop / sr * nzindex, f0[nzindex], left, right), f64.  Query i and node i are
    // two roundings of the same number, so the search's "xp[j] <= x" is decided on the values themselves.
    const double hs = (double)hop / (double)sr;
    const double xlast = hs * (double)vlast;
    for (int i = tid; i < P; i += PT) {
        const double xq = (double)((int64_t)i * hop) / (double)sr;
        int j = prev[i];
        if (j == i && hs * (double)j > xq) j = i > 0 ? prev[i - 1] : -1;
        double r;
        if (j < 0) {
            r = (double)g[vfirst];
        } else if (xq > xlast || j == vlast) {
            r = (double)g[vlast];
        } else {
            const double xj = hs * (double)j, fj = (double)g[j];
            if (xj == xq) {
                r = fj;
            } else {
                const int n = next[j + 1];
                const double slope = ((double)g[n] - fj) / (hs * (double)n - xj);
                r = slope * (xq - xj) + fj;
            }
        }
        out[i] = r;
    }
}

}  // namespace

extern "C" int rvc_fcpe_mel(const float* x, const float* basis, float* mel, int64_t B, int64_t N,
                            rvc_stream_t stream) {
    RVC_CHECK_ARG(x && basis && mel, "fcpe_mel: null pointer");
    RVC_CHECK_ARG(B >= 1 && B <= 65535, "fcpe_mel: bad batch %lld", (long long)B);
    RVC_CHECK_ARG(N > PADL, "fcpe_mel: %lld samples: at most %d is the reference's constant-padding case, "
                  "which is not supported", (long long)N, PADL);
    RVC_CHECK_ARG(N < (1ll << 31), "fcpe_mel: bad length %lld", (long long)N);
    const int64_t T = N / HOP + 1;
    hipLaunchKernelGGL(fcpe_mel_kernel, dim3((unsigned)T, (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, basis,
                       mel, N, T);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int64_t rvc_groupnorm_work_bytes(int64_t B, int G) {
    if (B < 1 || G < 1 || B * G > 65535) return -1;
    return B * G * GN_CHUNKS * 2 * (int64_t)sizeof(double);
}

extern "C" int rvc_groupnorm_act(const float* x, const float* gamma, const float* beta, float* y, int64_t B,
                                 int64_t C, int64_t T, int G, float eps, float slope, void* work, int64_t work_bytes,
                                 rvc_stream_t stream) {
    RVC_CHECK_ARG(x && gamma && beta && y && work, "groupnorm_act: null pointer");
    RVC_CHECK_ARG(B >= 1 && C >= 1 && T >= 1 && G >= 1, "groupnorm_act: bad shape B=%lld C=%lld T=%lld G=%d",
                  (long long)B, (long long)C, (long long)T, G);
    RVC_CHECK_ARG(C % G == 0, "groupnorm_act: %lld channels do not divide into %d groups", (long long)C, G);
    RVC_CHECK_ARG(B * G <= 65535 && (C / G) * T < (1ll << 40), "groupnorm_act: shape too large");
    RVC_CHECK_ARG(work_bytes >= rvc_groupnorm_work_bytes(B, G), "groupnorm_act: work buffer too small");
    const int64_t Cg = C / G, n = Cg * T;
    double* part = (double*)work;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gn_partial_kernel, dim3(GN_CHUNKS, (unsigned)(B * G)), dim3(256), 0, s, x, n, part);
    hipLaunchKernelGGL(gn_apply_kernel, dim3(cdiv(n, 2048), (unsigned)(B * G)), dim3(256), 0, s, x, gamma, beta, y, n,
                       T, Cg, G, (double)eps, slope, part);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_glu_dwconv_silu(const float* x, const float* w, const float* bias, float* y, int64_t B, int64_t H,
                                   int64_t T, int K, rvc_stream_t stream) {
    RVC_CHECK_ARG(x && w && bias && y, "glu_dwconv_silu: null pointer");
    RVC_CHECK_ARG(x != y, "glu_dwconv_silu: in place");
    RVC_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && H <= 65535 && T >= 1 && T < (1ll << 31),
                  "glu_dwconv_silu: bad shape B=%lld H=%lld T=%lld", (long long)B, (long long)H, (long long)T);
    RVC_CHECK_ARG(K >= 1 && K <= DW_KMAX && (K & 1), "glu_dwconv_silu: K=%d (odd, at most %d)", K, DW_KMAX);
    hipLaunchKernelGGL(glu_dwconv_silu_kernel, dim3(cdiv(T, DW_TILE), (unsigned)H, (unsigned)B), dim3(DW_TILE), 0,
                       (hipStream_t)stream, x, w, bias, y, H, T, K);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_fcpe_decode(const float* latent, const float* cent_table, float* f0, int64_t B, int64_t C,
                               int64_t T, float threshold, float f0_min, float f0_max, rvc_stream_t stream) {
    RVC_CHECK_ARG(latent && cent_table && f0, "fcpe_decode: null pointer");
    RVC_CHECK_ARG(B >= 1 && B <= 65535 && C >= 1 && T >= 1 && T < (1ll << 31),
                  "fcpe_decode: bad shape B=%lld C=%lld T=%lld", (long long)B, (long long)C, (long long)T);
    RVC_CHECK_ARG(f0_min <= f0_max, "fcpe_decode: f0_min %g > f0_max %g", (double)f0_min, (double)f0_max);
    hipLaunchKernelGGL(fcpe_decode_kernel, dim3(cdiv(T, DEC_F), (unsigned)B), dim3(DEC_F * DEC_S), 0,
                       (hipStream_t)stream, latent, cent_table, f0, C, T, threshold, f0_min, f0_max);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int64_t rvc_fcpe_post_work_bytes(int64_t p_len) {
    if (p_len <= 0 || p_len >= (1ll << 24)) return -1;
    return p_len * 3 * (int64_t)sizeof(int);
}

extern "C" int rvc_fcpe_post(const float* f0, int64_t T, int64_t p_len, int hop_length, int sample_rate, void* work,
                             int64_t work_bytes, double* out, rvc_stream_t stream) {
    RVC_CHECK_ARG(f0 && work && out, "fcpe_post: null pointer");
    RVC_CHECK_ARG(T >= 1 && T < (1ll << 24), "fcpe_post: bad track length %lld", (long long)T);
    RVC_CHECK_ARG(p_len >= 1 && p_len < (1ll << 24), "fcpe_post: bad p_len %lld", (long long)p_len);
    RVC_CHECK_ARG(hop_length >= 1 && hop_length <= 65536 && sample_rate >= 1, "fcpe_post: bad hop_length %d / "
                  "sample_rate %d", hop_length, sample_rate);
    RVC_CHECK_ARG(work_bytes >= rvc_fcpe_post_work_bytes(p_len), "fcpe_post: work buffer too small");
    float* g = (float*)work;
    int* prev = (int*)work + p_len;
    int* next = (int*)work + 2 * p_len;
    hipLaunchKernelGGL(fcpe_post_kernel, dim3(1), dim3(PT), 0, (hipStream_t)stream, f0, (int)T, (int)p_len,
                       hop_length, sample_rate, g, prev, next, out);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

// The MultiPeriodDiscriminator's pieces the conv engine does not hold (main/inference/train.py:608-674) and the GAN
// losses on its outputs (train.py:286-315): DiscriminatorP's reflect pad + [H][p] view + first Conv2d in one launch,
// DiscriminatorS's four grouped k = 41 convs as a direct f32 kernel, and feature_loss / discriminator_loss /
// generator_loss as fixed-order f64 sums.  Every other layer runs on the conv engine (rvc_amd/discriminator.py).
#include "reduce64.h"

namespace {

constexpr int PF_CO = 32, PF_K = 5, PF_STRIDE = 3, PF_PAD = 2;  // Conv2d(1, 32, (5,1), (3,1), padding=(2,0))
constexpr int GC_K = 41, GC_STRIDE = 4, GC_PAD = 20, GC_CIG = 4;  // DiscriminatorS.convs[1..4]
constexpr int GC_TT = 64;                                         // outputs along t per block
constexpr int GC_NJ = GC_TT + (GC_K - 1) / GC_STRIDE;             // window samples per stride phase (74)
constexpr int GC_W = GC_NJ * GC_STRIDE;                           // window samples per channel (296 >= 63 * 4 + 41)
constexpr int GC_CK = GC_CIG * GC_K;                              // terms per output (164)

// ------------------------------------------------------------------ DiscriminatorP.forward up to fmap[0]
// Signal s of y [S][t], right reflect pad (p - t % p) % p (train.py:665), viewed [H][p] (row h, column c is sample
// h * p + c), Conv2d over H only: column c is batch element s * p + c of out [S * p][32][H1].  A lane per output row h1
// (stores coalesced along h1); the five taps are read once through the reflected index (i >= t reads y[2 (t - 1) - i];
// the host checks pad < t) and feed all 32 channels, whose weights and bias sit at wave-uniform addresses.  f32 FMA,
// taps in order 0..4, then the bias, as a conv accumulates them.
__global__ __launch_bounds__(64) void period_front_kernel(const float* __restrict__ y, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ out,
                                                          int64_t t, int p, int64_t H, int64_t H1, float slope) {
    const int64_t h1 = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int c = blockIdx.y;
    const int64_t s = blockIdx.z;
    if (h1 >= H1) return;
    const float* ys = y + s * t;
    float x[PF_K];
#pragma unroll
    for (int k = 0; k < PF_K; ++k) {
        const int64_t h = h1 * PF_STRIDE - PF_PAD + k;
        float v = 0.f;
        if (h >= 0 && h < H) {
            int64_t i = h * p + c;
            i = i >= t ? 2 * (t - 1) - i : i;
            v = ys[i];
        }
        x[k] = v;
    }
    float* o = out + ((s * p + c) * PF_CO) * H1 + h1;
#pragma unroll 4
    for (int co = 0; co < PF_CO; ++co) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < PF_K; ++k) acc = fmaf(w[co * PF_K + k], x[k], acc);
        acc += bias[co];
        o[(int64_t)co * H1] = acc >= 0.f ? acc : acc * slope;
    }
}

// ------------------------------------------------------------------ DiscriminatorS's grouped convs
// Conv1d(Ci, Co, 41, 4, groups = Ci / 4, padding = 20) + bias + LeakyReLU: every output is a 164-term dot product of
// its group's 4 input channels.  A block per (64 outputs along t, group, batch element): the group's input window
// (4 channels x 296 samples, zeros outside [0, Lin)) goes to LDS split by stride phase -- xs[c][i & 3][i >> 2] -- so
// that the 64 lanes of a wave, one output each, read consecutive words for any tap; the group's COG x 164 weights go
// to LDS as [164][COG], and wave v reads its COG / 4 rows of a term in one broadcast load.  f32 FMA, terms in the order
// channel-major, tap-minor, then the bias.
template <int COG>
__global__ __launch_bounds__(256) void gconv_small_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ y,
                                                          int64_t Ci, int64_t Co, int64_t Lin, int64_t Lout,
                                                          float slope) {
    constexpr int ROWS = COG / 4;  // rows per wave
    __shared__ float xs[GC_CIG][GC_STRIDE][GC_NJ];
    __shared__ __attribute__((aligned(16))) float wsh[GC_CK][COG];
    const int64_t t0 = (int64_t)blockIdx.x * GC_TT, g = blockIdx.y, b = blockIdx.z;
    const float* xb = x + (b * Ci + g * GC_CIG) * Lin;
    const int64_t i0 = t0 * GC_STRIDE - GC_PAD;
    for (int idx = threadIdx.x; idx < GC_CIG * GC_W; idx += 256) {
        const int c = idx / GC_W, i = idx - c * GC_W;
        const int64_t pos = i0 + i;
        xs[c][i & 3][i >> 2] = (pos >= 0 && pos < Lin) ? xb[(int64_t)c * Lin + pos] : 0.f;
    }
    const float* wg = w + g * COG * GC_CK;
    for (int idx = threadIdx.x; idx < COG * GC_CK; idx += 256) {
        const int r = idx / GC_CK, ck = idx - r * GC_CK;
        wsh[ck][r] = wg[idx];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * ROWS;
    float acc[ROWS] = {};
#pragma unroll
    for (int c = 0; c < GC_CIG; ++c) {
#pragma unroll
        for (int k = 0; k < GC_K; ++k) {
            const float v = xs[c][k & 3][lane + (k >> 2)];
            const float* wr = &wsh[c * GC_K + k][r0];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) acc[r] = fmaf(wr[r], v, acc[r]);
        }
    }
    const int64_t t = t0 + lane;
    if (t >= Lout) return;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int64_t co = g * COG + r0 + r;
        const float v = acc[r] + bias[co];
        y[(b * Co + co) * Lout + t] = v >= 0.f ? v : v * slope;
    }
}

// ------------------------------------------------------------------ the GAN losses
// feature_loss's term of one feature-map pair: mean |a - b| (train.py:290)
__global__ __launch_bounds__(256) void pair_l1_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                      int64_t n, double* __restrict__ part) {
    reduce_stage1(n, part, [&](int64_t i) -> double { return fabs((double)a[i] - (double)b[i]); });
}

// one discriminator's LSGAN terms, blockIdx.y = 0: (1 - d_r)^2, 1: d_g^2, 2: (1 - d_g)^2 (train.py:300-301, 312)
__global__ __launch_bounds__(256) void lsgan_kernel(const float* __restrict__ dr, const float* __restrict__ dg,
                                                    int64_t n, double* __restrict__ part) {
    const int which = blockIdx.y;
    reduce_stage1(n, part + which * RED_BLOCKS, [&](int64_t i) -> double {
        const double v = which == 0 ? 1.0 - (double)dr[i] : which == 1 ? (double)dg[i] : 1.0 - (double)dg[i];
        return v * v;
    });
}

// stage 2: block j adds the RED_BLOCKS partials of term j by the wave tree -> table[j] = sum / n, kept in f64
__global__ __launch_bounds__(64) void mean_stage2(const double* __restrict__ part, double n,
                                                  double* __restrict__ table) {
    static_assert(RED_BLOCKS == 64, "stage 2 is one wave over the partials");
    const double s = wave_sum64(part[blockIdx.x * RED_BLOCKS + threadIdx.x]);
    if (threadIdx.x == 0) table[blockIdx.x] = s / n;
}

// The reference's sums over the table, each mean rounded to f32 as torch.mean returns it and added in f32 in list order
// (train.py:286-315): loss_fm = 2 * sum of the n_fm pair terms; loss_disc += r_i + g_i; loss_gen += l_i;
// loss_gen_all = loss_gen + loss_fm + loss_mel + loss_kl (train.py:869), loss_mel = l1 * c_mel and loss_kl = kl * c_kl
// being f32 products.  No product may fuse into an add here.
__global__ void disc_finish_kernel(const double* __restrict__ table, int n_fm, int n_disc, const float* l1,
                                   float c_mel, const float* kl, float c_kl, float* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double* ls = table + n_fm;
    float fm = 0.f, disc = 0.f, gen = 0.f;
    for (int i = 0; i < n_fm; ++i) fm = __fadd_rn(fm, (float)table[i]);
    fm = __fmul_rn(fm, 2.f);
    float* lg = out + RVC_DISC_OUT_LISTS;
    for (int i = 0; i < n_disc; ++i) {
        const float r = (float)ls[3 * i], g = (float)ls[3 * i + 1], l = (float)ls[3 * i + 2];
        disc = __fadd_rn(disc, __fadd_rn(r, g));
        gen = __fadd_rn(gen, l);
        lg[i] = l;
        lg[n_disc + i] = r;
        lg[2 * n_disc + i] = g;
    }
    out[0] = disc;
    out[1] = gen;
    out[2] = fm;
    float all = NAN, mel = NAN, klw = NAN;
    if (l1 && kl) {
        mel = __fmul_rn(l1[0], c_mel);
        klw = __fmul_rn(kl[0], c_kl);
        all = __fadd_rn(__fadd_rn(__fadd_rn(gen, fm), mel), klw);
    }
    out[3] = all;
    out[4] = mel;
    out[5] = klw;
}

}  // namespace

extern "C" int64_t rvc_period_front_rows(int64_t t, int p) {
    if (t <= 0 || p <= 0) return -1;
    const int64_t pad = (p - t % p) % p;
    if (pad >= t) return -1;  // F.pad's reflect needs pad < t
    return ((t + pad) / p + 2 * PF_PAD - PF_K) / PF_STRIDE + 1;
}

extern "C" int rvc_period_front(const float* y, const float* w, const float* bias, float* out, int64_t S, int64_t t,
                                int p, int64_t H1, float slope, rvc_stream_t stream) {
    RVC_CHECK_ARG(y && w && bias && out, "period_front: null pointer");
    RVC_CHECK_ARG(S > 0 && S <= 65535 && p > 0 && p <= 65535 && t > 0 && t <= ((int64_t)1 << 40),
                  "period_front: bad sizes S=%lld t=%lld p=%d", (long long)S, (long long)t, p);
    const int64_t want = rvc_period_front_rows(t, p);
    RVC_CHECK_ARG(want > 0, "period_front: %lld samples do not hold the reflect pad of period %d", (long long)t, p);
    RVC_CHECK_ARG(H1 == want, "period_front: H1 = %lld, expected %lld", (long long)H1, (long long)want);
    const int64_t H = (t + (p - t % p) % p) / p;
    hipLaunchKernelGGL(period_front_kernel, dim3(cdiv(H1, 64), (unsigned)p, (unsigned)S), dim3(64), 0,
                       (hipStream_t)stream, y, w, bias, out, t, p, H, H1, slope);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_gconv_small(const float* x, const float* w, const float* bias, float* y, int64_t B, int64_t Ci,
                               int64_t Co, int64_t Lin, int64_t Lout, float slope, rvc_stream_t stream) {
    RVC_CHECK_ARG(x && w && bias && y, "gconv_small: null pointer");
    RVC_CHECK_ARG(B > 0 && B <= 65535 && Ci > 0 && Ci % GC_CIG == 0 && Ci / GC_CIG <= 65535 && Lin > 0 &&
                  Lin <= ((int64_t)1 << 32), "gconv_small: bad sizes B=%lld Ci=%lld Lin=%lld", (long long)B,
                  (long long)Ci, (long long)Lin);
    const int64_t G = Ci / GC_CIG;
    RVC_CHECK_ARG(Co == 16 * G || Co == 4 * G, "gconv_small: %lld -> %lld channels: 4 inputs per group take 16 or 4 "
                  "outputs per group", (long long)Ci, (long long)Co);
    RVC_CHECK_ARG(Lout == (Lin + 2 * GC_PAD - GC_K) / GC_STRIDE + 1, "gconv_small: Lout = %lld for Lin = %lld",
                  (long long)Lout, (long long)Lin);
    const dim3 grid(cdiv(Lout, GC_TT), (unsigned)G, (unsigned)B);
    if (Co == 16 * G)
        hipLaunchKernelGGL(gconv_small_kernel<16>, grid, dim3(256), 0, (hipStream_t)stream, x, w, bias, y, Ci, Co, Lin,
                           Lout, slope);
    else
        hipLaunchKernelGGL(gconv_small_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, x, w, bias, y, Ci, Co, Lin,
                           Lout, slope);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int64_t rvc_disc_work_bytes(void) { return (int64_t)3 * RED_BLOCKS * sizeof(double); }

extern "C" int64_t rvc_disc_table_slots(int n_fm, int n_disc) { return (int64_t)n_fm + 3 * (int64_t)n_disc; }

extern "C" int rvc_pair_l1(const float* a, const float* b, int64_t n, double* table, int64_t slot, void* work,
                           int64_t work_bytes, rvc_stream_t stream) {
    RVC_CHECK_ARG(a && b && table && work, "pair_l1: null pointer");
    RVC_CHECK_ARG(n > 0 && n <= ((int64_t)1 << 40) && slot >= 0, "pair_l1: bad size or slot");
    RVC_CHECK_ARG(work_bytes >= rvc_disc_work_bytes(), "pair_l1: work buffer too small");
    hipLaunchKernelGGL(pair_l1_kernel, dim3(RED_BLOCKS), dim3(256), 0, (hipStream_t)stream, a, b, n, (double*)work);
    hipLaunchKernelGGL(mean_stage2, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)work, (double)n,
                       table + slot);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_lsgan_terms(const float* d_r, const float* d_g, int64_t n, double* table, int64_t slot, void* work,
                               int64_t work_bytes, rvc_stream_t stream) {
    RVC_CHECK_ARG(d_r && d_g && table && work, "lsgan_terms: null pointer");
    RVC_CHECK_ARG(n > 0 && n <= ((int64_t)1 << 40) && slot >= 0, "lsgan_terms: bad size or slot");
    RVC_CHECK_ARG(work_bytes >= rvc_disc_work_bytes(), "lsgan_terms: work buffer too small");
    hipLaunchKernelGGL(lsgan_kernel, dim3(RED_BLOCKS, 3), dim3(256), 0, (hipStream_t)stream, d_r, d_g, n,
                       (double*)work);
    hipLaunchKernelGGL(mean_stage2, dim3(3), dim3(64), 0, (hipStream_t)stream, (const double*)work, (double)n,
                       table + slot);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_disc_finish(const double* table, int n_fm, int n_disc, const float* l1, float c_mel, const float* kl,
                               float c_kl, float* out, rvc_stream_t stream) {
    RVC_CHECK_ARG(table && out, "disc_finish: null pointer");
    RVC_CHECK_ARG(n_fm > 0 && n_disc > 0 && n_fm <= 4096 && n_disc <= 256, "disc_finish: bad counts");
    RVC_CHECK_ARG((l1 == nullptr) == (kl == nullptr), "disc_finish: loss_mel and loss_kl go together");
    hipLaunchKernelGGL(disc_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, table, n_fm, n_disc, l1, c_mel, kl,
                       c_kl, out);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

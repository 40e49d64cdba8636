// The discriminator half of one training step (main/inference/train.py:851-860) behind the forward of discriminator.hip:
// the gradient of discriminator_loss on a conv_post map, Conv1d backward-data and backward-weight with the LeakyReLU
// factor taken from the stored forward output on load, the weight-norm backward + AdamW update per output row, and
// grad_norm_d.  All products and sums of the convolutions are exact f32 FMA / MFMA chains in one fixed order; the
// norms, the bias gradient and the update are f64, rounded once.  No atomics: two runs give the same bits.
#include "reduce64.h"

namespace {

constexpr int BT = 64;        // block tile: 64 x 64 outputs, wave v the rows 16 v .. 16 v + 15
constexpr int BT_K = 16;      // reduction terms per stage (four 16x16x4 MFMAs per column tile)
constexpr int BT_LD = BT + 4; // LDS row pitch

// dy * LeakyReLU'(input) from the layer's stored output: an output has the sign of its input, 0 takes the slope
RVC_DEV float dyp_load(const float* __restrict__ dy, const float* __restrict__ y, int64_t idx, float slope) {
    const float g = dy[idx];
    if (!y) return g;
    return y[idx] > 0.f ? g : g * slope;
}

// acc[tn] += A[64][kd] * B[kd][64] for the block's tile: fa(m, kk) and fb(kk, n) return the operands (0 outside the
// problem), kk in [k0, k1) in ascending order -- every output is one f32 FMA chain over kk.
template <typename FA, typename FB>
RVC_DEV void gemm_tile(int k0, int k1, FA fa, FB fb, floatx4 (&acc)[4]) {
    __shared__ float As[BT_K][BT_LD];
    __shared__ float Bs[BT_K][BT_LD];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int kb = k0; kb < k1; kb += BT_K) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid & 63, kk = (tid >> 6) + 4 * i;
            const bool in = kb + kk < k1;
            As[kk][c] = in ? fa(c, kb + kk) : 0.f;
            Bs[kk][c] = in ? fb(kb + kk, c) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float a = As[4 * q + (lane >> 4)][16 * wv + (lane & 15)];
#pragma unroll
            for (int tn = 0; tn < 4; ++tn)
                acc[tn] = mfma16(a, Bs[4 * q + (lane >> 4)][16 * tn + (lane & 15)], acc[tn]);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ discriminator_loss' gradient (train.py:293-303)
// loss = mean (1 - d_r)^2 + mean d_g^2 over n values each: d [2 n], real half first
__global__ __launch_bounds__(256) void lsgan_grad_kernel(const float* __restrict__ d, float* __restrict__ dy, int64_t n,
                                                         double scale) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * n) return;
    const double v = d[i];
    dy[i] = (float)((i < n ? -2.0 * (1.0 - v) : 2.0 * v) / (double)n * scale);
}

// ------------------------------------------------------------------ backward-data
struct ConvShape {
    int B, Ci, Co, Lin, Lout, K, stride, pad, groups;
};

// Dense layers as an implicit GEMM per stride phase phi = (i + pad) % stride (blockIdx.z): M = Ci, N = (b, u) with
// i = u * stride + phi - pad, reduction over (co, tap), k = phi + tap * stride, j = u - tap.  Every i < Lin belongs to
// exactly one (phi, u), so every row of dx is written, those no output reaches as zeros.
__global__ __launch_bounds__(256) void bwd_data_mfma_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                            const float* __restrict__ w, float* __restrict__ dx,
                                                            ConvShape s, int U, float slope) {
    const int phi = blockIdx.z;
    const int T = phi < s.K ? (s.K - phi + s.stride - 1) / s.stride : 0;
    const int m0 = blockIdx.y * BT, n0 = blockIdx.x * BT, NN = s.B * U;
    floatx4 acc[4] = {};
    auto fa = [&](int m, int kk) -> float {
        const int ci = m0 + m;
        if (ci >= s.Ci) return 0.f;
        const int co = kk / T, tap = kk - co * T;
        return w[((int64_t)co * s.Ci + ci) * s.K + phi + tap * s.stride];
    };
    auto fb = [&](int kk, int n) -> float {
        const int nn = n0 + n;
        if (nn >= NN) return 0.f;
        const int b = nn / U, u = nn - b * U;
        const int co = kk / T, tap = kk - co * T;
        const int j = u - tap;
        if (j < 0 || j >= s.Lout) return 0.f;
        return dyp_load(dy, y, ((int64_t)b * s.Co + co) * s.Lout + j, slope);
    };
    gemm_tile(0, s.Co * T, fa, fb, acc);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
        const int nn = n0 + 16 * tn + (lane & 15);
        if (nn >= NN) continue;
        const int b = nn / U, u = nn - b * U;
        const int i = u * s.stride + phi - s.pad;
        if (i < 0 || i >= s.Lin) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ci = m0 + 16 * wv + (lane >> 4) * 4 + r;
            if (ci < s.Ci) dx[((int64_t)b * s.Ci + ci) * s.Lin + i] = acc[tn][r];
        }
    }
}

// Grouped layers directly: a thread per dx[b][ci][i], terms in the order output channel-major, tap-minor.  With 4 input
// channels per group a GEMM tile would be 1/16 full (the reason rvc_gconv_small is direct).
__global__ __launch_bounds__(256) void bwd_data_direct_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                              const float* __restrict__ w, float* __restrict__ dx,
                                                              ConvShape s, float slope) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)s.B * s.Ci * s.Lin) return;
    const int i = (int)(idx % s.Lin);
    const int ci = (int)((idx / s.Lin) % s.Ci), b = (int)(idx / ((int64_t)s.Lin * s.Ci));
    const int cig = s.Ci / s.groups, cog = s.Co / s.groups, g = ci / cig, c = ci - g * cig;
    const int phi = (i + s.pad) % s.stride;
    float acc = 0.f;
    for (int o = 0; o < cog; ++o) {
        const int co = g * cog + o;
        const float* wr = w + ((int64_t)co * cig + c) * s.K;
        const int64_t row = ((int64_t)b * s.Co + co) * s.Lout;
        for (int k = phi; k < s.K; k += s.stride) {
            const int j = (i + s.pad - k) / s.stride;
            if (i + s.pad - k >= 0 && j < s.Lout) acc = fmaf(wr[k], dyp_load(dy, y, row + j, slope), acc);
        }
    }
    dx[idx] = acc;
}

// ------------------------------------------------------------------ backward-weight
// Dense layers: M = Co, N = (ci, k) in dW's own order, reduction over r = (b, j); blockIdx.z takes the z-th chunk of
// the reduction and writes part[z][co][ci * K + k]; bwd_weight_stage2 adds the chunks in order.
__global__ __launch_bounds__(256) void bwd_weight_mfma_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                              const float* __restrict__ x, float* __restrict__ part,
                                                              ConvShape s, int chunk, float slope) {
    const int m0 = blockIdx.y * BT, n0 = blockIdx.x * BT, NN = s.Ci * s.K, R = s.B * s.Lout;
    const int r0 = blockIdx.z * chunk, r1 = min(R, r0 + chunk);
    floatx4 acc[4] = {};
    auto fa = [&](int m, int r) -> float {
        const int co = m0 + m;
        if (co >= s.Co) return 0.f;
        const int b = r / s.Lout, j = r - b * s.Lout;
        return dyp_load(dy, y, ((int64_t)b * s.Co + co) * s.Lout + j, slope);
    };
    auto fb = [&](int r, int n) -> float {
        const int nn = n0 + n;
        if (nn >= NN) return 0.f;
        const int ci = nn / s.K, k = nn - ci * s.K;
        const int b = r / s.Lout, j = r - b * s.Lout;
        const int i = j * s.stride + k - s.pad;
        if (i < 0 || i >= s.Lin) return 0.f;
        return x[((int64_t)b * s.Ci + ci) * s.Lin + i];
    };
    gemm_tile(r0, r1, fa, fb, acc);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
        const int nn = n0 + 16 * tn + (lane & 15);
        if (nn >= NN) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = m0 + 16 * wv + (lane >> 4) * 4 + r;
            if (co < s.Co) part[((int64_t)blockIdx.z * s.Co + co) * NN + nn] = acc[tn][r];
        }
    }
}

// Grouped layers and the two first layers directly: a block per (output channel, chunk), a thread per (c, k) of the
// channel's Ci / groups x K weights, its chunk's terms in order.  PERIOD: x is DiscriminatorP's view of the signal
// sig [S][t] -- batch element b is column b % p of signal b / p, row i is sample i * p + column, reflected about the
// last sample once past it (rvc_period_front's index); Lin is the view's row count H.
template <bool PERIOD>
__global__ __launch_bounds__(256) void bwd_weight_direct_kernel(const float* __restrict__ dy,
                                                                const float* __restrict__ y,
                                                                const float* __restrict__ x, float* __restrict__ part,
                                                                ConvShape s, int chunk, float slope, int64_t t, int p) {
    const int co = blockIdx.x, cig = s.Ci / s.groups, cog = s.Co / s.groups, g = co / cog;
    const int NN = cig * s.K, R = s.B * s.Lout;
    const int r0 = blockIdx.y * chunk, r1 = min(R, r0 + chunk);
    for (int n = threadIdx.x; n < NN; n += 256) {
        const int c = n / s.K, k = n - c * s.K;
        float acc = 0.f;
        int b = r0 / s.Lout, j = r0 - b * s.Lout;
        for (int r = r0; r < r1; ++r) {
            const int i = j * s.stride + k - s.pad;
            if (i >= 0 && i < s.Lin) {
                float xv;
                if (PERIOD) {
                    const int sg = b / p, col = b - sg * p;
                    int64_t q = (int64_t)i * p + col;
                    q = q >= t ? 2 * (t - 1) - q : q;
                    xv = x[sg * t + q];
                } else {
                    xv = x[((int64_t)b * s.Ci + g * cig + c) * s.Lin + i];
                }
                acc = fmaf(dyp_load(dy, y, ((int64_t)b * s.Co + co) * s.Lout + j, slope), xv, acc);
            }
            if (++j == s.Lout) {
                j = 0;
                ++b;
            }
        }
        part[((int64_t)blockIdx.y * s.Co + co) * NN + n] = acc;
    }
}

// dW[e] (+)= scale * (part[0][e] + part[1][e] + ...), the chunks added in order in f32
__global__ __launch_bounds__(256) void bwd_weight_stage2(const float* __restrict__ part, float* __restrict__ dW,
                                                         int64_t n, int nsplit, float scale, int accumulate) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float sum = part[e];
    for (int z = 1; z < nsplit; ++z) sum = __fadd_rn(sum, part[(int64_t)z * n + e]);
    sum = __fmul_rn(sum, scale);
    dW[e] = accumulate ? __fadd_rn(dW[e], sum) : sum;
}

// db[co] (+)= scale * sum over (b, j) of dyp: a block per channel, an f64 sum in a fixed order, rounded once
__global__ __launch_bounds__(256) void bwd_bias_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                       float* __restrict__ db, ConvShape s, float slope, float scale,
                                                       int accumulate) {
    __shared__ double ws[4];
    const int co = blockIdx.x, R = s.B * s.Lout;
    double sum = 0.0;
    for (int r = threadIdx.x; r < R; r += 256) {
        const int b = r / s.Lout, j = r - b * s.Lout;
        sum += (double)dyp_load(dy, y, ((int64_t)b * s.Co + co) * s.Lout + j, slope);
    }
    sum = wave_sum64(sum);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float v = (float)(((ws[0] + ws[1]) + (ws[2] + ws[3])) * (double)scale);
        db[co] = accumulate ? __fadd_rn(db[co], v) : v;
    }
}

// ------------------------------------------------------------------ weight-norm backward + AdamW
struct AdamW {
    double lr, beta1, beta2, eps, wd, step_size, bc2_sqrt;  // step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t)
};

// torch.optim.AdamW's update of one value (amsgrad False), in f64 from the f32 states, each result rounded once
RVC_DEV void adamw_update(float* p, float* m, float* v, double grad, const AdamW& h) {
    const double pm = (double)*p * (1.0 - h.lr * h.wd);
    const double mm = h.beta1 * (double)*m + (1.0 - h.beta1) * grad;
    const double vv = h.beta2 * (double)*v + (1.0 - h.beta2) * grad * grad;
    *m = (float)mm;
    *v = (float)vv;
    *p = (float)(pm - h.step_size * mm / (sqrt(vv) / h.bc2_sqrt + h.eps));
}

RVC_DEV double block_sum64(double v, double* ws) {
    v = wave_sum64(v);
    __syncthreads();  // ws may still be read from the sum before
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    return (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// A block per output row of one conv: w = g v / |v| (torch._weight_norm(v, g, 0)), so dg = <dW, v> / |v| and
// dv = g / |v| (dW - v dg / |v|); the row's |dg|^2, |dv|^2, |db|^2 go to table[row][0..2]; then g, v and the bias
// take their AdamW update in place.
__global__ __launch_bounds__(256) void wn_adamw_kernel(const float* __restrict__ dW, const float* __restrict__ db,
                                                       float* __restrict__ v, float* __restrict__ g,
                                                       float* __restrict__ bias, float* __restrict__ m_v,
                                                       float* __restrict__ s_v, float* __restrict__ m_g,
                                                       float* __restrict__ s_g, float* __restrict__ m_b,
                                                       float* __restrict__ s_b, int64_t n, AdamW h,
                                                       double* __restrict__ table) {
    __shared__ double ws[4];
    const int64_t row = blockIdx.x;
    const float* dWr = dW + row * n;
    float* vr = v + row * n;
    double nn = 0.0, dot = 0.0;
    for (int64_t e = threadIdx.x; e < n; e += 256) {
        const double ve = vr[e];
        nn += ve * ve;
        dot += (double)dWr[e] * ve;
    }
    nn = block_sum64(nn, ws);
    dot = block_sum64(dot, ws);
    const double norm = sqrt(nn), dg = dot / norm, gv = g[row], c0 = gv / norm, c1 = dg / norm;
    double sq = 0.0;
    for (int64_t e = threadIdx.x; e < n; e += 256) {
        const double dv = c0 * ((double)dWr[e] - (double)vr[e] * c1);
        sq += dv * dv;
        adamw_update(vr + e, m_v + row * n + e, s_v + row * n + e, dv, h);
    }
    sq = block_sum64(sq, ws);  // its barriers also order every read of g[row] above before the write below
    if (threadIdx.x == 0) {
        const double gb = db[row];
        table[3 * row] = dg * dg;
        table[3 * row + 1] = sq;
        table[3 * row + 2] = gb * gb;
        adamw_update(g + row, m_g + row, s_g + row, dg, h);
        adamw_update(bias + row, m_b + row, s_b + row, gb, h);
    }
}

__global__ __launch_bounds__(256) void table_sum_kernel(const double* __restrict__ table, int64_t n,
                                                        double* __restrict__ part) {
    reduce_stage1(n, part, [&](int64_t i) -> double { return table[i]; });
}

// clip_grad_value(parameters, None)'s return (commons.py:48-60): sqrt of the sum of every parameter's |grad|^2
__global__ __launch_bounds__(64) void grad_norm_stage2(const double* __restrict__ part, double* __restrict__ out) {
    static_assert(RED_BLOCKS == 64, "stage 2 is one wave over the partials");
    const double s = wave_sum64(part[threadIdx.x]);
    if (threadIdx.x == 0) out[0] = sqrt(s);
}

constexpr int64_t BW_WORK_CAP = (int64_t)64 << 20;  // bytes of chunk partials a launch asks for at the most
constexpr int BW_CHUNK_MFMA = 512, BW_CHUNK_DIRECT = 256, BW_SPLIT_MAX = 64;

bool dense(const ConvShape& s) { return s.groups == 1 && s.Ci >= 16; }

int64_t weight_count(const ConvShape& s) { return (int64_t)s.Co * (s.Ci / s.groups) * s.K; }

// chunks of the reduction over R = B * Lout terms: by the chunk length aimed at, at most what `bytes` holds
int bw_splits(const ConvShape& s, int64_t bytes) {
    const int64_t R = (int64_t)s.B * s.Lout, target = dense(s) ? BW_CHUNK_MFMA : BW_CHUNK_DIRECT;
    int64_t ns = (R + target - 1) / target;
    if (ns > BW_SPLIT_MAX) ns = BW_SPLIT_MAX;
    const int64_t fit = bytes / (weight_count(s) * (int64_t)sizeof(float));
    if (ns > fit) ns = fit;
    return (int)ns;
}

int check_shape(const char* what, const ConvShape& s) {
    RVC_CHECK_ARG(s.B > 0 && s.Ci > 0 && s.Co > 0 && s.Lin > 0 && s.Lout > 0 && s.K > 0 && s.stride > 0 && s.pad >= 0 &&
                  s.groups > 0, "%s: sizes must be positive", what);
    RVC_CHECK_ARG(s.Ci % s.groups == 0 && s.Co % s.groups == 0, "%s: %d -> %d channels in %d groups", what, s.Ci, s.Co,
                  s.groups);
    RVC_CHECK_ARG(s.stride <= 65535 && s.K <= 4096 && s.pad <= 4096, "%s: stride %d, kernel %d, pad %d", what, s.stride,
                  s.K, s.pad);
    RVC_CHECK_ARG((int64_t)s.Lin + 2 * s.pad >= s.K && s.Lout == (s.Lin + 2 * s.pad - s.K) / s.stride + 1,
                  "%s: Lout = %d for Lin = %d (k %d, stride %d, pad %d)", what, s.Lout, s.Lin, s.K, s.stride, s.pad);
    const int64_t lim = (int64_t)1 << 30;  // the kernels index (b, position), (co, tap) and (ci, k) in 32 bits
    RVC_CHECK_ARG((int64_t)s.B * (s.Lin + s.pad + s.stride) < lim && (int64_t)s.B * s.Lout < lim &&
                  (int64_t)s.Co * s.K < lim && (int64_t)s.Ci * s.K < lim, "%s: sizes past the 32-bit index range", what);
    return RVC_OK;
}

ConvShape make_shape(int64_t B, int64_t Ci, int64_t Co, int64_t Lin, int64_t Lout, int K, int stride, int pad,
                     int groups) {
    const int64_t lim = (int64_t)1 << 30;
    auto cl = [&](int64_t v) { return (int)(v < 0 || v > lim ? -1 : v); };  // out of range -> refused by check_shape
    return ConvShape{cl(B), cl(Ci), cl(Co), cl(Lin), cl(Lout), K, stride, pad, groups};
}

}  // namespace

extern "C" int rvc_lsgan_grad(const float* d, float* dy, int64_t n, float scale, rvc_stream_t stream) {
    RVC_CHECK_ARG(d && dy, "lsgan_grad: null pointer");
    RVC_CHECK_ARG(n > 0 && n <= ((int64_t)1 << 36), "lsgan_grad: bad size %lld", (long long)n);
    hipLaunchKernelGGL(lsgan_grad_kernel, dim3(cdiv(2 * n, 256)), dim3(256), 0, (hipStream_t)stream, d, dy, n,
                       (double)scale);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_conv_bwd_data(const float* dy, const float* y, const float* w, float* dx, int64_t B, int64_t Ci,
                                 int64_t Co, int64_t Lin, int64_t Lout, int K, int stride, int pad, int groups,
                                 float slope, rvc_stream_t stream) {
    RVC_CHECK_ARG(dy && w && dx, "conv_bwd_data: null pointer");
    const ConvShape s = make_shape(B, Ci, Co, Lin, Lout, K, stride, pad, groups);
    if (int rc = check_shape("conv_bwd_data", s)) return rc;
    if (dense(s)) {
        const int U = (s.Lin - 1 + s.pad) / s.stride + 1;
        const int64_t nx = ((int64_t)s.B * U + BT - 1) / BT, ny = (s.Ci + BT - 1) / BT;
        RVC_CHECK_ARG(ny <= 65535, "conv_bwd_data: %d input channels", s.Ci);
        hipLaunchKernelGGL(bwd_data_mfma_kernel, dim3((unsigned)nx, (unsigned)ny, (unsigned)s.stride), dim3(256), 0,
                           (hipStream_t)stream, dy, y, w, dx, s, U, slope);
    } else {
        hipLaunchKernelGGL(bwd_data_direct_kernel, dim3(cdiv((int64_t)s.B * s.Ci * s.Lin, 256)), dim3(256), 0,
                           (hipStream_t)stream, dy, y, w, dx, s, slope);
    }
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int64_t rvc_conv_bwd_weight_work_bytes(int64_t B, int64_t Ci, int64_t Co, int64_t Lout, int K, int groups) {
    if (B <= 0 || Ci <= 0 || Co <= 0 || Lout <= 0 || K <= 0 || groups <= 0 || Ci % groups) return -1;
    const ConvShape s = make_shape(B, Ci, Co, 1, Lout, K, 1, 0, groups);
    if (s.B < 0 || s.Ci < 0 || s.Co < 0 || s.Lout < 0 || (int64_t)s.B * s.Lout >= ((int64_t)1 << 30)) return -1;
    const int64_t one = weight_count(s) * (int64_t)sizeof(float);
    const int ns = bw_splits(s, BW_WORK_CAP > one ? BW_WORK_CAP : one);
    return one * ns;
}

// x: the layer's input [B][Ci][Lin]; with period > 0 the signals [B / period][t] that DiscriminatorP views as
// [B][1][Lin] (Ci = 1, Lin = the padded length / period)
extern "C" int rvc_conv_bwd_weight(const float* dy, const float* y, const float* x, float* dW, float* db, int64_t B,
                                   int64_t Ci, int64_t Co, int64_t Lin, int64_t Lout, int K, int stride, int pad,
                                   int groups, float slope, float scale, int accumulate, int period, int64_t t,
                                   void* work, int64_t work_bytes, rvc_stream_t stream) {
    RVC_CHECK_ARG(dy && x && dW && db && work, "conv_bwd_weight: null pointer");
    const ConvShape s = make_shape(B, Ci, Co, Lin, Lout, K, stride, pad, groups);
    if (int rc = check_shape("conv_bwd_weight", s)) return rc;
    RVC_CHECK_ARG(s.Co <= 65535, "conv_bwd_weight: %d output channels", s.Co);
    if (period > 0) {
        RVC_CHECK_ARG(s.Ci == 1 && s.groups == 1 && s.B % period == 0 && t > 0, "conv_bwd_weight: the period view is one "
                      "channel of B = signals x period columns");
        const int64_t padn = (period - t % period) % period;
        RVC_CHECK_ARG(padn < t && (t + padn) / period == s.Lin, "conv_bwd_weight: %lld samples at period %d are not %d "
                      "rows", (long long)t, period, s.Lin);
    }
    const int ns = bw_splits(s, work_bytes);
    RVC_CHECK_ARG(ns >= 1, "conv_bwd_weight: work buffer too small");
    const int R = s.B * s.Lout;
    float* part = (float*)work;
    const int64_t nw = weight_count(s);
    if (dense(s) && period <= 0) {
        int chunk = (R + ns - 1) / ns;
        chunk = (chunk + BT_K - 1) / BT_K * BT_K;
        const int nz = (R + chunk - 1) / chunk;
        const int64_t nx = ((int64_t)s.Ci * s.K + BT - 1) / BT, ny = (s.Co + BT - 1) / BT;
        hipLaunchKernelGGL(bwd_weight_mfma_kernel, dim3((unsigned)nx, (unsigned)ny, (unsigned)nz), dim3(256), 0,
                           (hipStream_t)stream, dy, y, x, part, s, chunk, slope);
        hipLaunchKernelGGL(bwd_weight_stage2, dim3(cdiv(nw, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const float*)part, dW, nw, nz, scale, accumulate);
    } else {
        const int chunk = (R + ns - 1) / ns, nz = (R + chunk - 1) / chunk;
        if (period > 0)
            hipLaunchKernelGGL(bwd_weight_direct_kernel<true>, dim3((unsigned)s.Co, (unsigned)nz), dim3(256), 0,
                               (hipStream_t)stream, dy, y, x, part, s, chunk, slope, t, period);
        else
            hipLaunchKernelGGL(bwd_weight_direct_kernel<false>, dim3((unsigned)s.Co, (unsigned)nz), dim3(256), 0,
                               (hipStream_t)stream, dy, y, x, part, s, chunk, slope, (int64_t)0, 1);
        hipLaunchKernelGGL(bwd_weight_stage2, dim3(cdiv(nw, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const float*)part, dW, nw, nz, scale, accumulate);
    }
    hipLaunchKernelGGL(bwd_bias_kernel, dim3((unsigned)s.Co), dim3(256), 0, (hipStream_t)stream, dy, y, db, s, slope,
                       scale, accumulate);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_wn_adamw(const float* dW, const float* db, float* v, float* g, float* bias, float* m_v, float* s_v,
                            float* m_g, float* s_g, float* m_b, float* s_b, int64_t Co, int64_t n, double lr,
                            double beta1, double beta2, double eps, double weight_decay, int64_t step, double* table,
                            rvc_stream_t stream) {
    RVC_CHECK_ARG(dW && db && v && g && bias && m_v && s_v && m_g && s_g && m_b && s_b && table,
                  "wn_adamw: null pointer");
    RVC_CHECK_ARG(Co > 0 && Co <= ((int64_t)1 << 30) && n > 0 && n <= ((int64_t)1 << 32), "wn_adamw: bad sizes");
    RVC_CHECK_ARG(step >= 1 && lr >= 0 && beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps >= 0 &&
                  weight_decay >= 0, "wn_adamw: bad hyper-parameters (step counts from 1)");
    AdamW h;
    h.lr = lr, h.beta1 = beta1, h.beta2 = beta2, h.eps = eps, h.wd = weight_decay;
    h.step_size = lr / (1.0 - pow(beta1, (double)step));
    h.bc2_sqrt = sqrt(1.0 - pow(beta2, (double)step));
    hipLaunchKernelGGL(wn_adamw_kernel, dim3((unsigned)Co), dim3(256), 0, (hipStream_t)stream, dW, db, v, g, bias, m_v,
                       s_v, m_g, s_g, m_b, s_b, n, h, table);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_grad_norm(const double* table, int64_t n, double* out, void* work, int64_t work_bytes,
                             rvc_stream_t stream) {
    RVC_CHECK_ARG(table && out && work, "grad_norm: null pointer");
    RVC_CHECK_ARG(n > 0 && n <= ((int64_t)1 << 40), "grad_norm: bad size");
    RVC_CHECK_ARG(work_bytes >= (int64_t)RED_BLOCKS * (int64_t)sizeof(double), "grad_norm: work buffer too small");
    hipLaunchKernelGGL(table_sum_kernel, dim3(RED_BLOCKS), dim3(256), 0, (hipStream_t)stream, table, n, (double*)work);
    hipLaunchKernelGGL(grad_norm_stage2, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)work, out);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

// Performer (FAVOR+) self-attention of the fcpe-legacy f0 model (main/library/predictors/FCPE.py: softmax_kernel
// :108-116, linear_attention :87-88, FastAttention.forward :576-583): non-causal, no mask, 64 channels per head.
//   dq[t][j] = c q[t] . P[j]     gq[t] = 0.5 c^2 |q[t]|^2            c = 64^-0.25, r = M^-0.5
//   q'[t][j] = r (exp(dq - gq - max_j dq) + 1e-4)      k'[t][j] = r exp(dk - gk + 1e-4)
//   out[t]   = (q'[t] . ctx) / (q'[t] . ksum + 1e-8)   ctx = k'^T v, ksum = sum_t k'
// Three launches: a key pass (a block per (chunk of time tiles, head, batch element) accumulates its share of ctx and
// ksum in registers and writes one partial), a reduction of the partials in chunk order (no float atomics: two calls
// give the same bits), and a query pass (a block per time tile).  Every product is the f32-input MFMA
// (16x16x4: an f32 fma chain); the feature dimension is padded to a multiple of 16 and the padded columns are
// held at zero in k' and q' and left out of the row maximum.
#include "rvc_common.h"

namespace {

constexpr int PD = 64, TILE = RVC_PERFORMER_TILE, MMAX = RVC_PERFORMER_MAX_FEATURES, MAX_CHUNKS = 32;
constexpr int XS = TILE + 1;  // staged q / k rows [d][t]: an odd stride spreads the d = 16 g + s reads over the banks
constexpr int VS = TILE + 4;  // v rows [e][t] and k' rows [j][t], read at t = 4 s + g
constexpr int QS = TILE + 8;  // q' rows [j][t], read at j = jj + g
constexpr int NJ = (MMAX / 16 + 3) / 4;  // feature tiles per wave, at most
constexpr float CNORM = 0.35355339059327373f;  // 64^-0.25
static_assert(TILE == 32 && MMAX % 16 == 0, "the staging and the wave split assume 32 time steps");

// rows [64][TILE] of a channels-first head (row stride ld) from t0 on -> xs = c * x (zero past T) and
// g[t] = 0.5 c^2 sum_d x^2.  Ends with a barrier.
RVC_DEV void stage_scaled(const float* __restrict__ x, int64_t ld, int64_t t0, int64_t T, float (*xs)[XS],
                          float (*gp)[TILE], float* g) {
    const int t = threadIdx.x & 31, d0 = threadIdx.x >> 5;
    const bool in = t0 + t < T;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int d = d0 + 8 * i;
        const float v = in ? x[d * ld + t0 + t] : 0.f;
        ss = fmaf(v, v, ss);
        xs[d][t] = CNORM * v;
    }
    gp[d0][t] = ss;
    __syncthreads();
    if (threadIdx.x < TILE) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += gp[i][t];
        g[t] = (s * 0.5f) * 0.125f;
    }
    __syncthreads();
}

// acc[tt] = P[16 jt .. 16 jt + 15] times the staged tile: D row j = 16 jt + 4 (lane >> 4) + r, column
// t = 16 tt + (lane & 15).  Rows past M read row M - 1 (the caller discards them).  k index d = 16 g + s: a lane's
// 16 operands of P are one contiguous 64-byte run.
RVC_DEV void dash(const float* __restrict__ P, int M, int jt, const float (*xs)[XS], floatx4 acc[2]) {
    const int lane = threadIdx.x & 63, g = lane >> 4, c15 = lane & 15;
    int row = jt * 16 + c15;
    row = row < M ? row : M - 1;
    const float4* pr = (const float4*)(P + row * PD + g * 16);
    float a[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = pr[q];
        a[4 * q] = v.x;
        a[4 * q + 1] = v.y;
        a[4 * q + 2] = v.z;
        a[4 * q + 3] = v.w;
    }
    acc[0] = acc[1] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        acc[0] = mfma16(a[s], xs[g * 16 + s][c15], acc[0]);
        acc[1] = mfma16(a[s], xs[g * 16 + s][16 + c15], acc[1]);
    }
}

// ------------------------------------------------------------------ key pass
// part[(chunk * BH + bh)] = [MT * 16][64] ctx, then [MT * 16] ksum, over the chunk's time tiles
__global__ __launch_bounds__(256) void performer_key_kernel(const float* __restrict__ k, const float* __restrict__ v,
                                                            const float* __restrict__ P, float* __restrict__ part,
                                                            int64_t T, int M, int MT, int64_t ld, int64_t bs,
                                                            int64_t per, float ratio) {
    __shared__ float xs[PD][XS], vs[PD][VS], kp[4][16][VS], gp[8][TILE], g[TILE];
    const int64_t b = blockIdx.z, h = blockIdx.y, H = gridDim.y;
    const float* kb = k + b * bs + h * PD * ld;
    const float* vb = v + b * bs + h * PD * ld;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gq = lane >> 4, c15 = lane & 15;
    floatx4 acc[NJ][4];
    float ks[NJ];
#pragma unroll
    for (int ji = 0; ji < NJ; ++ji) {
        ks[ji] = 0.f;
#pragma unroll
        for (int et = 0; et < 4; ++et) acc[ji][et] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    const int64_t ntile = (T + TILE - 1) / TILE;
    const int64_t tile0 = blockIdx.x * per, tile1 = tile0 + per < ntile ? tile0 + per : ntile;
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t t0 = tile * TILE;
        __syncthreads();  // the last tile's readers of xs / vs are done
        {
            const int t = threadIdx.x & 31, d0 = threadIdx.x >> 5;
            const bool in = t0 + t < T;
#pragma unroll
            for (int i = 0; i < 8; ++i) vs[d0 + 8 * i][t] = in ? vb[(d0 + 8 * i) * ld + t0 + t] : 0.f;
        }
        stage_scaled(kb, ld, t0, T, xs, gp, g);
#pragma unroll
        for (int ji = 0; ji < NJ; ++ji) {
            const int jt = wave + 4 * ji;
            if (jt < MT) {  // the same for every lane of the wave
                floatx4 d2[2];
                dash(P, M, jt, xs, d2);
#pragma unroll
                for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = jt * 16 + 4 * gq + r, t = tt * 16 + c15;
                        const bool live = j < M && t0 + t < T;
                        kp[wave][4 * gq + r][t] = live ? ratio * expf(d2[tt][r] - g[t] + 1e-4f) : 0.f;
                    }
                __builtin_amdgcn_wave_barrier();  // kp[wave] is this wave's own: written and read in program order
#pragma unroll
                for (int s = 0; s < TILE / 4; ++s) {
                    const float a = kp[wave][c15][4 * s + gq];
#pragma unroll
                    for (int et = 0; et < 4; ++et)
                        acc[ji][et] = mfma16(a, vs[et * 16 + c15][4 * s + gq], acc[ji][et]);
                }
                if (gq == 0) {
                    float s = 0.f;
#pragma unroll
                    for (int t = 0; t < TILE; ++t) s += kp[wave][c15][t];
                    ks[ji] += s;
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    const int64_t R = (int64_t)MT * 16 * (PD + 1);
    float* dst = part + ((int64_t)blockIdx.x * gridDim.z * H + b * H + h) * R;
#pragma unroll
    for (int ji = 0; ji < NJ; ++ji) {
        const int jt = wave + 4 * ji;
        if (jt < MT) {
#pragma unroll
            for (int et = 0; et < 4; ++et)
#pragma unroll
                for (int r = 0; r < 4; ++r) dst[(jt * 16 + 4 * gq + r) * PD + et * 16 + c15] = acc[ji][et][r];
            if (gq == 0) dst[MT * 16 * PD + jt * 16 + c15] = ks[ji];
        }
    }
}

// fin[bh][i] = sum over the chunks, in chunk order
__global__ __launch_bounds__(256) void performer_reduce_kernel(const float* __restrict__ part, float* __restrict__ fin,
                                                               int64_t R, int64_t BH, int nchunks) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, bh = blockIdx.y;
    if (i >= R) return;
    float s = 0.f;
    for (int c = 0; c < nchunks; ++c) s += part[(c * BH + bh) * R + i];
    fin[bh * R + i] = s;
}

// ------------------------------------------------------------------ query pass
__global__ __launch_bounds__(256) void performer_query_kernel(const float* __restrict__ q, const float* __restrict__ P,
                                                              const float* __restrict__ fin, float* __restrict__ out,
                                                              int64_t T, int M, int MT, int64_t ld, int64_t in_bs,
                                                              int64_t out_bs, float ratio) {
    __shared__ float xs[PD][XS], qp[MMAX][QS], gp[8][TILE], g[TILE], mx[TILE], inv[TILE], ksm[MMAX];
    const int64_t b = blockIdx.z, h = blockIdx.y, H = gridDim.y;
    const int64_t t0 = (int64_t)blockIdx.x * TILE;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gq = lane >> 4, c15 = lane & 15;
    const int tl = threadIdx.x & 31, p8 = threadIdx.x >> 5;
    const int MP = MT * 16;
    const float* ctx = fin + (b * H + h) * (int64_t)MP * (PD + 1);
    for (int j = threadIdx.x; j < MP; j += 256) ksm[j] = ctx[MP * PD + j];
    stage_scaled(q + b * in_bs + h * PD * ld, ld, t0, T, xs, gp, g);
    for (int jt = wave; jt < MT; jt += 4) {
        floatx4 d2[2];
        dash(P, M, jt, xs, d2);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) qp[jt * 16 + 4 * gq + r][tt * 16 + c15] = d2[tt][r];
    }
    __syncthreads();
    // the row maximum over the M real features
    float m = -INFINITY;
    for (int j = p8; j < M; j += 8) m = fmaxf(m, qp[j][tl]);
    gp[p8][tl] = m;
    __syncthreads();
    if (threadIdx.x < TILE) {
#pragma unroll
        for (int i = 1; i < 8; ++i) m = fmaxf(m, gp[i][tl]);
        mx[tl] = m;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < MP * TILE; idx += 256) {
        const int j = idx >> 5, t = idx & 31;
        qp[j][t] = j < M ? ratio * (expf(qp[j][t] - g[t] - mx[t]) + 1e-4f) : 0.f;
    }
    __syncthreads();
    // the denominator q' . ksum, eight interleaved partial sums added in a fixed order
    float s = 0.f;
    for (int j = p8; j < M; j += 8) s = fmaf(qp[j][tl], ksm[j], s);
    gp[p8][tl] = s;
    // the numerator q' ctx: a wave owns 16 time steps and 32 of the 64 output channels
    const int tw = wave & 1, eh = wave >> 1;
    floatx4 acc[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
    for (int jj = 0; jj < MP; jj += 4) {
        const float a = qp[jj + gq][tw * 16 + c15];
        const float* cr = ctx + (jj + gq) * PD + eh * 32 + c15;
        acc[0] = mfma16(a, cr[0], acc[0]);
        acc[1] = mfma16(a, cr[16], acc[1]);
    }
    __syncthreads();
    if (threadIdx.x < TILE) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) d += gp[i][tl];
        inv[tl] = 1.f / (d + 1e-8f);
    }
    __syncthreads();
    // through LDS (xs is free since the projections) so that the stores run along time
#pragma unroll
    for (int e2 = 0; e2 < 2; ++e2)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = tw * 16 + 4 * gq + r;
            xs[eh * 32 + e2 * 16 + c15][t] = acc[e2][r] * inv[t];
        }
    __syncthreads();
    if (t0 + tl < T) {
        float* ob = out + b * out_bs + h * PD * ld + t0 + tl;
#pragma unroll
        for (int i = 0; i < 8; ++i) ob[(p8 + 8 * i) * ld] = xs[p8 + 8 * i][tl];
    }
}

int64_t chunk_tiles(int64_t T) {  // time tiles per key-pass block: at most MAX_CHUNKS blocks per head
    const int64_t ntile = cdiv(T, TILE);
    return cdiv(ntile, MAX_CHUNKS);
}

bool shape_ok(int64_t B, int64_t H, int64_t T, int M) {
    return B >= 1 && B <= 65535 && H >= 1 && H <= 65535 && T >= 1 && T < (1ll << 31) && M >= 1 && M <= MMAX;
}

}  // namespace

extern "C" int64_t rvc_performer_work_bytes(int64_t B, int64_t H, int64_t T, int M) {
    if (!shape_ok(B, H, T, M)) return -1;
    const int64_t R = (int64_t)cdiv(M, 16) * 16 * (PD + 1);
    const int64_t nchunks = cdiv(cdiv(T, TILE), chunk_tiles(T));
    return (1 + nchunks) * B * H * R * (int64_t)sizeof(float);
}

extern "C" int rvc_performer_attention(const float* q, const float* k, const float* v, const float* proj, float* out,
                                       int64_t B, int64_t H, int64_t T, int D, int M, int64_t ldc, int64_t in_bs,
                                       int64_t out_bs, void* work, int64_t work_bytes, rvc_stream_t stream) {
    RVC_CHECK_ARG(q && k && v && proj && out && work, "performer_attention: null pointer");
    RVC_CHECK_ARG(D == PD, "performer_attention: D=%d (64 channels per head)", D);
    RVC_CHECK_ARG(M >= 1 && M <= MMAX, "performer_attention: M=%d features (1..%d)", M, MMAX);
    RVC_CHECK_ARG(shape_ok(B, H, T, M), "performer_attention: bad shape B=%lld H=%lld T=%lld", (long long)B,
                  (long long)H, (long long)T);
    if (ldc == 0) ldc = T;
    if (in_bs == 0) in_bs = H * PD * ldc;
    if (out_bs == 0) out_bs = H * PD * ldc;
    RVC_CHECK_ARG(ldc >= T && in_bs >= H * PD * ldc && out_bs >= H * PD * ldc,
                  "performer_attention: bad strides ldc=%lld in_bs=%lld out_bs=%lld", (long long)ldc, (long long)in_bs,
                  (long long)out_bs);
    RVC_CHECK_ARG(((uintptr_t)proj & 15) == 0 && ((uintptr_t)work & 15) == 0,
                  "performer_attention: proj and work must be 16-byte aligned");
    RVC_CHECK_ARG(work_bytes >= rvc_performer_work_bytes(B, H, T, M), "performer_attention: work buffer too small");
    const int MT = (int)cdiv(M, 16);
    const int64_t R = (int64_t)MT * 16 * (PD + 1), BH = B * H;
    const int64_t per = chunk_tiles(T), nchunks = cdiv(cdiv(T, TILE), per);
    const float ratio = (float)(1.0 / sqrt((double)M));
    float* fin = (float*)work;
    float* part = fin + BH * R;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(performer_key_kernel, dim3((unsigned)nchunks, (unsigned)H, (unsigned)B), dim3(256), 0, s, k, v,
                       proj, part, T, M, MT, ldc, in_bs, per, ratio);
    hipLaunchKernelGGL(performer_reduce_kernel, dim3((unsigned)cdiv(R, 256), (unsigned)BH), dim3(256), 0, s, part, fin,
                       R, BH, (int)nchunks);
    hipLaunchKernelGGL(performer_query_kernel, dim3((unsigned)cdiv(T, TILE), (unsigned)H, (unsigned)B), dim3(256), 0, s,
                       q, proj, fin, out, T, M, MT, ldc, in_bs, out_bs, ratio);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

// Kernels of the MRF-HiFi-GAN and RefineGAN decoders that the NSF-HiFiGAN path has no use for
// (mrf_hifigan.py, refinegan.py): the per-sample harmonic source, the linear upsample and AdaIN.
// All three are memory-bound; B clips of one length per launch, clip b independent of the others.
#include "rvc_common.h"

namespace {

// ---------------------------------------------------------------- per-sample harmonic source
// SineGenerator + merge (mrf_hifigan.py:45-94, refinegan.py:66-107).  Per harmonic h the phase is the cumulative sum
// over ALL L = T*upp samples of rad[i] = f32((f0up[i] * (h+1)) / sr) % 1 (+ the initial phase at sample 0).  torch's CPU
// cumsum of f32 accumulates in f64 and rounds each output, and the reference's "-1 at each wrap" only keeps that sum
// near [0, 1); so: the f32 increments summed in f64, the fractional part taken in f64, then sinf.
//
// Scan scheme (block partials + carry pass): a block covers HS_CHUNK = 256 threads x HS_ITEMS consecutive samples.
//   1. hs_partial_kernel: every block's f64 sum of increments per harmonic        -> part[b][h][blk]
//   2. hs_carry_kernel:   per (b, h) the exclusive f64 prefix of the partials, reduced to its fractional part
//   3. hs_apply_kernel:   per block the thread prefixes (f64, LDS), then each thread walks its samples
constexpr int HS_THREADS = 256;
constexpr int HS_ITEMS = 16;
constexpr int HS_CHUNK = HS_THREADS * HS_ITEMS;

struct HsArgs {
    const float* f0;      // [B][T]
    const float* phase0;  // [B][H]
    const float* noise;   // [B][L][H]
    float* har;           // [B][L]
    double* part;         // [B][H][nblk]
    int64_t T, L;
    int upp, H, linear, nblk;
    float sr, lin_b;
    float lin_w[RVC_HARMONIC_MAX];
};

// f0 at sample i (scale = f32(1 / upp)): nearest (nn.Upsample(scale_factor=upp)) or torch's linear rule
// (align_corners=False) in the operation order of its CPU kernel: src = fma(scale, i + 0.5, -0.5), y = fma(l0, x0, l1 * x1)
RVC_DEV float f0_at(const float* fb, int64_t T, int upp, int64_t i, int linear, float scale) {
#pragma clang fp contract(off)
    if (!linear) {  // torch's legacy "nearest": floorf(i * f32(1 / upp)), which may lag a frame at multiples of upp
        int64_t t = (int64_t)floorf((float)i * scale);
        return fb[t > T - 1 ? T - 1 : t];
    }
    float src = fmaf(scale, (float)i + 0.5f, -0.5f);
    if (src < 0.f) src = 0.f;
    int64_t i0 = (int64_t)src;
    if (i0 > T - 1) i0 = T - 1;
    const int64_t i1 = i0 + (i0 < T - 1 ? 1 : 0);
    float l1 = src - (float)i0;
    l1 = fminf(fmaxf(l1, 0.f), 1.f);
    const float l0 = 1.f - l1;
    return fmaf(l0, fb[i0], l1 * fb[i1]);
}

// the f32 increment of harmonic h at sample i (rad_values, with the initial phase added at sample 0)
RVC_DEV float hs_inc(float f, int h, float sr, int64_t i, float ph0) {
#pragma clang fp contract(off)
    float r = fmodf((f * (float)(h + 1)) / sr, 1.0f);
    if (r < 0.f) r += 1.0f;
    if (i == 0) r = r + ph0;
    return r;
}

// block-wide f64 sum / exclusive prefix over HS_THREADS values through LDS
RVC_DEV double block_excl_scan(double v, double* sh, double* total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int o = 1; o < HS_THREADS; o <<= 1) {
        const double a = tid >= o ? sh[tid - o] : 0.0;
        __syncthreads();
        sh[tid] += a;
        __syncthreads();
    }
    const double excl = tid > 0 ? sh[tid - 1] : 0.0;
    if (total) *total = sh[HS_THREADS - 1];
    __syncthreads();
    return excl;
}

__global__ __launch_bounds__(HS_THREADS) void hs_partial_kernel(HsArgs a) {
    __shared__ double sh[HS_THREADS];
    const int blk = blockIdx.x, b = blockIdx.y;
    const float* fb = a.f0 + (int64_t)b * a.T;
    const float scale = (float)(1.0 / (double)a.upp);
    const int64_t lo = (int64_t)blk * HS_CHUNK + (int64_t)threadIdx.x * HS_ITEMS;
    float f[HS_ITEMS];
#pragma unroll
    for (int k = 0; k < HS_ITEMS; ++k) f[k] = lo + k < a.L ? f0_at(fb, a.T, a.upp, lo + k, a.linear, scale) : 0.f;
    for (int h = 0; h < a.H; ++h) {
        const float ph0 = a.phase0[(int64_t)b * a.H + h];
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < HS_ITEMS; ++k)
            if (lo + k < a.L) s += (double)hs_inc(f[k], h, a.sr, lo + k, ph0);
        double total;
        block_excl_scan(s, sh, &total);
        if (threadIdx.x == 0) a.part[((int64_t)b * a.H + h) * a.nblk + blk] = total;
    }
}

// one block per (b, h): part[.] <- fractional part of the exclusive prefix of the block sums
__global__ __launch_bounds__(HS_THREADS) void hs_carry_kernel(double* part, int nblk) {
    __shared__ double sh[HS_THREADS];
    double* p = part + (int64_t)blockIdx.x * nblk;
    double run = 0.0;
    for (int base = 0; base < nblk; base += HS_THREADS) {
        const int i = base + threadIdx.x;
        const double v = i < nblk ? p[i] : 0.0;
        double total;
        const double excl = block_excl_scan(v, sh, &total);
        if (i < nblk) {
            const double c = run + excl;
            p[i] = c - floor(c);
        }
        run += total;
        run -= floor(run);
    }
}

__global__ __launch_bounds__(HS_THREADS) void hs_apply_kernel(HsArgs a) {
#pragma clang fp contract(off)
    __shared__ double sh[HS_THREADS];
    const int blk = blockIdx.x, b = blockIdx.y;
    const float* fb = a.f0 + (int64_t)b * a.T;
    const float scale = (float)(1.0 / (double)a.upp);
    const int64_t lo = (int64_t)blk * HS_CHUNK + (int64_t)threadIdx.x * HS_ITEMS;
    float f[HS_ITEMS], acc[HS_ITEMS];
#pragma unroll
    for (int k = 0; k < HS_ITEMS; ++k) {
        f[k] = lo + k < a.L ? f0_at(fb, a.T, a.upp, lo + k, a.linear, scale) : 0.f;
        acc[k] = 0.f;
    }
    const float* nb = a.noise + (int64_t)b * a.L * a.H;
    for (int h = 0; h < a.H; ++h) {
        const float ph0 = a.phase0[(int64_t)b * a.H + h];
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < HS_ITEMS; ++k)
            if (lo + k < a.L) s += (double)hs_inc(f[k], h, a.sr, lo + k, ph0);
        double run = block_excl_scan(s, sh, nullptr) + a.part[((int64_t)b * a.H + h) * a.nblk + blk];
        const float w = a.lin_w[h];
#pragma unroll
        for (int k = 0; k < HS_ITEMS; ++k) {
            if (lo + k >= a.L) break;
            run += (double)hs_inc(f[k], h, a.sr, lo + k, ph0);
            run -= floor(run);
            const float c = (float)run;
            const float sine = sinf((c * 2.f) * 3.14159274101257324f) * 0.1f;
            const float uv = f[k] > 0.f ? 1.f : 0.f;
            const float n = nb[(lo + k) * a.H + h];
            const float v = sine * uv + ((uv * 0.003f + ((1.f - uv) * 0.1f) / 3.0f) * n);
            acc[k] += v * w;
        }
    }
    float* hb = a.har + (int64_t)b * a.L;
#pragma unroll
    for (int k = 0; k < HS_ITEMS; ++k)
        if (lo + k < a.L) hb[lo + k] = tanhf(acc[k] + a.lin_b);
}

// ---------------------------------------------------------------- linear upsample
// y[b][c][j] = lerp of act(x[b][c][.]) at (j + 0.5)/r - 0.5 (clamped at 0; right neighbour clamped at Lin-1), the
// operation order of torch's CPU kernel: src = fma(1/r, j + 0.5, -0.5), y = fma(l0, x0, l1 * x1).  A block stages the
// activated inputs of its UP_TILE outputs in LDS (coalesced loads); a thread stores UP_VECS float4s.
constexpr int UP_THREADS = 256;
constexpr int UP_VECS = 4;                        // float4 stores per thread
constexpr int UP_TILE = UP_THREADS * 4 * UP_VECS;  // outputs per block
constexpr int UP_IN_MAX = UP_TILE + 4;             // r = 1

template <bool VEC>
__global__ __launch_bounds__(UP_THREADS) void upsample_linear_kernel(const float* x, float* y, int C, int Lin, int r,
                                                                     int64_t x_bstride, int64_t y_bstride, int act,
                                                                     float slope) {
#pragma clang fp contract(off)
    __shared__ float sx[UP_IN_MAX];
    const int c = blockIdx.y, b = blockIdx.z;
    const int Lout = Lin * r;  // <= 2^24 (checked by the entry point)
    const int j0 = blockIdx.x * UP_TILE;
    const float* xr = x + (int64_t)b * x_bstride + (int64_t)c * Lin;
    float* yr = y + (int64_t)b * y_bstride + (int64_t)c * Lout;
    int i_lo = j0 / r - 1;
    if (i_lo < 0) i_lo = 0;
    int n_in = UP_TILE / r + 4;
    if (n_in > UP_IN_MAX) n_in = UP_IN_MAX;
    if (i_lo + n_in > Lin) n_in = Lin - i_lo;
    for (int i = threadIdx.x; i < n_in; i += UP_THREADS) sx[i] = act_apply(xr[i_lo + i], act, slope);
    __syncthreads();
    const float scale = (float)(1.0 / (double)r);
#pragma unroll
    for (int v = 0; v < UP_VECS; ++v) {
        const int jb = j0 + (v * UP_THREADS + (int)threadIdx.x) * 4;  // a wave stores 1 KiB contiguous
        if (jb >= Lout) break;
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = jb + k;
            float src = fmaf(scale, (float)j + 0.5f, -0.5f);
            if (src < 0.f) src = 0.f;
            int i0 = (int)src;
            if (i0 > Lin - 1) i0 = Lin - 1;
            const int i1 = i0 + (i0 < Lin - 1 ? 1 : 0);
            float l1 = src - (float)i0;
            l1 = fminf(fmaxf(l1, 0.f), 1.f);
            const float l0 = 1.f - l1;
            // LDS indices clamped to the staged range (they lie inside it for every j < Lout; the clamp is the bound)
            int a0 = i0 - i_lo, a1 = i1 - i_lo;
            a0 = a0 < 0 ? 0 : (a0 > n_in - 1 ? n_in - 1 : a0);
            a1 = a1 < 0 ? 0 : (a1 > n_in - 1 ? n_in - 1 : a1);
            o[k] = fmaf(l0, sx[a0], l1 * sx[a1]);
        }
        if (VEC) {  // Lout % 4 == 0 and 16-byte aligned rows: jb + 3 < Lout
            *reinterpret_cast<float4*>(yr + jb) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (jb + k < Lout) yr[jb + k] = o[k];
        }
    }
}

// ---------------------------------------------------------------- AdaIN
// y (+)= out_scale * lrelu(x + n * w[c], slope) over [B][C][L] (refinegan.py:39-46).  n: a buffer, or drawn here from
// the Philox4x32-10 stream exactly as rand_kernel (elementwise.hip) fills a buffer of C*L values per clip: element
// e = c*L + t of clip b is draw e % 4 of counter e / 4 + offset under seed seeds[b] (+ *seed_add).
struct AdainSeeds {
    uint64_t s[RVC_ADAIN_BMAX];
};

RVC_DEV void philox10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void adain_kernel(const float* x, const float* noise, const float* w, float* y,
                                                    int64_t L, int64_t n, float slope, float out_scale, int accumulate,
                                                    AdainSeeds seeds, uint64_t offset, const uint64_t* seed_add) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one thread -> 4 elements of clip b
    const int b = blockIdx.y;
    const int64_t base = i * 4;
    if (base >= n) return;
    const float* xb = x + (int64_t)b * n;
    float* yb = y + (int64_t)b * n;
    float nv[4], xv[4], yv[4] = {0.f, 0.f, 0.f, 0.f};
    if (noise) {
        const float* nb = noise + (int64_t)b * n;
        if (VEC) {
            const float4 t = *reinterpret_cast<const float4*>(nb + base);
            nv[0] = t.x; nv[1] = t.y; nv[2] = t.z; nv[3] = t.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) nv[j] = base + j < n ? nb[base + j] : 0.f;
        }
    } else {
        uint64_t seed = seeds.s[b];
        if (seed_add) seed += *seed_add;
        const uint64_t ctr = (uint64_t)i + offset;
        uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0x7A3Bu, 0x52u};
        philox10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float u1 = ((c[2 * j] >> 8) + 1) * (1.0f / 16777216.0f);  // (0, 1]
            float u2 = (c[2 * j + 1] >> 8) * (1.0f / 16777216.0f);
            float rad = sqrtf(-2.0f * logf(u1));
            float s, co;
            sincosf(6.2831853071795864f * u2, &s, &co);
            nv[2 * j] = rad * co;
            nv[2 * j + 1] = rad * s;
        }
    }
    if (VEC) {
        const float4 t = *reinterpret_cast<const float4*>(xb + base);
        xv[0] = t.x; xv[1] = t.y; xv[2] = t.z; xv[3] = t.w;
        if (accumulate) {
            const float4 u = *reinterpret_cast<const float4*>(yb + base);
            yv[0] = u.x; yv[1] = u.y; yv[2] = u.z; yv[3] = u.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            xv[j] = base + j < n ? xb[base + j] : 0.f;
            if (accumulate) yv[j] = base + j < n ? yb[base + j] : 0.f;
        }
    }
    float o[4];
    {
#pragma clang fp contract(off)
        int64_t c0 = base / L;
        int64_t left = (c0 + 1) * L - base;  // elements before the next channel row starts
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (left == 0) {
                ++c0;
                left = L;
            }
            --left;
            float v = 0.f;
            if (base + j < n) {
                v = xv[j] + nv[j] * w[c0];
                v = v >= 0.f ? v : v * slope;
                v = v * out_scale;
                if (accumulate) v = yv[j] + v;
            }
            o[j] = v;
        }
    }
    if (VEC) {
        *reinterpret_cast<float4*>(yb + base) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (base + j < n) yb[base + j] = o[j];
    }
}

__global__ void rand_uniform_kernel(float* out, int64_t n, uint64_t seed, uint64_t offset, const uint64_t* seed_add) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one thread -> 4 draws
    const int64_t base = i * 4;
    if (base >= n) return;
    if (seed_add) seed += *seed_add;
    const uint64_t ctr = (uint64_t)i + offset;
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0x7A3Bu, 0x52u};
    philox10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (base + j < n) out[base + j] = (c[j] >> 8) * (1.0f / 16777216.0f);  // [0, 1)
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int rvc_rand_uniform(float* out, int64_t n, uint64_t seed, uint64_t offset, const uint64_t* seed_add,
                                rvc_stream_t stream) {
    RVC_CHECK_ARG(out && n >= 0, "rand_uniform: bad args");
    if (n == 0) return RVC_OK;
    hipLaunchKernelGGL(rand_uniform_kernel, dim3(cdiv((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, out, n,
                       seed, offset, seed_add);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int64_t rvc_harmonic_source_ws_bytes(int64_t B, int64_t T, int upp, int H) {
    if (B <= 0 || T <= 0 || upp <= 0 || H <= 0 || H > RVC_HARMONIC_MAX) return -1;
    const int64_t nblk = (T * upp + HS_CHUNK - 1) / HS_CHUNK;
    return B * H * nblk * (int64_t)sizeof(double);
}

extern "C" int64_t rvc_harmonic_source_chunk(void) { return HS_CHUNK; }

extern "C" int rvc_harmonic_source(const float* f0, const float* phase0, const float* noise, float* har, int64_t B,
                                   int64_t T, int upp, int H, int linear, float sr, const float* lin_w, float lin_b,
                                   void* ws, int64_t ws_bytes, rvc_stream_t stream) {
    RVC_CHECK_ARG(f0 && phase0 && noise && har && lin_w && ws, "harmonic_source: null pointer");
    RVC_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && upp > 0 && H > 0 && H <= RVC_HARMONIC_MAX && sr > 0.f,
                  "harmonic_source: bad shape (1 <= H <= %d)", RVC_HARMONIC_MAX);
    const int64_t L = T * upp;
    RVC_CHECK_ARG(L <= ((int64_t)1 << 24) || !linear,
                  "harmonic_source: linear f0 upsampling takes at most 2^24 samples per clip");
    const int64_t need = rvc_harmonic_source_ws_bytes(B, T, upp, H);
    RVC_CHECK_ARG(ws_bytes >= need && ((uintptr_t)ws & 7u) == 0, "harmonic_source: workspace of %lld bytes, 8-aligned",
                  (long long)need);
    HsArgs a;
    a.f0 = f0; a.phase0 = phase0; a.noise = noise; a.har = har; a.part = (double*)ws;
    a.T = T; a.L = L; a.upp = upp; a.H = H; a.linear = linear ? 1 : 0;
    a.nblk = (int)((L + HS_CHUNK - 1) / HS_CHUNK);
    a.sr = sr; a.lin_b = lin_b;
    for (int h = 0; h < RVC_HARMONIC_MAX; ++h) a.lin_w[h] = h < H ? lin_w[h] : 0.f;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)a.nblk, (unsigned)B);
    hipLaunchKernelGGL(hs_partial_kernel, grid, dim3(HS_THREADS), 0, s, a);
    RVC_HIP(hipGetLastError());
    hipLaunchKernelGGL(hs_carry_kernel, dim3((unsigned)(B * H)), dim3(HS_THREADS), 0, s, a.part, a.nblk);
    RVC_HIP(hipGetLastError());
    hipLaunchKernelGGL(hs_apply_kernel, grid, dim3(HS_THREADS), 0, s, a);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_upsample_linear(const float* x, float* y, int64_t B, int64_t C, int64_t Lin, int r,
                                   int64_t x_bstride, int64_t y_bstride, int act, float slope, rvc_stream_t stream) {
    RVC_CHECK_ARG(x && y && x != y, "upsample_linear: null or aliased pointers");
    RVC_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && C <= 65535 && Lin > 0 && r >= 1, "upsample_linear: bad shape");
    const int64_t Lout = Lin * r;
    RVC_CHECK_ARG(Lout <= ((int64_t)1 << 24), "upsample_linear: at most 2^24 output samples per row");
    if (!x_bstride) x_bstride = C * Lin;
    if (!y_bstride) y_bstride = C * Lout;
    RVC_CHECK_ARG(x_bstride >= C * Lin && y_bstride >= C * Lout, "upsample_linear: batch stride below C*L");
    RVC_CHECK_ARG(act == RVC_ACT_NONE || act == RVC_ACT_LRELU, "upsample_linear: act none or lrelu");
    const dim3 grid(cdiv(Lout, UP_TILE), (unsigned)C, (unsigned)B);
    const bool vec = Lout % 4 == 0 && y_bstride % 4 == 0 && aligned16(y);
    if (vec)
        hipLaunchKernelGGL(upsample_linear_kernel<true>, grid, dim3(UP_THREADS), 0, (hipStream_t)stream, x, y, (int)C,
                           (int)Lin, r, x_bstride, y_bstride, act, slope);
    else
        hipLaunchKernelGGL(upsample_linear_kernel<false>, grid, dim3(UP_THREADS), 0, (hipStream_t)stream, x, y, (int)C,
                           (int)Lin, r, x_bstride, y_bstride, act, slope);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_adain(const float* x, const float* noise, const float* w, float* y, int64_t B, int64_t C, int64_t L,
                         float slope, float out_scale, int accumulate, const uint64_t* seeds, uint64_t offset,
                         const uint64_t* seed_add, rvc_stream_t stream) {
    RVC_CHECK_ARG(x && w && y, "adain: null pointer");
    RVC_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && L > 0, "adain: bad shape");
    RVC_CHECK_ARG(noise || (seeds && B <= RVC_ADAIN_BMAX), "adain: the in-kernel draw takes one seed per clip, B <= %d",
                  RVC_ADAIN_BMAX);
    RVC_CHECK_ARG(!(accumulate && x == y), "adain: accumulate needs y distinct from x");
    const int64_t n = C * L;
    AdainSeeds sd = {};
    if (!noise)
        for (int64_t b = 0; b < B; ++b) sd.s[b] = seeds[b];
    const dim3 grid(cdiv((n + 3) / 4, 256), (unsigned)B);
    const bool vec = n % 4 == 0 && aligned16(x) && aligned16(y) && (!noise || aligned16(noise));
    if (vec)
        hipLaunchKernelGGL(adain_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, noise, w, y, L, n, slope,
                           out_scale, accumulate, sd, offset, seed_add);
    else
        hipLaunchKernelGGL(adain_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, noise, w, y, L, n, slope,
                           out_scale, accumulate, sd, offset, seed_add);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

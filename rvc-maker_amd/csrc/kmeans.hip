// IVF training on the device: the k-means of faiss's IndexIVFFlat::train (Clustering::train with niter = 10, as
// create_index.py:66-83 reaches it through index_factory("IVF{n},Flat").train) and the list assignment of add.
// Host control (initial permutation, split of empty clusters, the iteration loop) is rvc_amd/index_train.py.
// rvc_minibatch_assign (the MiniBatchKMeans reduction, minibatch.hip) is the same assignment with k > n allowed.
//
//   kmeans_prep_kernel      ||c_j||^2 and ||x_i||^2 in f32 (one wave per row), and the (value, index) cells reset
//   kmeans_assign_kernel    block = 128 rows x a run of 128-centroid tiles; <c_j, x_i> on v_mfma_f32_32x32x2_f32 (exact
//                           f32 products in an f32 fma chain over the dimensions in order), M = centroids, N = rows, so a
//                           lane's 16 accumulator registers are 16 centroids of ONE row: the running (min, argmin) of
//                           cnorm_j - 2 <x_i, c_j> is two registers per row tile, carried across centroid tiles.  The
//                           [n][k] matrix never exists.  At the end the two half-waves and the block's waves (and the
//                           blocks of a split centroid axis, grid.y) meet in a 64-bit integer atomic min on
//                           (order-preserving bits of the value << 32 | index): equal values keep the lowest index, and
//                           no floating-point atomic is involved, so two runs give identical bits.
//   kmeans_finalize_kernel  cell -> assign, dist = max(0, value + ||x_i||^2)
//   kmeans_count / scan     list sizes (integer atomics) and their exclusive scan -> list_off
//   kmeans_radix_*          stable LSD radix sort of the row numbers by list, 8 bits a pass (2 passes up to 65536
//                           lists): per-chunk digit histograms, their scan in (digit, chunk) order, and a one-wave
//                           scatter per chunk whose rank inside a 64-row step is a ballot match -- ids ascending inside
//                           each list, as faiss's sequential add leaves them; a list of any length (nothing sits in LDS
//                           per list)
//   kmeans_update_kernel    faiss compute_centroids: one thread per (centroid, 4 dimensions) adds its members in ascending
//                           row order from 0 in f32 and multiplies by 1.f / count; empty lists copy the previous centroid
//   gather_rows_kernel      out[m] = x[ids[m]]
//
// No contraction anywhere in the file: the update's sums are compared bit for bit with their restatement.
#include <algorithm>

#include "rvc_common.h"

#pragma clang fp contract(off)

namespace {
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

constexpr int TM = 128;           // centroids per block tile (MFMA M)
constexpr int TN = 128;           // rows per block tile (MFMA N)
constexpr int KT = 32;            // dimensions per LDS stage: one 128-byte line of a row
constexpr int NLD = TN * KT / 4 / 256;  // float4 loads per thread, operand and stage
constexpr int LDT = TM + 2;       // LDS row stride (words): 4 * LDT = 8 (mod 32) spreads a store's dimension quads
constexpr size_t ASSIGN_LDS = (4 * KT * LDT + TM) * sizeof(float);  // both operands, double-buffered, and cnorm
constexpr int FILL_BLOCKS = 256;  // below this many row blocks the centroid axis is split over grid.y (one per CU)
constexpr int CH = 2048;          // rows per radix chunk
constexpr int64_t NMAX = (1ll << 31) - 4096;

// f32 -> u32 whose unsigned order is the floats' order (-0 below +0; NaNs at the ends)
RVC_DEV unsigned ord_bits(float v) {
    const unsigned b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
RVC_DEV float ord_value(unsigned u) { return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xffffffffu)); }

// rows [0, k): centroids -> cnorm; rows [k, k + n): x -> xnorm and the row's cell reset.  One wave per row.
__global__ __launch_bounds__(256) void kmeans_prep_kernel(const float* __restrict__ x, int64_t n, int d,
                                                          const float* __restrict__ cent, int64_t k, float* cnorm,
                                                          float* xnorm, u64* best) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n + k) return;
    const float4* p = (const float4*)(r < k ? cent + r * d : x + (r - k) * d);
    float s = 0.f;
    for (int c = lane; c < d / 4; c += 64) {
        const float4 v = p[c];
        s = s + v.x * v.x;
        s = s + v.y * v.y;
        s = s + v.z * v.z;
        s = s + v.w * v.w;
    }
    s = wave_sum(s);
    if (lane == 0) {
        if (r < k) {
            cnorm[r] = s;
        } else {
            xnorm[r - k] = s;
            best[r - k] = ~0ull;
        }
    }
}

// grid (cdiv(n, TN), gy); block y takes centroid tiles [y * tiles_per, (y + 1) * tiles_per)
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const float* __restrict__ x, int n, int d,
                                                            const float* __restrict__ cent, int k,
                                                            const float* __restrict__ cnorm, int tiles_per,
                                                            u64* best) {
    extern __shared__ float lds_[];  // ASSIGN_LDS bytes: over the 64 KiB a static image may take
    float(*Cs)[KT][LDT] = (float(*)[KT][LDT])lds_;
    float(*Xs)[KT][LDT] = Cs + 2;
    float* cn_s = lds_ + 4 * KT * LDT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lh = lane >> 5;
    const int row0 = blockIdx.x * TN;
    const int ctiles = (k + TM - 1) / TM;
    const int ct0 = blockIdx.y * tiles_per;
    const int ct1 = min(ct0 + tiles_per, ctiles);
    // loader: 8 lanes cover one row's 32 dimensions of the stage (a whole 128-byte line), a wave-load 8 rows; thread
    // -> dimension quad kq and tile rows lr + 32 s.  Rows past the end re-read the last row (their results are dropped),
    // dimensions past d are zeros (exact: fma(0, 0, acc) = acc).  Words of one store: bank 8 kq + row (mod 32), at
    // most 2-way, which a ds_write_b32 absorbs.
    const int lr = tid >> 3, kq = tid & 7;
    const float* xp[NLD];
#pragma unroll
    for (int s = 0; s < NLD; ++s) xp[s] = x + (int64_t)min(row0 + lr + 32 * s, n - 1) * d + 4 * kq;
    const int nk = (d + KT - 1) / KT;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float bv[2] = {INFINITY, INFINITY};
    int bi[2] = {0x7fffffff, 0x7fffffff};

    for (int ct = ct0; ct < ct1; ++ct) {
        const int c0 = ct * TM;
        const float* cp[NLD];
#pragma unroll
        for (int s = 0; s < NLD; ++s) cp[s] = cent + (int64_t)min(c0 + lr + 32 * s, k - 1) * d + 4 * kq;
        __syncthreads();  // the previous tile's epilogue has read cn_s
        if (tid < TM) cn_s[tid] = c0 + tid < k ? cnorm[c0 + tid] : INFINITY;
        floatx16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
        float4 gx[NLD], gc[NLD];
        auto fetch = [&](int kt) {
            const int kk = kt * KT;
            const bool in = kk + 4 * kq < d;
#pragma unroll
            for (int s = 0; s < NLD; ++s) {
                gx[s] = in ? *(const float4*)(xp[s] + kk) : zero4;
                gc[s] = in ? *(const float4*)(cp[s] + kk) : zero4;
            }
        };
        auto stage = [&](int buf) {
            float(*X)[LDT] = Xs[buf];
            float(*C)[LDT] = Cs[buf];
#pragma unroll
            for (int s = 0; s < NLD; ++s) {
                const int r = lr + 32 * s;
                X[4 * kq + 0][r] = gx[s].x, X[4 * kq + 1][r] = gx[s].y, X[4 * kq + 2][r] = gx[s].z, X[4 * kq + 3][r] = gx[s].w;
                C[4 * kq + 0][r] = gc[s].x, C[4 * kq + 1][r] = gc[s].y, C[4 * kq + 2][r] = gc[s].z, C[4 * kq + 3][r] = gc[s].w;
            }
        };
        fetch(0);
        stage(0);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            const bool more = kt + 1 < nk;
            if (more) fetch(kt + 1);  // the next stage's global loads fly over this stage's MFMAs
#pragma unroll
            for (int k2 = 0; k2 < KT / 2; ++k2) {
                const int kr = 2 * k2 + lh;
                float a[2], b[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    a[t] = Cs[buf][kr][wm * 64 + t * 32 + l31];
                    b[t] = Xs[buf][kr][wn * 64 + t * 32 + l31];
                }
#pragma unroll
                for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                    for (int tn = 0; tn < 2; ++tn)
                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
            }
            if (more) stage(buf ^ 1);  // the other buffer: its readers passed the barrier that ended stage kt - 1
            __syncthreads();
        }
        // D[m][nn]: nn = lane & 31, m = (r & 3) + 8 (r >> 2) + 4 (lane >> 5): ascending in (tm, r), and tiles ascend,
        // so a strict < keeps the lowest centroid among equal values inside a lane
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = wm * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    const float v = fmaf(-2.f, acc[tm][tn][r], cn_s[m]);  // 2 <x, c> is exact: one rounding
                    if (v < bv[tn]) {
                        bv[tn] = v;
                        bi[tn] = c0 + m;
                    }
                }
    }
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        u64 p = ((u64)ord_bits(bv[tn]) << 32) | (unsigned)bi[tn];
        const u64 o = __shfl_xor(p, 32, 64);
        p = o < p ? o : p;
        const int i = row0 + wn * 64 + tn * 32 + l31;
        if (lh == 0 && i < n) atomicMin(best + i, p);
    }
}

__global__ __launch_bounds__(256) void kmeans_finalize_kernel(const u64* best, const float* xnorm, int n, int k,
                                                              int* assign, float* dist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 p = best[i];
    const unsigned idx = (unsigned)p;
    assign[i] = idx < (unsigned)k ? (int)idx : 0;  // a row of NaNs never wins a comparison: list 0, dist NaN
    const float v = ord_value((unsigned)(p >> 32)) + xnorm[i];
    dist[i] = v < 0.f ? 0.f : v;
}

RVC_DEV int clamp_key(int a, int k) { return a < 0 ? 0 : (a >= k ? k - 1 : a); }

__global__ __launch_bounds__(256) void kmeans_count_kernel(const int* assign, int n, int k, int* counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(counts + clamp_key(assign[i], k), 1);
}

// one block: list_off[j] = sum of counts[0..j), list_off[k] = n
__global__ __launch_bounds__(1024) void kmeans_scan_counts_kernel(const int* counts, int k, int64_t* list_off) {
    __shared__ int64_t sh[1024];
    __shared__ int64_t carry_s;
    const int t = threadIdx.x;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int j0 = 0; j0 < k; j0 += 1024) {
        const int64_t own = j0 + t < k ? counts[j0 + t] : 0;
        sh[t] = own;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int64_t v = t >= o ? sh[t - o] : 0;
            __syncthreads();
            sh[t] += v;
            __syncthreads();
        }
        const int64_t carry = carry_s;
        if (j0 + t < k) list_off[j0 + t] = carry + sh[t] - own;
        __syncthreads();
        if (t == 1023) carry_s = carry + sh[1023];
        __syncthreads();
    }
    if (t == 0) list_off[k] = carry_s;
}

// hist[digit * nb + chunk] = rows of the chunk whose key has that digit
__global__ __launch_bounds__(256) void kmeans_radix_hist_kernel(const int* key_in, int n, int k, int shift, int nb,
                                                                int* hist) {
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int i0 = blockIdx.x * CH, i1 = min(n, i0 + CH);
    for (int i = i0 + threadIdx.x; i < i1; i += 256) atomicAdd(&h[(clamp_key(key_in[i], k) >> shift) & 255], 1);
    __syncthreads();
    hist[threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

// one block: exclusive scan of hist[0..m) in place
__global__ __launch_bounds__(1024) void kmeans_radix_scan_kernel(int* hist, int m) {
    __shared__ int sh[1024];
    __shared__ int carry_s;
    const int t = threadIdx.x;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int j0 = 0; j0 < m; j0 += 1024) {
        const int own = j0 + t < m ? hist[j0 + t] : 0;
        sh[t] = own;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int v = t >= o ? sh[t - o] : 0;
            __syncthreads();
            sh[t] += v;
            __syncthreads();
        }
        const int carry = carry_s;
        if (j0 + t < m) hist[j0 + t] = carry + sh[t] - own;
        __syncthreads();
        if (t == 1023) carry_s = carry + sh[1023];
        __syncthreads();
    }
}

// one wave per chunk, 64 rows a step in row order: a row's slot is its digit's running base plus the number of lower
// lanes of the step with the same digit (stable).  row_in NULL: the rows are i themselves (first pass); ids_out set:
// the last pass, which writes the int64 ids.
__global__ __launch_bounds__(64) void kmeans_radix_scatter_kernel(const int* key_in, const int* row_in, int n, int k,
                                                                  int shift, const int* hist, int nb, int* key_out,
                                                                  int* row_out, int64_t* ids_out) {
    __shared__ int base[256];
    const int lane = threadIdx.x;
    for (int j = lane; j < 256; j += 64) base[j] = hist[j * nb + blockIdx.x];
    __syncthreads();
    const int i0 = blockIdx.x * CH, i1 = min(n, i0 + CH);
    for (int s = i0; s < i1; s += 64) {
        const int i = s + lane;
        const bool valid = i < i1;
        const int key = valid ? clamp_key(key_in[i], k) : 0;
        const int row = valid ? (row_in ? row_in[i] : i) : 0;
        const int dg = (key >> shift) & 255;
        u64 mask = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool on = (dg >> b) & 1;
            const u64 bb = __ballot(on);
            mask &= on ? bb : ~bb;
        }
        const int rank = __popcll(mask & ((1ull << lane) - 1ull));
        const int cnt = __popcll(mask);
        const int pos = valid ? base[dg] + rank : 0;
        __syncthreads();
        if (valid && rank == cnt - 1) base[dg] += cnt;
        __syncthreads();
        if (valid && pos >= 0 && pos < n) {
            if (ids_out) {
                ids_out[pos] = row;
            } else {
                key_out[pos] = key;
                row_out[pos] = row;
            }
        }
    }
}

__global__ __launch_bounds__(256) void kmeans_update_kernel(const float* __restrict__ x, int64_t n, int d4,
                                                            const int64_t* __restrict__ list_off,
                                                            const int64_t* __restrict__ ids, int64_t k,
                                                            const float* __restrict__ prev, float* out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= k * d4) return;
    const int64_t c = t / d4;
    const int ch = (int)(t - c * d4);
    int64_t o0 = list_off[c], o1 = list_off[c + 1];
    o0 = o0 < 0 ? 0 : o0;
    o1 = o1 > n ? n : o1;
    if (o1 <= o0) {
        ((float4*)out)[t] = ((const float4*)prev)[t];
        return;
    }
    const float4* x4 = (const float4*)x + ch;
    auto row = [&](int64_t v) {
        const int64_t r = ids[v];
        return x4[(r < 0 ? 0 : (r >= n ? n - 1 : r)) * d4];
    };
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    auto add = [&](const float4& a) {
        s.x = s.x + a.x, s.y = s.y + a.y, s.z = s.z + a.z, s.w = s.w + a.w;
    };
    int64_t v = o0;
    for (; v + 4 <= o1; v += 4) {  // four rows in flight, added in order
        const float4 a0 = row(v), a1 = row(v + 1), a2 = row(v + 2), a3 = row(v + 3);
        add(a0), add(a1), add(a2), add(a3);
    }
    for (; v < o1; ++v) add(row(v));
    const float inv = 1.f / (float)(o1 - o0);
    ((float4*)out)[t] = make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ x, int d4,
                                                          const int64_t* __restrict__ ids, int64_t m, float* out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= m * d4) return;
    const int64_t r = t / d4;
    const int ch = (int)(t - r * d4);
    ((float4*)out)[t] = ((const float4*)x)[ids[r] * d4 + ch];
}

bool dim_ok(int64_t d) { return d >= 8 && d <= 1024 && d % 8 == 0; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
int radix_passes(int64_t k) {
    int p = 1;
    while (p < 4 && (1ll << (8 * p)) < k) ++p;
    return p;
}
}  // namespace

extern "C" int64_t rvc_kmeans_assign_work_bytes(int64_t n, int64_t d, int64_t k) {
    if (n < 1 || k < 1 || n > NMAX || k > NMAX || !dim_ok(d)) return -1;
    return n * 8 + ((n + 3) / 4 * 4 + (k + 3) / 4 * 4) * 4;  // cells u64 [n], xnorm f32 [n], cnorm f32 [k]
}

// The launches of an assignment whose arguments have been validated.  Nothing in them needs k <= n: rows past n and
// centroids past k are clamped reads whose results are dropped (cnorm = +inf), and the centroid axis is split over
// grid.y whenever the rows alone do not fill the device.
static int assign_launch(const float* x, int64_t n, int64_t d, const float* cent, int64_t k, void* work, int32_t* assign,
                         float* dist, hipStream_t s) {
    u64* best = (u64*)work;
    float* xnorm = (float*)(best + n);
    float* cnorm = xnorm + (n + 3) / 4 * 4;
    const int64_t gx = (n + TN - 1) / TN, ctiles = (k + TM - 1) / TM;
    int64_t gy = 1;
    if (gx < FILL_BLOCKS) gy = std::min<int64_t>(ctiles, (FILL_BLOCKS + gx - 1) / gx);
    const int64_t tiles_per = (ctiles + gy - 1) / gy;
    gy = (ctiles + tiles_per - 1) / tiles_per;
    hipLaunchKernelGGL(kmeans_prep_kernel, dim3(cdiv(n + k, 4)), dim3(256), 0, s, x, n, (int)d, cent, k, cnorm, xnorm,
                       best);
    static bool attr = false;
    if (!attr) {
        RVC_HIP(hipFuncSetAttribute((const void*)kmeans_assign_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)ASSIGN_LDS));
        attr = true;
    }
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), ASSIGN_LDS, s, x, (int)n, (int)d, cent,
                       (int)k, (const float*)cnorm, (int)tiles_per, best);
    hipLaunchKernelGGL(kmeans_finalize_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, (const u64*)best,
                       (const float*)xnorm, (int)n, (int)k, assign, dist);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_kmeans_assign(const float* x, int64_t n, int64_t d, const float* cent, int64_t k, void* work,
                                 int64_t work_bytes, int32_t* assign, float* dist, rvc_stream_t stream) {
    RVC_CHECK_ARG(x && cent && work && assign && dist, "kmeans_assign: null pointer");
    RVC_CHECK_ARG(dim_ok(d), "kmeans_assign: d=%lld must be a multiple of 8 in [8, 1024]", (long long)d);
    RVC_CHECK_ARG(k >= 1 && n >= k && n <= NMAX, "kmeans_assign: bad sizes n=%lld k=%lld (1 <= k <= n)", (long long)n,
                  (long long)k);
    RVC_CHECK_ARG(work_bytes >= rvc_kmeans_assign_work_bytes(n, d, k), "kmeans_assign: workspace too small");
    RVC_CHECK_ARG(aligned16(x) && aligned16(cent) && aligned16(work), "kmeans_assign: x, cent, work 16-byte aligned");
    return assign_launch(x, n, d, cent, k, work, assign, dist, (hipStream_t)stream);
}

// The same assignment for a mini-batch: k may exceed n (2048 rows against 10000 centres).
extern "C" int rvc_minibatch_assign(const float* x, int64_t n, int64_t d, const float* cent, int64_t k, void* work,
                                    int64_t work_bytes, int32_t* assign, float* dist, rvc_stream_t stream) {
    RVC_CHECK_ARG(x && cent && work && assign && dist, "minibatch_assign: null pointer");
    RVC_CHECK_ARG(dim_ok(d), "minibatch_assign: d=%lld must be a multiple of 8 in [8, 1024]", (long long)d);
    RVC_CHECK_ARG(k >= 1 && n >= 1 && n <= NMAX && k <= NMAX, "minibatch_assign: bad sizes n=%lld k=%lld", (long long)n,
                  (long long)k);
    RVC_CHECK_ARG(work_bytes >= rvc_kmeans_assign_work_bytes(n, d, k), "minibatch_assign: workspace too small");
    RVC_CHECK_ARG(aligned16(x) && aligned16(cent) && aligned16(work), "minibatch_assign: x, cent, work 16-byte aligned");
    return assign_launch(x, n, d, cent, k, work, assign, dist, (hipStream_t)stream);
}

extern "C" int64_t rvc_kmeans_lists_work_bytes(int64_t n, int64_t k) {
    if (n < 1 || k < 1 || n > NMAX || k > NMAX) return -1;
    const int64_t nb = (n + CH - 1) / CH;
    return (4 * ((n + 3) / 4 * 4) + 256 * nb) * 4;  // two (key, row) int32 buffers of n, the digit histograms
}

extern "C" int rvc_kmeans_lists(const int32_t* assign, int64_t n, int64_t k, void* work, int64_t work_bytes,
                                int64_t* list_off, int64_t* ids, int32_t* counts, rvc_stream_t stream) {
    RVC_CHECK_ARG(assign && work && list_off && ids && counts, "kmeans_lists: null pointer");
    RVC_CHECK_ARG(n >= 1 && k >= 1 && n <= NMAX && k <= NMAX, "kmeans_lists: bad sizes n=%lld k=%lld", (long long)n,
                  (long long)k);
    RVC_CHECK_ARG(work_bytes >= rvc_kmeans_lists_work_bytes(n, k), "kmeans_lists: workspace too small");
    RVC_CHECK_ARG(aligned16(work), "kmeans_lists: work 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int64_t np = (n + 3) / 4 * 4;
    const int nb = (int)((n + CH - 1) / CH);
    int* key[2] = {(int*)work, (int*)work + 2 * np};
    int* row[2] = {(int*)work + np, (int*)work + 3 * np};
    int* hist = (int*)work + 4 * np;
    RVC_HIP(hipMemsetAsync(counts, 0, (size_t)k * 4, s));
    hipLaunchKernelGGL(kmeans_count_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, assign, (int)n, (int)k, counts);
    hipLaunchKernelGGL(kmeans_scan_counts_kernel, dim3(1), dim3(1024), 0, s, (const int*)counts, (int)k, list_off);
    const int passes = radix_passes(k);
    for (int p = 0; p < passes; ++p) {
        const int* kin = p == 0 ? assign : key[(p - 1) & 1];
        const int* rin = p == 0 ? nullptr : row[(p - 1) & 1];
        const bool last = p == passes - 1;
        hipLaunchKernelGGL(kmeans_radix_hist_kernel, dim3(nb), dim3(256), 0, s, kin, (int)n, (int)k, 8 * p, nb, hist);
        hipLaunchKernelGGL(kmeans_radix_scan_kernel, dim3(1), dim3(1024), 0, s, hist, 256 * nb);
        hipLaunchKernelGGL(kmeans_radix_scatter_kernel, dim3(nb), dim3(64), 0, s, kin, rin, (int)n, (int)k, 8 * p,
                           (const int*)hist, nb, key[p & 1], row[p & 1], last ? ids : nullptr);
    }
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_kmeans_update(const float* x, int64_t n, int64_t d, const int64_t* list_off, const int64_t* ids,
                                 int64_t k, const float* cent_prev, float* cent_out, rvc_stream_t stream) {
    RVC_CHECK_ARG(x && list_off && ids && cent_prev && cent_out, "kmeans_update: null pointer");
    RVC_CHECK_ARG(dim_ok(d), "kmeans_update: d=%lld must be a multiple of 8 in [8, 1024]", (long long)d);
    RVC_CHECK_ARG(n >= 1 && k >= 1 && n <= NMAX && k <= NMAX, "kmeans_update: bad sizes n=%lld k=%lld", (long long)n,
                  (long long)k);
    RVC_CHECK_ARG(aligned16(x) && aligned16(cent_prev) && aligned16(cent_out), "kmeans_update: 16-byte aligned arrays");
    RVC_CHECK_ARG(cent_prev != cent_out, "kmeans_update: cent_out must not alias cent_prev");
    hipLaunchKernelGGL(kmeans_update_kernel, dim3(cdiv(k * (d / 4), 256)), dim3(256), 0, (hipStream_t)stream, x, n,
                       (int)(d / 4), list_off, ids, k, cent_prev, cent_out);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_gather_rows(const float* x, int64_t d, const int64_t* ids, int64_t m, float* out,
                               rvc_stream_t stream) {
    RVC_CHECK_ARG(x && ids && out, "gather_rows: null pointer");
    RVC_CHECK_ARG(dim_ok(d), "gather_rows: d=%lld must be a multiple of 8 in [8, 1024]", (long long)d);
    RVC_CHECK_ARG(m >= 1 && m <= NMAX, "gather_rows: bad size m=%lld", (long long)m);
    RVC_CHECK_ARG(aligned16(x) && aligned16(out), "gather_rows: 16-byte aligned arrays");
    hipLaunchKernelGGL(gather_rows_kernel, dim3(cdiv(m * (d / 4), 256)), dim3(256), 0, (hipStream_t)stream, x,
                       (int)(d / 4), ids, m, out);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

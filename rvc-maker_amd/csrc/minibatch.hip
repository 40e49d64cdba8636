// The reduction of create_index.py:63-76 on the device: sklearn's MiniBatchKMeans (1.7.2, dense, unit sample weights)
// step by step.  A step is rvc_gather_rows (the batch), rvc_minibatch_assign (kmeans.hip's assignment, k > n allowed),
// rvc_kmeans_lists (the batch's CSR lists) and the kernels of this file.  Host control (the RandomState, the loop,
// which centres are reassigned, the stopping rule) is rvc_amd/index_train.py.
//
//   minibatch_update_kernel   _minibatch_update_dense: one thread per (centre, 4 dimensions): row = centre * weight (an
//                             f32 product rounded on its own), += the members in batch order (ascending list position),
//                             *= 1.f / (weight + members); a centre with no member is copied.  Reads the weights only.
//   minibatch_weights_kernel  weight_sums[c] += members, after every thread of the update has read the old weight
//   minibatch_rowdist_kernel  one wave per row: sum over the dimensions of ((double)x - (double)c)^2, the lanes' partial
//                             sums met in a fixed xor tree
//   minibatch_status_kernel   one block: the rows' sums added in a fixed order (thread t takes rows t, t + 256, ...; an
//                             LDS tree over the threads) -> status.inertia; the weights' maximum and whether one is 0
//   minibatch_scatter_kernel  cent[dst[i]] = xb[src[i]], weight_sums[dst[i]] = v (the reassigned centres)
//
// No contraction anywhere in the file: the update is compared bit for bit with sklearn's arithmetic, where the product
// centre * weight and the first add are two roundings.  No floating-point atomics: two runs give identical bits.
#include "rvc_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int64_t NMAX = (1ll << 31) - 4096;

struct Status {  // rvc_minibatch_status_bytes() = 32
    double inertia;
    float wmax;
    int32_t any_zero;
    int64_t reserved[2];
};
static_assert(sizeof(Status) == 32, "status block layout");

__global__ __launch_bounds__(256) void minibatch_update_kernel(const float* __restrict__ xb, int64_t n, int d4,
                                                               const int64_t* __restrict__ list_off,
                                                               const int64_t* __restrict__ ids, int64_t k,
                                                               const float* __restrict__ prev,
                                                               const float* __restrict__ weight_sums, float* out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= k * d4) return;
    const int64_t c = t / d4;
    const int ch = (int)(t - c * d4);
    int64_t o0 = list_off[c], o1 = list_off[c + 1];
    o0 = o0 < 0 ? 0 : o0;
    o1 = o1 > n ? n : o1;
    const float4 p = ((const float4*)prev)[t];
    if (o1 <= o0) {
        ((float4*)out)[t] = p;
        return;
    }
    const float w = weight_sums[c];
    float4 s = make_float4(p.x * w, p.y * w, p.z * w, p.w * w);
    const float4* x4 = (const float4*)xb + ch;
    auto row = [&](int64_t v) {
        const int64_t r = ids[v];
        return x4[(r < 0 ? 0 : (r >= n ? n - 1 : r)) * d4];
    };
    auto add = [&](const float4& a) {
        s.x = s.x + a.x, s.y = s.y + a.y, s.z = s.z + a.z, s.w = s.w + a.w;
    };
    int64_t v = o0;
    for (; v + 4 <= o1; v += 4) {  // four rows in flight, added in order
        const float4 a0 = row(v), a1 = row(v + 1), a2 = row(v + 2), a3 = row(v + 3);
        add(a0), add(a1), add(a2), add(a3);
    }
    for (; v < o1; ++v) add(row(v));
    const float alpha = 1.f / (w + (float)(o1 - o0));
    ((float4*)out)[t] = make_float4(s.x * alpha, s.y * alpha, s.z * alpha, s.w * alpha);
}

__global__ __launch_bounds__(256) void minibatch_weights_kernel(const int64_t* __restrict__ list_off, int64_t n,
                                                                int64_t k, float* weight_sums) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= k) return;
    int64_t o0 = list_off[c], o1 = list_off[c + 1];
    o0 = o0 < 0 ? 0 : o0;
    o1 = o1 > n ? n : o1;
    if (o1 > o0) weight_sums[c] = weight_sums[c] + (float)(o1 - o0);
}

RVC_DEV double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void minibatch_rowdist_kernel(const float* __restrict__ xb, int64_t n, int d4,
                                                                const float* __restrict__ cent, int64_t k,
                                                                const int32_t* __restrict__ assign, double* rowsum) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n) return;
    int64_t a = assign[r];
    a = a < 0 ? 0 : (a >= k ? k - 1 : a);
    const float4* xp = (const float4*)xb + r * d4;
    const float4* cp = (const float4*)cent + a * d4;
    double s = 0.0;
    for (int c = lane; c < d4; c += 64) {
        const float4 x = xp[c], m = cp[c];
        const double e0 = (double)x.x - (double)m.x, e1 = (double)x.y - (double)m.y;
        const double e2 = (double)x.z - (double)m.z, e3 = (double)x.w - (double)m.w;
        s = s + e0 * e0;
        s = s + e1 * e1;
        s = s + e2 * e2;
        s = s + e3 * e3;
    }
    s = wave_sum_f64(s);
    if (lane == 0) rowsum[r] = s;
}

__global__ __launch_bounds__(256) void minibatch_status_kernel(const double* __restrict__ rowsum, int64_t n,
                                                               const float* __restrict__ weight_sums, int64_t k,
                                                               Status* status) {
    __shared__ double sh[256];
    __shared__ float mx[256];
    __shared__ int zr[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int64_t i = t; i < n; i += 256) s = s + rowsum[i];
    float m = 0.f;
    int z = 0;
    if (weight_sums)
        for (int64_t c = t; c < k; c += 256) {
            const float w = weight_sums[c];
            m = fmaxf(m, w);
            z |= w == 0.f;
        }
    sh[t] = s, mx[t] = m, zr[t] = z;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            sh[t] = sh[t] + sh[t + o];
            mx[t] = fmaxf(mx[t], mx[t + o]);
            zr[t] |= zr[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        status->inertia = sh[0];
        status->wmax = mx[0];
        status->any_zero = zr[0];
        status->reserved[0] = 0;
        status->reserved[1] = 0;
    }
}

__global__ __launch_bounds__(256) void minibatch_scatter_kernel(const float* __restrict__ xb, int64_t n, int d4,
                                                                const int64_t* __restrict__ src,
                                                                const int64_t* __restrict__ dst, int64_t m, float v,
                                                                float* cent, int64_t k, float* weight_sums) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= m * d4) return;
    const int64_t i = t / d4;
    const int ch = (int)(t - i * d4);
    const int64_t to = dst[i];
    if (to < 0 || to >= k) return;
    if (ch == 0) weight_sums[to] = v;
    int64_t from = src[i];
    from = from < 0 ? 0 : (from >= n ? n - 1 : from);
    ((float4*)cent)[to * d4 + ch] = ((const float4*)xb)[from * d4 + ch];
}

bool dim_ok(int64_t d) { return d >= 8 && d <= 1024 && d % 8 == 0; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

extern "C" int rvc_minibatch_update(const float* xb, int64_t n, int64_t d, const int64_t* list_off, const int64_t* ids,
                                    int64_t k, const float* cent_prev, float* weight_sums, float* cent_out,
                                    rvc_stream_t stream) {
    RVC_CHECK_ARG(xb && list_off && ids && cent_prev && weight_sums && cent_out, "minibatch_update: null pointer");
    RVC_CHECK_ARG(dim_ok(d), "minibatch_update: d=%lld must be a multiple of 8 in [8, 1024]", (long long)d);
    RVC_CHECK_ARG(n >= 1 && k >= 1 && n <= NMAX && k <= NMAX, "minibatch_update: bad sizes n=%lld k=%lld", (long long)n,
                  (long long)k);
    RVC_CHECK_ARG(aligned16(xb) && aligned16(cent_prev) && aligned16(cent_out),
                  "minibatch_update: 16-byte aligned arrays");
    RVC_CHECK_ARG(cent_prev != cent_out, "minibatch_update: cent_out must not alias cent_prev");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(minibatch_update_kernel, dim3(cdiv(k * (d / 4), 256)), dim3(256), 0, s, xb, n, (int)(d / 4),
                       list_off, ids, k, cent_prev, (const float*)weight_sums, cent_out);
    hipLaunchKernelGGL(minibatch_weights_kernel, dim3(cdiv(k, 256)), dim3(256), 0, s, list_off, n, k, weight_sums);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int64_t rvc_minibatch_status_bytes(void) { return (int64_t)sizeof(Status); }

extern "C" int64_t rvc_minibatch_inertia_work_bytes(int64_t n) {
    if (n < 1 || n > NMAX) return -1;
    return n * 8;  // the rows' f64 sums
}

extern "C" int rvc_minibatch_inertia(const float* xb, int64_t n, int64_t d, const float* cent, int64_t k,
                                     const int32_t* assign, const float* weight_sums, void* work, int64_t work_bytes,
                                     void* status, rvc_stream_t stream) {
    RVC_CHECK_ARG(xb && cent && assign && work && status, "minibatch_inertia: null pointer");
    RVC_CHECK_ARG(dim_ok(d), "minibatch_inertia: d=%lld must be a multiple of 8 in [8, 1024]", (long long)d);
    RVC_CHECK_ARG(n >= 1 && k >= 1 && n <= NMAX && k <= NMAX, "minibatch_inertia: bad sizes n=%lld k=%lld",
                  (long long)n, (long long)k);
    RVC_CHECK_ARG(work_bytes >= rvc_minibatch_inertia_work_bytes(n), "minibatch_inertia: workspace too small");
    RVC_CHECK_ARG(aligned16(xb) && aligned16(cent) && aligned16(work) && ((uintptr_t)status & 7) == 0,
                  "minibatch_inertia: xb, cent, work 16-byte aligned, status 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(minibatch_rowdist_kernel, dim3(cdiv(n, 4)), dim3(256), 0, s, xb, n, (int)(d / 4), cent, k, assign,
                       (double*)work);
    hipLaunchKernelGGL(minibatch_status_kernel, dim3(1), dim3(256), 0, s, (const double*)work, n, weight_sums, k,
                       (Status*)status);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_minibatch_scatter(const float* xb, int64_t n, int64_t d, const int64_t* src, const int64_t* dst,
                                     int64_t m, float v, float* cent, int64_t k, float* weight_sums,
                                     rvc_stream_t stream) {
    RVC_CHECK_ARG(xb && src && dst && cent && weight_sums, "minibatch_scatter: null pointer");
    RVC_CHECK_ARG(dim_ok(d), "minibatch_scatter: d=%lld must be a multiple of 8 in [8, 1024]", (long long)d);
    RVC_CHECK_ARG(n >= 1 && k >= 1 && m >= 1 && n <= NMAX && k <= NMAX && m <= k,
                  "minibatch_scatter: bad sizes n=%lld k=%lld m=%lld (1 <= m <= k)", (long long)n, (long long)k,
                  (long long)m);
    RVC_CHECK_ARG(aligned16(xb) && aligned16(cent), "minibatch_scatter: 16-byte aligned arrays");
    hipLaunchKernelGGL(minibatch_scatter_kernel, dim3(cdiv(m * (d / 4), 256)), dim3(256), 0, (hipStream_t)stream, xb, n,
                       (int)(d / 4), src, dst, m, v, cent, k, weight_sums);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

// hybrid[a+b+...] f0 (VC.get_f0_hybrid, convert.py:283-302) on the device: the 0.999 |x| quantile every member's
// input is divided by, and the resample-and-median mix of the members' raw tracks.
//
//   abs_quantile   np.quantile(np.abs(x), 0.999) of f32 x as the installed NumPy (2.x) evaluates it for an f32
//                  array: q, the virtual index (n - 1) q, gamma and the lerp are all f32.  The two order
//                  statistics come from a radix select on the bit patterns of |x| (non-negative floats order
//                  as their bits do): three 11 / 11 / 9-bit histogram passes (LDS histograms per block, added
//                  into the global one), every block of a pass re-deriving the earlier passes' selections from
//                  their histograms, then the successor's minimum and the lerp.  No sort.
//   div_scalar     x / q element-wise, a true f32 division by the device scalar
//   f0_mix         per output frame: np.interp(np.linspace(0, n_m, p_len)[k], np.arange(n_m), f0_m) in f64 for
//                  every track, then np.nanmedian over the tracks (the resampled track itself for one)
//   f0_resample_nan  get_f0_mangio_crepe's tail (convert.py:226-228): values below 0.001 -> NaN, np.interp onto
//                  p_len frames (the same np.interp device function as f0_mix), np.nan_to_num
// The f64 post (autotune / shift / f0 file / quantiser) of the mixed track is rvc_pm_post with nf = p_len.
#include "rvc_common.h"
#include <algorithm>

namespace {

constexpr int QT = 1024;     // threads of a select block
constexpr int QB = 2048;     // histogram bins per pass
constexpr int QPER = 8;      // samples per thread and pass
constexpr int QMAXBLK = 256;

struct MixTracks {
    const void* f0[RVC_F0_MIX_MAX];
    int64_t n[RVC_F0_MIX_MAX];
    int is64[RVC_F0_MIX_MAX];
    int M;
};

// work: three histograms (one per radix pass) and the successor cell, zeroed before the first pass
struct QWork {
    unsigned hist[3][QB];
    unsigned succ_inv;  // ~(the smallest pattern above rank k0's), folded with atomicMax
};

struct QSel {
    unsigned prefix;   // the selected high bits so far
    unsigned k;        // the rank looked for among the samples sharing them
    unsigned below;    // samples smaller than every sample sharing them
    unsigned cnt;      // samples sharing them
};

__device__ __forceinline__ int q_shift(int pass) { return pass == 0 ? 20 : (pass == 1 ? 9 : 0); }
__device__ __forceinline__ unsigned q_mask(int pass) { return pass == 2 ? 0x1ffu : 0x7ffu; }
__device__ __forceinline__ unsigned q_himask(int pass) { return pass == 0 ? 0u : (pass == 1 ? 0x7ff00000u : 0x7ffffe00u); }

// NumPy's index arithmetic for np.quantile(f32 array, 0.999): q, the virtual index (n - 1) q and gamma are f32
__device__ __forceinline__ void q_index(int64_t n, int64_t* k0, int64_t* k1, float* gamma) {
#pragma clang fp contract(off)
    const float q = 0.999f;
    const float virt = (float)(n - 1) * q;
    const float prevf = floorf(virt);
    *k0 = (int64_t)prevf;
    *k1 = *k0 + 1;
    *gamma = virt - prevf;
    if (virt >= (float)(n - 1)) *k0 = *k1 = n - 1;  // _get_indexes: above bounds takes the maximum
}

// By every thread of a QT-thread block: the bin of hist [QB] holding rank sel.k, folded into sel.  Thread t sums
// bins 2t and 2t + 1, a Hillis-Steele scan over the QT sums in LDS, and the one thread whose range holds the rank
// publishes the answer.
__device__ void q_select(const unsigned* hist, int pass, QSel& sel, unsigned* scan, unsigned* res) {
    const int tid = threadIdx.x;
    const unsigned h0 = hist[2 * tid], h1 = hist[2 * tid + 1];
    unsigned v = h0 + h1;
    scan[tid] = v;
    __syncthreads();
    for (int o = 1; o < QT; o <<= 1) {
        const unsigned add = tid >= o ? scan[tid - o] : 0u;
        __syncthreads();
        v += add;
        scan[tid] = v;
        __syncthreads();
    }
    const unsigned excl = v - (h0 + h1);
    if (excl <= sel.k && sel.k < v) {
        const bool first = sel.k < excl + h0;
        res[0] = 2 * tid + (first ? 0 : 1);
        res[1] = first ? excl : excl + h0;
        res[2] = first ? h0 : h1;
    }
    __syncthreads();
    sel.prefix |= res[0] << q_shift(pass);
    sel.k -= res[1];
    sel.below += res[1];
    sel.cnt = res[2];
    __syncthreads();
}

// radix pass PASS over the bit patterns of |x|: the selections of the earlier passes are recomputed by every
// block from their (complete) histograms; a block's counts go through an LDS histogram
template <int PASS>
__global__ __launch_bounds__(QT) void q_hist_kernel(const float* x, int64_t n, QWork* w) {
    __shared__ unsigned lh[QB];
    __shared__ unsigned scan[QT];
    __shared__ unsigned res[3];
    const int tid = threadIdx.x;
    int64_t k0, k1;
    float gamma;
    q_index(n, &k0, &k1, &gamma);
    QSel sel = {0u, (unsigned)k0, 0u, 0u};
    for (int p = 0; p < PASS; ++p) q_select(w->hist[p], p, sel, scan, res);
    for (int b = tid; b < QB; b += QT) lh[b] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * QT + tid; i < n; i += (int64_t)gridDim.x * QT) {
        const unsigned u = __float_as_uint(x[i]) & 0x7fffffffu;
        if ((u & q_himask(PASS)) == sel.prefix) atomicAdd(&lh[(u >> q_shift(PASS)) & q_mask(PASS)], 1u);
    }
    __syncthreads();
    for (int b = tid; b < QB; b += QT)
        if (lh[b]) atomicAdd(&w->hist[PASS][b], lh[b]);
}

// rank k0 + 1 is rank k0's value when more copies of it remain, the smallest larger pattern otherwise
__global__ __launch_bounds__(QT) void q_succ_kernel(const float* x, int64_t n, QWork* w) {
    __shared__ unsigned scan[QT];
    __shared__ unsigned res[3];
    const int tid = threadIdx.x;
    int64_t k0, k1;
    float gamma;
    q_index(n, &k0, &k1, &gamma);
    QSel sel = {0u, (unsigned)k0, 0u, 0u};
    for (int p = 0; p < 3; ++p) q_select(w->hist[p], p, sel, scan, res);
    if (k1 == k0 || (int64_t)sel.below + sel.cnt > k1) return;
    unsigned m = 0xffffffffu;
    for (int64_t i = (int64_t)blockIdx.x * QT + tid; i < n; i += (int64_t)gridDim.x * QT) {
        const unsigned u = __float_as_uint(x[i]) & 0x7fffffffu;
        if (u > sel.prefix) m = min(m, u);
    }
    scan[tid] = m;
    __syncthreads();
    for (int o = QT / 2; o > 0; o >>= 1) {
        if (tid < o) scan[tid] = min(scan[tid], scan[tid + o]);
        __syncthreads();
    }
    if (tid == 0 && scan[0] != 0xffffffffu) atomicMax(&w->succ_inv, ~scan[0]);
}

__global__ __launch_bounds__(QT) void q_final_kernel(int64_t n, QWork* w, int fused, float* out) {
#pragma clang fp contract(off)
    __shared__ unsigned scan[QT];
    __shared__ unsigned res[3];
    int64_t k0, k1;
    float gamma;
    q_index(n, &k0, &k1, &gamma);
    QSel sel = {0u, (unsigned)k0, 0u, 0u};
    for (int p = 0; p < 3; ++p) q_select(w->hist[p], p, sel, scan, res);
    if (threadIdx.x != 0) return;
    const bool same = k1 == k0 || (int64_t)sel.below + sel.cnt > k1;
    // _lerp: a + (b - a) t, and b - (b - a)(1 - t) where t >= 0.5
    const float a = __uint_as_float(sel.prefix), b = same ? a : __uint_as_float(~w->succ_inv);
    const float diff = b - a;
    float r = a + diff * gamma;
    if (gamma >= 0.5f) r = b - diff * (1.f - gamma);
    // torch.quantile's lerp (ATen's CPU lerp): the same two branches, each one fused multiply-add
    if (fused) r = gamma < 0.5f ? fmaf(gamma, diff, a) : fmaf(gamma - 1.f, diff, b);
    out[0] = r;
}

__global__ __launch_bounds__(256) void div_scalar_kernel(const float* x, int64_t n, const float* q, float* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = __fdiv_rn(x[i], q[0]);
}

__device__ __forceinline__ double track_at(const MixTracks& t, int m, int64_t j) {
    return t.is64[m] ? ((const double*)t.f0[m])[j] : (double)((const float*)t.f0[m])[j];
}

// np.interp(xq, np.arange(n), fp) for one query xq >= 0 in f64, as NumPy's arr_interp evaluates it: right of
// xp[-1] -> fp[-1]; an exact hit (and the last node) -> fp[j]; else slope * (xq - j) + fp[j], with NumPy's two NaN
// fallbacks (the other end point, then the common value of two equal end points).  fp(j) fetches node j as f64.
template <typename Fetch>
__device__ __forceinline__ double np_interp_arange(double xq, int64_t n, Fetch fp) {
#pragma clang fp contract(off)
    if (xq > (double)(n - 1)) return fp(n - 1);
    int64_t j = (int64_t)floor(xq);
    if (j > n - 1) j = n - 1;
    const double f0 = fp(j);
    if (j == n - 1 || (double)j == xq) return f0;
    const double f1 = fp(j + 1);
    const double slope = (f1 - f0) / ((double)(j + 1) - (double)j);
    double r = slope * (xq - (double)j) + f0;
    if (r != r) {  // numpy's NaN rescue (an infinite or NaN end point)
        r = slope * (xq - (double)(j + 1)) + f1;
        if (r != r && f0 == f1) r = f0;
    }
    return r;
}

__global__ __launch_bounds__(256) void f0_mix_kernel(MixTracks t, int64_t p_len, double* out) {
#pragma clang fp contract(off)
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= p_len) return;
    double v[RVC_F0_MIX_MAX];
    int cnt = 0;
    double single = 0.0;
    for (int m = 0; m < t.M; ++m) {
        const int64_t n = t.n[m];
        // np.linspace(0, n, p_len): arange(p_len) * ((n - 0) / (p_len - 1)) + 0, the last point set to n
        const double step = (double)n / (double)(p_len - 1);
        const double xq = k == p_len - 1 ? (double)n : (double)k * step + 0.0;
        const double r = np_interp_arange(xq, n, [&](int64_t j) { return track_at(t, m, j); });
        single = r;
        if (r == r) {  // nanmedian drops NaNs; insertion into the sorted prefix
            int p = cnt++;
            while (p > 0 && v[p - 1] > r) {
                v[p] = v[p - 1];
                --p;
            }
            v[p] = r;
        }
    }
    double res;
    if (t.M == 1) res = single;
    else if (cnt == 0) res = __longlong_as_double(0x7ff8000000000000ll);
    else if (cnt & 1) res = v[cnt / 2];
    else res = (v[cnt / 2 - 1] + v[cnt / 2]) / 2.0;
    out[k] = res;
}

// get_f0_mangio_crepe's tail (convert.py:226-228) per output frame k: source[source < 0.001] = nan (an f32 compare),
// np.interp(k * T / p_len, np.arange(T), source) in f64, np.nan_to_num
__global__ __launch_bounds__(256) void f0_resample_nan_kernel(const float* src, int64_t T, int64_t p_len, double* out) {
#pragma clang fp contract(off)
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= p_len) return;
    const double xq = (double)(k * T) / (double)p_len;  // np.arange(0, T * p_len, T) / p_len
    double r = np_interp_arange(xq, T, [&](int64_t j) {
        const float s = src[j];
        return s < 0.001f ? __longlong_as_double(0x7ff8000000000000ll) : (double)s;
    });
    if (r != r) r = 0.0;  // nan_to_num: nan -> 0, +-inf -> the largest finite f64
    else if (r > 1.7976931348623157e308) r = 1.7976931348623157e308;
    else if (r < -1.7976931348623157e308) r = -1.7976931348623157e308;
    out[k] = r;
}

}  // namespace

extern "C" int64_t rvc_abs_quantile_work_bytes(void) { return (int64_t)sizeof(QWork); }

extern "C" int rvc_abs_quantile(const float* x, int64_t n, void* work, int64_t work_bytes, float* q_out,
                                rvc_stream_t stream) {
    return rvc_abs_quantile_as(x, n, RVC_QUANTILE_NUMPY, work, work_bytes, q_out, stream);
}

extern "C" int rvc_abs_quantile_as(const float* x, int64_t n, int lerp, void* work, int64_t work_bytes, float* q_out,
                                   rvc_stream_t stream) {
    RVC_CHECK_ARG(x && work && q_out, "abs_quantile: null pointer");
    RVC_CHECK_ARG(lerp == RVC_QUANTILE_NUMPY || lerp == RVC_QUANTILE_TORCH, "abs_quantile: unknown lerp %d", lerp);
    RVC_CHECK_ARG(n > 0 && n < (1ll << 31), "abs_quantile: bad length %lld", (long long)n);
    RVC_CHECK_ARG(work_bytes >= (int64_t)sizeof(QWork), "abs_quantile: work buffer too small");
    hipStream_t s = (hipStream_t)stream;
    QWork* w = (QWork*)work;
    const unsigned nb = std::min(cdiv(n, (int64_t)QT * QPER), (unsigned)QMAXBLK);
    RVC_HIP(hipMemsetAsync(w, 0, sizeof(QWork), s));
    hipLaunchKernelGGL(q_hist_kernel<0>, dim3(nb), dim3(QT), 0, s, x, n, w);
    hipLaunchKernelGGL(q_hist_kernel<1>, dim3(nb), dim3(QT), 0, s, x, n, w);
    hipLaunchKernelGGL(q_hist_kernel<2>, dim3(nb), dim3(QT), 0, s, x, n, w);
    hipLaunchKernelGGL(q_succ_kernel, dim3(nb), dim3(QT), 0, s, x, n, w);
    hipLaunchKernelGGL(q_final_kernel, dim3(1), dim3(QT), 0, s, n, w, lerp == RVC_QUANTILE_TORCH ? 1 : 0,
                       q_out);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_div_scalar(const float* x, int64_t n, const float* q, float* out, rvc_stream_t stream) {
    RVC_CHECK_ARG(x && q && out, "div_scalar: null pointer");
    RVC_CHECK_ARG(n > 0, "div_scalar: bad length %lld", (long long)n);
    hipLaunchKernelGGL(div_scalar_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, n, q, out);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_f0_mix(const rvc_f0_track* tracks, int M, int64_t p_len, double* out, rvc_stream_t stream) {
    RVC_CHECK_ARG(tracks && out, "f0_mix: null pointer");
    RVC_CHECK_ARG(M >= 1 && M <= RVC_F0_MIX_MAX, "f0_mix: %d tracks (1..%d)", M, RVC_F0_MIX_MAX);
    RVC_CHECK_ARG(p_len >= 2, "f0_mix: p_len %lld < 2", (long long)p_len);
    MixTracks t;
    t.M = M;
    for (int m = 0; m < M; ++m) {
        RVC_CHECK_ARG(tracks[m].f0 && tracks[m].n > 0, "f0_mix: track %d is empty", m);
        t.f0[m] = tracks[m].f0;
        t.n[m] = tracks[m].n;
        t.is64[m] = tracks[m].is_f64;
    }
    hipLaunchKernelGGL(f0_mix_kernel, dim3(cdiv(p_len, 256)), dim3(256), 0, (hipStream_t)stream, t, p_len, out);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_f0_resample_nan(const float* source, int64_t T, int64_t p_len, double* out, rvc_stream_t stream) {
    RVC_CHECK_ARG(source && out, "f0_resample_nan: null pointer");
    RVC_CHECK_ARG(T >= 1 && p_len >= 1 && T < (1ll << 31) && p_len < (1ll << 31),
                  "f0_resample_nan: bad lengths %lld, %lld", (long long)T, (long long)p_len);
    hipLaunchKernelGGL(f0_resample_nan_kernel, dim3(cdiv(p_len, 256)), dim3(256), 0, (hipStream_t)stream, source, T,
                       p_len, out);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

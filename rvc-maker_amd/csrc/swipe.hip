// SWIPE' f0 on the device (main/library/predictors/SWIPE.py as VC.get_f0_swipe calls it: 16 kHz, floor 50 Hz,
// ceiling 1100 Hz, 10 ms frames, strength threshold 0.3), then get_f0's autotune / shift / f0 file / mel
// quantiser in f32 (the reference's swipe f0 is an f32 array).  All of the estimator is f64 on the f32 samples
// promoted exactly, as the reference computes it.
//
// The method in matrix form.  429 pitch candidates pc (1/96 octave apart), 328 ERB-spaced frequencies fERBs,
// five window sizes ws = 2048 .. 128 (hop ws/2, Hann window, the signal zero-padded by ws/2 in front and ws
// behind).  Per window size i:
//     A_i  [frame][bin]   = |FFT(frame x window)| / sum(window)                     (mlab.specgram, mode complex)
//     M_i                 = max(0, W_i A_i),   W_i [328][ws/2 + 1]  the not-a-knot cubic spline onto fERBs
//                           (linear in its data, so a constant matrix: the spline of each unit vector)
//     L_i                 = sqrt(M_i) / ||sqrt(M_i)||_2 per frame                   (2.22e-16 for a zero norm)
//     S_i  [cand][frame]  = K_i L_i,           K_i the prime-harmonic cosine kernel of the candidates i serves
// then S [429][F] = sum_i mu_i * (S_i linearly interpolated in time to t = k 10 ms): every candidate is served
// by at most two adjacent window sizes, added in window order.  Per frame: argmax over the candidates, the 0.3
// threshold, a parabola through the three neighbours and the 17-point 1/768-octave grid.
//
// Launch plan (every stage is ONE launch over all five window sizes; no synchronisation, no allocation):
//   sw_fft       a block per 2048 / ws frames of a window size: frame x window -> radix-2 f64 FFTs side by side
//                in LDS (twiddles from a table) -> A_i
//   sw_gemm<0>   W_i A_i on the f64 matrix cores; a block owns 16 frames and all 336 (= 328 padded) rows, so
//                the clamp, sqrt and per-frame L2 norm are its epilogue -> L_i (336 per frame)
//   sw_gemm<1>   K_i L_i, the same kernel with a plain epilogue -> S_i [cand][frame]
//   sw_sum       one thread per (candidate, output frame): the time lerps, mu and the sum -> S (no atomics)
//   sw_pick      argmax (first index on ties), threshold, parabola, grid -> f0 f32 [F]
// Both GEMMs are Out[m][f] = sum_k P[m][k] Q[f][k].  All four operands are stored in MFMA operand order
// (sw_pack: [16-row tile][K / 16][lane][4 k steps]), the constant ones by the host, A_i and L_i by the kernels
// that produce them (the MFMA's D layout is the next GEMM's operand layout, so L_i is one 32-byte store per lane
// and tile): every wave load is 2 KB in a row and there is no LDS staging.  K is padded to a multiple of 16
// with zeros.  (Row-major operands read 32 bytes per lane at a row stride: 64 cache lines per wave load, each
// fetched four times over -- the loudness GEMM then took 212-305 us against 21 us of MFMAs.)
//
// The tables (pc, fERBs, windows, W_i, K_i, the candidate map, the pick grids) are built on the HOST by
// rvc_swipe_tables into one blob the caller uploads once.
#include "rvc_common.h"
#include <string.h>
#include <vector>

typedef double doublex4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int SW_NW = 5;          // window sizes 2048 >> i
constexpr int SW_NC = 429;        // pitch candidates
constexpr int SW_NE = 328;        // fERBs
constexpr int SW_NEP = 336;       // ... padded to a multiple of 16
constexpr int SW_NG = 17;         // pick grid points
constexpr int SW_FS = 16000;
constexpr int SW_HOPOUT = 160;    // 10 ms
constexpr double SW_THR = 0.3;
constexpr int SW_TF = 16;         // frames per GEMM block
constexpr int SW_GT = 512;        // threads of a GEMM block (8 waves)
constexpr int SW_MTW = 3;         // row tiles per wave (ceil(21 / 8))

constexpr int sw_ws(int i) { return 2048 >> i; }
constexpr int sw_hop(int i) { return 1024 >> i; }
constexpr int sw_nbin(int i) { return (1024 >> i) + 1; }
constexpr int sw_kpad(int i) { return ((1024 >> i) + 16) / 16 * 16; }   // nbin rounded up to 16
inline int pad16(int v) { return (v + 15) / 16 * 16; }
inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }
inline int64_t sw_nfr(int i, int64_t n) { return n / sw_hop(i) + 2; }

// ---------------------------------------------------------------- host tables
enum {
    T_PC = 0, T_FERBS, T_IDX, T_MU, T_W, T_K, T_WIN, T_TW, T_CMAP, T_CMU, T_PX, T_GRIDX, T_GRIDF0, T_WP, T_KP, T_COUNT
};

struct SwLayout {
    int nc[SW_NW];                  // candidates per window size
    int64_t off[T_COUNT][SW_NW];    // byte offsets (per-window tables use [which][i], the others [which][0])
    int64_t bytes;
};

struct SwHost {
    double log2pc[SW_NC], pc[SW_NC], d[SW_NC], ferbs[SW_NE];
    std::vector<int> j[SW_NW];
    std::vector<double> mu[SW_NW];
};

// the reference's sieve (SWIPE.py:123-140), statement for statement: multiples of num are struck while
// num < sqrt(n), so n itself survives when it is a prime's square
std::vector<int> sw_sieve(int n) {
    std::vector<char> in(n + 2 > 0 ? n + 2 : 2, 0);
    for (int v = 2; v <= n; ++v) in[v] = 1;
    int num = 2;
    while ((double)num < sqrt((double)n)) {
        for (int i = 2 * num; i <= n + num; i += num)
            if (i <= n) in[i] = 0;
        for (int v = num + 1; v <= n; ++v)
            if (in[v]) {
                num = v;
                break;
            }
    }
    std::vector<int> out;
    for (int v = 2; v <= n; ++v)
        if (in[v]) out.push_back(v);
    return out;
}

void sw_host(SwHost& h) {
#pragma clang fp contract(off)
    const double lo = log2(50.0) * 96.0, hi = log2(1100.0) * 96.0;
    const int npc = (int)ceil(hi - lo);  // np.arange(lo, hi): 429
    for (int k = 0; k < SW_NC && k < npc; ++k) {
        h.log2pc[k] = (lo + (double)k) * (1.0 / 96.0);
        h.pc[k] = pow(2.0, h.log2pc[k]);
    }
    const double l0 = log2(4.0 * 2.0 * SW_FS / 2048.0);
    for (int k = 0; k < SW_NC; ++k) h.d[k] = 1.0 + h.log2pc[k] - l0;
    // fERBs = erbs2hz(np.arange(hz2erbs(pc[0] / 4), hz2erbs(fs / 2), 0.1)): arange fills start + k * delta
    // with delta = (start + 0.1) - start
    const double e0 = 21.4 * log10(1.0 + (h.pc[0] / 4.0) / 229.0);
    const double delta = (e0 + 0.1) - e0;
    for (int k = 0; k < SW_NE; ++k) h.ferbs[k] = (pow(10.0, (e0 + (double)k * delta) / 21.4) - 1.0) * 229.0;
    for (int i = 0; i < SW_NW; ++i) {
        h.j[i].clear();
        h.mu[i].clear();
        for (int c = 0; c < SW_NC; ++c) {
            const double dd = h.d[c] - (double)(i + 1);
            bool in, tap;
            if (i == SW_NW - 1) { in = dd > -1.0; tap = dd < 0.0; }
            else if (i == 0) { in = dd < 1.0; tap = dd > 0.0; }
            else { in = fabs(dd) < 1.0; tap = true; }
            if (!in) continue;
            h.j[i].push_back(c);
            h.mu[i].push_back(tap ? 1.0 - fabs(h.d[c] - (double)i - 1.0) : 1.0);
        }
    }
}

SwLayout sw_layout(const SwHost& h) {
    SwLayout L;
    memset(&L, 0, sizeof(L));
    size_t o = 0;
    auto put = [&](int which, int i, size_t b) {
        L.off[which][i] = (int64_t)o;
        o += align256(b);
    };
    put(T_PC, 0, sizeof(double) * SW_NC);
    put(T_FERBS, 0, sizeof(double) * SW_NE);
    put(T_TW, 0, sizeof(double) * 2 * 1024);
    put(T_CMAP, 0, sizeof(int) * SW_NC * 4);
    put(T_CMU, 0, sizeof(double) * SW_NC * 2);
    put(T_PX, 0, sizeof(double) * SW_NC * 2);
    put(T_GRIDX, 0, sizeof(double) * SW_NC * SW_NG);
    put(T_GRIDF0, 0, sizeof(float) * SW_NC * SW_NG);
    for (int i = 0; i < SW_NW; ++i) {
        L.nc[i] = (int)h.j[i].size();
        put(T_IDX, i, sizeof(int) * L.nc[i]);
        put(T_MU, i, sizeof(double) * L.nc[i]);
        put(T_W, i, sizeof(double) * SW_NEP * sw_kpad(i));
        put(T_K, i, sizeof(double) * pad16(L.nc[i]) * SW_NEP);
        put(T_WIN, i, sizeof(double) * (sw_ws(i) + 1));  // the window, then its sum
        put(T_WP, i, sizeof(double) * SW_NEP * sw_kpad(i));        // W and K again, in MFMA operand order
        put(T_KP, i, sizeof(double) * pad16(L.nc[i]) * SW_NEP);
    }
    L.bytes = (int64_t)o;
    return L;
}

// W [SW_NEP][kpad]: column b = the not-a-knot cubic spline through the unit vector e_b on the nb uniform
// bins, evaluated at u[e] = fERBs[e] / (fs / ws).  Second-derivative form with h = 1: interior rows
// m[i-1] + 4 m[i] + m[i+1] = 6 (y[i-1] - 2 y[i] + y[i+1]); the not-a-knot ends m[0] - 2 m[1] + m[2] = 0 (and
// its mirror) turn rows 1 and nb - 2 into 6 m[1] = rhs[1], 6 m[nb-2] = rhs[nb-2]; Thomas in between.
void sw_spline(const double* ferbs, int ws, double* W, int kpad) {
#pragma clang fp contract(off)
    const int nb = ws / 2 + 1;
    std::vector<double> cp(nb), m(nb), rhs(nb), dp(nb);
    std::vector<int> iv(SW_NE);
    std::vector<double> tt(SW_NE);
    for (int e = 0; e < SW_NE; ++e) {
        const double u = ferbs[e] * (double)ws / (double)SW_FS;
        int i = (int)floor(u);
        if (i > nb - 2) i = nb - 2;
        if (i < 0) i = 0;
        iv[e] = i;
        tt[e] = u - (double)i;
    }
    // the forward sweep's pivots do not depend on the data
    cp[2] = 1.0 / 4.0;
    for (int i = 3; i <= nb - 3; ++i) cp[i] = 1.0 / (4.0 - cp[i - 1]);
    for (int b = 0; b < nb; ++b) {
        for (int i = 0; i < nb; ++i) rhs[i] = 0.0;
        if (b - 1 >= 1 && b - 1 <= nb - 2) rhs[b - 1] += 6.0;
        if (b >= 1 && b <= nb - 2) rhs[b] += -12.0;
        if (b + 1 >= 1 && b + 1 <= nb - 2) rhs[b + 1] += 6.0;
        m[1] = rhs[1] / 6.0;
        m[nb - 2] = rhs[nb - 2] / 6.0;
        // rows 2 .. nb - 3 with m[1], m[nb-2] known
        for (int i = 2; i <= nb - 3; ++i) {
            double r = rhs[i];
            if (i == 2) r -= m[1];
            if (i == nb - 3) r -= m[nb - 2];
            dp[i] = i == 2 ? r / 4.0 : (r - dp[i - 1]) / (4.0 - cp[i - 1]);
        }
        for (int i = nb - 3; i >= 2; --i) m[i] = i == nb - 3 ? dp[i] : dp[i] - cp[i] * m[i + 1];
        m[0] = 2.0 * m[1] - m[2];
        m[nb - 1] = 2.0 * m[nb - 2] - m[nb - 3];
        for (int e = 0; e < SW_NE; ++e) {
            const int i = iv[e];
            const double t = tt[e], s = 1.0 - t;
            const double y0 = i == b ? 1.0 : 0.0, y1 = i + 1 == b ? 1.0 : 0.0;
            W[(size_t)e * kpad + b] = y0 * s + y1 * t + ((s * s * s - s) * m[i] + (t * t * t - t) * m[i + 1]) / 6.0;
        }
    }
}

// pitchStrengthOneCandidate's kernel over fERBs for the candidate frequency pc -> k [SW_NE]
void sw_kernel_row(const double* f, double pc, double* k) {
#pragma clang fp contract(off)
    std::vector<int> pr = sw_sieve((int)trunc(f[SW_NE - 1] / pc - 0.75));
    pr.insert(pr.begin(), 1);
    for (int e = 0; e < SW_NE; ++e) k[e] = 0.0;
    for (int prime : pr) {
        for (int e = 0; e < SW_NE; ++e) {
            const double q = f[e] / pc;
            const double a = fabs(q - (double)prime);
            if (a < 0.25) k[e] = cos(2.0 * M_PI * q);
            if (0.25 < a && a < 0.75) k[e] = k[e] + cos(2.0 * M_PI * q) / 2.0;
        }
    }
    double ss = 0.0;
    for (int e = 0; e < SW_NE; ++e) {
        k[e] *= sqrt(1.0 / f[e]);
        if (k[e] > 0.0) ss += k[e] * k[e];
    }
    const double nrm = sqrt(ss);
    for (int e = 0; e < SW_NE; ++e) k[e] /= nrm;
}

// MFMA operand order of a row-major [rows][K] matrix (rows, K multiples of 16): [row tile][K / 16][lane][u] holds
// src[16 tile + (lane & 15)][4 (4 k16 + u) + (lane >> 4)], so lane l of a wave reads, for four k steps at once,
// the 32 bytes at ((tile K/16 + k16) 64 + l) and the wave 2 KB in a row.  The frame-side operands (A_i, L_i) are
// written in the same order by the kernels that produce them.
void sw_pack(const double* src, int rows, int K, double* dst) {
    for (int tile = 0; tile < rows / 16; ++tile)
        for (int k16 = 0; k16 < K / 16; ++k16)
            for (int lane = 0; lane < 64; ++lane)
                for (int u = 0; u < 4; ++u)
                    dst[(((size_t)tile * (K / 16) + k16) * 64 + lane) * 4 + u] =
                        src[(size_t)(16 * tile + (lane & 15)) * K + 4 * (4 * k16 + u) + (lane >> 4)];
}

void sw_fill(const SwHost& h, const SwLayout& L, char* blob) {
#pragma clang fp contract(off)
    memset(blob, 0, (size_t)L.bytes);
    memcpy(blob + L.off[T_PC][0], h.pc, sizeof(double) * SW_NC);
    memcpy(blob + L.off[T_FERBS][0], h.ferbs, sizeof(double) * SW_NE);
    double* tw = (double*)(blob + L.off[T_TW][0]);  // exp(-2 pi i k / 2048), k < 1024
    for (int k = 0; k < 1024; ++k) {
        tw[2 * k] = cos(2.0 * M_PI * (double)k / 2048.0);
        tw[2 * k + 1] = -sin(2.0 * M_PI * (double)k / 2048.0);
    }
    int* cmap = (int*)(blob + L.off[T_CMAP][0]);  // [cand][slot](window, local index), -1 = none
    double* cmu = (double*)(blob + L.off[T_CMU][0]);
    for (int c = 0; c < SW_NC * 4; ++c) cmap[c] = -1;
    for (int i = 0; i < SW_NW; ++i) {
        int* idx = (int*)(blob + L.off[T_IDX][i]);
        double* mu = (double*)(blob + L.off[T_MU][i]);
        double* K = (double*)(blob + L.off[T_K][i]);
        for (int l = 0; l < L.nc[i]; ++l) {
            const int c = h.j[i][l];
            idx[l] = c;
            mu[l] = h.mu[i][l];
            const int slot = cmap[c * 4] < 0 ? 0 : 1;
            cmap[c * 4 + 2 * slot] = i;
            cmap[c * 4 + 2 * slot + 1] = l;
            cmu[c * 2 + slot] = h.mu[i][l];
            sw_kernel_row(h.ferbs, h.pc[c], K + (size_t)l * SW_NEP);
        }
        sw_spline(h.ferbs, sw_ws(i), (double*)(blob + L.off[T_W][i]), sw_kpad(i));
        sw_pack((const double*)(blob + L.off[T_W][i]), SW_NEP, sw_kpad(i), (double*)(blob + L.off[T_WP][i]));
        sw_pack(K, pad16(L.nc[i]), SW_NEP, (double*)(blob + L.off[T_KP][i]));
        // np.hanning(ws + 2)[1:-1]: 0.5 + 0.5 cos(pi n / (M - 1)), n = 1 - M, 3 - M, ...
        double* win = (double*)(blob + L.off[T_WIN][i]);
        const int M = sw_ws(i) + 2;
        double sum = 0.0;
        for (int m = 0; m < sw_ws(i); ++m) {
            const double nn = (double)(1 - M + 2 * (m + 1));
            win[m] = 0.5 + 0.5 * cos(M_PI * nn / (double)(M - 1));
            sum += win[m];
        }
        win[sw_ws(i)] = sum;
    }
    // pick: for a peak at candidate i, the parabola's abscissae x0, x2 (x1 = 0) and the 17 grid points
    // 1/768 octave apart from pc[i-1] (SWIPE.py:62-78), as abscissae and as the f32 f0 each stands for
    double* px = (double*)(blob + L.off[T_PX][0]);
    double* gx = (double*)(blob + L.off[T_GRIDX][0]);
    float* gf = (float*)(blob + L.off[T_GRIDF0][0]);
    for (int i = 1; i + 1 < SW_NC; ++i) {
        const double tc0 = 1.0 / h.pc[i - 1], tc1 = 1.0 / h.pc[i], tc2 = 1.0 / h.pc[i + 1];
        px[2 * i] = (tc0 / tc1 - 1.0) * 2.0 * M_PI;
        px[2 * i + 1] = (tc2 / tc1 - 1.0) * 2.0 * M_PI;
        const double start = log2(h.pc[i - 1]);
        const double step = 1.0 / 12.0 / 64.0;
        const double dl = (start + step) - start;  // np.arange's fill
        for (int g = 0; g < SW_NG; ++g) {
            const double lg = start + (double)g * dl;
            gx[i * SW_NG + g] = ((1.0 / pow(2.0, lg)) / tc1 - 1.0) * 2.0 * M_PI;
            gf[i * SW_NG + g] = (float)pow(2.0, start + (double)g / 12.0 / 64.0);
        }
    }
}

const SwHost& sw_host_once() {
    static const SwHost h = [] {
        SwHost v;
        sw_host(v);
        return v;
    }();
    return h;
}

// ---------------------------------------------------------------- device side
struct SwTabs {
    const double* W[SW_NW];
    const double* K[SW_NW];
    const double* win[SW_NW];
    int nc[SW_NW];
    const double* tw;
    const int* cmap;
    const double* cmu;
    const double* px;
    const double* gx;
    const float* gf;
    const double* pc;
};

struct SwWork {
    double* A[SW_NW];   // [frame tile][kpad / 16][64][4]: |X| in MFMA operand order (sw_pack), whole 16-frame tiles
    double* L[SW_NW];   // [frame tile][SW_NEP / 16][64][4]: the normalised loudness, likewise
    double* Si[SW_NW];  // [pad16(nc)][nfr]
    int nfr[SW_NW];
    int fft_blk0[SW_NW + 1];   // first block of each window size in sw_fft
    int gemm_blk0[SW_NW + 1];  // ... in the GEMMs
};

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

__device__ __forceinline__ int sw_window_of(const int* blk0, int b) {
    int i = 0;
#pragma unroll
    for (int k = 1; k < SW_NW; ++k) i += b >= blk0[k];
    return i;
}

// frame k of window size i covers the samples [k hop - ws/2, k hop + ws/2) (zero outside [0, n)).  A block
// transforms 2048 / ws frames of its window size side by side in LDS, so every block is 2048 points whatever
// the size.  Radix-2 DIT as denoise.hip's fft_lds, with the twiddles exp(-2 pi i k / 2048) from the table.
__global__ __launch_bounds__(256) void sw_fft_kernel(const float* x, int64_t n, SwTabs t, SwWork w) {
    __shared__ double2 a[2048];
    const int i = sw_window_of(w.fft_blk0, blockIdx.x);
    const int fb = (blockIdx.x - w.fft_blk0[i]) << i;  // the block's first frame
    const int ws = 2048 >> i, logn = 11 - i, nbin = ws / 2 + 1, kpad = (ws / 2 + 16) / 16 * 16;
    const double* win = t.win[i];
    for (int p = threadIdx.x; p < 2048; p += 256) {
        const int seg = p >> logn, m = p & (ws - 1);
        const int64_t g = (int64_t)(fb + seg) * (ws / 2) - ws / 2 + m;
        const double v = (g >= 0 && g < n) ? (double)x[g] : 0.0;  // (the frames past nfr are all zeros)
        a[(seg << logn) + (int)(__brev((unsigned)m) >> (32 - logn))] = make_double2(v * win[m], 0.0);
    }
    __syncthreads();
    const double2* tw = (const double2*)t.tw;
    for (int s = 1; s <= logn; ++s) {
        const int half = 1 << (s - 1);
        for (int p = threadIdx.x; p < 1024; p += 256) {
            const int seg = p >> (logn - 1), j = p & (ws / 2 - 1);
            const int pos = j & (half - 1);
            const int i0 = (seg << logn) + ((j >> (s - 1)) << s) + pos;
            const int i1 = i0 + half;
            const double2 tv = cmul(tw[pos * (1024 >> (s - 1))], a[i1]);
            const double2 u = a[i0];
            a[i0] = make_double2(u.x + tv.x, u.y + tv.y);
            a[i1] = make_double2(u.x - tv.x, u.y - tv.y);
        }
        __syncthreads();
    }
    // operand order (sw_pack): u fastest, so a thread quad writes 32 contiguous bytes
    const double wsum = win[ws];
    for (int p = threadIdx.x; p < (kpad << i); p += 256) {
        const int seg = p / kpad, q = p - seg * kpad;
        const int u = q & 3, lq = (q >> 2) & 3, k16 = q >> 4;
        const int k = 4 * (4 * k16 + u) + lq;
        const int fr = fb + seg;
        const double2 v = a[(seg << logn) + (k < nbin ? k : 0)];
        // the pad columns meet zero weights in the GEMM
        w.A[i][((((int64_t)(fr >> 4) * (kpad / 16) + k16) * 64) + lq * 16 + (fr & 15)) * 4 + u] =
            k < nbin ? hypot(v.x / wsum, v.y / wsum) : 0.0;
    }
}

RVC_DEV doublex4 mfma64(double a, double b, doublex4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// Out[m][f] = sum_k P[m][k] Q[f][k].  MODE 0: P = W_i, Q = A_i, the loudness epilogue -> L_i (operand order);
// MODE 1: P = K_i, Q = L_i -> S_i [m][nfr].  8 waves; wave w owns the row tiles w, w + 8, ... of the block's one
// 16-frame column tile.  v_mfma_f64_16x16x4_f64: lane l holds P[l & 15][l >> 4], Q[l >> 4][l & 15]; D: col
// l & 15, row (l >> 4) + 4 r.
// The shape follows from the f64 MFMA's 64 cycles and the five window sizes' very different depths (K = 1040 ..
// 80 for the same flop count each): a wave that owned 6 row tiles x 2 column tiles spent 65 x 48 MFMAs = 83 us
// on a 2048-window block, of which there are only 15 -- the launch then took 305 us against a 21 us matrix-core
// floor (kernel trace, 30 s clip).  With 3 x 1 tiles per wave the longest wave is 21 us of MFMAs and there
// are ~7 waves per SIMD to cover each other's loads.
template <int MODE>
__global__ __launch_bounds__(SW_GT) void sw_gemm_kernel(SwTabs t, SwWork w) {
    __shared__ double red[SW_GT / 64][SW_TF];
    const int i = sw_window_of(w.gemm_blk0, blockIdx.x);
    const int f0 = (blockIdx.x - w.gemm_blk0[i]) * SW_TF;
    const int nfr = w.nfr[i];
    const int K = MODE == 0 ? (((1024 >> i) + 16) / 16 * 16) : SW_NEP;
    const int mtiles = MODE == 0 ? SW_NEP / 16 : (t.nc[i] + 15) / 16;
    const double* P = MODE == 0 ? t.W[i] : t.K[i];
    const double* Q = MODE == 0 ? w.A[i] : w.L[i];
    constexpr int NWV = SW_GT / 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
    const int K16 = K / 16;
    const int f = f0 + lr;
    // operand order (sw_pack): [tile][K / 16][lane] of 32 bytes -- a wave load is 2 KB in a row
    const doublex4* qp = (const doublex4*)Q + (int64_t)(f0 >> 4) * K16 * 64 + lane;
    const doublex4* pp = (const doublex4*)P + (int64_t)wave * K16 * 64 + lane;
    doublex4 acc[SW_MTW];
#pragma unroll
    for (int j = 0; j < SW_MTW; ++j) acc[j] = doublex4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
    for (int s = 0; s < K16; ++s) {
        const doublex4 b = qp[s * 64];
#pragma unroll
        for (int j = 0; j < SW_MTW; ++j) {
            if (wave + NWV * j < mtiles) {  // wave-uniform
                const doublex4 a = pp[((int64_t)NWV * j * K16 + s) * 64];
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[j] = mfma64(a[u], b[u], acc[j]);
            }
        }
    }
    if (MODE == 0) {
        double ss = 0.0;
#pragma unroll
        for (int j = 0; j < SW_MTW; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double v = wave + NWV * j < mtiles ? sqrt(fmax(0.0, acc[j][r])) : 0.0;
                acc[j][r] = v;
                ss += v * v;
            }
        ss += __shfl_xor(ss, 16, 64);
        ss += __shfl_xor(ss, 32, 64);
        if (lq == 0) red[wave][lr] = ss;
        __syncthreads();
        double tot = 0.0;
#pragma unroll
        for (int q = 0; q < NWV; ++q) tot += red[q][lr];
        double den = sqrt(tot);
        if (den == 0.0) den = 2.220446049250313e-16;
        // L_i in operand order for the next GEMM: row 16 mt + 4 r + lq is k step 4 mt + r, k lane group lq, so a
        // lane's four values are one 32-byte piece at [frame tile][mt][lane] (the frames past nfr: den = eps, 0)
        doublex4* out = (doublex4*)w.L[i] + (int64_t)(f0 >> 4) * (SW_NEP / 16) * 64 + lane;
#pragma unroll
        for (int j = 0; j < SW_MTW; ++j)
            if (wave + NWV * j < mtiles)
                out[(wave + NWV * j) * 64] = doublex4{acc[j][0] / den, acc[j][1] / den, acc[j][2] / den, acc[j][3] / den};
    } else if (f < nfr) {
#pragma unroll
        for (int j = 0; j < SW_MTW; ++j)
            if (wave + NWV * j < mtiles)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    w.Si[i][(int64_t)(16 * (wave + NWV * j) + lq + 4 * r) * nfr + f] = acc[j][r];
    }
}

// S[c][k] = sum over the (at most two) window sizes serving c, in window order, of mu * (S_i row linearly
// interpolated to t = k * 0.01 as scipy's interp1d does: x_new_indices = searchsorted(ti, t) clipped to
// [1, nfr - 1], slope * (t - x_lo) + y_lo), with ti[f] = f hop / fs
__global__ __launch_bounds__(256) void sw_sum_kernel(SwTabs t, SwWork w, int64_t F, double* S) {
#pragma clang fp contract(off)
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    if (k >= F) return;
    const double tq = (double)k * (10.0 / 1000.0);
    double s = 0.0;
#pragma unroll
    for (int slot = 0; slot < 2; ++slot) {
        const int i = t.cmap[c * 4 + 2 * slot];
        if (i < 0) continue;
        const int l = t.cmap[c * 4 + 2 * slot + 1];
        const int nfr = w.nfr[i];
        const double hop = (double)(1024 >> i);
        int g = (int)ceil(tq * (double)SW_FS / hop);
        while (g > 0 && (double)(g - 1) * hop / (double)SW_FS >= tq) --g;
        while (g < nfr && (double)g * hop / (double)SW_FS < tq) ++g;
        g = min(max(g, 1), nfr - 1);
        const double xlo = (double)(g - 1) * hop / (double)SW_FS, xhi = (double)g * hop / (double)SW_FS;
        const double* row = w.Si[i] + (int64_t)l * nfr;
        const double ylo = row[g - 1], yhi = row[g];
        const double slope = (yhi - ylo) / (xhi - xlo);
        const double y = slope * (tq - xlo) + ylo;
        s = s + t.cmu[c * 2 + slot] * y;
    }
    S[(int64_t)c * F + k] = s;
}

// 16 frames x 16 candidate ranges per block; strict > keeps the first index on ties, in a range and across them
__global__ __launch_bounds__(256) void sw_pick_kernel(const double* S, int64_t F, SwTabs t, float* f0) {
#pragma clang fp contract(off)
    __shared__ double bv[16][16];
    __shared__ int bi[16][16];
    const int fx = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int64_t k = (int64_t)blockIdx.x * 16 + fx;
    constexpr int R = (SW_NC + 15) / 16;
    const int c0 = sl * R, c1 = min(SW_NC, c0 + R);
    double best = 0.0;
    int arg = c0;
    if (k < F) {
        best = S[(int64_t)c0 * F + k];
        for (int c = c0 + 1; c < c1; ++c) {
            const double v = S[(int64_t)c * F + k];
            if (v > best) {
                best = v;
                arg = c;
            }
        }
    }
    bv[sl][fx] = best;
    bi[sl][fx] = arg;
    __syncthreads();
    if (sl != 0 || k >= F) return;
    for (int q = 1; q < 16; ++q)
        if (bv[q][fx] > best) {
            best = bv[q][fx];
            arg = bi[q][fx];
        }
    float out;
    if (best < SW_THR) out = 0.f;
    else if (arg == 0 || arg == SW_NC - 1) out = (float)t.pc[0];
    else {
        // the parabola through (x0, y0), (0, y1), (x2, y2), then np.polyval's Horner form on the grid
        const double x0 = t.px[2 * arg], x2 = t.px[2 * arg + 1];
        const double y0 = S[(int64_t)(arg - 1) * F + k], y1 = best, y2 = S[(int64_t)(arg + 1) * F + k];
        const double d0 = (y0 - y1) / x0, d2 = (y2 - y1) / x2;
        const double ca = (d0 - d2) / (x0 - x2);
        const double cb = d0 - ca * x0;
        double pm = 0.0;
        int pg = 0;
        for (int g = 0; g < SW_NG; ++g) {
            const double xv = t.gx[arg * SW_NG + g];
            const double pv = (ca * xv + cb) * xv + y1;
            if (g == 0 || pv > pm) {
                pm = pv;
                pg = g;
            }
        }
        out = t.gf[arg * SW_NG + pg];
    }
    f0[k] = out;
}

// get_f0 (convert.py:308-323) on the f32 swipe f0: NumPy keeps the f0 array's f32 through the autotune, the
// shift and the mel expression, and the f64 mel_min / mel_max scalars promote the quantiser's affine step
__global__ __launch_bounds__(256) void sw_post_kernel(const float* f0, int64_t F, float shift, double mel_min,
                                                      double mel_max, rvc_f0_post post, int64_t* coarse,
                                                      float* pitchf) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= F) return;
    const float f = f0_post_apply<float>(f0[k], k, shift, post);
    coarse[k] = f0_coarse(f, mel_min, mel_max);
    pitchf[k] = f;
}

SwTabs sw_tabs(const void* tables) {
    const SwHost& h = sw_host_once();
    const SwLayout L = sw_layout(h);
    const char* b = (const char*)tables;
    SwTabs t;
    for (int i = 0; i < SW_NW; ++i) {
        t.W[i] = (const double*)(b + L.off[T_WP][i]);  // the kernels read the operand-order copies
        t.K[i] = (const double*)(b + L.off[T_KP][i]);
        t.win[i] = (const double*)(b + L.off[T_WIN][i]);
        t.nc[i] = L.nc[i];
    }
    t.tw = (const double*)(b + L.off[T_TW][0]);
    t.cmap = (const int*)(b + L.off[T_CMAP][0]);
    t.cmu = (const double*)(b + L.off[T_CMU][0]);
    t.px = (const double*)(b + L.off[T_PX][0]);
    t.gx = (const double*)(b + L.off[T_GRIDX][0]);
    t.gf = (const float*)(b + L.off[T_GRIDF0][0]);
    t.pc = (const double*)(b + L.off[T_PC][0]);
    return t;
}

int64_t sw_work_bytes(int64_t n, const int* nc) {
    size_t o = 0;
    for (int i = 0; i < SW_NW; ++i) {
        const size_t nfr = (size_t)sw_nfr(i, n), nfp = (nfr + 15) / 16 * 16;  // A_i, L_i: whole 16-frame tiles
        o += align256(sizeof(double) * nfp * sw_kpad(i)) + align256(sizeof(double) * nfp * SW_NEP) +
             align256(sizeof(double) * nfr * pad16(nc[i]));
    }
    return (int64_t)o;
}

}  // namespace

extern "C" int64_t rvc_swipe_frames(int64_t n) { return n > 0 ? n / SW_HOPOUT + 1 : -1; }

extern "C" int64_t rvc_swipe_work_bytes(int64_t n) {
    if (n <= 0 || n >= (1ll << 30)) return -1;
    return sw_work_bytes(n, sw_layout(sw_host_once()).nc);
}

extern "C" int64_t rvc_swipe_tables_bytes(void) { return sw_layout(sw_host_once()).bytes; }

extern "C" int64_t rvc_swipe_table_dims(int which, int window, int64_t* dims) {
    if (!dims || which < 0 || which >= T_COUNT || window < 0 || window >= SW_NW) {
        rvc_set_error("swipe_table_dims: bad args");
        return RVC_EINVAL;
    }
    const SwLayout L = sw_layout(sw_host_once());
    const bool per_window = which == T_IDX || which == T_MU || which == T_W || which == T_K || which == T_WIN ||
                            which == T_WP || which == T_KP;
    int64_t rows = 1, cols = 0, ld = 0;
    switch (which) {
        case T_PC: cols = SW_NC; break;
        case T_FERBS: cols = SW_NE; break;
        case T_IDX: case T_MU: cols = L.nc[window]; break;
        case T_W: rows = SW_NE; cols = sw_nbin(window); ld = sw_kpad(window); break;
        case T_K: rows = L.nc[window]; cols = SW_NE; ld = SW_NEP; break;
        case T_WIN: cols = sw_ws(window) + 1; break;
        case T_TW: rows = 1024; cols = 2; break;
        case T_CMAP: rows = SW_NC; cols = 4; break;
        case T_CMU: case T_PX: rows = SW_NC; cols = 2; break;
        case T_WP: rows = SW_NEP / 16; cols = sw_kpad(window) * 16; break;
        case T_KP: rows = pad16(L.nc[window]) / 16; cols = SW_NEP * 16; break;
        default: rows = SW_NC; cols = SW_NG; break;
    }
    dims[0] = rows;
    dims[1] = cols;
    dims[2] = ld ? ld : cols;
    return L.off[which][per_window ? window : 0];
}

extern "C" int rvc_swipe_tables(void* blob, int64_t bytes) {
    RVC_CHECK_ARG(blob, "swipe_tables: null pointer");
    const SwHost& h = sw_host_once();
    const SwLayout L = sw_layout(h);
    RVC_CHECK_ARG(bytes >= L.bytes, "swipe_tables: %lld bytes given, %lld needed", (long long)bytes,
                  (long long)L.bytes);
    sw_fill(h, L, (char*)blob);
    return RVC_OK;
}

extern "C" int rvc_swipe_strength(const float* x, int64_t n, const void* tables, void* work, int64_t work_bytes,
                                  double* S, rvc_stream_t stream) {
    RVC_CHECK_ARG(x && tables && work && S, "swipe_strength: null pointer");
    RVC_CHECK_ARG(n > 0 && n < (1ll << 30), "swipe_strength: bad length %lld", (long long)n);
    const SwTabs t = sw_tabs(tables);
    RVC_CHECK_ARG(work_bytes >= sw_work_bytes(n, t.nc), "swipe_strength: work buffer too small");
    SwWork w;
    char* p = (char*)work;
    w.fft_blk0[0] = w.gemm_blk0[0] = 0;
    for (int i = 0; i < SW_NW; ++i) {
        const size_t nfr = (size_t)sw_nfr(i, n), nfp = (nfr + 15) / 16 * 16;
        w.nfr[i] = (int)nfr;
        w.A[i] = (double*)p; p += align256(sizeof(double) * nfp * sw_kpad(i));
        w.L[i] = (double*)p; p += align256(sizeof(double) * nfp * SW_NEP);
        w.Si[i] = (double*)p; p += align256(sizeof(double) * nfr * pad16(t.nc[i]));
        w.fft_blk0[i + 1] = w.fft_blk0[i] + (int)(nfp >> i);  // whole tiles: the frames past nfr come out 0
        w.gemm_blk0[i + 1] = w.gemm_blk0[i] + (int)cdiv((int64_t)nfr, SW_TF);
    }
    const int64_t F = rvc_swipe_frames(n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sw_fft_kernel, dim3((unsigned)w.fft_blk0[SW_NW]), dim3(256), 0, s, x, n, t, w);
    hipLaunchKernelGGL(sw_gemm_kernel<0>, dim3((unsigned)w.gemm_blk0[SW_NW]), dim3(SW_GT), 0, s, t, w);
    hipLaunchKernelGGL(sw_gemm_kernel<1>, dim3((unsigned)w.gemm_blk0[SW_NW]), dim3(SW_GT), 0, s, t, w);
    hipLaunchKernelGGL(sw_sum_kernel, dim3(cdiv(F, 256), SW_NC), dim3(256), 0, s, t, w, F, S);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_swipe_pick(const double* S, int64_t F, const void* tables, float* f0, rvc_stream_t stream) {
    RVC_CHECK_ARG(S && tables && f0, "swipe_pick: null pointer");
    RVC_CHECK_ARG(F > 0 && F < (1ll << 24), "swipe_pick: bad frame count %lld", (long long)F);
    hipLaunchKernelGGL(sw_pick_kernel, dim3(cdiv(F, 16)), dim3(256), 0, (hipStream_t)stream, S, F, sw_tabs(tables),
                       f0);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

extern "C" int rvc_swipe_post(const float* f0, int64_t F, float shift, const rvc_f0_post* post, int64_t* coarse,
                              float* pitchf, rvc_stream_t stream) {
    RVC_CHECK_ARG(f0 && coarse && pitchf && F > 0, "swipe_post: bad args");
    RVC_CHECK_ARG(!post || !post->rep || (post->rep_off >= 0 && post->rep_len >= 0), "swipe_post: bad f0 post");
    const F0MelRange mel = f0_mel_range();
    hipLaunchKernelGGL(sw_post_kernel, dim3(cdiv(F, 256)), dim3(256), 0, (hipStream_t)stream, f0, F, shift, mel.min,
                       mel.max, f0_post_or_none(post), coarse, pitchf);
    RVC_HIP(hipGetLastError());
    return RVC_OK;
}

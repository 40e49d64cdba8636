// Radix-2 f64 FFT of one frame in LDS, shared by the f64 STFT chains (denoise.hip, formant.hip).
#pragma once
#include "rvc_common.h"

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// In-place iterative radix-2 DIT FFT (forward, e^{-2 pi i k n / N}) of N points in LDS `a`, input
// already in bit-reversed order.  Twiddles by sincospi in f64.
__device__ inline void fft_lds(double2* a, int N, int logn) {
    for (int s = 1; s <= logn; ++s) {
        const int half = 1 << (s - 1);
        for (int j = threadIdx.x; j < N / 2; j += blockDim.x) {
            const int pos = j & (half - 1);
            const int i0 = ((j >> (s - 1)) << s) + pos;
            const int i1 = i0 + half;
            double sn, cs;
            sincospi(-(double)pos / (double)half, &sn, &cs);
            const double2 t = cmul(make_double2(cs, sn), a[i1]);
            const double2 u = a[i0];
            a[i0] = make_double2(u.x + t.x, u.y + t.y);
            a[i1] = make_double2(u.x - t.x, u.y - t.y);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int bitrev(int i, int logn) { return (int)(__brev((unsigned)i) >> (32 - logn)); }

// The fixed two-stage f64 sum of the training losses (trainfwd.hip, discriminator.hip).
// Stage 1: RED_BLOCKS blocks of 256 threads, block i over the i-th contiguous chunk of the n terms; a thread adds its
// terms in index order, the wave by the xor tree, the four waves in one written order -> part[i].  Stage 2 (the
// caller's kernel): one wave adds the RED_BLOCKS partials by the same tree.  No atomics, so two runs give the same bits.
#pragma once
#include "rvc_common.h"

namespace {

constexpr int RED_BLOCKS = RVC_TRAINFWD_RED_BLOCKS;  // stage-1 blocks of every reduction

RVC_DEV double wave_sum64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <typename Term>
RVC_DEV void reduce_stage1(int64_t n, double* __restrict__ part, Term term) {
    __shared__ double ws[4];
    const int64_t len = (n + RED_BLOCKS - 1) / RED_BLOCKS;
    const int64_t i0 = blockIdx.x * len, i1 = i0 + len < n ? i0 + len : n;
    double s = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) s += term(i);
    s = wave_sum64(s);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

}  // namespace

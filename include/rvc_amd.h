/*
 * rvc_amd.h -- C ABI of librvc_amd.so, the MI355X (gfx950) kernels behind the
 * RVC-MAKER voice-conversion hot path (main/inference/convert.py:VC.pipeline).
 *
 * The reference is pure Python/PyTorch: it has no FFI of its own on this path
 * (SURVEY §0).  Every entry point below replaces the torch op(s) the reference
 * executes at the cited file:line; the Python host package (rvc-maker_amd/rvc_amd)
 * binds them with ctypes the way the reference's only native binding
 * (main/library/predictors/WORLD_WRAPPER.py:30-90: ctypes.CDLL, option structs,
 * caller-allocated outputs) does.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - All tensors are caller-owned DEVICE buffers (fp32 unless stated), dense,
 *     channels-first [B][C][L] like torch's NCL.  The library allocates nothing.
 *   - Every call is stream-ordered on the given hipStream_t and never
 *     synchronises; it returns RVC_OK or a negative code, with the message in
 *     rvc_last_error() (thread-local).
 *   - Weights are pre-packed by the host loader (weight-norm / BatchNorm folded,
 *     transposed to K-major "KM" = [groups][Cin/groups * K][Cout/groups]).
 */
#ifndef RVC_AMD_H
#define RVC_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* rvc_stream_t; /* == hipStream_t */

enum { RVC_OK = 0, RVC_EINVAL = -22, RVC_EHIP = -5 };

enum {
    RVC_ACT_NONE = 0,
    RVC_ACT_LRELU = 1,
    RVC_ACT_RELU = 2,
    RVC_ACT_TANH = 3,
    RVC_ACT_GELU = 4, /* exact erf GELU (torch.nn.GELU / F.gelu) */
    RVC_ACT_SIGMOID = 5,
    RVC_ACT_LOGCLAMP = 6, /* log(max(v, slope))  (RMVPE.py:181) */
};

const char* rvc_last_error(void);
int rvc_version(void);

/* ------------------------------------------------------------------ conv1d
 * Implicit-GEMM 1-D convolution on f32 MFMA (v_mfma_f32_16x16x4_f32).
 * Replaces every torch.nn.Conv1d / F.conv1d on the path:
 *   NSF-HiFiGAN conv_pre / noise_convs / ResBlock convs / conv_post
 *     (synthesizers.py:123,136,161; residuals.py:16-17,32-36),
 *   flow WaveNet + 1x1 convs (modules.py:27-44, residuals.py:120-129),
 *   TextEncoder FFN / q,k,v,o / proj (synthesizers.py:198-202,298-305,364),
 *   ContentVec conv feature extractor and pos_conv and every nn.Linear
 *     (fairseq.py:1165-1195, 585-592, 204-225, 778-814) as a K=1 conv,
 *   and, one phase per grid.z, ConvTranspose1d (synthesizers.py:133) through
 *   the polyphase weight packing done by the host.
 *
 *   v = out_scale * act(sum_{c,k} W[m][c][k] * pre(x[b][c][col*stride - pad + k*dil]) + bias[m] + bias2[m])
 *   v += res[b][m][t]                       (if res)
 *   y[b][m][t] = v  or  y[b][m][t] += v     (accumulate),   t = col*ostride + ooffset + phase
 *   pre(v) = in_act(v * in_scale)
 */
#define RVC_ARITH_F16X3 16 /* rvc_conv1d_args.wx_passes / rvc_resblock_args.passes: split-fp16, 3 passes */
#define RVC_AMAX_SHARDS 64 /* u32 words per |max| cell (rvc_conv1d_args.amax_in / amax_out) */
#define RVC_ARITH_FP32_SA 7 /* rvc_conv1d_args.wx_passes: 6-pass split-bf16 with the correction passes in their
                               own f32 accumulators (fewer roundings of the large sum; RMVPE) */

typedef struct rvc_conv1d_args {
    const float* x;    /* [B][Ci][Lin] with batch stride x_bstride           */
    const float* w;    /* KM packed: [nphase][groups][Ci/g*K][Co/g]            */
    const float* bias; /* [Co] or NULL                                          */
    const float* bias2;/* [Co] or NULL: second per-channel term added after bias
                          (speaker conditioning: synthesizers.py:147, modules.py:39-43) */
    const float* res;  /* [B][Co][Lout] residual added after the activation, or NULL */
    float* y;          /* [B][Co][Lout]                                         */
    int64_t B, Ci, Co, Lin, Lout;
    int64_t ncols;     /* GEMM columns per phase (== Lout for a plain conv)     */
    int64_t x_bstride, y_bstride, res_bstride, w_bstride; /* 0 = dense default; w: 0 = shared */
    int K, stride, dil, pad, groups;
    int nphase, ostride, ooffset;
    int in_act, out_act, accumulate, _pad0;
    float in_scale, in_slope, out_slope, out_scale;
    /* 2-D mode (RMVPE 3x3 convs on zero-bordered [C][H+2][W+2] images flattened to L):
       ntoff > 0 replaces tap*dil by toff[tap]; wrap > 0 skips stores to border cells
       (t % wrap in {0, wrap-1}, or t / wrap in {0, Lout/wrap - 1}). */
    int ntoff, wrap;
    int toff[16];
    /* Split-bf16 engine: wx = the same weights pre-split into bf16 h/m/l planes by
       rvc_conv1d_pack_x6 (NULL = f32 MFMA engine).  Used for stride-1 (and stride-2) 1-D convs --
       ungrouped (<= 64 taps), or grouped (<= 128 taps, nphase 1, stride 1, no src_*) with the image packed
       with the groups as phases: pack_x6(w, groups, Ci/g, K, Co/g); other shapes ignore it.
       wx_nmf = its padded 16-row fragment count.
       wx_passes: bf16 MFMA passes per product -- 0 or 6 = f32-accurate (hH+hM+mH+hL+mM+lH, products to
       2^-24), RVC_ARITH_FP32_SA = the same 6 passes with hH and the 5 corrections accumulated apart (RMVPE,
       whose f0 is a per-frame decision), 3 = hH+hM+mH (16-bit operand mantissas), 1 = hH (bf16 operands);
       f32 accumulation always.
       RVC_ARITH_F16X3: wx is an rvc_conv1d_pack_f16 image instead -- split-fp16 operands (per-row
       weight and per-tile activation power-of-2 scales, 11 + 11 significant bits each), hH + hL + lH
       on the fp16 MFMA: ~2^-20 relative per product, f32 accumulation. */
    const void* wx;
    int wx_nmf, wx_passes;
    /* Tensor |max| side channel (round 5): amax_out (or NULL) is a cell of RVC_AMAX_SHARDS u32 words that receives
       max |y| over every value the launch stores (atomic maxes of the f32 bits, spread over the words; the caller
       zeroes the cell before the producing launch), and amax_in (or NULL) is such a cell for x: a split-fp16
       launch (RVC_ARITH_F16X3) then takes its activation scale from the largest word (times |in_scale|: an upper
       bound of |pre(x)|) instead of a per-tile |max| pre-pass over its input.
       A batched launch (B > 1) takes B consecutive cells, one per batch element: element b's at
       amax + b * RVC_AMAX_SHARDS (round 6), so a clip's scale never depends on the other clips of its batch. */
    const unsigned* amax_in;
    unsigned* amax_out;
    /* Fused source conv (round 6; NULL src_x = none): every stored output y[b][m][t] also adds
       sum_k src_w[k][m] * src_x[b][t * src_stride - src_pad + k] + src_b[m] (zero outside [0, src_len)), after the
       residual and accumulate operands -- a 1-input-channel conv of src_K taps over a [B][src_len] signal (batch
       stride src_bstride, 0 = src_len; src_w KM-packed [src_K][Co] as a Ci = 1 conv weight, src_b [Co] or NULL).
       The NSF generator's x = ups(x) + noise_convs(har) (synthesizers.py:156) in the upsampling conv's call: a
       read-modify-write pass right after the conv (a direct kernel, HBM-bound, instead of the 1-channel conv as an
       implicit GEMM K deep); amax_out then receives the final values' |max|.  The k-sum is an fmaf chain in tap
       order from 0, then + src_b, so it equals the separate 1-channel conv on the f32 engine with accumulate. */
    const float* src_x;
    const float* src_w;
    const float* src_b;
    int src_K, src_stride, src_pad, _pad1;
    int64_t src_len, src_bstride;
} rvc_conv1d_args;

/* Split-K (chosen by the library when the tile grid would underfill the 256 CUs) needs a caller-owned
 * device workspace of rvc_conv1d_workspace_bytes(a) bytes (0 when not split; -1 on bad args).  Launches
 * that may run concurrently need separate workspaces. */
int64_t rvc_conv1d_workspace_bytes(const rvc_conv1d_args* a);
/* Which engine a call would run on: 0 = f32 MFMA, 1 = split-bf16 (x6); -1 on bad args. */
int rvc_conv1d_engine(const rvc_conv1d_args* a);
/* The output tile a call's blocks would compute: (rows << 16) | columns, e.g. 128 x 256 = 0x800100; -1 on bad args.
 * The choice depends on the shape, the pass set and the device's CU count (how the tile grid fills its rounds). */
int rvc_conv1d_tile(const rvc_conv1d_args* a);
int rvc_conv1d(const rvc_conv1d_args* a, void* ws, int64_t ws_bytes, rvc_stream_t stream);
/* Profiling hook (this host thread): while set to a hipEvent_t, each rvc_conv1d call records it on its stream
 * right after the conv kernel, before any split-K reduce, so that a caller's events can bracket the conv
 * kernel alone (bench.py's roofline probe).  NULL (the default) turns it off. */
void rvc_conv1d_set_probe_event(void* hip_event);
/* Diagnostic build only (-DRVC_CONV_STAMPS=1, scripts/conv_stamps.py): the split-operand conv engine's per-block
 * phase stamps (s_memtime) go to buf ([bytes / 2048][256] u64); returns -1 in a production build. */
int rvc_conv1d_set_stamps(void* buf, int64_t bytes);
/* The same for the fused ResBlock pair (rvc_resblock_pair): per workgroup, per tile phase stamps (scripts/rb_stamps.py);
 * -1 in a production build. */
int rvc_resblock_set_stamps(void* buf, int64_t bytes);
/* The fused pair's output path for this thread's launches (round 6): 1 = split-fp16 pairs at C <= 64 write c2's results
 * into LDS (over the tile's residual rows) and the loader waves store them during the next tile (the compute waves go
 * straight on); 2 = the same, and at C = 32 (two R buffers by tile parity) after the next tile's c1 barriers instead of
 * before them; 0 = the compute waves' own global stores; -1 = RVC_RB_YLDS (default 2).  Same bits in every form. */
int rvc_resblock_set_ylds(int on);
/* The fused pair's C = 64 tiling for this thread's launches (round 6): 1 = 2 row fragments per compute wave, 240
 * outputs per tile (the <= 2-plane pass sets; 6-pass pairs keep the narrow form), 0 = 1 row fragment, 112 outputs,
 * -1 = RVC_RB_WIDE64 (default 1).  The same sums in the same order; split-fp16's power-of-2 tile scales follow the
 * tile, so results agree to that arithmetic's precision rather than bit for bit.  Returns the previous setting. */
int rvc_resblock_set_wide64(int on);
/* The split-operand engine's epilogue form for this thread's launches: 1 = the tile epilogue through LDS (on the
 * 128-wide tiles where it needs no extra LDS), 0 = the in-register epilogue, -1 = RVC_X6_TILE_EPI (default 0).  Both give the same bits (tests/test_gpu_ops.py);
 * an A/B switch for measurements in one process. */
int rvc_conv1d_set_tile_epi(int on);
/* The split-operand engine's in-register epilogue in 128-byte rows (round 6: a v_permlane16_swap per accumulator pair
 * regroups two 16-column fragments into 2 rows x 32 columns per register, so every residual / accumulate load and
 * store moves 2 x 128-B segments instead of 4 x 64 B): 1 on, 0 off, -1 RVC_X6_SWZ (default 1).  Same bits. */
int rvc_conv1d_set_swz(int on);
/* Per-thread override of the split-fp16 loaders' fast form (used with amax_in on the 8-compute-wave tiles; same
 * bits as the general form): 1 on, 0 off, -1 back to RVC_X6_F16FAST (default on).  Diagnostic / test knob. */
int rvc_conv1d_set_f16_fast(int on);
/* Split-K policy (this host thread): the library splits a conv's k range over blocks while its tile grid is
 * below `target` tiles (default 256 = 1 per CU, halved for tiles of which one block fills a CU; or
 * RVC_SPLITK_TILES); 0 = never split, -1 = back to the default.  Returns the previous setting.  Results depend on it at f32 rounding level (the split changes the
 * summation order). */
int rvc_conv1d_set_splitk_target(int target);
/* A stream restricted to the CUs set in mask (nwords 32-bit words, bit i = CU i), and its release. */
int rvc_stream_create_cu_mask(const uint32_t* mask, int nwords, rvc_stream_t* out);
int rvc_stream_destroy(rvc_stream_t stream);
/* Pack KM weights [nphase][Ci*K][Co] (one group) for the split-bf16 engine: out must hold
 * rvc_conv1d_x6_bytes(nphase, Ci, K, Co) bytes; *nmf_out receives wx_nmf. */
int64_t rvc_conv1d_x6_bytes(int64_t nphase, int64_t Ci, int K, int64_t Co);
int rvc_conv1d_pack_x6(const float* w_km, int64_t nphase, int64_t Ci, int K, int64_t Co, void* out, int* nmf_out,
                       rvc_stream_t stream);
/* The split-fp16 image (wx with wx_passes = RVC_ARITH_F16X3): the x6 fragment layout holding the fp16 h / l
 * planes of each output row's weights scaled by a power of 2 (max |w| below 2^14), followed by the rows'
 * reciprocal scales (f32 [wx_nmf * 16]); rvc_conv1d_f16_bytes(...) bytes, *nmf_out as for pack_x6. */
int64_t rvc_conv1d_f16_bytes(int64_t nphase, int64_t Ci, int K, int64_t Co);
int rvc_conv1d_pack_f16(const float* w_km, int64_t nphase, int64_t Ci, int K, int64_t Co, void* out, int* nmf_out,
                        rvc_stream_t stream);

/* ------------------------------------------------------------------ fused ResBlock pair
 * One (convs1[i], convs2[i]) pair of the NSF-HiFiGAN ResBlock (residuals.py:22-44) in one launch:
 *   y = x + c2(lrelu(c1(lrelu(x), dilation dil, pad dil*(K-1)/2)), pad (K-1)/2)   [+ y when accumulate]
 * on the split-bf16 engine, with c1's output kept in LDS (never written to HBM).  C = 32 or 64 channels
 * (the generator's last two stages, synthesizers.py:157-159), odd K <= 15, (K-1)*dil <= 64.
 * w1x / w2x: the convs' rvc_conv1d_pack_x6 images (nphase 1, Ci = Co = C; nmf1 / nmf2 their wx_nmf);
 * b1 / b2: f32 biases [C]; passes 6 / 3 / 1 as rvc_conv1d_args.wx_passes; slope: the lrelu slope (0.1).
 * x and y must not alias.  Bit-identical to the two rvc_conv1d launches it replaces.
 * B clips (0 = 1): x, y are [B][C][L] (dense); each clip's result is bit-identical to a B = 1 call on it. */
typedef struct rvc_resblock_args {
    const float* x;
    float* y;
    const void* w1x;
    const float* b1;
    const void* w2x;
    const float* b2;
    int64_t C, L;
    int K, dil, nmf1, nmf2, passes, accumulate;
    float slope;
    int B;
} rvc_resblock_args;

int64_t rvc_resblock_lds_bytes(int64_t C, int K, int dil, int passes);
int rvc_resblock_pair(const rvc_resblock_args* a, rvc_stream_t stream);

/* ------------------------------------------------------------------ attention
 * Flash-style multi-head attention on f32 MFMA over channels-first Q/K/V
 * ([B][H][D][T], channel stride ldc, t contiguous); O written in the same layout.
 * Replaces F.multi_head_attention_forward in ContentVec (fairseq.py:355-357,
 * D = 64, no mask: the single padded key of :1106-1111 has weight exactly 0) and
 * the TextEncoder's relative-position MHA (synthesizers.py:227-251, D = 96,
 * window W = 10): pass rk = scale * Q^T Ek as [B][H][2W+1][T], ev = Ev [2W+1][D]
 * and an ml scratch [B][H][2][T]; the value band term is added in a second pass.
 */
typedef struct rvc_attn_args {
    const float* q;
    const float* k;
    const float* v;
    float* o;
    const float* rk; /* NULL = no relative band                */
    const float* ev; /* [2W+1][D] (shared by heads) or NULL     */
    float* ml;       /* [B][H][2][T] scratch (required with rk) */
    int64_t B, H, D, T;
    int64_t ldc;                    /* channel stride (0 = T) */
    int64_t q_hs, k_hs, v_hs, o_hs; /* head strides           */
    int64_t q_bs, k_bs, v_bs, o_bs; /* batch strides          */
    int W, _pad0;
    float scale, _pad1;
} rvc_attn_args;

/* Long sequences are split over the keys (split-KV) to fill the chip; the partials need a
 * workspace of rvc_attention_workspace_bytes(a) bytes (0 when not split). */
int64_t rvc_attention_workspace_bytes(const rvc_attn_args* a);
int rvc_attention(const rvc_attn_args* a, void* ws, int64_t ws_bytes, rvc_stream_t stream);
/* the same, also folding max |o| into a |max| cell per batch element (amax_out as rvc_layernorm_cf_amax; with the
 * relative band only together with its value term ev, whose kernel publishes the final values) */
int rvc_attention_amax(const rvc_attn_args* a, unsigned* amax_out, void* ws, int64_t ws_bytes, rvc_stream_t stream);
/* Round 6: with amax_in (the |max| cell of q, k and v -- the QKV projection's published cell, one per batch element)
 * both products run in split-fp16 on the fp16 matrix cores (power-of-2 scaled operands split into 11 + 11 bit fp16
 * pieces, hH + hL + lH, f32 accumulation: ~2^-22 relative per product, the conv engine's arithmetic); NULL amax_in =
 * the f32-MFMA kernel.  amax_out as rvc_attention_amax. */
int rvc_attention_ex(const rvc_attn_args* a, const unsigned* amax_in, unsigned* amax_out, void* ws, int64_t ws_bytes,
                     rvc_stream_t stream);
/* This thread's choice for rvc_attention_ex with amax_in: 1 split-fp16, 0 the f32 kernel, -1 RVC_ATTN_F16 (default 1).
 * A/B and test knob. */
int rvc_attention_set_f16(int on);

/* ------------------------------------------------------------------ elementwise
 * Memory-bound pieces of Synthesizer.infer (synthesizers.py:446-465).  All
 * [B][C][T] channels-first.
 */
/* out = lrelu((lin + emb[pitch]) * scale, slope)       synthesizers.py:367 */
int rvc_textenc_embed(const float* lin, const float* emb, const int64_t* pitch, float* out, int64_t B, int64_t C,
                      int64_t T, float scale, float slope, rvc_stream_t stream);
/* the same, also folding max |out| into a |max| cell per batch element (round 6: the TextEncoder's first split-fp16
 * GEMM takes its scale from it) */
int rvc_textenc_embed_amax(const float* lin, const float* emb, const int64_t* pitch, float* out, int64_t B, int64_t C,
                           int64_t T, float scale, float slope, unsigned* amax_out, rvc_stream_t stream);
/* LayerNorm over channels of (x + res)                  synthesizers.py:170-181, fairseq.py:700 */
int rvc_layernorm_cf(const float* x, const float* res, const float* gamma, const float* beta, float* out, int64_t B,
                     int64_t C, int64_t T, float eps, rvc_stream_t stream);
/* the same, also folding max |out| into a |max| cell (amax_out: RVC_AMAX_SHARDS zeroed u32 words per batch element, the
 * amax_in of the GEMM that reads out; ContentVec's LayerNorms -- any C <= 2048, both LayerNorm forms) */
int rvc_layernorm_cf_amax(const float* x, const float* res, const float* gamma, const float* beta, float* out,
                          int64_t B, int64_t C, int64_t T, float eps, unsigned* amax_out, rvc_stream_t stream);
/* GroupNorm(C, C) over time + affine (+ exact GELU)      fairseq.py:1149-1155,1183-1185 */
int rvc_chnorm_gelu(const float* x, const float* gamma, const float* beta, float* out, int64_t B, int64_t C, int64_t L,
                    float eps, int gelu, rvc_stream_t stream);
/* ContentVec's first layer fused (fairseq.py:1165-1195, layer 0): conv(1 -> C, k K, stride) of the 16 kHz signal x
 * [B][N] (w_km: the K-major packed weight [K][C], no bias) + GroupNorm(C, C) over time + affine (+ exact GELU) ->
 * out [B][C][T], T = (N - K) / stride + 1; statistics in f64.  ws: rvc_fe0_ws_bytes(B, C, T) device bytes.
 * Replaces rvc_conv1d + rvc_chnorm_gelu for that layer (no HBM round trip of the conv output). */
int64_t rvc_fe0_ws_bytes(int64_t B, int64_t C, int64_t T);
int rvc_fe0_gn_gelu(const float* x, int64_t B, int64_t N, int64_t x_bstride, const float* w_km, int64_t C, int K,
                    int stride, const float* gamma, const float* beta, float* out, float eps, int gelu, void* ws,
                    int64_t ws_bytes, rvc_stream_t stream);
/* the same, also folding max |out| into a |max| cell per batch element (amax_out as rvc_layernorm_cf_amax): layer 1's
 * split-fp16 conv takes its activation scale from it (round 6).  C <= 819 (the per-channel LDS records), K <= 16. */
int rvc_fe0_gn_gelu_amax(const float* x, int64_t B, int64_t N, int64_t x_bstride, const float* w_km, int64_t C, int K,
                         int stride, const float* gamma, const float* beta, float* out, float eps, int gelu,
                         unsigned* amax_out, void* ws, int64_t ws_bytes, rvc_stream_t stream);
/* z_p = m + exp(logs) * noise * nscale, stats = [m; logs]  synthesizers.py:449 */
int rvc_prior_sample(const float* stats, const float* noise, float* zp, int64_t B, int64_t C, int64_t T, float nscale,
                     rvc_stream_t stream);
/* out = tanh(a[:H]) * sigmoid(a[H:])                    commons.py:35-41 */
int rvc_gate(const float* a, float* out, int64_t B, int64_t H, int64_t T, rvc_stream_t stream);
/* out[c] = x[C-1-c]                                      residuals.py:53-58 */
int rvc_flip_channels(const float* x, float* out, int64_t B, int64_t C, int64_t T, rvc_stream_t stream);
/* out[b][c][r] = in[b][r][c] */
int rvc_transpose(const float* in, float* out, int64_t B, int64_t R, int64_t C, rvc_stream_t stream);
/* standard normal noise, Philox4x32-10 counter stream (seed, offset): value e of a call is draw e % 4 of counter
 * e / 4 + offset.  Counter ranges the synthesizer's draws take under a clip's seed (disjoint for clips below 2^36
 * values per draw):
 *   0                      the prior's z noise                                     [inter][T]
 *   1 << 40                the harmonic source's additive noise                    [L] (Default), [L][H] (MRF, RefineGAN)
 *   1 << 39                the harmonic source's initial phases (rvc_rand_uniform)  [H] (MRF, RefineGAN)
 *   (2 + k) << 40          RefineGAN's k-th AdaIN draw, k = 0 .. 6 * stages - 1 in the reference's draw order
 *                          (stage-major, then branch, then the leading and the trailing AdaIN) */
int rvc_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, rvc_stream_t stream);
/* the same with seed += *seed_add read on the device (seed_add may be NULL): graph replays draw fresh noise */
int rvc_randn_ex(float* out, int64_t n, uint64_t seed, uint64_t offset, const uint64_t* seed_add,
                 rvc_stream_t stream);
/* symmetric triangular draws on [lo, hi] (CREPE's dither, scipy.stats.triang(c=0.5), CREPE.py:118),
 * same counter stream; used when the CREPE pass is graph-captured (host numpy draws cannot be) */
int rvc_rand_triang(float* out, int64_t n, float lo, float hi, uint64_t seed, uint64_t offset,
                    const uint64_t* seed_add, rvc_stream_t stream);
/* NSF harmonic source: SineGen + Linear(1,1) + tanh    synthesizers.py:69-112
 * f0 [B][T] -> har [B][T*upp]; noise [B][T*upp]; work: [B][T] floats scratch */
int rvc_sine_source(const float* f0, const float* noise, float* har, float* work, int64_t B, int64_t T, int upp,
                    float sr, float lin_w, float lin_b, rvc_stream_t stream);

/* ------------------------------------------------------------------ MRF-HiFi-GAN / RefineGAN decoders (vocoder.hip)
 * Every call takes B clips of one length; clip b's result does not depend on the other clips. */
#define RVC_HARMONIC_MAX 16 /* harmonics per source */
#define RVC_ADAIN_BMAX 16   /* clips per rvc_adain call that draws its noise in the kernel */
/* uniform draws on [0, 1) (24 bits), the Philox counter stream of rvc_randn */
int rvc_rand_uniform(float* out, int64_t n, uint64_t seed, uint64_t offset, const uint64_t* seed_add,
                     rvc_stream_t stream);
/* Per-sample harmonic source: SineGenerator + merge    mrf_hifigan.py:45-94 (H = 9, nearest f0, bias),
 * refinegan.py:66-107 (H = 1, linear f0, lin_b = 0).
 *   f0 [B][T] -> har [B][L], L = T*upp;  phase0 [B][H] (harmonic 0's is used as given: pass 0 as the reference does);
 *   noise [B][L][H] (h contiguous);  lin_w: H HOST floats (the merge's weight row), lin_b its bias;
 *   linear: 0 = nearest f0 upsampling (torch's legacy rule, floorf(i * f32(1/upp))), 1 = linear (align_corners=False).
 * The phase of harmonic h is the prefix sum over all L samples of the f32 increments ((f0*(h+1))/sr) % 1, accumulated
 * in f64 with the fractional part taken before sinf (what torch's CPU cumsum computes, up to the wraps it subtracts);
 * a multi-block scan: block sums, a carry pass, then the per-sample pass.
 * ws: rvc_harmonic_source_ws_bytes(B, T, upp, H) bytes, 8-byte aligned (-1: bad shape).  Limits: 1 <= H <=
 * RVC_HARMONIC_MAX, B <= 65535, and L <= 2^24 with linear = 1 (sample indices pass through f32 as in torch).
 * rvc_harmonic_source_chunk(): samples per block of the scan. */
int64_t rvc_harmonic_source_ws_bytes(int64_t B, int64_t T, int upp, int H);
int64_t rvc_harmonic_source_chunk(void);
int rvc_harmonic_source(const float* f0, const float* phase0, const float* noise, float* har, int64_t B, int64_t T,
                        int upp, int H, int linear, float sr, const float* lin_w, float lin_b, void* ws,
                        int64_t ws_bytes, rvc_stream_t stream);
/* y[b][c][j] = linear interpolation of act(x[b][c][.]) by the integer rate r, j < Lin*r    nn.Upsample(scale_factor=r,
 * mode="linear"), align_corners=False: source position (j + 0.5)/r - 0.5 clamped at 0, right neighbour clamped at Lin-1,
 * in the operation order of torch's CPU kernel.  act: RVC_ACT_NONE or RVC_ACT_LRELU(slope), applied to the INPUT samples.
 * x rows [Lin] contiguous, batch stride x_bstride (0 = C*Lin); y rows [Lin*r] contiguous, batch stride y_bstride
 * (0 = C*Lin*r; larger to write the first C channels of a wider buffer, whose other rows are left alone).
 * Limits: B, C <= 65535, Lin*r <= 2^24, x != y. */
int rvc_upsample_linear(const float* x, float* y, int64_t B, int64_t C, int64_t Lin, int r, int64_t x_bstride,
                        int64_t y_bstride, int act, float slope, rvc_stream_t stream);
/* AdaIN: y = out_scale * lrelu(x + n * w[c], slope), or y += that with accumulate    refinegan.py:39-46
 *   x, y [B][C][L] contiguous (y may be x unless accumulate), w [C].
 *   noise [B][C][L], or NULL: n is drawn in the kernel, bit-identical to rvc_randn_ex(buf_b, C*L, seeds[b], offset,
 *   seed_add) filling clip b's buffer; seeds: B HOST values, B <= RVC_ADAIN_BMAX.
 * The three branches' trailing AdaINs form their mean with accumulate and out_scale = 1/3. */
int rvc_adain(const float* x, const float* noise, const float* w, float* y, int64_t B, int64_t C, int64_t L,
              float slope, float out_scale, int accumulate, const uint64_t* seeds, uint64_t offset,
              const uint64_t* seed_add, rvc_stream_t stream);

/* ------------------------------------------------------------------ RMVPE (RMVPE.py)
 * framesT[n][f] = x[reflect(f*hop + n - nfft/2)] * win[n]               RMVPE.py:168 (torch.stft center)
 * mag[k][f] = |spec[k][f] + i spec[K+k][f]|                            RMVPE.py:169
 * img (bordered [Tp+2][M+2]) = BN(mel^T), frames reflect-padded to Tp     RMVPE.py:64,144,213
 * avgpool2 / interleave4 on bordered images                              RMVPE.py:35,93
 * img_to_seq: [C][H][W] image -> [C*W][H] sequence                       RMVPE.py:144
 *        mel_image, avgpool2 and interleave4 write the zero border of the image they produce (interleave4: of its
 *        C channels) as well as its interior: the output needs no zero fill.  One image per call; the f64 forms
 *        below (the same kernels) take B images.
 * bigru: recurrence of nn.GRU(384, 256, bidirectional); gi = W_ih x + b_ih
 *        [2][768][T], whh [2][768][256], bhh [2][768], y [512][T];
 *        gran_ws: 8 KiB scratch (zeroed by the call), err: device int set to 1 when a step's hand-off wait
 *        exceeds the spin limit (the kernel then drains and y is incomplete); sticky until the caller clears it
 * bigru_set_spin_limit: polls per hand-off wait before the timeout fires (default 2^22); 0 only queries.
 *        Returns the previous limit.  For tests that force the timeout path.
 * rmvpe_decode: salience [360][ld] -> f0 (f64, optional), coarse (int64), pitchf (f32)
 *        RMVPE.py:217-252 + convert.py:311-323, f64, numpy's reduction order
 */
int rvc_stft_frames(const float* x, const float* win, float* framesT, int64_t N, int64_t F, int nfft, int hop,
                    rvc_stream_t stream);
int rvc_spec_mag(const float* spec, float* mag, int64_t K, int64_t F, rvc_stream_t stream);
/* stft_mag: B signals x [b * x_bstride + n] (n < N) -> mag [b * mag_bstride + k * F + f] = |STFT| (k <= nfft/2),
 *        reflect-centred frames x win (torch.stft center=True + sqrt(re^2 + im^2), RMVPE.py:168-169), an f64 FFT
 *        rounded to f32 once; nfft a power of 2 <= 1024.  Replaces stft_frames + the DFT GEMM + spec_mag. */
int rvc_stft_mag(const float* x, const float* win, float* mag, int64_t B, int64_t N, int64_t F, int nfft, int hop,
                 int64_t x_bstride, int64_t mag_bstride, rvc_stream_t stream);
int rvc_mel_image(const float* mel, float* img, int64_t M, int64_t F, int64_t Tp, float scale, float shift,
                  rvc_stream_t stream);
int rvc_avgpool2(const float* in, float* out, int64_t C, int64_t H, int64_t W, rvc_stream_t stream);
int rvc_interleave4(const float* phases, float* out, int64_t C, int64_t H, int64_t W, rvc_stream_t stream);
int rvc_img_to_seq(const float* img, float* x, int64_t C, int64_t H, int64_t W, rvc_stream_t stream);
int rvc_bigru(const float* gi, const float* whh, const float* bhh, float* y, void* gran_ws, int* err, int64_t T,
              rvc_stream_t stream);
unsigned rvc_bigru_set_spin_limit(unsigned limit);
/* bigru_batched: B independent sequences (gi + b*gi_bs, y + b*y_bs); gran_ws: 8192 B * min(B, 16) scratch. */
int rvc_bigru_batched(const float* gi, int64_t gi_bs, const float* whh, const float* bhh, float* y, int64_t y_bs,
                      void* gran_ws, int* err, int64_t B, int64_t T, rvc_stream_t stream);

/* ------------------------------------------------------------------ RMVPE in f64 (rmvpe64.hip)
 * RMVPE's f0 is a per-frame decision (argmax over 360 bins, 0.03 voicing threshold, RMVPE.py:217-252) and
 * some frames' top two bins lie closer than any f32 evaluation of the network resolves, so the f0 model runs
 * in f64 end to end (rvc_rmvpe_forward): the same steps as the f32 entry points above, on f64
 * buffers, with the salience rounded to f32 once.
 *
 * conv64: y[b][m][t] = act(sum_{c,k} w[c*K + k][m] x[b][c][t - pad + off(k)] + bias[m]) (+ res[b][m][t]),
 *   off(k) = toff[k] (ntoff == K) or k; x positions outside [0, Lin) read 0.  w is KM [Ci*K][Co] f64.
 *   wrap > 0: 2-D mode on zero-bordered images flattened to Lout = rows x wrap -- border cells are stored as 0.
 *   y is f64, or f32 (rounded once) when y_f32.  out_act: RVC_ACT_NONE / RELU / SIGMOID / LOGCLAMP (out_slope =
 *   the clamp).
 *   Stride 1, no groups.  Replaces torch.nn.Conv2d (3x3 pad 1 / 1x1) and nn.Linear in E2E / MelSpectrogram
 *   (RMVPE.py:11-44, 78-107, 141-144, 162-181), batch b in [0, B) with strides (0 = dense). */
typedef struct rvc_conv64_args {
    const double* x;
    const double* w;
    const double* bias;
    const double* res;
    void* y;
    int64_t B, Ci, Co, Lin, Lout;
    int64_t x_bstride, y_bstride, res_bstride;
    int K, pad, out_act, y_f32;
    double out_slope;
    int ntoff, wrap;
    int toff[16];
    /* per-batch weights: batch b uses w + (b % w_bmod) * w_bstride (w_bmod 0: every batch the same w) */
    int64_t w_bstride;
    int w_bmod, _pad0;
} rvc_conv64_args;
/* split-K workspace (bytes; 0 = none, -1 = bad args), as rvc_conv1d_workspace_bytes */
int64_t rvc_conv64_workspace_bytes(const rvc_conv64_args* a);
/* the planner's choice for a (diagnostics): out[0] tile (0..7: 16x512, 16x256, 32x256, 32x128, 64x128, 64x64,
 * 128x128, 128x64 with 16-deep k chunks; 8..12: 16x256, 32x128, 64x128, 64x64, 128x64 with 32-deep; 13, 14: 128x16
 * with 16- / 32-deep; 15..17: 16x256, 32x128, 32x256 with 36-deep = 4 whole channels of a 3x3 conv), out[1] split-K, out[2] compact form (wrap > 0: the H x W interior cells as the GEMM's
 * columns instead of the bordered image), out[3] blocks of the conv launch */
int rvc_conv64_plan(const rvc_conv64_args* a, int* out);
/* force the planner (process-wide; sweeps and tests): tile -1..17, ksplit -1..32, compact -1..1 (-1 = planner's) */
int rvc_conv64_set_plan(int tile, int ksplit, int compact);
int rvc_conv64(const rvc_conv64_args* a, void* ws, int64_t ws_bytes, rvc_stream_t stream);
/* Winograd F(4x4, 3x3) f64 conv for RMVPE's deep levels (3x3 pad 1 on bordered [C][H+2][W+2] images, as
 * conv64 with wrap): y = act(conv(x) + bias) (+ res), border cells 0.  v = rvc_wino64_weights(KM w [Ci*9][Co])
 * = the 36 transformed weight matrices [36][Ci][Co] (G g G^T).  rvc_wino64_use(Ci, Co, H, W): whether the f64
 * RMVPE takes this form for a Ci -> Co conv on an H x W image (>= 64 channels each and >= 90 4x4 output tiles,
 * RVC_RMVPE_WINO_MINP; H or W <= 0: the channel rule alone, whether to prepare v; RVC_RMVPE_WINO=0: never).
 * rvc_wino64_conv itself takes any channel counts: 16 / 32 / 64 -> 16 / 32 channels run one fused kernel (transforms
 * in LDS, no workspace; measured no faster than conv64, so rvc_wino64_use leaves those shapes to conv64 unless
 * RVC_RMVPE_WINO=3), the rest the three-step form with its workspace. */
typedef struct rvc_wino64_args {
    const double* x;
    const double* v;
    const double* bias;
    const double* res;
    void* y;
    int64_t B, Ci, Co, H, W;
    int64_t x_bstride, y_bstride, res_bstride;
    int out_act, y_f32;
} rvc_wino64_args;
int rvc_wino64_use(int64_t Ci, int64_t Co, int64_t H, int64_t W);
int rvc_wino64_weights(const double* w, double* v, int64_t Ci, int64_t Co, rvc_stream_t stream);
int64_t rvc_wino64_workspace_bytes(const rvc_wino64_args* a);
int rvc_wino64_conv(const rvc_wino64_args* a, void* ws, int64_t ws_bytes, rvc_stream_t stream);
/* stft_mag64: rvc_stft_mag with the f64 magnitudes unrounded */
int rvc_stft_mag64(const float* x, const float* win, double* mag, int64_t B, int64_t N, int64_t F, int nfft, int hop,
                   int64_t x_bstride, int64_t mag_bstride, rvc_stream_t stream);
/* f64 forms of rvc_mel_image / avgpool2 / interleave4 / img_to_seq (the same kernels) over B images (batch strides
 * in elements, unused when B == 1); like them, the three that produce a bordered image write its zero border. */
int rvc_mel_image64(const double* mel, double* img, int64_t B, int64_t M, int64_t F, int64_t Tp, double scale,
                    double shift, int64_t mel_bstride, int64_t img_bstride, rvc_stream_t stream);
int rvc_avgpool2_64(const double* in, double* out, int64_t B, int64_t C, int64_t H, int64_t W, int64_t in_bstride,
                    int64_t out_bstride, rvc_stream_t stream);
int rvc_interleave4_64(const double* phases, double* out, int64_t B, int64_t C, int64_t H, int64_t W,
                       int64_t ph_bstride, int64_t out_bstride, rvc_stream_t stream);
int rvc_img_to_seq64(const double* img, double* x, int64_t B, int64_t C, int64_t H, int64_t W, int64_t img_bstride,
                     int64_t x_bstride, rvc_stream_t stream);
/* bigru64_batched: rvc_bigru_batched in f64 (gi [2][768][T], whh [2][768][256], bhh [2][768], y [512][T] per
 * sequence); gran_ws: RVC_BIGRU64_GRAN_BYTES * min(B, 16) scratch (zeroed by the call); err as rvc_bigru. */
#define RVC_BIGRU64_GRAN_BYTES 16384
/* The f64 BiGRU's recurrence arithmetic, per thread: 1 = W_hh h and the gates in f32 (the default: its decision noise
 * on the headline clip is 1.8e-9, three orders below the smallest exact margin; gi and y stay f64), 0 = all f64,
 * -1 = back to RVC_BIGRU64_F32 (default 1). */
int rvc_bigru64_set_f32(int on);
int rvc_bigru64_batched(const double* gi, int64_t gi_bs, const double* whh, const double* bhh, double* y,
                        int64_t y_bs, void* gran_ws, int* err, int64_t B, int64_t T, rvc_stream_t stream);
/* Optional steps of VC.get_f0 between the raw f0 and the mel quantiser (convert.py:311-318), in
 * the reference's order: autotune (Autotune.autotune_f0, convert.py:168-179: f += (nearest of the 54
 * reference notes - f) * strength, first note on ties, unvoiced frames included) on the raw f0, then
 * the pitch shift, then the f0-file override f0[rep_off + i] = rep[i] for i < rep_len (convert.py:314-318,
 * rep = the host's np.interp of the file, f64).  NULL = none of them.  Arithmetic is f64 on the RMVPE
 * path (its f0 is f64) and f32 on the CREPE path (its f0 is f32), as in NumPy 2. */
typedef struct rvc_f0_post {
    int autotune, _pad0;
    double strength;
    const double* rep; /* device f64 [rep_len] or NULL */
    int64_t rep_off, rep_len;
} rvc_f0_post;

int rvc_rmvpe_decode(const float* sal, int64_t ld, int64_t F, double thred, double shift, const rvc_f0_post* post,
                     double* f0, int64_t* coarse, float* pitchf, rvc_stream_t stream);
/* rmvpe-legacy (get_f0_rmvpe(legacy=True), convert.py:248-255; RMVPE.infer_from_audio_with_pitch, RMVPE.py:228-234):
 * rvc_rmvpe_decode with f0[(f0 < f0_min) | (f0 > f0_max)] = 0 on the decoded f64 f0 (VC passes 50 and 1100; the bins
 * span 31.7 .. 2005 Hz), in the same kernel, before the autotune / shift / f0 file of `post` and the quantiser.
 * rvc_rmvpe_decode is this entry at (-inf, +inf), where the test is never true.  A NaN bound is RVC_EINVAL. */
int rvc_rmvpe_decode_range(const float* sal, int64_t ld, int64_t F, double thred, double f0_min, double f0_max,
                           double shift, const rvc_f0_post* post, double* f0, int64_t* coarse, float* pitchf,
                           rvc_stream_t stream);

/* pm f0 (VC.get_f0_pm, convert.py:206-213): Praat's To Pitch (ac) with get_f0_pm's settings on the f64
 * 16 kHz signal x [n] -> f0 [rvc_pm_frames(n)] (0 = unvoiced); window [958] = Praat's Hann window
 * 0.5 - 0.5 cos(2 pi i / 959), i = 1..958, window_r [480] its normalised autocorrelation; work:
 * rvc_pm_work_bytes(n) bytes.  rvc_pm_post: get_f0_pm's zero padding to p_len (when p_len > nf), then
 * get_f0's autotune / shift / f0 file (post, as rvc_rmvpe_decode) and mel quantiser -> coarse, pitchf
 * [max(p_len, nf)].  Restated from Boersma (1993) / Praat: parity unpinned (no parselmouth here). */
int64_t rvc_pm_frames(int64_t n);
int64_t rvc_pm_work_bytes(int64_t n);
int rvc_pm_f0(const double* x, int64_t n, const double* window, const double* window_r, void* work,
              int64_t work_bytes, double* f0, rvc_stream_t stream);
/* rvc_pm_windows: the window [958] and window_r [480] rvc_pm_f0 takes, computed on the HOST (host pointers). */
int rvc_pm_windows(double* window, double* window_r);
int rvc_pm_post(const double* f0, int64_t nf, int64_t p_len, double shift, const rvc_f0_post* post,
                int64_t* coarse, float* pitchf, rvc_stream_t stream);

/* swipe f0 (VC.get_f0_swipe, convert.py:272-276: SWIPE' at 16 kHz, 50..1100 Hz, 10 ms frames, strength
 * threshold 0.3), f64 on the f32 samples.  rvc_swipe_tables builds, on the HOST (host pointer), the constant
 * blob of rvc_swipe_tables_bytes() bytes that the device entries take as `tables` once it is uploaded.
 * rvc_swipe_table_dims(which, window, dims) returns the byte offset of one table in the blob and writes
 * dims = {rows, cols, leading dimension}; `window` (0..4 = window size 2048 >> window) selects among the
 * per-window tables and is ignored by the others.
 *   rvc_swipe_strength  x f32 [n] -> S f64 [429][rvc_swipe_frames(n)]; work: rvc_swipe_work_bytes(n) bytes
 *   rvc_swipe_pick      S [429][F] -> f0 f32 [F] (0 = unvoiced)
 *   rvc_swipe_post      get_f0's autotune / shift / f0 file (post, as rvc_rmvpe_decode) and mel quantiser
 *                       in f32 arithmetic -> coarse, pitchf [F]
 * No entry synchronises or allocates. */
enum {
    RVC_SWIPE_PC = 0,    /* f64 [429] pitch candidates */
    RVC_SWIPE_FERBS = 1, /* f64 [328] ERB-spaced frequencies */
    RVC_SWIPE_IDX = 2,   /* int32 [nc_w] the candidates window w serves */
    RVC_SWIPE_MU = 3,    /* f64 [nc_w] their weights */
    RVC_SWIPE_W = 4,     /* f64 [328][ws/2 + 1] (ld: padded to 16) not-a-knot cubic spline onto fERBs */
    RVC_SWIPE_K = 5,     /* f64 [nc_w][328] (ld 336) prime-harmonic cosine kernels */
    RVC_SWIPE_WIN = 6,   /* f64 [ws + 1] np.hanning(ws + 2)[1:-1], then its sum */
    RVC_SWIPE_TW = 7,    /* f64 [1024][2] exp(-2 pi i k / 2048) */
    RVC_SWIPE_CMAP = 8,  /* int32 [429][2][2] (window, index in it) of the windows serving a candidate; -1 none */
    RVC_SWIPE_CMU = 9,   /* f64 [429][2] their weights */
    RVC_SWIPE_PX = 10,   /* f64 [429][2] the pick parabola's outer abscissae */
    RVC_SWIPE_GRIDX = 11,  /* f64 [429][17] the pick grid's abscissae */
    RVC_SWIPE_GRIDF0 = 12, /* f32 [429][17] the f0 each grid point stands for */
    /* W and K again as the kernels read them, in MFMA operand order: [row tile][K/16][lane 0..63][u 0..3] =
     * M[16 tile + (lane & 15)][4 (4 k16 + u) + (lane >> 4)] over the zero-padded matrix (dims: tiles x K*16) */
    RVC_SWIPE_WP = 13,
    RVC_SWIPE_KP = 14
};
int64_t rvc_swipe_frames(int64_t n);     /* n / 160 + 1; -1 for n <= 0 */
int64_t rvc_swipe_work_bytes(int64_t n); /* -1 for n <= 0 or n >= 2^30 */
int64_t rvc_swipe_tables_bytes(void);
int64_t rvc_swipe_table_dims(int which, int window, int64_t* dims);
int rvc_swipe_tables(void* blob, int64_t bytes);
int rvc_swipe_strength(const float* x, int64_t n, const void* tables, void* work, int64_t work_bytes, double* S,
                       rvc_stream_t stream);
int rvc_swipe_pick(const double* S, int64_t F, const void* tables, float* f0, rvc_stream_t stream);
int rvc_swipe_post(const float* f0, int64_t F, float shift, const rvc_f0_post* post, int64_t* coarse,
                   float* pitchf, rvc_stream_t stream);

/* hybrid[a+b+...] f0 (VC.get_f0_hybrid, convert.py:283-302).
 *   rvc_abs_quantile  np.quantile(np.abs(x), 0.999) of f32 x [n] -> device f32 scalar q_out, as NumPy 2
 *                     evaluates it for an f32 array (index, gamma and lerp in f32); a radix select, no sort;
 *                     work: rvc_abs_quantile_work_bytes() bytes of device memory
 *   rvc_abs_quantile_as  the same with the last step named: RVC_QUANTILE_NUMPY is rvc_abs_quantile;
 *                     RVC_QUANTILE_TORCH is torch.quantile(torch.abs(x), 0.999) as ATen's CPU kernel evaluates it
 *                     (FeatureInput.get_mangio_crepe, extract.py:166): the same f32 rank and order statistics, but
 *                     each branch of the lerp is one fused multiply-add, which moves the last bit of about one
 *                     result in a hundred
 *   rvc_div_scalar    out[i] = x[i] / q[0], a true f32 division by the device scalar (out may be x)
 *   rvc_f0_mix        M <= RVC_F0_MIX_MAX raw tracks (device f32 or f64, each with its own length) -> out f64
 *                     [p_len]: np.interp(np.linspace(0, n_m, p_len), np.arange(n_m), f0_m) in f64 per track,
 *                     then np.nanmedian over the tracks (one track: the resampled track).  p_len >= 2.
 *   rvc_f0_resample_nan  the tail of get_f0_mangio_crepe (convert.py:226-228; the same expression ends get_f0_yin):
 *                     source f32 [T] -> out f64 [p_len] in one launch: source[source < 0.001] = nan (an f32
 *                     compare), np.interp(np.arange(0, T * p_len, T) / p_len, np.arange(T), source) in f64 by
 *                     NumPy's rules (an exact hit returns fp[j]; a position past T - 1 returns fp[-1]; a NaN result
 *                     is retried from the other end point, then takes the common value of two equal end points),
 *                     then np.nan_to_num (nan -> 0, +-inf -> +-DBL_MAX).  T, p_len >= 1.  It shares rvc_f0_mix's
 *                     np.interp device function.
 * The mixed track's autotune / shift / f0 file / quantiser is rvc_pm_post with nf = p_len. */
enum { RVC_F0_MIX_MAX = 8 };
typedef struct rvc_f0_track {
    const void* f0; /* device f32 or f64 [n] */
    int64_t n;
    int is_f64, _pad0;
} rvc_f0_track;
int64_t rvc_abs_quantile_work_bytes(void);
int rvc_abs_quantile(const float* x, int64_t n, void* work, int64_t work_bytes, float* q_out, rvc_stream_t stream);
enum { RVC_QUANTILE_NUMPY = 0, RVC_QUANTILE_TORCH = 1 };
int rvc_abs_quantile_as(const float* x, int64_t n, int lerp, void* work, int64_t work_bytes, float* q_out,
                        rvc_stream_t stream);
int rvc_div_scalar(const float* x, int64_t n, const float* q, float* out, rvc_stream_t stream);
int rvc_f0_mix(const rvc_f0_track* tracks, int M, int64_t p_len, double* out, rvc_stream_t stream);
int rvc_f0_resample_nan(const float* source, int64_t T, int64_t p_len, double* out, rvc_stream_t stream);

/* fcpe f0 (VC.get_f0_fcpe, convert.py:239-246: the conv-only CFNaiveMelPE of main/library/predictors/FCPE.py).
 * A host runs, per signal: rvc_fcpe_mel; rvc_conv1d (k=3, 128 -> C); rvc_groupnorm_act; rvc_conv1d (k=3);
 * per layer rvc_layernorm_cf, rvc_conv1d (1x1, C -> 4C), rvc_glu_dwconv_silu, rvc_conv1d (1x1, 2C -> C, res =
 * the layer's input); rvc_layernorm_cf; rvc_conv1d (1x1, C -> 360, out_act = sigmoid); rvc_fcpe_decode;
 * rvc_fcpe_post; rvc_pm_post (nf = p_len).  All tensors channels-first [B][C][T] f32.
 *   rvc_fcpe_mel         MelModule.__call__ at key_shift 0, speed 1 + Wav2MelModule's frame fix-up
 *                        (FCPE.py:838-876, 898-913): x [B][N] at 16 kHz, reflect-padded by 432 on both sides,
 *                        non-centred frames of 1024 at hop 160 under a periodic Hann window, sqrt(re^2 + im^2 +
 *                        1e-9), basis [128][513] (f32), log(max(., 1e-5)) -> mel [B][128][T], T = N / 160 + 1,
 *                        frame T-1 a copy of frame T-2.  f64 FFT and sums, rounded to f32 once.  N <= 432 (where
 *                        the reference switches to constant padding) is rejected with RVC_EINVAL.
 *   rvc_groupnorm_act    GroupNorm(G, C) over (C/G) x T per batch element (f64 statistics, biased variance),
 *                        affine, then LeakyReLU(slope) (FCPE.py:422; slope 1 = none); work:
 *                        rvc_groupnorm_work_bytes(B, G) bytes
 *   rvc_glu_dwconv_silu  ConformerConvModule's middle (FCPE.py:550): x [B][2H][T] -> u = x[:H] * sigmoid(x[H:]),
 *                        depthwise conv of K taps (K odd <= 31, zero padding K/2, w [H][K], bias [H]), SiLU ->
 *                        y [B][H][T].  One block per channel and RVC_GLU_DW_TILE time steps.
 *   rvc_fcpe_decode      latent2cents_local_decoder + cent_to_f0 + infer's masks (FCPE.py:451-468, 479-480,
 *                        751-756) on the LATENT (after the sigmoid) [B][C][T], C >= 1: first-index argmax, the 9
 *                        bins argmax-4..argmax+4 clamped into [0, C-1] (a clamped bin counts again),
 *                        sum(cent_table * y) / sum(y) and 10 * 2^(cents / 1200) in f32; confidence <= threshold
 *                        -> 0, f0 < f0_min -> 0, f0 > f0_max -> f0_max  -> f0 f32 [B][T]
 *   rvc_fcpe_post        the rest of infer, then FCPE.compute_f0 / post_process (FCPE.py:757-759, 975-1000) on one
 *                        track f0 f32 [T]: zeros -> NaN, F.interpolate(mode="linear") to p_len as torch's CPU
 *                        kernel evaluates it in f32 (a copy when p_len == T), NaN -> 0; no voiced frame -> zeros,
 *                        one -> p_len copies of it, else np.interp in f64 over the voiced frames (nodes
 *                        (hop_length / sample_rate) * idx, queries i * hop_length / sample_rate, ends held)
 *                        -> out f64 [p_len].  One block, no host read-back; work: rvc_fcpe_post_work_bytes(p_len)
 * No entry synchronises or allocates. */
enum { RVC_GLU_DW_TILE = 256, RVC_FCPE_MELS = 128, RVC_FCPE_NFFT = 1024, RVC_FCPE_HOP = 160 };
int rvc_fcpe_mel(const float* x, const float* basis, float* mel, int64_t B, int64_t N, rvc_stream_t stream);
int64_t rvc_groupnorm_work_bytes(int64_t B, int G);
int rvc_groupnorm_act(const float* x, const float* gamma, const float* beta, float* y, int64_t B, int64_t C,
                      int64_t T, int G, float eps, float slope, void* work, int64_t work_bytes,
                      rvc_stream_t stream);
int rvc_glu_dwconv_silu(const float* x, const float* w, const float* bias, float* y, int64_t B, int64_t H,
                        int64_t T, int K, rvc_stream_t stream);
int rvc_fcpe_decode(const float* latent, const float* cent_table, float* f0, int64_t B, int64_t C, int64_t T,
                    float threshold, float f0_min, float f0_max, rvc_stream_t stream);
int64_t rvc_fcpe_post_work_bytes(int64_t p_len); /* -1 for p_len <= 0 or p_len >= 2^24 */
int rvc_fcpe_post(const float* f0, int64_t T, int64_t p_len, int hop_length, int sample_rate, void* work,
                  int64_t work_bytes, double* out, rvc_stream_t stream);

/* fcpe-legacy f0 (get_f0_fcpe(legacy=True): FCPE_LEGACY behind Wav2Mel, threshold 0.03).  The front end, the stack,
 * the Conformer conv module, the decoder and the post stages are the entries above (rvc_fcpe_decode with f0_min = 0
 * and f0_max = FLT_MAX: the legacy model has no range clamp); a layer adds, before its conv module, rvc_layernorm_cf;
 * rvc_conv1d (1x1, C -> 3 * 512: to_q, to_k, to_v stacked); rvc_performer_attention; rvc_conv1d (1x1, 512 -> C,
 * res = the layer's input).
 *   rvc_performer_attention  FAVOR+ linear attention (FCPE.py:87-88, 108-116, 576-583), non-causal, no mask, per
 *                        batch element and head, D = 64 channels per head, proj [M][64] (16-byte aligned),
 *                        1 <= M <= RVC_PERFORMER_MAX_FEATURES, c = 64^-0.25, r = M^-0.5:
 *                          dq[t][j] = c q[t].proj[j]   gq[t] = 0.5 c^2 |q[t]|^2   (dk, gk likewise)
 *                          q'[t][j] = r (exp(dq - gq - max_j dq) + 1e-4)    k'[t][j] = r exp(dk - gk + 1e-4)
 *                          out[t] = (q'[t] . sum_t k'[t]^T v[t]) / (q'[t] . sum_t k'[t] + 1e-8)
 *                        q, k, v, out channels-first: head h is channels 64 h .. 64 h + 63, channel stride ldc
 *                        (0 = T), batch strides in_bs (q, k, v) and out_bs (0 = H * 64 * ldc), so q, k and v may be
 *                        slices of one [B][3 * 64 H][T] buffer.  Every product is an f32 fma chain (f32-input MFMA);
 *                        the partial sums over time are added in a fixed order, so two calls give the same bits.
 *                        Anything else (D != 64, M out of range, a short work buffer) is RVC_EINVAL, before any
 *                        launch.  work: rvc_performer_work_bytes(B, H, T, M) bytes (-1 for a bad shape), 16-byte
 *                        aligned.  Time tiles are RVC_PERFORMER_TILE steps in both passes. */
enum { RVC_PERFORMER_TILE = 32, RVC_PERFORMER_MAX_FEATURES = 272 };
int64_t rvc_performer_work_bytes(int64_t B, int64_t H, int64_t T, int M);
int rvc_performer_attention(const float* q, const float* k, const float* v, const float* proj, float* out, int64_t B,
                            int64_t H, int64_t T, int D, int M, int64_t ldc, int64_t in_bs, int64_t out_bs, void* work,
                            int64_t work_bytes, rvc_stream_t stream);

/* ------------------------------------------------------------------ VC.pipeline glue
 * phone_upsample: nearest x2 + protect blend (convert.py:361-378) -> phone [C][T]
 * peak_normalize: x /= max|x|/0.99 when > 1 (convert.py:450-451); ws: 16 B scratch;
 *                 scale_out (optional device float) receives max|x|/0.99
 */
/* filtfilt_pad: scipy.signal.filtfilt(b, a, x) (padtype odd, padlen 18; convert.py:403) in f64, then
 *   reflect padding by tpad (convert.py:416): x f32 [N] -> out f32 [N + 2*tpad] (+ optional f64 copy).
 *   b[6], a[6], zi[5] (= lfilter_zi(b, a)) are HOST arrays; work: device scratch of
 *   rvc_filtfilt_work_bytes(N) bytes (8-byte aligned). */
int64_t rvc_filtfilt_work_bytes(int64_t N);
int rvc_filtfilt_pad(const float* x, int64_t N, const double* b, const double* a, const double* zi, int64_t tpad,
                     double* work, float* out, double* out64, rvc_stream_t stream);
int rvc_phone_upsample(const float* feats, const float* feats0, const float* pitchf, float* out, int64_t C, int64_t Tf,
                       int64_t T, float protect, rvc_stream_t stream);
int rvc_peak_normalize(float* x, int64_t n, void* ws, float* scale_out, rvc_stream_t stream);
/* quiet_points: VC.pipeline's segmentation of inputs over x_max (convert.py:404-412) on the filtered f64 signal
 *   x [n] (before the t_pad reflect padding): for n + window > t_max, one quiet point per t in
 *   range(t_center, n, t_center): t - t_query + the first argmin of |moving window-sum| over [t - t_query,
 *   t + t_query) (the reference's f64 sums, in its order) -> opt_ts int64 [count] (device).  count =
 *   rvc_quiet_points_count(...) (0 for short inputs); ws: rvc_quiet_points_ws_bytes(...) bytes. */
int64_t rvc_quiet_points_count(int64_t n, int window, int64_t t_center, int64_t t_max);
int64_t rvc_quiet_points_ws_bytes(int64_t n, int window, int64_t t_center, int64_t t_query, int64_t t_max);
int rvc_quiet_points(const double* x, int64_t n, int window, int64_t t_center, int64_t t_query, int64_t t_max,
                     void* ws, int64_t ws_bytes, int64_t* opt_ts, rvc_stream_t stream);
/* change_rms (convert.py:150-152, VC.pipeline volume_envelope != 1, convert.py:449):
 *   rms_frames: librosa.feature.rms(y, frame_length = 2*hop, hop_length = hop) (center, zero pad)
 *     of y [n] (f64 when y64 != NULL, else f32 y32) -> out f32 [1 + n / hop] (mean square in f64).
 *   rms_mix: y[i] *= r1(i)^(1 - rate) * max(r2(i), 1e-6)^(rate - 1), r(i) = F.interpolate(r, n,
 *     "linear", align_corners=False) of the source (r1 [n1]) and output (r2 [n2]) envelopes, f32. */
int64_t rvc_rms_frames_len(int64_t n, int64_t hop);
int rvc_rms_frames(const double* y64, const float* y32, int64_t n, int64_t hop, float* out, rvc_stream_t stream);
int rvc_rms_mix(float* y, int64_t n, const float* r1, int64_t n1, const float* r2, int64_t n2, double rate,
                rvc_stream_t stream);

/* ------------------------------------------------------------------ spectral-gate denoise
 * Replaces main/tools/noisereduce.py:reduce_noise(y, sr, prop_decrease=clean_strength) as
 * VoiceConverter.convert_audio calls it for clean_audio (convert.py:514-516): the non-stationary TG
 * (noisereduce.py:124-180) over SpectralGate.get_traces' chunks (:96-122: chunk_size samples, each
 * zero-padded by `padding` both sides and gated independently), in f64 like the reference.
 *   window: device f64 [n_fft] = torch.hann_window(n_fft) (float32, promoted);
 *   filt:   device f64 [filt_h][filt_w] (TG._generate_mask_smoothing_filter, :144-154) or NULL
 *           with filt_h = filt_w = 0;
 *   n_movemean = int(time_constant_s / hop * sr) (:193); n_thresh = thresh_n_mult_nonstationary;
 *   temp_coeff = 1 / sigmoid_slope_nonstationary.
 * y f32 [n] -> out f32 [n]; work: rvc_denoise_work_bytes(n, a) bytes of device scratch. */
typedef struct rvc_denoise_args {
    int64_t chunk_size, padding;
    int n_fft, hop, n_movemean, filt_h, filt_w, _pad0;
    double prop_decrease, n_thresh, temp_coeff;
    const double* window;
    const double* filt;
} rvc_denoise_args;

int64_t rvc_denoise_work_bytes(int64_t n, const rvc_denoise_args* a);
int rvc_denoise(const float* y, int64_t n, const rvc_denoise_args* a, void* work, int64_t work_bytes, float* out,
                rvc_stream_t stream);

/* ------------------------------------------------------------------ formant shifting
 * Replaces StftPitchShift(n_fft, hop, sample_rate).shiftpitch(x, factors=1, quefrency, distortion)
 * (main/library/algorithm/stftpitchshift.py) as load_audio calls it for formant_shifting
 * (main/library/utils.py:104-108): a phase vocoder at factor 1 whose cepstral envelope is resampled
 * along frequency by `distortion`, in f64 like the reference.  M = (n - n_fft) / hop + 1 frames, no
 * centre padding; the tail the frames do not reach is exactly 0.
 *   n_fft: a power of two in [64, 2048] (the reference's call: 1024); hop in [1, n_fft] (32);
 *   quefrency_samples = int(quefrency * sample_rate), in [0, n_fft / 2]; 0 skips the lifter and
 *     `distortion` with it;
 *   distortion: finite, > 0, int((n_fft / 2 + 1) * distortion) >= 1; 1 leaves the envelope in place;
 *   window:       device f64 [n_fft] = 0.5 - 0.5 cos(2 pi i / n_fft);
 *   synth_window: device f64 [n_fft] = window * hop / sum(window^2).
 * x f32 [n] -> out f32 [n]; work: rvc_formant_work_bytes(n, a) bytes of device scratch (-1 on bad
 * arguments).  Stream-ordered, no host synchronisation, no atomics (bit-reproducible). */
typedef struct rvc_formant_args {
    int n_fft, hop, sample_rate, quefrency_samples;
    double distortion;
    const double* window;
    const double* synth_window;
} rvc_formant_args;

int64_t rvc_formant_work_bytes(int64_t n, const rvc_formant_args* a);
int rvc_formant_shift(const float* x, int64_t n, const rvc_formant_args* a, void* work, int64_t work_bytes, float* out,
                      rvc_stream_t stream);

/* ------------------------------------------------------------------ FAISS IVF-Flat retrieval
 * Replaces faiss IndexIVFFlat(L2).search(feats, k=8) + the blend of convert.py:349-359.
 * Queries (query i, dim c) live at q[c*cs + i*qs] (channels-first [d][nq]: cs = nq, qs = 1).
 * centT: centroids transposed [d][nlist]; inverted lists in CSR form: list_off [nlist+1],
 * codes [ntotal][d] (list-major), ids [ntotal].  Results are D f32 [nq][k] (squared L2), I int64 [nq][k],
 * ascending by (distance, id), missing results (FLT_MAX, -1) as in faiss.
 * Arithmetic (rvc_ivf_search = RVC_IVF_FAISS): faiss's own f32 evaluation -- coarse ||x||^2 + ||c||^2 - 2<x,c>
 * clamped at 0 for nq >= 20 (knn_L2sqr's BLAS path), fvec_L2sqr below 20 and in the list scan, each f32 sum in
 * the structure of faiss's AVX2 kernels (d % 8 == 0); RVC_IVF_EXACT: f64 distances (a diagnostic).
 * ws: rvc_ivf_coarse_ws_bytes(nq, nlist) bytes; probes: int64 [nq][nprobe] scratch/out. */
enum { RVC_IVF_FAISS = 0, RVC_IVF_EXACT = 1 };
int64_t rvc_ivf_coarse_ws_bytes(int64_t nq, int64_t nlist);
int rvc_ivf_search(const float* q, int64_t nq, int64_t d, int64_t cs, int64_t qs, const float* centT, int64_t nlist,
                   int nprobe, const int64_t* list_off, const float* codes, const int64_t* ids, int k, void* ws,
                   int64_t ws_bytes, int64_t* probes, float* D, int64_t* I, rvc_stream_t stream);
int rvc_ivf_search_ex(const float* q, int64_t nq, int64_t d, int64_t cs, int64_t qs, const float* centT,
                      int64_t nlist, int nprobe, const int64_t* list_off, const float* codes, const int64_t* ids,
                      int k, void* ws, int64_t ws_bytes, int64_t* probes, float* D, int64_t* I, int arithmetic,
                      rvc_stream_t stream);
/* out = (sum_j big[I_j] * w_j / sum w) * index_rate + (1 - index_rate) * feats, w = (1/D)^2, in the
 * f32 operation order of the reference's numpy/torch code; big = reconstruct_n(0, ntotal) [ntotal][d]. */
int rvc_ivf_blend(const float* feats, int64_t nq, int64_t d, int64_t fcs, int64_t fqs, const float* D, const int64_t* I,
                  int k, const float* big, int64_t ntotal, double index_rate, float* out, int64_t ocs, int64_t oqs,
                  rvc_stream_t stream);

/* ------------------------------------------------------------------ IVF training (kmeans.hip)
 * The device side of create_index.py:66-83 (index_factory("IVF{n},Flat"), train, add): faiss's k-means steps and the
 * inverted lists.  The iteration loop, the initial permutation and the split of empty clusters are host control
 * (rvc_amd/index_train.py).  Every entry point validates before any launch (d % 8 == 0, 8 <= d <= 1024, as
 * rvc_load_index), runs on the given stream, allocates nothing, never synchronises with the host and uses no
 * floating-point atomics: two runs give identical bits.  x [n][d], cent [k][d]: row-major f32, 16-byte aligned.
 *
 * rvc_kmeans_assign: the nearest centroid of every row, 1 <= k <= n.  The decision value is ||c_j||^2 - 2 <x_i, c_j>
 *   in f32, the inner products on v_mfma_f32_32x32x2_f32 (exact f32 products, one f32 fma chain over the dimensions
 *   in order); equal values resolve to the lowest j.  assign int32 [n]; dist f32 [n] = that value + ||x_i||^2,
 *   clamped at 0.  The [n][k] matrix is never written.  work: rvc_kmeans_assign_work_bytes(n, d, k) bytes.
 * rvc_kmeans_lists: stable counting sort of the row numbers by list: counts int32 [k], list_off int64 [k + 1] (CSR),
 *   ids int64 [n] ascending inside each list, as faiss's sequential add leaves them.  assign values outside [0, k)
 *   are clamped.  work: rvc_kmeans_lists_work_bytes(n, k) bytes.
 * rvc_kmeans_update: faiss compute_centroids: per centroid and dimension the f32 sum of the members in ascending
 *   list position from 0, times 1.f / count (f32); an empty list copies cent_prev.  cent_out != cent_prev.
 * rvc_gather_rows: out [m][d] = x[ids[i]] (ids int64, the caller guarantees their range).
 * The *_work_bytes queries return -1 on bad sizes. */
int64_t rvc_kmeans_assign_work_bytes(int64_t n, int64_t d, int64_t k);
int rvc_kmeans_assign(const float* x, int64_t n, int64_t d, const float* cent, int64_t k, void* work,
                      int64_t work_bytes, int32_t* assign, float* dist, rvc_stream_t stream);
int64_t rvc_kmeans_lists_work_bytes(int64_t n, int64_t k);
int rvc_kmeans_lists(const int32_t* assign, int64_t n, int64_t k, void* work, int64_t work_bytes, int64_t* list_off,
                     int64_t* ids, int32_t* counts, rvc_stream_t stream);
int rvc_kmeans_update(const float* x, int64_t n, int64_t d, const int64_t* list_off, const int64_t* ids, int64_t k,
                      const float* cent_prev, float* cent_out, rvc_stream_t stream);
int rvc_gather_rows(const float* x, int64_t d, const int64_t* ids, int64_t m, float* out, rvc_stream_t stream);

/* The MiniBatchKMeans reduction of create_index.py:63-76 (sklearn 1.7.2, dense, unit sample weights), one mini-batch
 * step at a time (minibatch.hip); the same contract as above.  xb [n][d] is the batch (rvc_gather_rows of x by the
 * batch's row numbers), cent [k][d], weight_sums f32 [k] sklearn's _counts.  The RandomState, the loop, the choice of
 * the centres to reassign and the stopping rule are host control (rvc_amd/index_train.py).
 *
 * rvc_minibatch_assign: rvc_kmeans_assign with k > n allowed (a batch is smaller than the 10000 centres); the same
 *   kernels, workspace (rvc_kmeans_assign_work_bytes) and results.
 * rvc_minibatch_update: _minibatch_update_dense over the CSR lists rvc_kmeans_lists makes of the batch's assignment.
 *   Per centre with members: row = cent_prev * weight (an f32 product rounded on its own, no fma with the first add),
 *   row += x for the members in batch order, weight += members, row *= 1.f / weight; a centre with no member is copied.
 *   sklearn's arithmetic bit for bit.  weight_sums is updated in place; cent_out != cent_prev.
 * rvc_minibatch_inertia: sum_i ||xb_i - cent[assign_i]||^2 with differences and squares in f64 from the f32 operands,
 *   added in a fixed order (two stages, no atomics) into status->inertia.  The same block receives what the host needs
 *   once per step from weight_sums as it is when this runs: wmax (the largest weight) and any_zero (1 if a weight is
 *   0); weight_sums NULL leaves them 0.  assign values outside [0, k) are clamped.  status: 32 bytes, 8-byte aligned
 *   { double inertia; float wmax; int32_t any_zero; int64_t reserved[2]; }.  work: rvc_minibatch_inertia_work_bytes(n).
 * rvc_minibatch_scatter: the reassignment: cent[dst[i]] = xb[src[i]] and weight_sums[dst[i]] = v for i < m; the dst
 *   are distinct (the caller guarantees it), src may repeat; a dst outside [0, k) is skipped, src is clamped. */
int rvc_minibatch_assign(const float* x, int64_t n, int64_t d, const float* cent, int64_t k, void* work,
                         int64_t work_bytes, int32_t* assign, float* dist, rvc_stream_t stream);
int rvc_minibatch_update(const float* xb, int64_t n, int64_t d, const int64_t* list_off, const int64_t* ids, int64_t k,
                         const float* cent_prev, float* weight_sums, float* cent_out, rvc_stream_t stream);
int64_t rvc_minibatch_status_bytes(void);
int64_t rvc_minibatch_inertia_work_bytes(int64_t n);
int rvc_minibatch_inertia(const float* xb, int64_t n, int64_t d, const float* cent, int64_t k, const int32_t* assign,
                          const float* weight_sums, void* work, int64_t work_bytes, void* status, rvc_stream_t stream);
int rvc_minibatch_scatter(const float* xb, int64_t n, int64_t d, const int64_t* src, const int64_t* dst, int64_t m,
                          float v, float* cent, int64_t k, float* weight_sums, rvc_stream_t stream);

/* ------------------------------------------------------------------ CREPE f0 (VC.get_f0_crepe, convert.py:230-237)
 * crepe_frames: CREPE.py:151-171 framing (1024 @ hop, 512 zero pad) + per-frame zero-mean / unbiased-std
 *   normalisation of frames [frame0, frame0 + nframes) -> out [nframes][1024].
 * bn_maxpool: BatchNorm(eval, alpha/beta precomputed) + MaxPool(2) of y [B][C][L] into strided out.
 * crepe_decode: probs [360][T] sigmoid outputs (masked in place to -inf outside [lo, hi)), softmax,
 *   librosa Viterbi per sequence [seq_off[i], seq_off[i+1]) with log_trans[j][k] = log(A[k][j] + tiny),
 *   bins -> Hz with dither cents [T], periodicity -> f0_raw [T], pd_raw [T].
 * crepe_decode_as: crepe_decode with the power of two of bins -> Hz (10 * 2^((cents + dither) / 1200), f32) named:
 *   RVC_CREPE_HZ_POWF is crepe_decode (the device's powf, within 1 ulp).  RVC_CREPE_HZ_TORCH restates, step for step
 *   in f32 operations and fused multiply-adds, the VECTOR path of torch's CPU pow(2, y) on x86 hosts with FMA (a
 *   1-ulp routine, not the correctly rounded value).  That is the reference's value for every frame torch sends
 *   through whole vector blocks.  torch computes the tail of each call (each batch of 2 * hop_length frames here:
 *   its last n mod 32 frames with 16-lane vectors, n mod 16 with 8-lane ones) with the C library's powf, which
 *   differs in the last bit of about 2 % of values; on those frames, and on hosts without such a vector unit, the
 *   two are 1 ulp apart there.  mangio-crepe-* uses this form: its track does not depend on a host.
 * crepe_smooth_coarse: mean3(f0), median3(pd), f0[pd < 0.1] = 0, then get_f0's shift + coarse mel bins.
 *
 * mangio-crepe-<capacity> (VC.get_f0_mangio_crepe, convert.py:215-228) is the same network behind another framing and
 * decode; it is the CREPE route that reads hop_length.  A host runs, on the f32 signal x [N]:
 *   rvc_abs_quantile, rvc_div_scalar   x / np.quantile(|x|, 0.999) (inside a hybrid the signal was divided once
 *                                      already and is divided again; the extraction twin, extract.py:162-171,
 *                                      divides by torch.quantile: rvc_abs_quantile_as)
 *   rvc_crepe_frames                   hop = hop_length, T = 1 + N / hop_length frames
 *   the network                        as for crepe-<capacity>, in batches of any size (frames are independent)
 *   rvc_crepe_decode_as (HZ_TORCH)     seq_off = 0, 2 hop, 4 hop, ..., T: predict(batch_size = 2 * hop_length)
 *                                      restarts the Viterbi at every batch; dither [T] in frame order; pd_raw unused
 *                                      (no periodicity gate, no mean / median)
 *   rvc_f0_resample_nan                f0_raw [T] -> f64 [p_len]
 *   rvc_pm_post (nf = p_len)           get_f0's autotune / shift / f0 file / quantiser in f64 */
int rvc_crepe_frames(const float* audio, int64_t n, int hop, int64_t frame0, int64_t nframes, float* out,
                     rvc_stream_t stream);
int rvc_bn_maxpool(const float* y, int64_t B, int64_t C, int64_t L, const float* alpha, const float* beta, float* out,
                   int64_t obs, int64_t ocs, int64_t ois, rvc_stream_t stream);
int64_t rvc_crepe_decode_ws_bytes(int64_t T);
int rvc_crepe_decode(float* probs, int64_t T, int lo, int hi, const int64_t* seq_off, int nseq, const double* log_trans,
                     double log_off, double log_p_init, const float* dither, void* ws, int64_t ws_bytes, float* f0_raw,
                     float* pd_raw, rvc_stream_t stream);
enum { RVC_CREPE_HZ_POWF = 0, RVC_CREPE_HZ_TORCH = 1 };
int rvc_crepe_decode_as(float* probs, int64_t T, int lo, int hi, const int64_t* seq_off, int nseq,
                        const double* log_trans, double log_off, double log_p_init, const float* dither, int hz,
                        void* ws, int64_t ws_bytes, float* f0_raw, float* pd_raw, rvc_stream_t stream);
int rvc_crepe_smooth_coarse(const float* f0_raw, const float* pd_raw, int64_t T, float shift, double mel_min,
                            double mel_max, const rvc_f0_post* post, int64_t* coarse, float* pitchf,
                            rvc_stream_t stream);

/* ------------------------------------------------------------------ model-level API
 * A context per device that owns the weights of a voice model and its scratch, so that a non-Python
 * host can run Synthesizer.infer (synthesizers.py:446-465) through this header alone: the folding and
 * packing the Python loader does (rvc_amd/synth.py) and the launch sequence of its infer are native
 * (csrc/rvc_model.cpp), with the same kernels, pass sets and order -- bit-identical to the Python path
 * on the same fp32 weights.
 *   rvc_ctx_create / destroy   one context per HIP device (not re-entrant; calls are stream-ordered).
 *   rvc_ctx_set_precision      the conv engine's arithmetic: RVC_PREC_FP32 (default: 6-pass split-bf16
 *                              mixed with split-fp16 where measured faster), _FP32X6, _FP32SA, _F16X3,
 *                              _BF16X3, _BF16.  RMVPE has its own setting (below).
 *   rvc_ctx_set_rmvpe_precision RMVPE's arithmetic, read by the next rvc_load_rmvpe: RVC_PREC_FP64 (default: the
 *                              network in f64, rmvpe64.hip -- the f0 decisions of the exact model -- with ONE
 *                              exception: the BiGRU recurrence runs in f32 behind the f64 interface (f64 inputs, f64
 *                              output; its decision noise 1.8e-9, profiles/r5_rmvpe_stage_prec.json); all-f64 is
 *                              rvc_bigru64_set_f32(0) or RVC_BIGRU64_F32=0), or a conv precision above for the
 *                              f32 form (_FP32SA: round 3's split-accumulator convs).
 *   rvc_load_synth             params = the .pth "weight" dict (train.py:729-742) as named HOST arrays,
 *                              f32 or f16; weight-norm pairs (x.weight_g / x.weight_v) are folded at load
 *                              (torch._weight_norm, dim 0), already-folded x.weight is taken as is.
 *                              cfg = the .pth "config" list.  Synchronous; replaces a loaded model.
 *   rvc_synth_infer            phone f32 [B][T][E], pitch int64 [B][T], pitchf f32 [B][T] (device);
 *                              sid: HOST int64 [B]; z_noise [B][inter][T] / sine_noise [B][T*upp] device
 *                              or NULL (NULL = device Philox draws from seed + b, as the Python path);
 *                              wav f32 [B][rvc_synth_out_len(ctx, T)] device.  Scratch grows on demand
 *                              (a stream sync when it does); nothing else synchronises. */
typedef struct rvc_ctx rvc_ctx;

enum { RVC_DT_F32 = 0, RVC_DT_F16 = 1, RVC_DT_F64 = 2 };
enum { RVC_PREC_FP32 = 0, RVC_PREC_BF16 = 1, RVC_PREC_BF16X3 = 3, RVC_PREC_FP32X6 = 6, RVC_PREC_FP32SA = 7,
       RVC_PREC_F16X3 = 16, RVC_PREC_FP64 = 64 };

typedef struct rvc_param {
    const char* name;  /* state-dict key, e.g. "dec.ups.0.weight_v" */
    const void* data;  /* host, dense row-major                     */
    int dtype;         /* RVC_DT_F32 / RVC_DT_F16 (RVC_DT_F64: constants) */
    int ndim;
    int64_t shape[4];
} rvc_param;

typedef struct rvc_synth_cfg { /* the checkpoint's "config" list (train.py:729-742) */
    int inter_channels, hidden_channels, filter_channels, n_heads, n_layers, kernel_size;
    int n_resblocks, n_dilations;          /* len(resblock_kernel_sizes), len(resblock_dilation_sizes[0]) */
    int resblock_kernel_sizes[4];
    int resblock_dilation_sizes[4][4];
    int n_upsamples;
    int upsample_rates[8];
    int upsample_kernel_sizes[8];
    int upsample_initial_channel;
    int spk_embed_dim, gin_channels, sr;
} rvc_synth_cfg;

int rvc_ctx_create(int hip_device, rvc_ctx** out);
void rvc_ctx_destroy(rvc_ctx* ctx);
int rvc_ctx_set_precision(rvc_ctx* ctx, int prec);
int rvc_ctx_set_rmvpe_precision(rvc_ctx* ctx, int prec);
int rvc_load_synth(rvc_ctx* ctx, const rvc_param* params, int n, const rvc_synth_cfg* cfg);
int64_t rvc_synth_out_len(const rvc_ctx* ctx, int64_t T);
int rvc_synth_infer(rvc_ctx* ctx, const float* phone, const int64_t* pitch, const float* pitchf, int64_t B, int64_t T,
                    const int64_t* sid, const float* z_noise, const float* sine_noise, uint64_t seed, float* wav,
                    rvc_stream_t stream);

/* ContentVec / HuBERT-base (HubertModel.extract_features, fairseq.py:1459 -> :1412-1431; extractor "default",
 * post-LN).  params = the fairseq .pt "model" dict (floating entries); encoder.pos_conv's weight-norm pair
 * (dim 2) is folded at load.  cfg = the .pt "cfg"/"model" fields below.
 *   rvc_contentvec_forward: wav f32 [B][N] (16 kHz, device) -> feats f32 [B][T][C] time-major like
 *   extract_features' x (T = rvc_contentvec_frames(N)), after out_layer encoder layers (12 for v2, 9 for v1,
 *   convert.py:338); final_proj != 0 applies model.final_proj (convert.py:340) and C = its width. */
typedef struct rvc_contentvec_cfg {
    int encoder_embed_dim, encoder_attention_heads, conv_pos_groups, _pad0;
} rvc_contentvec_cfg;

int rvc_load_contentvec(rvc_ctx* ctx, const rvc_param* params, int n, const rvc_contentvec_cfg* cfg);
int64_t rvc_contentvec_frames(int64_t n16k);
int rvc_contentvec_forward(rvc_ctx* ctx, const float* wav, int64_t B, int64_t N, int out_layer, int final_proj,
                           float* feats, rvc_stream_t stream);

/* RMVPE (E2E(4, 1, (2, 2)), RMVPE.py:183-226 as VC.get_f0_rmvpe uses it, convert.py:248-255).
 * params = the rmvpe.pt state dict; BatchNorm folded at load.  Optional extra params: "mel_basis" f32 [128][513]
 * (librosa.filters.mel(16000, 1024, 128, 30, 8000, htk=True); default: restated natively, rvc_amd/melbasis.py)
 * and "window" f32 [1024] (torch.hann_window(1024); default: computed natively).
 *   rvc_rmvpe_forward: wav f32 [B][N] (device) -> salience f32 [B][360][Tp], Tp = rvc_rmvpe_salience_ld(N)
 *   (frames rounded up to 32); mel -> U-Net -> BiGRU -> Linear + sigmoid.  The first rvc_rmvpe_frames(N)
 *   columns decode with rvc_rmvpe_decode (ld = Tp) into f0 / coarse / pitchf.  Always f32-accurate arithmetic
 *   (the f0 is a per-frame decision, as rvc_amd/rmvpe.py).
 *   rvc_rmvpe_check: synchronises; returns RVC_EHIP (and clears the flag) if a BiGRU hand-off timed out since
 *   the last check (that salience is invalid), else RVC_OK. */
int rvc_load_rmvpe(rvc_ctx* ctx, const rvc_param* params, int n);
int64_t rvc_rmvpe_frames(int64_t n16k);
int64_t rvc_rmvpe_salience_ld(int64_t n16k);
int rvc_rmvpe_forward(rvc_ctx* ctx, const float* wav, int64_t B, int64_t N, float* salience, rvc_stream_t stream);
int rvc_rmvpe_check(rvc_ctx* ctx);

/* CREPE f0 (VC.get_f0_crepe, convert.py:230-237; CREPE.py, any capacity -- taken from the conv shapes).
 * params = the CREPE state dict (conv{1..6}, conv{1..6}_BN, classifier); BatchNorm (eps 1e-3) folded at load
 * in f32 as rvc_amd/crepe.py (or taken from optional "conv{i}_BN.alpha" / ".beta" f32 [C]); optional "log_trans"
 * f64 [360][360] (default: the 12-bin triangular transition matrix's log, computed natively).
 *   rvc_crepe_f0: the padded 16 kHz audio f32 [N] (device) -> coarse int64 [T], pitchf f32 [T],
 *   T = rvc_rmvpe_frames(N): 1024-sample frames at hop 160, the network in 512-frame batches, the librosa
 *   Viterbi per batch with the dither (device f32 cents [T], or NULL = the triangular law drawn on the device
 *   from seed), periodicity smoothing, then get_f0's pitch shift (semitones), `post` and the mel quantiser.
 *   probs (optional, device f32 [360][T]) receives the sigmoid outputs. */
int rvc_load_crepe(rvc_ctx* ctx, const rvc_param* params, int n);

/* VC.pipeline (convert.py:388-458) with inputs and output in device memory: filtfilt + reflect padding by
 * x_pad s; for inputs over x_max s the quiet-point segmentation (convert.py:404-412, rvc_quiet_points -- the
 * one device->host read-back: the segment plan needs the points); f0 over the whole padded input on a side
 * stream (RMVPE thred 0.03, CREPE or pm; pitch shift, then the optional autotune and f0-file override of
 * get_f0, convert.py:304-323); per segment ContentVec (v2: layer 12; v1: layer 9 + final_proj), the optional
 * FAISS retrieval (index_rate, rvc_load_index), phone upsample + protect, Synthesizer.infer with device noise
 * at seed + segment, the x_pad trim at tgt_sr; the optional volume envelope (change_rms, convert.py:449) and
 * the peak normalisation.  Needs ContentVec, the synthesizer and the chosen f0 model loaded on the context;
 * audio f32 [N] 16 kHz (device) -> out f32 (device).  Equal to rvc_amd.pipeline.VC.pipeline_device on the
 * same models, options and seed (tests/test_gpu_native.py).
 *   rvc_vc_out_len: the output length for inputs of one segment (N + 160 <= x_max s); for longer inputs an
 *   upper bound (the quiet points decide the exact length).  rvc_vc_convert_ex writes the exact length to
 *   *out_len; rvc_vc_convert = rvc_vc_convert_ex with default options and one-segment inputs only. */
typedef struct rvc_vc_args {
    int64_t sid;
    double pitch_shift; /* semitones */
    float protect;
    int version;        /* 1 or 2 */
    int x_pad, x_max;   /* Config: 1 and 41 at full precision */
    int tgt_sr, _pad0;
    double index_rate;  /* != 0: FAISS IVF-Flat retrieval + blend (convert.py:349-359), index from rvc_load_index */
    uint64_t seed;
} rvc_vc_args;

/* The retrieval index rvc_vc_convert blends with (a faiss IndexIVFFlat(L2) as create_index.py writes it; read
 * without faiss by rvc_amd.faiss_index): HOST arrays, copied to the device.  centroids [nlist][d]; inverted lists
 * in CSR form: list_off [nlist + 1], codes [ntotal][d] (list-major), ids [ntotal]; big = reconstruct_n(0, ntotal)
 * [ntotal][d]; nprobe as the index stores it.  Validated on the host (d a multiple of 8 up to 1024, ntotal > 0,
 * list_off non-decreasing from 0 to ntotal, every id in [0, ntotal)): a malformed index is a load error.
 * Loading again replaces the index and frees the previous one's device arrays (after a device sync). */
typedef struct rvc_ivf_index {
    int64_t d, nlist, ntotal;
    int nprobe, _pad0;
    const float* centroids;
    const int64_t* list_off;
    const float* codes;
    const int64_t* ids;
    const float* big;
} rvc_ivf_index;

int rvc_load_index(rvc_ctx* ctx, const rvc_ivf_index* index);
/* device memory in use on the current device (hipMemGetInfo total - free), for load / reload accounting */
int64_t rvc_device_bytes_in_use(void);

/* The model-level rvc_vc_convert[_ex] keeps these three f0 methods: swipe, fcpe, fcpe-legacy, mangio-crepe-*,
 * rmvpe-legacy and the hybrids are reached through the op-level entries above (and the Python VC). */
enum { RVC_F0_RMVPE = 0, RVC_F0_CREPE = 1, RVC_F0_PM = 2 };
typedef struct rvc_vc_opts {
    int f0_method;               /* RVC_F0_RMVPE (default), RVC_F0_CREPE (the model of rvc_load_crepe), RVC_F0_PM */
    int f0_autotune;             /* != 0: Autotune.autotune_f0 at f0_autotune_strength (convert.py:311-313) */
    double f0_autotune_strength;
    const float* f0_file;        /* HOST f32 [f0_file_rows][2] "time, f0" rows (read_f0_file, convert.py:425-436) */
    int64_t f0_file_rows;        /*   0 = none; resampled to 100 frames/s as np.interp (convert.py:316-318) */
    double volume_envelope;      /* != 1: change_rms of the output against the filtered input (convert.py:449) */
    const float* crepe_dither;   /* CREPE: device f32 [1 + (N + 2 x_pad 16000) / 160] cents, or NULL = drawn on the
                                    device from seed (the triangular law of CREPE.py:119) */
} rvc_vc_opts;

int64_t rvc_vc_out_len(const rvc_ctx* ctx, int64_t N, const rvc_vc_args* args);
/* the f0-file override values rvc_vc_convert_ex writes from opts.f0_file (host; convert.py:316-318's np.interp of
 * the rows at 100 frames/s): returns their count n and writes min(n, cap) of them to out (HOST f64); -1 on bad
 * input.  Exposed for the parity test against the reference's numpy. */
int64_t rvc_f0_file_resample(const float* rows, int64_t nrows, double* out, int64_t cap);
int rvc_vc_convert(rvc_ctx* ctx, const float* audio, int64_t N, const rvc_vc_args* args, float* out,
                   rvc_stream_t stream);
int rvc_vc_convert_ex(rvc_ctx* ctx, const float* audio, int64_t N, const rvc_vc_args* args, const rvc_vc_opts* opts,
                      float* out, int64_t out_cap, int64_t* out_len, rvc_stream_t stream);
int rvc_crepe_f0(rvc_ctx* ctx, const float* audio, int64_t N, const float* dither, uint64_t seed, double pitch_shift,
                 const rvc_f0_post* post, float* probs, int64_t* coarse, float* pitchf, rvc_stream_t stream);

/* ------------------------------------------------------------------ dataset preprocessing
 * PreProcess.process_audio (main/inference/preprocess.py:129-185) in f64 (preprocess.hip).  No entry synchronises
 * or allocates; x_is_f64 selects f64 (!= 0) or f32 input samples; every pointer is device memory unless it says HOST.
 *
 * lfilter64: scipy.signal.lfilter(b, a, x) for order 5 from a zero state (preprocess.py:160): x [N] -> y f64 [N].
 *   b[6], a[6] are HOST arrays (normalised by a[0] as scipy does).  The signal is cut into RVC_LFILTER_CHUNK-sample
 *   chunks, one per lane (RVC_LFILTER_WAVE samples per 64-lane block); a lane rebuilds its entry state by running
 *   the recurrence over the `warm` samples before its chunk, staged in tiles of RVC_LFILTER_TILE samples.
 *   warm = rvc_lfilter64_warmup(b, a): the first multiple of the tile past the last sample whose |impulse response|
 *   is >= 1e-12, or -1 for a filter that needs more than RVC_LFILTER_WARM_CAP (rvc_lfilter64 rejects those).
 *   work: rvc_lfilter64_work_bytes(N, warm) bytes of scratch (0 today, NULL is accepted then; -1 on bad arguments).
 * frame_rms64: get_rms (preprocess.py:119-127): constant padding of frame / 2 each side, frames of `frame` samples
 *   every `hop`, sqrt(mean(x^2)) summed in f64 in a fixed order -> out f64 [rvc_frame_rms64_len(N, frame, hop)]
 *   (= 1 + N / hop for an even frame).
 * peak_mix64: _normalize_audio (preprocess.py:142-145): *peak = max|x| (exact; a NaN sample gives NaN), then
 *   y = (x / *peak * gain) + rest * x with numpy's roundings (y may be x).  The caller reads *peak back and takes the
 *   reference's `> 2.5` decision.
 * resample_poly64: scipy.signal.resample_poly(x, up, down) (padtype "constant") of nseg chunks in one launch.
 *   h f64 [h_len]: firwin(2 * 10 * max(up, down) + 1, 1 / max(up, down), window=("kaiser", 5.0)) * up behind
 *   scipy's n_pre_pad zeros; n_pre_remove as scipy computes it.  seg int64 [nseg][4] = (in_offset, in_len, out_offset,
 *   out_len), out_len = ceil(in_len * up / down), given twice with the same contents: seg_host (HOST, validated
 *   against n_in / n_out before the launch) and seg_dev (device, read by the kernel).  Every chunk sees zeros outside
 *   its own samples.  y64 f64 [n_out] and y32 = the same values cast to f32. */
enum {
    RVC_LFILTER_CHUNK = 512,        /* output samples per lane */
    RVC_LFILTER_WAVE = 64 * 512,    /* output samples per block (one wave) */
    RVC_LFILTER_TILE = 32,          /* samples per staged tile; warm is a multiple of it */
    RVC_LFILTER_WARM_CAP = 16384    /* longest supported warm-up */
};
int64_t rvc_lfilter64_warmup(const double* b, const double* a);
int64_t rvc_lfilter64_work_bytes(int64_t N, int64_t warm);
int rvc_lfilter64(const void* x, int x_is_f64, int64_t N, const double* b, const double* a, int64_t warm, void* work,
                  int64_t work_bytes, double* y, rvc_stream_t stream);
int64_t rvc_frame_rms64_len(int64_t N, int64_t frame, int64_t hop);
int rvc_frame_rms64(const void* x, int x_is_f64, int64_t N, int64_t frame, int64_t hop, double* out,
                    rvc_stream_t stream);
int rvc_peak_mix64(const double* x, int64_t N, double gain, double rest, double* peak, double* y,
                   rvc_stream_t stream);
int rvc_resample_poly64(const void* x, int x_is_f64, int64_t n_in, const double* h, int64_t h_len, int up, int down,
                        int64_t n_pre_remove, const int64_t* seg_host, const int64_t* seg_dev, int64_t nseg,
                        double* y64, float* y32, int64_t n_out, rvc_stream_t stream);

/* ------------------------------------------------------------------ training forward and losses
 * The pieces of the training step's forward (main/inference/train.py:843-866) that the inference path lacks
 * (trainfwd.hip); the posterior encoder, the flow forward and the decoder are rvc_conv1d launches.  No entry
 * synchronises or allocates; every pointer is device memory.
 *
 * spectrogram: spectrogram_torch (train.py:700-706): B signals x [B][N], reflect-padded by (n_fft - hop) / 2 on both
 *   sides (which must be < N, and n_fft - hop even), framed every hop with center=False, times win f32 [n_fft] (the
 *   reference's torch.hann_window(n_fft): win_size == n_fft), an f64 FFT -> spec [B][n_fft / 2 + 1][F] = sqrt(re^2 + im^2 + 1e-6) rounded to f32 once.
 *   n_fft 1024 or 2048; F = rvc_spectrogram_frames(N, n_fft, hop) (-1: N too short or bad sizes).
 * mel_log: spec_to_mel_torch (train.py:708-713): mel [B][M][F] = log(max(basis [M][K] @ spec [B][K][F], 1e-5)), one
 *   launch, the products summed over k in order in f64 and rounded once after the log.
 * slice_l1: F.l1_loss(slice_segments(mel, ids, S), yhat_mel) (train.py:845, :865): the mean over [B][M][S] of
 *   |mel [B][M][T] at frames ids[b] + s  -  yhat_mel [B][M][S]|; ids int64 [B] on the device; a start outside
 *   [0, T - S] reads nothing and gives NaN.
 * kl_loss: kl_loss (train.py:317-325) at an all-ones mask over z_p, logs_q, m_p, logs_p [B][C][T]: the sum divided
 *   by B * T.  q_bstride is the batch stride of logs_q, p_bstride that of m_p and logs_p (0: C * T), so the halves
 *   of stacked [m; logs] statistics pass without a copy.
 * Both losses: a fixed two-stage sum (RVC_TRAINFWD_RED_BLOCKS partials, then one wave), f64 accumulators, one f32
 *   result in out[0], no atomics -- bit-identical from run to run.  work: rvc_trainfwd_work_bytes() bytes. */
enum { RVC_TRAINFWD_RED_BLOCKS = 64 };
int64_t rvc_spectrogram_frames(int64_t N, int nfft, int hop);
int rvc_spectrogram(const float* x, const float* win, float* spec, int64_t B, int64_t N, int64_t F, int nfft,
                    int hop, rvc_stream_t stream);
int rvc_mel_log(const float* spec, const float* basis, float* mel, int64_t B, int64_t M, int64_t K, int64_t F,
                rvc_stream_t stream);
int64_t rvc_trainfwd_work_bytes(void);
int rvc_slice_l1(const float* mel, const int64_t* ids, const float* yhat_mel, int64_t B, int64_t M, int64_t T, int64_t S,
                 void* work, int64_t work_bytes, float* out, rvc_stream_t stream);
int rvc_kl_loss(const float* z_p, const float* logs_q, const float* m_p, const float* logs_p, int64_t B, int64_t C,
                int64_t T, int64_t q_bstride, int64_t p_bstride, void* work, int64_t work_bytes, float* out,
                rvc_stream_t stream);

/* ---- the discriminators' own kernels and the GAN losses (csrc/discriminator.hip; train.py:608-674, 286-315)
 * period_front: DiscriminatorP.forward up to its first feature map, for S signals y [S][t]: the right reflect pad
 *   (p - t % p) % p (which must be < t), the [H][p] view, Conv2d(1, 32, (5,1), (3,1), padding=(2,0)) with w [32][5] and
 *   bias [32], LeakyReLU(slope) -> out [S * p][32][H1]: column c of signal s is batch element s * p + c, so every later
 *   (k,1) Conv2d is a batched Conv1d over H.  H1 = rvc_period_front_rows(t, p) (-1: the pad does not fit).
 * gconv_small: Conv1d(Ci, Co, 41, 4, groups = Ci / 4, padding = 20) + bias + LeakyReLU(slope) as a direct f32 kernel:
 *   x [B][Ci][Lin], w [Co][4][41], y [B][Co][Lout], Lout = (Lin - 1) / 4 + 1; Co / groups is 16 or 4.
 * pair_l1: table[slot] = mean |a[i] - b[i]| over n values.  lsgan_terms: table[slot .. slot + 2] = mean (1 - d_r)^2,
 *   mean d_g^2, mean (1 - d_g)^2 over n values each.  Both are the fixed two-stage f64 sum of slice_l1, kept in f64;
 *   work: rvc_disc_work_bytes() bytes, reused by calls on one stream.
 * disc_finish: table = n_fm feature-map terms in the reference's list order, then (r, g, gen) per discriminator
 *   (rvc_disc_table_slots(n_fm, n_disc) doubles).  Each term is rounded to f32 and added in f32 in list order, as the
 *   reference's Python sums do: out[0] = loss_disc, [1] = loss_gen, [2] = loss_fm = 2 * sum, and -- with the device
 *   scalars l1 and kl (rvc_slice_l1 / rvc_kl_loss; both or neither) -- [4] = loss_mel = l1 * c_mel, [5] = loss_kl =
 *   kl * c_kl, [3] = loss_gen_all = loss_gen + loss_fm + loss_mel + loss_kl (NaN without them); from
 *   out[RVC_DISC_OUT_LISTS]: losses_gen [n_disc], losses_disc_r [n_disc], losses_disc_g [n_disc]. */
enum { RVC_DISC_OUT_LISTS = 6 };
int64_t rvc_period_front_rows(int64_t t, int p);
int rvc_period_front(const float* y, const float* w, const float* bias, float* out, int64_t S, int64_t t, int p,
                     int64_t H1, float slope, rvc_stream_t stream);
int rvc_gconv_small(const float* x, const float* w, const float* bias, float* y, int64_t B, int64_t Ci, int64_t Co,
                    int64_t Lin, int64_t Lout, float slope, rvc_stream_t stream);
int64_t rvc_disc_work_bytes(void);
int64_t rvc_disc_table_slots(int n_fm, int n_disc);
int rvc_pair_l1(const float* a, const float* b, int64_t n, double* table, int64_t slot, void* work, int64_t work_bytes,
                rvc_stream_t stream);
int rvc_lsgan_terms(const float* d_r, const float* d_g, int64_t n, double* table, int64_t slot, void* work,
                    int64_t work_bytes, rvc_stream_t stream);
int rvc_disc_finish(const double* table, int n_fm, int n_disc, const float* l1, float c_mel, const float* kl, float c_kl,
                    float* out, rvc_stream_t stream);

/* The discriminator's training step (train.py:851-860) behind that forward (csrc/disc_backward.hip).  Convolutions are
 * exact f32 FMA / MFMA chains in a fixed order, every reduction is fixed-order: two runs give the same bits.
 * lsgan_grad: d [2 n], a discriminator's conv_post map, real half first -> dy [2 n], the gradient of
 *   discriminator_loss times scale: -2 (1 - d_r) / n and 2 d_g / n.
 * dyp below is dy * (y > 0 ? 1 : slope) with y the stored forward output of the layer that produced dy (a LeakyReLU
 *   output has its input's sign; 0 takes the slope); y = NULL: no activation (conv_post).
 * conv_bwd_data: dx[b][ci][i] = sum_co sum_k w[co][ci][k] dyp[b][co][j], i = j stride + k - pad, for Conv1d weights
 *   w [Co][Ci / groups][K]; every row i < Lin is written.  groups = 1 with Ci >= 16 runs on v_mfma_f32_16x16x4_f32
 *   per stride phase, anything else directly.
 * conv_bwd_weight: dW[co][ci][k] (+)= scale sum_b sum_j dyp[b][co][j] x[b][ci][j stride + k - pad] and
 *   db[co] (+)= scale sum_b sum_j dyp[b][co][j]; accumulate != 0 adds to what dW and db hold.  The sum over (b, j) is
 *   split into chunks whose partials go to work (rvc_conv_bwd_weight_work_bytes asks for what it would like; any
 *   buffer that holds dW once is enough) and are added in order.  period > 0: x is the signals [B / period][t] read as
 *   DiscriminatorP's first conv reads them (rvc_period_front's reflected index and [Lin][period] view; Ci = 1).
 * wn_adamw: one conv's rows.  From dW [Co][n], v [Co][n], g [Co]: dg = <dW, v> / |v|, dv = g / |v| (dW - v dg / |v|)
 *   (the backward of torch._weight_norm(v, g, 0)); table[3 row + 0..2] = |dg|^2, |dv|^2, |db|^2 of the row; then
 *   torch.optim.AdamW's update (amsgrad off) of g, v and bias with their exp_avg (m_*) and exp_avg_sq (s_*) in place,
 *   step counting from 1.  f64 arithmetic on the f32 values, every stored value rounded once.
 * grad_norm: out[0] = sqrt(sum of table[0 .. n)), clip_grad_value(parameters, None)'s return; work: RED_BLOCKS doubles
 *   (rvc_disc_work_bytes() is enough). */
int rvc_lsgan_grad(const float* d, float* dy, int64_t n, float scale, rvc_stream_t stream);
int rvc_conv_bwd_data(const float* dy, const float* y, const float* w, float* dx, int64_t B, int64_t Ci, int64_t Co,
                      int64_t Lin, int64_t Lout, int K, int stride, int pad, int groups, float slope,
                      rvc_stream_t stream);
int64_t rvc_conv_bwd_weight_work_bytes(int64_t B, int64_t Ci, int64_t Co, int64_t Lout, int K, int groups);
int rvc_conv_bwd_weight(const float* dy, const float* y, const float* x, float* dW, float* db, int64_t B, int64_t Ci,
                        int64_t Co, int64_t Lin, int64_t Lout, int K, int stride, int pad, int groups, float slope,
                        float scale, int accumulate, int period, int64_t t, void* work, int64_t work_bytes,
                        rvc_stream_t stream);
int rvc_wn_adamw(const float* dW, const float* db, float* v, float* g, float* bias, float* m_v, float* s_v, float* m_g,
                 float* s_g, float* m_b, float* s_b, int64_t Co, int64_t n, double lr, double beta1, double beta2,
                 double eps, double weight_decay, int64_t step, double* table, rvc_stream_t stream);
int rvc_grad_norm(const double* table, int64_t n, double* out, void* work, int64_t work_bytes, rvc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RVC_AMD_H */

"""Tensor-level wrappers over the C ABI (torch tensors are only device buffers + streams here).

Every function checks shapes on the host before launching (a kernel that reads out
of bounds can reset the GPU), passes raw pointers, and raises on a non-zero status.
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import ACT_GELU, ACT_LOGCLAMP, ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, check  # noqa: F401


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    if not t.is_cuda or t.dtype not in (torch.float32, torch.int64, torch.int32, torch.uint8):  # uint8: table blobs
        raise TypeError(f"rvc_amd: expected a CUDA f32/int tensor, got {t.dtype} on {t.device}")
    return ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------ weight packing (host, load time)
def pack_km(w: torch.Tensor, groups: int = 1) -> torch.Tensor:
    """Conv weight [Co, Ci/g, K] -> KM layout [g][Ci/g*K][Co/g] (k = c*K + tap, m contiguous)."""
    Co, Cig, K = w.shape
    Cog = Co // groups
    return w.reshape(groups, Cog, Cig, K).permute(0, 2, 3, 1).reshape(groups, Cig * K, Cog).contiguous()


def pack_convT(w: torch.Tensor, u: int) -> tuple[torch.Tensor, int]:
    """ConvTranspose1d weight [Ci, Co, K] (stride u) -> polyphase KM [u][Ci*T][Co], T = ceil(K/u).

    Phase r computes outputs t with (t + pad) % u == r as a stride-1 conv over x with taps
    tp in [0, T): x[q - (T-1) + tp] * W[ci][co][r + (T-1-tp)*u]  (zero where that tap >= K)."""
    Ci, Co, K = w.shape
    T = -(-K // u)
    out = torch.zeros(u, Ci, T, Co, dtype=w.dtype)
    for r in range(u):
        for tp in range(T):
            j = r + (T - 1 - tp) * u
            if j < K:
                out[r, :, tp, :] = w[:, :, j]
    return out.reshape(u, Ci * T, Co).contiguous(), T


# Split-bf16 engine switch (the f32-MFMA engine runs when off); RVC_AMD_X6=0 disables it.
X6 = os.environ.get("RVC_AMD_X6", "1") != "0"

# Arithmetic of the split-operand MFMA engine (f32 accumulation always):
#   "fp32"   f32-equivalent (the default; BASELINE configs 1-2, 4): "fp32x6" everywhere except the convs where
#            "f16x3" measured faster (conv_passes, rb_passes; F16_MIX; RVC_AMD_F16MIX=0 turns it off)
#   "fp32x6" 6 bf16 passes, f32-accurate products (~2^-22 relative per product)
#   "fp32sa" "fp32x6" with the 5 correction passes accumulated apart from hH (RMVPE, whose f0 is a per-frame
#            decision: the large sum is rounded once per 32 products, scripts/conv_prec.py)
#   "f16x3"  3 fp16 passes over power-of-2-scaled 22-bit operands (~2^-20 relative per product)
#   "bf16x3" 3 bf16 passes, 16-bit operand mantissas (~2^-16 relative per product)
#   "bf16"   1 pass, bf16 operands (BASELINE configs 3 and 5)
F16X3 = 16  # RVC_ARITH_F16X3
PASSES = {"fp32": 6, "fp32x6": 6, "fp32sa": 7, "f16x3": F16X3, "bf16x3": 3, "bf16": 1}
F16_MIX = os.environ.get("RVC_AMD_F16MIX", "1") != "0"
# with the producer's |max| (amax side channel), split-fp16 for every stride-1 1-D conv (RVC_AMD_AMAX_F16ALL=0: only
# where conv_passes picks it anyway; the cell then just replaces the per-tile pre-pass)
AMAX_F16ALL = os.environ.get("RVC_AMD_AMAX_F16ALL", "1") != "0"
AMAX_SHARDS = 64  # RVC_AMAX_SHARDS: u32 words per |max| cell
# round 6: the stride-2 convs with a producer's |max| (ContentVec's feature extractor) in split-fp16 too
# (RVC_AMD_AMAX_S2=0: 6-pass split-bf16 there, the round-5 form; rvc_model_common's conv_passes reads the same switch)
AMAX_S2 = os.environ.get("RVC_AMD_AMAX_S2", "1") != "0"


def conv_passes(K, Ci, stride=1, two_d=False, amax=False):
    """The pass set a conv launch runs at under the current precision (see PASSES): in "fp32", split-fp16
    where it measured faster than 6-pass split-bf16 (scripts/conv_bench.py, same box: k >= 7 up to 256
    input channels, and k = 3 at 64-128 channels; 6-pass at k = 3 over 256 or 32 channels) -- and every stride-1
    1-D conv whose input's |max| comes from its producer (``amax``: no per-tile pre-pass, which is what made the
    short-tap and wide convs slower in split-fp16)."""
    if _PRECISION == "fp32" and F16_MIX and not two_d and \
            ((stride == 1 and ((amax and AMAX_F16ALL) or (K >= 7 and Ci <= 256) or (K >= 3 and 64 <= Ci <= 128))) or
             (stride == 2 and amax and AMAX_F16ALL and AMAX_S2)):
        return F16X3
    return PASSES[_PRECISION]
_PRECISION = os.environ.get("RVC_AMD_PRECISION", "fp32")
if _PRECISION not in PASSES:
    raise ValueError(f"RVC_AMD_PRECISION must be one of {sorted(PASSES)}")


def get_precision() -> str:
    return _PRECISION


def set_precision(name: str) -> str:
    """Set the conv engine's arithmetic for subsequent launches; returns the previous setting."""
    global _PRECISION
    if name not in PASSES:
        raise ValueError(f"precision must be one of {sorted(PASSES)}, got {name!r}")
    prev, _PRECISION = _PRECISION, name
    return prev


class splitk_target:
    """Context manager: the conv engine's split-K target grid for the launches issued inside (tiles below which a
    conv's k range is split over blocks; 0 = never split, None = leave the current setting)."""

    def __init__(self, target):
        self.target = target

    def __enter__(self):
        if self.target is not None:
            self.prev = _lib.load().rvc_conv1d_set_splitk_target(int(self.target))
        return self

    def __exit__(self, *a):
        if self.target is not None:
            _lib.load().rvc_conv1d_set_splitk_target(self.prev)


class precision:
    """Context manager: ``with ops.precision("bf16"): ...``."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.prev = set_precision(self.name)
        return self

    def __exit__(self, *a):
        set_precision(self.prev)


class SplitImages:
    """The two operand images of one weight for the split-operand engine: ``bf`` (rvc_conv1d_pack_x6, the
    bf16 planes every bf16 pass count reads) and ``hf`` (rvc_conv1d_pack_f16, fp16 planes + row scales)."""

    def __init__(self, bf, hf):
        self.bf, self.hf = bf, hf

    def for_passes(self, passes):
        return self.hf if passes == F16X3 else self.bf

    def data_ptr(self, passes=None):
        return self.for_passes(PASSES[_PRECISION] if passes is None else passes).data_ptr()


def pack_x6(w_km: torch.Tensor, nphase: int, Ci: int, K: int, Co: int):
    """Device KM weights [nphase][Ci*K][Co] -> (SplitImages, nmf): the split-bf16 image
    (rvc_conv1d_pack_x6) and the split-fp16 image (rvc_conv1d_pack_f16) for the split-operand engine, or
    (None, 0) when the engine is off."""
    if not X6:
        return None, 0
    lib = _lib.load()
    imgs = []
    for size_fn, pack_fn in ((lib.rvc_conv1d_x6_bytes, lib.rvc_conv1d_pack_x6),
                             (lib.rvc_conv1d_f16_bytes, lib.rvc_conv1d_pack_f16)):
        nbytes = size_fn(nphase, Ci, K, Co)
        if nbytes <= 0:
            raise ValueError("pack_x6: bad shape")
        out = torch.empty(nbytes, dtype=torch.uint8, device=w_km.device)
        nmf = ctypes.c_int(0)
        check(pack_fn(_p(w_km), nphase, Ci, K, Co, ctypes.c_void_p(out.data_ptr()), ctypes.byref(nmf), _stream()),
              "conv1d_pack")
        imgs.append(out)
    return SplitImages(*imgs), nmf.value


class Conv:
    """A packed Conv1d (weight [Co, Ci/g, K], bias [Co]) resident on the device, with the split-operand images
    (pack_x6) the library's engine reads."""

    def __init__(self, w, b=None, groups=1, device="cuda"):
        self.Co, self.Cig, self.K = (int(s) for s in w.shape)
        self.groups = groups
        self.Ci = self.Cig * groups
        self.w = pack_km(w.float(), groups).to(device)
        self.b = b.float().to(device) if b is not None else None
        # the split-operand engine takes ungrouped convs with <= 64 taps (X6_K_MAX / x6_eligible in conv1d.hip;
        # CREPE's k=64 layers are the widest) and grouped ones with <= 128 (ContentVec's pos_conv), whose image holds
        # the groups as phases (ConvParams.gx6)
        if groups == 1 and self.K <= 64:
            self.wx, self.wx_nmf = pack_x6(self.w, 1, self.Ci, self.K, self.Co)
        elif groups > 1 and self.K <= 128:
            self.wx, self.wx_nmf = pack_x6(self.w, groups, self.Cig, self.K, self.Co // groups)
        else:
            self.wx, self.wx_nmf = None, 0

    def __call__(self, x, Lout=None, stride=1, pad=0, dil=1, **kw):
        return conv1d(x, self.w, self.Ci, self.Co, self.K, bias=self.b, stride=stride, pad=pad, dil=dil,
                      groups=self.groups, Lout=Lout, wx=self.wx, wx_nmf=self.wx_nmf, **kw)


class ConvT:
    """ConvTranspose1d(Ci, Co, K, stride u, padding p, output_padding 0) as u phase convs."""

    def __init__(self, w, b, u, pad, device="cuda"):
        self.Ci, self.Co, self.K = (int(s) for s in w.shape)
        self.u, self.pad = u, pad
        wp, self.T = pack_convT(w.float(), u)
        self.w = wp.to(device)
        self.b = b.float().to(device)
        self.wx, self.wx_nmf = pack_x6(self.w, u, self.Ci, self.T, self.Co)

    def out_len(self, Lin):
        return (Lin - 1) * self.u - 2 * self.pad + self.K

    def __call__(self, x, out=None, **kw):
        B, Ci, Lin = _shape3(x)
        Lout = self.out_len(Lin)
        ncols = (Lout - 1 + self.pad) // self.u + 1
        return conv1d(x, self.w, Ci, self.Co, self.T, bias=self.b, stride=1, pad=self.T - 1, dil=1, Lout=Lout,
                      ncols=ncols, nphase=self.u, ostride=self.u, ooffset=-self.pad, out=out,
                      flops=2.0 * B * Ci * self.Co * self.K * Lin, wx=self.wx, wx_nmf=self.wx_nmf, **kw)


class AmaxSlots:
    """n |max| cells (the conv engine's amax side channel, AMAX_SHARDS words each) for one pass of B batch elements,
    zeroed by one launch: ``s[k]`` is cell k -- B consecutive cells, one per batch element (element b's |max| at word
    b * AMAX_SHARDS: a clip's split-fp16 scale never depends on the other clips of its batch) -- handed to a producer
    as ``amax_out`` and to its consumers as ``amax_in``."""

    def __init__(self, n, device, B=1):
        self.B = B
        self.words = torch.zeros(n * B * AMAX_SHARDS, dtype=torch.int32, device=device)

    def __getitem__(self, k):
        w = self.B * AMAX_SHARDS
        return self.words[k * w:(k + 1) * w]


def amax_value(cell, b=0):
    """The |max| a cell holds for batch element b (the largest of its words, read back as f32)."""
    import numpy as np
    words = cell[b * AMAX_SHARDS:(b + 1) * AMAX_SHARDS].cpu().numpy().astype(np.int32)
    return float(words.view(np.float32).max())


LAST_CONV_FLOPS = 0.0
LAST_CONV_ENGINE = 0  # 0 = f32 MFMA engine, 1 = split-bf16 (x6) engine
LAST_CONV_PASSES = 0  # the split-operand launch's pass set (PASSES values; F16X3 = split-fp16), 0 = f32 engine
LAST_CONV_WS = 0  # its split-K workspace bytes (0 = not split)
_LAST_CONV_ARGS = None  # its argument block, for last_conv_tile()
_WS = {}
_WS_PRIVATE = None  # a workspace store owned by a captured graph (private_workspaces)


def last_conv_tile():
    """The (rows, columns) output tile the last conv1d launch's blocks computed (rvc_conv1d_tile: the plan for its
    arguments under the current switches; asked on demand, so a launch pays nothing for it)."""
    if _LAST_CONV_ARGS is None:
        return 0, 0
    return divmod(_lib.load().rvc_conv1d_tile(ctypes.byref(_LAST_CONV_ARGS)), 1 << 16)


class private_workspaces:
    """``with ops.private_workspaces(store):`` -- split-K / split-KV / decode scratch comes from ``store``
    (a dict the caller keeps) instead of the shared per-stream pool.  A captured graph bakes the raw
    workspace pointers into its kernel nodes, so it must own them: buffers in a private store are never
    freed while the store lives (a grown buffer's predecessor is retired into the store, not released),
    and no eager launch or other graph draws from it (graph.ClipGraph)."""

    def __init__(self, store: dict):
        self.store = store

    def __enter__(self):
        global _WS_PRIVATE
        self.prev, _WS_PRIVATE = _WS_PRIVATE, self.store
        return self.store

    def __exit__(self, *a):
        global _WS_PRIVATE
        _WS_PRIVATE = self.prev


def _workspace(device, nbytes, kind="conv"):
    """Split-K / split-KV scratch per (device, stream), grown on demand: reuse is stream-ordered, and
    work running concurrently on another stream (VC's side stream) gets its own buffer."""
    key = f"{device}/{kind}/{torch.cuda.current_stream(device).stream_id}"
    pool = _WS if _WS_PRIVATE is None else _WS_PRIVATE
    buf = pool.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        if buf is not None and _WS_PRIVATE is not None:
            pool.setdefault("_retired", []).append(buf)  # a captured node may still point at it
        buf = torch.empty((nbytes + 3) // 4 + (1 << 20), dtype=torch.float32, device=device)
        pool[key] = buf
    return buf


def _room(t):
    """Elements addressable from t.data_ptr() to the end of its storage (views of batched buffers are
    strided: their numel understates what a kernel with batch strides may touch)."""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


def _shape3(x):
    if x.dim() == 2:
        return 1, x.shape[0], x.shape[1]
    return x.shape[0], x.shape[1], x.shape[2]


def conv1d(x, w, Ci, Co, K, *, bias=None, bias2=None, stride=1, pad=0, dil=1, groups=1, Lout=None, ncols=0,
           nphase=1, ostride=1, ooffset=0, out=None, res=None, in_act=ACT_NONE, in_slope=0.0, in_scale=1.0,
           out_act=ACT_NONE, out_slope=0.0, out_scale=1.0, accumulate=False, B=None, Lin=None, x_bstride=0,
           w_bstride=0, y_bstride=0, res_bstride=0, toff=None, wrap=0, flops=None, wx=None, wx_nmf=0,
           amax_in=None, amax_out=None, src=None):
    """y = conv(pre(x)) with fused epilogue.  x: [B][Ci][Lin] device f32 (t contiguous).

    ``amax_out`` / ``amax_in``: cells of the |max| side channel (``AmaxSlots``: AMAX_SHARDS words per batch element)
    -- the launch folds max |y| into ``amax_out`` (zeroed beforehand), and a split-fp16 launch takes its activation
    scale from ``amax_in`` (the producer's cell for x) instead of a per-tile pre-pass (include/rvc_amd.h).

    ``src`` = (conv, signal [B][N], stride, pad): the fused source conv -- every stored output also adds
    ``conv(signal)[m][t]`` of a 1-input-channel ``ops.Conv`` (the NSF generator's noise_convs, synthesizers.py:156),
    the same bits as that conv run separately with ``accumulate`` (rvc_conv1d_args.src_*).

    ``flops`` is the launch's ALGORITHMIC FLOP count for roofline accounting (recorded in
    LAST_CONV_FLOPS); the default is 2*B*Co*(Ci/g)*K*(valid outputs)."""
    global LAST_CONV_FLOPS, LAST_CONV_ENGINE, LAST_CONV_PASSES, LAST_CONV_WS, _LAST_CONV_ARGS
    if B is None:
        B, Cx, Lx = _shape3(x)
        if Lin is None:
            Lin = Lx
        if Cx != Ci:
            raise ValueError(f"conv1d: x has {Cx} channels, weight expects {Ci}")
        if not x.is_contiguous():
            raise ValueError("conv1d: x must be contiguous")
    if Lout is None:
        Lout = (Lin + 2 * pad - dil * (K - 1) - 1) // stride + 1
    if Lout <= 0:
        raise ValueError("conv1d: empty output")
    Cig = Ci // groups
    need_w = nphase * Cig * K * Co
    if w.numel() < need_w or (w_bstride and w.numel() < need_w + (B - 1) * w_bstride):
        raise ValueError("conv1d: packed weight too small")
    if out is None:
        out = torch.empty(B, Co, Lout, device=x.device, dtype=torch.float32) if B > 1 else \
            torch.empty(Co, Lout, device=x.device, dtype=torch.float32)
    elif _room(out) < (B - 1) * (y_bstride or Co * Lout) + Co * Lout:
        raise ValueError("conv1d: output buffer too small")
    if res is not None and _room(res) < (B - 1) * (res_bstride or Co * Lout) + Co * Lout:
        raise ValueError("conv1d: residual too small")
    if _room(x) < (B - 1) * (x_bstride or Ci * Lin) + Ci * Lin:
        raise ValueError("conv1d: input buffer too small")
    if bias is not None and bias.numel() < Co:
        raise ValueError("conv1d: bias too small")
    a = _lib.Conv1dArgs()
    a.x, a.w, a.bias, a.bias2, a.res, a.y = _p(x), _p(w), _p(bias), _p(bias2), _p(res), _p(out)
    a.B, a.Ci, a.Co, a.Lin, a.Lout, a.ncols = B, Ci, Co, Lin, Lout, ncols
    a.x_bstride, a.y_bstride, a.res_bstride, a.w_bstride = x_bstride, y_bstride, res_bstride, w_bstride
    a.K, a.stride, a.dil, a.pad, a.groups = K, stride, dil, pad, groups
    a.nphase, a.ostride, a.ooffset = nphase, ostride, ooffset
    a.in_act, a.out_act, a.accumulate = in_act, out_act, int(bool(accumulate))
    a.in_scale, a.in_slope, a.out_slope, a.out_scale = in_scale, in_slope, out_slope, out_scale
    if toff is not None:
        if len(toff) != K or K > 16:
            raise ValueError("conv1d: toff must have K <= 16 entries")
        a.ntoff = K
        for i, v in enumerate(toff):
            a.toff[i] = int(v)
    a.wrap = wrap
    a.amax_in, a.amax_out = _p(amax_in), _p(amax_out)
    for cell in (amax_in, amax_out):
        if cell is not None and cell.numel() < B * AMAX_SHARDS:
            raise ValueError(f"conv1d: a |max| cell needs {AMAX_SHARDS} words per batch element (B={B})")
    if src is not None:
        sconv, sig, s_stride, s_pad = src
        if sconv.Ci != 1 or sconv.groups != 1 or sconv.Co != Co:
            raise ValueError("conv1d: src needs a 1-input-channel conv with the output's channels")
        s_len = sig.shape[-1]
        if sig.dim() not in (1, 2) or (sig.dim() == 2 and sig.shape[0] != B) or not sig.is_contiguous() or \
                (sig.dim() == 1 and B != 1):
            raise ValueError("conv1d: src signal must be contiguous [B][N]")
        a.src_x, a.src_w, a.src_b = _p(sig), _p(sconv.w), _p(sconv.b)
        a.src_K, a.src_stride, a.src_pad, a.src_len, a.src_bstride = sconv.K, s_stride, s_pad, s_len, s_len
    if wx is not None:
        passes = conv_passes(K, Ci // groups, stride, toff is not None, amax_in is not None)
        a.wx, a.wx_nmf, a.wx_passes = ctypes.c_void_p(wx.data_ptr(passes)), wx_nmf, passes
    if flops is None:
        valid = (Lout // wrap - 2) * (wrap - 2) if wrap else (ncols or Lout) * nphase
        flops = 2.0 * B * Co * Cig * K * min(valid, Lout)
    LAST_CONV_FLOPS = flops
    lib = _lib.load()
    need = lib.rvc_conv1d_workspace_bytes(ctypes.byref(a))
    if need < 0:
        raise RuntimeError(f"rvc_amd: conv1d plan failed: {lib.rvc_last_error().decode()}")
    ws = _workspace(out.device, need) if need else None
    LAST_CONV_WS = need
    LAST_CONV_ENGINE = lib.rvc_conv1d_engine(ctypes.byref(a))
    LAST_CONV_PASSES = a.wx_passes if LAST_CONV_ENGINE == 1 else 0
    _LAST_CONV_ARGS = a
    check(lib.rvc_conv1d(ctypes.byref(a), _p(ws), need, _stream()), "conv1d")
    return out


# Fused ResBlock pairs for the 32/64-channel generator stages (RVC_AMD_FUSED_RB=0: two conv launches each)
FUSED_RB = os.environ.get("RVC_AMD_FUSED_RB", "1") != "0"
RB_PASSES = (6, 3, 1, F16X3)  # pass sets the fused kernel takes


# the fused pair's smallest split-fp16 kernel size (RVC_AMD_RB_F16_KMIN, A/B switch): 3 since round 5 (C = 64 K = 3
# pairs 371 -> 327 us, C = 32 250 -> 231, clip stream +0.6 %; scripts/gpu_r5_rbk3.sh), 7 before
RB_F16_KMIN = int(os.environ.get("RVC_AMD_RB_F16_KMIN", "3"))


def rb_passes(K):
    """The fused ResBlock pair's pass set under the current precision: "fp32" mixes in split-fp16 for
    k >= RB_F16_KMIN (round 2: 7-8 % faster at k >= 7 and slower at k = 3; round 5: faster at k = 3 too)."""
    if _PRECISION == "fp32" and F16_MIX and K >= RB_F16_KMIN:
        return F16X3
    return PASSES[_PRECISION]


# the 128-channel fused pair (round 4; <= 2 split planes fit LDS: pass sets 3, 1, F16X3): correct (bit-identical to
# two launches, tests/test_gpu_resblock.py) but measured slower in the clip stream (893 vs 920 xRT), so only on
# request: RVC_AMD_FUSED_RB128=1
FUSED_RB128 = os.environ.get("RVC_AMD_FUSED_RB128", "0") != "0"


def resblock_fusable(c1: "Conv", c2: "Conv", dil: int) -> bool:
    passes = rb_passes(c1.K)
    chans = c1.Co in (32, 64) or (c1.Co == 128 and FUSED_RB128 and passes in (3, 1, F16X3))
    return (FUSED_RB and passes in RB_PASSES and c1.wx is not None and c2.wx is not None
            and c1.Ci == c1.Co == c2.Ci == c2.Co
            and chans and c1.K == c2.K and c1.K % 2 == 1 and c1.K <= 15 and (c1.K - 1) * dil <= 64)


def resblock_pair(x, y, c1: "Conv", c2: "Conv", dil: int, slope: float, accumulate: bool = False):
    """y (+)= x + c2(lrelu(c1(lrelu(x), dil)))  (residuals.py:22-44, one pair) in one launch; x [C][L] or
    [B][C][L] (B clips, each bit-identical to its own call)."""
    B, C, L = _shape3(x)
    if y.shape != x.shape or not x.is_contiguous() or not y.is_contiguous() or x.data_ptr() == y.data_ptr():
        raise ValueError("resblock_pair: x, y must be distinct contiguous [(B)][C][L] buffers")
    a = _lib.ResblockArgs()
    a.x, a.y = _p(x), _p(y)
    passes = rb_passes(c1.K)
    a.w1x, a.w2x = ctypes.c_void_p(c1.wx.data_ptr(passes)), ctypes.c_void_p(c2.wx.data_ptr(passes))
    a.b1, a.b2 = _p(c1.b), _p(c2.b)
    a.C, a.L, a.K, a.dil = C, L, c1.K, dil
    a.B = B
    a.nmf1, a.nmf2 = c1.wx_nmf, c2.wx_nmf
    a.passes, a.accumulate, a.slope = passes, int(bool(accumulate)), slope
    check(_lib.load().rvc_resblock_pair(ctypes.byref(a), _stream()), "resblock_pair")
    return y


def attention(q, k, v, o, *, B, H, D, T, ldc, q_hs, k_hs, v_hs, o_hs, scale, q_bs=0, k_bs=0, v_bs=0, o_bs=0,
              rk=None, ev=None, ml=None, W=0, amax_out=None, amax_in=None):
    """Flash attention (rvc_attention_ex); ``amax_out``: a |max| cell (``AmaxSlots``) that receives max |o|;
    ``amax_in``: the cell holding max |q|, |k|, |v| (the QKV projection's) -- both products then run in split-fp16
    on the fp16 matrix cores (round 6; ``rvc_attention_set_f16`` / RVC_ATTN_F16=0 keep the f32 kernel)."""
    a = _lib.AttnArgs()
    a.q, a.k, a.v, a.o, a.rk, a.ev, a.ml = _p(q), _p(k), _p(v), _p(o), _p(rk), _p(ev), _p(ml)
    a.B, a.H, a.D, a.T, a.ldc = B, H, D, T, ldc
    a.q_hs, a.k_hs, a.v_hs, a.o_hs = q_hs, k_hs, v_hs, o_hs
    a.q_bs, a.k_bs, a.v_bs, a.o_bs = q_bs, k_bs, v_bs, o_bs
    a.W, a.scale = W, scale
    lib = _lib.load()
    need = lib.rvc_attention_workspace_bytes(ctypes.byref(a))
    if need < 0:
        raise ValueError(f"attention: unsupported shape H={H} D={D} T={T}")
    ws = _workspace(o.device, need, "attn") if need else None
    for cell in (amax_in, amax_out):
        if cell is not None and cell.numel() < B * AMAX_SHARDS:
            raise ValueError("attention: a |max| cell needs AMAX_SHARDS words per batch element")
    check(lib.rvc_attention_ex(ctypes.byref(a), _p(amax_in), _p(amax_out), _p(ws), need, _stream()), "attention")
    return o


def textenc_embed(lin, emb, pitch, out, B, C, T, scale, slope, amax_out=None):
    """``amax_out``: a |max| cell (``AmaxSlots``) that receives max |out| per batch element."""
    if amax_out is not None and amax_out.numel() < B * AMAX_SHARDS:
        raise ValueError("textenc_embed: amax_out needs a cell per batch element")
    check(_lib.load().rvc_textenc_embed_amax(_p(lin), _p(emb), _p(pitch), _p(out), B, C, T, scale, slope,
                                             _p(amax_out), _stream()), "textenc_embed")
    return out


def layernorm_cf(x, res, gamma, beta, out, B, C, T, eps=1e-5, amax_out=None):
    """LayerNorm over channels of x (+ res); ``amax_out``: a |max| cell that receives max |out|."""
    if x.numel() < B * C * T or out.numel() < B * C * T or gamma.numel() < C:
        raise ValueError("layernorm_cf: size mismatch")
    if amax_out is not None:
        check(_lib.load().rvc_layernorm_cf_amax(_p(x), _p(res), _p(gamma), _p(beta), _p(out), B, C, T, eps,
                                                _p(amax_out), _stream()), "layernorm_cf")
    else:
        check(_lib.load().rvc_layernorm_cf(_p(x), _p(res), _p(gamma), _p(beta), _p(out), B, C, T, eps, _stream()),
              "layernorm_cf")
    return out


def chnorm_gelu(x, gamma, beta, out, B, C, L, eps=1e-5, gelu=True):
    if x.numel() < B * C * L or out.numel() < B * C * L:
        raise ValueError("chnorm_gelu: size mismatch")
    check(_lib.load().rvc_chnorm_gelu(_p(x), _p(gamma), _p(beta), _p(out), B, C, L, eps, int(gelu), _stream()),
          "chnorm_gelu")
    return out


def fe0_gn_gelu(wav, w_km, gamma, beta, B, N, C, K, stride, eps=1e-5, gelu=True, x_bstride=0, amax_out=None):
    """ContentVec's first layer fused: conv(1 -> C, k K, stride) of wav [B][N] + GroupNorm(C, C) + affine + GELU
    -> [B][C][T] (rvc_fe0_gn_gelu; w_km: the K-major packed conv weight [K][C], ops.Conv.w); ``amax_out``: a |max|
    cell (``AmaxSlots``) that receives max |out| per batch element (rvc_fe0_gn_gelu_amax)."""
    lib = _lib.load()
    T = (N - K) // stride + 1
    out = torch.empty(B, C, T, device=wav.device) if B > 1 else torch.empty(C, T, device=wav.device)
    need = lib.rvc_fe0_ws_bytes(B, C, T)
    ws = _workspace(wav.device, need, kind="fe0")
    if amax_out is not None and amax_out.numel() < B * AMAX_SHARDS:
        raise ValueError("fe0_gn_gelu: amax_out needs a cell per batch element")
    check(lib.rvc_fe0_gn_gelu_amax(_p(wav), B, N, x_bstride, _p(w_km), C, K, stride, _p(gamma), _p(beta), _p(out),
                                   eps, int(gelu), _p(amax_out), _p(ws), need, _stream()), "fe0_gn_gelu")
    return out


def prior_sample(stats, noise, zp, B, C, T, nscale=0.66666):
    check(_lib.load().rvc_prior_sample(_p(stats), _p(noise), _p(zp), B, C, T, nscale, _stream()), "prior_sample")
    return zp


def gate(a, out, B, H, T):
    check(_lib.load().rvc_gate(_p(a), _p(out), B, H, T, _stream()), "gate")
    return out


def flip_channels(x, out, B, C, T):
    check(_lib.load().rvc_flip_channels(_p(x), _p(out), B, C, T, _stream()), "flip")
    return out


def transpose(x, out, B, R, C):
    check(_lib.load().rvc_transpose(_p(x), _p(out), B, R, C, _stream()), "transpose")
    return out


# Device-resident seed added to every Philox draw while set (graph.ClipGraph: replays draw fresh noise).
_DEV_SEED = None


class device_seed:
    """``with ops.device_seed(t):`` -- t: device int64 [1]; draws use seed + t[0], read at run time."""

    def __init__(self, t):
        self.t = t

    def __enter__(self):
        global _DEV_SEED
        self.prev, _DEV_SEED = _DEV_SEED, self.t
        return self

    def __exit__(self, *a):
        global _DEV_SEED
        _DEV_SEED = self.prev


def graph_mode() -> bool:
    """True while a device seed is set, i.e. while ClipGraph warms up or captures."""
    return _DEV_SEED is not None


def randn(out, seed, offset=0):
    add = _p(_DEV_SEED) if _DEV_SEED is not None else None
    check(_lib.load().rvc_randn_ex(_p(out), out.numel(), seed, offset, add, _stream()), "randn")
    return out


def rand_triang(out, lo, hi, seed, offset=0):
    """Symmetric triangular draws on [lo, hi] (Philox counter stream; device seed added when set)."""
    add = _p(_DEV_SEED) if _DEV_SEED is not None else None
    check(_lib.load().rvc_rand_triang(_p(out), out.numel(), lo, hi, seed, offset, add, _stream()), "rand_triang")
    return out


def sine_source(f0, noise, har, work, B, T, upp, sr, lin_w, lin_b):
    if f0.numel() < B * T or noise.numel() < B * T * upp or har.numel() < B * T * upp or work.numel() < B * T:
        raise ValueError("sine_source: size mismatch")
    check(_lib.load().rvc_sine_source(_p(f0), _p(noise), _p(har), _p(work), B, T, upp, sr, lin_w, lin_b, _stream()),
          "sine_source")
    return har


# ------------------------------------------------------------------ MRF-HiFi-GAN / RefineGAN (vocoder.hip)
# Philox counter ranges of the extra draws under a clip's seed (include/rvc_amd.h, next to rvc_randn)
OFF_SINE = 1 << 40
OFF_PHASE = 1 << 39
ADAIN_BMAX = 16  # RVC_ADAIN_BMAX


def off_adain(k: int) -> int:
    """Counter offset of RefineGAN's k-th AdaIN draw (the reference's draw order)."""
    return (2 + k) << 40


def rand_uniform(out, seed, offset=0):
    """Uniform draws on [0, 1) (Philox counter stream; device seed added when set)."""
    add = _p(_DEV_SEED) if _DEV_SEED is not None else None
    check(_lib.load().rvc_rand_uniform(_p(out), out.numel(), seed, offset, add, _stream()), "rand_uniform")
    return out


def harmonic_source(f0, phase0, noise, har, B, T, upp, H, sr, lin_w, lin_b=0.0, linear=False):
    """The per-sample harmonic source (rvc_harmonic_source): f0 [B][T], phase0 [B][H], noise [B][T*upp][H] ->
    har [B][T*upp]; lin_w: the merge's H weights (host floats), lin_b its bias."""
    L = T * upp
    lin_w = [float(v) for v in lin_w]
    if len(lin_w) != H:
        raise ValueError("harmonic_source: one merge weight per harmonic")
    if f0.numel() < B * T or phase0.numel() < B * H or noise.numel() < B * L * H or har.numel() < B * L:
        raise ValueError("harmonic_source: size mismatch")
    for t in (f0, phase0, noise, har):
        if not t.is_contiguous() or t.dtype != torch.float32:
            raise ValueError("harmonic_source: contiguous f32 tensors")
    lib = _lib.load()
    need = lib.rvc_harmonic_source_ws_bytes(B, T, upp, H)
    if need < 0:
        raise ValueError(f"harmonic_source: unsupported shape B={B} T={T} upp={upp} H={H}")
    ws = _workspace(har.device, need, "hsrc")
    check(lib.rvc_harmonic_source(_p(f0), _p(phase0), _p(noise), _p(har), B, T, upp, H, int(bool(linear)), float(sr),
                                  (ctypes.c_float * H)(*lin_w), float(lin_b), _p(ws), need, _stream()),
          "harmonic_source")
    return har


def upsample_linear(x, r, out=None, act=ACT_NONE, slope=0.0, y_bstride=0):
    """nn.Upsample(scale_factor=r, mode="linear") of act(x), x [B][C][Lin] contiguous -> [B][C][Lin*r] (or the first C
    channels of ``out``, a wider [B][C'][Lin*r] buffer with batch stride ``y_bstride``)."""
    B, C, Lin = _shape3(x)
    Lout = Lin * r
    if not x.is_contiguous() or x.dtype != torch.float32:
        raise ValueError("upsample_linear: contiguous f32 input")
    if out is None:
        out = torch.empty(B, C, Lout, device=x.device)
    elif out.dtype != torch.float32 or _room(out) < (B - 1) * (y_bstride or C * Lout) + C * Lout or \
            (y_bstride and y_bstride < C * Lout):
        raise ValueError("upsample_linear: output buffer too small")
    check(_lib.load().rvc_upsample_linear(_p(x), _p(out), B, C, Lin, r, 0, y_bstride, act, slope, _stream()),
          "upsample_linear")
    return out


def adain(x, w, out, noise=None, seeds=None, offset=0, slope=0.2, out_scale=1.0, accumulate=False):
    """out (+)= out_scale * lrelu(x + n * w[c], slope) over x [B][C][L] (rvc_adain); n from ``noise`` [B][C][L], or
    drawn in the kernel exactly as ``randn(buf[b], seeds[b], offset)`` would fill it."""
    B, C, L = _shape3(x)
    if out.numel() < B * C * L or w.numel() < C or not x.is_contiguous() or not out.is_contiguous() or \
            x.dtype != torch.float32 or out.dtype != torch.float32:
        raise ValueError("adain: size mismatch")
    lib = _lib.load()
    if noise is not None:
        if noise.numel() < B * C * L or not noise.is_contiguous():
            raise ValueError("adain: noise [B][C][L]")
        check(lib.rvc_adain(_p(x), _p(noise), _p(w), _p(out), B, C, L, slope, out_scale, int(bool(accumulate)), None,
                            0, None, _stream()), "adain")
        return out
    if seeds is None or len(seeds) != B:
        raise ValueError("adain: one seed per clip")
    add = _p(_DEV_SEED) if _DEV_SEED is not None else None
    n = C * L
    for b0 in range(0, B, ADAIN_BMAX):
        nb = min(ADAIN_BMAX, B - b0)
        sd = (ctypes.c_uint64 * nb)(*[int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds[b0:b0 + nb]])
        xs, ys = x.reshape(-1)[b0 * n:], out.reshape(-1)[b0 * n:]
        check(lib.rvc_adain(_p(xs), None, _p(w), _p(ys), nb, C, L, slope, out_scale, int(bool(accumulate)), sd,
                            offset, add, _stream()), "adain")
    return out


def stft_frames(x, win, out, N, F, nfft, hop):
    if x.numel() < N or win.numel() < nfft or out.numel() < nfft * F:
        raise ValueError("stft_frames: size mismatch")
    check(_lib.load().rvc_stft_frames(_p(x), _p(win), _p(out), N, F, nfft, hop, _stream()), "stft_frames")
    return out


def stft_mag(x, win, mag, N, F, nfft, hop):
    """|STFT| in f64: x [N] or [B][N] -> mag [nfft/2+1][F] or [B][nfft/2+1][F], rounded once to f32, or unrounded
    for an f64 ``mag`` (stft_mag64)."""
    if mag.dtype == torch.float64:
        return stft_mag64(x, win, mag, N, F, nfft, hop)
    B = x.shape[0] if x.dim() == 2 else 1
    K = nfft // 2 + 1
    if (x.shape[-1] < N or win.numel() < nfft or mag.numel() < B * K * F or mag.shape[-1] != F
            or (B > 1 and (mag.dim() != 3 or mag.shape[0] != B))):
        raise ValueError("stft_mag: size mismatch")
    if x.stride(-1) != 1 or mag.stride(-1) != 1:
        raise ValueError("stft_mag: x / mag rows must be contiguous")
    xs = x.stride(0) if B > 1 else 0
    ms = mag.stride(0) if B > 1 else 0
    check(_lib.load().rvc_stft_mag(_p(x), _p(win), _p(mag), B, N, F, nfft, hop, xs, ms, _stream()), "stft_mag")
    return mag


def spec_mag(spec, mag, K, F):
    if spec.numel() < 2 * K * F or mag.numel() < K * F:
        raise ValueError("spec_mag: size mismatch")
    check(_lib.load().rvc_spec_mag(_p(spec), _p(mag), K, F, _stream()), "spec_mag")
    return mag


# RMVPE's image glue (rmvpe.hip), f32 or f64 by the tensors' dtype, on one image or on [B][...] views (batch strides
# from the views).  Every op that writes a bordered image writes its zero border too.
def _glue(fn32, fn64, src, src_nd, src_n, dst, dst_nd, dst_n, *dims):
    """src ([B] + src_nd dims, src_n elements each) -> dst: one launch of the batched f64 entry point, or the f32
    entry point (one image per launch) clip by clip."""
    B = src.shape[0] if src.dim() > src_nd else 1
    if src.dtype != dst.dtype or _room(src) < B * src_n or _room(dst) < B * dst_n:
        raise ValueError(fn32 + ": size or dtype mismatch")
    lib = _lib.load()
    if src.dtype == torch.float64:
        check(getattr(lib, fn64)(_pd(src), _pd(dst), B, *dims, _bs(src, src_nd), _bs(dst, dst_nd), _stream()), fn64)
    else:
        for b in range(B):
            check(getattr(lib, fn32)(_p(src[b] if src.dim() > src_nd else src),
                                     _p(dst[b] if dst.dim() > dst_nd else dst), *dims, _stream()), fn32)
    return dst


def mel_image(mel, img, M, F, Tp, scale, shift):
    """mel [(B)][M][F] -> bordered images [(B)][1][Tp+2][M+2]: reflect-padded frames, times scale plus shift."""
    return _glue("rvc_mel_image", "rvc_mel_image64", mel, 2, M * F, img, 3, (Tp + 2) * (M + 2), M, F, Tp, scale, shift)


def avgpool2(x, out, C, H, W):
    """AvgPool2d(2): bordered [(B)][C][H+2][W+2] -> bordered [(B)][C][H/2+2][W/2+2]."""
    return _glue("rvc_avgpool2", "rvc_avgpool2_64", x, 3, C * (H + 2) * (W + 2), out, 3,
                 C * (H // 2 + 2) * (W // 2 + 2), C, H, W)


def interleave4(phases, out, C, H, W):
    """phases [(B)][4][C][H+2][W+2] -> the first C channels of bordered out [(B)][*][2H+2][2W+2]."""
    return _glue("rvc_interleave4", "rvc_interleave4_64", phases, 4, 4 * C * (H + 2) * (W + 2), out, 3,
                 C * (2 * H + 2) * (2 * W + 2), C, H, W)


def img_to_seq(img, x, C, H, W):
    """bordered [(B)][C][H+2][W+2] -> sequence rows [(B)][C*W][H]."""
    return _glue("rvc_img_to_seq", "rvc_img_to_seq64", img, 3, C * (H + 2) * (W + 2), x, 2, C * W * H, C, H, W)


def bigru(gi, whh, bhh, y, gran, err, T):
    if gi.numel() < 2 * 768 * T or whh.numel() < 2 * 768 * 256 or y.numel() < 512 * T or gran.numel() < 1024:
        raise ValueError("bigru: size mismatch")
    check(_lib.load().rvc_bigru(_p(gi), _p(whh), _p(bhh), _p(y), _p(gran), _p(err), T, _stream()), "bigru")
    return y


GRU_B_MAX = 16  # sequences per bigru launch (rvc_bigru_batched); gran scratch is 1024 int64 per sequence


def bigru_batched(gi, whh, bhh, y, gran, err, B, T):
    """B independent BiGRU recurrences: gi [B][1536][T], y [B][512][T] (batch strides from the tensors)."""
    if gi.dim() != 3 or y.dim() != 3 or gi.shape[0] < B or y.shape[0] < B or gi.shape[1] != 1536 or y.shape[1] != 512:
        raise ValueError("bigru_batched: gi [B][1536][T], y [B][512][T] expected")
    if gi.shape[2] < T or y.shape[2] < T or gran.numel() < 1024 * min(B, GRU_B_MAX) or whh.numel() < 2 * 768 * 256:
        raise ValueError("bigru_batched: size mismatch")
    check(_lib.load().rvc_bigru_batched(_p(gi), gi.stride(0), _p(whh), _p(bhh), _p(y), y.stride(0), _p(gran), _p(err),
                                        B, T, _stream()), "bigru_batched")
    return y


# ------------------------------------------------------------------ f64 RMVPE (rmvpe64.hip)
def _pd(t):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.float64:
        raise TypeError(f"rvc_amd: expected a CUDA f64 tensor, got {t.dtype} on {t.device}")
    return ctypes.c_void_p(t.data_ptr())


class Conv64:
    """A Conv weight [Co, Ci, K] (and bias [Co]) kept in f64 KM layout for ``conv64``."""

    def __init__(self, w, b=None, device="cuda"):
        self.Co, self.Ci, self.K = (int(s) for s in w.shape)
        self.w = pack_km(w.double()).to(device)
        self.b = b.double().to(device) if b is not None else None

    def __call__(self, x, Lout=None, **kw):
        return conv64(x, self.w, self.Ci, self.Co, self.K, bias=self.b, Lout=Lout, **kw)


def conv64(x, w, Ci, Co, K, *, bias=None, pad=0, Lout=None, out=None, res=None, out_act=ACT_NONE, out_slope=0.0,
           B=None, Lin=None, x_bstride=0, y_bstride=0, res_bstride=0, toff=None, wrap=0, out_f32=False, plan=False):
    """The f64 conv (rvc_conv64): x [B][Ci][Lin] f64, y f64 (or f32 when ``out_f32``), stride 1, K taps at
    ``toff`` (or 0..K-1), 2-D border masking with ``wrap``; see include/rvc_amd.h.  ``plan=True`` launches
    nothing and returns the planner's choice (rvc_conv64_plan): (tile, split-K, compact, blocks)."""
    if B is None:
        B, Cx, Lx = _shape3(x)
        if Lin is None:
            Lin = Lx
        if Cx != Ci:
            raise ValueError(f"conv64: x has {Cx} channels, weight expects {Ci}")
        if not x.is_contiguous():
            raise ValueError("conv64: x must be contiguous")
    if Lout is None:
        Lout = Lin + 2 * pad - (K - 1)
    if Lout <= 0:
        raise ValueError("conv64: empty output")
    if w.numel() < Ci * K * Co or w.dtype != torch.float64:
        raise ValueError("conv64: f64 KM weight [Ci*K][Co] expected")
    ydt = torch.float32 if out_f32 else torch.float64
    if out is None:
        out = torch.empty(*((B,) if B > 1 else ()), Co, Lout, device=x.device, dtype=ydt)
    elif out.dtype != ydt or _room(out) < (B - 1) * (y_bstride or Co * Lout) + Co * Lout:
        raise ValueError("conv64: output buffer too small or of the wrong dtype")
    if res is not None and _room(res) < (B - 1) * (res_bstride or Co * Lout) + Co * Lout:
        raise ValueError("conv64: residual too small")
    if _room(x) < (B - 1) * (x_bstride or Ci * Lin) + Ci * Lin:
        raise ValueError("conv64: input buffer too small")
    if bias is not None and bias.numel() < Co:
        raise ValueError("conv64: bias too small")
    a = _lib.Conv64Args()
    a.x, a.w, a.bias, a.res = _pd(x), _pd(w), _pd(bias), _pd(res)
    a.y = _p(out) if out_f32 else _pd(out)
    a.B, a.Ci, a.Co, a.Lin, a.Lout = B, Ci, Co, Lin, Lout
    a.x_bstride, a.y_bstride, a.res_bstride = x_bstride, y_bstride, res_bstride
    a.K, a.pad, a.out_act, a.y_f32, a.out_slope = K, pad, out_act, int(bool(out_f32)), out_slope
    if toff is not None:
        if len(toff) != K or K > 16:
            raise ValueError("conv64: toff must have K <= 16 entries")
        a.ntoff = K
        for i, v in enumerate(toff):
            a.toff[i] = int(v)
    a.wrap = wrap
    lib = _lib.load()
    if plan:
        res4 = (ctypes.c_int * 4)()
        check(lib.rvc_conv64_plan(ctypes.byref(a), res4), "conv64_plan")
        return tuple(res4)
    need = lib.rvc_conv64_workspace_bytes(ctypes.byref(a))
    if need < 0:
        raise RuntimeError(f"rvc_amd: conv64 plan failed: {lib.rvc_last_error().decode()}")
    ws = _workspace(out.device, need, "c64") if need else None
    check(lib.rvc_conv64(ctypes.byref(a), _p(ws), need, _stream()), "conv64")
    return out


def wino64_use(Ci, Co, H=0, W=0):
    """Whether the f64 RMVPE takes the Winograd F(4x4, 3x3) form for a Ci -> Co 3x3 conv on an H x W image
    (rvc_wino64_use; H = W = 0: the channel rule alone, i.e. whether to prepare the transformed weights)."""
    return bool(_lib.load().rvc_wino64_use(Ci, Co, H, W))


def wino64_weights(w_km, Ci, Co):
    """KM f64 3x3 weights [Ci*9][Co] -> the 36 Winograd weight matrices [36][Ci][Co] (rvc_wino64_weights)."""
    v = torch.empty(36, Ci, Co, dtype=torch.float64, device=w_km.device)
    check(_lib.load().rvc_wino64_weights(_pd(w_km), _pd(v), Ci, Co, _stream()), "wino64_weights")
    return v


def wino64(x, v, Ci, Co, H, W, *, bias=None, res=None, out=None, out_act=ACT_NONE, B=1, x_bstride=0, y_bstride=0,
           res_bstride=0, out_f32=False):
    """The f64 Winograd F(4x4, 3x3) conv (rvc_wino64_conv) on bordered [Ci][H+2][W+2] images (or B of them with
    batch strides): y = act(conv3x3(x) + bias) (+ res), border cells 0."""
    L = (H + 2) * (W + 2)
    ydt = torch.float32 if out_f32 else torch.float64
    if out is None:
        out = torch.empty(*((B,) if B > 1 else ()), Co, H + 2, W + 2, device=x.device, dtype=ydt)
    elif out.dtype != ydt or _room(out) < (B - 1) * (y_bstride or Co * L) + Co * L:
        raise ValueError("wino64: output buffer too small or of the wrong dtype")
    if _room(x) < (B - 1) * (x_bstride or Ci * L) + Ci * L or x.dtype != torch.float64:
        raise ValueError("wino64: f64 input of [B][Ci][H+2][W+2] expected")
    if res is not None and _room(res) < (B - 1) * (res_bstride or Co * L) + Co * L:
        raise ValueError("wino64: residual too small")
    if v.numel() < 36 * Ci * Co or v.dtype != torch.float64:
        raise ValueError("wino64: f64 weights [36][Ci][Co] expected")
    a = _lib.Wino64Args()
    a.x, a.v, a.bias, a.res = _pd(x), _pd(v), _pd(bias), _pd(res)
    a.y = _p(out) if out_f32 else _pd(out)
    a.B, a.Ci, a.Co, a.H, a.W = B, Ci, Co, H, W
    a.x_bstride, a.y_bstride, a.res_bstride = x_bstride, y_bstride, res_bstride
    a.out_act, a.y_f32 = out_act, int(bool(out_f32))
    lib = _lib.load()
    need = lib.rvc_wino64_workspace_bytes(ctypes.byref(a))
    if need < 0:
        raise RuntimeError(f"rvc_amd: wino64 plan failed: {lib.rvc_last_error().decode()}")
    ws = _workspace(out.device, need, "w64")
    check(lib.rvc_wino64_conv(ctypes.byref(a), _p(ws), need, _stream()), "wino64")
    return out


def conv64_set_plan(tile=-1, ksplit=-1, compact=-1):
    """Force the f64 conv planner's choice (rvc_conv64_set_plan; -1 = the planner's): sweeps and tests."""
    check(_lib.load().rvc_conv64_set_plan(tile, ksplit, compact), "conv64_set_plan")


def _bs(t, nd):
    """Batch stride of a [B][...] view (0 for an unbatched tensor of ``nd`` dims)."""
    return t.stride(0) if t.dim() > nd else 0


def stft_mag64(x, win, mag, N, F, nfft, hop):
    """|STFT| in f64 (unrounded): x [N] or [B][N] f32 -> mag f64 [nfft/2+1][F] or [B][nfft/2+1][F].  Kept under its
    own name (stft_mag reaches it for an f64 ``mag``): bench.py's roofline pass wraps it to count the STFT family."""
    B = x.shape[0] if x.dim() == 2 else 1
    K = nfft // 2 + 1
    if (x.shape[-1] < N or win.numel() < nfft or mag.numel() < B * K * F or mag.shape[-1] != F
            or (B > 1 and (mag.dim() != 3 or mag.shape[0] != B))):
        raise ValueError("stft_mag64: size mismatch")
    if x.stride(-1) != 1 or mag.stride(-1) != 1:
        raise ValueError("stft_mag64: x / mag rows must be contiguous")
    check(_lib.load().rvc_stft_mag64(_p(x), _p(win), _pd(mag), B, N, F, nfft, hop, x.stride(0) if B > 1 else 0,
                                     mag.stride(0) if B > 1 else 0, _stream()), "stft_mag64")
    return mag


GRU64_GRAN = 16384 // 8  # int64 words of bigru64 hand-off scratch per sequence (RVC_BIGRU64_GRAN_BYTES)


def bigru64_batched(gi, whh, bhh, y, gran, err, B, T):
    """B f64 BiGRU recurrences: gi [(B)][1536][T], y [(B)][512][T] f64."""
    if gi.shape[-2] != 1536 or y.shape[-2] != 512 or gi.shape[-1] < T or y.shape[-1] < T:
        raise ValueError("bigru64: gi [(B)][1536][T], y [(B)][512][T] expected")
    if (gi.dim() == 3 and gi.shape[0] < B) or (y.dim() == 3 and y.shape[0] < B) or (B > 1 and gi.dim() != 3):
        raise ValueError("bigru64: batch mismatch")
    if gran.numel() < GRU64_GRAN * min(B, GRU_B_MAX) or whh.numel() < 2 * 768 * 256 or whh.dtype != torch.float64:
        raise ValueError("bigru64: size mismatch")
    check(_lib.load().rvc_bigru64_batched(_pd(gi), _bs(gi, 2), _pd(whh), _pd(bhh), _pd(y), _bs(y, 2), _p(gran), _p(err),
                                          B, T, _stream()), "bigru64")
    return y


class F0Post:
    """The optional steps of VC.get_f0 between the raw f0 and the quantiser (convert.py:311-318):
    autotune strength (None = off) and the f0-file override ``rep`` (f64 values for frames
    [rep_off, rep_off + len(rep)))."""

    def __init__(self, autotune_strength=None, rep=None, rep_off=0, device=None):
        self.autotune_strength = autotune_strength
        self.rep = None
        self.rep_off = int(rep_off)
        if rep is not None and len(rep) > 0:
            import numpy as np
            self.rep = torch.from_numpy(np.ascontiguousarray(rep, dtype=np.float64)).to(device)

    def struct(self, F):
        """ctypes rvc_f0_post for an f0 track of F frames (the override is clipped to it)."""
        s = _lib.F0Post()
        if self.autotune_strength is not None:
            s.autotune, s.strength = 1, float(self.autotune_strength)
        if self.rep is not None and self.rep_off < F:
            s.rep = ctypes.c_void_p(self.rep.data_ptr())
            s.rep_off, s.rep_len = self.rep_off, min(self.rep.numel(), F - self.rep_off)
        return s


def _post_ref(post, F):
    return ctypes.byref(post.struct(F)) if post is not None else None


def f0_post64(f0, p_len, pitch, post=None):
    """get_f0's tail on an f64 track (convert.py:308-323; rvc_pm_post): f0 device f64 [nf], zero-padded in front and
    behind to p_len when shorter (get_f0_pm's padding), then autotune / shift by ``pitch`` semitones / f0 file / the
    mel quantiser, all in f64 -> (coarse int64 [nout], pitchf f32 [nout]), nout = max(p_len, nf).  The tail of pm,
    fcpe, fcpe-legacy and the hybrids; rmvpe, crepe and swipe fuse theirs into their own decode kernels."""
    nf = f0.numel()
    nout = max(p_len, nf)
    coarse = torch.empty(nout, dtype=torch.int64, device=f0.device)
    pitchf = torch.empty(nout, dtype=torch.float32, device=f0.device)
    check(_lib.load().rvc_pm_post(_pd(f0), nf, p_len, float(2.0 ** (pitch / 12)), _post_ref(post, nout), _p(coarse),
                                  _p(pitchf), _stream()), "pm_post")
    return coarse, pitchf


def f0_resample_nan(source, p_len):
    """get_f0_mangio_crepe's tail (convert.py:226-228; rvc_f0_resample_nan): source device f32 [T] -> f64 [p_len],
    np.nan_to_num(np.interp(np.arange(0, T * p_len, T) / p_len, np.arange(T), source)) with source < 0.001 as NaN."""
    if not source.is_cuda or source.dtype != torch.float32 or source.dim() != 1 or not source.is_contiguous():
        raise TypeError(f"f0_resample_nan: expected a contiguous 1-D CUDA f32 tensor, got {source.dtype} "
                        f"{tuple(source.shape)} on {source.device}")
    out = torch.empty(int(p_len), dtype=torch.float64, device=source.device)
    check(_lib.load().rvc_f0_resample_nan(_p(source), source.numel(), int(p_len), _pd(out), _stream()),
          "f0_resample_nan")
    return out


def rmvpe_decode(sal, ld, F, thred, shift, f0, coarse, pitchf, post=None, f0_range=None):
    """rvc_rmvpe_decode; ``f0_range`` = (f0_min, f0_max) zeroes the decoded f0 outside it first (rmvpe-legacy,
    rvc_rmvpe_decode_range)."""
    if sal.numel() < 360 * ld or coarse.numel() < F or pitchf.numel() < F or (f0 is not None and f0.numel() < F):
        raise ValueError("rmvpe_decode: size mismatch")
    f0p = ctypes.c_void_p(f0.data_ptr()) if f0 is not None else None
    if f0_range is not None:
        check(_lib.load().rvc_rmvpe_decode_range(_p(sal), ld, F, thred, float(f0_range[0]), float(f0_range[1]), shift,
                                                 _post_ref(post, F), f0p, _p(coarse), _p(pitchf), _stream()),
              "rmvpe_decode_range")
        return
    check(_lib.load().rvc_rmvpe_decode(_p(sal), ld, F, thred, shift, _post_ref(post, F), f0p, _p(coarse), _p(pitchf),
                                       _stream()), "rmvpe_decode")


class FiltFilt:
    """scipy.signal.filtfilt(b, a, .) + reflect padding on the device (filtfilt.hip); zi = lfilter_zi(b, a)
    is computed once on the host like the filter design itself."""

    def __init__(self, b, a):
        from scipy import signal
        import numpy as np
        self.b = np.ascontiguousarray(b, dtype=np.float64)
        self.a = np.ascontiguousarray(a, dtype=np.float64)
        if self.b.size != 6 or self.a.size != 6 or self.a[0] != 1.0:
            raise ValueError("FiltFilt: 5th-order filter with a[0] == 1 expected")
        self.zi = np.ascontiguousarray(signal.lfilter_zi(self.b, self.a), dtype=np.float64)

    def __call__(self, x, tpad, want_f64=False):
        """x: device f32 [N] -> (reflect-padded filtered f32 [N + 2 tpad], f64 copy or None)."""
        N = x.numel()
        nbytes = _lib.load().rvc_filtfilt_work_bytes(N)
        if nbytes < 0:
            raise ValueError(f"filtfilt: bad length {N}")
        work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
        out = torch.empty(N + 2 * tpad, device=x.device)
        out64 = torch.empty(N + 2 * tpad, dtype=torch.float64, device=x.device) if want_f64 else None
        h = lambda arr: ctypes.c_void_p(arr.ctypes.data)  # noqa: E731
        check(_lib.load().rvc_filtfilt_pad(_p(x), N, h(self.b), h(self.a), h(self.zi), tpad,
                                           ctypes.c_void_p(work.data_ptr()), _p(out),
                                           ctypes.c_void_p(out64.data_ptr()) if want_f64 else None, _stream()),
              "filtfilt_pad")
        return out, out64


def quiet_points(x64, window, t_center, t_query, t_max):
    """VC.pipeline's quiet-point segmentation (convert.py:404-412) on the device: the filtered f64 signal
    x64 [n] (unpadded) -> host list of opt_ts (one small device->host copy; the segment plan needs it)."""
    lib = _lib.load()
    n = x64.numel()
    cnt = lib.rvc_quiet_points_count(n, window, t_center, t_max)
    if cnt < 0:
        raise ValueError("quiet_points: bad arguments")
    if cnt == 0:
        return []
    if x64.dtype != torch.float64 or not x64.is_cuda or not x64.is_contiguous():
        raise TypeError("quiet_points: a contiguous CUDA f64 signal")
    need = lib.rvc_quiet_points_ws_bytes(n, window, t_center, t_query, t_max)
    ws = _workspace(x64.device, need, "quiet")
    out = torch.empty(cnt, dtype=torch.int64, device=x64.device)
    check(lib.rvc_quiet_points(ctypes.c_void_p(x64.data_ptr()), n, window, t_center, t_query, t_max, _p(ws), need,
                               _p(out), _stream()), "quiet_points")
    return out.cpu().tolist()


IVF_FAISS, IVF_EXACT = 0, 1  # RVC_IVF_FAISS (faiss's own f32 arithmetic, the default) / RVC_IVF_EXACT (f64)


def ivf_search(q, nq, d, cs, qs, centT, nlist, nprobe, list_off, codes, ids, k, D, I, probes, arithmetic=IVF_FAISS):
    """FAISS IVF-Flat search (ivf.hip): see include/rvc_amd.h."""
    if D.numel() < nq * k or I.numel() < nq * k or probes.numel() < nq * nprobe or centT.numel() < d * nlist:
        raise ValueError("ivf_search: output / index buffers too small")
    if _room(q) < (d - 1) * cs + (nq - 1) * qs + 1:
        raise ValueError("ivf_search: query buffer too small")
    lib = _lib.load()
    need = lib.rvc_ivf_coarse_ws_bytes(nq, nlist)
    ws = _workspace(q.device, need, "ivf")
    check(lib.rvc_ivf_search_ex(_p(q), nq, d, cs, qs, _p(centT), nlist, nprobe, _p(list_off), _p(codes), _p(ids), k,
                                _p(ws), need, _p(probes), _p(D), _p(I), arithmetic, _stream()), "ivf_search")


def ivf_blend(feats, nq, d, fcs, fqs, D, I, k, big, ntotal, index_rate, out, ocs, oqs):
    if big.numel() < ntotal * d or D.numel() < nq * k or I.numel() < nq * k:
        raise ValueError("ivf_blend: buffers too small")
    check(_lib.load().rvc_ivf_blend(_p(feats), nq, d, fcs, fqs, _p(D), _p(I), k, _p(big), ntotal, float(index_rate),
                                    _p(out), ocs, oqs, _stream()), "ivf_blend")


def _rows(x, what):
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
        raise TypeError(f"{what}: a contiguous CUDA f32 [rows][d] tensor")
    return x.shape


def kmeans_assign(x, cent, assign=None, dist=None):
    """Nearest centroid of every row of x [n][d] (kmeans.hip): (assign int32 [n], dist f32 [n])."""
    (n, d), (k, dc) = _rows(x, "kmeans_assign"), _rows(cent, "kmeans_assign")
    if dc != d:
        raise ValueError(f"kmeans_assign: centroid dim {dc} != {d}")
    assign = torch.empty(n, dtype=torch.int32, device=x.device) if assign is None else assign
    dist = torch.empty(n, dtype=torch.float32, device=x.device) if dist is None else dist
    if assign.numel() < n or dist.numel() < n or assign.dtype != torch.int32:
        raise ValueError("kmeans_assign: output buffers too small")
    lib = _lib.load()
    need = lib.rvc_kmeans_assign_work_bytes(n, d, k)
    if need < 0:
        raise ValueError(f"kmeans_assign: bad sizes n={n} d={d} k={k}")
    ws = _workspace(x.device, need, "kmeans")
    check(lib.rvc_kmeans_assign(_p(x), n, d, _p(cent), k, _p(ws), need, _p(assign), _p(dist), _stream()),
          "kmeans_assign")
    return assign, dist


def kmeans_lists(assign, k):
    """Stable counting sort of the rows by list: (list_off int64 [k + 1], ids int64 [n], counts int32 [k])."""
    if assign.dim() != 1 or assign.dtype != torch.int32 or not assign.is_contiguous():
        raise TypeError("kmeans_lists: a contiguous CUDA int32 [n] tensor")
    n = assign.numel()
    lib = _lib.load()
    need = lib.rvc_kmeans_lists_work_bytes(n, k)
    if need < 0:
        raise ValueError(f"kmeans_lists: bad sizes n={n} k={k}")
    ws = _workspace(assign.device, need, "kmeans_lists")
    list_off = torch.empty(k + 1, dtype=torch.int64, device=assign.device)
    ids = torch.empty(n, dtype=torch.int64, device=assign.device)
    counts = torch.empty(k, dtype=torch.int32, device=assign.device)
    check(lib.rvc_kmeans_lists(_p(assign), n, k, _p(ws), need, _p(list_off), _p(ids), _p(counts), _stream()),
          "kmeans_lists")
    return list_off, ids, counts


def kmeans_update(x, list_off, ids, cent_prev, out=None):
    """faiss compute_centroids over the CSR lists: new centroids [k][d]; empty lists keep cent_prev's row."""
    (n, d), (k, dc) = _rows(x, "kmeans_update"), _rows(cent_prev, "kmeans_update")
    if dc != d or list_off.numel() < k + 1 or ids.numel() < n or list_off.dtype != torch.int64 or \
            ids.dtype != torch.int64:
        raise ValueError("kmeans_update: size mismatch")
    out = torch.empty_like(cent_prev) if out is None else out
    if out.shape != cent_prev.shape or out.data_ptr() == cent_prev.data_ptr():
        raise ValueError("kmeans_update: out must be a separate [k][d] tensor")
    check(_lib.load().rvc_kmeans_update(_p(x), n, d, _p(list_off), _p(ids), k, _p(cent_prev), _p(out), _stream()),
          "kmeans_update")
    return out


def gather_rows(x, ids):
    """out [m][d] = x[ids] for int64 device ids the caller knows to lie in [0, n)."""
    n, d = _rows(x, "gather_rows")
    if ids.dim() != 1 or ids.dtype != torch.int64 or not ids.is_contiguous():
        raise TypeError("gather_rows: a contiguous CUDA int64 [m] tensor")
    out = torch.empty(ids.numel(), d, dtype=torch.float32, device=x.device)
    check(_lib.load().rvc_gather_rows(_p(x), d, _p(ids), ids.numel(), _p(out), _stream()), "gather_rows")
    return out


def minibatch_assign(x, cent, assign=None, dist=None):
    """kmeans_assign for a mini-batch: k may exceed n (kmeans.hip, the same kernels)."""
    (n, d), (k, dc) = _rows(x, "minibatch_assign"), _rows(cent, "minibatch_assign")
    if dc != d:
        raise ValueError(f"minibatch_assign: centroid dim {dc} != {d}")
    assign = torch.empty(n, dtype=torch.int32, device=x.device) if assign is None else assign
    dist = torch.empty(n, dtype=torch.float32, device=x.device) if dist is None else dist
    if assign.numel() < n or dist.numel() < n or assign.dtype != torch.int32:
        raise ValueError("minibatch_assign: output buffers too small")
    lib = _lib.load()
    need = lib.rvc_kmeans_assign_work_bytes(n, d, k)
    if need < 0:
        raise ValueError(f"minibatch_assign: bad sizes n={n} d={d} k={k}")
    ws = _workspace(x.device, need, "kmeans")
    check(lib.rvc_minibatch_assign(_p(x), n, d, _p(cent), k, _p(ws), need, _p(assign), _p(dist), _stream()),
          "minibatch_assign")
    return assign, dist


def _weights(w, k, what):
    if w.dim() != 1 or w.dtype != torch.float32 or not w.is_contiguous() or not w.is_cuda or w.numel() != k:
        raise TypeError(f"{what}: weight_sums must be a contiguous CUDA f32 [{k}] tensor")


def minibatch_update(xb, list_off, ids, cent_prev, weight_sums, out=None):
    """sklearn's _minibatch_update_dense over the batch's CSR lists (minibatch.hip): new centres [k][d];
    weight_sums f32 [k] is updated in place."""
    (n, d), (k, dc) = _rows(xb, "minibatch_update"), _rows(cent_prev, "minibatch_update")
    if dc != d or list_off.numel() < k + 1 or ids.numel() < n or list_off.dtype != torch.int64 or \
            ids.dtype != torch.int64:
        raise ValueError("minibatch_update: size mismatch")
    _weights(weight_sums, k, "minibatch_update")
    out = torch.empty_like(cent_prev) if out is None else out
    if out.shape != cent_prev.shape or out.data_ptr() == cent_prev.data_ptr() or not out.is_contiguous():
        raise ValueError("minibatch_update: out must be a separate [k][d] tensor")
    check(_lib.load().rvc_minibatch_update(_p(xb), n, d, _p(list_off), _p(ids), k, _p(cent_prev), _p(weight_sums),
                                           _p(out), _stream()), "minibatch_update")
    return out


MINIBATCH_STATUS = np.dtype([("inertia", "<f8"), ("wmax", "<f4"), ("any_zero", "<i4"), ("reserved", "<i8", (2,))])


def minibatch_inertia(xb, cent, assign, weight_sums=None, status=None):
    """sum_i ||xb_i - cent[assign_i]||^2 in f64 into the 32-byte device status block (uint8 [32], returned), with
    the largest weight and whether a weight is 0; ``minibatch_status`` reads it on the host."""
    (n, d), (k, dc) = _rows(xb, "minibatch_inertia"), _rows(cent, "minibatch_inertia")
    if dc != d or assign.dim() != 1 or assign.dtype != torch.int32 or assign.numel() < n or \
            not assign.is_contiguous():
        raise ValueError("minibatch_inertia: size mismatch")
    if weight_sums is not None:
        _weights(weight_sums, k, "minibatch_inertia")
    lib = _lib.load()
    nbytes = lib.rvc_minibatch_status_bytes()
    status = torch.empty(nbytes, dtype=torch.uint8, device=xb.device) if status is None else status
    if status.dtype != torch.uint8 or status.numel() < nbytes or not status.is_contiguous():
        raise ValueError(f"minibatch_inertia: status must be a contiguous uint8 [{nbytes}] tensor")
    need = lib.rvc_minibatch_inertia_work_bytes(n)
    if need < 0:
        raise ValueError(f"minibatch_inertia: bad size n={n}")
    ws = _workspace(xb.device, need, "minibatch")
    check(lib.rvc_minibatch_inertia(_p(xb), n, d, _p(cent), k, _p(assign), _p(weight_sums), _p(ws), need, _p(status),
                                    _stream()), "minibatch_inertia")
    return status


def minibatch_status(status):
    """The status block on the host (one synchronising read): (inertia, wmax, any_zero)."""
    s = status.cpu().numpy()[:MINIBATCH_STATUS.itemsize].view(MINIBATCH_STATUS)[0]
    return float(s["inertia"]), np.float32(s["wmax"]), bool(s["any_zero"])


def minibatch_scatter(xb, src, dst, value, cent, weight_sums):
    """cent[dst[i]] = xb[src[i]] and weight_sums[dst[i]] = value (int64 device src / dst, the dst distinct)."""
    (n, d), (k, dc) = _rows(xb, "minibatch_scatter"), _rows(cent, "minibatch_scatter")
    _weights(weight_sums, k, "minibatch_scatter")
    if dc != d or src.dtype != torch.int64 or dst.dtype != torch.int64 or src.dim() != 1 or \
            src.shape != dst.shape or not src.is_contiguous() or not dst.is_contiguous():
        raise ValueError("minibatch_scatter: src and dst must be contiguous int64 [m] tensors")
    check(_lib.load().rvc_minibatch_scatter(_p(xb), n, d, _p(src), _p(dst), src.numel(), float(value), _p(cent), k,
                                            _p(weight_sums), _stream()), "minibatch_scatter")
    return cent


def phone_upsample(feats, feats0, pitchf, out, C, Tf, T, protect):
    if feats.numel() < C * Tf or out.numel() < C * T or T > 2 * Tf or (pitchf is not None and pitchf.numel() < T):
        raise ValueError("phone_upsample: size mismatch")
    check(_lib.load().rvc_phone_upsample(_p(feats), _p(feats0), _p(pitchf), _p(out), C, Tf, T, protect, _stream()),
          "phone_upsample")
    return out


def peak_normalize(x, ws, scale_out=None):
    check(_lib.load().rvc_peak_normalize(_p(x), x.numel(), _p(ws), _p(scale_out), _stream()), "peak_normalize")
    return x


def change_rms(src, src64, out, hop, rate):
    """change_rms(audio, 16000, audio_opt, 16000, rate) (convert.py:150-152, :449) in place on the device
    output ``out`` [n]; src = the filtered 16 kHz input (f64 ``src64`` preferred, else f32 ``src``).
    The reference passes 16000 as both rates, so both envelopes use hop = 8000 (``hop``)."""
    lib = _lib.load()
    n_src = (src64 if src64 is not None else src).numel()
    n1, n2 = lib.rvc_rms_frames_len(n_src, hop), lib.rvc_rms_frames_len(out.numel(), hop)
    r1 = torch.empty(n1, device=out.device)
    r2 = torch.empty(n2, device=out.device)
    s64 = ctypes.c_void_p(src64.data_ptr()) if src64 is not None else None
    check(lib.rvc_rms_frames(s64, None if src64 is not None else _p(src), n_src, hop, _p(r1), _stream()),
          "rms_frames")
    check(lib.rvc_rms_frames(None, _p(out), out.numel(), hop, _p(r2), _stream()), "rms_frames")
    check(lib.rvc_rms_mix(_p(out), out.numel(), _p(r1), n1, _p(r2), n2, float(rate), _stream()), "rms_mix")
    return out


# ------------------------------------------------------------------ training forward (trainfwd.hip)
def spectrogram_frames(N, nfft, hop):
    """Frames of spectrogram_torch (train.py:700-706) on N samples; ValueError when N does not hold the reflect pad."""
    F = _lib.load().rvc_spectrogram_frames(N, nfft, hop)
    if F <= 0:
        raise ValueError(f"spectrogram: {N} samples do not hold the reflect pad of n_fft {nfft}, hop {hop}")
    return F


_HANN = {}


def hann_window(nfft, device):
    """The reference's window: torch.hann_window(nfft) (periodic, computed in f32 on the host), uploaded once."""
    key = (nfft, str(device))
    if key not in _HANN:
        _HANN[key] = torch.hann_window(nfft, dtype=torch.float32).to(device)
    return _HANN[key]


def spectrogram(x, nfft, hop, out=None):
    """x [B][N] (or [N]) f32 -> spec [B][nfft/2+1][F] = sqrt(|STFT|^2 + 1e-6) (rvc_spectrogram)."""
    x2 = x.reshape(1, -1) if x.dim() == 1 else x
    if x2.dim() != 2 or not x2.is_contiguous():
        raise ValueError("spectrogram: x must be contiguous [B][N]")
    win = hann_window(nfft, x.device)
    B, N = x2.shape
    F = spectrogram_frames(N, nfft, hop)
    K = nfft // 2 + 1
    if out is None:
        out = torch.empty(B, K, F, device=x.device, dtype=torch.float32)
    elif out.numel() < B * K * F or not out.is_contiguous():
        raise ValueError("spectrogram: output buffer too small")
    check(_lib.load().rvc_spectrogram(_p(x2), _p(win), _p(out), B, N, F, nfft, hop, _stream()), "spectrogram")
    return out


def mel_log(spec, basis, out=None):
    """spec [B][K][F], basis [M][K] -> log(max(basis @ spec, 1e-5)) [B][M][F] (rvc_mel_log)."""
    if spec.dim() != 3 or basis.dim() != 2 or not spec.is_contiguous() or not basis.is_contiguous():
        raise ValueError("mel_log: spec must be contiguous [B][K][F] and basis contiguous [M][K]")
    B, K, F = spec.shape
    M = basis.shape[0]
    if basis.shape[1] != K:
        raise ValueError(f"mel_log: basis has {basis.shape[1]} bins, spec {K}")
    if out is None:
        out = torch.empty(B, M, F, device=spec.device, dtype=torch.float32)
    elif out.numel() < B * M * F or not out.is_contiguous():
        raise ValueError("mel_log: output buffer too small")
    check(_lib.load().rvc_mel_log(_p(spec), _p(basis), _p(out), B, M, K, F, _stream()), "mel_log")
    return out


def _loss_work(device):
    n = _lib.load().rvc_trainfwd_work_bytes()
    return torch.empty(n // 4, device=device, dtype=torch.float32), n


def slice_l1(mel, ids, yhat_mel):
    """F.l1_loss(slice_segments(mel, ids, S), yhat_mel): mel [B][M][T], ids int64 [B] (device), yhat_mel [B][M][S] ->
    a device f32 scalar [1] (rvc_slice_l1: fixed-order f64 sum)."""
    if mel.dim() != 3 or yhat_mel.dim() != 3 or not mel.is_contiguous() or not yhat_mel.is_contiguous():
        raise ValueError("slice_l1: mel [B][M][T] and yhat_mel [B][M][S] must be contiguous")
    B, M, T = mel.shape
    S = yhat_mel.shape[2]
    if yhat_mel.shape[:2] != (B, M) or S > T or ids.dtype != torch.int64 or ids.numel() != B:
        raise ValueError("slice_l1: shape mismatch")
    work, nb = _loss_work(mel.device)
    out = torch.empty(1, device=mel.device, dtype=torch.float32)
    check(_lib.load().rvc_slice_l1(_p(mel), _p(ids), _p(yhat_mel), B, M, T, S, _p(work), nb, _p(out), _stream()),
          "slice_l1")
    return out


def kl_loss(z_p, logs_q, m_p, logs_p):
    """kl_loss(z_p, logs_q, m_p, logs_p, ones) (train.py:317-325) over [B][C][T] -> a device f32 scalar [1].  m_p and
    logs_p may be the two halves of stacked statistics [B][2C][T] (views with batch stride 2 * C * T)."""
    B, C, T = z_p.shape
    for t in (logs_q, m_p, logs_p):
        if tuple(t.shape) != (B, C, T) or t.stride(2) != 1 or t.stride(1) != T:
            raise ValueError("kl_loss: operands must be [B][C][T] with contiguous rows")
    if not z_p.is_contiguous() or m_p.stride(0) != logs_p.stride(0):
        raise ValueError("kl_loss: z_p must be contiguous, m_p and logs_p share a batch stride")
    work, nb = _loss_work(z_p.device)
    out = torch.empty(1, device=z_p.device, dtype=torch.float32)
    qs = logs_q.stride(0) if B > 1 else 0
    ps = m_p.stride(0) if B > 1 else 0
    check(_lib.load().rvc_kl_loss(_p(z_p), _p(logs_q), _p(m_p), _p(logs_p), B, C, T, qs, ps, _p(work), nb, _p(out),
                                  _stream()), "kl_loss")
    return out


# ------------------------------------------------------------------ discriminators and GAN losses (discriminator.hip)
def period_front_rows(t, p):
    """Rows H1 of DiscriminatorP's first feature map on t samples; ValueError when the reflect pad does not fit."""
    H1 = _lib.load().rvc_period_front_rows(t, p)
    if H1 <= 0:
        raise ValueError(f"period_front: {t} samples do not hold the reflect pad of period {p}")
    return H1


def period_front(y, w, bias, p, slope=0.1, out=None):
    """y [S][t] (or [t]) -> [S * p][32][H1]: reflect pad, [H][p] view, Conv2d(1, 32, (5,1), (3,1), (2,0)) with w [32][5]
    and bias [32], LeakyReLU -- column c of signal s is batch element s * p + c (rvc_period_front)."""
    y2 = y.reshape(1, -1) if y.dim() == 1 else y
    if y2.dim() != 2 or not y2.is_contiguous():
        raise ValueError("period_front: y must be contiguous [S][t]")
    if w.numel() != 32 * 5 or bias.numel() != 32 or not w.is_contiguous():
        raise ValueError("period_front: w must be [32][5] and bias [32]")
    S, t = y2.shape
    H1 = period_front_rows(t, p)
    if out is None:
        out = torch.empty(S * p, 32, H1, device=y.device, dtype=torch.float32)
    elif out.numel() < S * p * 32 * H1 or not out.is_contiguous():
        raise ValueError("period_front: output buffer too small")
    check(_lib.load().rvc_period_front(_p(y2), _p(w), _p(bias), _p(out), S, t, p, H1, slope, _stream()),
          "period_front")
    return out


def gconv_small(x, w, bias, slope=0.1, out=None):
    """Conv1d(Ci, Co, 41, 4, groups=Ci / 4, padding=20) + bias + LeakyReLU: x [B][Ci][Lin], w [Co][4][41] ->
    [B][Co][(Lin - 1) // 4 + 1] (rvc_gconv_small)."""
    if x.dim() != 3 or not x.is_contiguous() or w.dim() != 3 or not w.is_contiguous():
        raise ValueError("gconv_small: x must be contiguous [B][Ci][Lin] and w contiguous [Co][4][41]")
    B, Ci, Lin = x.shape
    Co = w.shape[0]
    if tuple(w.shape[1:]) != (4, 41) or Ci % 4 or Co * 4 not in (16 * Ci, 4 * Ci) or bias.numel() != Co:
        raise ValueError(f"gconv_small: {Ci} -> {Co} channels with weight {tuple(w.shape)} is not one of its layers")
    Lout = (Lin - 1) // 4 + 1
    if out is None:
        out = torch.empty(B, Co, Lout, device=x.device, dtype=torch.float32)
    elif out.numel() < B * Co * Lout or not out.is_contiguous():
        raise ValueError("gconv_small: output buffer too small")
    check(_lib.load().rvc_gconv_small(_p(x), _p(w), _p(bias), _p(out), B, Ci, Co, Lin, Lout, slope, _stream()),
          "gconv_small")
    return out


def _pd64(t):
    if not t.is_cuda or t.dtype != torch.float64:
        raise TypeError(f"rvc_amd: expected a CUDA f64 tensor, got {t.dtype} on {t.device}")
    return ctypes.c_void_p(t.data_ptr())


def disc_work(device):
    """The reductions' stage-1 scratch (rvc_disc_work_bytes) -> (f64 buffer, bytes); calls on one stream may share it."""
    n = _lib.load().rvc_disc_work_bytes()
    return torch.empty(n // 8, device=device, dtype=torch.float64), n


def disc_table(n_fm, n_disc, device):
    """The f64 table rvc_disc_finish sums: n_fm feature-map terms, then (r, g, gen) per discriminator."""
    return torch.zeros(_lib.load().rvc_disc_table_slots(n_fm, n_disc), device=device, dtype=torch.float64)


def _flat_pair(a, b, what):
    if a.numel() != b.numel() or a.numel() == 0 or not a.is_contiguous() or not b.is_contiguous():
        raise ValueError(f"{what}: two contiguous tensors of one size, not {tuple(a.shape)} and {tuple(b.shape)}")
    return a.numel()


def pair_l1(a, b, table, slot, work=None):
    """table[slot] = mean |a - b| (rvc_pair_l1: fixed-order f64 sum)."""
    n = _flat_pair(a, b, "pair_l1")
    if not 0 <= slot < table.numel():
        raise ValueError(f"pair_l1: slot {slot} outside a table of {table.numel()}")
    work, nb = (work, work.numel() * 8) if work is not None else disc_work(a.device)
    check(_lib.load().rvc_pair_l1(_p(a), _p(b), n, _pd64(table), slot, _pd64(work), nb, _stream()), "pair_l1")
    return table


def lsgan_terms(d_r, d_g, table, slot, work=None):
    """table[slot : slot + 3] = mean (1 - d_r)^2, mean d_g^2, mean (1 - d_g)^2 (rvc_lsgan_terms)."""
    n = _flat_pair(d_r, d_g, "lsgan_terms")
    if not 0 <= slot <= table.numel() - 3:
        raise ValueError(f"lsgan_terms: slots {slot}..{slot + 2} outside a table of {table.numel()}")
    work, nb = (work, work.numel() * 8) if work is not None else disc_work(d_r.device)
    check(_lib.load().rvc_lsgan_terms(_p(d_r), _p(d_g), n, _pd64(table), slot, _pd64(work), nb, _stream()),
          "lsgan_terms")
    return table


DISC_OUT_LISTS = 6  # RVC_DISC_OUT_LISTS


def disc_finish(table, n_fm, n_disc, l1=None, c_mel=1.0, kl=None, c_kl=1.0):
    """The reference's f32 sums over the table -> device f32 [6 + 3 * n_disc]: loss_disc, loss_gen, loss_fm,
    loss_gen_all, loss_mel, loss_kl (the last three NaN without the device scalars ``l1`` and ``kl``), then losses_gen,
    losses_disc_r, losses_disc_g (rvc_disc_finish)."""
    if table.numel() < n_fm + 3 * n_disc:
        raise ValueError("disc_finish: table too small")
    if (l1 is None) != (kl is None):
        raise ValueError("disc_finish: loss_mel and loss_kl go together")
    out = torch.empty(DISC_OUT_LISTS + 3 * n_disc, device=table.device, dtype=torch.float32)
    check(_lib.load().rvc_disc_finish(_pd64(table), n_fm, n_disc, _p(l1), c_mel, _p(kl), c_kl, _p(out), _stream()),
          "disc_finish")
    return out


# ------------------------------------------------------------------ the discriminator's step (disc_backward.hip)
def lsgan_grad(d, scale=1.0, out=None):
    """The gradient of discriminator_loss on one discriminator's conv_post map d (real half first, 2 n values) times
    ``scale``: -2 (1 - d_r) / n and 2 d_g / n, in d's shape (rvc_lsgan_grad)."""
    if d.numel() == 0 or d.numel() % 2 or not d.is_contiguous():
        raise ValueError(f"lsgan_grad: a contiguous map of two halves, not {tuple(d.shape)}")
    if out is None:
        out = torch.empty_like(d)
    check(_lib.load().rvc_lsgan_grad(_p(d), _p(out), d.numel() // 2, scale, _stream()), "lsgan_grad")
    return out


def _bwd_shapes(what, dy, y, w, groups, stride, pad, Lin):
    if dy.dim() != 3 or w.dim() != 3 or not dy.is_contiguous() or not w.is_contiguous():
        raise ValueError(f"{what}: dy must be contiguous [B][Co][Lout] and w contiguous [Co][Ci / groups][K]")
    if y is not None and (tuple(y.shape) != tuple(dy.shape) or not y.is_contiguous()):
        raise ValueError(f"{what}: the stored output must have dy's shape {tuple(dy.shape)}")
    B, Co, Lout = dy.shape
    if w.shape[0] != Co or Co % groups:
        raise ValueError(f"{what}: weight {tuple(w.shape)} against dy {tuple(dy.shape)} in {groups} groups")
    Ci, K = w.shape[1] * groups, w.shape[2]
    if Lin + 2 * pad < K or (Lin + 2 * pad - K) // stride + 1 != Lout:
        raise ValueError(f"{what}: Lin = {Lin} does not give Lout = {Lout} (k {K}, stride {stride}, pad {pad})")
    return B, Ci, Co, Lout, K


def conv_bwd_data(dy, y, w, Lin, stride=1, pad=0, groups=1, slope=0.1, out=None):
    """dx [B][Ci][Lin] of a Conv1d with weight w [Co][Ci / groups][K] from dy [B][Co][Lout] and the stored output y of the
    layer that produced dy (LeakyReLU factor taken on load; None: no activation) (rvc_conv_bwd_data)."""
    B, Ci, Co, Lout, K = _bwd_shapes("conv_bwd_data", dy, y, w, groups, stride, pad, Lin)
    if out is None:
        out = torch.empty(B, Ci, Lin, device=dy.device, dtype=torch.float32)
    elif out.numel() < B * Ci * Lin or not out.is_contiguous():
        raise ValueError("conv_bwd_data: output buffer too small")
    check(_lib.load().rvc_conv_bwd_data(_p(dy), _p(y), _p(w), _p(out), B, Ci, Co, Lin, Lout, K, stride, pad, groups,
                                        slope, _stream()), "conv_bwd_data")
    return out


def conv_bwd_weight_work(B, Ci, Co, Lout, K, groups=1):
    """Bytes of chunk partials rvc_conv_bwd_weight would like for this layer."""
    n = _lib.load().rvc_conv_bwd_weight_work_bytes(B, Ci, Co, Lout, K, groups)
    if n <= 0:
        raise ValueError("conv_bwd_weight: bad sizes")
    return n


def conv_bwd_weight(dy, y, x, dW, db, stride=1, pad=0, groups=1, slope=0.1, scale=1.0, accumulate=False, period=0,
                    work=None):
    """dW [Co][Ci / groups][K] and db [Co] (+)= scale * the weight and bias gradient of a Conv1d from dy [B][Co][Lout],
    the stored output y (as ``conv_bwd_data``) and the layer's input x [B][Ci][Lin]; ``period`` > 0: x is the signals
    [S][t] as DiscriminatorP's first conv views them, B = S * period (rvc_conv_bwd_weight)."""
    if not x.is_contiguous() or not dW.is_contiguous() or not db.is_contiguous():
        raise ValueError("conv_bwd_weight: x, dW and db must be contiguous")
    if period > 0:
        if x.dim() != 2 or dy.dim() != 3 or x.shape[0] * period != dy.shape[0]:
            raise ValueError(f"conv_bwd_weight: signals {tuple(x.shape)} at period {period} against dy {tuple(dy.shape)}")
        t = x.shape[1]
        Lin = (t + (period - t % period) % period) // period
    else:
        if x.dim() != 3 or dy.dim() != 3 or x.shape[0] != dy.shape[0] or x.shape[1] != dW.shape[1] * groups:
            raise ValueError(f"conv_bwd_weight: x {tuple(x.shape)} against dy {tuple(dy.shape)}, dW {tuple(dW.shape)}")
        t, Lin = 0, x.shape[2]
    B, Ci, Co, Lout, K = _bwd_shapes("conv_bwd_weight", dy, y, dW, groups, stride, pad, Lin)
    if db.numel() != Co:
        raise ValueError("conv_bwd_weight: db must be [Co]")
    if work is None:
        work = torch.empty(conv_bwd_weight_work(B, Ci, Co, Lout, K, groups), device=dy.device, dtype=torch.uint8)
    if work.numel() * work.element_size() < dW.numel() * 4:
        raise ValueError("conv_bwd_weight: work buffer too small")
    check(_lib.load().rvc_conv_bwd_weight(_p(dy), _p(y), _p(x), _p(dW), _p(db), B, Ci, Co, Lin, Lout, K, stride, pad,
                                          groups, slope, scale, int(accumulate), period, t,
                                          ctypes.c_void_p(work.data_ptr()), work.numel() * work.element_size(),
                                          _stream()), "conv_bwd_weight")
    return dW, db


def wn_adamw(dW, db, v, g, bias, state, table, lr, betas, eps, weight_decay, step):
    """Weight-norm backward, the rows' squared gradient norms into ``table`` [Co][3] (f64) and torch.optim.AdamW's
    update of g, v and bias in place; ``state`` = (m_v, s_v, m_g, s_g, m_b, s_b), ``step`` counting from 1
    (rvc_wn_adamw)."""
    Co = g.numel()
    n = v.numel() // Co
    m_v, s_v, m_g, s_g, m_b, s_b = state
    for a, size in ((dW, Co * n), (v, Co * n), (m_v, Co * n), (s_v, Co * n), (db, Co), (bias, Co), (m_g, Co), (s_g, Co),
                    (m_b, Co), (s_b, Co), (g, Co)):
        if a.numel() != size or not a.is_contiguous() or a.dtype != torch.float32:
            raise ValueError(f"wn_adamw: a tensor of {a.numel()} values where {size} contiguous f32 belong")
    if table.numel() < 3 * Co or not table.is_contiguous():
        raise ValueError("wn_adamw: the table holds three values per row")
    check(_lib.load().rvc_wn_adamw(_p(dW), _p(db), _p(v), _p(g), _p(bias), _p(m_v), _p(s_v), _p(m_g), _p(s_g), _p(m_b),
                                   _p(s_b), Co, n, lr, betas[0], betas[1], eps, weight_decay, step, _pd64(table),
                                   _stream()), "wn_adamw")


def grad_norm(table, work=None):
    """sqrt of the sum of an f64 table of squared norms -> device f64 [1] (rvc_grad_norm)."""
    if not table.is_contiguous():
        raise ValueError("grad_norm: table must be contiguous")
    work, nb = (work, work.numel() * 8) if work is not None else disc_work(table.device)
    out = torch.empty(1, device=table.device, dtype=torch.float64)
    check(_lib.load().rvc_grad_norm(_pd64(table), table.numel(), _pd64(out), _pd64(work), nb, _stream()), "grad_norm")
    return out


SQRT = math.sqrt

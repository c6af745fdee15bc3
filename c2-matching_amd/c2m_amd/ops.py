"""Tensor-level entry points of the MI355X hot path (PyTorch is plumbing only: memory, streams).

Every function takes CUDA(=HIP) float32 tensors, enqueues hand-written gfx950 kernels from libc2m_hip.so on the
current torch stream and returns freshly allocated tensors.  CPU tensors are rejected: there is no fallback path.
"""
import collections
import ctypes
import os
import threading
import warnings
import weakref

import torch

from . import _lib


def _dev_f32(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.C2MError(f"{name} must be a tensor on the GPU (the HIP path has no CPU fallback)")
    if t.dtype != torch.float32:
        raise _lib.C2MError(f"{name} must be float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


class NormalizedFeatures(torch.Tensor):
    """What `feature_normalize(x, with_sumsq=True)` returns: the normalised map (an ordinary tensor to every consumer) that also
    carries `.c2m_sumsq` -- its per-pixel sums of squares [B, H*W], formed by the normalisation kernel while the values were in
    registers.  `feature_match_index_batched` hands them to the library instead of launching a pass over each map; anything
    derived from the tensor (a slice, a copy, arithmetic) is a plain tensor again and simply loses the shortcut."""

    @staticmethod
    def wrap(t, ss):
        r = t.as_subclass(NormalizedFeatures)
        r.c2m_sumsq = ss
        r.c2m_version = r._version      # (an in-place write to the map bumps _version: the sums are then stale and are not used)
        return r

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **(kwargs or {}))


def feature_normalize(x, with_sumsq=False):
    """x [B,C,H,W] or [C,H,W] -> per-pixel channel-normalised copy (corres_generation_arch.py:56-58).  with_sumsq: the result is a
    NormalizedFeatures (same values; carries the per-pixel sums of squares for feature_match_index_batched)."""
    x = _dev_f32(x, "x")
    shp = x.shape
    xb = x.view(1, *shp) if x.dim() == 3 else x
    B, C = xb.shape[0], xb.shape[1]
    out = torch.empty_like(xb)
    HW = xb.numel() // (B * C)
    ss = torch.empty((B, HW), dtype=torch.float32, device=x.device) if with_sumsq else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().c2m_feature_normalize_ss_f32(_stream(), xb.data_ptr(), B, C, HW, out.data_ptr(),
                                                           ss.data_ptr() if ss is not None else None), "c2m_feature_normalize_ss_f32")
    out = out.view(shp)
    return NormalizedFeatures.wrap(out, ss) if with_sumsq else out


def _pre_sumsq(t, B, HW):
    """The sums of squares a NormalizedFeatures carries, if `t` still IS that very tensor (same storage, shape, contiguous)."""
    ss = getattr(t, "c2m_sumsq", None) if isinstance(t, NormalizedFeatures) else None
    if ss is None or not t.is_contiguous() or tuple(ss.shape) != (B, HW) or ss.device != t.device or t._version != getattr(t, "c2m_version", -1):
        return None
    return ss


_CORR_FORCE_GENERIC, _CORR_EXACT_SWEEP = 1, 2   # c2m_hip.h C2M_CORR_*: the `flags` word of the correlation entry points


def feature_match_index_batched(feat_in, feat_ref, patch_size=3, input_stride=1, ref_stride=1, is_norm=True,
                                norm_input=False, force_generic=False, return_skip=False, exact_sweep=None):
    """Batched ref_map_util.feature_match_index: feat_in [B,C,Hq,Wq], feat_ref [B,C,Hr,Wr] ->
    (max_idx int64 [B,Hqp,Wqp], max_val float32 [B,Hqp,Wqp]).  exact_sweep=True skips the f16 pre-filter and runs the exact
    fp32 sweep only (identical results), False uses the pre-filter, None follows an open `corr_filter_mode` block (else the
    pre-filter).  return_skip=True appends the MFMA kernel's duplicate-row
    table, int32 [B, x_tiles, 2] = (from, to) per (sample, ref x-tile) (c2m_feature_match_skip_table; diagnostics)."""
    fi, fr = _dev_f32(feat_in, "feat_in"), _dev_f32(feat_ref, "feat_ref")
    if fi.dim() != 4 or fr.dim() != 4 or fi.shape[:2] != fr.shape[:2] or fi.device != fr.device:
        raise _lib.C2MError("feat_in / feat_ref must be [B,C,H,W] with equal B, C and device")
    B, C, Hq, Wq = fi.shape
    Hr, Wr = fr.shape[2:]
    p, si, sr = int(patch_size), int(input_stride), int(ref_stride)
    if min(Hq, Wq, Hr, Wr) < p:
        raise _lib.C2MError("feature maps smaller than the patch")
    Hqp, Wqp = (Hq - p) // si + 1, (Wq - p) // si + 1
    L = _lib.lib()
    if exact_sweep is None:
        exact_sweep = _corr_exact_sweep   # (read here, on the launching thread: corr_filter_mode)
    flags = (_CORR_FORCE_GENERIC if force_generic else 0) | (_CORR_EXACT_SWEEP if exact_sweep else 0)
    with torch.cuda.device(fi.device):
        nbytes = L.c2m_feature_match_workspace_bytes_c(B, C, Hq, Wq, Hr, Wr)   # (sized by the maps' channels: ADVICE r4)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=fi.device)
        idx = torch.empty((B, Hqp, Wqp), dtype=torch.int64, device=fi.device)
        val = torch.empty((B, Hqp, Wqp), dtype=torch.float32, device=fi.device)
        ss_i, ss_r = _pre_sumsq(feat_in, B, Hq * Wq), _pre_sumsq(feat_ref, B, Hr * Wr)
        _lib.check(L.c2m_feature_match_index_pre_f32(_stream(), fi.data_ptr(), fr.data_ptr(), B, C, Hq, Wq, Hr, Wr, p, si,
                                                     sr, int(bool(is_norm)), int(bool(norm_input)), flags,
                                                     idx.data_ptr(), val.data_ptr(), ws.data_ptr(), nbytes,
                                                     ss_i.data_ptr() if ss_i is not None else None,
                                                     ss_r.data_ptr() if ss_r is not None else None),
                   "c2m_feature_match_index_pre_f32")
        mfma = not (flags & _CORR_FORCE_GENERIC) and p == 3 and si == 1 and sr == 1 and C in (64, 128, 256)   # restates mfma_channels() of csrc/corr_filter.h
        if return_skip or _corr_diag.enabled:
            # diagnostics only (bench.py's swept-row count, the dedup tests): the duplicate-row table exists only when the
            # MFMA kernel ran; nothing is kept otherwise, so the workspace dies with the call and no module state is
            # touched on the product path (DataParallel replicas run this function concurrently)
            table = _skip_table(ws, (B, Hq, Wq, Hr, Wr)) if mfma else None
            if _corr_diag.enabled:
                _corr_diag.table = table
                _corr_diag.filter = _filter_tables(ws, (B, Hq, Wq, Hr, Wr), Hqp * Wqp) if mfma else None
            if return_skip:
                if table is None:
                    raise _lib.C2MError("return_skip: the duplicate-row table exists only on the MFMA kernel's path "
                                        "(patch 3, strides 1, C in 64/128/256, force_generic=False)")
                return idx, val, table
    return idx, val


class _CorrDiag:
    """Opt-in diagnostics of the correlation launch: `with ops.record_corr_skip_table(): ...` keeps the duplicate-row table
    of the most recent MFMA launch inside the block (a small int32 tensor, not the workspace) and the pre-filter's
    candidate counts / flags."""
    enabled = False
    table = None
    filter = None


_corr_diag = _CorrDiag()


class record_corr_skip_table:
    def __enter__(self):
        _corr_diag.enabled, _corr_diag.table, _corr_diag.filter = True, None, None
        return self

    def __exit__(self, *exc):
        _corr_diag.enabled = False
        return False


def _skip_table(ws, shp):
    off, nxt = ctypes.c_size_t(0), ctypes.c_int(0)
    _lib.check(_lib.lib().c2m_feature_match_skip_table(*shp, ctypes.byref(off), ctypes.byref(nxt)),
               "c2m_feature_match_skip_table")
    B = shp[0]
    return ws[off.value:off.value + 8 * B * nxt.value].view(torch.int32).view(B, nxt.value, 2).clone()


def _filter_tables(ws, shp, nq):
    c, k, f, slots = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_int(0)
    _lib.check(_lib.lib().c2m_feature_match_filter_tables(*shp, ctypes.byref(c), ctypes.byref(k), ctypes.byref(f),
                                                          ctypes.byref(slots)), "c2m_feature_match_filter_tables")
    B, K = shp[0], slots.value
    return {"cnt": ws[c.value:c.value + 4 * B * nq].view(torch.int32).view(B, nq).clone(),
            "cand": ws[k.value:k.value + 4 * B * nq * K].view(torch.int32).view(B, nq, K).clone(),
            "flags": ws[f.value:f.value + 32].view(torch.int32).clone()}


def last_corr_filter_tables():
    """Pre-filter diagnostics recorded under `record_corr_skip_table()`: {'cnt': int32 [B, Nq] candidates per query (-1 =
    every ref patch re-scored), 'cand': int32 [B, Nq, slots], 'flags': int32 [8] ([0] != 0: the exact sweep produced the
    result)} -- meaningful only if the most recent launch took the pre-filter path (c2m_feature_match_filter_tables)."""
    if _corr_diag.filter is None:
        raise _lib.C2MError("no MFMA correlation launch was recorded (use `with ops.record_corr_skip_table():`)")
    return _corr_diag.filter


_corr_exact_sweep = False   # what `exact_sweep=None` means; corr_filter_mode saves, sets and restores it


class corr_filter_mode:
    """`with ops.corr_filter_mode(0): ...` -- exact fp32 sweep only; (1): pre-filter + exact re-score (default); results are
    identical (C2M_CORR_EXACT_SWEEP).  The default of feature_match_index_batched's `exact_sweep` for every thread's launches
    through this module while the block is open (measurement / tests); an explicit `exact_sweep=` wins."""

    def __init__(self, mode):
        self.mode = int(mode)
        if self.mode not in (0, 1):
            raise _lib.C2MError("corr_filter_mode: 0 or 1")

    def __enter__(self):
        global _corr_exact_sweep
        self.prev, _corr_exact_sweep = _corr_exact_sweep, self.mode == 0
        return self

    def __exit__(self, *exc):
        global _corr_exact_sweep
        _corr_exact_sweep = self.prev
        return False


def last_corr_skip_table():
    """Duplicate-row table recorded under `record_corr_skip_table()`: int32 [B, x_tiles, 2] = (from, to), ref rows
    [from, to) of that (sample, x-tile) were not swept (c2m_feature_match_skip_table).  Diagnostics / bench only."""
    if _corr_diag.table is None:
        raise _lib.C2MError("no MFMA correlation launch was recorded (use `with ops.record_corr_skip_table():`)")
    return _corr_diag.table


def build_pre_offsets(max_idx, h, w, scales=(1, 2, 4)):
    """max_idx int64 [B,h-2,w-2] -> tuple of pre-offset tensors [B,9,s*h,s*w,2] for s in scales (subset of 1,2,4)."""
    if not max_idx.is_cuda or max_idx.dtype != torch.int64:
        raise _lib.C2MError("max_idx must be an int64 GPU tensor")
    mi = max_idx.contiguous()
    B = mi.shape[0]
    if tuple(mi.shape[1:]) != (h - 2, w - 2):
        raise _lib.C2MError("max_idx must be [B, h-2, w-2]")
    if not set(scales) <= {1, 2, 4} or len(set(scales)) != len(tuple(scales)):
        raise _lib.C2MError(f"scales must be distinct members of (1, 2, 4), got {tuple(scales)}")
    outs = {s: torch.empty((B, 9, h * s, w * s, 2), dtype=torch.float32, device=mi.device) for s in scales}
    ptr = lambda s: outs[s].data_ptr() if s in outs else None  # noqa: E731
    with torch.cuda.device(mi.device):
        _lib.check(_lib.lib().c2m_build_pre_offsets_f32(_stream(), mi.data_ptr(), B, h, w, ptr(1), ptr(2), ptr(4)),
                   "c2m_build_pre_offsets_f32")
    return tuple(outs[s] for s in scales)


def _dcn_geom(inp, weight, stride, padding, dilation):
    B, C, H, W = inp.shape
    Co, Ck, kh, kw = weight.shape
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    if Ck != C:
        raise _lib.C2MError(f"Input shape and kernel channels wont match: ({C} vs {Ck}).")
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    return (B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw), Ho, Wo


def _check_offset_mask(offset, mask, B, dg, taps, Ho, Wo, names):
    """The planar offset / mask pair of a DCNv2 call; `names`: how the caller's message spells taps, Ho and Wo."""
    if tuple(offset.shape) != (B, 2 * dg * taps, Ho, Wo) or tuple(mask.shape) != (B, dg * taps, Ho, Wo):
        raise _lib.C2MError("offset/mask shape does not match [B, 2*dg*{0}, {1}, {2}] / [B, dg*{0}, {1}, {2}]".format(*names))


def dcn_v2_forward(inp, weight, bias, offset, mask, stride=1, padding=1, dilation=1, deformable_groups=1,
                   bf16_mma=False):
    """bf16_mma=True: the implicit GEMM runs on bf16 MFMA with fp32 accumulation (weights and blended samples rounded to
    bf16); tensors stay float32.  For callers that asked for reduced precision (bf16 autocast), not the default."""
    inp, weight, bias, offset, mask = (_dev_f32(t, n) for t, n in
                                       ((inp, "input"), (weight, "weight"), (bias, "bias"), (offset, "offset"), (mask, "mask")))
    g, Ho, Wo = _dcn_geom(inp, weight, stride, padding, dilation)
    B, C, H, W, Co, kh, kw = g[:7]
    dg = int(deformable_groups)
    _check_offset_mask(offset, mask, B, dg, kh * kw, Ho, Wo, ("kh*kw", "Ho", "Wo"))
    L = _lib.lib()
    with torch.cuda.device(inp.device):
        nbytes = L.c2m_dcn_v2_forward_workspace_bytes(B, C, H, W, Co, kh, kw, dg)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=inp.device)
        out = torch.empty((B, Co, Ho, Wo), dtype=torch.float32, device=inp.device)
        fn = L.c2m_dcn_v2_forward_bf16mma_f32 if bf16_mma else L.c2m_dcn_v2_forward_f32
        _lib.check(fn(_stream(), inp.data_ptr(), weight.data_ptr(), bias.data_ptr(), offset.data_ptr(), mask.data_ptr(),
                      *g, dg, out.data_ptr(), ws.data_ptr(), nbytes), "c2m_dcn_v2_forward")
    return out


def dcn_v2_backward(inp, weight, bias, offset, mask, grad_output, stride=1, padding=1, dilation=1, deformable_groups=1,
                    need_input_grad=True):
    """-> (grad_input or None, grad_offset, grad_mask, grad_weight, grad_bias)."""
    inp, weight, bias, offset, mask, grad_output = (_dev_f32(t, n) for t, n in (
        (inp, "input"), (weight, "weight"), (bias, "bias"), (offset, "offset"), (mask, "mask"), (grad_output, "grad_output")))
    g, Ho, Wo = _dcn_geom(inp, weight, stride, padding, dilation)
    dg = int(deformable_groups)
    L = _lib.lib()
    with torch.cuda.device(inp.device):
        nbytes = L.c2m_dcn_v2_backward_workspace_bytes(*g, dg)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=inp.device)
        go, gm, gw, gb = (torch.empty_like(t) for t in (offset, mask, weight, bias))
        gi = torch.empty_like(inp) if need_input_grad else None
        _lib.check(L.c2m_dcn_v2_backward_f32(_stream(), inp.data_ptr(), weight.data_ptr(), bias.data_ptr(),
                                             offset.data_ptr(), mask.data_ptr(), grad_output.data_ptr(), *g, dg,
                                             gi.data_ptr() if gi is not None else None, go.data_ptr(), gm.data_ptr(),
                                             gw.data_ptr(), gb.data_ptr(),
                                             ws.data_ptr(), nbytes), "c2m_dcn_v2_backward_f32")
    return gi, go, gm, gw, gb


def dcn_fuse_offsets(conv_out, pre_offset, deformable_groups, kernel_taps, abs_sum=None):
    """conv_offset_mask output [B,3*dg*K,H,W] (+ pre_offset [B,K,H,W,2] or None) -> (offset [B,2*dg*K,H,W], mask
    [B,dg*K,H,W]) as dcn_v2.py:229-245 builds them; abs_sum (float64 GPU tensor of 256 slots, zeroed by the caller) accumulates sum|learned offset| across its slots."""
    conv_out = _dev_f32(conv_out, "conv_out")
    B, C3, H, W = conv_out.shape
    dg, K = int(deformable_groups), int(kernel_taps)
    if C3 != 3 * dg * K:
        raise _lib.C2MError("conv_out must have 3*dg*K channels")
    if pre_offset is not None:
        pre_offset = _dev_f32(pre_offset, "pre_offset")
        if tuple(pre_offset.shape) != (B, K, H, W, 2):
            raise _lib.C2MError("pre_offset must be [B, K, H, W, 2]")
    _check_abs_sum(abs_sum)
    offset = torch.empty((B, 2 * dg * K, H, W), dtype=torch.float32, device=conv_out.device)
    mask = torch.empty((B, dg * K, H, W), dtype=torch.float32, device=conv_out.device)
    with torch.cuda.device(conv_out.device):
        _lib.check(_lib.lib().c2m_dcn_fuse_offsets_f32(_stream(), conv_out.data_ptr(),
                                                       pre_offset.data_ptr() if pre_offset is not None else None,
                                                       B, dg, K, H, W, offset.data_ptr(), mask.data_ptr(),
                                                       abs_sum.data_ptr() if abs_sum is not None else None),
                   "c2m_dcn_fuse_offsets_f32")
    return offset, mask


# ---------------------------------------------------------------------------------------------------------------------
# 3x3 convolution, channels-last, fused epilogue (csrc/conv3x3.hip)
# ---------------------------------------------------------------------------------------------------------------------
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2

# Kernel kinds = weight-cache slot keys.  The seven conv3x3 kinds are the rows of _KINDS (ALGO_IDS maps the public algo= names
# to them); the two DCNv2 images share the slot shape (id, rows, kind) but have no row.
K_DIRECT, K_WINO, K_WINO4, K_SPLIT, K_BF16, K_DGRAD, K_SPLIT16 = range(7)
K_DCN, K_DCN16 = "dcn", "dcn16"
# One row per conv3x3 kind: public algo= name (K_DGRAD, the data-gradient image of the bf16 x 3 kernel, has none),
# c2m_conv3x3_desc.algo, family name of the flop counters (conv_flops_by_family), matrix flops executed per algorithmic
# (direct-convolution) flop, pieces of its split image (0: not a split image), the C-ABI's size / re-layout entry points and
# whether Cin and Cout swap roles in the image (the data-gradient convolution maps dY's Cout channels to dX's Cin)
_Kind = collections.namedtuple("_Kind", "name algo family exec_factor pieces size_fn relayout_fn swap")
_SPLIT_IMAGE = ("c2m_conv3x3_relayout_split_bytes", "c2m_conv3x3_relayout_split_f32", False)
_KINDS = {
    K_DIRECT: _Kind("direct", 0, "direct", 1.0, 0, "c2m_conv3x3_relayout_bytes", "c2m_conv3x3_relayout_f32", False),
    K_WINO: _Kind("winograd", 1, "winograd_f23", 2.0 / 3.0, 0, "c2m_conv3x3_relayout_wino_bytes", "c2m_conv3x3_relayout_wino_f32", False),
    K_WINO4: _Kind("winograd4", 2, "winograd_f43", 0.5, 0, "c2m_conv3x3_relayout_wino4_bytes", "c2m_conv3x3_relayout_wino4_f32", False),
    K_SPLIT: _Kind("split", 3, "split_bf16x3", 6.0, 3, *_SPLIT_IMAGE),
    K_BF16: _Kind("bf16", 4, "bf16", 1.0, 1, *_SPLIT_IMAGE),
    K_DGRAD: _Kind(None, 3, "dgrad_split_bf16x3", 6.0, 3, "c2m_conv3x3_relayout_split_bytes", "c2m_conv3x3_relayout_split_dgrad_f32", True),
    K_SPLIT16: _Kind("split16", 5, "split_f16x2", 3.0, 2, *_SPLIT_IMAGE),
}
ALGO_IDS = {k.name: i for i, k in _KINDS.items() if k.name}
_SPLIT_KINDS = (K_SPLIT, K_BF16, K_SPLIT16)      # the split kernel's three forward flavours
_MFMA32_KINDS = (K_DIRECT, K_WINO, K_WINO4)      # the fp32-MFMA kernels
_POOL_KINDS = (K_WINO,) + _SPLIT_KINDS           # kernels with the pooled epilogue (out_mode "nhwc_pool2")


class _ConvFlops:
    """Opt-in FLOP accounting of the conv3x3 launches (bench.py's roofline line): off on the product path -- nothing is
    counted and no module state is written unless a caller enabled it with count_conv_flops(True)."""
    enabled = False
    algorithmic = 0.0    # direct-convolution flops 2*Cout*9*Cin*H*W*B
    executed = 0.0       # flops the matrix instructions actually perform (F(2,3): 2/3, F(4,3): 1/2 of the direct count)
    by_algo = None       # {kernel family: [launches, algorithmic, executed]}

    @classmethod
    def add(cls, family, algo, execd):
        if cls.enabled:
            cls.algorithmic += algo
            cls.executed += execd
            e = cls.by_algo.setdefault(family, [0, 0.0, 0.0])
            e[0] += 1
            e[1] += algo
            e[2] += execd


def count_conv_flops(on=True):
    """Enable / disable the accounting and reset the counters."""
    _ConvFlops.enabled = bool(on)
    _ConvFlops.algorithmic = _ConvFlops.executed = 0.0
    _ConvFlops.by_algo = {}


def conv_flops_of_last_steps(reset=True, executed=False):
    """2*Cout*9*Cin*H*W*B summed over the conv3x3 calls since the last reset (needs count_conv_flops(True)); executed=True:
    the flops the matrix instructions really perform (Winograd F(2,3) launches execute 2/3 of the direct count)."""
    v = _ConvFlops.executed if executed else _ConvFlops.algorithmic
    if reset:
        _ConvFlops.algorithmic = _ConvFlops.executed = 0.0
        _ConvFlops.by_algo = {}
    return v


def conv_flops_by_family():
    return {k: list(v) for k, v in (_ConvFlops.by_algo or {}).items()}


def _cout_tiles(cout):
    """The library's output-channel tile rule (csrc/conv3x3_shared.h cout_tiles): one 32-row tile for Cout <= 32, else two."""
    return 1 if cout <= 32 else 2


def _split_job_flags(k, cout):
    """Flags word of one c2m_conv3x3_relayout_split_multi job: pieces | tiles << 8 | data-gradient image << 16."""
    return k.pieces | (_cout_tiles(cout) << 8) | (int(k.swap) << 16)


class _WeightCache:
    """Re-laid-out conv weights, keyed by the parameter tensor and its version counter: inference re-uses them across
    calls; an optimiser step (in-place update -> new _version) or load_state_dict invalidates them.  An entry belongs to
    one tensor OBJECT (weak reference): a new parameter that happens to reuse a dead one's id, address and version never
    hits its entry, and entries die with their tensor.

    Writes through ``param.data`` (the reference's own init_offset / default_init_weights idiom, EMA updates, manual
    copies) do NOT bump ``_version``: ``refresh()`` re-runs the re-layout of the live entries from the tensors' current
    contents (a few microseconds of GPU time per entry, no host sync) and the fused inference entry points call it once
    per forward for the parameters of their module (refresh_weight_caches), so a cached image is never older than the
    forward that uses it; ``clear()`` drops everything (clear_weight_caches)."""

    def __init__(self):
        self._d = {}
        self._tables = {}    # refresh job tables: frozenset(param ids) | None -> (signature, device int64 [n, 8], nblocks, any_f16)
        # nn.DataParallel runs the fused forwards of its replicas on one Python thread per GPU: every access to the two
        # dicts goes through this lock (re-entrant: refresh() -> redo() -> _relayout() stays on one thread)
        self._lock = threading.RLock()

    def _lookup(self, slot, key, weight):
        with self._lock:
            hit = self._d.get(slot)
        if hit is not None and hit[0] == key and hit[2]() is weight:
            return hit[1]
        return None

    def _store(self, slot, key, weight, value, redo=None):
        d, lock = self._d, self._lock

        def _drop(ref, slot=slot):
            with lock:
                cur = d.get(slot)
                if cur is not None and cur[2] is ref:
                    del d[slot]
        with lock:
            self._d[slot] = (key, value, weakref.ref(weight, _drop), redo)

    def clear(self):
        with self._lock:
            self._d.clear()
            self._tables.clear()

    def refresh(self, param_ids=None, kinds=None):
        with self._lock:
            return self._refresh_locked(param_ids, kinds)

    def _refresh_locked(self, param_ids=None, kinds=None):
        """Re-run the re-layout of the live entries (of the tensors whose id() is in param_ids, or all) from the tensors'
        current contents.  The split-kernel images -- nearly all of them -- go through ONE multi-tensor call
        (c2m_conv3x3_relayout_split_multi: a device job table, rebuilt only when the set of images changes); the rest
        (fp32-MFMA kernels' layouts, padded input channels) one call per image.  kinds: restrict to these cache kinds (an
        inference forward has no use for the autograd path's images, and vice versa)."""
        n = 0
        jobs, sig, dev = [], [], None
        for slot, (key, value, ref, redo) in list(self._d.items()):
            w = ref()
            if w is None or redo is None or (param_ids is not None and id(w) not in param_ids):
                continue
            if key[0] != w.data_ptr() or key[1] != w._version:
                continue        # stale by key: the next get() rebuilds it anyway
            _, rows, kind = slot if len(slot) == 3 else (None, None, None)   # (id, rows, kind); anything else: redo only
            if kinds is not None and kind is not None and kind not in kinds:
                continue
            k = _KINDS.get(kind)      # (None: a DCNv2 image)
            if k is not None and k.pieces and len(key) == 5 and key[3] is None and w.is_contiguous() and (dev is None or dev == w.device):
                dev = w.device
                Co, Ci = (rows[1] - rows[0] if rows is not None else w.shape[0]), w.shape[1]
                cin_k, cout_k = (Co, Ci) if k.swap else (Ci, Co)
                nbytes = _lib.lib().c2m_conv3x3_relayout_split_bytes(cin_k, cout_k, k.pieces) - (256 if k.pieces == 2 else 0)
                wptr = w.data_ptr() + (rows[0] * Ci * 9 * 4 if rows is not None else 0)
                jobs.append((wptr, value.data_ptr(), cin_k, cout_k, _split_job_flags(k, cout_k), nbytes // 2))
                sig.append((slot, wptr, value.data_ptr()))
            else:
                redo(w, value)
            n += 1
        if jobs:
            tkey = (None if param_ids is None else frozenset(param_ids), None if kinds is None else frozenset(kinds))
            sig = tuple(sig)
            tab = self._tables.get(tkey)
            if tab is None or tab[0] != sig:
                if torch.cuda.is_current_stream_capturing():
                    raise _lib.C2MError("weight-cache refresh: the set of cached weight images changed during a hipGraph capture (its "
                                        "job table would need a host-to-device copy); run one eager forward before capturing")
                rowsl, first = [], 0
                for (wptr, iptr, ci, co, flags, elems) in jobs:
                    rowsl.append([wptr, iptr, ci, co, flags, elems, first, 0])
                    first += (elems + 255) // 256
                host = torch.tensor(rowsl, dtype=torch.int64).pin_memory()
                tab = (sig, host.to(dev, non_blocking=True), first, int(any((j[4] & 0xf) == 2 for j in jobs)), host)
                if len(self._tables) >= 64:      # (tables of parameter sets that no longer exist: a handful of KiB each)
                    self._tables.clear()
                self._tables[tkey] = tab
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().c2m_conv3x3_relayout_split_multi(_stream(), tab[1].data_ptr(), len(jobs), tab[2], tab[3]),
                           "c2m_conv3x3_relayout_split_multi")
        return n

    @staticmethod
    def _relayout(weight, rows, pad_cin_to, kind, wr=None):
        w = weight.detach()
        if rows is not None:
            w = w[rows[0]:rows[1]]
        if w.dtype != torch.float32 or not w.is_cuda or w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
            raise _lib.C2MError("conv3x3: weight must be a float32 GPU tensor [Cout, Cin, 3, 3]")
        Co, Ci = w.shape[:2]
        if pad_cin_to is not None and Ci < pad_cin_to:
            w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, pad_cin_to - Ci))
            Ci = pad_cin_to
        w = w.contiguous()
        L, k = _lib.lib(), _KINDS[kind]
        args = ((Co, Ci) if k.swap else (Ci, Co)) + ((k.pieces,) if k.pieces else ())   # split images: + the number of pieces
        nbytes = getattr(L, k.size_fn)(*args)
        if nbytes == 0:
            raise _lib.C2MError(f"conv3x3: unsupported channel counts Cin={Ci}, Cout={Co}" + (" for this kernel" if kind else
                                " (input channels must be a multiple of 32)"))
        if wr is None:
            wr = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=w.device)
        with torch.cuda.device(w.device):
            _lib.check(getattr(L, k.relayout_fn)(_stream(), w.data_ptr(), Ci, Co, *args[2:], wr.data_ptr()), k.relayout_fn)
        return wr

    def get(self, weight, pad_cin_to=None, rows=None, kind=K_DIRECT):   # kind: a row of _KINDS
        key = (weight.data_ptr(), weight._version, tuple(weight.shape), pad_cin_to, weight.device.index)
        slot = (id(weight), rows, kind)
        hit = self._lookup(slot, key, weight)
        if hit is not None:
            return hit
        wr = self._relayout(weight, rows, pad_cin_to, kind)
        self._store(slot, key, weight, wr,
                    redo=lambda w, buf, rows=rows, pad=pad_cin_to, kind=kind: self._relayout(w, rows, pad, kind, buf))
        return wr


_wcache = _WeightCache()


def _nhwc_src(t, name, bf16_ok=False):
    """channels_last float32 GPU tensor (logical [B,C,H,W], channel stride 1) or a channel slice of one -> ConvSrc.
    bf16_ok: bfloat16 tensors pass too (pitches are in elements either way; c2m_conv3x3_desc.io_flags names the types)."""
    if not t.is_cuda or t.dim() != 4 or not (t.dtype == torch.float32 or (bf16_ok and t.dtype == torch.bfloat16)):
        raise _lib.C2MError(f"{name} must be a 4-D float32 GPU tensor" + (" (or bfloat16)" if bf16_ok else ""))
    sb, sc, sh, sw = t.stride()
    if sc != 1:
        raise _lib.C2MError(f"{name} must be channels-last (stride 1 along C); got strides {t.stride()}")
    # torch leaves the stride of a size-1 dimension arbitrary (a [B,C,1,1] tensor is channels-last with strides (C,1,1,1)) and
    # no index ever multiplies it: where such a stride would fail the kernels' 16-byte pitch checks, describe the dense layout
    B, C, H, W = t.shape
    if W == 1 and sw % 8 != 0:
        sw = (C + 7) // 8 * 8
    if H == 1 and sh % 8 != 0:
        sh = W * sw
    if B == 1 and sb % 8 != 0:
        sb = H * sh
    return _lib.ConvSrc(t.data_ptr(), C, sw, sh, sb)


def empty_nhwc(B, C, H, W, device, dtype=torch.float32):
    return torch.empty((B, C, H, W), dtype=dtype, device=device, memory_format=torch.channels_last)


# C2M_CONV_SPLIT: "all" (default) -- every convolution the split-bf16 kernel supports runs on it (csrc/conv3x3_split.hip:
# fp32-accurate, 6 bf16 MFMAs per fp32 product sum), the extractor towers that feed the index search included (measured on
# configs[2]: 1 near-tie flip of 24 964 queries against the CPU chain, 2 with the fp32-MFMA kernels); "1" -- only calls
# with fast=True (decoder, DCN heads, VGG taps of the Ref); "0" -- never (fp32-MFMA direct / Winograd kernels only)
_SPLIT = os.environ.get("C2M_CONV_SPLIT", "all")
# C2M_CONV_SPLIT16: "1" (default) -- where the split kernel is chosen automatically, inference runs its f16 x 2 flavour
# (three f16 products per fp32 product sum instead of six bf16 ones; error of the class of an fp32 accumulation chain,
# domain |x| < 65520: include/c2m_hip.h C2M_CONV_SPLIT_F16X2); "0" -- the bf16 x 3 flavour (full fp32 range) everywhere.
# The autograd path (conv3x3_autograd: gradients can be tiny) always runs bf16 x 3.
_SPLIT16 = os.environ.get("C2M_CONV_SPLIT16", "1") != "0"


def experimental_built():
    """Always False: the experimental conv kernels (measured no-gos) were removed from the source."""
    return False


# C2M_DCN_F16X2: "1" (default) -- the DCNv2 forward's implicit GEMM follows the convolutions onto the f16 x 2 arithmetic
_DCN_F16X2 = os.environ.get("C2M_DCN_F16X2", "1") != "0"


# ---- f16 x 2 is the DEFAULT arithmetic of fp32 inference, and its domain is |activation| < 65520: outside it the kernel
# writes NaN where nn.Conv2d (arch_util.py:80-136) returns a number.  Every f16 x 2 launch therefore reports out-of-range
# inputs into a per-device flag (c2m_conv3x3_desc.range_flag), and the fused module forwards run under `f16_range_guard`: the
# flag is zeroed before, read once after (one 4-byte read-back per module forward), and if it is set the forward is repeated
# on the bf16 x 3 flavour (full fp32 exponent range) -- the module is then pinned to that flavour.
_tls = threading.local()
_range_flags = {}
_range_lock = threading.Lock()


def _device_flag(dev):
    """The per-device int32 flag (explicit f16 x 2 calls outside any guard report into it; range_flag_set() reads it)."""
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    t = _range_flags.get(key)
    if t is None:
        with _range_lock:
            t = _range_flags.get(key)
            if t is None:
                t = _range_flags[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    return t


def _range_flag(dev):
    """The int32 device flag f16 x 2 launches report into: the enclosing f16_range_guard's OWN flag (one per guard invocation,
    so that concurrent guards on other threads / streams of the device cannot zero each other's report), else -- explicit
    algo="split16" / "f16x2" calls outside any guard -- one per device, which the caller may read with range_flag_set()."""
    g = getattr(_tls, "guard_flag", None)
    if g is not None and g.device == (dev if dev.index is not None else torch.device(dev.type, torch.cuda.current_device())):
        return g
    return _device_flag(dev)


def _f16x2_auto():
    """What algo=None resolves to in conv3x3 / conv3x3_dcn_head / dcn_v2_forward_nhwc: the f16 x 2 arithmetic only where
    somebody reads the range flag afterwards -- inside an f16_range_guard (the fused module forwards) -- or where the caller
    asked for it by name (`with ops.conv_flavour("f16x2")`, then the flag is the caller's to read: range_flag_set()).  A bare
    direct call gets the full-range arithmetic (bf16 x 3 convolutions, fp32-MFMA DCNv2): never a silent NaN."""
    ov = getattr(_tls, "flavour", None)
    if ov is not None:
        return ov
    if getattr(_tls, "guarded", False):
        return _SPLIT16
    if _SPLIT16 and not _f16x2_auto.warned and not torch.cuda.is_current_stream_capturing():
        #  say it once: $C2M_CONV_SPLIT16=1 does NOT make a bare call f16 x 2 -- about twice the matrix work
        _f16x2_auto.warned = True
        warnings.warn("c2m_amd.ops: a conv3x3 / conv3x3_dcn_head / dcn_v2_forward_nhwc call outside `f16_range_guard` and without "
                      "`ops.conv_flavour(...)` runs the FULL-RANGE arithmetic (bf16 x 3 convolutions, fp32-MFMA DCNv2: ~2x the matrix "
                      "work of the f16 x 2 default of the fused module forwards).  For f16 x 2 wrap the calls in "
                      "`with ops.conv_flavour('f16x2'):` and poll `ops.range_flag_set(device)` (domain |x| < 65520); "
                      "`with ops.conv_flavour('bf16x3'):` silences this.", RuntimeWarning, stacklevel=3)
    return False


_f16x2_auto.warned = False


def range_flag_set(device, clear=True):
    """True if an f16 x 2 launch OUTSIDE any guard reported an out-of-domain activation on `device` (a torch.device, a string
    or an index) since the last clear (one 4-byte read-back).  Always the per-device flag: called from code that runs under an
    f16_range_guard it neither sees nor zeroes the guard's own per-invocation flag (ADVICE r5 -- clearing that one would make
    the guard return f16 x 2 overflow garbage instead of re-running on bf16 x 3)."""
    f = _device_flag(torch.device("cuda", device) if isinstance(device, int) else torch.device(device))
    v = int(f.item()) != 0
    if clear and v:
        f.zero_()
    return v


class conv_flavour:
    """`with ops.conv_flavour("bf16x3"): ...` / ("f16x2"): the fp32 split-kernel flavour of this thread's conv3x3 calls inside
    the block (overrides $C2M_CONV_SPLIT16)."""

    def __init__(self, name):
        if name not in ("f16x2", "bf16x3"):
            raise _lib.C2MError("conv_flavour: 'f16x2' or 'bf16x3'")
        self.val = name == "f16x2"

    def __enter__(self):
        self.prev = getattr(_tls, "flavour", None)
        _tls.flavour = self.val
        return self

    def __exit__(self, *exc):
        _tls.flavour = self.prev
        return False


def f16_range_guard(owner, fn, device):
    """Run `fn()` (a fused forward made of conv3x3 calls) so that it never returns f16 x 2 overflow garbage: see above.
    `owner` (an nn.Module or any object) remembers the pinned flavour in `owner._c2m_conv_bf16x3`.
    The outermost guard is also the scope in which the Ref's live extent is shared (ref_live_extent_shared)."""
    if getattr(_tls, "live_cache", None) is not None:
        return _f16_range_guard(owner, fn, device)
    _tls.live_cache = {}
    try:
        return _f16_range_guard(owner, fn, device)
    finally:
        _tls.live_cache = None


def _f16_range_guard(owner, fn, device):
    if getattr(_tls, "guarded", False):      # an enclosing guard (a parent module's forward) checks the flag for all of us
        return fn()
    # (under bf16 autocast the convolutions run the bf16 flavour and never touch the flag; the DCNv2 forwards -- fp32 under
    # autocast, as the reference's custom_fwd(cast_inputs=float32) makes them -- still run f16 x 2 and do)
    if getattr(owner, "_c2m_conv_bf16x3", False):
        with conv_flavour("bf16x3"):
            return fn()
    ov = getattr(_tls, "flavour", None)
    if not (_SPLIT16 if ov is None else ov):     # this thread's fp32 split-kernel calls run bf16 x 3 anyway: nothing to guard
        return fn()
    if torch.cuda.is_current_stream_capturing():
        # the range check reads a flag back, which a hipGraph capture cannot do: captured forwards run the full-range flavour
        with conv_flavour("bf16x3"):
            return fn()
    flag = torch.zeros(1, dtype=torch.int32, device=device)   # this invocation's own flag (see _range_flag)
    _tls.guarded, _tls.guard_flag = True, flag
    try:
        out = fn()
    finally:
        _tls.guarded, _tls.guard_flag = False, None
    if int(flag.item()) == 0:
        return out
    warnings.warn(f"{type(owner).__name__}: an activation left the f16 x 2 convolution flavour's domain (|x| >= 65520); the forward "
                  "was recomputed on the bf16 x 3 flavour (full fp32 range), which this module now keeps", RuntimeWarning)
    try:
        owner._c2m_conv_bf16x3 = True
    except Exception:  # noqa: BLE001 -- an owner without attributes: just recompute
        pass
    with conv_flavour("bf16x3"):
        return fn()


def _wino_ok(srcs, weight, out_mode, W):
    """Winograd F(2,3)-along-x kernel: channels-last output, 64-wide cout tiles, whole 32-pixel tiles along x."""
    return (out_mode in ("nhwc", "nhwc_pool2") and weight.shape[0] % 64 == 0 and W % 32 == 0 and
            all(s.shape[1] % 16 == 0 for s in srcs) and sum(s.shape[1] for s in srcs) == weight.shape[1])


def _wino4_ok(srcs, weight, out_mode, W):
    """Winograd F(4,3)-along-x kernel: as F(2,3) but plain channels-last output and whole 64-pixel tiles along x."""
    return W % 64 == 0 and out_mode == "nhwc" and _wino_ok(srcs, weight, out_mode, W)


def bf16_autocast():
    """True inside `torch.autocast('cuda', dtype=torch.bfloat16)`: the caller asked for reduced precision (BASELINE
    configs[4]) -- the convolutions then run the split kernel with ONE round-to-nearest bf16 piece per operand (algo
    "bf16": bf16 products, fp32 accumulation, fp32 tensors in and out), 1/6 of the matrix work of the fp32 flavour."""
    return torch.is_autocast_enabled('cuda') and torch.get_autocast_dtype('cuda') == torch.bfloat16


def _split_ok(srcs, weight, fast):
    """Split-bf16 kernel: any map size / output mode; 16-channel chunks; sources add up to the weight's input channels."""
    return ((_SPLIT == "all" or (fast and _SPLIT != "0")) and all(s.shape[1] % 16 == 0 for s in srcs) and
            sum(s.shape[1] for s in srcs) == weight.shape[1])


def _as_list(srcs):
    return list(srcs) if isinstance(srcs, (list, tuple)) else [srcs]


def _check_abs_sum(abs_sum):
    if abs_sum is not None and (abs_sum.dtype != torch.float64 or abs_sum.numel() < 256 or not abs_sum.is_cuda):
        raise _lib.C2MError("abs_sum must be a float64 GPU tensor with 256 slots (C2M_ABS_SUM_SLOTS)")


def _split_kind(algo):
    """The split kernel's flavour for `algo` (None: automatic): one rounded bf16 piece if asked for by name or under bf16
    autocast, else f16 x 2 if asked for by name or -- automatic only -- where somebody reads the range flag (_f16x2_auto, which
    is not consulted, and does not warn, once autocast has decided), else bf16 x 3."""
    if algo == "bf16" or (algo is None and bf16_autocast()):
        return K_BF16
    if algo == "split16" or (algo is None and _f16x2_auto()):
        return K_SPLIT16
    return K_SPLIT


def _conv_desc(kind, srcs, wr, B, H, W, Cin, Cout, names=None, bf16_ok=False):
    """A c2m_conv3x3_desc with the algo, geometry, sources, weight image and (f16 x 2) range flag of one launch filled in."""
    d = _lib.Conv3x3Desc()
    d.algo = _KINDS[kind].algo
    d.B, d.H, d.W, d.Cin, d.Cout, d.nsrc = B, H, W, Cin, Cout, len(srcs)
    for k, s in enumerate(srcs):
        if tuple(s.shape[2:]) != (H, W) or s.shape[0] != B:
            raise _lib.C2MError("conv3x3: sources must share B, H, W")
        d.src[k] = _nhwc_src(s, names[k] if names else f"src{k}", bf16_ok=bf16_ok)
    d.wr = wr.data_ptr()
    if kind == K_SPLIT16:
        d.range_flag = _range_flag(srcs[0].device).data_ptr()
    return d


def _desc_out(d, out, bf16_ok=False):
    """Point the descriptor's output at a channels-last tensor; -> its ConvSrc (pitches)."""
    o = _nhwc_src(out, "out", bf16_ok=bf16_ok)
    d.out, d.out_pix_pitch, d.out_row_pitch, d.out_img_pitch = out.data_ptr(), o.pix_pitch, o.row_pitch, o.img_pitch
    return o


def _roi_pixels(roi_tiles, H, W, rgb64=False):
    """(rows, columns) of the pixels a launch computes: the whole map, or the top-left `roi_tiles` = (tile rows, tile columns)."""
    if roi_tiles is None:
        return H, W
    th, tw = conv_roi_tile(rgb64)
    return min(roi_tiles[0] * th, H), min(roi_tiles[1] * tw, W)


def _launch_conv(d, dev, kind, family_prefix="", roi_tiles=None):
    """c2m_conv3x3_nhwc_f32 (roi_tiles: the top-left (tile rows, tile columns) only) on the current stream of `dev` (+ the
    opt-in flop accounting of the launch: the pixels of the tiles actually launched)."""
    if roi_tiles is not None:
        d.roi_tiles_y, d.roi_tiles_x = int(roi_tiles[0]), int(roi_tiles[1])
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().c2m_conv3x3_nhwc_f32(_stream(), d), "c2m_conv3x3_nhwc_f32")
    if _ConvFlops.enabled:
        rh, rw = _roi_pixels(roi_tiles, d.H, d.W)
        f = 2.0 * d.Cout * 9 * d.Cin * rh * rw * d.B
        _ConvFlops.add(family_prefix + _KINDS[kind].family, f, f * _KINDS[kind].exec_factor)


def conv3x3(srcs, weight, bias=None, act=ACT_NONE, slope=0.1, res1=None, res2=None, out_mode="nhwc", out=None, algo=None,
            out2_grouped8=None, fast=False, out_dtype=None, dword_stores=False, roi_tiles=None):
    """out = act(conv3x3(cat(srcs, dim=1)) + bias) + res1 + res2 on channels-last tensors, one kernel.

    bf16 tensors ("bf16" kernel and "nhwc" mode only -- what a bf16-autocast forward keeps its activations in between fused
    convolutions, BASELINE configs[4]): a single bfloat16 source, bfloat16 residuals and `out_dtype=torch.bfloat16` (or a
    bfloat16 `out`) are accepted in any combination with float32 ones; sums stay fp32, one rounding at the store.

    srcs: one or two channels_last tensors [B,Ci,H,W] (each Ci % 32 == 0; a single source with fewer input channels than
    the (zero-padded) weight is not accepted -- pad the tensor).  out_mode: "nhwc" -> channels_last [B,Cout,H,W];
    "pixel_shuffle" -> channels_last [B,Cout/4,2H,2W] (= PixelShuffle(2) of the conv output); "nchw" -> contiguous;
    "nhwc_pool2" -> channels_last [B,Cout,H/2,W/2] = MaxPool2d(2, 2) of the activated output (Winograd F(2,3) shapes only).
    out2_grouped8: a zero-bordered group-major buffer [B,Cout/8,H+3,W+3,8] that receives a second copy of the output
    (what the DCNv2 kernel gathers 8-channel groups from); "nhwc" mode on the direct kernel only.
    algo: None (auto), "direct", "winograd", "winograd4", "split" (fp32-accurate on the bf16 matrix pipe: three exact bf16
    pieces per operand, six MFMAs per product sum, csrc/conv3x3_split.hip), "split16" (fp32-accurate on the f16 matrix pipe:
    two round-to-nearest f16 pieces per activation, per-tensor-scaled weights, THREE MFMAs per product sum; |x| < 65520),
    "bf16" (one rounded piece: a bf16 convolution with fp32 accumulation).  Auto: the split kernel wherever it applies (any
    map size / mode, channels % 16 == 0) -- its f16 x 2 flavour inside an f16_range_guard (the fused module forwards) or under
    `ops.conv_flavour("f16x2")`, unless $C2M_CONV_SPLIT16=0; a bare direct call gets bf16 x 3 (full range: _f16x2_auto).
    dword_stores: split kernels, "pixel_shuffle" / "nchw" modes: this call's epilogue stores one dword per lane instead of
    the 16-byte lane-swapped / quad-transposed pieces (c2m_hip.h C2M_IO_DWORD_STORES: same bits, the other instruction
    sequence -- tests and measurement; per call, nothing process-wide).
    roi_tiles: (tile rows, tile columns) -- split kernels only: launch the top-left tiles of the grid (conv_roi_tile() pixels
    each) and leave the rest of the output untouched (the Ref-side towers fill it from a template: _RefBand).
    $C2M_CONV_SPLIT=1 restricts it to calls with fast=True (the decoder; the extractor towers that feed the index search
    then stay on the fp32-MFMA kernels), $C2M_CONV_SPLIT=0 restores the round-2 choice everywhere: Winograd F(4,3) with
    fast=True / F(2,3) where the shapes allow, else direct."""
    srcs = _as_list(srcs)
    B, _, H, W = srcs[0].shape
    Cin = sum(s.shape[1] for s in srcs)
    Cout = weight.shape[0]
    dev = srcs[0].device
    if algo is None:
        reduced = bf16_autocast()
        if (out2_grouped8 is None and (_split_ok(srcs, weight, fast) or (reduced and _split_ok(srcs, weight, True))) and (out_mode != "nhwc_pool2" or (H % 2 == 0 and W % 2 == 0))
                and (out_mode not in ("nhwc", "nhwc_pool2") or Cout % 4 == 0)):   # channels-last stores are 16-byte vectors
            kind = _split_kind(None)
        else:
            kind = K_WINO4 if (fast and _wino4_ok(srcs, weight, out_mode, W)) else K_WINO if _wino_ok(srcs, weight, out_mode, W) else K_DIRECT
    elif algo in ALGO_IDS:
        kind = ALGO_IDS[algo]
    else:
        raise _lib.C2MError(f"conv3x3: unknown algo {algo!r} (one of {', '.join(ALGO_IDS)})")
    if out2_grouped8 is not None:
        if algo not in (None, "direct") or out_mode != "nhwc":
            raise _lib.C2MError("out2_grouped8 needs the direct kernel in nhwc mode")
        kind = K_DIRECT
    wr = _wcache.get(weight, pad_cin_to=Cin if weight.shape[1] < Cin else None, kind=kind)
    d = _conv_desc(kind, srcs, wr, B, H, W, Cin, Cout, bf16_ok=True)
    io = 1 if srcs[0].dtype == torch.bfloat16 else 0
    if any(s.dtype == torch.bfloat16 for s in srcs[1:]) or (io and len(srcs) != 1):
        raise _lib.C2MError("conv3x3: a bfloat16 source must be the only source")
    if out is not None:
        out_dtype = out.dtype
    if out_dtype == torch.bfloat16:
        io |= 2
    elif out_dtype not in (None, torch.float32):
        raise _lib.C2MError("conv3x3: out_dtype is float32 or bfloat16")
    for bit, r in ((4, res1), (8, res2)):
        if r is not None and r.dtype == torch.bfloat16:
            io |= bit
    if io and (kind != K_BF16 or out_mode != "nhwc"):
        raise _lib.C2MError("conv3x3: bfloat16 tensors need the bf16 kernel (algo='bf16' / bf16 autocast) in nhwc mode")
    if dword_stores:
        if io or kind not in _SPLIT_KINDS or out_mode not in ("pixel_shuffle", "nchw"):
            raise _lib.C2MError("conv3x3: dword_stores selects a store path of the split kernels' pixel_shuffle / nchw epilogues")
        io = 16
    d.io_flags = io
    if bias is not None:
        bias = _dev_f32(bias.detach(), "bias")
    d.bias = bias.data_ptr() if bias is not None else None
    d.act, d.slope = int(act), float(slope)
    if out_mode == "nhwc":
        if out is None:
            out = empty_nhwc(B, Cout, H, W, dev, torch.bfloat16 if io & 2 else torch.float32)
        d.out_mode = 0
        o = _desc_out(d, out, bf16_ok=True)
        for name, r in (("res1", res1), ("res2", res2)):
            if r is not None:
                rs = _nhwc_src(r, name, bf16_ok=True)
                if (rs.pix_pitch, rs.row_pitch, rs.img_pitch) != (o.pix_pitch, o.row_pitch, o.img_pitch) or r.shape != out.shape:
                    raise _lib.C2MError(f"{name} must have the geometry of the output")
                setattr(d, name, r.data_ptr())
        if out2_grouped8 is not None:
            d.out2, d.out2_row_pitch, d.out2_plane_pitch, d.out2_img_pitch = _grouped8_args(out2_grouped8, B, Cout, H, W, dev)
    elif out_mode == "pixel_shuffle":
        out = empty_nhwc(B, Cout // 4, 2 * H, 2 * W, dev)
        d.out_mode = 1
        _desc_out(d, out)
    elif out_mode == "nhwc_pool2":
        if kind not in _POOL_KINDS or H % 2 != 0 or W % 2 != 0:
            raise _lib.C2MError("conv3x3: the pooled epilogue needs the Winograd F(2,3) or the split-bf16 kernel and even H, W")
        out = empty_nhwc(B, Cout, H // 2, W // 2, dev)
        d.out_mode = 4
        _desc_out(d, out)
    elif out_mode == "nchw":
        out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=dev)
        d.out_mode = 2
        d.out = out.data_ptr()
    else:
        raise _lib.C2MError(f"unknown out_mode {out_mode}")
    if roi_tiles is not None and kind not in _SPLIT_KINDS:
        raise _lib.C2MError("conv3x3: roi_tiles needs one of the split kernels")
    _launch_conv(d, dev, kind, roi_tiles=roi_tiles)
    return out


def conv3x3_dgrad(grad_out, weight):
    """Data gradient of conv3x3: grad_out channels-last [B,Cout,H,W], weight [Cout,Cin,3,3] -> dX channels-last [B,Cin,H,W]
    = conv3x3(grad_out, W') with W'[ci][co][dy][dx] = W[co][ci][2-dy][2-dx], on the split-bf16 kernel (fp32-accurate)."""
    Cout, Cin = weight.shape[:2]
    B, Cg, H, W = grad_out.shape
    if Cg != Cout or Cout % 16 != 0 or Cin % 4 != 0:
        raise _lib.C2MError("conv3x3_dgrad: grad_out channels must equal weight.shape[0] (a multiple of 16); Cin % 4 == 0")
    wr = _wcache.get(weight, kind=K_DGRAD)
    out = empty_nhwc(B, Cin, H, W, grad_out.device)
    d = _conv_desc(K_DGRAD, [grad_out], wr, B, H, W, Cout, Cin, names=("grad_out",))   # the convolution maps Cout to Cin channels
    d.out_mode = 0
    _desc_out(d, out)
    _launch_conv(d, grad_out.device, K_DGRAD)
    return out


def conv3x3_wgrad(srcs, grad_out, Cout):
    """Weight gradient of conv3x3(cat(srcs)): srcs / grad_out channels-last -> grad_weight [Cout, Cin, 3, 3] (fp32 MFMA over
    pixel segments, deterministic two-stage reduction; csrc/conv3x3_wgrad.hip)."""
    srcs = _as_list(srcs)
    B, _, H, W = srcs[0].shape
    Cin = sum(s_.shape[1] for s_ in srcs)
    if tuple(grad_out.shape) != (B, Cout, H, W):
        raise _lib.C2MError("conv3x3_wgrad: grad_out must be [B, Cout, H, W]")
    dev = grad_out.device
    L = _lib.lib()
    arr = (_lib.ConvSrc * 2)()
    for k, s_ in enumerate(srcs):
        arr[k] = _nhwc_src(s_, f"src{k}")
    g = _nhwc_src(grad_out, "grad_out")
    gw = torch.empty((Cout, Cin, 3, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nbytes = L.c2m_conv3x3_wgrad_workspace_bytes(B, H, W, Cin, Cout)
        ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=dev)
        _lib.check(L.c2m_conv3x3_wgrad_f32(_stream(), arr, len(srcs), grad_out.data_ptr(), g.pix_pitch, g.row_pitch, g.img_pitch,
                                           B, H, W, Cin, Cout, gw.data_ptr(), ws.data_ptr(), nbytes), "c2m_conv3x3_wgrad_f32")
    return gw


def _as_nhwc(t):
    """float32 channels-last view / copy of a [B,C,H,W] tensor (what the kernels' pitch descriptors need)."""
    t = t.float() if t.dtype != torch.float32 else t
    return t if t.stride(1) == 1 else t.contiguous(memory_format=torch.channels_last)


class _Conv3x3Fn(torch.autograd.Function):
    """Differentiable act(conv3x3(cat(srcs)) + bias) on the hand-written kernels: forward = the split-bf16 kernel, backward =
    the same kernel on rotated / transposed weights (data gradient) + the fp32-MFMA weight-gradient kernel + two elementwise
    torch ops (activation mask, bias sum).  Stage-3 training (ref_restoration_model.py:192-269) runs its decoder through this
    instead of cuDNN/MIOpen convolutions."""

    @staticmethod
    def forward(ctx, weight, bias, act, slope, *srcs):
        srcs = [_as_nhwc(s_) for s_ in srcs]
        out = conv3x3(srcs, weight, bias, act=act, slope=slope, algo="split")
        ctx.act, ctx.slope, ctx.nsrc = int(act), float(slope), len(srcs)
        ctx.save_for_backward(weight, *(srcs + ([out] if act != ACT_NONE else [])))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        weight, srcs = saved[0], list(saved[1:1 + ctx.nsrc])
        g = _as_nhwc(grad_out)
        if ctx.act != ACT_NONE:
            out = saved[1 + ctx.nsrc]
            g = g * torch.where(out > 0, 1.0, ctx.slope if ctx.act == ACT_LRELU else 0.0)
            g = _as_nhwc(g)
        need = ctx.needs_input_grad
        gw = conv3x3_wgrad(srcs, g, weight.shape[0]) if need[0] else None
        gb = g.sum(dim=(0, 2, 3)) if need[1] else None
        gsrc = [None] * ctx.nsrc
        if any(need[4:4 + ctx.nsrc]):
            Co = weight.shape[0]
            if Co % 16 != 0:   # the data-gradient convolution sweeps dY in 16-channel chunks: zero-pad (216-channel DCN heads)
                pad = 16 - Co % 16
                dx = conv3x3_dgrad(_as_nhwc(torch.nn.functional.pad(g, (0, 0, 0, 0, 0, pad))),
                                   torch.nn.functional.pad(weight.detach(), (0, 0, 0, 0, 0, 0, 0, pad)))
            else:
                dx = conv3x3_dgrad(g, weight)
            c0 = 0
            for k, s_ in enumerate(srcs):
                if need[4 + k]:
                    gsrc[k] = dx[:, c0:c0 + s_.shape[1]]
                c0 += s_.shape[1]
        return (gw, gb, None, None, *gsrc)


def conv3x3_autograd(srcs, weight, bias=None, act=ACT_NONE, slope=0.1):
    """act(conv3x3(cat(srcs)) + bias) with gradients (channels-last float32 in and out; sources a multiple of 32 channels,
    Cout a multiple of 16).  See _Conv3x3Fn."""
    srcs = _as_list(srcs)
    return _Conv3x3Fn.apply(weight, bias, int(act), float(slope), *srcs)


def conv3x3_autograd_ok(srcs, weight):
    """Shapes the differentiable path supports: 32-channel source blocks (weight-gradient kernel) and 16-byte channels-last
    output vectors (Cout % 4 == 0; the data-gradient convolution pads Cout to a multiple of 16 itself)."""
    srcs = _as_list(srcs)
    return (all(s_.is_cuda and s_.dim() == 4 and s_.shape[1] % 32 == 0 for s_ in srcs) and weight.shape[0] % 4 == 0 and
            sum(s_.shape[1] for s_ in srcs) == weight.shape[1] and tuple(weight.shape[2:]) == (3, 3) and _SPLIT != "0")


def _grouped8_args(g2, B, Cout, H, W, dev):
    if g2 is None:
        return None, 0, 0, 0
    if (g2.dtype != torch.float32 or not g2.is_contiguous() or Cout % 8 != 0 or
            tuple(g2.shape) != (B, Cout // 8, H + 3, W + 3, 8) or g2.device != dev):
        raise _lib.C2MError("out2_grouped8 must be a contiguous float32 [B, Cout/8, H+3, W+3, 8] buffer")
    # image pixel (0, 0) = bordered pixel (1, 1); pitches in floats
    return g2.data_ptr() + ((W + 3) + 1) * 8 * 4, (W + 3) * 8, (H + 3) * (W + 3) * 8, (Cout // 8) * (H + 3) * (W + 3) * 8


def conv3x3_rgb64(image, weight, bias=None, act=ACT_NONE, slope=0.1, mean=None, std=None, out=None, out2_grouped8=None,
                  roi_tiles=None):
    """First layer of an image tower (3 -> 64 channels; vgg conv1_1, conv_first) as its own im2col kernel:
    out = act(conv3x3((image - mean) / std) + bias), channels_last [B,64,H,W].  image: [B,3,H,W] (any layout; read as
    contiguous NCHW); mean / std: [1,3,1,1] buffers of the extractor or None.  out / out2_grouped8 / roi_tiles as in conv3x3
    (the tile of this kernel: conv_roi_tile(rgb64=True))."""
    if image.dim() != 4 or image.shape[1] != 3 or not image.is_cuda:
        raise _lib.C2MError("conv3x3_rgb64: image must be a GPU tensor [B,3,H,W]")
    if tuple(weight.shape) != (64, 3, 3, 3):
        raise _lib.C2MError("conv3x3_rgb64: weight must be [64,3,3,3]")
    B, _, H, W = image.shape
    if (mean is None) != (std is None):
        raise _lib.C2MError("conv3x3_rgb64: mean and std go together")
    if 12 * H * W >= 2 ** 31:
        # checked before anything is copied: the kernel addresses one image with 32-bit byte offsets (12 bytes per pixel), and
        # the generic kernel on a 32-channel padded copy has the same 2^31-byte bound per sample at a tenth of the pixels
        raise _lib.C2MError(f"conv3x3_rgb64: image of {H} x {W} pixels is too large (H * W < 178 956 971)")
    x = image.float().contiguous()
    dev = x.device
    w = _dev_f32(weight.detach(), "weight")
    bias = _dev_f32(bias.detach(), "bias") if bias is not None else None
    if mean is not None:
        mean, std = _dev_f32(mean.detach().reshape(3), "mean"), _dev_f32(std.detach().reshape(3), "std")
    if out is None:
        out = empty_nhwc(B, 64, H, W, dev)
    o = _nhwc_src(out, "out")
    if tuple(out.shape) != (B, 64, H, W):
        raise _lib.C2MError("conv3x3_rgb64: out must be [B,64,H,W]")
    o2, o2_row, o2_plane, o2_img = _grouped8_args(out2_grouped8, B, 64, H, W, dev)
    d = _lib.Conv3x3Rgb64Desc(
        image=x.data_ptr(), B=B, H=H, W=W, weight=w.data_ptr(), bias=bias.data_ptr() if bias is not None else None,
        mean=mean.data_ptr() if mean is not None else None, std_=std.data_ptr() if std is not None else None, act=int(act),
        slope=float(slope), out=out.data_ptr(), out_pix_pitch=o.pix_pitch, out_row_pitch=o.row_pitch, out_img_pitch=o.img_pitch,
        out2=o2, out2_row_pitch=o2_row, out2_plane_pitch=o2_plane, out2_img_pitch=o2_img)
    if roi_tiles is not None:
        d.roi_tiles_y, d.roi_tiles_x = int(roi_tiles[0]), int(roi_tiles[1])
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().c2m_conv3x3_rgb64_f32(_stream(), d), "c2m_conv3x3_rgb64_f32")
    if _ConvFlops.enabled:
        rh, rw = _roi_pixels(roi_tiles, H, W, rgb64=True)
        _ConvFlops.add("rgb_first_layer", 2.0 * 64 * 27 * rh * rw * B, 2.0 * 64 * 28 * rh * rw * B)
    return out


def index_to_flow(max_idx):
    """max_idx int64 [B,hq,wq] -> flow float32 [B,hq,wq,2] (x, y), un-padded (corres_generation_arch.py:29-46)."""
    if not max_idx.is_cuda or max_idx.dtype != torch.int64 or max_idx.dim() != 3:
        raise _lib.C2MError("max_idx must be an int64 GPU tensor [B, hq, wq]")
    mi = max_idx.contiguous()
    B, hq, wq = mi.shape
    flow = torch.empty((B, hq, wq, 2), dtype=torch.float32, device=mi.device)
    with torch.cuda.device(mi.device):
        _lib.check(_lib.lib().c2m_index_to_flow_f32(_stream(), mi.data_ptr(), B, hq, wq, flow.data_ptr()), "c2m_index_to_flow_f32")
    return flow


def conv3x3_dcn_head(srcs, weight, bias, deformable_groups, flow=None, scale=1, abs_sum=None, algo=None, dword_stores=False):
    """The DCN offset/mask head (conv_offset_mask of DCN_sep_pre_multi_offset, dcn_v2.py:229-245) fused with the
    pre-offset construction: -> (offset [B,2*dg*9,H,W], mask [B,dg*9,H,W]) planar, ready for dcn_v2_forward.
    flow: index_to_flow(max_idx) of the matched LR features (or None: no pre-offset); scale = H / h (1, 2, 4).
    The head's channels are computed in slices of 64-channel tiles + one 32-wide remainder (216 = 192 + 24) so that
    no padded tile is multiplied.
    dword_stores: split kernels: this call's epilogue stores one dword per lane and loads the flow per (4 channels, pixel)
    instead of the 16-byte quad-transposed stores + register flow window that maps with W % 4 == 0 take (c2m_hip.h
    C2M_IO_DWORD_STORES: same bits, the other instruction sequence; tests, measurement)."""
    srcs = _as_list(srcs)
    B, _, H, W = srcs[0].shape
    Cin = sum(s.shape[1] for s in srcs)
    dg = int(deformable_groups)
    Cout = weight.shape[0]
    if Cout != 3 * dg * 9:
        raise _lib.C2MError("conv3x3_dcn_head: weight must have 3*dg*9 output channels")
    dev = srcs[0].device
    bias = _dev_f32(bias.detach(), "bias")
    offset = torch.empty((B, 2 * dg * 9, H, W), dtype=torch.float32, device=dev)
    mask = torch.empty((B, dg * 9, H, W), dtype=torch.float32, device=dev)
    if flow is not None:
        if flow.dtype != torch.float32 or not flow.is_cuda or flow.dim() != 4 or flow.shape[0] != B or flow.shape[3] != 2:
            raise _lib.C2MError("flow must be float32 [B, fh, fw, 2] on the GPU")
        flow = flow.contiguous()
    _check_abs_sum(abs_sum)
    split = (Cout // 64) * 64
    slices = [(0, Cout)] if (split == 0 or Cout - split > 32 or split == Cout) else [(0, split), (split, Cout)]
    use_split = algo in ("split", "bf16", "split16") or (algo is None and _SPLIT != "0" and all(s_.shape[1] % 16 == 0 for s_ in srcs))
    split_kind = _split_kind(algo)
    wino = algo is None and W % 32 == 0 and all(s_.shape[1] % 16 == 0 for s_ in srcs)
    if dword_stores and not use_split:   # every slice's kind is then K_WINO / K_DIRECT, not one of _SPLIT_KINDS
        raise _lib.C2MError("conv3x3_dcn_head: dword_stores selects a store path of the split kernels' epilogue")
    for (c0, c1) in slices:
        # split-bf16 kernel (any shape); else 64-channel-tileable slices on whole 32-pixel tiles take the Winograd F(2,3)
        # kernel (1.5x fewer matrix instructions), the rest the direct kernel
        kind = split_kind if use_split else K_WINO if (wino and (c1 - c0) % 64 == 0) else K_DIRECT
        wr = _wcache.get(weight, rows=(c0, c1), kind=kind)
        d = _conv_desc(kind, srcs, wr, B, H, W, Cin, c1 - c0)
        d.bias = bias.data_ptr() + 4 * c0
        d.out_mode = 3
        d.out, d.mask_out, d.n_off, d.scale = offset.data_ptr(), mask.data_ptr(), 2 * dg * 9, int(scale)
        d.cout_offset, d.cout_total = c0, Cout
        if flow is not None:
            d.flow, d.fh, d.fw = flow.data_ptr(), flow.shape[1], flow.shape[2]
        if abs_sum is not None:
            d.abs_sum = abs_sum.data_ptr()
        if dword_stores:
            d.io_flags = 16
        _launch_conv(d, dev, kind, "dcn_head_")
    return offset, mask


# ---------------------------------------------------------------------------------------------------------------------
# DCNv2 forward on the fused decoder path: bordered channels-last input shared with the convolutions, cached weights,
# channels-last output with the activation folded in
# ---------------------------------------------------------------------------------------------------------------------
class BorderedNHWC:
    """Zero-bordered channels-last copy [B][H+3][W+3][C] of an NCHW feature map (what the DCNv2 kernels gather from).
    `grouped8`: optional twin in the 8-channel group-major layout [B][C/8][H+3][W+3][8], written by the producing
    convolution's epilogue; DCNv2 layers with 8 channels per deformable group gather from it instead."""
    grouped8 = None

    def __new__(cls, x=None):
        pre = bordered_of(x) if x is not None else None   # already the interior view of a bordered buffer: no copy
        return pre if pre is not None else super().__new__(cls)

    def __init__(self, x):
        if bordered_of(x) is self:
            return
        x = _dev_f32(x, "x")
        self.B, self.C, self.H, self.W = x.shape
        self.buf = torch.empty((self.B, self.H + 3, self.W + 3, self.C), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().c2m_nchw_to_nhwc_bordered_f32(_stream(), x.data_ptr(), self.B, self.C, self.H, self.W,
                                                               self.buf.data_ptr()), "c2m_nchw_to_nhwc_bordered_f32")

    def interior(self):
        """Logical [B,C,H,W] channels-last view of the image inside the border (a conv3x3 source)."""
        return self.buf[:, 1:self.H + 1, 1:self.W + 1, :].permute(0, 3, 1, 2)


class _DcnWeightCache(_WeightCache):
    # per DCNv2 kind: the C-ABI's size / re-layout entry points, what a geometry without that image is told
    _IMAGES = {K_DCN: ("c2m_dcn_v2_relayout_bytes", "c2m_dcn_v2_relayout_f32", "geometry is not on the channels-last path"),
               K_DCN16: ("c2m_dcn_v2_relayout_f16x2_bytes", "c2m_dcn_v2_relayout_f16x2",
                         "geometry has no f16 x 2 kernel (needs >= 16 channels per (virtual) group)")}

    @classmethod
    def _relayout_dcn(cls, weight, dg, kind, wt=None):
        size_fn, relayout_fn, why = cls._IMAGES[kind]
        w = _dev_f32(weight.detach(), "weight")
        Co, C, kh, kw = w.shape
        L = _lib.lib()
        nbytes = getattr(L, size_fn)(C, Co, kh, kw, dg)
        if nbytes == 0:
            raise _lib.C2MError("dcn_v2_forward_nhwc: " + why)
        if wt is None:
            wt = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
        with torch.cuda.device(w.device):
            _lib.check(getattr(L, relayout_fn)(_stream(), w.data_ptr(), C, Co, kh, kw, dg, wt.data_ptr()), relayout_fn)
        return wt

    def get(self, weight, dg, f16x2=False):
        key = (weight.data_ptr(), weight._version, tuple(weight.shape), dg, weight.device.index)
        kind = K_DCN16 if f16x2 else K_DCN
        slot = (id(weight), None, kind)
        hit = self._lookup(slot, key, weight)
        if hit is not None:
            return hit
        wt = self._relayout_dcn(weight, dg, kind)
        self._store(slot, key, weight, wt, redo=lambda w, buf, dg=dg, kind=kind: self._relayout_dcn(w, dg, kind, buf))
        return wt


_dcn_wcache = _DcnWeightCache()


def refresh_weight_caches(module_or_params=None, all_kinds=False):
    """Rebuild the cached weight images (conv3x3 re-layouts, DCNv2 re-layouts) of the given module's / iterable's
    parameters -- or of every live entry -- from the tensors' CURRENT contents; unless all_kinds, only the images the
    CURRENT path multiplies with (no-grad forward: the f16 x 2 / bf16 / bf16 x 3 forward images of the active flavour and the
    fp32-MFMA layouts, not the autograd path's data-gradient images).  The fused inference entry points call
    this once per forward: in-place writes through ``param.data`` do not bump the version counter the caches are keyed
    on, so without it such an update would keep computing with the old weights.  Returns the number of
    images rebuilt.  No host synchronisation."""
    ids = None
    if module_or_params is not None:
        params = module_or_params.parameters() if hasattr(module_or_params, "parameters") else module_or_params
        ids = {id(p) for p in params}
    kinds = None
    if not all_kinds and not torch.is_grad_enabled():
        kinds = {*_MFMA32_KINDS, _split_kind(None)}
    return _wcache.refresh(ids, kinds) + _dcn_wcache.refresh(ids)


def clear_weight_caches():
    """Drop every cached weight image (they are rebuilt on the next use)."""
    _wcache.clear()
    _dcn_wcache.clear()


def dcn_f16x2_ok(weight, deformable_groups):
    Co, C, kh, kw = weight.shape
    return _lib.lib().c2m_dcn_v2_relayout_f16x2_bytes(C, Co, kh, kw, int(deformable_groups)) != 0


def dcn_v2_forward_nhwc(inp_bordered, weight, bias, offset, mask, deformable_groups, act=ACT_NONE, slope=0.1,
                        nhwc_out=True, algo=None):
    """3x3 / stride 1 / pad 1 DCNv2 forward from a BorderedNHWC input; planar offset / mask as dcn_v2_forward takes them.
    -> channels_last [B,Co,H,W] (nhwc_out) or contiguous NCHW, with the activation applied.
    algo: "fp32" (implicit GEMM on the fp32 matrix pipe), "f16x2" (fp32 result on the f16 pipe, three products per k step:
    the convolutions' f16 x 2 arithmetic, domain |sample| < 65520 reported through the same range flag), None: f16 x 2
    wherever the convolutions of this thread run it by default (_f16x2_auto: inside an f16_range_guard -- the fused module
    forwards -- or under `ops.conv_flavour("f16x2")`; $C2M_DCN_F16X2=0 keeps fp32) and the geometry has that kernel; a bare
    direct call runs fp32."""
    if not isinstance(inp_bordered, BorderedNHWC):
        raise _lib.C2MError("inp_bordered must be a BorderedNHWC")
    B, C, H, W = inp_bordered.B, inp_bordered.C, inp_bordered.H, inp_bordered.W
    Co = weight.shape[0]
    dg = int(deformable_groups)
    offset, mask, bias = _dev_f32(offset, "offset"), _dev_f32(mask, "mask"), _dev_f32(bias.detach(), "bias")
    _check_offset_mask(offset, mask, B, dg, 9, H, W, ("9", "H", "W"))
    if algo is None:
        f16 = _DCN_F16X2 and _SPLIT != "0" and _f16x2_auto() and dcn_f16x2_ok(weight, dg)
    elif algo in ("fp32", "f16x2"):
        f16 = algo == "f16x2"
    else:
        raise _lib.C2MError("dcn_v2_forward_nhwc: algo is None, 'fp32' or 'f16x2'")
    wt = _dcn_wcache.get(weight, dg, f16x2=f16)
    dev = offset.device
    grouped = inp_bordered.grouped8 is not None and C == 8 * dg
    src = inp_bordered.grouped8 if grouped else inp_bordered.buf
    d = _lib.DcnNhwcDesc(B=B, C=C, H=H, W=W, Co=Co, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, dg=dg,
                         input_bordered=src.data_ptr(), input_grouped=int(grouped), wt=wt.data_ptr(), bias=bias.data_ptr(),
                         offset=offset.data_ptr(), mask=mask.data_ptr(), act=int(act), slope=float(slope))
    if nhwc_out:
        out = empty_nhwc(B, Co, H, W, dev)
        o = _nhwc_src(out, "out")
        d.out_nhwc, d.out_pix_pitch, d.out_row_pitch, d.out_img_pitch = 1, o.pix_pitch, o.row_pitch, o.img_pitch
    else:
        out = torch.empty((B, Co, H, W), dtype=torch.float32, device=dev)
    d.output = out.data_ptr()
    with torch.cuda.device(dev):
        if f16:
            d.arith, d.range_flag = _lib.DCN_F16X2, _range_flag(dev).data_ptr()
        _lib.check(_lib.lib().c2m_dcn_v2_forward_nhwc(_stream(), d), "c2m_dcn_v2_forward_nhwc")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The padding band of a zero-padded Ref (csrc/ref_band.hip): behind the live region plus a layer's receptive radius a
# Ref-side feature map depends on the distances to the canvas edges only.  The Ref towers launch their convolutions on the
# top-left tiles, run the same layers on a small all-zero canvas (the template) and copy the band from it: the same bits.
# ---------------------------------------------------------------------------------------------------------------------
_ref_band_on = True   # what the fused Ref-side forwards do by default; ref_band_mode saves, sets and restores it


class ref_band_mode:
    """`with ops.ref_band_mode(0): ...` -- the Ref-side towers launch every tile (the path before the band fill); (1): live
    tiles + band fill (default).  Results are identical; for every thread's forwards through this module while the block is
    open (measurement / tests).  Per call: vgg_stack_forward(live=...)."""

    def __init__(self, mode):
        self.mode = int(mode)
        if self.mode not in (0, 1):
            raise _lib.C2MError("ref_band_mode: 0 or 1")

    def __enter__(self):
        global _ref_band_on
        self.prev, _ref_band_on = _ref_band_on, self.mode == 1
        return self

    def __exit__(self, *exc):
        global _ref_band_on
        _ref_band_on = self.prev
        return False


def conv_roi_tile(rgb64=False):
    """(rows, columns) of the pixel tile of a workgroup: of conv3x3_rgb64's kernel, or of the split kernels (what `roi_tiles`
    counts; c2m_conv3x3_roi_tile: host-side, no GPU needed)."""
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.lib().c2m_conv3x3_roi_tile(int(bool(rgb64)), ctypes.byref(th), ctypes.byref(tw)), "c2m_conv3x3_roi_tile")
    return th.value, tw.value


def band_src_index(v, n, t, margin):
    """The fill's edge-distance clamp (csrc/ref_band.hip band_src) for coordinate v of an extent n and a template extent t."""
    return v if v < margin else (t - (n - v) if n - v <= margin else margin)


def stack_geometry(layers):
    """['conv' | 'pool', ...] of an ordered {name: layer} stack (ReLUs dropped): what ref_band_plan walks."""
    return ["conv" if isinstance(m, torch.nn.Conv2d) else "pool" for m in layers.values()
            if isinstance(m, (torch.nn.Conv2d, torch.nn.MaxPool2d))]


def ref_band_plan(geometry, H, W, live_h, live_w, first_rgb64=True, tiles=None):
    """Host arithmetic of the band path for a stack of 3x3 / pad 1 convolutions and 2x2 / stride 2 pools on an H x W canvas whose
    non-zero pixels lie inside [0, live_h) x [0, live_w).  geometry: ['conv' | 'pool', ...] in order.  tiles: ((th, tw) of the
    first-layer kernel, (th, tw) of the split kernels), default: the library's.  Per convolution, at its own resolution (scale
    s = 2^pools before it): R = its cumulative receptive radius in full-resolution pixels (each convolution adds s), the extent
    that can differ from the band ceil((live + R) / s), and that extent in whole tiles.  -> None where the path declines (no
    layer would skip a tile, or a map is too small to have an interior), else
    {'convs': [{'scale', 'radius', 'extent': (h, w), 'tile': (th, tw), 'tiles': (rows, columns), 'roi': (rows, columns)}, ...],
     'template': (Ht, Wt)}: the template canvas has >= 2 R + 2 coarsest-scale tiles on every side."""
    if tiles is None:
        tiles = (conv_roi_tile(True), conv_roi_tile(False))
    n_pool = sum(1 for g in geometry if g == "pool")
    if live_h is None or live_w is None or H % (1 << n_pool) != 0 or W % (1 << n_pool) != 0 or (live_h >= H and live_w >= W):
        return None
    convs, s, R, any_saved = [], 1, 0, False
    for k, g in enumerate(geometry):
        if g == "pool":
            s *= 2
            continue
        R += s
        th, tw = tiles[0] if (k == 0 and first_rgb64) else tiles[1]
        Hc, Wc = H // s, W // s
        full = (-(-Hc // th), -(-Wc // tw))
        ext = (-(-(live_h + R) // s), -(-(live_w + R) // s))
        roi = (max(1, min(full[0], -(-ext[0] // th))), max(1, min(full[1], -(-ext[1] // tw))))
        any_saved |= roi != full
        convs.append({"scale": s, "radius": R, "extent": ext, "tile": (th, tw), "tiles": full, "roi": roi})
    if not convs or not any_saved:
        return None
    align = 4 * s
    th, tw = tiles[1]
    Ht = -(-(2 * R + 2 * s * th) // align) * align
    Wt = -(-(2 * R + 2 * s * tw) // align) * align
    for c in convs:   # every map (and its pooled successor: scale 2 s) keeps three disjoint zones of the clamp
        for sc in (c["scale"], 2 * c["scale"]):
            m = band_margin(c["radius"], sc)
            if min(H // sc, W // sc, Ht // sc, Wt // sc) < 2 * m + 1:
                return None
    return {"convs": convs, "template": (Ht, Wt)}


def band_margin(radius, scale):
    """Pixels (at `scale`) from a canvas edge within which a map of receptive radius `radius` (full-resolution pixels) may see
    that edge: ceil(radius / scale), plus one to spare."""
    return -(-radius // scale) + 1


def ref_live_extent(img):
    """img [B,3,H,W] float32 on the GPU -> (live_h, live_w) host ints: the bounding box, anchored at (0, 0), of the pixels that
    are not exactly 0.0 in all three channels, over the batch.  One kernel launch and one 8-byte read-back."""
    if not img.is_cuda or img.dim() != 4 or img.shape[1] != 3 or img.dtype != torch.float32 or not img.is_contiguous():
        raise _lib.C2MError("ref_live_extent: a contiguous float32 GPU tensor [B,3,H,W]")
    B, _, H, W = img.shape
    ext = torch.zeros(2, dtype=torch.int32, device=img.device)
    with torch.cuda.device(img.device):
        _lib.check(_lib.lib().c2m_ref_live_extent_f32(_stream(), img.data_ptr(), B, H, W, ext.data_ptr()), "c2m_ref_live_extent_f32")
    lh, lw = ext.tolist()
    return int(lh), int(lw)


def ref_live_extent_shared(img):
    """ref_live_extent(img) for the fused Ref-side forwards, or None where the band path does not apply (switched off, not a
    contiguous float32 GPU image, a stream capture: no read-back).  Inside an f16_range_guard -- one inference step of
    RefRestorationModel.test() / bench.py -- the extent of an image is read once and shared by the modules of that step; it
    is never kept across guards."""
    if (not _ref_band_on or not isinstance(img, torch.Tensor) or not img.is_cuda or img.dim() != 4 or img.shape[1] != 3 or
            img.dtype != torch.float32 or not img.is_contiguous() or img.numel() >= 2 ** 31 or
            torch.cuda.is_current_stream_capturing()):
        return None
    cache = getattr(_tls, "live_cache", None)
    key = (img.data_ptr(), tuple(img.shape), img._version, img.device)
    if cache is not None and key in cache:
        return cache[key]
    live = ref_live_extent(img)
    if cache is not None:
        cache[key] = live
    return live


def band_fill(dst, tmpl, roi_h, roi_w, margin_y, margin_x, layout="nhwc"):
    """Write every pixel of `dst` outside [0, roi_h) x [0, roi_w) from the one-sample template through the edge-distance clamp
    (c2m_band_fill_f32).  layout "nhwc": logical [B,C,H,W] tensors with channel stride 1 (channels-last tensors, interior views
    of bordered buffers); "grouped8": zero-bordered group-major buffers [B,C/8,H+3,W+3,8]; "nchw": contiguous [B,C,H,W]."""
    L = _lib.lib()
    if layout == "grouped8":
        B, G, Hb, Wb, e = dst.shape
        _, Gt, Htb, Wtb, et = tmpl.shape
        if e != 8 or et != 8 or G != Gt or not dst.is_contiguous() or not tmpl.is_contiguous() or tmpl.shape[0] != 1:
            raise _lib.C2MError("band_fill: grouped8 buffers are contiguous [B, C/8, H+3, W+3, 8]")
        H, W, Ht, Wt = Hb - 3, Wb - 3, Htb - 3, Wtb - 3
        args = (dst.data_ptr() + (Wb + 1) * 32, B, G * 8, H, W, 8, 8, Wb * 8, Hb * Wb * 8, G * Hb * Wb * 8,
                tmpl.data_ptr() + (Wtb + 1) * 32, Ht, Wt, 8, Wtb * 8, Htb * Wtb * 8)
        planar = 0
    elif layout == "nhwc":
        B, C, H, W = dst.shape
        Ht, Wt = tmpl.shape[2:]
        d, t = _nhwc_src(dst, "dst"), _nhwc_src(tmpl, "tmpl")
        if tmpl.shape[0] != 1 or tmpl.shape[1] != C:
            raise _lib.C2MError("band_fill: the template is [1, C, Ht, Wt]")
        args = (dst.data_ptr(), B, C, H, W, C, d.pix_pitch, d.row_pitch, 0, d.img_pitch,
                tmpl.data_ptr(), Ht, Wt, t.pix_pitch, t.row_pitch, 0)
        planar = 0
    elif layout == "nchw":
        B, C, H, W = dst.shape
        Ht, Wt = tmpl.shape[2:]
        if not dst.is_contiguous() or not tmpl.is_contiguous() or tuple(tmpl.shape[:2]) != (1, C):
            raise _lib.C2MError("band_fill: nchw tensors are contiguous, the template [1, C, Ht, Wt]")
        args = (dst.data_ptr(), B, C, H, W, 1, 0, 0, 0, 0, tmpl.data_ptr(), Ht, Wt, 0, 0, 0)
        planar = 1
    else:
        raise _lib.C2MError(f"band_fill: unknown layout {layout}")
    if dst.dtype != torch.float32 or tmpl.dtype != torch.float32 or not dst.is_cuda or tmpl.device != dst.device:
        raise _lib.C2MError("band_fill: float32 GPU tensors on one device")
    with torch.cuda.device(dst.device):
        _lib.check(L.c2m_band_fill_f32(_stream(), *args, int(roi_h), int(roi_w), int(margin_y), int(margin_x), planar),
                   "c2m_band_fill_f32")
    return dst


class _RefBand:
    """State of one vgg_stack_forward on the band path: the plan, the template's current activation and the position in
    both.  conv() runs one layer: the template (every tile, B = 1), the image (the plan's tiles) and the fill."""

    def __init__(self, plan, H, W, dev, algo):
        self.plan, self.H, self.W, self.algo, self.k = plan, H, W, algo, 0
        self.tcur = torch.zeros((1, 3) + tuple(plan["template"]), dtype=torch.float32, device=dev)

    def conv(self, call, first, src, cout, out_mode, out, out2):
        c = self.plan["convs"][self.k]
        self.k += 1
        # the same kernel kind and arithmetic for the template as for the image, whatever the size-dependent rules would pick
        extra = {} if first else {"algo": self.algo}
        t2 = None
        if out2 is not None:
            t2 = torch.empty((1, cout // 8, self.tcur.shape[2] + 3, self.tcur.shape[3] + 3, 8), dtype=torch.float32, device=src.device)
        t_out = call(self.tcur, None, t2, **extra)
        self.tcur = t_out
        if c["roi"] == c["tiles"]:
            return call(src, out, out2, **extra)
        res = call(src, out, out2, roi_tiles=c["roi"], **extra)
        pooled = out_mode == "nhwc_pool2"
        so = c["scale"] * (2 if pooled else 1)
        Hc, Wc = self.H // c["scale"], self.W // c["scale"]
        roi_h, roi_w = min(c["roi"][0] * c["tile"][0], Hc), min(c["roi"][1] * c["tile"][1], Wc)
        if pooled:
            roi_h, roi_w = roi_h // 2, roi_w // 2
        m = band_margin(c["radius"], so)
        band_fill(res, t_out, roi_h, roi_w, m, m, layout="nchw" if out_mode == "nchw" else "nhwc")
        if out2 is not None:
            band_fill(out2, t2, roi_h, roi_w, m, m, layout="grouped8")
        return res


# ---------------------------------------------------------------------------------------------------------------------
# VGG-style feature stacks (conv3x3 + ReLU + 2x2 max-pool) on the channels-last kernels
# ---------------------------------------------------------------------------------------------------------------------
def _bordered_empty(B, C, H, W, device, grouped8=False):
    """BorderedNHWC whose border is zero and whose interior is uninitialised (to be written by a conv epilogue).
    grouped8: also allocate the group-major twin (same border)."""
    def zero_border(t):     # [..., H + 3, W + 3, channels]: row 0, rows H + 1 .., column 0, columns W + 1 ..
        t[..., 0, :, :].zero_()
        t[..., H + 1:, :, :].zero_()
        t[..., 1:H + 1, 0, :].zero_()
        t[..., 1:H + 1, W + 1:, :].zero_()
        return t

    o = BorderedNHWC.__new__(BorderedNHWC)
    o.B, o.C, o.H, o.W = B, C, H, W
    o.buf = zero_border(torch.empty((B, H + 3, W + 3, C), dtype=torch.float32, device=device))
    if grouped8:
        if C % 8 != 0:
            raise _lib.C2MError("a group-major twin needs C % 8 == 0")
        o.grouped8 = zero_border(torch.empty((B, C // 8, H + 3, W + 3, 8), dtype=torch.float32, device=device))
    return o


def bordered_of(t):
    """The BorderedNHWC a tensor is the interior view of (set by vgg_stack_forward), else None."""
    return getattr(t, "_c2m_bordered", None)


def _pool_is_2x2(m):
    two = lambda v: v in (2, (2, 2))   # noqa: E731
    return two(m.kernel_size) and two(m.stride) and m.padding in (0, (0, 0)) and m.dilation in (1, (1, 1)) and not m.ceil_mode


def _band_split_ok(layer, fast):
    """conv3x3's automatic choice for this layer is a split kernel at every map size (what the band path launches by name)."""
    co, ci = layer.weight.shape[:2]
    return (_SPLIT == "all" or ((fast or bf16_autocast()) and _SPLIT != "0")) and ci % 16 == 0 and co % 4 == 0


def vgg_stack_forward(layers, x, taps=(), mean=None, std=None, last_nchw=False, grouped8_taps=(), fast=False, live=None):
    """Run an ordered {name: nn.Conv2d(3x3, pad 1) | nn.ReLU | nn.MaxPool2d(2, 2)} stack (torchvision's vgg `features`
    layout, mmsr/models/archs/vgg_arch.py:107-123) on the fused channels-last convolution: every conv + its ReLU is one
    launch.  x: [B,3,H,W] image; (x - mean) / std is applied while the image is widened to the kernel's 32-channel chunk.
    Returns {tap name: tensor}; tapped activations are written by the conv epilogue straight into zero-bordered
    channels-last buffers (logical NCHW views of their interiors are returned: the DCNv2 gathers and the offset
    convolutions of the decoder read those buffers in place).  last_nchw: the final layer's output as a contiguous NCHW
    tensor under the key of that layer (the correlation kernels read planar features).  grouped8_taps: taps that also get
    the group-major twin (BorderedNHWC.grouped8) a DCNv2 layer with 8-channel deformable groups gathers from.  fast: as in
    conv3x3 (the split-bf16 kernel for every layer but the first): the VGG taps of the Ref do, the extractor towers that feed
    the index search do not.  live: (live_h, live_w) of a zero-padded Ref (ref_live_extent) or None -- the convolutions launch
    only the tiles the live region reaches and the band behind them is filled from a template (_RefBand): the same bits.  The
    path declines (every tile is launched) where no tile would be skipped or the stack is not one it covers."""
    names = list(layers.keys())
    B, C, H, W = x.shape
    dev = x.device
    # cached weight images follow in-place writes through .data (which the version counter does not see)
    refresh_weight_caches([p_ for layer_ in layers.values() for p_ in layer_.parameters()])
    first = layers[names[0]]
    rgb64 = C == 3 and isinstance(first, torch.nn.Conv2d) and tuple(first.weight.shape) == (64, 3, 3, 3)
    if rgb64:
        cur = x      # the first layer reads the planar image itself and normalises it while staging
    else:
        cur = torch.zeros((B, 32, H, W), dtype=torch.float32, device=dev).contiguous(memory_format=torch.channels_last)
        xin = x.float()
        if mean is not None:
            xin = (xin - mean) / std
        cur[:, :C] = xin
    out, k = {}, 0
    band = None
    convs_ = [m for m in layers.values() if isinstance(m, torch.nn.Conv2d)]
    if (live is not None and rgb64 and x.dtype == torch.float32 and
            all(isinstance(m, (torch.nn.Conv2d, torch.nn.ReLU)) or (isinstance(m, torch.nn.MaxPool2d) and _pool_is_2x2(m))
                for m in layers.values()) and
            all(m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == (1, 1) and m.groups == 1 for m in convs_) and
            all(_band_split_ok(m, fast) for m in convs_[1:])):
        plan = ref_band_plan(stack_geometry(layers), H, W, live[0], live[1])
        if plan is not None:
            band = _RefBand(plan, H, W, dev, _KINDS[_split_kind(None)].name)

    def conv(k_, src, layer_, act=ACT_NONE, out_mode="nhwc", out=None, out2_grouped8=None):
        first = k_ == 0 and rgb64

        def call(src_, out_, out2_, **kw):
            if first:
                return conv3x3_rgb64(src_, layer_.weight, layer_.bias, act=act, mean=mean, std=std, out=out_, out2_grouped8=out2_, **kw)
            return conv3x3(src_, layer_.weight, layer_.bias, act=act, out_mode=out_mode, out=out_, out2_grouped8=out2_, fast=fast, **kw)
        if band is None:
            return call(src, out, out2_grouped8)
        return band.conv(call, first, src, layer_.out_channels, out_mode, out, out2_grouped8)

    while k < len(names):
        name, layer = names[k], layers[names[k]]
        if isinstance(layer, torch.nn.Conv2d):
            if layer.kernel_size != (3, 3) or layer.stride != (1, 1) or layer.padding != (1, 1) or layer.groups != 1:
                raise _lib.C2MError(f"vgg_stack_forward: {name} is not a 3x3 / stride 1 / pad 1 convolution")
            relu = k + 1 < len(names) and isinstance(layers[names[k + 1]], torch.nn.ReLU)
            tap_name = names[k + 1] if (relu and names[k + 1] in taps) else (name if name in taps and not relu else None)
            if name in taps and relu:
                raise _lib.C2MError("tapping a conv output that is followed by an in-place ReLU is not supported")
            last = (k + (2 if relu else 1)) >= len(names)
            Bc, _, Hc, Wc = cur.shape
            nxt = layers[names[k + 2]] if (relu and k + 2 < len(names)) else None
            pool = (isinstance(nxt, torch.nn.MaxPool2d) and _pool_is_2x2(nxt) and tap_name is None and not (k == 0 and rgb64) and
                    Hc % 2 == 0 and Wc % 2 == 0 and
                    (_wino_ok([cur], layer.weight, "nhwc_pool2", Wc) or _split_ok([cur], layer.weight, fast)))
            if last and last_nchw:
                cur = conv(-1, cur, layer, act=ACT_RELU if relu else ACT_NONE, out_mode="nchw")
                out[names[k + 1] if relu else name] = cur
            elif tap_name is not None:
                bo = _bordered_empty(Bc, layer.out_channels, Hc, Wc, dev, grouped8=tap_name in grouped8_taps)
                view = bo.interior()
                conv(k, cur, layer, act=ACT_RELU if relu else ACT_NONE, out=view, out2_grouped8=bo.grouped8)
                view._c2m_bordered = bo
                out[tap_name] = view
                cur = view
            elif pool:   # conv -> ReLU -> MaxPool2d(2, 2) in one launch: only the pooled map is written
                cur = conv(k, cur, layer, act=ACT_RELU, out_mode="nhwc_pool2")
                k += 1   # (the pool layer)
            else:
                cur = conv(k, cur, layer, act=ACT_RELU if relu else ACT_NONE)
            k += 2 if relu else 1
        elif isinstance(layer, torch.nn.MaxPool2d):
            cur = torch.nn.functional.max_pool2d(cur, layer.kernel_size, layer.stride, layer.padding)
            if band is not None:
                band.tcur = torch.nn.functional.max_pool2d(band.tcur, layer.kernel_size, layer.stride, layer.padding)
            k += 1
        elif isinstance(layer, torch.nn.ReLU):
            cur = torch.relu(cur)
            if band is not None:
                band.tcur = torch.relu(band.tcur)
            k += 1
        else:
            raise _lib.C2MError(f"vgg_stack_forward: unsupported layer {name}: {type(layer).__name__}")
    return out


# ---- contrastive correspondence loss of the extractor training (stages 1-2; csrc/contras_loss.hip) --------------------

CONTRAS_MIN_IDS = 128   # a sample with fewer valid correspondences is skipped (teacher_contras_model.py:155-156)


def contras_correspondences(transformed_coordinates, H1, W1, scaling_steps=2, min_ids=CONTRAS_MIN_IDS):
    """The valid correspondences of a whole batch (the reference's per-sample `warp` + skip test, batched).

    transformed_coordinates [B, >=4*H1 (rows), >=4*W1, >=2]: (x, y) in image pixels; the grid is sampled at [::4, ::4].
    A position is valid iff 10 < x < 4*W1-10 and 10 < y < 4*H1-10 (strict); pos2 = round((y, x) / 2**scaling_steps)
    with torch.round (half to even).  Samples with fewer than `min_ids` valid positions are dropped.
    -> dict: ids [Ntot] int32 (ascending per sample), pos2 [Ntot, 2] int32 (y, x), offsets [B+1] int32, keep [B] bool,
    counts (host list of rows per sample after the skip), n_valid (host int).  Pure batched torch on the tensor's own
    device; one small device->host copy for the counts."""
    tc = transformed_coordinates[:, ::4, ::4, :2]
    B = tc.shape[0]
    if tc.shape[1] != H1 or tc.shape[2] != W1:
        raise ValueError(f"transformed_coordinates[:, ::4, ::4] is {tuple(tc.shape[1:3])}, the feature grid is {(H1, W1)}")
    x = tc[..., 0].reshape(B, -1)
    y = tc[..., 1].reshape(B, -1)
    valid = (x > 10) & (x < 4 * W1 - 10) & (y > 10) & (y < 4 * H1 - 10)
    keep = valid.sum(1) >= min_ids
    valid = valid & keep[:, None]
    counts = valid.sum(1)
    nz = valid.nonzero()                                  # row-major: sample, then ascending grid index
    bi, ids = nz[:, 0], nz[:, 1]
    div = float(2 ** scaling_steps)
    pos2 = torch.stack([torch.round(y[bi, ids] / div), torch.round(x[bi, ids] / div)], 1).to(torch.int32)
    offsets = torch.zeros(B + 1, dtype=torch.int32, device=tc.device)
    offsets[1:] = torch.cumsum(counts, 0).to(torch.int32)
    return {"ids": ids.to(torch.int32).contiguous(), "pos2": pos2.contiguous(), "offsets": offsets, "keep": keep,
            "counts": [int(c) for c in counts.cpu()], "n_valid": int(keep.sum())}


class _ContrasLossFn(torch.autograd.Function):
    """(f1, f2) -> terms [B, 2] = per-sample (hinge, KL), dists [B, 2] = per-sample (mean pos, mean min(neg1, neg2)).
    The teacher maps are constants (no gradient); dists is not differentiable."""

    @staticmethod
    def forward(ctx, f1, f2, tf1, tf2, corr, margin, safe_radius, temperature):
        B, C, H1, W1 = f1.shape
        H2, W2 = f2.shape[2], f2.shape[3]
        teacher = tf1 is not None
        Ntot, max_n = int(corr["ids"].numel()), max(corr["counts"])
        L = _lib.lib()
        nbytes = L.c2m_contras_loss_workspace_bytes(B, C, H1, W1, Ntot, int(teacher))
        if nbytes == 0:
            raise _lib.C2MError("c2m_contras_loss_workspace_bytes: invalid shapes")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=f1.device)
        out = torch.empty((B, 4), dtype=torch.float32, device=f1.device)
        with torch.cuda.device(f1.device):
            _lib.check(L.c2m_contras_loss_forward_f32(
                _stream(), f1.data_ptr(), f2.data_ptr(), tf1.data_ptr() if teacher else None,
                tf2.data_ptr() if teacher else None, B, C, H1, W1, H2, W2, corr["ids"].data_ptr(), corr["pos2"].data_ptr(),
                corr["offsets"].data_ptr(), Ntot, max_n, float(margin), float(safe_radius), float(temperature),
                out.data_ptr(), ws.data_ptr(), nbytes), "c2m_contras_loss_forward_f32")
        ctx.meta = (B, C, H1, W1, H2, W2, Ntot, max_n, float(margin), float(safe_radius), float(temperature), teacher, nbytes)
        ctx.corr = corr
        corr["_workspace"] = ws          # (contras_loss_rows reads the per-row statistics from it)
        ctx.save_for_backward(ws)
        dists = out[:, 1:3].contiguous()
        ctx.mark_non_differentiable(dists)
        return out[:, 0::3].contiguous(), dists

    @staticmethod
    def backward(ctx, g_terms, g_dists):
        (ws,) = ctx.saved_tensors
        B, C, H1, W1, H2, W2, Ntot, max_n, margin, radius, tau, teacher, nbytes = ctx.meta
        corr = ctx.corr
        g_terms = (g_terms if g_terms is not None else torch.zeros((B, 2), device=ws.device)).float().contiguous()
        gf1 = torch.empty((B, C, H1, W1), dtype=torch.float32, device=ws.device)
        gf2 = torch.empty((B, C, H2, W2), dtype=torch.float32, device=ws.device)
        with torch.cuda.device(ws.device):
            _lib.check(_lib.lib().c2m_contras_loss_backward_f32(
                _stream(), B, C, H1, W1, H2, W2, corr["ids"].data_ptr(), corr["pos2"].data_ptr(),
                corr["offsets"].data_ptr(), Ntot, max_n, margin, radius, tau, int(teacher), g_terms.data_ptr(),
                gf1.data_ptr(), gf2.data_ptr(), ws.data_ptr(), nbytes), "c2m_contras_loss_backward_f32")
        return gf1, gf2, None, None, None, None, None, None


def contras_loss(f1, f2, transformed_coordinates, margin=1.0, safe_radius=4, scaling_steps=2, teacher=None,
                 temperature=0.15, distill_weight=15.0):
    """The extractor-training loss of C2-Matching for a whole batch on the fused gfx950 kernels.

    f1 [B,C,H1,W1], f2 [B,C,H2,W2]: the (student) dense features, float32 on the GPU; gradients flow to both.
    teacher: None (stage 1, TeacherContrasModel) or a pair (tf1, tf2) of the teacher's features (stage 2,
    StudentContrasDistillationModel); the teacher is a constant: no gradient reaches it.
    -> (loss [1], pos_dist, neg_dist) for stage 1, (loss [1], pos_dist, neg_dist, distill_loss) for stage 2 -- the
    reference's return tuples.  Raises NotImplementedError when every sample has fewer than 128 valid correspondences,
    as the reference does."""
    f1, f2 = _dev_f32(f1, "f1"), _dev_f32(f2, "f2")
    if f1.dim() != 4 or f2.dim() != 4 or f1.shape[:2] != f2.shape[:2] or f1.device != f2.device:
        raise _lib.C2MError("f1 / f2 must be [B,C,H,W] with equal B, C and device")
    tf1 = tf2 = None
    if teacher is not None:
        tf1, tf2 = (_dev_f32(t.detach(), n) for t, n in zip(teacher, ("teacher f1", "teacher f2")))
        if tf1.shape != f1.shape or tf2.shape != f2.shape:
            raise _lib.C2MError("teacher features must have the student's shapes")
    if not isinstance(transformed_coordinates, torch.Tensor) or not transformed_coordinates.is_cuda:
        raise _lib.C2MError("transformed_coordinates must be a tensor on the GPU")
    B, C, H1, W1 = f1.shape
    corr = contras_correspondences(transformed_coordinates.to(f1.device), H1, W1, scaling_steps)
    if corr["n_valid"] == 0:
        raise NotImplementedError("no sample has 128 valid correspondences")
    H2, W2 = f2.shape[2], f2.shape[3]
    if corr["pos2"].numel():
        lim = torch.stack([corr["pos2"].min(0).values, corr["pos2"].max(0).values]).cpu()
        if int(lim[0].min()) < 0 or int(lim[1, 0]) >= H2 or int(lim[1, 1]) >= W2:
            raise IndexError(f"pos2 outside the {H2}x{W2} map of f2")
    terms, dists = _ContrasLossFn.apply(f1, f2, tf1, tf2, corr, margin, safe_radius, temperature)
    wgt = corr["keep"].to(torch.float32)
    n = float(corr["n_valid"])
    if teacher is None:
        loss = (terms[:, 0] * wgt).sum().view(1) / n
    else:
        loss = ((terms[:, 0] + distill_weight * terms[:, 1]) * wgt).sum().view(1) / n
    pos_dist = (dists[:, 0] * wgt).sum() / n
    neg_dist = (dists[:, 1] * wgt).sum() / n
    if teacher is None:
        return loss, pos_dist, neg_dist
    return loss, pos_dist, neg_dist, (terms[:, 1] * wgt).sum() / n


def contras_loss_rows(f1, f2, transformed_coordinates, margin=1.0, safe_radius=4, scaling_steps=2, teacher=None,
                      temperature=0.15):
    """Forward only, for inspection: the per-row statistics of contras_loss for the kept samples, concatenated in
    sample order -> dict of pos, neg1, neg2 [Ntot] and the arg-mins neg1_idx (grid position in f1) / neg2_idx (row within
    the sample's valid list) [Ntot] int32, plus the correspondences (ids, pos2, offsets, counts, keep)."""
    f1, f2 = _dev_f32(f1, "f1"), _dev_f32(f2, "f2")
    B, C, H1, W1 = f1.shape
    corr = contras_correspondences(transformed_coordinates.to(f1.device), H1, W1, scaling_steps)
    if corr["n_valid"] == 0:
        raise NotImplementedError("no sample has 128 valid correspondences")
    tf1, tf2 = (None, None) if teacher is None else (_dev_f32(teacher[0], "teacher f1"), _dev_f32(teacher[1], "teacher f2"))
    with torch.no_grad():
        _ContrasLossFn.apply(f1, f2, tf1, tf2, corr, margin, safe_radius, temperature)
    ws = corr.pop("_workspace")
    N = int(corr["ids"].numel())
    rows = {k: torch.empty(N, dtype=torch.float32, device=f1.device) for k in ("pos", "neg1", "neg2")}
    rows.update({k: torch.empty(N, dtype=torch.int32, device=f1.device) for k in ("neg1_idx", "neg2_idx")})
    with torch.cuda.device(f1.device):
        _lib.check(_lib.lib().c2m_contras_loss_rows_f32(
            _stream(), B, C, H1, W1, N, int(teacher is not None), ws.data_ptr(), ws.numel(), rows["pos"].data_ptr(),
            rows["neg1"].data_ptr(), rows["neg1_idx"].data_ptr(), rows["neg2"].data_ptr(), rows["neg2_idx"].data_ptr()),
            "c2m_contras_loss_rows_f32")
    rows.update(corr)
    return rows


# ---- training pairs of the extractor training (stages 1-2; csrc/contras_pairs.hip) ------------------------------------

_PIL_PRECISION_BITS = 32 - 8 - 2


def _dev_u8(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.C2MError(f"{name} must be a tensor on the GPU (the HIP path has no CPU fallback)")
    if t.dtype != torch.uint8:
        raise _lib.C2MError(f"{name} must be uint8, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _pil_bicubic_weight(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pil_bicubic_tables(in_size, out_size):
    """Pillow's fixed-point bicubic coefficients for resampling one axis from in_size to out_size (Resample.c:
    precompute_coeffs + normalize_coeffs_8bpc, 22 fraction bits), in banded form: (start [out] int32, count [out] int32,
    coeff [out, K] int32 with K = the largest count, rows padded with zeros).  Row i weighs input pixels
    start[i] .. start[i] + count[i] - 1.  Host tensors; the same numbers as the non-zero band of
    mmsr.data.pil_bicubic._coeff_matrix."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError("sizes must be positive")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    rows, starts = [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = [_pil_bicubic_weight((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        row = []
        for v in w:
            k = v / ww if ww != 0.0 else v
            row.append(int(-0.5 + k * (1 << _PIL_PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << _PIL_PRECISION_BITS)))
        # the kernel accumulates in int32: 255 * sum |c| plus the rounding constant must fit
        if 255 * sum(abs(c) for c in row) + (1 << (_PIL_PRECISION_BITS - 1)) >= 1 << 31:
            raise _lib.C2MError(f"pil_bicubic_tables({in_size}, {out_size}): row {xx} can overflow an int32 accumulator")
        rows.append(row)
        starts.append(xmin)
    K = max(1, max(len(r) for r in rows))
    coeff = torch.zeros((out_size, K), dtype=torch.int32)
    for i, r in enumerate(rows):
        if r:
            coeff[i, :len(r)] = torch.tensor(r, dtype=torch.int32)
    return (torch.tensor(starts, dtype=torch.int32), torch.tensor([len(r) for r in rows], dtype=torch.int32), coeff)


_pil_tables = {}
_pil_tables_lock = threading.Lock()


def _pil_tables_on(in_size, out_size, device):
    key = (int(in_size), int(out_size), str(device))
    with _pil_tables_lock:
        if key not in _pil_tables:
            _pil_tables[key] = tuple(t.to(device) for t in pil_bicubic_tables(in_size, out_size))
        return _pil_tables[key]


def _pil_pass(x, vertical, out_size, as_float):
    N, (H, W) = x.numel() // (x.shape[-2] * x.shape[-1]), x.shape[-2:]
    start, count, coeff = _pil_tables_on(H if vertical else W, out_size, x.device)
    shape = tuple(x.shape[:-2]) + ((out_size, W) if vertical else (H, out_size))
    out = torch.empty(shape, dtype=torch.uint8, device=x.device)
    outf = torch.empty(shape, dtype=torch.float32, device=x.device) if as_float else None
    _lib.check(_lib.lib().c2m_pil_bicubic_u8(_stream(), x.data_ptr(), N, H, W, int(vertical), int(out_size), start.data_ptr(),
                                             count.data_ptr(), coeff.data_ptr(), coeff.shape[1], out.data_ptr(),
                                             outf.data_ptr() if as_float else None), "c2m_pil_bicubic_u8")
    return out, outf


def pil_bicubic_resize_u8(img_u8, out_h, out_w, as_float=False):
    """img_u8: uint8 [..., H, W] on the GPU -> uint8 [..., out_h, out_w], identical to ``PIL.Image.resize((out_w, out_h),
    Image.BICUBIC)`` per plane (and to mmsr.data.pil_bicubic.pil_bicubic_resize): a horizontal and a vertical launch in
    Pillow's integer arithmetic with the uint8 intermediate between them; an axis whose size does not change is skipped.
    as_float: -> (uint8, float32 = uint8 / 255 exactly), the float image written by the last pass (when no axis changes
    size, by one pass with the identity table)."""
    x = _dev_u8(img_u8, "img_u8")
    if x.dim() < 2 or x.numel() == 0:
        raise _lib.C2MError("img_u8 must be a non-empty [..., H, W] tensor")
    out_h, out_w = int(out_h), int(out_w)
    if out_h <= 0 or out_w <= 0:
        raise _lib.C2MError("out_h / out_w must be positive")
    H, W = x.shape[-2:]
    passes = [(False, out_w)] if W != out_w else []
    if H != out_h:
        passes.append((True, out_h))
    if not passes:
        if not as_float:
            return x.clone()
        passes = [(False, W)]
    xf = None
    with torch.cuda.device(x.device):
        for k, (vertical, size) in enumerate(passes):
            x, xf = _pil_pass(x, vertical, size, as_float and k == len(passes) - 1)
    return (x, xf) if as_float else x


# ---- stage-3 batches: both resampling passes in one launch, flips / transpose on read (csrc/ref_pairs.hip) ---------------

PIL2D_FLIP_H, PIL2D_FLIP_V, PIL2D_TRANSPOSE = 1, 2, 4      # the flag bits of a sample, applied in this order
_PIL2D_TILE = 32                                           # C2M_PIL2D_TILE of include/c2m_hip.h
_PIL2D_LDS_BUDGET = 64 * 1024                              # C2M_PIL2D_LDS_BUDGET

Pil2dPlan = collections.namedtuple("Pil2dPlan", "win_h win_w Kh Kv lds_bytes fused")
_pil2d_plans = {}


def _pil2d_window(in_size, out_size):
    """-> (the largest source window of any run of _PIL2D_TILE output pixels, K) of one axis' table."""
    start, count, coeff = pil_bicubic_tables(in_size, out_size)
    start, end = start.tolist(), (start + count).tolist()
    win = max(max(end[t:t + _PIL2D_TILE]) - min(start[t:t + _PIL2D_TILE]) for t in range(0, len(start), _PIL2D_TILE))
    return max(win, 1), int(coeff.shape[1])


def pil_bicubic2d_plan(H, W, out_h, out_w):
    """How pil_bicubic_resize2d_u8 runs a geometry: the source window (rows, columns) of one output tile, the tables' tap
    counts, the LDS one workgroup needs, and `fused`: whether that fits the kernel's budget (else: two passes)."""
    key = (int(H), int(W), int(out_h), int(out_w))
    with _pil_tables_lock:
        if key not in _pil2d_plans:
            (win_h, Kv), (win_w, Kh) = _pil2d_window(key[0], key[2]), _pil2d_window(key[1], key[3])
            lds = int(_lib.lib().c2m_pil_bicubic2d_lds_bytes(Kh, Kv, win_h, win_w))
            _pil2d_plans[key] = Pil2dPlan(win_h, win_w, Kh, Kv, lds, 0 < lds <= _PIL2D_LDS_BUDGET)
        return _pil2d_plans[key]


def _pil2d_flags(flags, samples):
    """flags (None, or one integer 0..7 per sample: a sequence, a numpy array or a CPU tensor) -> list of ints or None."""
    if flags is None:
        return None
    if isinstance(flags, torch.Tensor):
        if flags.is_cuda:
            raise _lib.C2MError("flags stay on the host (they are checked there and uploaded with the launch)")
        flags = flags.tolist()
    try:
        fl = [int(f) for f in flags]
    except (TypeError, ValueError):
        raise _lib.C2MError("flags must be one integer per sample")
    if len(fl) != samples or any(f < 0 or f > 7 for f in fl):
        raise _lib.C2MError(f"flags must be {samples} integers in 0..7 (bit 0 hflip, bit 1 vflip, bit 2 transpose)")
    return fl


def _orient_torch(x, flags):
    """x [S, P, H, W], flags one int per sample -> the oriented batch by torch ops (sample by sample)."""
    out = None
    for b, f in enumerate(flags):
        if not f:
            continue
        s = x[b]
        dims = [d for d, bit in ((2, PIL2D_FLIP_H), (1, PIL2D_FLIP_V)) if f & bit]
        if dims:
            s = torch.flip(s, dims)
        if f & PIL2D_TRANSPOSE:
            s = s.transpose(1, 2)
        if out is None:
            out = x.clone()
        out[b] = s
    return x if out is None else out


def pil_bicubic_resize2d_u8(img_u8, out_h, out_w, flags=None, as_float=False, oriented_float=False):
    """pil_bicubic_resize_u8 in ONE launch, with each sample's orientation applied while its planes are read.

    img_u8: uint8 [H, W], [P, H, W] (one sample) or [S, P, H, W] on the GPU.  flags: None, or one integer per sample on
    the host: bit 0 horizontal flip, bit 1 vertical flip, bit 2 transpose (square planes only), applied in that order as
    the reference's augment does.  -> uint8 [..., out_h, out_w], bit for bit pil_bicubic_resize_u8 of the oriented image
    (Pillow's horizontal pass, uint8, vertical pass; an unchanged axis is skipped).  as_float adds float32 = uint8 / 255
    of the result, oriented_float adds float32 = the oriented, unresized input / 255; the return value is the uint8
    tensor alone or a tuple in that order.
    A workgroup makes one 32 x 32 output tile from a source window held in LDS.  Where that window does not fit the
    kernel's budget (pil_bicubic2d_plan(...).fused is False: down-scaling ratios above about 6) the same bits come from
    torch flips and the two-pass operator."""
    x = _dev_u8(img_u8, "img_u8")
    if x.dim() not in (2, 3, 4) or x.numel() == 0:
        raise _lib.C2MError("img_u8 must be a non-empty [H, W], [P, H, W] or [S, P, H, W] tensor")
    out_h, out_w = int(out_h), int(out_w)
    if out_h <= 0 or out_w <= 0:
        raise _lib.C2MError("out_h / out_w must be positive")
    H, W = x.shape[-2:]
    S = x.shape[0] if x.dim() == 4 else 1
    N = x.numel() // (H * W)
    fl = _pil2d_flags(flags, S)
    if fl is not None and not any(fl):
        fl = None
    if fl is not None and H != W and any(f & PIL2D_TRANSPOSE for f in fl):
        raise _lib.C2MError(f"a transpose flag needs square planes, got {H} x {W}")
    if fl is None and not as_float and not oriented_float and (H, W) == (out_h, out_w):
        return x.clone()
    plan = pil_bicubic2d_plan(H, W, out_h, out_w)
    with torch.cuda.device(x.device):
        if plan.fused:
            shape = tuple(x.shape[:-2]) + (out_h, out_w)
            out = torch.empty(shape, dtype=torch.uint8, device=x.device)
            outf = torch.empty(shape, dtype=torch.float32, device=x.device) if as_float else None
            orient = torch.empty(x.shape, dtype=torch.float32, device=x.device) if oriented_float else None
            fdev = torch.tensor(fl, dtype=torch.uint8).to(x.device) if fl is not None else None
            ht, vt = _pil_tables_on(W, out_w, x.device), _pil_tables_on(H, out_h, x.device)
            _lib.check(_lib.lib().c2m_pil_bicubic2d_u8(
                _stream(), x.data_ptr(), fdev.data_ptr() if fdev is not None else None, N, N // S, H, W, out_h, out_w,
                ht[0].data_ptr(), ht[1].data_ptr(), ht[2].data_ptr(), plan.Kh, vt[0].data_ptr(), vt[1].data_ptr(),
                vt[2].data_ptr(), plan.Kv, plan.win_h, plan.win_w, out.data_ptr(),
                outf.data_ptr() if as_float else None, orient.data_ptr() if oriented_float else None), "c2m_pil_bicubic2d_u8")
        else:
            o = x if fl is None else _orient_torch(x.reshape(S, N // S, H, W), fl).reshape(x.shape)
            out = pil_bicubic_resize_u8(o, out_h, out_w, as_float=as_float)
            out, outf = out if as_float else (out, None)
            orient = pil_bicubic_resize_u8(o, H, W, as_float=True)[1] if oriented_float else None
    res = (out,) + ((outf,) if as_float else ()) + ((orient,) if oriented_float else ())
    return res if len(res) > 1 else out


def warp_perspective_u8(src_u8, M):
    """The reference's ``cv2.warpPerspective(img, H_inverse, (W, H))`` and its transformed-coordinate grid for a batch.

    src_u8 [B,3,H,W] uint8 on the GPU; M [B,3,3] (or [3,3], used for every sample): float64 array or tensor, the matrix
    handed to warpPerspective (the reference's H_inverse).  It is inverted here, on the host, in float64.
    -> (dst_f32 [B,3,H,W] in [0,1], dst_u8 = trunc(dst_f32 * 255), coords [B,H,W,3] float64 = M.(x, y, 1) / third component).
    Bilinear on a 1/32-pixel position grid with a constant zero border (include/c2m_hip.h states the rule); parity with
    OpenCV unpinned."""
    import numpy as np
    src = _dev_u8(src_u8, "src_u8")
    if src.dim() != 4 or src.shape[1] != 3 or src.numel() == 0:
        raise _lib.C2MError("src_u8 must be [B,3,H,W]")
    B, _, H, W = src.shape
    m = np.asarray(M.detach().cpu() if isinstance(M, torch.Tensor) else M, dtype=np.float64)
    if m.shape == (3, 3):
        m = np.broadcast_to(m, (B, 3, 3))
    if m.shape != (B, 3, 3) or not np.isfinite(m).all():
        raise _lib.C2MError(f"M must be {B} finite 3x3 matrices, got shape {m.shape}")
    try:
        mi = np.linalg.inv(m)
    except np.linalg.LinAlgError as e:
        raise _lib.C2MError(f"M is not invertible: {e}")
    mats = torch.from_numpy(np.ascontiguousarray(np.stack([m, mi]))).to(src.device)
    dst_f32 = torch.empty((B, 3, H, W), dtype=torch.float32, device=src.device)
    dst_u8 = torch.empty((B, 3, H, W), dtype=torch.uint8, device=src.device)
    coords = torch.empty((B, H, W, 3), dtype=torch.float64, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().c2m_warp_perspective_u8(_stream(), src.data_ptr(), mats[0].data_ptr(), mats[1].data_ptr(), B, H, W,
                                                      dst_f32.data_ptr(), dst_u8.data_ptr(), coords.data_ptr()),
                   "c2m_warp_perspective_u8")
    return dst_f32, dst_u8, coords


# ---- the end of validation: uint8 images and the metric sums in one pass (csrc/val_metrics.hip) ---------------------------

def val_metrics_tile():
    """(rows, columns) of SSIM-map positions one workgroup of the validation kernel makes, as the library reports them."""
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.lib().c2m_val_metrics_tile(ctypes.byref(th), ctypes.byref(tw)), "c2m_val_metrics_tile")
    return th.value, tw.value


def _image_src(t, name):
    """fp32 [B,3,H,W] (or [3,H,W]) on the GPU -> (the 4-d tensor, its c2m_image_src).  Views are described, never copied."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.C2MError(f"{name} must be a tensor on the GPU (the HIP path has no CPU fallback)")
    if t.dtype != torch.float32:
        raise _lib.C2MError(f"{name} must be float32, got {t.dtype}")
    t = t.detach()
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4 or t.shape[1] != 3 or t.numel() == 0:
        raise _lib.C2MError(f"{name} must be a non-empty [B,3,H,W] tensor, got {tuple(t.shape)}")
    si, sp, sr, sx = t.stride()
    return t, _lib.ImageSrc(t.data_ptr(), sx, sr, sp, si)


def _image_order(images):
    if images not in (None, 'bgr', 'rgb'):
        raise _lib.C2MError(f"images must be None, 'bgr' or 'rgb', got {images!r}")
    return int(images == 'rgb')


def _valid_hw(valid_hw, H, W):
    vh, vw = (H, W) if valid_hw is None else (int(valid_hw[0]), int(valid_hw[1]))
    if not (0 < vh <= H and 0 < vw <= W):
        raise _lib.C2MError(f"valid_hw {(vh, vw)} does not lie inside the {H} x {W} tensor")
    return vh, vw


def tensor_to_u8(t, order='bgr', valid_hw=None):
    """fp32 RGB [B,3,H,W] (or [3,H,W]) on the GPU -> uint8 [B,vh,vw,3] (or [vh,vw,3]) = rint(clamp(t, 0, 1) * 255), half to
    even, channels in `order` ('bgr': the reference's tensor2img; 'rgb': what Pillow writes), of the window valid_hw."""
    if order not in ('bgr', 'rgb'):
        raise _lib.C2MError(f"order must be 'bgr' or 'rgb', got {order!r}")
    x, src = _image_src(t, "t")
    B, _, H, W = x.shape
    vh, vw = _valid_hw(valid_hw, H, W)
    out = torch.empty((B, vh, vw, 3), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().c2m_val_metrics_f32(_stream(), ctypes.byref(src), None, B, H, W, vh, vw, 0, _image_order(order),
                                                  out.data_ptr(), None, None, None, 0), "c2m_val_metrics_f32")
    return out[0] if t.dim() == 3 else out


def val_metrics_sums(sr, gt, crop_border=4, valid_hw=None, images=None):
    """The kernel's own results: (sums float64 [B,3] = squared 8-bit difference, squared Y difference, SSIM_Y map, each
    summed over the border-cropped window; sr_u8, gt_u8 uint8 [B,vh,vw,3] or None; (h, w) of the cropped window)."""
    rgb = _image_order(images)
    s, s_src = _image_src(sr, "sr")
    g, g_src = _image_src(gt, "gt")
    if s.shape[0] != g.shape[0] or s.device != g.device or (valid_hw is None and s.shape != g.shape):
        raise _lib.C2MError(f"sr and gt must have one batch size and one device, and one shape unless valid_hw names their "
                            f"common window; got {tuple(s.shape)} and {tuple(g.shape)}")
    crop = int(crop_border)
    if crop < 0:
        raise _lib.C2MError("crop_border must be >= 0")
    B, H, W = s.shape[0], min(s.shape[2], g.shape[2]), min(s.shape[3], g.shape[3])   # (only one of the two may be padded)
    vh, vw = _valid_hw(valid_hw, H, W)
    L = _lib.lib()
    ws_bytes = int(L.c2m_val_metrics_workspace_bytes(B, vh, vw, crop))
    sums = torch.empty((B, 3), dtype=torch.float64, device=s.device)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=s.device)
    s8 = torch.empty((B, vh, vw, 3), dtype=torch.uint8, device=s.device) if images else None
    g8 = torch.empty((B, vh, vw, 3), dtype=torch.uint8, device=s.device) if images else None
    with torch.cuda.device(s.device):
        _lib.check(L.c2m_val_metrics_f32(_stream(), ctypes.byref(s_src), ctypes.byref(g_src), B, H, W, vh, vw, crop, rgb,
                                         s8.data_ptr() if images else None, g8.data_ptr() if images else None,
                                         sums.data_ptr(), ws.data_ptr(), ws_bytes), "c2m_val_metrics_f32")
    return sums, s8, g8, (vh - 2 * crop, vw - 2 * crop)


def _psnr_of_mse(mse):
    # the expression of mmsr.utils.metrics.psnr
    return torch.where(mse == 0, torch.full_like(mse, float('inf')), 20.0 * torch.log10(255.0 / torch.sqrt(mse)))


def val_metrics(sr, gt, crop_border=4, valid_hw=None, images=None):
    """PSNR, PSNR_Y and SSIM_Y of ``nondist_validation`` for a batch, in one pass over both tensors.

    sr, gt: fp32 RGB [B,3,H,W] on the GPU; any view with a unit innermost stride is read in place.  valid_hw: the
    un-padded (rows, columns) both are cropped to (default: everything); crop_border pixels are left out on every side of
    that window.  -> dict of float64 tensors [B] 'psnr', 'psnr_y', 'ssim_y' with the definitions of
    mmsr.utils.metrics.validation_metrics (inf where the mean squared error is 0).  images='bgr' / 'rgb' adds 'sr_u8' and
    'gt_u8', uint8 [B,vh,vw,3] of the whole valid window in that channel order.  Nothing here waits for the device.
    A cropped window with a side below 11 pixels (an empty SSIM map) raises C2MError."""
    sums, s8, g8, (h, w) = val_metrics_sums(sr, gt, crop_border, valid_hw, images)
    out = {'psnr': _psnr_of_mse(sums[:, 0] / (3 * h * w)), 'psnr_y': _psnr_of_mse(sums[:, 1] / (h * w)),
           'ssim_y': sums[:, 2] / ((h - 10) * (w - 10))}
    if images:
        out['sr_u8'], out['gt_u8'] = s8, g8
    return out


# ---- the WGAN-GP penalty on the critic's input gradient (csrc/gp_penalty.hip, include/c2m_gan_hip.h) -----------------------

class _GradientPenaltyFn(torch.autograd.Function):
    """G fp32 [N, ...] -> (mean_n (||G[n]||_2 - 1)^2 as a 0-d tensor, norms [N]).  G is the output of
    autograd.grad(create_graph=True), so the gradient this returns for it feeds the critic's double-backward graph; the
    backward itself is not differentiable again.  norms is not differentiable."""

    @staticmethod
    def forward(ctx, G):
        N, M = G.shape[0], G.numel() // G.shape[0]
        L = _lib.lib()
        nbytes = int(L.c2m_gp_penalty_workspace_bytes(N, M))
        if nbytes == 0:
            raise _lib.C2MError(f"c2m_gp_penalty_workspace_bytes: unsupported shape {tuple(G.shape)}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=G.device)
        norms = torch.empty(N, dtype=torch.float32, device=G.device)
        out = torch.empty((), dtype=torch.float32, device=G.device)
        with torch.cuda.device(G.device):
            _lib.check(L.c2m_gp_penalty_forward_f32(_stream(), G.data_ptr(), N, M, norms.data_ptr(), out.data_ptr(),
                                                    ws.data_ptr(), nbytes), "c2m_gp_penalty_forward_f32")
        ctx.save_for_backward(G, norms)
        ctx.mark_non_differentiable(norms)
        return out, norms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout, _g_norms):
        G, norms = ctx.saved_tensors
        N, M = G.shape[0], G.numel() // G.shape[0]
        gout = gout.to(torch.float32).contiguous()       # stays on the device: the kernel reads it there
        dG = torch.empty_like(G)
        with torch.cuda.device(G.device):
            _lib.check(_lib.lib().c2m_gp_penalty_backward_f32(_stream(), G.data_ptr(), norms.data_ptr(), gout.data_ptr(), N, M,
                                                              dG.data_ptr()), "c2m_gp_penalty_backward_f32")
        return dG


def gradient_penalty(grad, with_norms=False):
    """The WGAN-GP penalty ``((grad.flatten(1).norm(2, dim=1) - 1) ** 2).mean()`` of fp32 ``grad`` [N, ...] on the GPU, in two
    launches forward and one backward (no atomics: the same input gives the same bits on every call).  Differentiable once
    with respect to ``grad``; a sample whose gradient is all zero gets a zero gradient, as torch's norm gives it.
    -> the 0-d penalty, or (penalty, norms [N]) with with_norms."""
    g = _dev_f32(grad, "grad")
    if g.dim() < 2 or g.numel() == 0:
        raise _lib.C2MError(f"grad must be a non-empty [N, ...] tensor with at least two dimensions, got {tuple(g.shape)}")
    out, norms = _GradientPenaltyFn.apply(g)
    return (out, norms) if with_norms else out

"""Tensor-level wrappers over the C ABI (include/magicdec_hip.h).

These are the seven ``mylib::*`` operators of the reference (Engine/utils.py:31-66,
Engine/SnapKV/backend.py:56-107, Engine/SnapKV/model.py:133-156) plus the fused
small ops of the decode loop, with the same tensor-level signatures, backed by
hand-written gfx950 kernels.  Differences from the reference's op boundary:

* no hidden ``plan()`` state: the page table is passed to the attention op
  explicitly and read on the device (no host sync, graph-capturable);
* tensors must live on the GPU; there is no CPU implementation here
  (``MagicDecHipError`` if the library is missing, ``ValueError`` for CPU tensors).

The C side sees raw pointers and a few integers, so this file checks device, dtype, shape and strides of every tensor
whose pointer it passes, through the contracts below (attribute reads only: free inside a hipGraph capture).  An operand
the kernels would mis-read raises before any launch: ``ValueError`` for shape, stride or device, ``TypeError`` for dtype.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._lib import MagicDecHipError, check  # noqa: F401

PAGE_SIZE = 128
MD_KV_BF16, MD_KV_FP8_E4M3 = 0, 1      # include/magicdec_hip.h
MD_KV_LAYOUT_HND = 0x100
FP8_DTYPE = torch.float8_e4m3fn
KV_LAYOUTS = ("NHD", "HND")
BF16, I32, I64 = torch.bfloat16, torch.int32, torch.int64


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------- operand contracts
class _DtypeError(TypeError, ValueError):
    """A wrong dtype.  New checks promise a TypeError for it, the older wrappers raised ValueError: this is both, so
    `except ValueError` around any wrapper of this file also catches every dtype error."""


def _gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("magicdec_amd.ops: tensors must be on the GPU (no CPU path exists)")


def _tensor(what, name, t, shape, dtype, optional=False):
    """`t` is a contiguous `dtype` tensor on the GPU of `shape` (a tuple; an int: that many elements; None: any)."""
    if t is None:
        if optional:
            return
        raise ValueError(f"{what}: {name} is missing")
    _gpu(t)
    if t.dtype != dtype:
        raise _DtypeError(f"{what}: {name} must be {dtype}, got {t.dtype}")
    fits = shape is None or (t.numel() == shape if isinstance(shape, int) else tuple(t.shape) == tuple(shape))
    if not fits or not t.is_contiguous():
        want = "" if shape is None else f" of {shape} elements" if isinstance(shape, int) else f" of shape {list(shape)}"
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} tensor{want}, got {tuple(t.shape)}")


def _mat(what, name, t, shape=None):
    """`t` is a 2-D bf16 tensor on the GPU with unit inner stride (row stride free), of `shape` if given -> (rows, cols)."""
    _gpu(t)
    msg = f"{what}: {name} must be bf16 {list(shape) if shape else '[rows, cols]'} with unit inner stride"
    if t.dtype != BF16:
        raise _DtypeError(f"{msg}, got {t.dtype}")
    if t.dim() != 2 or t.stride(1) != 1 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{msg}, got {tuple(t.shape)} strides {t.stride()}")
    return t.shape


def _out(what, out, M, N, like):
    """The [M, N] result of a linear: allocated, or the caller's `out` validated."""
    if out is None:
        return torch.empty((M, N), dtype=like.dtype, device=like.device)
    _mat(what, "out", out, (M, N))
    return out


def _add_norm_io(what, resid, norm_weight, M, N, like):
    """The residual [M, N] and norm weight [N] of an *_add_rmsnorm form -> freshly allocated (h, y)."""
    _mat(what, "resid", resid, (M, N))
    _tensor(what, "norm_weight", norm_weight, N, BF16)
    return (torch.empty((M, N), dtype=like.dtype, device=like.device),
            torch.empty((M, N), dtype=like.dtype, device=like.device))


def _i32(what, **table):
    """Page-table tensors (indices, indptr, last_page_len, the append / query indptr, offsets): int32 on the GPU."""
    for name, t in table.items():
        _tensor(what, name, t, None, I32)


def _heads(what, name, t, rows=None, heads=None, D=None):
    """`t` is a bf16 [rows, heads, D] tensor on the GPU whose last two dims are dense (row stride free), of the sizes
    that are given -> its row stride in elements."""
    _gpu(t)
    if t.dtype != BF16:
        raise _DtypeError(f"{what}: {name} must be bf16, got {t.dtype}")
    if (t.dim() != 3 or t.stride(2) != 1 or t.stride(1) != t.shape[2]
            or any(want is not None and want != got for want, got in zip((rows, heads, D), t.shape))):
        raise ValueError(f"{what}: {name} must be [{rows or 'rows'}, {heads or 'heads'}, {D or 'D'}] with dense "
                         f"(heads, D), got {tuple(t.shape)} strides {t.stride()}")
    return t.stride(0)


def _kv_geom(kv_cache, kv_layout):
    """(page_size, KH, D) of a paged cache [pages, 2, page_size, KH, D] ("NHD", the reference's layout:
    Engine/SnapKV/backend.py:30) or [pages, 2, KH, page_size, D] ("HND", rows of a kv head contiguous)."""
    if kv_layout not in KV_LAYOUTS:
        raise ValueError(f"kv_layout must be one of {KV_LAYOUTS}, got {kv_layout!r}")
    if kv_cache.dim() != 5 or kv_cache.shape[1] != 2 or not kv_cache.is_contiguous():
        raise ValueError("paged KV cache must be a contiguous [pages, 2, ., ., D] tensor")
    if kv_layout == "HND":
        return kv_cache.shape[3], kv_cache.shape[2], kv_cache.shape[4]
    return kv_cache.shape[2], kv_cache.shape[3], kv_cache.shape[4]


def _kv_args(kv_cache, kv_scales, kv_layout="NHD"):
    """(kv_dtype | layout flag, k_scale ptr, v_scale ptr) for a paged cache: bf16 caches take no scales, e4m3fn
    caches need per-kv-head float32 dequantisation scales `(k_scale[KH], v_scale[KH])`."""
    flag = MD_KV_LAYOUT_HND if kv_layout == "HND" else 0
    if kv_cache.dtype == BF16:
        return MD_KV_BF16 | flag, None, None
    if kv_cache.dtype != FP8_DTYPE:
        raise TypeError(f"paged KV cache must be bfloat16 or float8_e4m3fn, got {kv_cache.dtype}")
    if kv_scales is None:
        raise ValueError("an fp8 KV cache needs kv_scales=(k_scale, v_scale)")
    ks, vs = kv_scales
    for t in (ks, vs):
        _tensor("fp8 KV cache", "a kv scale", t, _kv_geom(kv_cache, kv_layout)[1], torch.float32)
    return MD_KV_FP8_E4M3 | flag, _p(ks), _p(vs)


def _second_cache(what, kv_cache, kv_layout, kv_cache2, **table2):
    """The optional second cache of an append (self-spec verify): bf16 NHD pages of the first cache's geometry, with a
    whole page table of its own."""
    if kv_cache2 is None:
        return
    _gpu(kv_cache2)
    if kv_cache2.dtype != BF16:
        raise TypeError(f"{what}: the second cache must be bfloat16, got {kv_cache2.dtype}")
    if _kv_geom(kv_cache2, "NHD") != _kv_geom(kv_cache, kv_layout):
        raise ValueError(f"{what}: the second cache must be NHD pages with the first cache's (page_size, KH, D)")
    _i32(what, **table2)


# ----------------------------------------------------------------------------- K4
def update_kv(k, v, kv_append_indptr, kv_cache, kv_page_indices, kv_page_indptr, kv_page_lastlen, n_max=None,
              kv_scales=None, kv_layout="NHD"):
    """mylib::update_kv (Engine/utils.py:31-54).  In place on kv_cache."""
    _gpu(kv_cache)
    _i32("update_kv", kv_append_indptr=kv_append_indptr, kv_page_indices=kv_page_indices,
         kv_page_indptr=kv_page_indptr, kv_page_lastlen=kv_page_lastlen)
    B = kv_page_indptr.numel() - 1
    page_size, KH, D = _kv_geom(kv_cache, kv_layout)
    k_stride, v_stride = _heads("update_kv", "k", k, None, KH, D), _heads("update_kv", "v", v, k.shape[0], KH, D)
    if n_max is None:
        n_max = max((k.shape[0] + B - 1) // B if B > 0 else 0, 1)
    lib = _lib.load()
    check(lib.md_append_paged_kv(_p(k), _p(v), k_stride, v_stride, _p(kv_append_indptr),
                                 _p(kv_cache), _p(kv_page_indices), _p(kv_page_indptr),
                                 _p(kv_page_lastlen), B, n_max, KH, D, page_size,
                                 *_kv_args(kv_cache, kv_scales, kv_layout), _stream()),
          "md_append_paged_kv")


def page_overflow_count(reset=True):
    """KV rows dropped by the append kernels because their request's last page was full (see
    md_page_overflow_count).  Synchronises with the device: call it per batch, not per step."""
    n = ctypes.c_uint(0)
    check(_lib.load().md_page_overflow_count(ctypes.byref(n), 1 if reset else 0), "md_page_overflow_count")
    return int(n.value)


# ----------------------------------------------------------------------------- K5
class RopeTable:
    """Host-precomputed cos/sin table on the device (float32 [max_pos, D/2, 2])."""

    def __init__(self, max_pos, head_dim, rope_theta, rope_scale, low_freq_factor=None, high_freq_factor=None,
                 old_context_len=None, device="cuda"):
        lib = _lib.load()
        host = torch.empty(max_pos, head_dim // 2, 2, dtype=torch.float32)
        llama31 = low_freq_factor is not None and high_freq_factor is not None
        check(lib.md_rope_fill_table_host(ctypes.c_void_p(host.data_ptr()), max_pos, head_dim, float(rope_theta),
                                          float(rope_scale), float(low_freq_factor) if llama31 else 0.0,
                                          float(high_freq_factor) if llama31 else 0.0,
                                          float(old_context_len) if llama31 else 0.0),
              "md_rope_fill_table_host")
        self.table = host.to(device)
        self.max_pos = max_pos
        self.head_dim = head_dim


def rope(q, k, indptr, offsets, table: RopeTable, n_max=None):
    """mylib::rope / mylib::draft_rope (Engine/SnapKV/model.py:133-156): returns new (q, k)."""
    _gpu(table.table)
    _i32("rope", indptr=indptr, offsets=offsets)
    B = indptr.numel() - 1
    q_stride = _heads("rope", "q", q, None, None, table.head_dim)
    H, D = q.shape[1], q.shape[2]
    k_stride, KH = (_heads("rope", "k", k, q.shape[0], None, D), k.shape[1]) if k is not None else (0, 0)
    if n_max is None:
        n_max = max((q.shape[0] + B - 1) // B, 1)
    q_out = torch.empty((q.shape[0], H, D), dtype=q.dtype, device=q.device)
    k_out = torch.empty((k.shape[0], KH, D), dtype=k.dtype, device=k.device) if k is not None else None
    lib = _lib.load()
    check(lib.md_rope(_p(q), _p(k), q_stride, k_stride, _p(q_out), _p(k_out),
                      _p(indptr), _p(offsets), B, n_max, H, KH, D, _p(table.table), table.max_pos,
                      _stream()), "md_rope")
    return q_out, k_out


def rope_append(q, k, v, indptr, offsets, table: RopeTable, kv_cache, page_indices, page_indptr, last_page_len,
                kv_cache2=None, page_indices2=None, page_indptr2=None, last_page_len2=None, n_max=None,
                kv_scales=None, kv_layout="NHD"):
    """Fused mylib::rope + mylib::update_kv (+ second cache for self-spec verify).  Returns rotated q.
    kv_cache may be fp8 (with kv_scales) and/or HND (kv_layout); kv_cache2 is always bf16 NHD."""
    _gpu(kv_cache, table.table)
    _i32("rope_append", indptr=indptr, offsets=offsets, page_indices=page_indices, page_indptr=page_indptr,
         last_page_len=last_page_len)
    _second_cache("rope_append", kv_cache, kv_layout, kv_cache2, page_indices2=page_indices2,
                  page_indptr2=page_indptr2, last_page_len2=last_page_len2)
    B = indptr.numel() - 1
    page_size, KH, D = _kv_geom(kv_cache, kv_layout)
    if D != table.head_dim:
        raise ValueError(f"rope_append: the table was built for D={table.head_dim}, the cache has D={D}")
    strides = [_heads("rope_append", name, t, q.shape[0], heads, D) for name, t, heads in (("q", q, None), ("k", k, KH),
                                                                                           ("v", v, KH))]
    H = q.shape[1]
    if n_max is None:
        n_max = max((q.shape[0] + B - 1) // B, 1)
    q_out = torch.empty((q.shape[0], H, D), dtype=q.dtype, device=q.device)
    lib = _lib.load()
    check(lib.md_rope_append(_p(q), _p(k), _p(v), *strides, _p(q_out),
                             _p(indptr), _p(offsets), B, n_max, H, KH, D, _p(table.table), table.max_pos,
                             _p(kv_cache), _p(page_indices), _p(page_indptr), _p(last_page_len),
                             _p(kv_cache2), _p(page_indices2), _p(page_indptr2), _p(last_page_len2),
                             page_size, *_kv_args(kv_cache, kv_scales, kv_layout), _stream()),
          "md_rope_append")
    return q_out


# ----------------------------------------------------------------------------- K1/K2/K3
class AttnWorkspace:
    """Scratch for split-KV partials, grown on demand (never inside a captured graph)."""

    def __init__(self, device="cuda"):
        self.device = device
        self.buf = torch.empty(1 << 20, dtype=torch.uint8, device=device)
        self._retired = []     # outgrown buffers stay allocated: captured hipGraphs have their addresses baked in

    def get(self, nbytes):
        if self.buf.numel() < nbytes:
            self._retired.append(self.buf)
            self.buf = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=self.device)
        return self.buf

    def carve(self, nbytes, slack=256):
        """A 256-byte aligned view of `nbytes` of the scratch (`slack`: the room asked for on top, for the alignment)."""
        ws = self.get(nbytes + slack)
        off = (-ws.data_ptr()) % 256
        return ws[off:off + nbytes]


def _carve(what, workspace, nbytes):
    """(pointer, nbytes) of the aligned scratch of a linear that splits K; (None, 0) when it needs none."""
    if not nbytes:
        return None, 0
    if workspace is None:
        raise ValueError(f"{what}: this shape splits K and needs a workspace")
    return _p(workspace.carve(nbytes)), nbytes


def paged_attention(q, kv_cache, qo_indptr, page_indices, page_indptr, last_page_len, n_max, max_pages_per_req,
                    workspace: AttnWorkspace, causal=True, sm_scale=None, out=None, kv_scales=None,
                    kv_layout="NHD"):
    """mylib::target_decode / target_prefill / draft_decode / draft_prefill
    (Engine/SnapKV/backend.py:56-107): flashinfer BatchPrefillWithPagedKVCacheWrapper.run with the
    plan() arguments passed explicitly."""
    _gpu(kv_cache)
    _i32("paged_attention", qo_indptr=qo_indptr, page_indices=page_indices, page_indptr=page_indptr,
         last_page_len=last_page_len)
    B = page_indptr.numel() - 1
    page_size, KH, D = _kv_geom(kv_cache, kv_layout)
    q_stride = _heads("paged_attention", "q", q, None, None, D)
    H = q.shape[1]
    if H % KH:
        raise ValueError(f"paged_attention: {H} query heads do not group over {KH} kv heads")
    if sm_scale is None:
        sm_scale = 1.0 / math.sqrt(D)
    if out is None:
        out = torch.empty((q.shape[0], H, D), dtype=q.dtype, device=q.device)
    else:
        _tensor("paged_attention", "out", out, (q.shape[0], H, D), q.dtype)
    lib = _lib.load()
    nbytes = lib.md_paged_attn_workspace_bytes(B, n_max, H, KH, D, max_pages_per_req, page_size)
    ws = workspace.get(nbytes)
    check(lib.md_paged_attn(_p(q), q_stride, _p(kv_cache), _p(out), _p(qo_indptr), _p(page_indices),
                            _p(page_indptr), _p(last_page_len), B, n_max, H, KH, D, page_size,
                            1 if causal else 0, float(sm_scale), max_pages_per_req,
                            *_kv_args(kv_cache, kv_scales, kv_layout),
                            _p(ws), ws.numel(), _stream()),
          "md_paged_attn")
    return out


# ----------------------------------------------------------------------------- K6
def snapkv_select(q_win, kv_cache, page_indices, page_indptr, ctx_len, window, budget, pool_kernel, draft_cache,
                  draft_page_indices, draft_page_indptr, draft_last_page_len, workspace: AttnWorkspace,
                  return_scores=False, kv_scales=None, kv_layout="NHD"):
    """Attention.gen_draft_kv (Engine/SnapKV/model.py:389-439): writes budget rows per request and kv head
    into draft_cache; returns the selected positions [B, KH, budget-window] int32 (reference order).
    kv_layout describes kv_cache (the source); draft_cache is always bf16 NHD."""
    _gpu(q_win, kv_cache)
    _i32("snapkv_select", page_indices=page_indices, page_indptr=page_indptr)
    _second_cache("snapkv_select", kv_cache, kv_layout, draft_cache, draft_page_indices=draft_page_indices,
                  draft_page_indptr=draft_page_indptr, draft_last_page_len=draft_last_page_len)
    B = page_indptr.numel() - 1
    page_size, KH, D = _kv_geom(kv_cache, kv_layout)
    if not q_win.is_contiguous():
        q_win = q_win.contiguous()
    _heads("snapkv_select", "q_win", q_win, None, None, D)
    H = q_win.shape[1]
    idx = torch.empty((B, KH, budget - window), dtype=torch.int32, device=q_win.device)
    lib = _lib.load()
    nbytes = lib.md_snapkv_workspace_bytes(B, H, KH, ctx_len, window)
    if nbytes == 0:
        raise ValueError("md_snapkv_workspace_bytes: bad shape")
    ws = workspace.carve(nbytes, slack=512)
    check(lib.md_snapkv_select(_p(q_win), _p(kv_cache), _p(page_indices), _p(page_indptr), B, H, KH, D,
                               page_size, ctx_len, window, budget, pool_kernel, _p(draft_cache),
                               _p(draft_page_indices), _p(draft_page_indptr), _p(draft_last_page_len),
                               _p(idx), *_kv_args(kv_cache, kv_scales, kv_layout), _p(ws), nbytes, _stream()),
          "md_snapkv_select")
    if return_scores:
        soff = lib.md_snapkv_scores_offset(B, H, KH, ctx_len, window)
        n = B * KH * (ctx_len - window)
        sc = ws[soff: soff + 2 * n].view(torch.bfloat16).view(B, KH, ctx_len - window).clone()
        return idx, sc
    return idx


# ----------------------------------------------------------------------------- K7
def _stream_cache(what, kv_cache):
    """The StreamingLLM draft cache: bf16 NHD pages -> (page_size, KH, D)."""
    _gpu(kv_cache)
    if kv_cache.dtype != BF16:
        raise TypeError(f"{what}: the cache must be bfloat16, got {kv_cache.dtype}")
    return _kv_geom(kv_cache, "NHD")


def streaming_shift_append(k_new, v_new, kv_cache, n_new, kv_len, sink, pages_per_req):
    """In-place equivalent of KVCache.prefill's eviction branch (Engine/StreamingLLM/model_draft.py:122-134)."""
    page_size, KH, D = _stream_cache("streaming_shift_append", kv_cache)
    k_stride = _heads("streaming_shift_append", "k_new", k_new, None, KH, D)
    v_stride = _heads("streaming_shift_append", "v_new", v_new, k_new.shape[0], KH, D)
    if n_new < 1 or k_new.shape[0] % n_new:
        raise ValueError(f"streaming_shift_append: {k_new.shape[0]} rows of k_new are not B x n_new = {n_new}")
    B = k_new.shape[0] // n_new
    lib = _lib.load()
    check(lib.md_streaming_shift_append(_p(k_new), _p(v_new), k_stride, v_stride, _p(kv_cache), B,
                                        n_new, kv_len, sink, pages_per_req, KH, D, page_size, _stream()),
          "md_streaming_shift_append")


def streaming_rotate(kv_cache, rot_cache, B, valid_len, pages_per_req, table: RopeTable):
    """Rotated clone of the draft cache (Engine/StreamingLLM/model_draft.py:112-118,135-143): K rotated by
    slot position, V copied, rows [0, valid_len) of every request.  rot_cache may be kv_cache (in place)."""
    _gpu(table.table)
    page_size, KH, D = _stream_cache("streaming_rotate", kv_cache)
    _stream_cache("streaming_rotate", rot_cache)
    if rot_cache.shape != kv_cache.shape:
        raise ValueError("streaming_rotate: rot_cache must have the cache's shape")
    lib = _lib.load()
    check(lib.md_streaming_rotate(_p(kv_cache), _p(rot_cache), B, valid_len, pages_per_req, KH, D, page_size,
                                  _p(table.table), table.max_pos, _stream()), "md_streaming_rotate")


# ----------------------------------------------------------------------------- K8
MD_W_BF16, MD_W_INT8 = 0, 1
EPI_NONE, EPI_SWIGLU = 0, 1


def linear_supported(M, N, K, swiglu=False):
    """True when md_linear (the weight-streaming skinny GEMM) takes this shape; otherwise use a library GEMM."""
    return bool(_lib.load().md_linear_supported(int(M), int(N), int(K), EPI_SWIGLU if swiglu else EPI_NONE))


class PackedWeight:
    """A linear's weight in the streaming layout of md_linear (include/magicdec_hip.h: w_packed = 1):
    [ceil(N/32)][K/16][64 lanes][8] -- element (t, s, lane, e) = W[32t + lane%32][16s + 8*(lane/32) + e], rows past N
    zero; for swiglu=True tile t = rows 16t..16t+15 of w1 then rows 16t..16t+15 of w3 (weight = [w1; w3], N = 2I).
    Built once at load time (a torch permute: plumbing); bf16 or int8."""

    def __init__(self, weight, swiglu=False):
        N, K = weight.shape
        if K % 16:
            raise ValueError("PackedWeight needs K % 16 == 0")
        self.N, self.K, self.swiglu, self.dtype = N, K, swiglu, weight.dtype
        if swiglu:
            inter = N // 2
            t = (inter + 15) // 16
            w1 = torch.zeros((t * 16, K), dtype=weight.dtype, device=weight.device)
            w3 = torch.zeros((t * 16, K), dtype=weight.dtype, device=weight.device)
            w1[:inter], w3[:inter] = weight[:inter], weight[inter:]
            rows = torch.cat([w1.view(t, 16, K), w3.view(t, 16, K)], dim=1)          # [t, 32, K]
        else:
            t = (N + 31) // 32
            rows = torch.zeros((t * 32, K), dtype=weight.dtype, device=weight.device)
            rows[:N] = weight
            rows = rows.view(t, 32, K)
        # [t, j, s, kh, e] -> [t, s, kh, j, e]
        self.data = rows.view(t, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()

    def unpack(self):
        """The row-major [N, K] tensor this copy was built from (the inverse permute: plumbing).  Used to re-materialise
        a row-major weight that was released after prefill (Transformer.release_rowmajor): the streaming layout is then
        the ONE resident copy of the weight."""
        t, K = self.data.shape[0], self.K
        rows = self.data.permute(0, 3, 1, 2, 4).reshape(t, 32, K)      # [t, s, kh, j, e] -> [t, j, (s, kh, e)]
        if not self.swiglu:
            return rows.view(t * 32, K)[:self.N] if t * 32 != self.N else rows.view(t * 32, K)
        inter = self.N // 2
        out = torch.empty((self.N, K), dtype=self.data.dtype, device=self.data.device)
        out[:inter].copy_(rows[:, :16].reshape(t * 16, K)[:inter])
        out[inter:].copy_(rows[:, 16:].reshape(t * 16, K)[:inter])
        return out


def _weight(what, weight, K, swiglu=False, scales=None, int8=False, rowmajor=False):
    """A linear's weight for rows of K columns: a PackedWeight packed for this epilogue or (rowmajor) a contiguous [N, K]
    tensor, bf16 or (int8) int8 with bf16 per-row scales [N] -> (tensor, packed flag, N, dtype code)."""
    packed = isinstance(weight, PackedWeight)
    if packed:
        if weight.swiglu != swiglu:
            raise ValueError(f"{what}: the PackedWeight was packed for a different epilogue")
        wt, N, wk = weight.data, weight.N, weight.K
    elif not rowmajor:
        raise TypeError(f"{what} streams a bf16 PackedWeight")
    else:
        if weight.dim() != 2 or not weight.is_contiguous():
            raise ValueError(f"{what} expects a contiguous weight [N, K]")
        wt, (N, wk) = weight, weight.shape
    _gpu(wt)
    if wk != K:
        raise ValueError(f"{what}: x has K={K}, weight has K={wk}")
    if wt.dtype != BF16 and not (int8 and wt.dtype == torch.int8):
        raise _DtypeError(f"{what}: weight dtype {wt.dtype} unsupported ({'bf16 or int8' if int8 else 'bf16'})")
    if wt.dtype == torch.int8 and scales is None:
        raise ValueError("int8 weights need per-row scales")
    _tensor(what, "scales", scales, N, BF16, optional=True)
    return wt, packed, N, MD_W_INT8 if wt.dtype == torch.int8 else MD_W_BF16


class DeferredNorm:
    """An RMSNorm that has NOT been applied yet: `h` [M, K] are the un-normalised hidden states and `ssq` [M, K/32]
    the per-row partial sums of squares the residual epilogue of the producing linear wrote; the consuming fused
    linear normalises on the fly (md_linear_fused, deferred RMSNorm).  `materialize()` is the stand-alone kernel."""

    def __init__(self, h, ssq, weight, eps):
        self.h, self.ssq, self.weight, self.eps = h, ssq, weight, float(eps)

    def materialize(self):
        return rmsnorm(self.h, self.weight, self.eps)


def _pro(x, pro: DeferredNorm):
    """A deferred norm handed to the linear that consumes x [M, K]: x is pro.h, ssq [M, K / 32] float32 holds one partial
    per 32-column tile of the producer (a shorter one would give a silently wrong rstd), the norm weight is bf16 [K]."""
    M, K = x.shape
    if pro.h.data_ptr() != x.data_ptr():
        raise ValueError("deferred norm: x must be the un-normalised h the partial sums belong to")
    if K % 32:
        raise ValueError(f"deferred norm: K={K} is not a whole number of 32-column tiles")
    _tensor("deferred norm", "ssq", pro.ssq, (M, K // 32), torch.float32)
    _tensor("deferred norm", "the norm weight", pro.weight, K, BF16)


def linear(x, weight, bias=None, scales=None, swiglu=False, workspace: "AttnWorkspace" = None, out=None,
           pro: "DeferredNorm" = None):
    """F.linear(x, weight, bias) for M = x.shape[0] <= 256 rows on the hand-written gfx950 skinny GEMM (md_linear).
    x [M, K] bf16 with unit inner stride (row stride free); weight: a contiguous [N, K] tensor or a PackedWeight
    (streaming layout), bf16 -- or int8 with bf16 per-row `scales` (WeightOnlyInt8Linear semantics:
    bf16(x.w^T) * scales).  swiglu=True: weight = [w1; w3] (N = 2*I rows) and the result is
    silu(x.w1^T) * (x.w3^T) [M, I] with the reference's bf16 rounding points.
    pro (bf16 weights): x is pro.h, the un-normalised hidden state, and is normalised on the fly (md_linear_normed)."""
    M, K = _mat("linear", "x", x)
    wt, packed, N, wd = _weight("linear", weight, K, swiglu, scales, int8=pro is None, rowmajor=True)
    _tensor("linear", "bias", bias, N, BF16, optional=True)
    epi = EPI_SWIGLU if swiglu else EPI_NONE
    out = _out("linear", out, M, N // 2 if swiglu else N, x)
    lib = _lib.load()
    wsp, nbytes = _carve("linear", workspace, lib.md_linear_workspace_bytes(M, N, K, epi))
    if pro is not None:
        _pro(x, pro)
        check(lib.md_linear_normed(_p(x), x.stride(0), _p(pro.ssq), pro.ssq.shape[1], _p(pro.weight), pro.eps, _p(wt),
                                   1 if packed else 0, _p(bias), _p(out), out.stride(0), M, N, K, epi, wsp, nbytes,
                                   _stream()),
              "md_linear_normed")
        return out
    check(lib.md_linear(_p(x), x.stride(0), _p(wt), wd, 1 if packed else 0, _p(scales), _p(bias), _p(out),
                        out.stride(0), M, N, K, epi, wsp, nbytes, _stream()),
          "md_linear")
    return out


def linear_add_rmsnorm_supported(M, N, K):
    """True when md_linear_add_rmsnorm takes this shape (an md_linear shape whose K is split, N <= 8192)."""
    return bool(_lib.load().md_linear_add_rmsnorm_supported(int(M), int(N), int(K)))


def linear_add_rmsnorm(x, weight, resid, norm_weight, eps, bias=None, scales=None, workspace: "AttnWorkspace" = None):
    """(h, y) = (resid + F.linear(x, W, bias), rmsnorm(h) * norm_weight) on md_linear with the residual add and the norm
    fused into its split-K combine launch -- bit-identical to linear() followed by add_rmsnorm()."""
    M, K = _mat("linear_add_rmsnorm", "x", x)
    wt, packed, N, wd = _weight("linear_add_rmsnorm", weight, K, False, scales, int8=True, rowmajor=True)
    _tensor("linear_add_rmsnorm", "bias", bias, N, BF16, optional=True)
    lib = _lib.load()
    nbytes = lib.md_linear_workspace_bytes(M, N, K, EPI_NONE)
    if workspace is None or not nbytes:
        raise ValueError("linear_add_rmsnorm: needs a workspace and a shape whose K is split")
    wsp, nbytes = _carve("linear_add_rmsnorm", workspace, nbytes)
    h, y = _add_norm_io("linear_add_rmsnorm", resid, norm_weight, M, N, x)
    check(lib.md_linear_add_rmsnorm(_p(x), x.stride(0), _p(wt), wd, 1 if packed else 0, _p(scales), _p(bias), _p(resid),
                                    resid.stride(0), _p(norm_weight), float(eps), _p(h), _p(y), M, N, K,
                                    wsp, nbytes, _stream()), "md_linear_add_rmsnorm")
    return h, y


# ----------------------------------------------------------------------------- K8b, K split over workgroups
def fused_split_supported(M, N, K):
    """md_linear_fused_split takes this shape (M <= 256, K % 128 == 0, N % 32 == 0)."""
    return 1 <= M <= 256 and K >= 128 and K % 128 == 0 and N >= 32 and N % 32 == 0


def _split_args(what, x, weight, bias, workspace):
    """Operands of the split tile kernel -> (M, N, K, workspace pointer, nbytes)."""
    M, K = _mat(what, "x", x)
    N = _weight(what, weight, K)[2]
    _tensor(what, "bias", bias, N, BF16, optional=True)
    nbytes = _lib.load().md_linear_fused_split_workspace_bytes(M, N, K)
    if not nbytes or workspace is None:
        raise ValueError(f"{what}: needs a workspace and a supported shape")
    return (M, N, K, *_carve(what, workspace, nbytes))


def fused_split_linear(x, weight: "PackedWeight", bias=None, workspace: "AttnWorkspace" = None):
    """F.linear(x, W, bias) on the tile kernel with K also split over workgroups + the fixed-order combine launch
    (md_linear_fused_split; csrc/tilegemm.hip)."""
    M, N, K, wsp, nbytes = _split_args("fused_split_linear", x, weight, bias, workspace)
    out = _out("fused_split_linear", None, M, N, x)
    check(_lib.load().md_linear_fused_split(_p(x), x.stride(0), _p(weight.data), _p(bias), _p(out), out.stride(0), M, N,
                                            K, wsp, nbytes, _stream()), "md_linear_fused_split")
    return out


def fused_split_linear_add_rmsnorm(x, weight: "PackedWeight", resid, norm_weight, eps, bias=None,
                                   workspace: "AttnWorkspace" = None):
    """(h, y) = (resid + F.linear(x, W, bias), rmsnorm(h) * norm_weight): the split tile kernel + ONE combine launch that
    adds the slices in order, the residual, and normalises (md_linear_fused_split_add_rmsnorm) -- bit-identical to
    fused_split_linear() followed by add_rmsnorm()."""
    M, N, K, wsp, nbytes = _split_args("fused_split_linear_add_rmsnorm", x, weight, bias, workspace)
    h, y = _add_norm_io("fused_split_linear_add_rmsnorm", resid, norm_weight, M, N, x)
    check(_lib.load().md_linear_fused_split_add_rmsnorm(_p(x), x.stride(0), _p(weight.data), _p(bias), _p(resid),
                                                        resid.stride(0), _p(norm_weight), float(eps), _p(h), _p(y), M, N,
                                                        K, wsp, nbytes, _stream()),
          "md_linear_fused_split_add_rmsnorm")
    return h, y


# ----------------------------------------------------------------------------- K8c
def linear_block_supported(M, N, K, swiglu=False):
    """True when md_linear_block (csrc/blockgemm.hip: the block-tile GEMM of the 129..256-row verify linears) takes
    this shape (M <= 256, N % 128 == 0, K % 64 == 0)."""
    return bool(_lib.load().md_linear_block_supported(int(M), int(N), int(K), EPI_SWIGLU if swiglu else EPI_NONE))


def _block_args(x, weight, bias, swiglu, force_split, workspace):
    """Operands of the block-tile GEMM -> (M, N, K, workspace pointer, nbytes).  md_linear_block reads the bias as
    16-byte vectors of N bf16 values."""
    M, K = _mat("linear_block", "x", x)
    N = _weight("linear_block", weight, K, swiglu)[2]
    _tensor("linear_block", "bias", bias, N, BF16, optional=True)
    if bias is not None and bias.data_ptr() % 16:
        raise ValueError(f"linear_block: bias must be a contiguous, 16-byte aligned bf16 vector of {N} elements")
    nbytes = _lib.load().md_linear_block_workspace_bytes(M, N, K, 1 if force_split else 0)
    return (M, N, K, *_carve("linear_block", workspace, nbytes))


def linear_block(x, weight: "PackedWeight", bias=None, swiglu=False, workspace: "AttnWorkspace" = None, out=None):
    """F.linear(x, W, bias) (or silu(x.w1^T) * (x.w3^T) for swiglu=True, weight = [w1; w3]) for 129..256 rows on the
    block-tile GEMM md_linear_block; same contract and rounding points as linear()."""
    M, N, K, wsp, nbytes = _block_args(x, weight, bias, swiglu, False, workspace)
    out = _out("linear_block", out, M, N // 2 if swiglu else N, x)
    check(_lib.load().md_linear_block(_p(x), x.stride(0), _p(weight.data), _p(bias), _p(out), out.stride(0), M, N, K,
                                      EPI_SWIGLU if swiglu else EPI_NONE, wsp, nbytes, _stream()), "md_linear_block")
    return out


def linear_block_add_rmsnorm(x, weight: "PackedWeight", resid, norm_weight, eps, bias=None,
                             workspace: "AttnWorkspace" = None):
    """(h, y) = (resid + F.linear(x, W, bias), rmsnorm(h) * norm_weight): md_linear_block with the residual add and the
    norm in its combine launch -- the combine kernel of linear_add_rmsnorm (same rounding points)."""
    M, N, K, wsp, nbytes = _block_args(x, weight, bias, False, True, workspace)
    h, y = _add_norm_io("linear_block_add_rmsnorm", resid, norm_weight, M, N, x)
    check(_lib.load().md_linear_block_add_rmsnorm(_p(x), x.stride(0), _p(weight.data), _p(bias), _p(resid),
                                                  resid.stride(0), _p(norm_weight), float(eps), _p(h), _p(y), M, N, K,
                                                  wsp, nbytes, _stream()),
          "md_linear_block_add_rmsnorm")
    return h, y


# ----------------------------------------------------------------------------- K8b
FL_NONE, FL_SWIGLU, FL_RESID, FL_ROPE_APPEND = 0, 1, 2, 3


def fused_linear_supported(M, N, K, epilogue=FL_NONE):
    """True when md_linear_fused (csrc/tilegemm.hip) takes this shape."""
    return bool(_lib.load().md_linear_fused_supported(int(M), int(N), int(K), int(epilogue)))


def _fused_args(x, weight: "PackedWeight", bias, epilogue, pro):
    """md_fused_linear_args with the product's operands (and the deferred norm of x, if any) filled in."""
    M, K = _mat("fused linear", "x", x)
    wt, _, N, _ = _weight("fused linear", weight, K, epilogue == FL_SWIGLU)
    _tensor("fused linear", "bias", bias, N, BF16, optional=True)
    a = _lib.FusedLinearArgs()
    a.x, a.ldx, a.w_packed, a.bias = x.data_ptr(), x.stride(0), wt.data_ptr(), (bias.data_ptr() if bias is not None else None)
    a.M, a.N, a.K, a.epilogue = M, N, K, epilogue
    if pro is not None:                      # x is the un-normalised h: normalise on the fly (deferred RMSNorm)
        _pro(x, pro)
        a.pro_ssq, a.pro_tiles = pro.ssq.data_ptr(), pro.ssq.shape[1]
        a.pro_norm_w, a.pro_eps = pro.weight.data_ptr(), pro.eps
    return a


def _run_fused(a):
    check(_lib.load().md_linear_fused(ctypes.byref(a), _stream()), "md_linear_fused")


def fused_linear(x, weight: "PackedWeight", bias=None, swiglu=False, resid=None, out=None, want_ssq=False,
                 pro: "DeferredNorm" = None):
    """One launch (md_linear_fused): F.linear(x, W, bias) for M <= 256 rows over a PackedWeight, optionally followed by
    SiLU(h1) * h3 (swiglu=True, weight = [w1; w3]) or by the bf16 residual add `resid + linear` (resid [M, N]).
    want_ssq (with resid): also return the per-row partial sums of squares [M, N/32] of the result (the producer half of
    a deferred RMSNorm).  pro (with swiglu): x is pro.h and is normalised on the fly (the consumer half)."""
    if pro is not None and not swiglu:
        raise ValueError("fused linear: the deferred-norm prologue exists for the w1|w3 and qkv linears")
    if want_ssq and resid is None:
        raise ValueError("fused linear: want_ssq belongs to the residual epilogue")
    a = _fused_args(x, weight, bias, FL_SWIGLU if swiglu else (FL_RESID if resid is not None else FL_NONE), pro)
    out = _out("fused linear", out, a.M, a.N // 2 if swiglu else a.N, x)
    a.out, a.ldo = out.data_ptr(), out.stride(0)
    ssq = None
    if resid is not None:
        _mat("fused linear", "resid", resid, out.shape)
        a.resid, a.ldr = resid.data_ptr(), resid.stride(0)
        if want_ssq:
            ssq = torch.empty((a.M, a.N // 32), dtype=torch.float32, device=x.device)
            a.ssq_out = ssq.data_ptr()
    _run_fused(a)
    return (out, ssq) if want_ssq else out


def fused_qkv_rope_append(x, weight: "PackedWeight", bias, H, KH, D, rows_per_req, offsets, table: RopeTable, kv_cache,
                          page_indices, page_indptr, last_page_len, kv_cache2=None, page_indices2=None,
                          page_indptr2=None, last_page_len2=None, kv_scales=None, kv_layout="NHD",
                          pro: "DeferredNorm" = None):
    """wqkv + RoPE + paged KV append in one launch (md_linear_fused, MD_FL_ROPE_APPEND): x [M, K] are the normalised
    hidden states of a decode / verify step in which request b owns rows [b * rows_per_req, (b+1) * rows_per_req).
    Returns the rotated q [M, H, D]; rotated k and v go to the paged cache (and to kv_cache2, bf16 NHD, when given).
    Same results as linear -> rope_append."""
    a = _fused_args(x, weight, bias, FL_ROPE_APPEND, pro)
    _gpu(kv_cache, table.table)
    _i32("fused qkv", offsets=offsets, page_indices=page_indices, page_indptr=page_indptr, last_page_len=last_page_len)
    _second_cache("fused qkv", kv_cache, kv_layout, kv_cache2, page_indices2=page_indices2,
                  page_indptr2=page_indptr2, last_page_len2=last_page_len2)
    M = a.M
    if a.N != (H + 2 * KH) * D:
        raise ValueError("fused qkv: weight rows must be (H + 2 KH) * D")
    page_size, *kh_d = _kv_geom(kv_cache, kv_layout)
    if kh_d != [KH, D] or table.head_dim != D:
        raise ValueError(f"fused qkv: KH={KH}, D={D} are not the cache's {kh_d} and the table's D={table.head_dim}")
    if M % rows_per_req:
        raise ValueError("fused qkv: every request must own rows_per_req rows")
    q_out = torch.empty((M, H, D), dtype=x.dtype, device=x.device)
    a.out, a.ldo = q_out.data_ptr(), H * D
    a.H, a.KH, a.D, a.rows_per_req, a.max_pos = H, KH, D, rows_per_req, table.max_pos
    a.offsets, a.cos_sin = offsets.data_ptr(), table.table.data_ptr()
    a.cache, a.page_indices, a.page_indptr, a.last_page_len = (kv_cache.data_ptr(), page_indices.data_ptr(),
                                                               page_indptr.data_ptr(), last_page_len.data_ptr())
    if kv_cache2 is not None:
        a.cache2, a.page_indices2, a.page_indptr2, a.last_page_len2 = (
            kv_cache2.data_ptr(), page_indices2.data_ptr(), page_indptr2.data_ptr(), last_page_len2.data_ptr())
    a.page_size = page_size
    a.kv_dtype, a.k_scale, a.v_scale = _kv_args(kv_cache, kv_scales, kv_layout)
    _run_fused(a)
    return q_out


# ----------------------------------------------------------------------------- K9
def _norm_rows(what, x):
    """x [..., dim] bf16 on the GPU as contiguous rows [rows, dim]."""
    _gpu(x)
    if x.dtype != BF16:
        raise _DtypeError(f"{what}: x and r must be bf16, got {x.dtype}")
    x2 = x.reshape(-1, x.shape[-1])
    return x2 if x2.is_contiguous() else x2.contiguous()


def rmsnorm(x, weight, eps):
    x2 = _norm_rows("rmsnorm", x)
    _tensor("rmsnorm", "weight", weight, x2.shape[1], BF16)
    y = torch.empty_like(x2)
    lib = _lib.load()
    check(lib.md_rmsnorm(_p(x2), _p(weight), _p(y), x2.shape[0], x2.shape[1], float(eps), _stream()), "md_rmsnorm")
    return y.view(x.shape)


def add_rmsnorm(x, r, weight, eps):
    """h = x + r ; y = rmsnorm(h).  Returns (h, y)."""
    x2, r2 = _norm_rows("add_rmsnorm", x), _norm_rows("add_rmsnorm", r)
    if r2.shape != x2.shape:
        raise ValueError(f"add_rmsnorm: x {tuple(x.shape)} and r {tuple(r.shape)} differ")
    _tensor("add_rmsnorm", "weight", weight, x2.shape[1], BF16)
    h = torch.empty_like(x2)
    y = torch.empty_like(x2)
    lib = _lib.load()
    check(lib.md_add_rmsnorm(_p(x2), _p(r2), _p(weight), _p(h), _p(y), x2.shape[0], x2.shape[1], float(eps), _stream()),
          "md_add_rmsnorm")
    return h.view(x.shape), y.view(x.shape)


def silu_mul(a, b):
    """bf16(silu(a)) * b for 2-D row-strided views (e.g. the two halves of a fused w1|w3 GEMM output)."""
    rows, dim = _mat("silu_mul", "a", a)
    _mat("silu_mul", "b", b, (rows, dim))
    y = torch.empty((rows, dim), dtype=a.dtype, device=a.device)
    lib = _lib.load()
    check(lib.md_silu_mul(_p(a), _p(b), a.stride(0), b.stride(0), _p(y), rows, dim, _stream()), "md_silu_mul")
    return y


# ----------------------------------------------------------------------------- K10
def argmax(logits, index_offset=0, return_values=False):
    """Row-wise argmax of bf16 logits [rows, vocab] (lowest index among equal maxima)."""
    rows, vocab = _mat("argmax", "logits", logits)
    idx = torch.empty(rows, dtype=torch.int64, device=logits.device)
    vals = torch.empty(rows, dtype=logits.dtype, device=logits.device) if return_values else None
    lib = _lib.load()
    check(lib.md_argmax(_p(logits), logits.stride(0), rows, vocab, int(index_offset), _p(vals), _p(idx), _stream()),
          "md_argmax")
    return (vals, idx) if return_values else idx


def argmax_tp_slots(logits, tp_rank, tp_world, index_offset=0):
    """(vals [rows, tp_world] bf16, idx [rows, tp_world] int64): the row-wise argmax of this rank's vocab shard in column
    tp_rank, zeros elsewhere -- the tensors the reference sum-all-reduces before its merge (Engine/SnapKV/model.py:178-184),
    written by the argmax launch itself."""
    rows, vocab = _mat("argmax_tp_slots", "logits", logits)
    if not 0 <= tp_rank < tp_world:
        raise ValueError(f"argmax_tp_slots: rank {tp_rank} is not one of {tp_world}")
    vals = torch.empty((rows, tp_world), dtype=logits.dtype, device=logits.device)
    idx = torch.empty((rows, tp_world), dtype=torch.int64, device=logits.device)
    check(_lib.load().md_argmax_tp_slots(_p(logits), logits.stride(0), rows, vocab, int(index_offset), int(tp_rank),
                                         int(tp_world), _p(vals), _p(idx), _stream()), "md_argmax_tp_slots")
    return vals, idx


def tp_argmax_merge(vals, idx):
    """vals [rows, tp] bf16, idx [rows, tp] int64 -> winning global index per row (lowest rank on ties).  Views are
    fine: the kernel reads dense [rows, tp] copies of them."""
    _gpu(vals, idx)
    if vals.dim() != 2 or vals.shape != idx.shape:
        raise ValueError("tp_argmax_merge: vals and idx must be [rows, tp] tensors of one shape")
    if vals.dtype != BF16 or idx.dtype != I64:
        raise TypeError(f"tp_argmax_merge: vals must be bf16 and idx int64, got {vals.dtype}, {idx.dtype}")
    rows, tp = vals.shape
    out = torch.empty(rows, dtype=torch.int64, device=vals.device)
    lib = _lib.load()
    dense_vals, dense_idx = vals.contiguous(), idx.contiguous()      # named: a copy lives until the launch is queued
    check(lib.md_tp_argmax_merge(_p(dense_vals), _p(dense_idx), rows, tp, _p(out), _stream()), "md_tp_argmax_merge")
    return out


# ----------------------------------------------------------------------------- a1
def accept_rollback(tokens_buffer, target_tokens, output, num_nodes, cachelens, last_page_len, draft_cachelens,
                    draft_last_page_len, gamma, draft_rollback, draft_cap, eot_1, eot_2, max_nodes, accept_nums,
                    bonus, double_buffer, cachelens_update, flags):
    """The verify-loop body (tests/SnapKV/longspec_benchmark.py:208-285) as one launch; all tensors are
    updated in place, `flags` = int32[2] (terminal, next_double)."""
    B = tokens_buffer.shape[0]
    for name, t, shape, dtype, optional in (
            ("tokens_buffer", tokens_buffer, (B, gamma + 1), I64, False),
            ("target_tokens", target_tokens, (B, gamma + 1), I64, False),
            ("output", output, (B, output.shape[-1]), I64, False), ("num_nodes", num_nodes, B, I64, False),
            ("cachelens", cachelens, B, I32, False), ("last_page_len", last_page_len, B, I32, False),
            ("draft_cachelens", draft_cachelens, B, I32, True),
            ("draft_last_page_len", draft_last_page_len, B, I32, True),
            ("accept_nums", accept_nums, B, I64, False), ("bonus", bonus, B, I64, False),
            ("double_buffer", double_buffer, (B, 2), I64, True),
            ("cachelens_update", cachelens_update, B, I64, True), ("flags", flags, 2, I32, False)):
        _tensor("accept_rollback", name, t, shape, dtype, optional)
    lib = _lib.load()
    check(lib.md_accept_rollback(_p(tokens_buffer), _p(target_tokens), _p(output), output.shape[1], _p(num_nodes),
                                 _p(cachelens), _p(last_page_len), _p(draft_cachelens), _p(draft_last_page_len), B,
                                 gamma, draft_rollback, draft_cap, int(eot_1), int(eot_2), int(max_nodes),
                                 _p(accept_nums), _p(bonus), _p(double_buffer), _p(cachelens_update), _p(flags),
                                 _stream()), "md_accept_rollback")


# ------------------------------------------------------------------ K11 sampling (include/magicdec_hip.h)
SAMPLE_PREFILL, SAMPLE_BASELINE, SAMPLE_DRAFT, SAMPLE_ACCEPT, SAMPLE_RESIDUAL, SAMPLE_BONUS = range(6)
ADVANCE_NONE, ADVANCE_STEP, ADVANCE_ITER = 0, 1, 2
STATS_WORDS = 2          # md_sample_stats = 16 bytes = two int64 words per row
HIST_BINS = 256
CAND_WORDS = 3           # md_spec_verify_shard: residual-or-bonus candidate, fallback candidate, jr


def _logits(what, logits, temperature=1.0, top_p=1.0, n=1, row_sel=None):
    """bf16 logits [R * n, vocab] with unit inner stride, of which one row per group of n is drawn (row row_sel[r] - 1,
    else the last), and the sampling parameters -> (R, vocab)."""
    rows, vocab = _mat(what, "logits", logits)
    if not (temperature > 0 and 0 < top_p <= 1):
        raise ValueError(f"sampling needs temperature > 0 and 0 < top_p <= 1, got {temperature}, {top_p}")
    if n < 1 or rows % n:
        raise ValueError(f"{what}: {rows} rows are not R x n = {n}")
    _tensor(what, "row_sel", row_sel, (rows // n,), I64, optional=True)
    return rows // n, vocab


def _counters(counters):
    _gpu(counters)
    if counters.dtype != I32 or counters.numel() < 4 or not counters.is_contiguous():
        raise ValueError("sampling: counters must be a contiguous int32 [4] tensor")


def _draft_ring(what, ring, ring_stats, B, width):
    """The ring a draft draw writes its row to: contiguous bf16 [B, gamma, width] with stats [B, gamma, 2] -> gamma
    (0: no ring)."""
    if (ring is None) != (ring_stats is None):
        raise ValueError(f"{what}: ring and ring_stats go together")
    if ring is None:
        return 0
    _gpu(ring)
    if (ring.dim() != 3 or ring.shape[0] != B or ring.shape[2] != width or not ring.is_contiguous()
            or ring.dtype != BF16):
        raise ValueError(f"{what}: the draft ring must be a contiguous bf16 [B={B}, gamma, {width}] tensor (draft and "
                         f"target vocabularies must be equal and sharded alike); got {tuple(ring.shape)}")
    gamma = ring.shape[1]
    if gamma < 1:               # an empty ring has a null data pointer: the library would take it for "no ring"
        raise ValueError(f"{what}: a draft ring needs gamma >= 1")
    _tensor(what, "ring_stats", ring_stats, (B, gamma, STATS_WORDS), I64)
    return gamma


def _tokens_buffer(what, tokens_buffer):
    """tokens_buffer [B, gamma+1] int64 (a view is fine) -> (B, gamma+1, contiguous tensor).  The caller keeps the third
    in a named local: a temporary copy must stay alive until the launch is queued."""
    _gpu(tokens_buffer)
    if tokens_buffer.dim() != 2 or tokens_buffer.shape[1] < 2 or tokens_buffer.dtype != I64:
        raise ValueError(f"{what}: tokens_buffer must be int64 [B, gamma+1]")
    return (*tokens_buffer.shape, tokens_buffer.contiguous())


def _tokens_out(what, out, B, n, device):
    """The [B, n] int64 tokens a draw or a verify returns: allocated, or the caller's `out` validated."""
    if out is None:
        return torch.empty((B, n), dtype=torch.int64, device=device)
    _tensor(what, "out", out, (B, n), I64)
    return out


def _verify_stats(what, target_stats, ring_stats, B, gamma):
    _tensor(what, "target_stats", target_stats, (B * (gamma + 1), STATS_WORDS), I64)
    _tensor(what, "ring_stats", ring_stats, (B, gamma, STATS_WORDS), I64)


def sample_rows(logits, n, temperature, top_p, seed, purpose, counters, advance, row_sel=None, ring=None,
                ring_stats=None, out=None):
    """Tempered top-p Gumbel-max draw of ONE row per request from logits [B*n, vocab] bf16 (row row_sel[b]-1 of the
    request, else its last row); returns tokens [B, n] int64 with the token in every column.  counters: int32 [4] on the
    device (iteration, draft step, ticket, -).  Draft mode (ring [B, gamma, vocab] bf16, ring_stats [B, gamma, 2] int64):
    the row and its stats also go to ring slot counters[1]."""
    B, vocab = _logits("sample_rows", logits, temperature, top_p, n, row_sel)
    _counters(counters)
    gamma = _draft_ring("sample_rows", ring, ring_stats, B, vocab)
    out = _tokens_out("sample_rows", out, B, n, logits.device)
    check(_lib.load().md_sample_rows(_p(logits), logits.stride(0), B, n, vocab, float(temperature), float(top_p),
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(purpose), _p(row_sel), _p(counters),
                                     int(advance), _p(ring), _p(ring_stats), gamma, _p(out), _stream()),
          "md_sample_rows")
    return out


def spec_verify_sample(logits, tokens_buffer, ring, ring_stats, target_stats, counters, temperature, top_p, seed,
                       out=None):
    """Speculative-sampling verify: target logits [B*(gamma+1), vocab] bf16, the draft ring / stats of this iteration and
    tokens_buffer [B, gamma+1] -> target_tokens [B, gamma+1] int64 in the encoding ops.accept_rollback consumes
    unchanged.  target_stats: [B*(gamma+1), 2] int64 workspace (holds the target rows' stats afterwards).  A draft
    token outside [0, vocab) is rejected at its position.  tokens_buffer may be a non-contiguous view (it is copied)."""
    rows, vocab = _logits("spec_verify_sample", logits, temperature, top_p)
    _counters(counters)
    B, G1, tb = _tokens_buffer("spec_verify_sample", tokens_buffer)
    _gpu(ring)
    if (rows != B * G1 or tuple(ring.shape) != (B, G1 - 1, vocab) or ring.dtype != BF16 or not ring.is_contiguous()):
        raise ValueError(f"spec_verify_sample: logits {tuple(logits.shape)}, ring {tuple(ring.shape)} and tokens_buffer "
                         f"{tuple(tokens_buffer.shape)} disagree (draft and target vocabularies must be equal)")
    _verify_stats("spec_verify_sample", target_stats, ring_stats, B, G1 - 1)
    out = _tokens_out("spec_verify_sample", out, B, G1, logits.device)
    check(_lib.load().md_spec_verify_sample(_p(logits), logits.stride(0), B, G1 - 1, vocab, float(temperature),
                                            float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(tb),
                                            _p(ring), _p(ring_stats), _p(target_stats), _p(counters), _p(out),
                                            _stream()), "md_spec_verify_sample")
    return out


# ---- the vocab-sharded phases (K11 "sharded"): local launches; the caller all-reduces red / hist / cand between them
def _shard_offset(what, v_loc, vocab_offset, vocab_total):
    if vocab_offset < 0 or vocab_total < 1 or vocab_offset + v_loc > vocab_total:
        raise ValueError(f"{what}: columns [{vocab_offset}, {vocab_offset} + {v_loc}) are not inside the vocabulary "
                         f"of {vocab_total}")


def _shard_ring(what, ring, B, gamma, v_loc, col_offset):
    """The ring a verify phase reads: [B, gamma, W] bf16 with unit inner stride and dense requests (a ring shard, or a
    column view of / an offset into a full ring) -> row stride."""
    _gpu(ring)
    if (ring.dim() != 3 or ring.dtype != BF16 or ring.shape[0] != B or ring.shape[1] != gamma
            or ring.stride(2) != 1 or ring.stride(0) != gamma * ring.stride(1)):
        raise ValueError(f"{what}: the ring must be bf16 [B={B}, gamma={gamma}, W] with unit inner stride and "
                         f"stride(0) = gamma * stride(1); got {tuple(ring.shape)} strides {ring.stride()}")
    if col_offset < 0 or col_offset + v_loc > ring.shape[2]:
        raise ValueError(f"{what}: ring columns [{col_offset}, {col_offset} + {v_loc}) exceed its width {ring.shape[2]} "
                         "(draft and target must shard the vocabulary alike)")
    return ring.stride(1)


def _shard_hists(what, R, top_p, hist_hi, hist_lo):
    _tensor(what, "hist_hi", hist_hi, (R, HIST_BINS), I64)
    if (hist_lo is not None) != (top_p < 1):
        raise ValueError(f"{what}: the low-byte histogram goes with top_p < 1, and only with it")
    _tensor(what, "hist_lo", hist_lo, (R, HIST_BINS), I64, optional=True)


def shard_max(logits, n, vocab_offset, vocab_total, red, row_sel=None, tokens_buffer=None, ring=None,
              ring_col_offset=0):
    """Phase A on this rank's columns logits [R*n, v_loc] bf16: red[:R] = key of the shard's max of each drawn row.
    With tokens_buffer [B, gamma+1] (verify; n = 1, R = B (gamma+1)) red [R + B gamma] also takes the probes of the
    draft tokens this rank owns (0 elsewhere).  The caller MAX-all-reduces red."""
    R, v_loc = _logits("shard_max", logits, n=n, row_sel=row_sel)
    _shard_offset("shard_max", v_loc, vocab_offset, vocab_total)
    B, gamma, tb, stride = 0, 0, None, 0
    if tokens_buffer is not None:
        B, G1, tb = _tokens_buffer("shard_max", tokens_buffer)
        gamma = G1 - 1
        if n != 1 or row_sel is not None or R != B * G1 or ring is None:
            raise ValueError(f"shard_max: a verify probe needs n = 1, no row_sel, a ring and logits of B (gamma+1) = "
                             f"{B * G1} rows; got {R}")
        stride = _shard_ring("shard_max", ring, B, gamma, v_loc, ring_col_offset)
    elif ring is not None:
        raise ValueError("shard_max: a ring without tokens_buffer")
    _tensor("shard_max", "red", red, (R + B * gamma,), I64)
    check(_lib.load().md_sample_shard_max(_p(logits), logits.stride(0), R, n, v_loc, _p(row_sel), _p(tb), _p(ring),
                                          stride, int(ring_col_offset), gamma, int(vocab_offset), int(vocab_total),
                                          _p(red), _stream()), "md_sample_shard_max")
    return red


def shard_hist(logits, n, temperature, top_p, red, hist_out, hist_hi=None, row_sel=None):
    """Phase B (hist_hi None) / C (hist_hi = the reduced phase-B tensor; top_p < 1): hist_out [R, 256] int64 masses of
    this rank's columns under the global max in the reduced `red`.  The caller SUM-all-reduces hist_out."""
    R, v_loc = _logits("shard_hist", logits, temperature, top_p, n, row_sel)
    _tensor("shard_hist", "red", red, None, I64)
    if red.dim() != 1 or red.numel() < R:
        raise ValueError(f"shard_hist: red must be a contiguous int64 tensor of at least {R} elements")
    _tensor("shard_hist", "hist_out", hist_out, (R, HIST_BINS), I64)
    if hist_hi is not None and top_p >= 1:
        raise ValueError("shard_hist: top_p = 1 has no low-byte phase")
    _tensor("shard_hist", "hist_hi", hist_hi, (R, HIST_BINS), I64, optional=True)
    check(_lib.load().md_sample_shard_hist(_p(logits), logits.stride(0), R, n, v_loc, _p(row_sel), float(temperature),
                                           float(top_p), _p(red), _p(hist_hi), _p(hist_out), _stream()),
          "md_sample_shard_hist")
    return hist_out


def shard_draw(logits, n, vocab_offset, vocab_total, temperature, top_p, seed, purpose, counters, red, hist_hi, hist_lo,
               cand, row_sel=None, ring=None, ring_stats=None):
    """Phase D of a draw: cand [B] int64 = this rank's Gumbel-max winner (global index) under the stats derived from
    the reduced red / hist_hi / hist_lo (hist_lo None iff top_p == 1).  Draft mode (ring [B, gamma, v_loc] bf16 = this
    rank's ring shard, ring_stats [B, gamma, 2]): the local columns and the stats go to slot counters[1].  The caller
    MAX-all-reduces cand; the counters are only read."""
    B, v_loc = _logits("shard_draw", logits, temperature, top_p, n, row_sel)
    _counters(counters)
    _shard_offset("shard_draw", v_loc, vocab_offset, vocab_total)
    gamma = _draft_ring("shard_draw", ring, ring_stats, B, v_loc)
    _tensor("shard_draw", "red", red, (B,), I64)
    _shard_hists("shard_draw", B, top_p, hist_hi, hist_lo)
    _tensor("shard_draw", "cand", cand, (B,), I64)
    check(_lib.load().md_sample_shard_draw(_p(logits), logits.stride(0), B, n, v_loc, int(vocab_offset),
                                           int(vocab_total), float(temperature), float(top_p),
                                           int(seed) & 0xFFFFFFFFFFFFFFFF, int(purpose), _p(row_sel), _p(counters),
                                           _p(red), _p(hist_hi), _p(hist_lo), _p(ring), _p(ring_stats), gamma, _p(cand),
                                           _stream()), "md_sample_shard_draw")
    return cand


def shard_finish(cand, n, counters, advance, out=None):
    """Phase E of a draw: the reduced cand [B] -> tokens [B, n] int64 (the token in every column); advances the counters."""
    _counters(counters)
    B = cand.numel()
    _tensor("shard_finish", "cand", cand, (B,), I64)
    out = _tokens_out("shard_finish", out, B, n, cand.device)
    check(_lib.load().md_sample_shard_finish(_p(cand), B, n, _p(counters), int(advance), _p(out), _stream()),
          "md_sample_shard_finish")
    return out


def spec_verify_shard(logits, tokens_buffer, vocab_offset, vocab_total, ring, ring_stats, red, hist_hi, hist_lo,
                      target_stats, counters, temperature, top_p, seed, cand, ring_col_offset=0):
    """Phase D of a verify on this rank's columns logits [B*(gamma+1), v_loc]: the target stats of every row (from the
    reduced red [B (gamma+1) + B gamma] / hist_hi / hist_lo) into target_stats, the accept walk from the probes, and
    cand [B, 3] int64 = (residual-or-bonus candidate, fallback candidate, jr).  ring: [B, gamma, W] -- this rank's ring
    shard, or a full ring with ring_col_offset = vocab_offset.  The caller MAX-all-reduces cand."""
    rows, v_loc = _logits("spec_verify_shard", logits, temperature, top_p)
    _counters(counters)
    B, G1, tb = _tokens_buffer("spec_verify_shard", tokens_buffer)
    if rows != B * G1:
        raise ValueError(f"spec_verify_shard: logits {tuple(logits.shape)} and tokens_buffer "
                         f"{tuple(tokens_buffer.shape)} disagree")
    _shard_offset("spec_verify_shard", v_loc, vocab_offset, vocab_total)
    stride = _shard_ring("spec_verify_shard", ring, B, G1 - 1, v_loc, ring_col_offset)
    _verify_stats("spec_verify_shard", target_stats, ring_stats, B, G1 - 1)
    _tensor("spec_verify_shard", "red", red, (rows + B * (G1 - 1),), I64)
    _shard_hists("spec_verify_shard", rows, top_p, hist_hi, hist_lo)
    _tensor("spec_verify_shard", "cand", cand, (B, CAND_WORDS), I64)
    check(_lib.load().md_spec_verify_shard(_p(logits), logits.stride(0), B, G1 - 1, v_loc, int(vocab_offset),
                                           int(vocab_total), float(temperature), float(top_p),
                                           int(seed) & 0xFFFFFFFFFFFFFFFF, _p(tb), _p(ring), stride,
                                           int(ring_col_offset), _p(ring_stats), _p(red), _p(hist_hi), _p(hist_lo),
                                           _p(target_stats), _p(counters), _p(cand), _stream()), "md_spec_verify_shard")
    return cand


def spec_verify_shard_finish(cand, tokens_buffer, counters, out=None):
    """Phase E of a verify: the reduced cand [B, 3] -> target_tokens [B, gamma+1] in the encoding of spec_verify_sample;
    advances the iteration counter."""
    _counters(counters)
    B, G1, tb = _tokens_buffer("spec_verify_shard_finish", tokens_buffer)
    _tensor("spec_verify_shard_finish", "cand", cand, (B, CAND_WORDS), I64)
    out = _tokens_out("spec_verify_shard_finish", out, B, G1, cand.device)
    check(_lib.load().md_spec_verify_shard_finish(_p(cand), _p(tb), B, G1 - 1, _p(counters), _p(out), _stream()),
          "md_spec_verify_shard_finish")
    return out


def philox_host(counters, key0, key1):
    """Philox4x32-10 of the library (host): counters uint32-valued [n, 4] -> [n, 4] words (numpy uint32 arrays)."""
    import numpy as np
    c = np.ascontiguousarray(counters, dtype=np.uint32).reshape(-1, 4)
    out = np.empty_like(c)
    check(_lib.load().md_philox4x32_10_host(c.ctypes.data, c.shape[0], int(key0) & 0xFFFFFFFF,
                                            int(key1) & 0xFFFFFFFF, out.ctypes.data), "md_philox4x32_10_host")
    return out

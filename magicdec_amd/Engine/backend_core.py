"""Host side of the four MagicDec back-ends (L4 of SURVEY.md section 1), MI355X-native.

Public surface = the reference's: classes `LMBackend` / `LMBackend_Draft` with
`load_model, setup_caches, compile, encode, inference, verify, speculate,
draft_encode, clear_kv` and the tensors the harness reads AND REBINDS between
calls (`cachelens, paged_kv_last_page_len, draft_cachelens,
draft_paged_kv_last_page_len`, tests/SnapKV/longspec_benchmark.py:228-256) --
every method therefore re-reads those attributes at call time.

What is different underneath:
  * no flashinfer wrappers and no plan(): the page table goes to the kernels as
    device pointers; nothing in a step reads device memory on the host;
  * request b owns pages [b*P, (b+1)*P) (as in the reference, backend.py:273) so the
    page-index vector is built once per chunk by one vectorised op, not B aranges;
  * the lm head runs only on the last prefill chunk (the reference computes and
    discards 128 x vocab logits per chunk);
  * `compile()` captures the decode step into a hipGraph (there is no Inductor).

How the file reads: `_PagedState` is one page table (its three attributes on the back-end, the form it resets to);
`_BackendBase` holds what the four back-ends share -- `_alloc_state` / `clear_kv`, the chunked `_paged_prefill`, and
`_step`, the body of every inference / verify / speculate: it alone advances lengths and hands Engine/graph.py the names
of the attributes the step reads.  The four classes keep their own `setup_caches` (the reference's attribute names
differ) and, around their `_step` call, whatever the reference does for that method only.
"""
from __future__ import annotations

import torch

from .model_core import PageTable

PAGE_SIZE = 128    # Engine/SnapKV/backend.py:31
CHUNK = 128        # Engine/SnapKV/backend.py:236


def default_kv_layout():
    """Page layout of the full-context cache when setup_caches() is not told one: "HND" (rows of one kv head contiguous
    inside a page: the verify step's stream is read in 128-row runs, 85 % instead of 82 % of the HBM peak in bf16, 81 %
    instead of 71 % in fp8 -- DESIGN.md section 3.1) unless MAGICDEC_KV_LAYOUT=NHD asks for the reference's flashinfer
    layout (Engine/SnapKV/backend.py:30).  The layout is internal to the Engine API (the harness never touches the
    cache tensors) and moves bytes, not arithmetic: every kernel's output is bit-identical between the two
    (tests/test_gpu_hnd.py), and the whole GPU suite is green under either default (profiles/r03_hnd_suite_summary.txt).
    The mylib::* operator boundary (magicdec_amd/mylib_ops.py) keeps the reference's NHD signature default."""
    import os
    v = os.environ.get("MAGICDEC_KV_LAYOUT", "HND").upper()
    if v not in ("NHD", "HND"):
        raise ValueError(f"MAGICDEC_KV_LAYOUT must be NHD or HND, got {v!r}")
    return v


def _pages_per_request(max_batch_size, max_seq_length, page_size=PAGE_SIZE):
    """Engine/SnapKV/backend.py:32-35."""
    n = max_batch_size * max_seq_length // page_size
    if n * page_size < max_batch_size * max_seq_length:
        n += max_batch_size
    return n, n // max_batch_size


class _PagedState:
    """One paged cache's bookkeeping under a name prefix ('' or 'draft_') on the owning back-end, and the form its table
    starts from (at construction and at every reset()): empty with `indptr_stride` entries of the index vector per
    request, or -- `full_table`, the SnapKV draft cache -- every page mapped from the start."""

    def __init__(self, owner, prefix, ppr, last_page_len_init=0, full_table=False, indptr_stride=1):
        self.o, self.p, self.ppr = owner, prefix, ppr
        self.last_page_len_init, self.full_table, self.indptr_stride = last_page_len_init, full_table, indptr_stride
        # the attributes a step that is passed table() reads (Engine/graph.py pins them)
        self.names = tuple(prefix + n for n in ("paged_kv_indices", "paged_kv_indptr", "paged_kv_last_page_len"))
        self.reset()

    def _get(self, name):
        return getattr(self.o, self.p + name)

    def _set(self, name, val):
        setattr(self.o, self.p + name, val)

    # `state.last_page_len += n` updates the owner's tensor in place, `state.last_page_len = t` rebinds the attribute
    last_page_len = property(lambda self: self._get("paged_kv_last_page_len"),
                             lambda self, val: self._set("paged_kv_last_page_len", val))

    def reset(self):
        o, B, dev = self.o, self.o.batch_size, self.o.device
        ppr = self.ppr
        self._set("num_pages_per_request", torch.zeros(B, dtype=torch.int32, device=dev))
        self.host_pages = 0
        if self.full_table:   # SnapKV draft cache: all pages mapped from the start (backend.py:87-90)
            self._set("paged_kv_indptr", torch.arange(B + 1, dtype=torch.int32, device=dev) * ppr)
            self._set("paged_kv_indices", torch.arange(B * ppr, dtype=torch.int32, device=dev))
            self.host_pages = ppr
        else:
            self._set("paged_kv_indptr", torch.arange(B + 1, dtype=torch.int32, device=dev) * self.indptr_stride)
            self._set("paged_kv_indices", torch.zeros(B * ppr, dtype=torch.int32, device=dev))
        self.last_page_len = torch.full((B,), self.last_page_len_init, dtype=torch.int32, device=dev)

    def map_pages(self, n_pages, last_page_len):
        """Request b maps pages b*ppr .. b*ppr+n_pages-1; last page holds `last_page_len` rows
        (pre_encode, Engine/SnapKV/backend.py:270-275)."""
        o, B, dev = self.o, self.o.batch_size, self.o.device
        self.host_pages = n_pages
        self._get("num_pages_per_request").fill_(n_pages)
        base = torch.arange(B, dtype=torch.int32, device=dev).view(-1, 1) * self.ppr
        self._set("paged_kv_indices", (base + torch.arange(n_pages, dtype=torch.int32, device=dev).view(1, -1)).flatten())
        self._get("paged_kv_indptr").copy_(torch.arange(B + 1, dtype=torch.int32, device=dev) * n_pages)
        self.last_page_len = torch.full((B,), last_page_len, dtype=torch.int32, device=dev)

    def table(self):
        return PageTable(self._get("paged_kv_indices"), self._get("paged_kv_indptr"), self.last_page_len,
                         max(self.host_pages, 1))


def _chunks(input_ids):
    """The prefill walk: per chunk of CHUNK columns (ids, n, is_last, final).  `is_last` is the reference's flag -- a
    chunk shorter than CHUNK was seen, and it sticks (backend.py:238-245); it is what triggers the SnapKV select and the
    StreamingLLM rotation.  `final` is the walk's last chunk, the only one whose tokens anybody reads.  A prefix that is
    a multiple of CHUNK has a final chunk and no is_last one."""
    seq_len = input_ids.shape[1]
    num_chunks = (seq_len + CHUNK - 1) // CHUNK
    is_last = False
    for i in range(num_chunks):
        ids = input_ids[:, i * CHUNK:min((i + 1) * CHUNK, seq_len)]
        n = ids.shape[1]
        if n != CHUNK:
            is_last = True
        yield ids, n, is_last, i == num_chunks - 1


class _BackendBase:
    def __init__(self, dtype=torch.bfloat16, device="cuda:0"):
        self.dtype, self.device = dtype, device
        self.model = None
        self.cachelens = None
        self._graphs = {}
        self._use_graphs = False

    # -- to be provided by the wrapper modules (which loader / which Transformer class)
    _loader = None

    def load_model(self, checkpoints, use_tp: bool, rank_group=None, group=None):
        from .utils import enable_tuned_gemms
        enable_tuned_gemms()
        self.model = type(self)._loader(checkpoint_path=checkpoints, device=self.device, precision=self.dtype,
                                        use_tp=use_tp, rank_group=rank_group, group=group)

    def compile(self):
        """The reference compiles with Inductor/Triton + CUDA graphs (Engine/SnapKV/backend.py:116-125); here the
        decode steps are captured into hipGraphs on first use (see Engine/graph.py)."""
        self._use_graphs = True

    def _alloc_state(self, max_batch_size, pages_per_request):
        """What every setup_caches() allocates: the length tensor, qo_indptr and the un-prefixed paged state `_t`.  An
        engine with a second cache then makes its 'draft_' state `_d`, stating that table's initial form."""
        self.batch_size, self.page_size = max_batch_size, PAGE_SIZE
        self.cachelens = torch.zeros(max_batch_size, dtype=torch.int32, device=self.device)
        self.qo_indptr = torch.arange(max_batch_size + 1, dtype=torch.int32, device=self.device)
        self._t = _PagedState(self, "", pages_per_request)
        self._d = None

    @torch.no_grad()
    def clear_kv(self):
        for b in self.model.layers:
            b.attention.kv_cache.kv_cache.zero_()
            if self._d is not None:
                b.attention.kv_cache.draft_cache.zero_()
        self._reset_kv_calibration()
        self.cachelens.zero_()
        if getattr(self, "draft_cachelens", None) is not None:
            self.draft_cachelens.zero_()
        self.qo_indptr = torch.arange(self.batch_size + 1, dtype=torch.int32, device=self.device)
        self._t.reset()
        if self._d is not None:
            self._d.reset()

    def _qo(self, n):
        return self.qo_indptr * n

    def _decode_rows(self, *per_request, two_token_step=True):
        """Row counts of this engine's decode / verify steps: batch x (1, dec_len ..., and 2 -- the two-token step after an
        all-accept iteration -- for the engines that DRAFT with it: the stand-alone draft models and the StreamingLLM
        self-speculation engine; a longspec target and the SnapKV self-speculation engine never see it); the model packs /
        releases weight copies for exactly these (Transformer.setup_caches(decode_rows=...))."""
        B = self.batch_size
        return sorted({B * int(n) for n in (1,) + ((2,) if two_token_step else ()) + tuple(per_request) if n})

    def _prefill_begin(self):
        """Prefill-sized products run on the library GEMM over the row-major weights: re-materialise the ones released
        after the previous prefill (Transformer.restore_rowmajor)."""
        if hasattr(self.model, "restore_rowmajor"):
            self.model.restore_rowmajor()

    def _prefill_end(self):
        """Decode reads most weights in the streaming layout only: free their row-major tensors (one resident copy)."""
        if hasattr(self.model, "release_rowmajor"):
            self.model.release_rowmajor()

    def _reset_kv_calibration(self):
        """fp8 caches re-calibrate their static scales on the first prefill chunk of every encode()."""
        for b in self.model.layers:
            b.attention.kv_cache.calibrated = False

    def _paged_prefill(self, input_ids, draft: _PagedState = None):
        """Chunked prefill of the full-context cache `_t` (backend.py:232-268, backend_draft.py:176-209,
        StreamingLLM/backend.py:190-211); with `draft`, the is_last chunk also runs the SnapKV select into that cache.
        Returns (tokens of the final chunk, whether an is_last chunk ran)."""
        tokens, is_last, done = None, False, 0
        for i, (ids, n, is_last, final) in enumerate(_chunks(input_ids)):
            self._t.map_pages(i + 1, n)                       # pre_encode
            self.model.skip_head = not final
            self.model.sample_role = "prefill"
            tokens = self.model.prefill(ids, self.cachelens, self._qo(n), self._t.table(), is_last=is_last,
                                        draft_tab=draft.table() if (draft is not None and is_last) else None,
                                        ctx_len=done + n)
            self.cachelens += n
            done += n
        self.model.skip_head = False
        return tokens, is_last

    def _step(self, kind, model_fn, lens_attr, state: _PagedState, tables, role, input_ids, cachelen_update=None,
              benchmark=False):
        """One decode step, as every public step method runs it: the rows are counted into `state`'s last page
        (pre_decode / pre_verify / pre_spec), `model_fn(ids, lengths, qo_indptr * n, *tables)` runs -- as a replay of its
        captured hipGraph after compile(), keyed by `kind` and pinning exactly the attributes it reads -- and the length
        attribute `lens_attr` advances by n, or by `cachelen_update` after a two-token step, whose last-page length is
        REBOUND to a new tensor like the reference's; benchmark=True undoes the updates (backend.py:140-143)."""
        n = input_ids.shape[1]
        state.last_page_len += n
        self.model.sample_role = role
        fn = lambda ids: model_fn(ids, getattr(self, lens_attr), self._qo(n), *(t.table() for t in tables))
        if self._use_graphs:
            from .graph import run_captured
            names = (lens_attr, "qo_indptr") + tuple(name for t in tables for name in t.names)
            out = run_captured(self, (kind, n), names, fn, input_ids)
        else:
            out = fn(input_ids)
        lens = getattr(self, lens_attr)
        if cachelen_update is None:
            lens += n
        else:
            cu = cachelen_update.to(torch.int32).flatten()
            lens += cu
            state.last_page_len = state.last_page_len - n + cu
        if benchmark:
            lens -= n
            state.last_page_len -= n
        return out


# ======================================================================================= target (+ SnapKV self-spec)
class SnapKVTargetBackend(_BackendBase):
    """Engine/SnapKV/backend.py LMBackend: the paged-KV target engine of every longspec / baseline run and,
    with draft_dec_len set, the SnapKV self-speculation engine (two caches, one set of weights)."""

    def __init__(self, dtype=torch.bfloat16, device: str = "cuda:0", dec_len: int = 1, draft_dec_len: int = None):
        super().__init__(dtype, device)
        self.dec_len = dec_len
        self.is_spec = draft_dec_len is not None
        self.draft_dec_len = draft_dec_len
        self.draft_cachelens = None

    @torch.no_grad()
    def setup_caches(self, max_batch_size: int = 1, max_seq_length: int = 2048, draft_budget=0, window_size=32,
                     kv_dtype="bf16", kv_layout=None):
        """kv_dtype="fp8": the full-context cache is OCP e4m3fn with static per-head scales calibrated on the
        first prefill chunk (not in the reference; BASELINE.json configs[4]).  The compressed draft cache stays bf16.
        kv_layout="HND": the full-context cache keeps the rows of one kv head contiguous inside a page (the
        reference's flashinfer wrappers are planned "NHD": Engine/SnapKV/backend.py:30); same results, longer
        contiguous runs for the verify step's stream (matters for fp8 rows of 128 bytes).  None = default_kv_layout()."""
        kv_layout = default_kv_layout() if kv_layout is None else kv_layout
        self.max_length = max_seq_length
        self.max_num_pages, self.max_num_pages_per_request = _pages_per_request(max_batch_size, max_seq_length)
        self._alloc_state(max_batch_size, self.max_num_pages_per_request)
        if self.is_spec:
            self.draft_budget, self.window_size = draft_budget, window_size
            self.draft_pages_per_request = draft_budget // PAGE_SIZE + 1
            self.draft_num_pages = self.draft_pages_per_request * max_batch_size
            self.draft_cachelens = torch.zeros(max_batch_size, dtype=torch.int32, device=self.device)
            self._d = _PagedState(self, "draft_", self.draft_pages_per_request, last_page_len_init=1, full_table=True)
            self.model.setup_caches(num_pages=self.max_num_pages, page_size=PAGE_SIZE, spec=True,
                                    draft_num_pages=self.draft_num_pages, draft_budget=draft_budget,
                                    window_size=window_size, max_positions=max_seq_length + 256, kv_dtype=kv_dtype,
                                    kv_layout=kv_layout,
                                    decode_rows=self._decode_rows(self.dec_len, getattr(self, "draft_dec_len", None),
                                                                 two_token_step=False))
        else:
            self.model.setup_caches(num_pages=self.max_num_pages, page_size=PAGE_SIZE,
                                    max_positions=max_seq_length + 256, kv_dtype=kv_dtype, kv_layout=kv_layout,
                                    decode_rows=self._decode_rows(self.dec_len, two_token_step=False))

    @torch.no_grad()
    def encode(self, input_ids: torch.LongTensor, benchmark=False):
        """Chunked prefill (backend.py:232-268)."""
        self.clear_kv()
        self._prefill_begin()
        tokens, is_last = self._paged_prefill(input_ids, self._d)
        if self.is_spec:
            if not is_last:
                raise ValueError("SnapKV self-speculation: prefix_len is a multiple of 128, so no last chunk ran the "
                                 "select and the draft cache is empty (need (prefix_len - window_size) % 128 == 0)")
            self.draft_cachelens.copy_(self.cachelens)
        self._prefill_end()
        return tokens

    @torch.no_grad()
    def inference(self, input_ids: torch.LongTensor, benchmark=False):
        """Autoregressive step / longspec verification (backend.py:129-159)."""
        role = "verify" if input_ids.shape[1] > 1 else "baseline"
        return self._step("fwd", self.model.forward, "cachelens", self._t, (self._t,), role, input_ids,
                          benchmark=benchmark)

    @torch.no_grad()
    def verify(self, input_ids: torch.LongTensor, benchmark=False):
        """Self-spec verification: also appends the gamma+1 rows to the draft cache (backend.py:163-197)."""
        self.draft_paged_kv_last_page_len += 1                # pre_verify; benchmark=True leaves these two as they are
        self.draft_cachelens += 1
        return self._step("verify", self.model.verify, "cachelens", self._t, (self._t, self._d), "verify", input_ids,
                          benchmark=benchmark)

    @torch.no_grad()
    def speculate(self, input_ids: torch.LongTensor, benchmark=False):
        """Self-spec draft step over the SnapKV draft cache (backend.py:200-229)."""
        return self._step("spec", self.model.draft_forward, "draft_cachelens", self._d, (self._d,), "draft", input_ids,
                          benchmark=benchmark)


# ======================================================================================= SnapKV stand-alone draft
class SnapKVDraftBackend(_BackendBase):
    """Engine/SnapKV/backend_draft.py LMBackend_Draft: small draft model, full-KV prefill, SnapKV select on the
    last chunk into `draft_cache`, decode over the draft cache only (draft_budget == -1: full-KV draft)."""

    def __init__(self, dtype=torch.bfloat16, device: str = "cuda:0", dec_len: list = [1], draft_budget: int = None):
        super().__init__(dtype, device)
        self.dec_len = dec_len
        self.is_compress = draft_budget != -1

    @torch.no_grad()
    def setup_caches(self, max_batch_size: int = 1, max_seq_length: int = 2048, draft_budget=0, window_size=32):
        self.max_num_pages, self.max_num_pages_per_request = _pages_per_request(max_batch_size, max_seq_length)
        self._alloc_state(max_batch_size, self.max_num_pages_per_request)
        if self.is_compress:
            self.draft_budget, self.window_size = draft_budget, window_size
            self.draft_pages_per_request = draft_budget // PAGE_SIZE + 1
            self.draft_num_pages = self.draft_pages_per_request * max_batch_size
            self._d = _PagedState(self, "draft_", self.draft_pages_per_request, last_page_len_init=1, full_table=True)
            self.model.setup_caches(num_pages=self.max_num_pages, page_size=PAGE_SIZE, spec=True,
                                    draft_num_pages=self.draft_num_pages, draft_budget=draft_budget,
                                    window_size=window_size, max_positions=max_seq_length + 256,
                                    decode_rows=self._decode_rows())
        else:
            self.model.setup_caches(num_pages=self.max_num_pages, page_size=PAGE_SIZE,
                                    max_positions=max_seq_length + 256, decode_rows=self._decode_rows())

    @torch.no_grad()
    def encode(self, input_ids: torch.LongTensor, benchmark=False):
        """backend_draft.py:176-209."""
        self.clear_kv()
        self._prefill_begin()
        tokens, is_last = self._paged_prefill(input_ids, self._d)
        if self.is_compress and not is_last:
            raise ValueError("SnapKV draft: prefix_len is a multiple of 128, so no last chunk ran the select and the "
                             "draft cache is empty (need (prefix_len - window_size) % 128 == 0)")
        self._prefill_end()
        return tokens

    @torch.no_grad()
    def inference(self, input_ids: torch.LongTensor, benchmark=False, cachelen_update=None):
        """One (or, after an all-accept iteration, a two-token) draft step (backend_draft.py:113-173)."""
        if self.is_compress:                                  # pre_decode: into the cache the step reads
            out = self._step("draft", self.model.draft_forward, "cachelens", self._d, (self._d,), "draft", input_ids,
                             cachelen_update)
        else:
            out = self._step("fwd", self.model.forward, "cachelens", self._t, (self._t,), "draft", input_ids,
                             cachelen_update)
        if benchmark:   # as the reference: always the un-prefixed table (backend_draft.py:139-142)
            n = input_ids.shape[1]
            self.cachelens -= n
            self.paged_kv_last_page_len -= n
        return out


# ======================================================================================= StreamingLLM drafts
class _StreamingMixin:
    """Sink(16)+window prefill shared by the stand-alone StreamingLLM draft and the self-spec engine."""

    def _stream_encode(self, input_ids, state: _PagedState, lens_attr, which):
        self._prefill_begin()
        tokens = None
        ctx = 0                                       # host mirror of the (capped) cache length
        for ids, n, is_last, final in _chunks(input_ids):
            if ctx + n <= self.draft_budget:          # pre_encode (StreamingLLM/backend_draft.py:155-192)
                state.map_pages(state.host_pages + 1, n)
            else:
                state.map_pages(state.ppr, self.draft_budget % PAGE_SIZE)
            self.model.skip_head = not final
            self.model.sample_role = "prefill"
            tokens = self.model.stream_prefill(ids, ctx, self._qo(n), state.table(), is_last, which, self.batch_size)
            ctx += n
            lens = getattr(self, lens_attr)
            lens += n
            if ctx >= self.draft_budget:
                ctx = self.draft_budget
                lens.fill_(self.draft_budget)
        self.model.skip_head = False
        self._prefill_end()
        return tokens


class StreamingDraftBackend(_BackendBase, _StreamingMixin):
    """Engine/StreamingLLM/backend_draft.py LMBackend_Draft: the draft's only cache holds 16 sink tokens plus the
    most recent budget-16; RoPE positions are cache slots."""

    def __init__(self, dtype=torch.bfloat16, device: str = "cuda:0"):
        super().__init__(dtype, device)

    @torch.no_grad()
    def setup_caches(self, max_batch_size: int = 1, draft_budget=0):
        self.draft_budget = draft_budget
        self.max_num_pages_per_request = draft_budget // PAGE_SIZE + 1
        self.max_num_pages = self.max_num_pages_per_request * max_batch_size
        self._alloc_state(max_batch_size, self.max_num_pages_per_request)
        self.model.setup_caches(num_pages=self.max_num_pages, page_size=PAGE_SIZE, draft_budget=draft_budget,
                                streaming=True, max_positions=self.max_num_pages_per_request * PAGE_SIZE + 256,
                                decode_rows=self._decode_rows())

    @torch.no_grad()
    def encode(self, input_ids: torch.LongTensor, benchmark=False):
        self.clear_kv()
        return self._stream_encode(input_ids, self._t, "cachelens", "kv_cache")

    @torch.no_grad()
    def inference(self, input_ids: torch.LongTensor, benchmark=False, cachelen_update=None):
        """StreamingLLM/backend_draft.py:89-124."""
        return self._step("fwd", self.model.forward, "cachelens", self._t, (self._t,), "draft", input_ids,
                          cachelen_update, benchmark)


class StreamingSelfSpecBackend(_BackendBase, _StreamingMixin):
    """Engine/StreamingLLM/backend.py LMBackend: one set of weights, the full target cache and a streaming
    draft cache (config 2 of BASELINE.json)."""

    def __init__(self, dtype=torch.bfloat16, device: str = "cuda:0", dec_len: int = 1):
        super().__init__(dtype, device)
        self.dec_len = dec_len
        self.draft_cachelens = None

    @torch.no_grad()
    def setup_caches(self, max_batch_size: int = 1, max_seq_length: int = 2048, draft_budget=0, kv_dtype="bf16",
                     kv_layout=None):
        kv_layout = default_kv_layout() if kv_layout is None else kv_layout
        self.draft_budget = draft_budget
        self.max_num_pages, self.max_num_pages_per_request = _pages_per_request(max_batch_size, max_seq_length)
        self._alloc_state(max_batch_size, self.max_num_pages_per_request)
        self.draft_cachelens = torch.zeros(max_batch_size, dtype=torch.int32, device=self.device)
        self.draft_max_num_pages_per_request = draft_budget // PAGE_SIZE + 1
        self.draft_max_num_pages = self.draft_max_num_pages_per_request * max_batch_size
        self._d = _PagedState(self, "draft_", self.draft_max_num_pages_per_request,
                              indptr_stride=self.draft_max_num_pages_per_request)   # StreamingLLM/backend.py:316
        self.model.setup_caches(num_pages=self.max_num_pages, page_size=PAGE_SIZE, spec=True,
                                draft_num_pages=self.draft_max_num_pages, draft_budget=draft_budget, streaming=True,
                                max_positions=max_seq_length + 256, kv_dtype=kv_dtype, kv_layout=kv_layout,
                                decode_rows=self._decode_rows(self.dec_len))

    @torch.no_grad()
    def encode(self, input_ids: torch.LongTensor, benchmark=False):
        """Target prefill (StreamingLLM/backend.py:190-211)."""
        self.clear_kv()
        self._prefill_begin()
        tokens, _ = self._paged_prefill(input_ids)
        self._prefill_end()
        return tokens

    @torch.no_grad()
    def draft_encode(self, input_ids: torch.LongTensor, benchmark=False):
        """Second pass filling the streaming draft cache (StreamingLLM/backend.py:234-258)."""
        return self._stream_encode(input_ids, self._d, "draft_cachelens", "draft_cache")

    @torch.no_grad()
    def verify(self, input_ids: torch.LongTensor, benchmark=False):
        return self._step("verify", self.model.verify, "cachelens", self._t, (self._t,), "verify", input_ids,
                          benchmark=benchmark)

    @torch.no_grad()
    def speculate(self, input_ids: torch.LongTensor, benchmark=False, cachelen_update=None):
        return self._step("spec", self.model.draft_forward, "draft_cachelens", self._d, (self._d,), "draft", input_ids,
                          cachelen_update, benchmark)

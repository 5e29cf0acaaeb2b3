"""The operand boundary of magicdec_amd.ops, checked on the CPU against a recording stand-in for the library.

ops.py is the only way from tensors to the kernels, and the C side sees raw pointers: an operand the wrapper lets through
is read or written out of bounds on the GPU.  So the bad operands exist only here: `_lib.load` returns a recorder, the
tensors are CPU tensors that answer `is_cuda`, and two tables drive every wrapper --

* ACCEPTED: one valid call per wrapper and optional form; it reaches exactly one launch, the named one, and returns
  tensors of the documented shape and dtype;
* REFUSED: one row per wrapper and bad operand; it raises the stated exception type before any launch.

`python -m tests.test_ops_contract_cpu [FILE]` writes the call vector of every ACCEPTED row (profiles/README.md).
"""
import ctypes
import sys

import pytest
import torch

from magicdec_amd import _lib, ops

BF, F32, I8, I32, I64, FP8 = torch.bfloat16, torch.float32, torch.int8, torch.int32, torch.int64, torch.float8_e4m3fn


class OnGpu(torch.Tensor):
    is_cuda = property(lambda self: True)


def gpu(t):
    return t.as_subclass(OnGpu)


def host(t):
    return t.as_subclass(torch.Tensor)


def z(*shape, dtype=BF):
    return gpu(torch.zeros(shape, dtype=dtype))


def i32(*shape):
    return z(*shape, dtype=I32)


def i64(*shape):
    return z(*shape, dtype=I64)


class Recorder:
    """Every md_* attribute records (name, args): 0 for a launch, 256 for a *_workspace_bytes query, 0 for
    md_snapkv_scores_offset, 1 for a *_supported query."""
    QUERIES = ("_workspace_bytes", "_supported", "_scores_offset")

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("md_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return 256 if name.endswith("_workspace_bytes") else 1 if name.endswith("_supported") else 0
        return fn

    def launches(self):
        return [c for c in self.calls if not c[0].endswith(self.QUERIES)]


@pytest.fixture
def rec(monkeypatch):
    return install(monkeypatch)


def install(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: r)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    return r


# ----------------------------------------------------------------------------------------- operands
def packed(N, K, swiglu=False, dtype=BF):
    pw = ops.PackedWeight(z(N, K, dtype=dtype), swiglu=swiglu)
    pw.data = gpu(pw.data)
    return pw


def workspace():
    w = ops.AttnWorkspace("cpu")
    base = (-w.buf.data_ptr()) % 256 + 16                     # 16 bytes past a boundary: a carve lands 240 in
    w.buf = gpu(w.buf[base:base + (1 << 19)])
    return w


def table():
    t = ops.RopeTable(16, 64, 10000.0, 1.0, device="cpu")
    t.table = gpu(t.table)
    return t


def cache(layout="NHD", dtype=BF):
    """Two pages of 128 rows, one kv head, D = 64."""
    return z(2, 2, 128, 1, 64, dtype=dtype) if layout == "NHD" else z(2, 2, 1, 128, 64, dtype=dtype)


def tab(fmt="page_indices{} page_indptr{} last_page_len{}", sfx=""):
    """The page table of one request."""
    return dict(zip(fmt.format(sfx, sfx, sfx).split(), (i32(1), i32(2), i32(1))))


def fp8():
    return dict(kv_cache=cache("HND", FP8), kv_scales=(z(1, dtype=F32), z(1, dtype=F32)), kv_layout="HND")


def qkv():
    return dict(q=z(2, 2, 64), k=z(2, 1, 64), v=z(2, 1, 64))


def pro_of(x):
    return ops.DeferredNorm(x, z(2, 4, dtype=F32), z(128), 1e-5)


def rows_and(**kw):
    return dict(x=z(2, 128), **kw)


def with_pro(**kw):
    o = rows_and(**kw)
    return dict(o, pro=pro_of(o["x"]))


def add_norm(**kw):
    return rows_and(resid=z(2, 32), norm_weight=z(32), eps=1e-5, bias=z(32), workspace=workspace(), **kw)


def fused_qkv(**kw):
    return dict(rows_and(weight=packed(256, 128), bias=z(256), H=2, KH=1, D=64, rows_per_req=2, offsets=i32(1),
                         table=table(), kv_cache=cache()), **tab(), **kw)


def halves():
    h = z(2, 128)
    return dict(a=h[:, :64], b=h[:, 64:])


def accept(**kw):
    o = dict(tokens_buffer=i64(2, 2), target_tokens=i64(2, 2), output=i64(2, 8), num_nodes=i64(2), cachelens=i32(2),
             last_page_len=i32(2), draft_cachelens=i32(2), draft_last_page_len=i32(2), gamma=1, draft_rollback=1,
             draft_cap=1, eot_1=1, eot_2=2, max_nodes=8, accept_nums=i64(2), bonus=i64(2), double_buffer=i64(2, 2),
             cachelens_update=i64(2), flags=i32(2))
    return dict(o, **kw)


def draw(rows=2, n=1, **kw):
    return dict(logits=z(rows, 64), n=n, temperature=0.8, top_p=0.9, seed=7, purpose=ops.SAMPLE_DRAFT, counters=i32(4),
                advance=ops.ADVANCE_STEP, **kw)


def ring(width=64):
    return dict(ring=z(2, 1, width), ring_stats=i64(2, 1, 2))


def verify(**kw):
    return dict(dict(logits=z(4, 64), tokens_buffer=i64(2, 2), target_stats=i64(4, 2), counters=i32(4), temperature=0.8,
                     top_p=0.9, seed=7, **ring()), **kw)


def shard(rows=2, **kw):
    return dict(logits=z(rows, 32), vocab_offset=32, vocab_total=64, **kw)


def shard_draw(top_p=0.9, **kw):
    return shard(n=1, temperature=0.8, top_p=top_p, seed=7, purpose=ops.SAMPLE_DRAFT, counters=i32(4), red=i64(2),
                 hist_hi=i64(2, 256), hist_lo=i64(2, 256) if top_p < 1 else None, cand=i64(2), **kw)


def shard_verify(top_p=0.9, **kw):
    return dict(shard(4, tokens_buffer=i64(2, 2), red=i64(6), hist_hi=i64(4, 256),
                      hist_lo=i64(4, 256) if top_p < 1 else None, target_stats=i64(4, 2), counters=i32(4),
                      temperature=0.8, top_p=top_p, seed=7, cand=i64(2, 3), **ring(32)), **kw)


SNAP = dict(ctx_len=64, window=2, budget=6, pool_kernel=5)

# name -> (wrapper, builder of its keyword operands)
CASES = {
    "update_kv": ("update_kv", lambda: dict(k=z(2, 1, 64), v=z(2, 1, 64), kv_append_indptr=i32(2), kv_cache=cache(),
                                            **tab("kv_page_indices kv_page_indptr kv_page_lastlen"))),
    "update_kv_fp8_hnd": ("update_kv", lambda: dict(k=z(2, 1, 64), v=z(2, 1, 64), kv_append_indptr=i32(2), **fp8(),
                                                    **tab("kv_page_indices kv_page_indptr kv_page_lastlen"))),
    "rope": ("rope", lambda: dict(q=z(2, 2, 64), k=z(2, 1, 64), indptr=i32(2), offsets=i32(1), table=table())),
    "rope_q_only": ("rope", lambda: dict(q=z(2, 2, 64), k=None, indptr=i32(2), offsets=i32(1), table=table())),
    "rope_append": ("rope_append", lambda: dict(qkv(), indptr=i32(2), offsets=i32(1), table=table(), kv_cache=cache(),
                                                **tab())),
    "rope_append_two_caches": ("rope_append", lambda: dict(qkv(), indptr=i32(2), offsets=i32(1), table=table(),
                                                           kv_cache=cache(), kv_cache2=cache(), **tab(),
                                                           **tab(sfx="2"))),
    "rope_append_fp8_hnd": ("rope_append", lambda: dict(qkv(), indptr=i32(2), offsets=i32(1), table=table(), **fp8(),
                                                        **tab())),
    "paged_attention": ("paged_attention", lambda: dict(q=z(2, 2, 64), kv_cache=cache(), qo_indptr=i32(2), n_max=2,
                                                        max_pages_per_req=1, workspace=workspace(), **tab())),
    "paged_attention_out_fp8_hnd": ("paged_attention", lambda: dict(q=z(2, 2, 64), qo_indptr=i32(2), n_max=2,
                                                                    max_pages_per_req=1, workspace=workspace(),
                                                                    out=z(2, 2, 64), **fp8(), **tab())),
    "snapkv_select": ("snapkv_select", lambda: dict(
        q_win=z(2, 2, 64), kv_cache=cache(), **tab("page_indices page_indptr _"), **SNAP, draft_cache=cache(),
        **tab("draft_page_indices draft_page_indptr draft_last_page_len"), workspace=workspace())),
    "snapkv_select_scores": ("snapkv_select", lambda: dict(
        q_win=z(2, 2, 64), **fp8(), **tab("page_indices page_indptr _"), **SNAP, draft_cache=cache(),
        **tab("draft_page_indices draft_page_indptr draft_last_page_len"), workspace=workspace(), return_scores=True)),
    "streaming_shift_append": ("streaming_shift_append", lambda: dict(k_new=z(2, 1, 64), v_new=z(2, 1, 64),
                                                                      kv_cache=cache(), n_new=2, kv_len=64, sink=4,
                                                                      pages_per_req=1)),
    "streaming_rotate": ("streaming_rotate", lambda: dict(kv_cache=cache(), rot_cache=cache(), B=1, valid_len=64,
                                                          pages_per_req=1, table=table())),
    "linear": ("linear", lambda: rows_and(weight=z(32, 128), bias=z(32), workspace=workspace())),
    "linear_packed_swiglu": ("linear", lambda: rows_and(weight=packed(64, 128, True), swiglu=True,
                                                        workspace=workspace())),
    "linear_int8": ("linear", lambda: rows_and(weight=z(32, 128, dtype=I8), scales=z(32), workspace=workspace())),
    "linear_out": ("linear", lambda: rows_and(weight=packed(32, 128), workspace=workspace(), out=z(2, 64)[:, :32])),
    "linear_pro": ("linear", lambda: with_pro(weight=packed(64, 128, True), swiglu=True, workspace=workspace())),
    "linear_add_rmsnorm": ("linear_add_rmsnorm", lambda: add_norm(weight=z(32, 128))),
    "linear_add_rmsnorm_int8": ("linear_add_rmsnorm", lambda: add_norm(weight=packed(32, 128, dtype=I8),
                                                                       scales=z(32))),
    "fused_split_linear": ("fused_split_linear", lambda: rows_and(weight=packed(32, 128), bias=z(32),
                                                                  workspace=workspace())),
    "fused_split_linear_add_rmsnorm": ("fused_split_linear_add_rmsnorm", lambda: add_norm(weight=packed(32, 128))),
    "linear_block": ("linear_block", lambda: rows_and(weight=packed(32, 128), bias=z(32), workspace=workspace())),
    "linear_block_swiglu_out": ("linear_block", lambda: rows_and(weight=packed(64, 128, True), swiglu=True,
                                                                 workspace=workspace(), out=z(2, 64)[:, :32])),
    "linear_block_add_rmsnorm": ("linear_block_add_rmsnorm", lambda: add_norm(weight=packed(32, 128))),
    "fused_linear": ("fused_linear", lambda: rows_and(weight=packed(32, 128), bias=z(32))),
    "fused_linear_swiglu_pro": ("fused_linear", lambda: with_pro(weight=packed(64, 128, True), swiglu=True)),
    "fused_linear_resid_ssq": ("fused_linear", lambda: rows_and(weight=packed(32, 128), resid=z(2, 64)[:, 32:],
                                                                want_ssq=True)),
    "fused_linear_out": ("fused_linear", lambda: rows_and(weight=packed(32, 128), out=z(2, 64)[:, :32])),
    "fused_qkv": ("fused_qkv_rope_append", fused_qkv),
    "fused_qkv_two_caches_pro": ("fused_qkv_rope_append", lambda: (lambda o: dict(o, pro=pro_of(o["x"])))(
        fused_qkv(kv_cache2=cache(), **tab(sfx="2")))),
    "fused_qkv_fp8_hnd": ("fused_qkv_rope_append", lambda: fused_qkv(**fp8())),
    "rmsnorm": ("rmsnorm", lambda: dict(x=z(1, 2, 128), weight=z(128), eps=1e-5)),
    "add_rmsnorm": ("add_rmsnorm", lambda: dict(x=z(2, 128), r=z(2, 128), weight=z(128), eps=1e-5)),
    "silu_mul": ("silu_mul", halves),
    "argmax": ("argmax", lambda: dict(logits=z(2, 64))),
    "argmax_values": ("argmax", lambda: dict(logits=z(2, 64), index_offset=64, return_values=True)),
    "argmax_tp_slots": ("argmax_tp_slots", lambda: dict(logits=z(2, 64), tp_rank=1, tp_world=2, index_offset=64)),
    "tp_argmax_merge": ("tp_argmax_merge", lambda: dict(vals=z(2, 2), idx=i64(2, 2))),
    "tp_argmax_merge_views": ("tp_argmax_merge", lambda: dict(vals=z(2, 4)[:, :2], idx=i64(2, 2).t())),
    "accept_rollback": ("accept_rollback", accept),
    "accept_rollback_no_draft": ("accept_rollback", lambda: accept(draft_cachelens=None, draft_last_page_len=None,
                                                                   double_buffer=None, cachelens_update=None)),
    "sample_rows": ("sample_rows", draw),
    "sample_rows_ring": ("sample_rows", lambda: draw(**ring())),
    "sample_rows_sel_out": ("sample_rows", lambda: draw(n=2, row_sel=i64(1), out=i64(1, 2))),
    "spec_verify_sample": ("spec_verify_sample", verify),
    "spec_verify_sample_view_out": ("spec_verify_sample", lambda: verify(tokens_buffer=i64(2, 4)[:, :2],
                                                                         out=i64(2, 2))),
    "shard_max": ("shard_max", lambda: shard(n=1, red=i64(2))),
    "shard_max_probe": ("shard_max", lambda: shard(4, n=1, red=i64(6), tokens_buffer=i64(2, 2), ring=z(2, 1, 64),
                                                   ring_col_offset=32)),
    "shard_hist": ("shard_hist", lambda: dict(logits=z(2, 32), n=1, temperature=0.8, top_p=0.9, red=i64(2),
                                              hist_out=i64(2, 256))),
    "shard_hist_low": ("shard_hist", lambda: dict(logits=z(2, 32), n=1, temperature=0.8, top_p=0.9, red=i64(2),
                                                  hist_out=i64(2, 256), hist_hi=i64(2, 256))),
    "shard_draw": ("shard_draw", shard_draw),
    "shard_draw_ring_top1": ("shard_draw", lambda: shard_draw(1.0, **ring(32))),
    "shard_finish": ("shard_finish", lambda: dict(cand=i64(2), n=1, counters=i32(4), advance=ops.ADVANCE_ITER)),
    "shard_finish_out": ("shard_finish", lambda: dict(cand=i64(2), n=2, counters=i32(4), advance=ops.ADVANCE_ITER,
                                                      out=i64(2, 2))),
    "spec_verify_shard": ("spec_verify_shard", shard_verify),
    "spec_verify_shard_top1": ("spec_verify_shard", lambda: shard_verify(1.0)),
    "spec_verify_shard_finish": ("spec_verify_shard_finish", lambda: dict(cand=i64(2, 3), tokens_buffer=i64(2, 2),
                                                                         counters=i32(4))),
}


def run(rec, case, bad=None):
    """Build the case's operands (with the overrides of `bad`), call the wrapper -> (operands, what it returned)."""
    fn, build = CASES[case]
    o = build()
    if bad is not None:
        o.update(bad(o))
    o.pop("_", None)
    rec.calls.clear()          # building a RopeTable goes through the library too
    return o, getattr(ops, fn)(**o)


# ----------------------------------------------------------------------------------------- accepted
Q, T = ((2, 2, 64), BF), ((2, 2), I64)
ACCEPTED = {    # case -> (the launch it reaches, (shape, dtype) of what it returns)
    "update_kv": ("md_append_paged_kv", None),
    "update_kv_fp8_hnd": ("md_append_paged_kv", None),
    "rope": ("md_rope", (Q, ((2, 1, 64), BF))),
    "rope_q_only": ("md_rope", (Q, None)),
    "rope_append": ("md_rope_append", Q),
    "rope_append_two_caches": ("md_rope_append", Q),
    "rope_append_fp8_hnd": ("md_rope_append", Q),
    "paged_attention": ("md_paged_attn", Q),
    "paged_attention_out_fp8_hnd": ("md_paged_attn", Q),
    "snapkv_select": ("md_snapkv_select", ((1, 1, 4), I32)),
    "snapkv_select_scores": ("md_snapkv_select", (((1, 1, 4), I32), ((1, 1, 62), BF))),
    "streaming_shift_append": ("md_streaming_shift_append", None),
    "streaming_rotate": ("md_streaming_rotate", None),
    "linear": ("md_linear", ((2, 32), BF)),
    "linear_packed_swiglu": ("md_linear", ((2, 32), BF)),
    "linear_int8": ("md_linear", ((2, 32), BF)),
    "linear_out": ("md_linear", ((2, 32), BF)),
    "linear_pro": ("md_linear_normed", ((2, 32), BF)),
    "linear_add_rmsnorm": ("md_linear_add_rmsnorm", (((2, 32), BF),) * 2),
    "linear_add_rmsnorm_int8": ("md_linear_add_rmsnorm", (((2, 32), BF),) * 2),
    "fused_split_linear": ("md_linear_fused_split", ((2, 32), BF)),
    "fused_split_linear_add_rmsnorm": ("md_linear_fused_split_add_rmsnorm", (((2, 32), BF),) * 2),
    "linear_block": ("md_linear_block", ((2, 32), BF)),
    "linear_block_swiglu_out": ("md_linear_block", ((2, 32), BF)),
    "linear_block_add_rmsnorm": ("md_linear_block_add_rmsnorm", (((2, 32), BF),) * 2),
    "fused_linear": ("md_linear_fused", ((2, 32), BF)),
    "fused_linear_swiglu_pro": ("md_linear_fused", ((2, 32), BF)),
    "fused_linear_resid_ssq": ("md_linear_fused", (((2, 32), BF), ((2, 1), F32))),
    "fused_linear_out": ("md_linear_fused", ((2, 32), BF)),
    "fused_qkv": ("md_linear_fused", Q),
    "fused_qkv_two_caches_pro": ("md_linear_fused", Q),
    "fused_qkv_fp8_hnd": ("md_linear_fused", Q),
    "rmsnorm": ("md_rmsnorm", ((1, 2, 128), BF)),
    "add_rmsnorm": ("md_add_rmsnorm", (((2, 128), BF),) * 2),
    "silu_mul": ("md_silu_mul", ((2, 64), BF)),
    "argmax": ("md_argmax", ((2,), I64)),
    "argmax_values": ("md_argmax", (((2,), BF), ((2,), I64))),
    "argmax_tp_slots": ("md_argmax_tp_slots", (((2, 2), BF), ((2, 2), I64))),
    "tp_argmax_merge": ("md_tp_argmax_merge", ((2,), I64)),
    "tp_argmax_merge_views": ("md_tp_argmax_merge", ((2,), I64)),      # the kernel is handed dense copies
    "accept_rollback": ("md_accept_rollback", None),
    "accept_rollback_no_draft": ("md_accept_rollback", None),
    "sample_rows": ("md_sample_rows", ((2, 1), I64)),
    "sample_rows_ring": ("md_sample_rows", ((2, 1), I64)),
    "sample_rows_sel_out": ("md_sample_rows", ((1, 2), I64)),
    "spec_verify_sample": ("md_spec_verify_sample", T),
    "spec_verify_sample_view_out": ("md_spec_verify_sample", T),
    "shard_max": ("md_sample_shard_max", ((2,), I64)),
    "shard_max_probe": ("md_sample_shard_max", ((6,), I64)),
    "shard_hist": ("md_sample_shard_hist", ((2, 256), I64)),
    "shard_hist_low": ("md_sample_shard_hist", ((2, 256), I64)),
    "shard_draw": ("md_sample_shard_draw", ((2,), I64)),
    "shard_draw_ring_top1": ("md_sample_shard_draw", ((2,), I64)),
    "shard_finish": ("md_sample_shard_finish", ((2, 1), I64)),
    "shard_finish_out": ("md_sample_shard_finish", T),
    "spec_verify_shard": ("md_spec_verify_shard", ((2, 3), I64)),
    "spec_verify_shard_top1": ("md_spec_verify_shard", ((2, 3), I64)),
    "spec_verify_shard_finish": ("md_spec_verify_shard_finish", T),
}


def signature(ret):
    if isinstance(ret, tuple):
        return tuple(signature(r) for r in ret)
    return None if ret is None else (tuple(ret.shape), ret.dtype)


def test_every_case_is_in_the_accepted_table():
    assert set(CASES) == set(ACCEPTED)
    public = {n for n, f in vars(ops).items() if callable(f) and not n.startswith("_") and f.__module__ == ops.__name__
              and not isinstance(f, type) and not n.endswith("_supported")}
    assert public - {fn for fn, _ in CASES.values()} == {"page_overflow_count", "philox_host"}


@pytest.mark.parametrize("case", list(ACCEPTED))
def test_accepted(rec, case):
    launch, returns = ACCEPTED[case]
    o, ret = run(rec, case)
    assert [name for name, _ in rec.launches()] == [launch]
    assert signature(ret) == returns
    if "out" in o:
        assert ret.data_ptr() == o["out"].data_ptr()


# ----------------------------------------------------------------------------------------- refused
def naming(match, bad):
    """An override whose refusal has to carry `match` in its message, unless the row names another fragment."""
    bad.match = match
    return bad


def on_host(name):
    return naming("on the GPU", lambda o: {name: host(o[name])})


def as_dtype(name, dtype):
    return naming(name, lambda o: {name: gpu(host(o[name]).to(dtype))})


def swap(**kw):
    return lambda o: {k: v() if callable(v) else v for k, v in kw.items()}


TABLES = {"update_kv": ("kv_append_indptr", "kv_page_indices", "kv_page_indptr", "kv_page_lastlen"),
          "rope": ("indptr", "offsets"),
          "rope_append": ("indptr", "offsets", "page_indices", "page_indptr", "last_page_len"),
          "rope_append_two_caches": ("page_indices2", "page_indptr2", "last_page_len2"),
          "paged_attention": ("qo_indptr", "page_indices", "page_indptr", "last_page_len"),
          "snapkv_select": ("page_indices", "page_indptr", "draft_page_indices", "draft_page_indptr",
                            "draft_last_page_len"),
          "fused_qkv": ("offsets", "page_indices", "page_indptr", "last_page_len"),
          "fused_qkv_two_caches_pro": ("page_indices2", "page_indptr2", "last_page_len2")}
ACCEPT_TENSORS = [k for k, v in accept().items() if isinstance(v, torch.Tensor)]
K256 = swap(weight=lambda: packed(32, 256))
NOT_DENSE = lambda: z(2, 1, 128)[:, :, ::2]
HND_PAGES = lambda: cache("HND")

REFUSED = [     # (case, exception, what is wrong, the override that makes it so[, a fragment of the message])
    # a page table: every tensor int32 and on the GPU, the second table whole
    *[(c, ValueError, f"{n} on the host", on_host(n)) for c, names in TABLES.items() for n in names],
    *[(c, TypeError, f"{n} int64", as_dtype(n, I64), "int32") for c, names in TABLES.items() for n in names],
    ("rope_append_two_caches", ValueError, "second table missing", swap(page_indptr2=None), "page_indptr2 is missing"),
    ("fused_qkv_two_caches_pro", ValueError, "second table missing", swap(last_page_len2=None),
     "last_page_len2 is missing"),
    *[(c, TypeError, "second cache fp8", swap(kv_cache2=lambda: cache(dtype=FP8)))
      for c in ("rope_append_two_caches", "fused_qkv_two_caches_pro")],
    *[(c, ValueError, "second cache HND", swap(kv_cache2=HND_PAGES))
      for c in ("rope_append_two_caches", "fused_qkv_two_caches_pro")],
    ("rope_append_two_caches", ValueError, "second cache on the host", on_host("kv_cache2")),
    ("snapkv_select", TypeError, "draft cache fp8", swap(draft_cache=lambda: cache(dtype=FP8))),
    ("snapkv_select", ValueError, "draft cache HND", swap(draft_cache=HND_PAGES)),
    # the paged cache
    ("update_kv", ValueError, "unknown layout", swap(kv_layout="DNH")),
    ("update_kv", ValueError, "cache of rank 4", swap(kv_cache=lambda: z(2, 2, 128, 64))),
    ("update_kv", TypeError, "cache float32", swap(kv_cache=lambda: cache(dtype=F32))),
    ("update_kv", ValueError, "cache on the host", on_host("kv_cache")),
    ("update_kv", ValueError, "k rows not dense", swap(k=NOT_DENSE)),
    ("update_kv_fp8_hnd", ValueError, "fp8 without scales", swap(kv_scales=None)),
    ("update_kv_fp8_hnd", ValueError, "two scales for one head", swap(kv_scales=lambda: (z(2, dtype=F32),) * 2)),
    ("update_kv_fp8_hnd", ValueError, "bf16 scales", swap(kv_scales=lambda: (z(1), z(1)))),
    ("update_kv_fp8_hnd", ValueError, "scales on the host", swap(kv_scales=lambda: (torch.zeros(1), torch.zeros(1)))),
    *[(c, TypeError, f"{n} float32", as_dtype(n, F32))
      for c, names in (("update_kv", "kv"), ("rope", "qk"), ("rope_append", "qkv"), ("paged_attention", "q"),
                       ("snapkv_select", ("q_win",))) for n in names],
    ("update_kv", ValueError, "k of D = 32 on a cache of D = 64", swap(k=lambda: z(2, 1, 32)), "k must be"),
    ("update_kv", ValueError, "v a row shorter than k", swap(v=lambda: z(1, 1, 64)), "v must be"),
    ("rope", ValueError, "q of D = 32 under a table for D = 64", swap(q=lambda: z(2, 2, 32)), "q must be"),
    ("rope", ValueError, "k a row shorter than q", swap(k=lambda: z(1, 1, 64)), "k must be"),
    ("rope_append", ValueError, "k of 2 heads on a cache of 1", swap(k=lambda: z(2, 2, 64)), "k must be"),
    ("rope_append", ValueError, "v a row shorter than q", swap(v=lambda: z(1, 1, 64)), "v must be"),
    ("rope_append", ValueError, "q of D = 128 on a cache of D = 64", swap(q=lambda: z(2, 2, 128)), "q must be"),
    ("paged_attention", ValueError, "q of D = 128 on a cache of D = 64", swap(q=lambda: z(2, 2, 128)), "q must be"),
    ("snapkv_select", ValueError, "q_win of D = 128 on a cache of D = 64", swap(q_win=lambda: z(2, 2, 128)), "q_win"),
    ("fused_qkv", ValueError, "heads of D = 32 on a cache of D = 64", swap(H=4, KH=2, D=32), "cache"),
    ("rope", ValueError, "q on the host", on_host("q")),
    ("rope", ValueError, "q rows not dense", swap(q=lambda: z(2, 2, 128)[:, :, ::2])),
    ("paged_attention", ValueError, "q on the host", on_host("q")),
    ("paged_attention", ValueError, "unknown layout", swap(kv_layout="NDH")),
    ("paged_attention_out_fp8_hnd", ValueError, "out of another shape", swap(out=lambda: z(2, 2, 32))),
    ("paged_attention_out_fp8_hnd", ValueError, "out on the host", on_host("out")),
    ("snapkv_select", ValueError, "q_win on the host", on_host("q_win")),
    # the two streaming ops
    *[(c, ValueError, "cache of rank 4", swap(kv_cache=lambda: z(2, 2, 128, 64)))
      for c in ("streaming_shift_append", "streaming_rotate")],
    *[(c, TypeError, "cache fp8", swap(kv_cache=lambda: cache(dtype=FP8)))
      for c in ("streaming_shift_append", "streaming_rotate")],
    *[(c, ValueError, "cache not contiguous", swap(kv_cache=lambda: z(2, 2, 128, 1, 128)[..., ::2]))
      for c in ("streaming_shift_append", "streaming_rotate")],
    *[(c, ValueError, "cache on the host", on_host("kv_cache"))
      for c in ("streaming_shift_append", "streaming_rotate")],
    ("streaming_shift_append", ValueError, "k_new on the host", on_host("k_new")),
    ("streaming_shift_append", ValueError, "v_new not dense", swap(v_new=NOT_DENSE)),
    ("streaming_shift_append", TypeError, "k_new float32", as_dtype("k_new", F32)),
    ("streaming_shift_append", TypeError, "v_new float32", as_dtype("v_new", F32)),
    ("streaming_shift_append", ValueError, "k_new of D = 32 on a cache of D = 64", swap(k_new=lambda: z(2, 1, 32)), "k_new"),
    ("streaming_shift_append", ValueError, "k_new of 2 heads on a cache of 1", swap(k_new=lambda: z(2, 2, 64)), "k_new"),
    ("streaming_shift_append", ValueError, "v_new a row shorter than k_new", swap(v_new=lambda: z(1, 1, 64)), "v_new"),
    ("streaming_shift_append", ValueError, "3 rows for n_new = 2",
     swap(k_new=lambda: z(3, 1, 64), v_new=lambda: z(3, 1, 64)), "n_new"),
    ("streaming_rotate", ValueError, "rot_cache of another shape", swap(rot_cache=lambda: z(1, 2, 128, 1, 64))),
    ("streaming_rotate", ValueError, "rot_cache on the host", on_host("rot_cache")),
    # activation rows
    *[(c, ValueError, "x of rank 3", swap(x=lambda: z(1, 2, 128)))
      for c in ("linear", "linear_add_rmsnorm", "fused_split_linear", "fused_split_linear_add_rmsnorm", "linear_block",
                "linear_block_add_rmsnorm", "fused_linear", "fused_qkv")],
    *[(c, ValueError, "x with an inner stride", swap(x=lambda: z(2, 256)[:, ::2]))
      for c in ("linear", "linear_add_rmsnorm", "fused_split_linear", "linear_block", "fused_linear")],
    *[(c, ValueError, "x on the host", on_host("x"))
      for c in ("linear", "linear_add_rmsnorm", "fused_split_linear", "linear_block", "fused_linear", "fused_qkv")],
    *[(c, TypeError, "x float32", as_dtype("x", F32))
      for c in ("linear", "linear_add_rmsnorm", "fused_split_linear", "fused_split_linear_add_rmsnorm")],
    *[(c, ValueError, "x float32", as_dtype("x", F32)) for c in ("linear_block", "fused_linear", "fused_qkv")],
    # the linear weight
    *[(c, ValueError, "weight packed for K = 256", K256)
      for c in ("linear", "linear_add_rmsnorm", "fused_split_linear", "fused_split_linear_add_rmsnorm", "linear_block",
                "linear_block_add_rmsnorm", "fused_linear")],
    ("linear", ValueError, "row-major weight of K = 256", swap(weight=lambda: z(32, 256))),
    ("linear_add_rmsnorm", ValueError, "row-major weight of K = 256", swap(weight=lambda: z(32, 256))),
    ("linear", ValueError, "weight not contiguous", swap(weight=lambda: z(128, 32).t())),
    ("linear", ValueError, "weight on the host", on_host("weight")),
    ("linear", TypeError, "weight float32", as_dtype("weight", F32)),
    ("linear_add_rmsnorm", TypeError, "weight float32", as_dtype("weight", F32)),
    ("linear_int8", ValueError, "int8 without scales", swap(scales=None)),
    ("linear_int8", ValueError, "scales of 16", swap(scales=lambda: z(16))),
    ("linear_int8", TypeError, "scales float32", swap(scales=lambda: z(32, dtype=F32))),
    ("linear_add_rmsnorm_int8", ValueError, "int8 without scales", swap(scales=None)),
    ("linear_pro", TypeError, "deferred norm over int8", swap(weight=lambda: packed(64, 128, True, I8), scales=z(64))),
    *[(c, ValueError, "packed for SwiGLU", swap(weight=lambda: packed(32, 128, True)))
      for c in ("linear", "linear_add_rmsnorm", "fused_split_linear", "fused_split_linear_add_rmsnorm", "linear_block",
                "linear_block_add_rmsnorm", "fused_linear", "fused_qkv")],
    ("linear_packed_swiglu", ValueError, "packed for no epilogue", swap(weight=lambda: packed(64, 128))),
    *[(c, TypeError, "int8 streaming weight", swap(weight=lambda: packed(32, 128, dtype=I8)))
      for c in ("fused_split_linear", "fused_split_linear_add_rmsnorm", "linear_block", "linear_block_add_rmsnorm",
                "fused_linear")],
    *[(c, TypeError, "row-major weight", swap(weight=lambda: z(32, 128)))
      for c in ("fused_split_linear", "linear_block", "linear_block_add_rmsnorm", "fused_linear")],
    ("fused_qkv", ValueError, "weight rows are not (H + 2 KH) D", swap(H=3)),
    ("fused_qkv", ValueError, "ragged requests", swap(x=lambda: z(3, 128), rows_per_req=2)),
    # per-column vectors
    *[(c, ValueError, "bias of 16", swap(bias=lambda: z(16)))
      for c in ("linear", "linear_add_rmsnorm", "fused_split_linear", "fused_split_linear_add_rmsnorm", "linear_block",
                "linear_block_add_rmsnorm", "fused_linear", "fused_qkv")],
    *[(c, TypeError, "bias float32", swap(bias=lambda: z(32, dtype=F32)))
      for c in ("linear", "linear_add_rmsnorm", "fused_split_linear", "fused_split_linear_add_rmsnorm", "fused_linear")],
    *[(c, ValueError, "bias float32", swap(bias=lambda: z(32, dtype=F32)))
      for c in ("linear_block", "linear_block_add_rmsnorm")],
    *[(c, ValueError, "bias strided", swap(bias=lambda: z(64)[::2]))
      for c in ("linear", "fused_split_linear", "linear_block", "fused_linear")],
    *[(c, ValueError, "bias on the host", on_host("bias"))
      for c in ("linear", "linear_add_rmsnorm", "fused_split_linear", "linear_block", "fused_linear", "fused_qkv")],
    *[(c, ValueError, "bias 2 bytes off a 16-byte boundary", swap(bias=lambda: z(33)[1:]))
      for c in ("linear_block", "linear_block_add_rmsnorm")],
    *[(c, ValueError, "norm weight of 16", swap(norm_weight=lambda: z(16)))
      for c in ("linear_add_rmsnorm", "fused_split_linear_add_rmsnorm", "linear_block_add_rmsnorm")],
    *[(c, TypeError, "norm weight float32", swap(norm_weight=lambda: z(32, dtype=F32)))
      for c in ("linear_add_rmsnorm", "fused_split_linear_add_rmsnorm", "linear_block_add_rmsnorm")],
    *[(c, ValueError, "norm weight on the host", on_host("norm_weight"))
      for c in ("linear_add_rmsnorm", "fused_split_linear_add_rmsnorm", "linear_block_add_rmsnorm")],
    ("rmsnorm", ValueError, "float32 weight of 64 on rows of 128", swap(weight=lambda: z(64, dtype=F32))),
    ("add_rmsnorm", ValueError, "float32 weight of 64 on rows of 128", swap(weight=lambda: z(64, dtype=F32))),
    ("rmsnorm", TypeError, "weight float32", as_dtype("weight", F32)),
    ("add_rmsnorm", TypeError, "weight float32", as_dtype("weight", F32)),
    ("rmsnorm", ValueError, "weight of 64", swap(weight=lambda: z(64))),
    ("add_rmsnorm", ValueError, "weight of 64", swap(weight=lambda: z(64))),
    ("rmsnorm", TypeError, "x float32", as_dtype("x", F32)),
    ("rmsnorm", ValueError, "x on the host", on_host("x")),
    ("rmsnorm", ValueError, "weight on the host", on_host("weight")),
    ("add_rmsnorm", ValueError, "r of another size", swap(r=lambda: z(2, 64))),
    ("add_rmsnorm", ValueError, "r on the host", on_host("r")),
    # 2-D outputs and the residual
    *[(c, ValueError, "out of another shape", swap(out=lambda: z(2, 16)))
      for c in ("linear_out", "linear_block_swiglu_out", "fused_linear_out")],
    *[(c, ValueError, "out with an inner stride", swap(out=lambda: z(2, 64)[:, ::2]))
      for c in ("linear_out", "linear_block_swiglu_out", "fused_linear_out")],
    *[(c, ValueError, "out on the host", on_host("out"))
      for c in ("linear_out", "linear_block_swiglu_out", "fused_linear_out")],
    ("linear_out", TypeError, "out float32", swap(out=lambda: z(2, 32, dtype=F32))),
    ("linear_block_swiglu_out", ValueError, "out float32", swap(out=lambda: z(2, 32, dtype=F32))),
    ("fused_linear_out", ValueError, "out float32", swap(out=lambda: z(2, 32, dtype=F32))),
    *[(c, ValueError, "resid of another shape", swap(resid=lambda: z(2, 64)))
      for c in ("linear_add_rmsnorm", "fused_split_linear_add_rmsnorm", "linear_block_add_rmsnorm",
                "fused_linear_resid_ssq")],
    *[(c, ValueError, "resid with an inner stride", swap(resid=lambda: z(2, 64)[:, ::2]))
      for c in ("linear_add_rmsnorm", "fused_split_linear_add_rmsnorm", "linear_block_add_rmsnorm",
                "fused_linear_resid_ssq")],
    *[(c, ValueError, "resid on the host", on_host("resid"))
      for c in ("linear_add_rmsnorm", "fused_split_linear_add_rmsnorm", "linear_block_add_rmsnorm",
                "fused_linear_resid_ssq")],
    *[(c, TypeError, "resid float32", as_dtype("resid", F32))
      for c in ("linear_add_rmsnorm", "fused_split_linear_add_rmsnorm", "linear_block_add_rmsnorm")],
    ("fused_linear_resid_ssq", ValueError, "resid float32", as_dtype("resid", F32)),
    ("fused_linear", ValueError, "want_ssq without a residual", swap(want_ssq=True)),
    # workspace
    *[(c, ValueError, "no workspace", swap(workspace=None))
      for c in ("linear", "linear_add_rmsnorm", "fused_split_linear", "fused_split_linear_add_rmsnorm", "linear_block",
                "linear_block_add_rmsnorm")],
    # deferred norm
    *[(c, ValueError, "x is not the h of the sums", swap(x=lambda: z(2, 128)))
      for c in ("linear_pro", "fused_linear_swiglu_pro", "fused_qkv_two_caches_pro")],
    *[(c, ValueError, "ssq of 2 tiles for K = 128",
       lambda o: {"pro": ops.DeferredNorm(o["x"], z(2, 2, dtype=F32), z(128), 1e-5)})
      for c in ("linear_pro", "fused_linear_swiglu_pro", "fused_qkv_two_caches_pro")],
    *[(c, ValueError, "ssq bf16", lambda o: {"pro": ops.DeferredNorm(o["x"], z(2, 4), z(128), 1e-5)})
      for c in ("linear_pro", "fused_linear_swiglu_pro")],
    *[(c, ValueError, "norm weight of 64 for K = 128",
       lambda o: {"pro": ops.DeferredNorm(o["x"], z(2, 4, dtype=F32), z(64), 1e-5)})
      for c in ("linear_pro", "fused_linear_swiglu_pro")],
    *[(c, ValueError, "norm weight float32",
       lambda o: {"pro": ops.DeferredNorm(o["x"], z(2, 4, dtype=F32), z(128, dtype=F32), 1e-5)})
      for c in ("linear_pro", "fused_linear_swiglu_pro")],
    ("fused_linear", ValueError, "deferred norm without SwiGLU", lambda o: {"pro": pro_of(o["x"])}),
    ("linear_pro", ValueError, "K = 144 is not whole 32-column tiles",
     lambda o: (lambda x: dict(x=x, weight=packed(64, 144, True),
                               pro=ops.DeferredNorm(x, z(2, 4, dtype=F32), z(144), 1e-5)))(z(2, 144)), "32"),
    # the small ops
    ("silu_mul", ValueError, "b of another shape", swap(b=lambda: z(2, 32))),
    ("silu_mul", ValueError, "b with an inner stride", swap(b=lambda: z(2, 128)[:, ::2])),
    ("silu_mul", ValueError, "a of rank 3", swap(a=lambda: z(1, 2, 64))),
    ("silu_mul", TypeError, "b float32", as_dtype("b", F32)),
    ("silu_mul", ValueError, "a on the host", on_host("a")),
    ("silu_mul", ValueError, "b on the host", on_host("b")),
    *[(c, ValueError, "logits with an inner stride", swap(logits=lambda: z(2, 128)[:, ::2]))
      for c in ("argmax", "argmax_tp_slots")],
    *[(c, TypeError, "logits float32", as_dtype("logits", F32)) for c in ("argmax", "argmax_tp_slots")],
    *[(c, ValueError, "logits on the host", on_host("logits")) for c in ("argmax", "argmax_tp_slots")],
    ("argmax_tp_slots", ValueError, "rank outside the world", swap(tp_rank=2)),
    ("tp_argmax_merge", TypeError, "idx int32", as_dtype("idx", I32)),
    ("tp_argmax_merge", TypeError, "vals float32", as_dtype("vals", F32)),
    ("tp_argmax_merge", ValueError, "shapes differ", swap(idx=lambda: i64(2, 3))),
    ("tp_argmax_merge", ValueError, "vals on the host", on_host("vals")),
    ("tp_argmax_merge", ValueError, "idx on the host", on_host("idx")),
    # accept_rollback: every tensor whose pointer is passed
    *[("accept_rollback", ValueError, f"{n} on the host", on_host(n)) for n in ACCEPT_TENSORS],
    *[("accept_rollback", TypeError, f"{n} of the other integer width",
       lambda o, n=n: {n: gpu(host(o[n]).to(I32 if o[n].dtype == I64 else I64))}, n) for n in ACCEPT_TENSORS],
    *[("accept_rollback", ValueError, f"{n} a row short", lambda o, n=n: {n: gpu(host(o[n])[:1].clone())}, n)
      for n in ACCEPT_TENSORS[1:]],
    ("accept_rollback", ValueError, "tokens_buffer a row short: B is its rows, so the next tensor is too long",
     swap(tokens_buffer=lambda: i64(1, 2)), "target_tokens"),
    ("accept_rollback", ValueError, "tokens_buffer is not gamma + 1 wide", swap(gamma=2), "tokens_buffer"),
    # sampling
    ("sample_rows", ValueError, "logits float32", as_dtype("logits", F32)),
    ("sample_rows", ValueError, "logits on the host", on_host("logits")),
    ("sample_rows", ValueError, "temperature 0", swap(temperature=0.0), "temperature"),
    ("sample_rows", ValueError, "top_p above 1", swap(top_p=1.5), "temperature"),
    ("sample_rows", ValueError, "rows are not B x n", swap(logits=lambda: z(3, 64), n=2)),
    ("sample_rows", ValueError, "counters int64", as_dtype("counters", I64)),
    ("sample_rows", ValueError, "counters of 2", swap(counters=lambda: i32(2))),
    ("sample_rows", ValueError, "counters on the host", on_host("counters")),
    ("sample_rows", ValueError, "a ring without stats", swap(ring=lambda: z(2, 1, 64)), "go together"),
    ("sample_rows_ring", ValueError, "ring of another vocabulary", swap(ring=lambda: z(2, 1, 32)), "ring"),
    ("sample_rows_ring", ValueError, "ring float32", as_dtype("ring", F32), "ring"),
    ("sample_rows_ring", ValueError, "empty ring", swap(ring=lambda: z(2, 0, 64)), "ring"),
    ("sample_rows_ring", ValueError, "ring on the host", on_host("ring")),
    ("sample_rows_ring", ValueError, "ring_stats of another shape", swap(ring_stats=lambda: i64(2, 1, 1))),
    ("sample_rows_ring", ValueError, "ring_stats int32", as_dtype("ring_stats", I32)),
    ("sample_rows_ring", ValueError, "ring_stats on the host", on_host("ring_stats")),
    ("sample_rows_sel_out", ValueError, "row_sel int32", as_dtype("row_sel", I32)),
    ("sample_rows_sel_out", ValueError, "row_sel of 2", swap(row_sel=lambda: i64(2))),
    ("sample_rows_sel_out", ValueError, "row_sel on the host", on_host("row_sel")),
    ("sample_rows_sel_out", ValueError, "out of another shape", swap(out=lambda: i64(2, 1))),
    ("sample_rows_sel_out", ValueError, "out int32", as_dtype("out", I32)),
    ("sample_rows_sel_out", ValueError, "out on the host", on_host("out")),
    ("spec_verify_sample", ValueError, "tokens_buffer of rank 1", swap(tokens_buffer=lambda: i64(4))),
    ("spec_verify_sample", ValueError, "tokens_buffer int32", as_dtype("tokens_buffer", I32)),
    ("spec_verify_sample", ValueError, "tokens_buffer on the host", on_host("tokens_buffer")),
    ("spec_verify_sample", ValueError, "logits of other rows", swap(logits=lambda: z(6, 64))),
    ("spec_verify_sample", ValueError, "ring of another vocabulary", swap(ring=lambda: z(2, 1, 32)), "vocabular"),
    ("spec_verify_sample", ValueError, "ring on the host", on_host("ring")),
    ("spec_verify_sample", ValueError, "target_stats of other rows", swap(target_stats=lambda: i64(2, 2))),
    ("spec_verify_sample", ValueError, "ring_stats of another shape", swap(ring_stats=lambda: i64(2, 2, 2))),
    ("spec_verify_sample", ValueError, "target_stats on the host", on_host("target_stats")),
    ("spec_verify_sample_view_out", ValueError, "out of another shape", swap(out=lambda: i64(2, 3))),
    ("spec_verify_sample_view_out", ValueError, "out on the host", on_host("out")),
    ("shard_max", ValueError, "columns past the vocabulary", swap(vocab_offset=40), "inside the vocabulary"),
    ("shard_max", ValueError, "negative offset", swap(vocab_offset=-1), "inside the vocabulary"),
    ("shard_max", ValueError, "red of 3", swap(red=lambda: i64(3)), "red"),
    ("shard_max", ValueError, "red int32", as_dtype("red", I32), "red"),
    ("shard_max", ValueError, "red on the host", on_host("red")),
    ("shard_max", ValueError, "a ring without tokens_buffer", swap(ring=lambda: z(2, 1, 64)), "ring"),
    ("shard_max_probe", ValueError, "a probe without a ring", swap(ring=None), "ring"),
    ("shard_max_probe", ValueError, "ring columns past its width", swap(ring=lambda: z(2, 1, 32)), "exceed"),
    ("shard_max_probe", ValueError, "ring of another batch", swap(ring=lambda: z(3, 1, 64)), "ring"),
    ("shard_max_probe", ValueError, "ring on the host", on_host("ring")),
    ("shard_max_probe", ValueError, "tokens_buffer int32", as_dtype("tokens_buffer", I32)),
    ("shard_max_probe", ValueError, "tokens_buffer on the host", on_host("tokens_buffer")),
    ("shard_max_probe", ValueError, "red without the probes", swap(red=lambda: i64(4)), "red"),
    ("shard_hist", ValueError, "temperature 0", swap(temperature=0.0), "temperature"),
    ("shard_hist", ValueError, "red shorter than the rows", swap(red=lambda: i64(1)), "red"),
    ("shard_hist", ValueError, "red on the host", on_host("red")),
    ("shard_hist", ValueError, "hist_out of 128 bins", swap(hist_out=lambda: i64(2, 128))),
    ("shard_hist", ValueError, "hist_out on the host", on_host("hist_out")),
    ("shard_hist_low", ValueError, "a low-byte phase at top_p = 1", swap(top_p=1.0), "low-byte"),
    ("shard_hist_low", ValueError, "hist_hi int32", as_dtype("hist_hi", I32)),
    ("shard_draw", ValueError, "a ring without stats", swap(ring=lambda: z(2, 1, 32)), "go together"),
    ("shard_draw", ValueError, "no low-byte histogram at top_p < 1", swap(hist_lo=None), "low-byte"),
    ("shard_draw_ring_top1", ValueError, "a low-byte histogram at top_p = 1", swap(hist_lo=lambda: i64(2, 256)),
     "low-byte"),
    ("shard_draw_ring_top1", ValueError, "ring as wide as the vocabulary", swap(ring=lambda: z(2, 1, 64)), "ring"),
    ("shard_draw", ValueError, "cand of another shape", swap(cand=lambda: i64(2, 1)), "cand"),
    ("shard_draw", ValueError, "cand on the host", on_host("cand")),
    ("shard_draw", ValueError, "columns past the vocabulary", swap(vocab_total=48), "inside the vocabulary"),
    ("shard_draw", ValueError, "counters on the host", on_host("counters")),
    ("shard_finish", ValueError, "cand of rank 2", swap(cand=lambda: i64(2, 1)), "cand"),
    ("shard_finish", ValueError, "cand int32", as_dtype("cand", I32), "cand"),
    ("shard_finish", ValueError, "cand on the host", on_host("cand")),
    ("shard_finish_out", ValueError, "out of another shape", swap(out=lambda: i64(2, 1))),
    ("spec_verify_shard", ValueError, "columns past the vocabulary", swap(vocab_offset=33), "inside the vocabulary"),
    ("spec_verify_shard", ValueError, "cand of 2 words", swap(cand=lambda: i64(2, 2)), "cand"),
    ("spec_verify_shard", ValueError, "logits of other rows", swap(logits=lambda: z(6, 32))),
    ("spec_verify_shard", ValueError, "red without the probes", swap(red=lambda: i64(4)), "red"),
    ("spec_verify_shard", ValueError, "target_stats of other rows", swap(target_stats=lambda: i64(2, 2))),
    ("spec_verify_shard", ValueError, "no low-byte histogram at top_p < 1", swap(hist_lo=None), "low-byte"),
    ("spec_verify_shard", ValueError, "ring narrower than the shard", swap(ring=lambda: z(2, 1, 16)), "exceed"),
    ("spec_verify_shard", ValueError, "ring on the host", on_host("ring")),
    ("spec_verify_shard", ValueError, "tokens_buffer of one column", swap(tokens_buffer=lambda: i64(4, 1))),
    ("spec_verify_shard_finish", ValueError, "cand of another shape", swap(cand=lambda: i64(2, 2)), "cand"),
    ("spec_verify_shard_finish", ValueError, "tokens_buffer of one column", swap(tokens_buffer=lambda: i64(2, 1))),
    ("spec_verify_shard_finish", ValueError, "cand on the host", on_host("cand")),
    ("spec_verify_shard_finish", ValueError, "counters int64", as_dtype("counters", I64)),
]


@pytest.mark.parametrize("row", REFUSED, ids=[f"{r[0]}-{r[2].replace(' ', '_')}" for r in REFUSED])
def test_refused(rec, row):
    case, exc, _, bad = row[:4]
    with pytest.raises(exc, match=row[4] if len(row) > 4 else getattr(bad, "match", None)):
        run(rec, case, bad)
    assert rec.launches() == []


def test_refused_rows_are_distinct():
    ids = [(r[0], r[2]) for r in REFUSED]
    assert len(ids) == len(set(ids))


# ----------------------------------------------------------------------------------------- call vectors
def operands(o, ret):
    """(name, tensor) of every tensor a call was given, then of what it returned."""
    for k, v in o.items():
        if isinstance(v, torch.Tensor):
            yield k, v
        elif isinstance(v, ops.PackedWeight):
            yield k + ".data", v.data
        elif isinstance(v, ops.DeferredNorm):
            yield from ((f"{k}.{f}", getattr(v, f)) for f in ("h", "ssq", "weight"))
        elif isinstance(v, ops.RopeTable):
            yield k + ".table", v.table
        elif isinstance(v, ops.AttnWorkspace):
            yield k + ".buf", v.buf
        elif isinstance(v, tuple):
            yield from ((f"{k}[{i}]", t) for i, t in enumerate(v))
    rets = ret if isinstance(ret, tuple) else (ret,)
    yield from ((f"ret[{i}]", t) for i, t in enumerate(rets) if t is not None)


def call_vector(case, name, args, o, ret):
    """One line: the function, every scalar, and for every pointer the operand it lies in and its byte offset."""
    known = list(operands(o, ret))

    def where(ptr):
        if not ptr:
            return "null"
        for exact in (True, False):
            for n, t in known:
                off = ptr - t.data_ptr()
                extent = (sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1) * t.element_size()
                if off == 0 if exact else 0 <= off < extent:
                    return f"{n}+{off}"
        return "temporary"

    def show(a):
        if hasattr(a, "_obj"):           # byref(md_fused_linear_args)
            s = a._obj
            return "{" + ", ".join(f"{f}=" + (where(getattr(s, f)) if ty is ctypes.c_void_p else repr(getattr(s, f)))
                                   for f, ty in s._fields_) + "}"
        if a is None or isinstance(a, ctypes.c_void_p):
            return where(a.value if a is not None else None)
        return repr(a)
    return f"{case}: {name}(" + ", ".join(show(a) for a in args) + ")"


def call_vectors():
    with pytest.MonkeyPatch.context() as mp:
        rec = install(mp)
        for case in ACCEPTED:
            o, ret = run(rec, case)
            for name, args in rec.launches():
                yield call_vector(case, name, args, o, ret)


if __name__ == "__main__":
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    out.write("".join(line + "\n" for line in call_vectors()))

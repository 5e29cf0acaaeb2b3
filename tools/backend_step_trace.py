#!/usr/bin/env python3
"""What the four back-ends ask of their model, call by call (CPU; the stand-in ops of tests/cpu_ops.py and the tiny
models of the trace tests) -- the characterisation a change to Engine/backend_core.py must leave byte-identical.

Runs the first iterations of one batch of each decode loop (longspec with a SnapKV draft, compressed and
draft_budget=-1; longspec with a StreamingLLM draft; SnapKV self-speculation; StreamingLLM self-speculation; baseline)
and the `benchmark=True` programs of tests/golden/benchflag_*.json.  Per back-end call one line: the method, the token
columns, `benchmark`, `cachelen_update`, and which of the six traced attributes the call REBOUND to a new tensor
object (what Engine/graph.py and the harness can see).  Under it, one line per call into the model: the method, n,
`sample_role` / `skip_head`, the length tensor (which back-end attribute it is, by identity, and its values), the values
of the append indptr, and for every PageTable argument which back-end attribute each of its three tensors is (by
identity) and its `max_pages`.  `prefill` takes `is_last` / `ctx_len` into account only together with a draft table
(Transformer.prefill), so they are recorded only then; `stream_prefill` always shows `ctx` / `is_last` / `which`.

usage: python tools/backend_step_trace.py [OUT]         (default: stdout)
"""
import inspect
import os
import sys
import tempfile
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import cpu_ops, golden_cfg as gc  # noqa: E402

TRACED = ("cachelens", "paged_kv_last_page_len", "paged_kv_indptr", "draft_cachelens", "draft_paged_kv_last_page_len",
          "draft_paged_kv_indptr")
NAMED = TRACED + ("paged_kv_indices", "draft_paged_kv_indices", "qo_indptr")
MODEL_FNS = ("forward", "verify", "draft_forward", "prefill", "stream_prefill")
BACKEND_FNS = ("encode", "draft_encode", "inference", "verify", "speculate")
ITERS = 8           # iterations per loop: enough for a two-token step after an all-accept iteration (asserted)


def _name_of(be, t):
    for name in NAMED:
        if getattr(be, name, None) is t:
            return name
    return "?"


def _table(be, tab):
    return (f"({_name_of(be, tab.indices)},{_name_of(be, tab.indptr)},{_name_of(be, tab.last_page_len)};"
            f"max_pages={tab.max_pages})")


def instrument(be, tag, out):
    """Wrap the model methods and the public step methods of back-end `be`; lines go to the list `out`."""
    from magicdec_amd.Engine.model_core import PageTable
    model, calls = be.model, []

    def wrap_model(name):
        orig = getattr(model, name)
        sig = inspect.signature(orig)

        def call(*a, **kw):
            args = sig.bind(*a, **kw)
            args.apply_defaults()
            args = args.arguments
            line = f"    {name} n={args['idx'].shape[1]} role={model.sample_role} skip_head={model.skip_head}"
            if name == "stream_prefill":
                line += f" ctx={args['ctx']} is_last={args['is_last']} which={args['which']}"
            else:
                pos = args["input_pos"]
                line += f" lens={_name_of(be, pos)}{pos.tolist()}"
            if name == "prefill":
                with_draft = args["draft_tab"] is not None
                line += (f" is_last={args['is_last']} ctx_len={args['ctx_len']}" if with_draft else
                         " is_last=- ctx_len=-")
            line += f" qo={args['kv_append_indptr'].tolist()}"
            for k, v in args.items():
                if isinstance(v, PageTable):
                    line += f" {k}={_table(be, v)}"
            calls.append(line)
            return orig(*a, **kw)
        setattr(model, name, call)

    def wrap_backend(name):
        orig = getattr(be, name)

        def call(*a, **kw):
            ids = a[0] if a else kw["input_ids"]
            before = {k: getattr(be, k, None) for k in TRACED}
            res = orig(*a, **kw)
            rebound = [k for k in TRACED if getattr(be, k, None) is not before[k]]
            cu = kw.get("cachelen_update")
            out.append(f"  {tag}.{name} n={ids.shape[1]} benchmark={bool(kw.get('benchmark', False))} "
                       f"cachelen_update={cu.flatten().tolist() if cu is not None else None} "
                       f"rebound=[{','.join(rebound)}]")
            out.extend(calls)
            calls.clear()
            return res
        setattr(be, name, call)

    for name in MODEL_FNS:
        wrap_model(name)
    for name in BACKEND_FNS:
        if hasattr(be, name):
            wrap_backend(name)
    return be


def _make(ckpt, module, cls, model, ctor, caches):
    import importlib
    e = getattr(importlib.import_module("magicdec_amd." + module), cls)(dtype=torch.bfloat16, device="cpu", **ctor)
    e.load_model(ckpt / model / "model.pth", use_tp=False)
    e.setup_caches(max_batch_size=gc.B, **caches)
    return e


def _spec_loop(iteration, st, two_token_step):
    terminal, nd, doubles = False, False, 0
    for _ in range(ITERS):
        if terminal:
            break
        doubles += int(nd)
        terminal, nd = iteration(st, nd)
    assert doubles > 0 or not two_token_step, "no two-token step in the traced iterations"


def loops(ckpt, out):
    from magicdec_amd import harness
    ids = gc.synthetic_batches()[0]
    full = dict(max_seq_length=gc.MAX_LEN)
    snap = dict(max_seq_length=gc.MAX_LEN, draft_budget=gc.BUDGET)
    tgt = lambda: _make(ckpt, "Engine.SnapKV.backend", "LMBackend", "tinytgt", dict(dec_len=gc.GAMMA + 1), full)
    G, args = gc.GAMMA, (gc.EOT_1, gc.EOT_2, gc.S + 80)

    def longspec(title, drf, topk, two_token_step):
        out.append(f"== {title}")
        cpu_ops.TOPK_REPLAY.update(table=topk, pos=0)
        T, D = instrument(tgt(), "T", out), instrument(drf, "D", out)
        st = harness.new_state(gc.B, G, gc.MAX_LEN + 1, "cpu", ids)
        st.tokens_buffer[:, :1] = T.encode(input_ids=ids)[:, -1:]
        D.encode(input_ids=ids)
        _spec_loop(lambda st, nd: harness.longspec_iteration(T, D, st, G, *args, nd), st, two_token_step)

    def selfspec(title, eng, topk, streaming):
        out.append(f"== {title}")
        cpu_ops.TOPK_REPLAY.update(table=topk, pos=0)
        T = instrument(eng, "T", out)
        st = harness.new_state(gc.B, G, gc.MAX_LEN + 1, "cpu", ids)
        st.tokens_buffer[:, :1] = T.encode(input_ids=ids)[:, -1:]
        if streaming:
            T.draft_encode(input_ids=ids)
        _spec_loop(lambda st, nd: harness.selfspec_iteration(T, st, G, *args, nd, streaming), st, streaming)

    longspec("longspec, SnapKV draft, draft_budget=129",
             _make(ckpt, "Engine.SnapKV.backend_draft", "LMBackend_Draft", "tinytgt", dict(draft_budget=gc.BUDGET), snap),
             gc.load_json("run_longspec_snapkv.json")["snapkv_topk"], True)
    # (the target's weights as the draft, unlike run_longspec_snapkv_fullkv.json: the two-token step of this branch runs)
    longspec("longspec, SnapKV draft, draft_budget=-1 (full KV)",
             _make(ckpt, "Engine.SnapKV.backend_draft", "LMBackend_Draft", "tinytgt", dict(draft_budget=-1),
                   dict(max_seq_length=gc.MAX_LEN, draft_budget=-1)), None, True)
    longspec("longspec, StreamingLLM draft, draft_budget=129",
             _make(ckpt, "Engine.StreamingLLM.backend_draft", "LMBackend_Draft", "tinytgt", {},
                   dict(draft_budget=gc.BUDGET)), None, True)
    selfspec("SnapKV self-speculation, draft_budget=129",
             _make(ckpt, "Engine.SnapKV.backend", "LMBackend", "tinytgt", dict(dec_len=G + 1, draft_dec_len=1), snap),
             gc.load_json("run_selfspec_snapkv.json")["snapkv_topk"], False)
    selfspec("StreamingLLM self-speculation, draft_budget=129",
             _make(ckpt, "Engine.StreamingLLM.backend", "LMBackend", "tinytgt", dict(dec_len=G + 1), snap), None, True)
    out.append("== baseline")
    cpu_ops.TOPK_REPLAY.update(table=None, pos=0)
    base = instrument(_make(ckpt, "Engine.SnapKV.backend", "LMBackend", "tinytgt", {}, full), "T", out)
    harness.run_baseline_batch(base, ids, gc.S + ITERS, gc.EOT_1, gc.EOT_2)


def benchflag_programs(ckpt, out):
    """The fixed programs of normal and benchmark=True calls the benchflag fixtures were recorded with."""
    for tag in ("benchflag_snapkv_self", "benchflag_longspec_snapkv", "benchflag_longspec_stream",
                "benchflag_stream_self"):
        j = gc.load_json(f"{tag}.json")
        out.append(f"== {tag}")
        cpu_ops.TOPK_REPLAY.update(table=j["snapkv_topk"] or None, pos=0)
        engines = {key: instrument(_make(ckpt, spec["module"], spec["cls"], "tinytgt", spec["ctor"], spec["caches"]),
                                   key, out) for key, spec in j["engines"].items()}
        for i, step in enumerate(j["program"]):
            kw = dict(step["kwargs"])
            if "cachelen_update" in kw:
                kw["cachelen_update"] = torch.tensor(kw["cachelen_update"])
            getattr(engines[step["key"]], step["fn"])(gc.benchflag_inputs(step["ncols"], i), **kw)


def trace(monkeypatch=None) -> str:
    """The whole trace as text.  `monkeypatch`: pytest's, so that the stand-in ops are undone after a test."""
    from magicdec_amd.Engine import model_core
    cpu_ops.install(monkeypatch)
    saved = dict(cpu_ops.TOPK_REPLAY)
    cfg, sd = gc.tiny("tinytgt")
    missing = object()
    registered = model_core.transformer_configs.get("tinytgt", missing)
    model_core.transformer_configs["tinytgt"] = gc.config_kwargs(cfg)
    out = []
    try:
        with tempfile.TemporaryDirectory(prefix="md_step_trace_") as d, torch.no_grad():
            ckpt = Path(d)
            os.makedirs(ckpt / "tinytgt")
            torch.save(sd, ckpt / "tinytgt" / "model.pth")
            loops(ckpt, out)
            benchflag_programs(ckpt, out)
    finally:
        cpu_ops.TOPK_REPLAY.update(saved)
        if registered is missing:
            del model_core.transformer_configs["tinytgt"]
        else:
            model_core.transformer_configs["tinytgt"] = registered
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    text = trace()
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text(text)
    else:
        sys.stdout.write(text)

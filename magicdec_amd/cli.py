"""Command lines of the reference's benchmark scripts (same flags, asserts and printed lines):
tests/SnapKV/longspec_benchmark.py:16-46, tests/StreamingLLM/longspec_benchmark.py, tests/*/selfspec_benchmark.py,
tests/baseline_benchmark.py.  The loops themselves live in magicdec_amd/harness.py."""
from __future__ import annotations

import argparse
import builtins
import time
from pathlib import Path

import torch
import torch.distributed as dist
from torch.utils.data.dataloader import DataLoader

from . import harness
from .data import convert_pg19_dataset, load_tokenizer
from .Engine.utils import setup_seed


# Per-script defaults of the reference's five entry points (their argparse blocks differ: e.g. the self-speculation scripts
# default to B = 45, prefix 100000, gamma 7, budget 4097; tests/SnapKV/selfspec_benchmark.py:17-36).  Checkpoint paths are
# the one deliberate difference: "checkpoints/..." relative to the working directory instead of "/scratch/models/...".
_CKPT_8B = Path("checkpoints/meta-llama/Meta-Llama-3.1-8B/model.pth")
_CKPT_1B = Path("checkpoints/meta-llama/Llama-3.2-1B/model.pth")
_DEFAULTS = {
    "longspec": dict(model=_CKPT_1B, B=1, prefix_len=4000, max_len=64, gamma=5),
    "selfspec": dict(model=_CKPT_8B, B=45, prefix_len=100000, max_len=100096, gamma=7, draft_budget=4097),
    "baseline": dict(model=_CKPT_8B, B=16, prefix_len=8065, max_len=8192),
}


def _common(parser, script, kind=None):
    d = _DEFAULTS[script]
    parser.add_argument('--model', type=Path, default=d["model"], help='model')
    parser.add_argument('--model_name', type=str, default="meta-llama/Meta-Llama-3.1-8B", help='model name')
    parser.add_argument('--dataset', type=str, default="pg19", help='Dataset name.')
    parser.add_argument('--rank_group', nargs='+', type=int, help='Target group of ranks')
    parser.add_argument('--compile', action='store_true', help='Capture the decode steps into hipGraphs.')
    parser.add_argument('--B', type=int, default=d["B"], help='Batch size.')
    parser.add_argument('--prefix_len', type=int, default=d["prefix_len"], help='Prefix length')
    parser.add_argument('--max_len', type=int, default=d["max_len"], help='Generate length')
    parser.add_argument('--seed', type=int, default=123, help='Random seed.')
    parser.add_argument('--printoutput', action='store_true', help='Whether to print the generated text.')
    parser.add_argument('--benchmark', action='store_true', help='Per-phase timing (adds synchronisations).')
    parser.add_argument('--kv_dtype', type=str, default="bf16", choices=["bf16", "fp8"],
                        help='Storage of the full-context KV cache (fp8 = OCP e4m3fn; not in the reference).')
    parser.add_argument('--kv_layout', type=str, default=None, choices=["NHD", "HND"],
                        help='Page layout of the full-context KV cache.  Default: the Engine default '
                             '(backend_core.default_kv_layout(): HND -- the rows of one kv head contiguous inside a '
                             'page, the layout bench.py measures -- unless MAGICDEC_KV_LAYOUT says otherwise); '
                             'NHD is the layout the reference plans flashinfer with.')
    if script != "baseline":
        budget = d.get("draft_budget", -1 if kind == "SnapKV" else 1025)     # longspec: SnapKV -1, StreamingLLM 1025
        parser.add_argument('--draft_budget', type=int, default=budget, help='Draft KV budget.')
        parser.add_argument('--gamma', type=int, default=d["gamma"], help='speculation length')
        if kind == "SnapKV":
            parser.add_argument('--window_size', type=int, default=32, help='SnapKV observation window')


def longspec_parser(kind="SnapKV"):
    """The flags and defaults of tests/<kind>/longspec_benchmark.py (+ --kv_dtype / --kv_layout)."""
    parser = argparse.ArgumentParser(description='Process model configuration and partitions.')
    _common(parser, "longspec", kind)
    parser.add_argument('--target', type=Path, default=_CKPT_8B, help='target model')
    parser.add_argument('--draft_rank_group', nargs='+', type=int, help='Draft group of ranks')
    # not in the reference: every rank of --rank_group runs the WHOLE draft model (no draft-side collectives, no
    # per-iteration token broadcast; greedy drafting is deterministic, so all ranks draft the same tokens).  Needs
    # --draft_rank_group to name at least two ranks only because the reference keys `use_tp` on it (kept verbatim).
    parser.add_argument('--replicate_draft', action='store_true',
                        help='run the whole draft model on every target rank instead of sharding it over --draft_rank_group')
    return parser


def selfspec_parser(kind="SnapKV"):
    """The flags and defaults of tests/<kind>/selfspec_benchmark.py (+ --kv_dtype / --kv_layout)."""
    parser = argparse.ArgumentParser(description='Process model configuration and partitions.')
    _common(parser, "selfspec", kind)
    return parser


def baseline_parser():
    """The flags and defaults of tests/baseline_benchmark.py (+ --dataset / --benchmark / --kv_dtype / --kv_layout)."""
    parser = argparse.ArgumentParser(description='Process model configuration and partitions.')
    _common(parser, "baseline")
    return parser


def add_sampling_args(parser):
    """--temperature / --top_p / --top_k / --sampling_params of the five entry points (not in the reference's scripts,
    whose flags the *_parser() functions above reproduce exactly): temperature 0 (the default) is the greedy loop,
    unchanged; > 0 samples with the tempered top-p filter and lossless speculative sampling (Engine/sampling.py), seeded
    by --seed.  --top_k > 0 or --sampling_params selects the per-request sampler (Engine/sampling.RequestSampler)."""
    parser.add_argument('--temperature', type=float, default=0.0,
                        help='Sampling temperature; 0 = greedy decoding (default).  One rank, unless '
                             '--sharded_sampling is given.')
    parser.add_argument('--top_p', type=float, default=1.0, help='Top-p (nucleus) mass kept when sampling, in (0, 1].')
    parser.add_argument('--top_k', type=int, default=0,
                        help='Top-k filter applied before top-p when sampling; 0 = off (default).  One rank only.')
    parser.add_argument('--sampling_params', type=Path, default=None, metavar='PATH',
                        help='JSON list of exactly --B objects with optional keys temperature, top_p, top_k: the '
                             'sampling parameters of each request (a missing key takes the value of the flag; '
                             'temperature 0 = that request decodes greedily).  One rank only.')
    parser.add_argument('--sharded_sampling', action='store_true',
                        help='allow --temperature > 0 with several ranks in --rank_group: the vocab-sharded sampler '
                             '(Engine/sampling.ShardedSampler; same tokens as one GPU).  Opt-in: validated with ranks '
                             'emulated on one GPU only, never across physical GPUs.')
    return parser


def parse_entry_args(parser, argv=None):
    """Parse an entry point's command line (the reference's flags + --temperature / --top_p) and validate the sampling
    flags before anything is loaded."""
    args = add_sampling_args(parser).parse_args(argv)
    if not args.temperature >= 0:
        parser.error(f"--temperature must be >= 0, got {args.temperature}")
    if not 0 < args.top_p <= 1:
        parser.error(f"--top_p must be in (0, 1], got {args.top_p}")
    if not args.top_k >= 0:
        parser.error(f"--top_k must be >= 0 (0 = off), got {args.top_k}")
    several = args.rank_group is not None and len(args.rank_group) > 1
    if (args.top_k > 0 or args.sampling_params is not None) and several:
        parser.error("--top_k / --sampling_params support one rank only (TP = 1): the vocab-sharded sampler takes one "
                     "(temperature, top_p) per run and has no top-k (no count histogram through its collectives)")
    args.request_params = None
    if args.sampling_params is not None:
        try:
            args.request_params = load_sampling_params(args.sampling_params, args.B, args.temperature, args.top_p,
                                                       args.top_k)
        except (OSError, ValueError) as e:
            parser.error(f"--sampling_params {args.sampling_params}: {e}")
    if args.temperature > 0 and several and not args.sharded_sampling:
        parser.error("--temperature > 0 supports one rank only (TP = 1): the vocab-sharded sampler needs cross-rank "
                     "max / Z / histogram reductions and is opt-in (--sharded_sampling)")
    draft_ranks = getattr(args, "draft_rank_group", None)
    if (args.sharded_sampling and args.temperature > 0 and several and draft_ranks is not None
            and not getattr(args, "replicate_draft", False) and len(draft_ranks) != len(args.rank_group)):
        parser.error(f"--sharded_sampling needs the draft on every target rank: --draft_rank_group has {len(draft_ranks)} "
                     f"ranks, --rank_group {len(args.rank_group)}.  With the draft sharded over a sub-group, the other "
                     "ranks hold no draft ring to verify against; give --draft_rank_group as many ranks as --rank_group, "
                     "or --replicate_draft")
    return args


def load_sampling_params(path, B, temperature, top_p, top_k):
    """--sampling_params: a JSON list of exactly B objects with optional keys temperature / top_p / top_k (a missing key
    takes the flag's value) -> (temperatures, top_ps, top_ks), range-checked.  ValueError names what is wrong."""
    import json
    with open(path) as f:
        try:
            rows = json.load(f)
        except json.JSONDecodeError as e:
            raise ValueError(f"not JSON ({e})") from None
    if not isinstance(rows, list) or len(rows) != B:
        raise ValueError(f"need a list of exactly B = {B} objects, got "
                         f"{len(rows) if isinstance(rows, list) else type(rows).__name__}")
    known = ("temperature", "top_p", "top_k")
    out = ([], [], [])
    for i, row in enumerate(rows):
        if not isinstance(row, dict) or set(row) - set(known):
            raise ValueError(f"entry {i} must be an object with keys among {list(known)}, got {row!r}")
        t, p, k = row.get("temperature", temperature), row.get("top_p", top_p), row.get("top_k", top_k)
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not t >= 0:
            raise ValueError(f"entry {i}: temperature must be >= 0, got {t!r}")
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0 < p <= 1:
            raise ValueError(f"entry {i}: top_p must be in (0, 1], got {p!r}")
        if isinstance(k, bool) or not isinstance(k, int) or k < 0:
            raise ValueError(f"entry {i}: top_k must be an integer >= 0, got {k!r}")
        for lst, v in zip(out, (float(t), float(p), k)):
            lst.append(v)
    return out


def _sampler(args, engine, gamma, device):
    """The run's Sampler (None for greedy decoding).  --top_k > 0 or --sampling_params: a RequestSampler."""
    params = getattr(args, "request_params", None)
    if getattr(args, "top_k", 0) > 0 or params is not None:
        from .Engine.sampling import RequestSampler
        t, p, k = params if params is not None else (args.temperature, args.top_p, args.top_k)
        return RequestSampler(t, p, k, args.seed, args.B, gamma, engine.model.output.weight.shape[0], device)
    if args.temperature == 0:
        return None
    from .Engine.sampling import Sampler, ShardedSampler
    width = engine.model.output.weight.shape[0]
    group = getattr(engine.model, "process_group", None)
    if group is not None and getattr(args, "sharded_sampling", False):
        return ShardedSampler(args.temperature, args.top_p, args.seed, args.B, gamma, width, device, group,
                              replicate_draft=bool(getattr(args, "replicate_draft", False)))
    return Sampler(args.temperature, args.top_p, args.seed, args.B, gamma, width, device)


def _eot(tokenizer):
    eot_1 = tokenizer.eos_token_id
    eot_2 = tokenizer.unk_token_id if tokenizer.unk_token_id is not None else tokenizer.encode("<|eot_id|>")[-1]
    return eot_1, eot_2


def _avg_len(num_gen_tokens, target_steps, batch_size):
    """"avg generate len per sentence" exactly as the reference prints it: its token counter is a 0-d int64 tensor, so
    the two divisions happen in float32 (tests/SnapKV/longspec_benchmark.py:307 prints 2.6111111640930176, not
    2.611111111111111)."""
    return (torch.tensor(num_gen_tokens) / target_steps / batch_size).item()


def _device():
    return 'cuda' if torch.cuda.is_available() else 'cpu'


def _dataset(args, tokenizer, vocab):
    if args.dataset != "pg19":
        raise ValueError(f"Unknown dataset {args.dataset}")
    return convert_pg19_dataset(tokenizer=tokenizer, seq_len=args.prefix_len, vocab_size=vocab,
                                num_sequences=10 * args.B)


def _setup(args, longspec=False):
    """What every entry point does first: the device, the process groups under tensor parallelism, prints on the first
    target rank only, the seed.  longspec: those two scripts key tensor parallelism on the size of
    --draft_rank_group and get a draft sub-group as well (tests/SnapKV/longspec_benchmark.py:60-66); the others key it
    on --rank_group.  Returns (device, use_tp, rank, global_group, draft_group, print_)."""
    DEVICE = _device()
    use_tp = len(args.draft_rank_group if longspec else args.rank_group) > 1
    rank, global_group, draft_group = 0, None, None
    print_ = builtins.print
    if use_tp:
        from .Engine.tp import init_dist
        if longspec:
            rank, global_group, draft_group = init_dist(args.draft_rank_group)
        else:
            rank, global_group = init_dist()
        if rank != args.rank_group[0]:
            print_ = lambda *a, **k: None
        DEVICE = f"cuda:{rank}" if torch.cuda.is_available() else "cpu"
    setup_seed(args.seed)
    print_(f"Using device={DEVICE}")
    return DEVICE, use_tp, rank, global_group, draft_group, print_


def _data(args, engine, print_):
    """Tokenizer, EOT ids and the evaluation batches.  Returns (tokenizer, eot_1, eot_2, dataloader, num_eval_steps)."""
    tokenizer = load_tokenizer(args.model_name)
    eot_1, eot_2 = _eot(tokenizer)
    print_(f"eot_1: {eot_1}, eot_2: {eot_2}")
    dataset = _dataset(args, tokenizer, engine.model.tok_embeddings.weight.shape[0])
    dataloader = DataLoader(dataset, batch_size=args.B, shuffle=False, drop_last=True)
    return tokenizer, eot_1, eot_2, dataloader, min(10, len(dataloader))


def _evaluate(args, run_batch, tokenizer, dataloader, num_eval_steps, DEVICE, use_tp, print_, avg_latency=False):
    """The evaluation loop of the four speculative scripts (tests/SnapKV/longspec_benchmark.py:131-319 and its three
    twins): run_batch(input_ids, timers) -> (state, seconds) per batch, the report lines, the totals reset after each
    of the first five batches.  avg_latency: only tests/SnapKV/longspec_benchmark.py:305 prints the latency; its
    StreamingLLM twin (:302) and the self-speculation scripts do not."""
    BATCH_SIZE = args.B
    total_time, num_gen_tokens, target_steps = 0.0, 0, 0
    timers = harness.PhaseTimers(DEVICE) if args.benchmark else None
    for step, batch in enumerate(dataloader):
        if step >= num_eval_steps:
            break
        input_ids = batch[0].to(DEVICE)
        st, dt = run_batch(input_ids, timers)
        total_time += dt
        target_steps += st.iters
        num_gen_tokens += int(st.num_nodes.sum() - (input_ids.shape[1] + 1) * BATCH_SIZE)
        if args.printoutput:
            for i in range(BATCH_SIZE):
                print_("Sequence ", i)
                print_(tokenizer.decode(st.output[i, args.prefix_len:st.num_nodes[i]]))
        if avg_latency:
            print_("total time :{:.5f}s, time per iter :{:.5f}s, decoding step: {}, large model step: {}, avg latency: {}".format(
                total_time, total_time / target_steps, num_gen_tokens, target_steps, total_time / num_gen_tokens * BATCH_SIZE))
        else:
            print_("total time :{:.5f}s, time per iter :{:.5f}s, decoding step: {}, large model step: {}".format(
                total_time, total_time / target_steps, num_gen_tokens, target_steps))
        if args.benchmark:     # tests/SnapKV/longspec_benchmark.py:305-307, the same line in the other three scripts
            print_("target time :{:.5f}s, draft time :{:.5f}s, verify loop : {}, avg generate len per sentence: {}".format(
                timers.target / target_steps, timers.draft / target_steps, timers.verify_loop / target_steps,
                _avg_len(num_gen_tokens, target_steps, BATCH_SIZE)))
        if step < 5:
            total_time, num_gen_tokens, target_steps = 0.0, 0, 0
            if timers is not None:
                timers.reset()
        if use_tp:
            dist.barrier()
    print_(f"Final tokens per second :{num_gen_tokens / total_time}")
    return num_gen_tokens / total_time


def longspec_main(kind: str, argv=None):
    """kind: 'SnapKV' | 'StreamingLLM' -- tests/<kind>/longspec_benchmark.py."""
    args = parse_entry_args(longspec_parser(kind), argv)
    assert args.prefix_len < args.max_len
    assert (args.max_len + 127) // 128 == args.prefix_len // 128 + 1
    if kind == "SnapKV":
        if args.draft_budget != -1:
            assert (args.prefix_len - args.window_size) % 128 == 0
            assert (args.draft_budget - 1) % 128 == 0
    else:
        assert (args.draft_budget - 1) % 128 == 0

    DEVICE, use_tp, rank, global_group, draft_group, print_ = _setup(args, longspec=True)
    replicate = bool(getattr(args, "replicate_draft", False)) and use_tp
    draft_target_equal = len(args.draft_rank_group) == len(args.rank_group) or replicate
    MAX_LEN_TARGET, BATCH_SIZE, DTYPE = args.max_len, args.B, torch.bfloat16

    from .Engine.SnapKV.backend import LMBackend
    if kind == "SnapKV":
        from .Engine.SnapKV.backend_draft import LMBackend_Draft
    else:
        from .Engine.StreamingLLM.backend_draft import LMBackend_Draft
    engine = LMBackend(dtype=DTYPE, device=DEVICE, dec_len=args.gamma + 1)
    engine.load_model(args.target, use_tp=use_tp, rank_group=args.rank_group, group=global_group)
    if args.compile:
        engine.compile()
    engine.setup_caches(max_batch_size=BATCH_SIZE, max_seq_length=MAX_LEN_TARGET, kv_dtype=args.kv_dtype,
                        kv_layout=args.kv_layout)

    draft = None
    if (not use_tp) or replicate or rank in args.draft_rank_group:
        if kind == "SnapKV":
            draft = LMBackend_Draft(dtype=DTYPE, device=DEVICE, draft_budget=args.draft_budget)
        else:
            draft = LMBackend_Draft(dtype=DTYPE, device=DEVICE)
        draft.load_model(args.model, use_tp=use_tp and not replicate, rank_group=args.draft_rank_group,
                         group=draft_group)
        if replicate:       # every rank runs the whole draft and must choose the same kernels (Transformer._pack_weights)
            draft.model.replica_group = global_group
        if args.compile:
            draft.compile()
        if kind == "SnapKV":
            draft.setup_caches(max_batch_size=BATCH_SIZE, max_seq_length=MAX_LEN_TARGET, draft_budget=args.draft_budget)
        else:
            draft.setup_caches(max_batch_size=BATCH_SIZE, draft_budget=args.draft_budget)
    if use_tp:
        dist.barrier()

    tokenizer, eot_1, eot_2, dataloader, num_eval_steps = _data(args, engine, print_)
    bcast = (args.draft_rank_group[0], global_group) if (use_tp and not draft_target_equal) else None
    sampler = _sampler(args, engine, args.gamma, DEVICE)
    barrier = dist.barrier if use_tp else None
    return _evaluate(
        args, lambda input_ids, timers: harness.run_longspec_batch(
            engine, draft, input_ids, args.gamma, MAX_LEN_TARGET, eot_1, eot_2, bcast=bcast, barrier=barrier,
            timers=timers, sampler=sampler),
        tokenizer, dataloader, num_eval_steps, DEVICE, use_tp, print_, avg_latency=kind == "SnapKV")


def selfspec_main(kind: str, argv=None):
    """kind: 'SnapKV' | 'StreamingLLM' -- tests/<kind>/selfspec_benchmark.py."""
    args = parse_entry_args(selfspec_parser(kind), argv)
    assert args.prefix_len < args.max_len
    assert (args.max_len + 127) // 128 == args.prefix_len // 128 + 1
    assert (args.draft_budget - 1) % 128 == 0
    if kind == "SnapKV":
        assert (args.prefix_len - args.window_size) % 128 == 0
    DEVICE, use_tp, _, global_group, _, print_ = _setup(args)
    MAX_LEN_TARGET, BATCH_SIZE, DTYPE = args.max_len, args.B, torch.bfloat16
    streaming = kind == "StreamingLLM"
    if streaming:
        from .Engine.StreamingLLM.backend import LMBackend
        engine = LMBackend(dtype=DTYPE, device=DEVICE, dec_len=args.gamma + 1)
    else:
        from .Engine.SnapKV.backend import LMBackend
        engine = LMBackend(dtype=DTYPE, device=DEVICE, dec_len=args.gamma + 1, draft_dec_len=1)
    engine.load_model(args.model, use_tp=use_tp, rank_group=args.rank_group, group=global_group)
    if args.compile:
        engine.compile()
    if streaming:
        engine.setup_caches(max_batch_size=BATCH_SIZE, max_seq_length=MAX_LEN_TARGET, draft_budget=args.draft_budget,
                            kv_dtype=args.kv_dtype, kv_layout=args.kv_layout)
    else:
        engine.setup_caches(max_batch_size=BATCH_SIZE, max_seq_length=MAX_LEN_TARGET, draft_budget=args.draft_budget,
                            window_size=args.window_size, kv_dtype=args.kv_dtype, kv_layout=args.kv_layout)
    tokenizer, eot_1, eot_2, dataloader, num_eval_steps = _data(args, engine, print_)
    sampler = _sampler(args, engine, args.gamma, DEVICE)
    return _evaluate(
        args, lambda input_ids, timers: harness.run_selfspec_batch(
            engine, input_ids, args.gamma, MAX_LEN_TARGET, eot_1, eot_2, streaming, timers=timers, sampler=sampler),
        tokenizer, dataloader, num_eval_steps, DEVICE, use_tp, print_)


def baseline_main(argv=None):
    """tests/baseline_benchmark.py: the autoregressive denominator of every speedup figure."""
    args = parse_entry_args(baseline_parser(), argv)
    assert args.prefix_len < args.max_len          # tests/baseline_benchmark.py:30-31
    assert args.max_len % 128 == 0
    DEVICE, use_tp, _, global_group, _, print_ = _setup(args)
    from .Engine.SnapKV.backend import LMBackend
    engine = LMBackend(dtype=torch.bfloat16, device=DEVICE)
    engine.load_model(args.model, use_tp=use_tp, rank_group=args.rank_group, group=global_group)
    if args.compile:
        engine.compile()
    engine.setup_caches(max_batch_size=args.B, max_seq_length=args.max_len, kv_dtype=args.kv_dtype,
                        kv_layout=args.kv_layout)
    tokenizer, eot_1, eot_2, dataloader, num_eval_steps = _data(args, engine, print_)
    sampler = _sampler(args, engine, 0, DEVICE)
    total_time, model_steps = 0.0, 0
    for step, batch in enumerate(dataloader):
        if step >= num_eval_steps:
            break
        input_ids = batch[0].to(DEVICE)
        output, steps, dt = harness.run_baseline_batch(engine, input_ids, args.max_len, eot_1, eot_2, sampler=sampler)
        total_time += dt
        model_steps += steps
        if args.printoutput:
            for i in range(args.B):
                print_(tokenizer.decode(output[i, args.prefix_len:]))
        print_(f"Tokens per second :{args.B * (model_steps / total_time)}")
        if step < 5:
            total_time, model_steps = 0.0, 0
        if use_tp:
            dist.barrier()
    print_(f"Final tokens per second :{args.B * (model_steps / total_time)}")
    return args.B * (model_steps / total_time)

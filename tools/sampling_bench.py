"""Per-iteration cost of the sampling head at cfg3 shapes (Llama-3.1-8B target + 1B draft, B = 64, gamma = 3,
V = 128 256): the only launches in which a sampled iteration differs from a greedy one.

Greedy head of one iteration:   3 x argmax over [B, V] (draft steps) + argmax over [B*(gamma+1), V] (verify).
Sampled head of one iteration:  3 x md_sample_rows in draft mode (stats, draw, ring copy) + md_spec_verify_sample.
Per-request head ("req_*" arms): the same launches through md_sample_rows_req / md_spec_verify_sample_req, whose
temperature / top_p / top_k are [B] device tensors -- uniform parameters with top-k off (the passes of the scalar form
plus the parameter loads), top-k 50 before top-p 0.9 (one more pass over the row), and a half-greedy batch.
Both arms are captured into one hipGraph each (as the decode steps are) and replayed alternately in one process;
the logits are realistic-scale random bf16 rows, re-used every iteration (the ring and stats are rewritten).
Prints one JSON line per configuration: ms per iteration of each arm and the difference.

  python tools/sampling_bench.py [--iters 200] [--rounds 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from magicdec_amd import ops  # noqa: E402
from magicdec_amd import sampling_ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--gamma", type=int, default=3)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    B, G, V = a.B, a.gamma, a.vocab
    g = torch.Generator(device=dev).manual_seed(0)
    draft_logits = [(torch.randn(B, V, device=dev, generator=g) * 3).to(torch.bfloat16) for _ in range(G)]
    tgt_logits = (torch.randn(B * (G + 1), V, device=dev, generator=g) * 3).to(torch.bfloat16)
    ctr = torch.zeros(4, dtype=torch.int32, device=dev)
    ring = torch.zeros((B, G, V), dtype=torch.bfloat16, device=dev)
    rst = torch.zeros((B, G, 2), dtype=torch.int64, device=dev)
    tst = torch.zeros((B * (G + 1), 2), dtype=torch.int64, device=dev)
    tb = torch.zeros((B, G + 1), dtype=torch.int64, device=dev)
    tok = torch.zeros((B, 1), dtype=torch.int64, device=dev)

    def greedy():
        for j in range(G):
            tb[:, j + 1:j + 2] = ops.argmax(draft_logits[j]).view(B, 1)
        return ops.argmax(tgt_logits)

    def sampled(T, top_p):
        def f():
            for j in range(G):
                ops.sample_rows(draft_logits[j], 1, T, top_p, 123, ops.SAMPLE_DRAFT, ctr, ops.ADVANCE_STEP, ring=ring,
                                ring_stats=rst, out=tok)
                tb[:, j + 1:j + 2] = tok
            return ops.spec_verify_sample(tgt_logits, tb, ring, rst, tst, ctr, T, top_p, 123)
        return f

    def per_request(T, top_p, top_k):
        Td = torch.tensor(T, dtype=torch.float32, device=dev)
        Pd = torch.tensor(top_p, dtype=torch.float32, device=dev)
        Kd = torch.tensor(top_k, dtype=torch.int32, device=dev)

        def f():
            for j in range(G):
                sampling_ops.sample_rows_req(draft_logits[j], 1, Td, Pd, Kd, 123, ops.SAMPLE_DRAFT, ctr,
                                             ops.ADVANCE_STEP, ring=ring, ring_stats=rst, out=tok)
                tb[:, j + 1:j + 2] = tok
            return sampling_ops.spec_verify_sample_req(tgt_logits, tb, ring, rst, tst, ctr, Td, Pd, Kd, 123)
        return f

    half = [0.0 if b % 2 else 0.6 for b in range(B)]
    arms = {"greedy": greedy, "T0.6_p0.9": sampled(0.6, 0.9), "T0.6_p1.0": sampled(0.6, 1.0),
            "req_uniform_T0.6_p0.9": per_request([0.6] * B, [0.9] * B, [0] * B),
            "req_uniform_T0.6_p1.0": per_request([0.6] * B, [1.0] * B, [0] * B),
            "req_T0.6_p0.9_k50": per_request([0.6] * B, [0.9] * B, [50] * B),
            "req_half_greedy_T0.6_p0.9": per_request(half, [0.9] * B, [0] * B)}
    graphs = {}
    for name, fn in arms.items():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            fn()
        graphs[name] = gr
    times = {n: [] for n in arms}
    for _ in range(a.rounds):
        for name, gr in graphs.items():
            for _ in range(5):
                gr.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                gr.replay()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.iters)
    med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
    for name in arms:
        print(json.dumps({"arm": name, "B": B, "gamma": G, "vocab": V, "ms_per_iteration_head": round(med[name], 4),
                          "rounds_ms": [round(x, 4) for x in times[name]],
                          "overhead_vs_greedy_ms": round(med[name] - med["greedy"], 4)}))


if __name__ == "__main__":
    main()

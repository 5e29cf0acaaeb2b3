"""Local-phase kernel time of the vocab-sharded sampling head at cfg3's TP-8 shard shapes (B = 64, gamma = 3,
V_loc = 16 032 of V = 128 256) against the one-GPU head at V = 128 256, on one GPU in one process.

What is measured: the launches of ONE rank -- a draft step (max, 1-2 histograms, draw, finish) and a verify (max + probe,
1-2 histograms, candidates, finish).  What is NOT measured: the 4 (top_p < 1) or 3 (top_p = 1) all-reduces per call that
sit between those launches on a real TP group; the rank's own buffers stand in for the reduced ones (self-consistent, so
every phase does its full work).  Each arm is one hipGraph, arms alternated, median round (tools/sampling_bench.py method).
Prints one JSON line per arm.

  python tools/sharded_sampling_bench.py [--iters 200] [--rounds 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from magicdec_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--gamma", type=int, default=3)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    B, G, V, W = a.B, a.gamma, a.vocab, a.world
    VL = -(-V // W)
    off = VL * (W // 2)
    R = B * (G + 1)
    g = torch.Generator(device=dev).manual_seed(0)
    bf, i64 = dict(dtype=torch.bfloat16, device=dev), dict(dtype=torch.int64, device=dev)
    draft = (torch.randn(B, V, device=dev, generator=g) * 3).to(torch.bfloat16)
    tgt = (torch.randn(R, V, device=dev, generator=g) * 3).to(torch.bfloat16)
    draft_s, tgt_s = draft[:, off:off + VL].contiguous(), tgt[:, off:off + VL].contiguous()
    ctr = torch.zeros(4, dtype=torch.int32, device=dev)
    ring, ring_s = torch.zeros((B, G, V), **bf), torch.zeros((B, G, VL), **bf)
    rst, tst = torch.zeros((B, G, 2), **i64), torch.zeros((R, 2), **i64)
    tb = torch.randint(0, V, (B, G + 1), device=dev, generator=g)
    tb[:, 1:] = off + tb[:, 1:] % VL                # every draft token on this rank: the probe does its reads
    tok, tt = torch.zeros((B, 1), **i64), torch.zeros((B, G + 1), **i64)
    red, hi, lo, cand = torch.zeros(B, **i64), torch.zeros((B, 256), **i64), torch.zeros((B, 256), **i64), torch.zeros(B, **i64)
    vred, vhi, vlo = torch.zeros(R + B * G, **i64), torch.zeros((R, 256), **i64), torch.zeros((R, 256), **i64)
    vcand = torch.zeros((B, 3), **i64)
    T, seed = 0.6, 123

    def one_draft(p):
        return lambda: ops.sample_rows(draft, 1, T, p, seed, ops.SAMPLE_DRAFT, ctr, ops.ADVANCE_NONE, ring=ring,
                                       ring_stats=rst, out=tok)

    def one_verify(p):
        return lambda: ops.spec_verify_sample(tgt, tb, ring, rst, tst, ctr, T, p, seed, out=tt)

    def shard_draft(p):
        def f():
            ops.shard_max(draft_s, 1, off, V, red)
            ops.shard_hist(draft_s, 1, T, p, red, hi)
            if p < 1:
                ops.shard_hist(draft_s, 1, T, p, red, lo, hist_hi=hi)
            ops.shard_draw(draft_s, 1, off, V, T, p, seed, ops.SAMPLE_DRAFT, ctr, red, hi, lo if p < 1 else None, cand,
                           ring=ring_s, ring_stats=rst)
            ops.shard_finish(cand, 1, ctr, ops.ADVANCE_NONE, out=tok)
        return f

    def shard_verify(p):
        def f():
            ops.shard_max(tgt_s, 1, off, V, vred, tokens_buffer=tb, ring=ring_s)
            ops.shard_hist(tgt_s, 1, T, p, vred, vhi)
            if p < 1:
                ops.shard_hist(tgt_s, 1, T, p, vred, vlo, hist_hi=vhi)
            ops.spec_verify_shard(tgt_s, tb, off, V, ring_s, rst, vred, vhi, vlo if p < 1 else None, tst, ctr, T, p, seed,
                                  vcand)
            ops.spec_verify_shard_finish(vcand, tb, ctr, out=tt)
        return f

    arms = {}
    for p in (0.9, 1.0):
        arms[f"one_gpu_draft_step_p{p}"] = one_draft(p)
        arms[f"shard_draft_step_p{p}"] = shard_draft(p)
        arms[f"one_gpu_verify_p{p}"] = one_verify(p)
        arms[f"shard_verify_p{p}"] = shard_verify(p)
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
            times[name].append(e0.elapsed_time(e1) * 1000 / a.iters)
    for name in arms:
        v = times[name]
        print(json.dumps({"arm": name, "B": B, "gamma": G, "vocab": V, "v_loc": VL if name.startswith("shard") else V,
                          "us_per_call": round(sorted(v)[len(v) // 2], 1), "rounds_us": [round(x, 1) for x in v]}))


if __name__ == "__main__":
    main()

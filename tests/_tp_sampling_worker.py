"""Worker of tests/test_gpu_sampling_tp.py: one of two TP ranks, both on GPU 0 (MAGICDEC_TP_SINGLE_GPU=1, gloo), running
the four sampled loops on the tiny checkpoints with a recording ShardedSampler.  Writes its final state as JSON and every
recorded sampler launch (this rank's logits and ring shards, counters, tokens, stats) with torch.save."""
import json
import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import golden_cfg as gc  # noqa: E402

T, TOP_P = 0.8, 0.9


def main():
    from magicdec_amd import harness
    from magicdec_amd.Engine import model_core, sampling
    from magicdec_amd.Engine.SnapKV.backend import LMBackend
    from magicdec_amd.Engine.SnapKV.backend_draft import LMBackend_Draft
    from magicdec_amd.Engine.StreamingLLM.backend import LMBackend as StreamBackend
    from magicdec_amd.Engine.tp import init_dist

    class Recording(sampling.ShardedSampler):
        log = None

        def head(self, logits, role, idx, B, n):
            if self.log is None:
                return super().head(logits, role, idx, B, n)
            rec = dict(role=role, n=n, B=B, logits=logits.cpu(), before=self.counters.tolist(),
                       row_sel=self.row_sel.cpu())
            if role == "verify":
                rec.update(tokens=idx.cpu(), ring=self.ring.cpu(), ring_stats=self.ring_stats.cpu())
            out = super().head(logits, role, idx, B, n)
            rec.update(out=out.cpu(), after=self.counters.tolist())
            if role == "draft":
                j = rec["before"][1]
                rec.update(slot=self.ring[:, j].cpu(), slot_stats=self.ring_stats[:, j].cpu())
            if role == "verify":
                rec["target_stats"] = self.target_stats.cpu()
            self.log.append(rec)
            return out

    ck = Path(os.environ["MD_CKPT"]) / "tinytgt" / "model.pth"
    out_dir = os.environ["MD_OUT"]
    gc.register_tiny(model_core)
    rank, group, dgroup = init_dist([0, 1])
    other = dist.new_group([0])                 # a one-rank group: the draft-sub-group topology
    dev, bf = "cuda:0", torch.bfloat16
    tp = dict(use_tp=True, rank_group=[0, 1])

    tgt = LMBackend(dtype=bf, device=dev, dec_len=gc.GAMMA + 1)
    tgt.load_model(ck, group=group, **tp)
    tgt.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN)
    drf = LMBackend_Draft(dtype=bf, device=dev, draft_budget=gc.BUDGET)
    drf.load_model(ck, group=dgroup, **tp)
    drf.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN, draft_budget=gc.BUDGET)
    rep = LMBackend_Draft(dtype=bf, device=dev, draft_budget=gc.BUDGET)
    rep.load_model(ck, use_tp=False)
    rep.model.replica_group = group
    rep.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN, draft_budget=gc.BUDGET)
    slf = StreamBackend(dtype=bf, device=dev, dec_len=gc.GAMMA + 1)
    slf.load_model(ck, group=group, **tp)
    slf.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN, draft_budget=gc.BUDGET)
    base = LMBackend(dtype=bf, device=dev)
    base.load_model(ck, group=group, **tp)
    base.setup_caches(max_batch_size=gc.B, max_seq_length=gc.MAX_LEN)
    v_loc = tgt.model.output.weight.shape[0]
    ids = gc.synthetic_batches()[1].to(dev)

    def run(loop, seed, record=False):
        gamma = 0 if loop == "baseline" else gc.GAMMA
        smp = None
        if seed is not None:
            smp = Recording(T, TOP_P, seed, gc.B, gamma, v_loc, dev, group, replicate_draft=loop == "longspec_replicate")
            smp.log = [] if record else None
        trace = []
        tf = lambda s: trace.append(s.accept_nums.tolist())
        if loop.startswith("longspec"):
            st, _ = harness.run_longspec_batch(tgt, rep if loop.endswith("replicate") else drf, ids, gc.GAMMA, gc.MAX_LEN,
                                               gc.EOT_1, gc.EOT_2, trace_fn=tf, barrier=dist.barrier, sampler=smp)
            res = dict(output=st.output.cpu().tolist(), num_nodes=st.num_nodes.cpu().tolist())
        elif loop == "selfspec_stream":
            st, _ = harness.run_selfspec_batch(slf, ids, gc.GAMMA, gc.MAX_LEN, gc.EOT_1, gc.EOT_2, True, trace_fn=tf,
                                               sampler=smp)
            res = dict(output=st.output.cpu().tolist(), num_nodes=st.num_nodes.cpu().tolist())
        else:
            o, steps, _ = harness.run_baseline_batch(base, ids, ids.shape[1] + 32, gc.EOT_1, gc.EOT_2, sampler=smp)
            res = dict(output=o.cpu().tolist(), num_nodes=[steps])
        res.update(trace=trace, counters=smp.counters.tolist() if smp is not None else None)
        if record:
            torch.save(dict(log=smp.log, vocab_offset=smp.vocab_offset, vocab_total=smp.vocab_total, seed=smp.seed),
                       os.path.join(out_dir, f"log_{loop}_rank{rank}.pt"))
        return res

    results = {}
    for loop in ("longspec_snapkv", "longspec_replicate", "selfspec_stream", "baseline"):
        results[loop] = run(loop, 5, record=True)
    results["again"] = run("longspec_snapkv", 5)
    results["other_seed"] = run("longspec_snapkv", 6)
    results["greedy"] = run("longspec_snapkv", None)

    # a draft sharded over another group than the target's is refused, with the reason
    smp = sampling.ShardedSampler(T, TOP_P, 1, gc.B, gc.GAMMA, v_loc, dev, group)
    stub = type("M", (), {})()
    stub.process_group, stub.output = other, tgt.model.output
    try:
        smp.check_model(stub)
        results["other_group"] = "accepted"
    except ValueError as e:
        results["other_group"] = str(e)
    results["widths"] = [smp.v_loc, smp.vocab_offset, smp.vocab_total, smp.rank, smp.world]
    json.dump(results, open(os.path.join(out_dir, f"rank{rank}.json"), "w"))
    dist.barrier()
    dist.destroy_process_group()
    print(f"rank {rank}: OK")


if __name__ == "__main__":
    main()

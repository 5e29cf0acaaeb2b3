"""Vocab-sharded sampling in the decode loops: ONE launch of two TP ranks sharing GPU 0 (MAGICDEC_TP_SINGLE_GPU=1, gloo
as the transport of the sampler's all-reduces) runs longspec SnapKV with the draft sharded over the same ranks, longspec
with a replicated draft, StreamingLLM self-speculation and the baseline loop on the tiny checkpoints, with a recording
ShardedSampler (tests/_tp_sampling_worker.py).  Both ranks must end in the same state, and every recorded launch -- the
two ranks' logits shards and ring shards concatenated -- must be what the one-GPU kernel gives with the recorded
counters, bit for bit.  Eager steps: gloo collectives cannot be captured (Engine/graph.py falls back the same way)."""
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from magicdec_amd import ops
from tests import golden_cfg as gc
from tests.test_gpu_engine import ckpt_dir  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, TOP_P = 0.8, 0.9
LOOPS = ("longspec_snapkv", "longspec_replicate", "selfspec_stream", "baseline")


@pytest.fixture(scope="module")
def pair(ckpt_dir):  # noqa: F811
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tempfile.mkdtemp(prefix="md_tp_sampling_")
    port = 29300 + (os.getpid() % 200)
    procs = []
    for r in range(2):
        env = dict(os.environ, LOCAL_RANK=str(r), LOCAL_WORLD_SIZE="2", RANK=str(r), WORLD_SIZE="2",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MD_CKPT=str(ckpt_dir), MD_OUT=out,
                   MAGICDEC_TP_SINGLE_GPU="1", MAGICDEC_ONESHOT_AR="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tests", "_tp_sampling_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=300)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    return out, [json.load(open(os.path.join(out, f"rank{r}.json"))) for r in range(2)]


def test_both_ranks_end_in_the_same_state(pair):
    _, (r0, r1) = pair
    for key in LOOPS + ("again", "other_seed", "greedy"):
        assert r0[key] == r1[key], key
    for loop in LOOPS:
        assert r0[loop]["counters"][0] > 3 and r0[loop]["counters"][1:] == [0, 0, 0]
    assert r0["again"] == r0["longspec_snapkv"], "two runs with the same seed differ"
    assert r0["other_seed"]["output"] != r0["longspec_snapkv"]["output"], "another seed drew the same tokens"
    assert r0["greedy"]["output"] != r0["longspec_snapkv"]["output"], "the sampled run equals the greedy run"
    assert len(r0["longspec_snapkv"]["trace"]) > 3
    # torch.chunk of the 2048-token head over two ranks
    assert r0["widths"] == [1024, 0, 2048, 0, 2] and r1["widths"] == [1024, 1024, 2048, 1, 2]
    for r in (r0, r1):
        assert "sub-group" in r["other_group"] and "not supported" in r["other_group"]


def _ctr(vals):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("loop", LOOPS)
def test_every_recorded_launch_is_the_one_gpu_kernel_on_the_concatenated_shards(pair, loop):
    out, _ = pair
    l0, l1 = (torch.load(os.path.join(out, f"log_{loop}_rank{r}.pt")) for r in range(2))
    assert (l0["vocab_offset"], l1["vocab_offset"], l0["vocab_total"]) == (0, 1024, 2048)
    seed, V = l0["seed"], l0["vocab_total"]
    G = 0 if loop == "baseline" else gc.GAMMA
    replicate = loop == "longspec_replicate"
    assert len(l0["log"]) == len(l1["log"]) > 3
    roles = set()
    ring = torch.zeros((gc.B, max(G, 1), V), dtype=torch.bfloat16, device=DEV)
    rst = torch.zeros((gc.B, max(G, 1), 2), dtype=torch.int64, device=DEV)
    for a, b in zip(l0["log"], l1["log"]):
        role, n, B = a["role"], a["n"], a["B"]
        roles.add(role)
        for k in ("role", "n", "B", "before", "after"):
            assert a[k] == b[k], k
        for k in ("out", "row_sel"):
            assert torch.equal(a[k], b[k]), (role, k)
        whole = a["logits"].shape[1] == V                   # the replicated draft (prefill and steps): full rows on every rank
        assert whole == (replicate and role in ("draft", "prefill") and whole)
        logits = (a["logits"] if whole else torch.cat([a["logits"], b["logits"]], dim=1)).to(DEV)
        assert logits.shape == (B * n, V) and (not whole or torch.equal(a["logits"], b["logits"]))
        ctr = _ctr(a["before"])
        if role == "verify":
            full = a["ring"] if replicate else torch.cat([a["ring"], b["ring"]], dim=2)
            assert torch.equal(a["ring_stats"], b["ring_stats"]) and torch.equal(a["target_stats"], b["target_stats"])
            assert torch.equal(full.to(DEV), ring) and torch.equal(a["ring_stats"].to(DEV), rst), "the ring the drafts wrote"
            tst = torch.zeros((B * (G + 1), 2), dtype=torch.int64, device=DEV)
            ref = ops.spec_verify_sample(logits, a["tokens"].to(DEV), ring, rst, tst, ctr, T, TOP_P, seed)
            assert torch.equal(tst.cpu(), a["target_stats"])
        elif role == "draft":
            ref = ops.sample_rows(logits, n, T, TOP_P, seed, ops.SAMPLE_DRAFT, ctr, ops.ADVANCE_STEP,
                                  row_sel=a["row_sel"].to(DEV) if n == 2 else None, ring=ring, ring_stats=rst)
            j = a["before"][1]
            slot = a["slot"] if replicate else torch.cat([a["slot"], b["slot"]], dim=1)
            assert torch.equal(ring[:, j].cpu(), slot) and torch.equal(rst[:, j].cpu(), a["slot_stats"])
            assert torch.equal(a["slot_stats"], b["slot_stats"])
        else:
            purpose = ops.SAMPLE_PREFILL if role == "prefill" else ops.SAMPLE_BASELINE
            ref = ops.sample_rows(logits, n, T, TOP_P, seed, purpose, ctr, ops.ADVANCE_ITER)
        assert torch.equal(ref.cpu(), a["out"]), (loop, role, a["before"])
        assert ctr.tolist() == a["after"]
    assert roles >= ({"prefill", "baseline"} if loop == "baseline" else {"prefill", "draft", "verify"})

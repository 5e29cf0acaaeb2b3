"""CPU tests of vocab-sharded sampling (include/magicdec_hip.h K11 "sharded"): the --sharded_sampling flag of the five
entry points, ShardedSampler.check_model, the offsets of uneven vocabulary chunks, and the candidate packing of
csrc/sample.hip restated in Python."""
import random
import struct

import numpy as np
import pytest
import torch

from magicdec_amd import cli
from magicdec_amd.Engine import sampling

PARSERS = [lambda: cli.longspec_parser("SnapKV"), lambda: cli.longspec_parser("StreamingLLM"),
           lambda: cli.selfspec_parser("SnapKV"), lambda: cli.selfspec_parser("StreamingLLM"), cli.baseline_parser]


def test_sharded_sampling_flag_on_all_five_entry_points(capsys):
    for i, mk in enumerate(PARSERS):
        assert cli.parse_entry_args(mk(), ["--rank_group", "0"]).sharded_sampling is False
        a = cli.parse_entry_args(mk(), ["--rank_group", "0", "1", "--temperature", "0.6", "--sharded_sampling"])
        assert a.sharded_sampling is True and a.temperature == 0.6
        # without the flag nothing changed: exit 2, and the message now names the way out
        with pytest.raises(SystemExit) as e:
            cli.parse_entry_args(mk(), ["--rank_group", "0", "1", "--temperature", "0.6"])
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert "TP = 1" in err and "--sharded_sampling" in err
        cli.parse_entry_args(mk(), ["--rank_group", "0", "1"])                         # greedy TP
        cli.parse_entry_args(mk(), ["--rank_group", "0", "1", "--sharded_sampling"])   # the flag alone changes nothing
        cli.parse_entry_args(mk(), ["--rank_group", "0", "--temperature", "0.6", "--sharded_sampling"])
        if i < 2:                                                                       # longspec: the draft group
            ok = ["--rank_group", "0", "1", "--temperature", "0.6", "--sharded_sampling"]
            cli.parse_entry_args(mk(), ok + ["--draft_rank_group", "0", "1"])
            cli.parse_entry_args(mk(), ["--rank_group", "0", "1", "2", "3", "--temperature", "0.6", "--sharded_sampling",
                                        "--draft_rank_group", "0", "1", "--replicate_draft"])
            with pytest.raises(SystemExit) as e:
                cli.parse_entry_args(mk(), ["--rank_group", "0", "1", "2", "3", "--temperature", "0.6",
                                            "--sharded_sampling", "--draft_rank_group", "0", "1"])
            assert e.value.code == 2
            err = capsys.readouterr().err
            assert "no draft ring" in err and "--replicate_draft" in err
            # greedy with a shorter draft group stays allowed
            cli.parse_entry_args(mk(), ["--rank_group", "0", "1", "2", "3", "--sharded_sampling", "--draft_rank_group",
                                        "0", "1"])


class _Model:
    def __init__(self, width, group):
        self.output = type("o", (), {"weight": torch.zeros(width, 1)})()
        self.process_group = group


def _sharded(v_loc, total, group, replicate=False):
    s = sampling.ShardedSampler.__new__(sampling.ShardedSampler)
    s.group, s.v_loc, s.vocab_total, s.vocab, s.replicate_draft = group, v_loc, total, total, replicate
    return s


def test_sharded_sampler_check_model(monkeypatch):
    ga, gb, ga2 = object(), object(), object()
    ranks = {id(ga): (0, 1), id(gb): (0,), id(ga2): (0, 1)}
    ranks[id(None)] = None
    monkeypatch.setattr(sampling, "_group_ranks", lambda g: ranks.get(id(g)))
    s = _sharded(334, 1001, ga)
    s.check_model(_Model(334, ga))
    s.check_model(_Model(334, ga2))            # another group object over the same ranks (a draft group): accepted
    with pytest.raises(ValueError, match="sub-group.*not supported"):
        s.check_model(_Model(334, gb))
    with pytest.raises(ValueError, match="local head width"):
        s.check_model(_Model(333, ga))
    unseen = _sharded(334, 1001, object())      # two groups this rank is in neither of do not match each other
    with pytest.raises(ValueError, match="not supported"):
        unseen.check_model(_Model(334, object()))
    with pytest.raises(ValueError, match="replicate_draft"):
        s.check_model(_Model(1001, None))      # an unsharded model next to a sharded sampler
    r = _sharded(334, 1001, ga, replicate=True)
    r.check_model(_Model(1001, None))          # the replicated draft
    r.check_model(_Model(334, ga))             # and the sharded target
    with pytest.raises(ValueError, match="vocabulary"):
        r.check_model(_Model(1000, None))
    # the base class is untouched
    b = sampling.Sampler.__new__(sampling.Sampler)
    b.vocab = 334
    with pytest.raises(ValueError, match="TP = 1"):
        b.check_model(_Model(334, ga))


@pytest.mark.parametrize("V,W", [(1001, 3), (2048, 8), (151936, 8), (128256, 8), (32003, 4), (10, 4), (7, 3)])
def test_offsets_of_uneven_chunks(V, W):
    widths = [t.shape[0] for t in torch.chunk(torch.empty(V, 1), W, dim=0)]
    offs, total = sampling.shard_offsets(widths)
    assert total == V and offs[0] == 0
    assert offs == [sum(widths[:i]) for i in range(len(widths))]
    full = torch.arange(V)
    for o, w, t in zip(offs, widths, torch.chunk(full, W)):
        assert torch.equal(full[o:o + w], t)
    if (V, W) == (1001, 3):
        assert widths == [334, 334, 333] and offs == [0, 334, 668]
    with pytest.raises(ValueError):
        sampling.shard_offsets([4, 0, 4])


# ---- the candidate packing of csrc/sample.hip (pack_cand / cand_index), restated.  This checks the ENCODING (that a
# signed int64 MAX is block_argmax's order), on a Python restatement: it passes without the kernels.  The pin on the
# kernel's own pack_cand is tests/test_gpu_sampling_sharded.py.  Form differs in one place: the kernel maps a best of
# -inf to "none" in block_argmax_sc (index -1) before packing; here pack_cand does both.
NONE = -1


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def pack_cand(score, v):
    if v < 0 or score == float("-inf"):
        return NONE
    u = _bits(score)
    if (u << 1) & 0xFFFFFFFF == 0:
        u = 0
    u = (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)
    return (u << 31) | (0x7FFFFFFF - v)


def cand_index(c):
    return 0x7FFFFFFF - (c & 0x7FFFFFFF)


def test_candidate_packing_is_order_isomorphic_to_score_then_lowest_index():
    r = random.Random(5)
    f32 = lambda x: float(np.float32(x))
    scores = [0.0, -0.0, f32(1e-45), f32(-1e-45), f32(1e-40), f32(-1e-40), f32(1.17549435e-38), 1.0, -1.0, 1.5, -1.5,
              f32(3.4e38), f32(-3.4e38), float("inf"), float("-inf")]
    scores += [f32(r.gauss(0, 10)) for _ in range(40)] + [f32(r.uniform(-1e-38, 1e-38)) for _ in range(10)]
    idx = [0, 1, 2, 3, 333, 334, 151935, 2 ** 31 - 1] + [r.randrange(2 ** 31) for _ in range(8)]
    cands = [(s, v) for s in scores for v in idx]
    r.shuffle(cands)
    for s, v in cands:
        c = pack_cand(s, v)
        if s == float("-inf"):
            assert c == NONE                    # a best of -inf is "no candidate"
            continue
        assert 0 <= c < 2 ** 63 and cand_index(c) == v
    assert pack_cand(0.0, 7) == pack_cand(-0.0, 7)

    def better(a, b):                           # block_argmax: the larger score, the lower index among equal scores
        return a[0] > b[0] or (a[0] == b[0] and a[1] < b[1])
    live = [c for c in cands if c[0] != float("-inf")]
    for _ in range(4000):
        a, b = r.choice(live), r.choice(live)
        pa, pb = pack_cand(*a), pack_cand(*b)
        assert (pa > pb) == better(a, b), (a, b)
        assert (pa == pb) == (a[0] == b[0] and a[1] == b[1])
        assert pa > NONE
    # MAX over "ranks" reproduces the argmax over the union, and all-none stays none
    for _ in range(200):
        group = [r.choice(cands) for _ in range(r.randint(1, 8))]
        best = None
        for c in group:
            if c[0] != float("-inf") and (best is None or better(c, best)):
                best = c
        m = max(pack_cand(*c) for c in group)
        assert (m == NONE) if best is None else (cand_index(m) == best[1])


def test_sharded_gpu_inputs_leave_the_oracle_unambiguous():
    """Every case that tests/test_gpu_sampling_sharded.py also gives to the oracle -- random, planted and fuzz, with the
    planted tokens_buffer edits -- through the restatement alone, as sampling_cases.cpu_iteration does for the one-GPU
    cases: the float64 outcome is always admissible, and no restated request has more than one admissible outcome
    (check_iteration tests membership, so an ambiguous request would make the GPU test check less)."""
    from tests import sampling_cases as sc
    from tests import sampling_ref as sr
    from tests import test_gpu_sampling_sharded as g
    total = 0
    for c, edit in g.oracle_cases():
        T, top_p, seed, it, G = c["T"], c["top_p"], c["seed"], c["it"], c["G"]
        tb, rb = sc.bits_of(c["tl"]), sc.bits_of(sc.drawn_rows(c))
        for b in c["restate"]:
            rrows = [sr.ref_row(rb[b, j], T, top_p) for j in range(G)]
            trows = [sr.ref_row(tb[b, j], T, top_p) for j in range(G + 1)]
            tokens = [int(c["tok0"][b])]
            for j in range(G):
                adm = sr.draw_admissible(rrows[j], seed, sr.DRAFT, j, b, it)
                assert len(adm) == 1, f"{c['name']}: draft [{b},{j}] has admissible tokens {adm.tolist()}"
                assert adm[0] == sr.draw_admissible(rrows[j], seed, sr.DRAFT, j, b, it, widen=0.0)[0]
                tokens.append(int(adm[0]))
            if edit is not None:
                row = torch.tensor([tokens] * c["B"])
                edit(row)
                tokens = row[b].tolist()
            outs = sr.verify_admissible(trows, rrows, tokens, seed, b, it)
            exact = sr.verify_admissible(trows, rrows, tokens, seed, b, it, widen=0.0)
            assert len(exact) == 1 and sr.contains(outs, exact[0]), c["name"]
            assert len(outs) == 1, f"{c['name']}: request {b} has {len(outs)} admissible verify outcomes"
            total += 1
    assert total >= 100
    print(f"[sampling] oracle on the sharded GPU cases' inputs: 0 of {total} restated requests ambiguous")

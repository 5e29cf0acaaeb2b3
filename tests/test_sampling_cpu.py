"""CPU tests of temperature / top-p sampling (include/magicdec_hip.h K11): the host Philox of the library, the numpy
restatement's filter against the reference's rule, the verify encoding through the accept loop, and the command-line
flags.  No GPU needed."""
import numpy as np
import pytest
import torch

from tests import sampling_ref as sr


def test_philox_known_answer_and_library_host_entry():
    # Random123 known-answer vectors (philox4x32_10, kat_vectors)
    assert [hex(x) for x in sr.philox4x32_10(np.zeros((1, 4)), 0, 0)[0]] == \
        ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    assert [hex(x) for x in sr.philox4x32_10(np.full((1, 4), 0xFFFFFFFF), 0xFFFFFFFF, 0xFFFFFFFF)[0]] == \
        ["0x408f276d", "0x41c83b0e", "0xa20bc7c6", "0x6d5451fd"]
    from magicdec_amd import ops
    rng = np.random.default_rng(0)
    for _ in range(8):
        ctr = rng.integers(0, 2 ** 32, size=(257, 4), dtype=np.uint64).astype(np.uint32)
        k0, k1 = (int(x) for x in rng.integers(0, 2 ** 32, size=2))
        assert np.array_equal(ops.philox_host(ctr, k0, k1), sr.philox4x32_10(ctr, k0, k1))


def test_uniforms_are_strictly_inside_the_unit_interval_and_exact_in_fp32():
    u = sr.uniforms(np.array([0, 1, 511, 512, 0xFFFFFFFF], dtype=np.uint64))
    assert u.min() > 0 and u.max() < 1
    assert np.array_equal(u, u.astype(np.float32).astype(np.float64))


def _reference_keep(logits, top_p, T):
    """Engine/utils.py:68-83 (get_sampling_logits) restated in torch: sort descending, cumsum of softmax(l / T), shift
    by one, remove what exceeds top_p -> kept mask."""
    logits = logits.clone()
    if top_p < 1.0:
        sorted_logits, sorted_indices = torch.sort(logits, descending=True)
        cumulative_probs = torch.cumsum(torch.nn.functional.softmax(sorted_logits / T, dim=-1), dim=-1)
        filt = cumulative_probs > top_p
        filt[..., 1:] = filt[..., :-1].clone()
        filt[..., 0] = 0
        remove = filt.scatter(-1, sorted_indices, filt)
        logits[remove] = float("-inf")
    return torch.isfinite(logits)


@pytest.mark.parametrize("T", [0.3, 0.6, 1.0, 1.5])
@pytest.mark.parametrize("top_p", [0.1, 0.5, 0.9, 0.99, 1.0])
def test_top_p_rule_equals_the_reference_on_distinct_logits(T, top_p):
    rng = np.random.default_rng(int(T * 10) + int(top_p * 1000))
    checked = 0
    for trial in range(20):
        V = 3000
        # distinct bf16 values: a random subset of distinct bit patterns of [-8, 8)
        cand = np.unique(sr.bf16_bits(rng.uniform(-8, 8, size=4 * V).astype(np.float32)))
        bits = rng.permutation(cand)[:V].astype(np.uint16)
        f = sr.row_filter(bits, T, top_p)
        if f["margin"] < 1e-9:
            continue
        ref = _reference_keep(torch.from_numpy(sr.bits_to_f(bits)), top_p, T).numpy()
        assert np.array_equal(f["keep"], ref), (trial, f["keep"].sum(), ref.sum())
        checked += 1
    assert checked >= 15


def test_top_p_keeps_or_drops_a_tie_group_whole():
    T, top_p = 1.0, 0.5
    vals = np.array([3.0] * 1 + [2.0] * 6 + [0.0] * 20, dtype=np.float32)
    bits = sr.bf16_bits(vals)
    f = sr.row_filter(bits, T, top_p)
    group = bits == sr.bf16_bits(np.float32(2.0))
    # the top token alone is below top_p of the mass, so the whole 2.0 group is kept (the reference's order-dependent
    # rule would cut somewhere inside it)
    assert f["keep"][group].all() and not f["keep"][vals == 0.0].any()
    f2 = sr.row_filter(bits, T, 0.01)
    assert f2["keep"].sum() == 1 and not f2["keep"][group].any()


def test_verify_encoding_through_the_cpu_accept_loop_matches_the_textbook_algorithm():
    from tests import cpu_ops
    rng = np.random.default_rng(3)
    V, G, B, T = 40, 3, 64, 0.8
    seed, iteration = 1234, 7
    for case in range(4):
        tl = rng.normal(size=(B, G + 1, V)).astype(np.float32) * 2
        dl = (tl[:, :G] + rng.normal(size=(B, G, V)).astype(np.float32) * (0.5 * case)).astype(np.float32)
        tbits, rbits = sr.bf16_bits(tl), sr.bf16_bits(dl)
        tokens = np.zeros((B, G + 1), dtype=np.int64)
        tokens[:, 0] = rng.integers(0, V, size=B)
        for b in range(B):
            for j in range(G):
                tokens[b, j + 1] = sr.draw(rbits[b, j], T, 0.9, seed, sr.DRAFT, j, b, iteration)[0]
        tt = np.zeros_like(tokens)
        exp_acc, exp_tok = [], []
        for b in range(B):
            tt[b], _ = sr.verify(tbits[b], rbits[b], tokens[b], T, 0.9, seed, b, iteration)
            p_rows = [sr.probs(sr.row_filter(tbits[b, j], T, 0.9)) for j in range(G + 1)]
            q_rows = [sr.probs(sr.row_filter(rbits[b, j], T, 0.9)) for j in range(G)]
            us = [sr.uniforms(sr.words(seed, sr.ACCEPT, j, b, iteration, [0]))[0] for j in range(G)]
            acc, tok = sr.textbook_verify(p_rows, q_rows, tokens[b, 1:], us, lambda j: tt[b, j])
            exp_acc.append(acc + 1)
            exp_tok.append(tok if tok is not None else tt[b, G])
            if tok is not None:
                assert tok != tokens[b, acc + 1]          # a residual sample is never the rejected draft
        dev = "cpu"
        tb = torch.from_numpy(tokens.copy())
        out = torch.zeros((B, 64), dtype=torch.long)
        num_nodes = torch.full((B,), 10, dtype=torch.long)
        cachelens = torch.full((B,), 10 + G + 1, dtype=torch.int32)
        lpl = cachelens.clone()
        an = torch.zeros(B, dtype=torch.long)
        bonus = torch.zeros(B, dtype=torch.long)
        dbl = torch.zeros((B, 2), dtype=torch.long)
        cu = torch.ones(B, dtype=torch.long)
        flags = torch.zeros(2, dtype=torch.int32, device=dev)
        cpu_ops.accept_rollback(tb, torch.from_numpy(tt), out, num_nodes, cachelens, lpl, None, None, G, G, G,
                                -5, -6, 10 ** 6, an, bonus, dbl, cu, flags)
        assert an.tolist() == exp_acc
        assert bonus.tolist() == [int(x) for x in exp_tok]


def test_cli_sampling_flags_defaults_validation_and_tp_rejection(monkeypatch):
    from magicdec_amd import cli
    parsers = [lambda: cli.longspec_parser("SnapKV"), lambda: cli.longspec_parser("StreamingLLM"),
               lambda: cli.selfspec_parser("SnapKV"), lambda: cli.selfspec_parser("StreamingLLM"), cli.baseline_parser]
    for mk in parsers:
        args = cli.parse_entry_args(mk(), ["--rank_group", "0"])
        assert args.temperature == 0.0 and args.top_p == 1.0
        a = cli.parse_entry_args(mk(), ["--rank_group", "0", "--temperature", "0.6", "--top_p", "0.9"])
        assert (a.temperature, a.top_p) == (0.6, 0.9)
        for bad in (["--temperature", "-0.1"], ["--top_p", "0"], ["--top_p", "1.5"], ["--temperature", "nan"]):
            with pytest.raises(SystemExit):
                cli.parse_entry_args(mk(), ["--rank_group", "0"] + bad)
        with pytest.raises(SystemExit):
            cli.parse_entry_args(mk(), ["--rank_group", "0", "1", "--temperature", "0.6"])
        cli.parse_entry_args(mk(), ["--rank_group", "0", "1"])        # greedy TP stays allowed

    # the entry points themselves reject TP > 1 with sampling before any model is loaded
    def no_load(*a, **k):
        raise AssertionError("a model was loaded")
    from magicdec_amd.Engine import backend_core, tp
    monkeypatch.setattr(backend_core._BackendBase, "load_model", no_load)
    monkeypatch.setattr(tp, "init_dist", no_load)
    for main, extra in ((lambda av: cli.longspec_main("SnapKV", av), ["--draft_rank_group", "0", "1"]),
                        (lambda av: cli.longspec_main("StreamingLLM", av), ["--draft_rank_group", "0", "1"]),
                        (lambda av: cli.selfspec_main("SnapKV", av), []),
                        (lambda av: cli.selfspec_main("StreamingLLM", av), []),
                        (cli.baseline_main, [])):
        with pytest.raises(SystemExit) as e:
            main(["--rank_group", "0", "1", "--temperature", "0.6"] + extra)
        assert e.value.code == 2


def test_sampler_rejects_tp_and_vocab_mismatch():
    from magicdec_amd.Engine import sampling

    class _W:
        def __init__(self, v):
            self.output = type("o", (), {"weight": torch.zeros(v, 1)})()
            self.process_group = None

    s = sampling.Sampler.__new__(sampling.Sampler)
    s.vocab = 100
    s.check_model(_W(100))
    with pytest.raises(ValueError, match="vocabulary"):
        s.check_model(_W(101))
    m = _W(100)
    m.process_group = object()
    with pytest.raises(ValueError, match="TP = 1"):
        s.check_model(m)
    with pytest.raises(ValueError):
        sampling.validate(-1.0, 0.5)
    with pytest.raises(ValueError):
        sampling.validate(0.5, 0.0)


def test_temperature_zero_selects_the_greedy_path():
    from magicdec_amd import cli
    for mk in (lambda: cli.longspec_parser("SnapKV"), cli.baseline_parser):
        a = cli.parse_entry_args(mk(), ["--rank_group", "0", "--temperature", "0"])
        b = cli.parse_entry_args(mk(), ["--rank_group", "0"])
        assert vars(a) == vars(b)
        assert cli._sampler(a, None, 3, "cpu") is None


# ------------------------------------------------------------------------------------ the admissible-outcome oracle
def _small_inputs(rng, V, G, B, sigma, scale=2.0):
    tl = rng.normal(size=(B, G + 1, V)).astype(np.float32) * scale
    dl = (tl[:, :G] + rng.normal(size=(B, G, V)).astype(np.float32) * sigma).astype(np.float32)
    return sr.bf16_bits(tl), sr.bf16_bits(dl)


def test_noise_row_equals_the_per_token_words():
    for V in (1, 5, 50, 1001):
        assert np.array_equal(sr.noise_row(77, sr.RESIDUAL, 3, 9, 123456, V),
                              sr.words(77, sr.RESIDUAL, 3, 9, 123456, np.arange(V)))


@pytest.mark.parametrize("top_p", [0.9, 1.0])
def test_admissible_set_is_the_restatement_outcome_where_that_is_unflagged(top_p):
    """Where sr.verify calls no decision close, the oracle (restatement's own stats) admits exactly its row; flagged or
    not, the oracle's set contains both its own float64 outcome and sr.verify's."""
    rng = np.random.default_rng(17)
    V, G, B, T, seed, it = 1000, 3, 48, 0.8, 31337, 3
    single = flagged = 0
    for sigma in (0.5, 1.0):
        tbits, rbits = _small_inputs(rng, V, G, B, sigma)
        for b in range(B):
            tokens = [5] + [sr.draw(rbits[b, j], T, top_p, seed, sr.DRAFT, j, b, it)[0] for j in range(G)]
            ref, fl = sr.verify(tbits[b], rbits[b], np.array(tokens), T, top_p, seed, b, it)
            trows = [sr.ref_row(tbits[b, j], T, top_p) for j in range(G + 1)]
            rrows = [sr.ref_row(rbits[b, j], T, top_p) for j in range(G)]
            outs = sr.verify_admissible(trows, rrows, tokens, seed, b, it)
            exact = sr.verify_admissible(trows, rrows, tokens, seed, b, it, widen=0.0)
            assert len(exact) == 1 and sr.contains(outs, exact[0])
            assert sr.contains(outs, ref), (b, ref, outs)
            flagged += fl
            if not fl:
                assert len(outs) == 1, (b, ref, outs)
                single += 1
    assert single >= 20 and single + flagged == 2 * B    # sr.verify flags most requests at top_p = 1 (the tail rule)


def test_oracle_out_of_range_draft_is_a_rejection_and_equal_rows_accept_everything():
    rng = np.random.default_rng(5)
    V, G, T, top_p, seed, it = 300, 3, 0.9, 0.9, 99, 8
    tbits, _ = _small_inputs(rng, V, G, 1, 0.0)
    trows = [sr.ref_row(tbits[0, j], T, top_p) for j in range(G + 1)]
    rrows = trows[:G]                                             # the same function of the same bits: r == 0 exactly
    drafts = [int(sr.draw_admissible(rrows[j], seed, sr.DRAFT, j, 0, it, widen=0.0)[0]) for j in range(G)]
    outs = sr.verify_admissible(trows, rrows, [7] + drafts, seed, 0, it)
    assert len(outs) == 1 and outs[0][:G].tolist() == drafts and outs[0][G] >= 0
    for bad in (-1, V):
        for pos in (0, 2):
            toks = [7] + drafts
            toks[pos + 1] = bad
            outs = sr.verify_admissible(trows, rrows, toks, seed, 0, it)
            # the residual is zero everywhere: the fallback draw from p~ (RESIDUAL key) that excludes nothing real
            want = sr.draw_admissible(trows[pos], seed, sr.RESIDUAL, pos, 0, it, exclude=bad)
            assert [o.tolist() for o in outs] == [drafts[:pos] + [int(t)] + [-1] * (G - pos) for t in want]
            assert len(outs) == 1


def test_check_stats_accepts_the_neighbour_key_only_at_a_boundary_margin():
    T, top_p = 1.0, 0.5
    vals = np.array([3.0] * 1 + [2.0] * 6 + [0.0] * 20, dtype=np.float32)
    bits = sr.bf16_bits(vals)
    m, kstar, zk = sr.ref_stats(bits, T, top_p)
    assert kstar == int(sr.key16(sr.bf16_bits(np.float32(2.0))))
    sr.check_stats(bits, T, top_p, m, kstar, zk)
    k3, k0 = int(sr.key16(sr.bf16_bits(np.float32(3.0)))), int(sr.key16(sr.bf16_bits(np.float32(0.0))))
    for wrong in (k3, k0, kstar + 1):
        with pytest.raises(AssertionError):
            sr.check_stats(bits, T, top_p, m, wrong, zk)
    with pytest.raises(AssertionError):
        sr.check_stats(bits, T, top_p, m, kstar, int(zk * (1 + 1e-4)))
    with pytest.raises(AssertionError):
        sr.check_stats(bits, T, top_p, np.float32(2.0), kstar, zk)
    # a top_p exactly on the boundary of the 2.0 group: the mass above the 0.0 group is top_p * Z up to rounding
    w = np.exp(vals.astype(np.float64) - 3.0)
    edge = float((w[:7].sum()) / w.sum())
    _, allowed = sr._select(sr.key16(bits), w, edge)
    assert allowed == {kstar, k0}


def test_new_gpu_case_inputs_leave_almost_no_request_ambiguous():
    """A condition on the chosen inputs, not on the kernel: with the restatement's own statistics, at most 1 restated
    request in 50 per case (none beyond one in a case of fewer than 50) has more than one admissible outcome."""
    from tests import sampling_cases as sc
    cases = [sc.real_case(n) for n in sc.REAL_CASES]
    for c in cases:
        assert len(c["restate"]) <= sc.MAX_RESTATED or c["V"] < 128256
    total = amb = 0
    for make, keys in ((sc.real_case, list(sc.REAL_CASES)), (sc.fuzz_case, list(range(sc.FUZZ_DEFAULT))),
                       (lambda i: sc.thread_count_cases()[i], [1])):   # the 8 requests both batches share
        for key in keys:
            c = make(key)
            n, a, missing = sc.cpu_iteration(c)
            assert missing == 0, c["name"]
            assert a <= max(1, n // 50), (c["name"], n, a)
            total, amb = total + n, amb + a
    print(f"[sampling] oracle on the GPU cases' inputs: {amb} of {total} restated requests ambiguous")


def test_the_end_of_text_case_has_requests_with_an_end_of_text_draft():
    from tests import sampling_cases as sc
    c, eot_1, eot_2, expect = sc.eot_case()
    assert len(expect) >= 2 and expect.get(7) == 0 and 2 in expect
    for b, pos in expect.items():
        assert c["cpu_drafts"][b, pos] in (eot_1, eot_2)

"""CPU tests of the per-request sampling form: the command-line flags (--top_k, --sampling_params), the sampler the
CLI builds, the operand contract of the two magicdec_amd.sampling_ops wrappers against the recording stand-in of
tests/test_ops_contract_cpu.py, the host-side validation of RequestSampler, and the top-k masking helper of the GPU tests
pinned against a direct numpy statement of K11's top-k-then-top-p rule."""
import json
import types

import numpy as np
import pytest
import torch

from magicdec_amd import cli, ops
from magicdec_amd import sampling_ops as so
from magicdec_amd.Engine import sampling
from tests import sampling_ref as sr
from tests.test_gpu_sampling_request import topk_mask
from tests.test_ops_contract_cpu import F32, I32, I64, as_dtype, draw, i32, install, on_host, ring, swap, verify, z

PARSERS = [lambda: cli.longspec_parser("SnapKV"), lambda: cli.longspec_parser("StreamingLLM"),
           lambda: cli.selfspec_parser("SnapKV"), lambda: cli.selfspec_parser("StreamingLLM"), cli.baseline_parser]


# ------------------------------------------------------------------------------------ the command line
def _file(tmp_path, rows, name="params.json"):
    p = tmp_path / name
    p.write_text(rows if isinstance(rows, str) else json.dumps(rows))
    return str(p)


def test_the_new_flags_are_on_all_five_entry_points(tmp_path):
    path = _file(tmp_path, [{"temperature": 0.7, "top_k": 40}, {}, {"top_p": 0.5}])
    for mk in PARSERS:
        a = cli.parse_entry_args(mk(), ["--rank_group", "0"])
        assert a.top_k == 0 and a.sampling_params is None and a.request_params is None
        a = cli.parse_entry_args(mk(), ["--rank_group", "0", "--temperature", "0.6", "--top_k", "50"])
        assert a.top_k == 50
        a = cli.parse_entry_args(mk(), ["--rank_group", "0", "--B", "3", "--top_p", "0.9", "--top_k", "7",
                                        "--sampling_params", path])
        # a missing key takes the value of the flag (temperature 0 = that request is greedy)
        assert a.request_params == ([0.7, 0.0, 0.0], [0.9, 0.9, 0.5], [40, 7, 7])


def test_range_checks_and_the_several_ranks_refusal(tmp_path, capsys):
    path = _file(tmp_path, [{}])
    for mk in PARSERS:
        with pytest.raises(SystemExit):
            cli.parse_entry_args(mk(), ["--rank_group", "0", "--top_k", "-1"])
        assert "--top_k must be >= 0" in capsys.readouterr().err
        for flags in (["--top_k", "5", "--temperature", "0.6", "--sharded_sampling"], ["--B", "1", "--sampling_params", path]):
            with pytest.raises(SystemExit):
                cli.parse_entry_args(mk(), ["--rank_group", "0", "1"] + flags)
            err = capsys.readouterr().err
            assert "one rank only" in err and "no top-k" in err
        cli.parse_entry_args(mk(), ["--rank_group", "0", "1"])                      # greedy TP stays allowed


@pytest.mark.parametrize("rows,B,fragment", [
    ([{}, {}], 3, "exactly B = 3"), ([{}] * 4, 3, "exactly B = 3"), ({"temperature": 1}, 1, "exactly B = 1"),
    ("[{]", 1, "not JSON"),
    ([{"temp": 0.5}], 1, "keys among"), ([0.5], 1, "keys among"),
    ([{"temperature": -0.5}], 1, "temperature must be >= 0"), ([{"temperature": "hot"}], 1, "temperature must be >= 0"),
    ([{"top_p": 0}], 1, "top_p must be in (0, 1]"), ([{"top_p": 1.5}], 1, "top_p must be in (0, 1]"),
    ([{"top_k": -2}], 1, "top_k must be an integer >= 0"), ([{"top_k": 2.5}], 1, "top_k must be an integer >= 0"),
    ([{"top_k": True}], 1, "top_k must be an integer >= 0"),
])
def test_the_sampling_params_file_is_checked(tmp_path, capsys, rows, B, fragment):
    with pytest.raises(SystemExit):
        cli.parse_entry_args(cli.baseline_parser(), ["--rank_group", "0", "--B", str(B), "--sampling_params",
                                                     _file(tmp_path, rows)])
    assert fragment in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.parse_entry_args(cli.baseline_parser(), ["--rank_group", "0", "--sampling_params", str(tmp_path / "missing")])


def test_sampler_selection(monkeypatch, tmp_path):
    made = []

    class Fake:
        def __init__(self, *a, **k):
            made.append((type(self).__name__, a))

    monkeypatch.setattr(sampling, "Sampler", type("Sampler", (Fake,), {}))
    monkeypatch.setattr(sampling, "RequestSampler", type("RequestSampler", (Fake,), {}))
    engine = types.SimpleNamespace(model=types.SimpleNamespace(output=types.SimpleNamespace(weight=torch.zeros(100, 1)),
                                                               process_group=None))
    mk = cli.baseline_parser
    assert cli._sampler(cli.parse_entry_args(mk(), ["--rank_group", "0"]), engine, 3, "cpu") is None
    # neither new flag: exactly what it returned before -- a plain Sampler with the flags' values
    a = cli.parse_entry_args(mk(), ["--rank_group", "0", "--B", "2", "--temperature", "0.6", "--top_p", "0.9"])
    assert type(cli._sampler(a, engine, 3, "cpu")).__name__ == "Sampler"
    assert made[-1] == ("Sampler", (0.6, 0.9, a.seed, 2, 3, 100, "cpu"))
    a = cli.parse_entry_args(mk(), ["--rank_group", "0", "--B", "2", "--temperature", "0.6", "--top_k", "50"])
    assert type(cli._sampler(a, engine, 3, "cpu")).__name__ == "RequestSampler"
    assert made[-1] == ("RequestSampler", (0.6, 1.0, 50, a.seed, 2, 3, 100, "cpu"))
    path = _file(tmp_path, [{"temperature": 0.7}, {"top_k": 5}])
    a = cli.parse_entry_args(mk(), ["--rank_group", "0", "--B", "2", "--sampling_params", path])
    assert type(cli._sampler(a, engine, 3, "cpu")).__name__ == "RequestSampler"      # even with every flag at its default
    assert made[-1] == ("RequestSampler", ([0.7, 0.0], [1.0, 1.0], [0, 5], a.seed, 2, 3, 100, "cpu"))


# ------------------------------------------------------------------------------------ RequestSampler on the host
def test_request_sampler_validates_on_the_host_and_allows_set_params_after_capture():
    s = sampling.RequestSampler([0.0, 0.8, 1.5], 0.9, [0, 50, 7], 11, 3, 2, 64, "cpu")
    assert s.T.tolist() == [0.0, pytest.approx(0.8), 1.5] and s.K.tolist() == [0, 50, 7] and s.K.dtype == torch.int32
    assert s.P.dtype == torch.float32 and s.T.shape == s.P.shape == s.K.shape == (3,)
    ptrs = (s.T.data_ptr(), s.P.data_ptr(), s.K.data_ptr())
    s.captured = True
    s.set_params(0.0, [0.3, 1.0, 0.5], 0)                        # an all-greedy batch is legal; copied in place
    assert s.T.tolist() == [0.0] * 3 and s.K.tolist() == [0] * 3 and s.P.tolist() == [pytest.approx(0.3), 1.0, 0.5]
    assert ptrs == (s.T.data_ptr(), s.P.data_ptr(), s.K.data_ptr())
    for bad, match in (((-1.0, 0.9, 0), "temperature"), ((float("nan"), 0.9, 0), "temperature"), ((float("inf"), 0.9, 0), "temperature"),
                       ((1e-45, 0.9, 0), "temperature"), ((1e39, 0.9, 0), "temperature"), ((1e-39, 0.9, 0), "reciprocal"),
                       ((1.0, 0.0, 0), "top_p"),
                       ((1.0, 1.5, 0), "top_p"), ((1.0, 0.9, -1), "top_k"), ((1.0, 0.9, 2.5), "top_k"),
                       (([1.0, 1.0], 0.9, 0), "3 requests")):
        with pytest.raises(ValueError, match=match):
            s.set_params(*bad)
    assert s.T.tolist() == [0.0] * 3                             # a refused call changed nothing
    plain = sampling.Sampler(0.8, 0.9, 11, 3, 2, 64, "cpu")
    plain.captured = True
    with pytest.raises(AssertionError):                          # the scalar form keeps its assertion
        plain.set_params(0.7, 0.9)

    model = types.SimpleNamespace(output=types.SimpleNamespace(weight=torch.zeros(64, 1)), process_group=None)
    s.check_model(model)
    model.process_group = object()
    with pytest.raises(ValueError, match="TP = 1 only.*no top-k"):
        s.check_model(model)
    with pytest.raises(ValueError, match="vocabulary"):
        s.check_model(types.SimpleNamespace(output=types.SimpleNamespace(weight=torch.zeros(65, 1)), process_group=None))


# ------------------------------------------------------------------------------------ the wrappers' operand contract
def f32(*shape):
    return z(*shape, dtype=F32)


def req(o):
    """The operands of a test_ops_contract_cpu case with its scalar parameters replaced by [B] tensors."""
    o = dict(o)
    del o["temperature"], o["top_p"]
    B = o["tokens_buffer"].shape[0] if "tokens_buffer" in o else o["logits"].shape[0] // o["n"]
    return dict(o, temperature=f32(B), top_p=f32(B), top_k=i32(B))


CASES = {
    "sample_rows_req": (so.sample_rows_req, lambda: req(draw(**ring()))),
    "sample_rows_req_sel_out_no_k": (so.sample_rows_req, lambda: dict(req(draw(n=2, row_sel=z(1, dtype=I64),
                                                                               out=z(1, 2, dtype=I64))), top_k=None)),
    "spec_verify_sample_req": (so.spec_verify_sample_req, lambda: req(verify())),
    "spec_verify_sample_req_no_k": (so.spec_verify_sample_req, lambda: dict(req(verify()), top_k=None)),
}
ACCEPTED = {
    "sample_rows_req": ("md_sample_rows_req", ((2, 1), I64)),
    "sample_rows_req_sel_out_no_k": ("md_sample_rows_req", ((1, 2), I64)),
    "spec_verify_sample_req": ("md_spec_verify_sample_req", ((2, 2), I64)),
    "spec_verify_sample_req_no_k": ("md_spec_verify_sample_req", ((2, 2), I64)),
}
PARAMS = (("temperature", F32, torch.float64), ("top_p", F32, torch.bfloat16), ("top_k", I32, I64))
REFUSED = [
    *[(c, ValueError, f"{n} on the host", on_host(n)) for c in ("sample_rows_req", "spec_verify_sample_req")
      for n, _, _ in PARAMS],
    *[(c, TypeError, f"{n} as {other}", as_dtype(n, other)) for c in ("sample_rows_req", "spec_verify_sample_req")
      for n, _, other in PARAMS],
    *[(c, ValueError, f"{n} of 3", swap(**{n: lambda dt=dt: z(3, dtype=dt)}), n)
      for c in ("sample_rows_req", "spec_verify_sample_req") for n, dt, _ in PARAMS],
    *[(c, ValueError, f"{n} of shape [B, 1]", swap(**{n: lambda dt=dt: z(2, 1, dtype=dt)}), n)
      for c in ("sample_rows_req", "spec_verify_sample_req") for n, dt, _ in PARAMS],
    *[(c, ValueError, f"{n} strided", swap(**{n: lambda dt=dt: z(4, dtype=dt)[::2]}), n)
      for c in ("sample_rows_req", "spec_verify_sample_req") for n, dt, _ in PARAMS],
    *[(c, ValueError, f"{n} missing", swap(**{n: None}), "missing") for c in ("sample_rows_req", "spec_verify_sample_req")
      for n in ("temperature", "top_p")],
    *[(c, TypeError, f"{n} a Python number", swap(**{n: 0.8}), "tensor") for c in ("sample_rows_req", "spec_verify_sample_req")
      for n in ("temperature", "top_p")],
    # the operands shared with the scalar wrappers go through the same contracts
    ("sample_rows_req", ValueError, "logits float32", as_dtype("logits", F32)),
    ("sample_rows_req", ValueError, "logits on the host", on_host("logits")),
    ("sample_rows_req", ValueError, "counters of 2", swap(counters=lambda: i32(2))),
    ("sample_rows_req", ValueError, "ring of another vocabulary", swap(ring=lambda: z(2, 1, 32)), "ring"),
    ("sample_rows_req", ValueError, "a ring without stats", swap(ring_stats=None), "go together"),
    ("sample_rows_req_sel_out_no_k", ValueError, "row_sel int32", as_dtype("row_sel", I32)),
    ("sample_rows_req_sel_out_no_k", ValueError, "out of another shape", swap(out=lambda: z(2, 1, dtype=I64))),
    ("spec_verify_sample_req", ValueError, "tokens_buffer int32", as_dtype("tokens_buffer", I32)),
    ("spec_verify_sample_req", ValueError, "logits of other rows", swap(logits=lambda: z(6, 64))),
    ("spec_verify_sample_req", ValueError, "ring missing", swap(ring=None), "ring"),
    ("spec_verify_sample_req", ValueError, "ring of another vocabulary", swap(ring=lambda: z(2, 1, 32)), "vocabular"),
    ("spec_verify_sample_req", ValueError, "target_stats of other rows", swap(target_stats=lambda: z(2, 2, dtype=I64))),
    ("spec_verify_sample_req", ValueError, "ring_stats on the host", on_host("ring_stats")),
    ("spec_verify_sample_req", ValueError, "counters int64", as_dtype("counters", I64)),
]


def _call(rec, case, bad=None):
    fn, build = CASES[case]
    o = build()
    if bad is not None:
        o.update(bad(o))
    rec.calls.clear()
    return o, fn(**o)


def test_the_wrappers_are_the_public_callables_of_the_module():
    public = {n for n, f in vars(so).items() if callable(f) and not n.startswith("_") and not isinstance(f, type)
              and getattr(f, "__module__", None) == so.__name__}
    assert public == {fn.__name__ for fn, _ in CASES.values()} == {"sample_rows_req", "spec_verify_sample_req"}
    assert set(CASES) == set(ACCEPTED)


@pytest.mark.parametrize("case", list(ACCEPTED))
def test_accepted(monkeypatch, case):
    rec = install(monkeypatch)
    launch, (shape, dtype) = ACCEPTED[case]
    o, ret = _call(rec, case)
    assert [name for name, _ in rec.launches()] == [launch]
    assert tuple(ret.shape) == shape and ret.dtype == dtype
    if o.get("out") is not None:
        assert ret.data_ptr() == o["out"].data_ptr()
    args = rec.launches()[0][1]
    # the three parameter pointers are passed where the header has them (after vocab), top_k null when absent
    want = [o["temperature"].data_ptr(), o["top_p"].data_ptr(), o["top_k"].data_ptr() if o["top_k"] is not None else None]
    assert [a.value if a is not None else None for a in args[5:8]] == want


@pytest.mark.parametrize("row", REFUSED, ids=[f"{r[0]}-{r[2].replace(' ', '_')}" for r in REFUSED])
def test_refused(monkeypatch, row):
    rec = install(monkeypatch)
    case, exc, _, bad = row[:4]
    with pytest.raises(exc, match=row[4] if len(row) > 4 else getattr(bad, "match", None)):
        _call(rec, case, bad)
    assert rec.launches() == []


def test_refused_rows_are_distinct():
    ids = [(r[0], r[2]) for r in REFUSED]
    assert len(ids) == len(set(ids))


def test_signatures_match_the_header_argument_counts():
    from magicdec_amd import _lib
    assert _lib.ABI_VERSION == 12
    assert len(_lib._SIGNATURES["md_sample_rows_req"][1]) == len(_lib._SIGNATURES["md_sample_rows"][1]) + 1
    assert len(_lib._SIGNATURES["md_spec_verify_sample_req"][1]) == len(_lib._SIGNATURES["md_spec_verify_sample"][1]) + 1


# ------------------------------------------------------------------------------------ the masking helper
def _k11_kept(bits, T, top_p, k):
    """K11 "per request", stated directly: top-k by counting strictly larger keys, then top-p over the survivors' mass
    (float64 masses; the kept set and the margin of the top-p test)."""
    V = len(bits)
    key = sr.key16(bits).astype(np.int64)
    l = sr.bits_to_f(bits)
    w = np.exp((l - l.max()) * sr.inv_t(T))
    larger = np.array([(key > kv).sum() for kv in key])
    survive = larger < k if 1 <= k < V else np.ones(V, dtype=bool)
    if top_p >= 1:
        return survive, np.inf
    zk = w[survive].sum()
    above = np.array([w[survive & (key > kv)].sum() for kv in key])
    margin = float(np.min(np.abs(above[survive] - top_p * zk)) / zk)
    return survive & (above <= top_p * zk), margin


def test_masking_helper_agrees_with_the_direct_statement_of_top_k_then_top_p():
    rng = np.random.default_rng(2024)
    checked = close = 0
    for i in range(300):
        V = int(rng.choice([5, 17, 64, 200]))
        x = rng.normal(size=V).astype(np.float32) * float(rng.choice([0.5, 2.5]))
        kind = i % 5
        if kind == 1:
            x[rng.integers(0, V, size=V // 2)] = x[0]                   # tie groups, often across place k
        elif kind == 2:
            x[rng.integers(0, V, size=V // 2)] = -np.inf
            x[0] = 0.25
        elif kind == 3:
            x[:3] = [0.0, -0.0, -0.0]
        x = np.round(x * 4) / 4 if kind == 4 else x                     # coarse values: many ties
        T = float(rng.choice([0.05, 0.6, 1.0, 4.0]))
        top_p = float(rng.choice([0.3, 0.9, 1.0]))
        k = int(rng.choice([0, 1, 2, 3, V // 2, V - 1, V, V + 7, -1]))
        xb = torch.from_numpy(x).to(torch.bfloat16)
        bits = xb.view(torch.int16).numpy().view(np.uint16)
        masked, keep = topk_mask(xb, k)
        mbits = masked.view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(mbits[keep], bits[keep]) and (mbits[~keep] == 0xFF80).all()
        want, margin = _k11_kept(bits, T, top_p, k)
        f = sr.row_filter(mbits, T, top_p)
        if min(margin, f["margin"]) < sr.TOL:                           # the top-p test sits on its boundary
            close += 1
            continue
        assert np.array_equal(f["keep"] & keep, want), (i, V, T, top_p, k)
        # what row_filter keeps beyond the survivors are -inf entries of mass 0 (top_p = 1 keeps everything)
        assert (f["w"][f["keep"] & ~keep] == 0).all()
        checked += 1
    assert checked >= 250 and close <= 30

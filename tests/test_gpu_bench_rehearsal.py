"""The multi-rank path of bench.py END TO END on HIP kernels, on the one GPU the development boxes have (run with -m gpu).

No multi-GPU node was available to any round, so the first `bench.py --gpus 8` must not be the first time this code runs.
`MAGICDEC_TP_SINGLE_GPU=1` puts every rank on GPU 0 with gloo as the bootstrap transport (RCCL refuses two ranks per
device; gloo's collectives cannot be captured, so the steps run eagerly): the plain command launches its own ranks
(VERDICT r5 missing #2), every rank starts the collective child processes (RCCL-role = gloo against the xGMI kernels over HIP
IPC, write-through and release-fence arms, bit-exact stress), rank 0 selects the collective, the models are sharded
(target TP2, draft TP2), the xGMI all-reduce passes its probation inside the run, the loops run with the replayed AND
the measured acceptance, and one JSON line comes out.  (`profiles/r06_bench_tp2_on_one_gpu_rehearsal.json`)"""
import json
import os
import subprocess
import sys

import pytest

from tests.conftest import parity_report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_gpus_2_on_one_gpu():
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(MAGICDEC_TP_SINGLE_GPU="1", MAGICDEC_BENCH_LAYOUT_AB="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("MAGICDEC_ONESHOT_AR", None)              # let the run choose from its own collectives report
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "cfg3-small", "--steps",
                        "8", "--warmup", "2", "--no-cpu-baseline", "--no-pmc", "--full"], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-2000:] + p.stderr[-2000:]
    line = json.loads(lines[0])
    cfg = line["config"]
    assert line["n_gpus"] == 2 and line["rccl_ranks"] == 2 and line["collective_backend"] == "gloo"
    assert "TP2" in cfg["workload"] and cfg["hip_graphs"] is False and line["value"] > 0
    # The children's report.  Four processes share one GPU here, so a bounded spin MAY time out under a scheduling hiccup
    # (the run then selects the bootstrap backend and still completes: that is the design); what may never happen is a
    # wrong bit without a time-out.
    rep = line["collectives_us"]
    assert isinstance(rep, dict) and "verify" in rep, rep
    for key in ("xgmi_stress", "xgmi_fence_stress"):
        st = rep.get(key)
        if isinstance(st, dict) and st.get("timeouts_all_ranks", 1) == 0:
            assert st["mismatched_elements_all_ranks"] == 0 and st["calls"] >= 100, (key, st)
    if "xgmi_fused_add_rmsnorm_auto" in rep["verify"]:
        assert "xgmi_fence_fused_add_rmsnorm_auto" in rep["verify"]      # the third arm was measured beside it
    if cfg["allreduce"] == "oneshot-ipc":             # selected and kept: it passed its probation inside the run
        assert cfg["allreduce_probation"]["drop"] is False and cfg["allreduce_probation"]["calls"] >= 24
        assert cfg["allreduce_probation"]["mismatched_elements_max_over_ranks"] == 0 and cfg["allreduce_timeouts"] == 0
    # the sharded draft and the sharded target agree as often as the draft's construction says (8 rows: a loose band)
    sw = line["measured_acceptance_sweep"]
    assert sw["miss=0.2"]["tokens_per_iter_per_seq"] > sw["miss=0.4"]["tokens_per_iter_per_seq"] > 1.3
    assert 0.6 < sw["miss=0.2"]["alpha_equivalent"] <= 1.0
    parity_report(f"[bench rehearsal] 2 ranks on one GPU: allreduce={cfg['allreduce']} ({cfg['allreduce_selection'][:80]}...), "
                  f"probation={cfg['allreduce_probation']}, measured tokens/iteration at miss 0.4 / 0.3 / 0.2: "
                  f"{sw['miss=0.4']['tokens_per_iter_per_seq']} / {sw['miss=0.3']['tokens_per_iter_per_seq']} / "
                  f"{sw['miss=0.2']['tokens_per_iter_per_seq']}")

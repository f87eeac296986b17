"""Full-command integration: the launcher spawning run.py at world 2 on
CPU/gloo — the closest CPU analog of the reference README launch
(reference README.md:25).  This wiring (launcher env + run.py + train +
DDP + amp + Lookahead) is exactly what exposed the bucket-view desync:
per-rank valid metrics MUST be identical (unsharded validation keeps the
un-collectivized EarlyStopping/plateau in lockstep — SURVEY A.7)."""
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_launch_world2_trains_in_lockstep(tmp_path):
    env = dict(os.environ)
    env.update({"DDPX_SYNTH_SAMPLES": "256", "DDPX_NO_TQDM": "1"})
    out = subprocess.run(
        [sys.executable, "-m", "ddp_tricks_amd.launch",
         "--nproc_per_node=2", "--master_port=29699", "run.py",
         "-n=L2E", "-e=2", "-w=1", "-b=64",
         f"-d={tmp_path / 'no_data'}", f"-p={tmp_path}"],
        env=env, cwd=REPO, capture_output=True, text=True, timeout=280)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("epoch:")]
    assert len(lines) == 4, out.stdout  # 2 epochs x 2 ranks

    def metrics(ln):
        return dict(re.findall(r"(valid_loss|valid_acc|learning_rate):"
                               r" ([\d.e+-]+)", ln))

    by_epoch = {}
    for ln in lines:
        ep = ln.split(",")[0]
        by_epoch.setdefault(ep, []).append(metrics(ln))
    for ep, ms in by_epoch.items():
        assert len(ms) == 2, (ep, lines)
        # rank-identical validation metrics and LR (train metrics are
        # rank-local shard averages and may differ)
        assert ms[0] == ms[1], (ep, ms)
    # reference-style best checkpoint written by rank 0
    assert os.path.exists(os.path.join(tmp_path, "L2E.pt"))

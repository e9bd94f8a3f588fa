"""`python bench.py --gpus 2` starts its own two ranks (bench.launch_ranks) and reports
n_gpus 2 with the same CMC/mAP as one GPU.  On a one-GPU box the two ranks share cuda:0 over
gloo (`--backend gloo`: host collectives; RCCL needs one GPU per rank), so this runs the whole
multi-rank bench path — self-launch, world-size check, sharded embed, gallery all-gather,
per-rank eval rows gathered and reduced in query order, the per-rank timing record — that the
driver's 8-GPU run takes with torchrun and nccl."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = ["--steps", "1", "--warmup", "0"]  # a plain run: no leg beside the Market step (those need --full)


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args, *QUICK], capture_output=True,
                       text=True, timeout=240, cwd=REPO,
                       env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_two_ranks_self_launched_equal_one(gpu, tmp_path):
    import numpy as np
    one = _bench("--gpus", "1", "--dump-outputs", str(tmp_path))
    two = _bench("--gpus", "2", "--backend", "gloo")
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2
    # a plain run carries the headline and none of the --full legs
    assert one["steps"] == 1 and one["ms_per_step"] > 0 and one["unit"] == "imgs/s"
    assert not {"msmt17", "backend", "preprocess", "jpeg", "files_to_map", "rerank", "text", "cpu_baseline"} & set(one)
    # --dump-outputs: what the timed step returned, as the line reports it
    out = {f[:-4]: np.load(tmp_path / f, allow_pickle=False) for f in os.listdir(tmp_path)}
    assert sorted(out) == ["cmc", "distmat", "embeddings", "eval_rows", "mAP"]
    assert round(float(out["mAP"][0]), 6) == one["mAP"] and round(float(out["cmc"][0]), 6) == one["rank1"]
    assert out["eval_rows"].shape == (3368, 4) and out["distmat"].shape == (256, 15913)
    assert out["embeddings"].shape == (4096, 1280) and np.isfinite(out["embeddings"]).all()
    assert sum(v.nbytes for v in out.values()) <= 64 << 20
    assert two["config"]["parallelism"].startswith("dp2")
    assert two["mAP"] == one["mAP"] and two["rank1"] == one["rank1"]
    rk = two["ranks"]
    assert len(rk["embed_s"]) == 2 and len(rk["allgather_s"]) == 2
    # the gathered gallery: 15913 rows x (768 + 512) fp32
    assert rk["allgather_bytes"] == 15913 * 1280 * 4


def test_bench_world_size_must_match_gpus(gpu):
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", *QUICK], capture_output=True,
                       text=True, timeout=120, cwd=REPO, env=env)
    assert r.returncode != 0 and "WORLD_SIZE=1 but --gpus 2" in r.stderr

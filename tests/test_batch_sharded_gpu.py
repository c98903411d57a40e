"""GPU: batched rounds on the served, row-sharded database (ShardedFeatureDB.open(..., batch_rounds=True)) with the real kernels,
against a one-GPU FeatureDB over the same store (tests/_sharded_batch_broker.py).  The box has ONE card, so N > 1 is rehearsed with
every rank on it over gloo -- shards of 32/32 and 22/21/21 rows, ragged tiles on every rank -- and RCCL is exercised with one rank.
Process start-up dominates the run time, as in tests/test_sharded_db_gpu.py."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("world,backend", [(2, "gloo"), (3, "gloo"), (1, "nccl")])
def test_batched_rounds_on_served_shards_equal_one_gpu(gpu, world, backend):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_sharded_batch_broker.py"), str(world), backend], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:]

"""GPU: a group's whole weight update as ONE operation of the served, row-sharded database (ShardedFeatureDB.batch_round_update on
ShardedFeatureDB.open(..., batch_rounds=True)) with the real kernels, against FeatureDB.batch_round_update on a one-GPU database over
the same store (tests/_sharded_update_broker.py): every array of the update, the ranking behind it, and the Ticket seam with
fit_on_device and a finalize ticket.  The box has ONE card, so N > 1 is rehearsed with every rank on it over gloo -- shards of 32/32
and 22/21/21 rows -- and RCCL is exercised with one rank; nothing here has crossed a second card.  Process start-up dominates the run
time, as in tests/test_batch_sharded_gpu.py."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("world,backend", [(2, "gloo"), (3, "gloo"), (1, "nccl")])
def test_the_update_on_served_shards_equals_one_gpu(gpu, world, backend):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_sharded_update_broker.py"), str(world), backend], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:]

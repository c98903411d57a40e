"""Test program (GPU box): a float16 ShardedFeatureDB over RCCL with ONE rank against a plain float16 FeatureDB, bit for bit on one
round (query from a resident row, scan, similarities, scores, selection, top-k) and on the rows read back.  Prints ``ok``."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    n = 2051
    import torch
    import torch.distributed as dist
    import video_query_algorithms_amd as vqa
    from video_query_algorithms_amd.shard import all_gather_rows
    from video_query_algorithms_amd.sharded_db import ShardedFeatureDB
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29578")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        sdb = ShardedFeatureDB.synthetic(n, 2, 3, 1024, seed=5, dtype=np.float16)
        one = vqa.FeatureDB.synthetic(n, 2, 3, 1024, seed=5, dtype=np.float16)
        assert sdb.dtype == np.float16
        t = one.set_query_from_row(11)
        one.scan(weights=[1.0, 1.5])
        assert (sdb.set_query_from_row(11) == t).all()
        sdb.scan(weights=[1.0, 1.5])
        avg_s, ne_s = sdb.similarities()
        avg_o, ne_o = one.similarities()
        assert (avg_s == avg_o).all() and (ne_s == ne_o).all()
        assert (sdb.scores() == one.scores()).all()
        sel_s, sel_o = sdb.select(0.8, 0.7), one.select(0.8, 0.7)
        assert all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(sel_s[:2], sel_o[:2])) and sel_s[2] == sel_o[2]
        top_s, top_o = sdb.topk(20), one.topk(20)
        assert (top_s[0] == top_o[0]).all() and (top_s[1] == top_o[1]).all()
        rows = [0, 11, 1000, n - 1]
        got = sdb.read_rows(rows)
        assert got.dtype == np.float16 and (got.view(np.uint16) == one.read_rows(rows).view(np.uint16)).all()
        # the feature all-gather takes half-precision blocks as they are
        block = torch.from_numpy(one.read_rows(rows)).cuda()
        assert all_gather_rows(block, len(rows)).dtype == torch.float16 and torch.equal(all_gather_rows(block, len(rows)), block)
        sdb.close()
        one.close()
    finally:
        dist.destroy_process_group()
    print("ok", flush=True)


if __name__ == "__main__":
    main()

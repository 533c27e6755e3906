"""host-side pieces of bench.py that only run with several ranks: the collective log (wraps torch.distributed's collectives, async Work handles
included) -- exercised here on CPU with a one-rank gloo group and a dummy event clock."""
import os
import sys
import time

import torch
import torch.distributed as dist

from conftest import ROOT

sys.path.insert(0, ROOT)


class _Clock:
    def record(self):
        self.t = time.perf_counter()

    def elapsed_time(self, other):
        return 1e3 * (other.t - self.t)


def test_collective_log_counts_blocking_and_async_collectives():
    import bench
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29577")
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        x, out = torch.ones(8), torch.empty(8)
        with bench._CollectiveLog(event_factory=_Clock) as log:
            for _ in range(2):
                dist.all_reduce(x)
                w = dist.all_reduce(x, async_op=True)
                dist.all_gather_into_tensor(out, x)
                w.wait()
                assert w.is_completed()                       # (the proxy forwards everything else)
        assert dist.all_reduce.__module__ != "bench"          # restored
        s = log.summary(2)
        assert s["per_step"] == 3
        rows = s["by_kind_and_payload"]
        assert rows["all_reduce:32B"]["per_step"] == 1 and rows["all_reduce(async):32B"]["per_step"] == 1 and rows["all_gather_into_tensor:32B"]["per_step"] == 1
        assert all(r["mean_us_stream_held"] is not None and r["mean_us_stream_held"] >= 0 for r in rows.values())
        assert s["sum_us_stream_held_per_step"] >= 0
    finally:
        dist.destroy_process_group()


def test_dump_outputs_writes_the_step_outputs_and_the_model_state_as_float_arrays(tmp_path):
    """--dump-outputs: one .npy per array, float32 / float64 only, a fixed row sample of an embedding matrix above DUMP_MAX_ROWS"""
    import numpy as np
    import bench
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    model.add_module("key_projection", torch.nn.Linear(2, 2))          # its bias is left out (see bench.dump_outputs)
    feats = torch.randn(bench.DUMP_MAX_ROWS + 5, 4)
    for d in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(str(d), feats, torch.tensor(1.5), torch.tensor([7], dtype=torch.int32), model)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(["embeddings.npy", "loss.npy", "train_correct.npy"] + [f"state.{k}.npy" for k in model.state_dict() if k != "key_projection.bias"])
    arrays = {n: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    e = arrays["embeddings.npy"]
    assert e.shape == (bench.DUMP_MAX_ROWS, 4) and np.array_equal(e, np.load(tmp_path / "b" / "embeddings.npy"))
    assert np.isin(e[:, 0], feats[:, 0].numpy()).all()
    assert float(arrays["loss.npy"]) == 1.5 and arrays["train_correct.npy"].dtype == np.float64 and arrays["train_correct.npy"][0] == 7
    np.testing.assert_array_equal(arrays["state.0.weight.npy"], model[0].weight.detach().numpy())
    assert arrays["state.1.num_batches_tracked.npy"].dtype == np.float64

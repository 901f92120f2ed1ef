"""cdr_dist.sharded_global_medians on CPU: gloo, world sizes 1-3, each rank's
device context replaced by a NumPy double of the pass protocol (global row
count -> per pass: local digit histograms, SUM all-reduce, digit selection),
against np.median of every column of the union (src/main.py:31-38,
src/scoring.py:50-54)."""
import os

import numpy as np
import pytest

from test_features_dist import _free_port
from test_medians_dist import NumpyMedians


class NumpyGlobalMedians:
    """Test double with the _cdr.Context global-median surface (fp64 keys):
    the cluster double with one cluster that holds every row."""

    def __init__(self, X, mode=2):
        self.X, self._mode = X, mode
        self._m = NumpyMedians(X, np.zeros(X.shape[0], dtype=np.int64))
        self.calls = []

    def info(self):
        return {"n": self.X.shape[0], "d": self.X.shape[1], "mode": self._mode, "scale_bits": 0}

    def medians_global(self):
        self.calls.append("whole")
        return self._m.medians_by_label(1)[0]

    def medians_global_begin(self, n_total):
        self.calls.append("begin")
        self._m.k = 1
        passes, words = self._m.medians_begin(np.array([n_total], dtype=np.int64))
        assert words == self.X.shape[1] * 512
        return passes, words

    def medians_global_pass_hist(self, p, hist):
        self._m.medians_pass_hist(p, hist)

    def medians_global_pass_select(self, p, hist):
        self._m.medians_pass_select(p, hist)

    def medians_global_finish(self):
        return self._m.medians_finish()[0]


def _data():
    rng = np.random.default_rng(4)
    X = rng.normal(0, 2, (3000, 3))
    X[::5, 1] = 0.25
    X[::2, 2] = -0.0      # the middle of column 2: -0.0 | +0.0
    X[1::2, 2] = np.where(rng.random(1500) < 0.5, 0.0, 1.5)
    return X


def _bounds(world, n, empty):
    """Row ranges per rank; with `empty`, rank 1 holds no rows."""
    cut = [(n * r) // world for r in range(world + 1)]
    if empty and world > 1:
        cut[1] = cut[2]
    return cut


def _worker(rank, world, port, out_dir, empty):
    import torch.distributed as dist

    from cdr_dist import Comm, sharded_global_medians

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    X = _data()
    cut = _bounds(world, X.shape[0], empty)
    stand = NumpyGlobalMedians(X[cut[rank]:cut[rank + 1]])
    med = sharded_global_medians(stand, Comm(dist, None))
    assert stand.calls == ["begin"]
    np.save(os.path.join(out_dir, f"g{rank}.npy"), med)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,empty", [(1, False), (2, False), (3, False), (2, True), (3, True)])
def test_sharded_global_medians_equal_numpy(tmp_path, world, empty):
    X = _data()
    exp = np.median(X, axis=0)
    assert exp[2] == 0 and not np.signbit(exp[2])
    if world == 1:
        from cdr_dist import Comm, sharded_global_medians

        stand = NumpyGlobalMedians(X)
        got = [sharded_global_medians(stand, Comm(None))]
        assert stand.calls == ["whole"]  # one shard: the histograms never leave the device
    else:
        if empty:
            cut = _bounds(world, X.shape[0], True)
            assert cut[2] - cut[1] == 0
        mp = pytest.importorskip("torch.multiprocessing")
        mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), empty), nprocs=world, join=True)
        got = [np.load(tmp_path / f"g{r}.npy") for r in range(world)]
    for g in got:
        np.testing.assert_array_equal(g, exp)
        np.testing.assert_array_equal(np.signbit(g), np.signbit(exp))


def _mode_worker(rank, world, port, out_dir):
    import torch.distributed as dist

    from cdr_dist import Comm, sharded_global_medians

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    X = _data()
    lo, hi = (X.shape[0] * rank) // world, (X.shape[0] * (rank + 1)) // world
    # rank 0 reports F32X (mode 1), rank 1 F64 (mode 2); the stand-in always
    # does 8 passes, so a library without the check returns instead of hanging
    msg = "returned"
    try:
        sharded_global_medians(NumpyGlobalMedians(X[lo:hi], mode=1 + rank), Comm(dist, None))
    except RuntimeError as e:
        msg = "RuntimeError: %s" % e
    with open(os.path.join(out_dir, f"gmode{rank}.txt"), "w") as fh:
        fh.write(msg)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_global_medians_refuse_mixed_modes(tmp_path):
    """One rank F32X, the other F64: both raise together before the first
    pass (neither is left waiting in a collective) and name unify_points."""
    mp = pytest.importorskip("torch.multiprocessing")
    mp.spawn(_mode_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        msg = (tmp_path / f"gmode{r}.txt").read_text()
        assert msg.startswith("RuntimeError"), (r, msg)
        assert "unify_points" in msg, (r, msg)

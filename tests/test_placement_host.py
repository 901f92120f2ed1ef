"""replica_placement.placement_host, the definition of the replica placement
(CPU): against a plain Python loop over the events, a hand-written case, the
golden pipeline's counts and the invariants."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

PDIR = os.path.join(GOLDEN, "pipeline")


def loop_placement(f, c, prim, n_nodes, factor, R, sizes=None):
    """The module docstring, one event and one file at a time."""
    nf = len(prim)
    cnt = [[0] * n_nodes for _ in range(nf)]
    total = [0] * nf
    for fi, ci in zip(f, c):
        if fi < 0 or fi >= nf:
            continue
        total[fi] += 1
        if 0 <= ci < n_nodes:
            cnt[fi][ci] += 1
    nodes, per_file = [], []
    rep, nbytes = [0] * n_nodes, [0] * n_nodes
    for i in range(nf):
        p = int(prim[i])
        pv = 0 <= p < n_nodes
        rest = sorted((j for j in range(n_nodes) if not (pv and j == p)),
                      key=lambda j: (-cnt[i][j], j))
        order = ([p] if pv else []) + rest
        chosen = order[:min(int(factor[i]), n_nodes)]
        nodes.append(chosen + [-1] * (R - len(chosen)))
        per_file.append([total[i], cnt[i][p] if pv else 0, sum(cnt[i][j] for j in chosen)])
        for j in chosen:
            rep[j] += 1
            if sizes is not None:
                nbytes[j] += int(sizes[i])
    return nodes, per_file, cnt, rep, nbytes


@pytest.mark.parametrize("seed", range(12))
def test_against_the_loop(seed):
    from replica_placement import placement_host

    rng = np.random.default_rng(seed)
    nf, n_nodes = int(rng.integers(1, 40)), int(rng.integers(1, 9))
    R = int(rng.integers(1, 9))
    ne = int(rng.integers(0, 600))
    f = rng.integers(-1, nf + 1, ne)                  # -1 and nf: not in the manifest
    c = rng.integers(-3, n_nodes + 2, ne)             # null, no datanode, past the nodes
    if seed % 3 == 0:
        c = rng.integers(0, min(2, n_nodes), ne)      # many ties
    prim = rng.integers(-2, n_nodes + 1, nf)
    factor = rng.integers(0, R + 1, nf)
    sizes = rng.integers(0, 2 ** 62, nf)
    k = 5
    labels = rng.integers(0, k, nf)
    got = placement_host(f, c, prim, n_nodes, factor, R, sizes=sizes, labels=labels, k=k)
    nodes, per_file, cnt, rep, nbytes = loop_placement(f, c, prim, n_nodes, factor, R, sizes)
    assert got["nodes"].dtype == np.int32 and got["nodes"].tolist() == nodes
    assert got["per_file"].tolist() == per_file
    assert got["counts"].tolist() == cnt
    assert got["node_replicas"].tolist() == rep
    assert got["node_bytes"] == nbytes
    cs = [[sum(per_file[i][col] for i in range(nf) if labels[i] == j) for col in range(3)]
          for j in range(k)]
    assert got["cluster_sums"].tolist() == cs
    assert placement_host(f, c, prim, n_nodes, factor, R)["node_bytes"] == [0] * n_nodes


def test_hand_written_six_files():
    from replica_placement import placement_host

    # three nodes; (file, client) events
    ev = ([(0, 1)] * 3 + [(0, 2)] * 3 + [(0, 0)] * 1      # file 0: tie between nodes 1 and 2
          + [(1, 2)] * 4 + [(1, 0)] * 2                    # file 1: null primary
          + [(2, 1)] * 5 + [(2, 2)] * 1                    # file 2: primary 0 has no access
          + [(4, 0)] * 2 + [(4, 1)] * 7                    # file 4: factor 0
          + [(5, 2)] * 2 + [(5, 1)] * 1 + [(5, -1)] * 4    # file 5: factor 5 > 3 nodes
          + [(-1, 0)] * 3)                                 # a path that is not in the manifest
    f = np.array([e[0] for e in ev])
    c = np.array([e[1] for e in ev])
    prim = np.array([0, -2, 0, 1, 0, 1])
    factor = np.array([2, 2, 2, 3, 0, 5])
    got = placement_host(f, c, prim, 3, factor, 5)
    assert got["nodes"].tolist() == [
        [0, 1, -1, -1, -1],     # the primary, then the lower id of the tie
        [2, 0, -1, -1, -1],     # no primary: by count
        [0, 1, -1, -1, -1],     # the primary first although nobody read from it
        [1, 0, 2, -1, -1],      # no events: the primary, then the ids in order
        [-1, -1, -1, -1, -1],   # factor 0
        [1, 2, 0, -1, -1],      # factor 5 of 3 nodes: all of them, then -1
    ]
    assert got["per_file"].tolist() == [[7, 1, 4], [6, 0, 6], [6, 0, 5], [0, 0, 0], [9, 2, 0],
                                        [7, 1, 3]]
    assert got["node_replicas"].tolist() == [5, 4, 3]


def test_golden_pipeline_counts():
    import compute_features as cf
    from replica_placement import placement_host

    paths, _, primary = cf.load_manifest(os.path.join(PDIR, "metadata.csv"))
    f, _, c, _, prim = cf.encode(paths, primary, *cf.load_access_log(os.path.join(PDIR,
                                                                                 "access.log")))
    n_nodes = len(cf.encode_primary(primary)[1])
    counts = np.load(os.path.join(PDIR, "features_oracle.npz"))["counts"]
    factor = np.arange(len(paths)) % 4
    got = placement_host(f, c, prim, n_nodes, factor, 3)
    np.testing.assert_array_equal(got["per_file"][:, 1], counts[:, 3])  # local_accesses
    np.testing.assert_array_equal(got["per_file"][:, 0], counts[:, 0])  # access_freq
    sel = (prim >= 0) & (prim < n_nodes) & (factor >= 1)
    assert sel.any() and (got["per_file"][sel, 2] >= got["per_file"][sel, 1]).all()
    assert (got["per_file"][factor >= 2, 2] > got["per_file"][factor >= 2, 1]).any()


def test_every_access_local_with_a_replica_on_every_node():
    from replica_placement import placement_host

    rng = np.random.default_rng(3)
    nf, n_nodes = 30, 5
    f = rng.integers(0, nf, 2000)
    c = rng.integers(0, n_nodes, 2000)
    prim = rng.integers(-2, n_nodes, nf)
    got = placement_host(f, c, prim, n_nodes, rng.integers(5, 8, nf), 7)
    np.testing.assert_array_equal(got["per_file"][:, 2], got["per_file"][:, 0])
    assert (np.sort(got["nodes"][:, :5], axis=1) == np.arange(5)).all()
    assert (got["nodes"][:, 5:] == -1).all()


def test_arguments():
    from replica_placement import placement_host

    e = np.zeros(0, dtype=np.int64)
    with pytest.raises(NotImplementedError):
        placement_host(e, e, [0], 65, [1], 1)
    with pytest.raises(NotImplementedError):
        placement_host(e, e, [0], 0, [1], 1)
    with pytest.raises(ValueError):
        placement_host(e, e, [0], 2, [2], 1)
    with pytest.raises(ValueError):
        placement_host(e, e, [0], 2, [1], 9)
    with pytest.raises(ValueError):
        placement_host(e, e, [0], 2, [1], 1, sizes=[-1])
    got = placement_host(e, e, [1], 2, [2], 2)
    assert got["nodes"].tolist() == [[1, 0]] and got["per_file"].tolist() == [[0, 0, 0]]

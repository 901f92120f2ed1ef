"""The evaluation of a given placement on the host (replica_placement.py):
evaluate_host against a plain-Python loop, its identities with placement_host,
its input cases, the placement CSV round trip and the summary arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

from replica_placement import (_eval_summary, evaluate_host, placement_host, read_placement_csv,
                               summary_json, write_placement_csv)

# (n_nodes, n_files, events, R, k)
SHAPES = [(1, 5, 300, 1, 1), (3, 700, 60000, 3, 4), (64, 300, 40000, 8, 9), (5, 50, 2000, 8, 1024)]


def loops(file_idx, op, client, nodes, n_nodes, labels, k):
    """The definition, one event at a time."""
    nf = len(nodes)
    mask, first, copies = [], [], []
    for row in nodes:
        m, fi = 0, -1
        for v in row:
            if v >= 0:
                m |= 1 << int(v)
                if fi < 0:
                    fi = int(v)
        mask.append(m)
        first.append(fi)
        copies.append(bin(m).count("1"))
    pf = [[0, 0] for _ in range(nf)]
    cs = [[0] * 6 for _ in range(k)]
    ns = [[0] * 5 for _ in range(n_nodes)]
    for f, o, c in zip(file_idx, op, client):
        f, o, c = int(f), int(o), int(c)
        if not 0 <= f < nf:
            continue
        node = 0 <= c < n_nodes
        inn = node and bool(mask[f] >> c & 1)
        row = cs[int(labels[f])]
        pf[f][0] += 1
        row[0] += 1
        if inn:
            pf[f][1] += 1
            row[1] += 1
        if node:
            ns[c][0] += 1
            ns[c][1] += inn
        if o == 2:
            row[2] += 1
            row[3] += inn
            srv = c if inn else first[f]
            if srv >= 0:
                ns[srv][2] += 1
        if o == 1:
            row[4] += 1
            row[5] += copies[f]
            for j in range(n_nodes):
                ns[j][3] += mask[f] >> j & 1
    for f in range(nf):
        for j in range(n_nodes):
            ns[j][4] += mask[f] >> j & 1
    return np.array(pf).reshape(nf, 2), np.array(cs), np.array(ns)


def inputs(rng, n_nodes, nf, ne, R):
    f = rng.integers(-1, nf + 2, ne)
    op = rng.integers(0, 3, ne)
    cl = rng.choice(np.concatenate([np.arange(n_nodes), [-3, -1, n_nodes, 200]]), ne)
    nodes = rng.integers(-1, n_nodes, (nf, R))
    nodes[rng.random(nf) < 0.1] = -1
    return f, op, cl, nodes


@pytest.mark.parametrize("n_nodes,nf,ne,R,k", [(1, 5, 300, 1, 1), (3, 40, 3000, 3, 4),
                                               (64, 30, 4000, 8, 9), (5, 20, 2000, 8, 1024)])
def test_against_the_loops(n_nodes, nf, ne, R, k):
    rng = np.random.default_rng(n_nodes)
    f, op, cl, nodes = inputs(rng, n_nodes, nf, ne, R)
    labels = rng.integers(0, k, nf)
    got = evaluate_host(f, op, cl, nodes, n_nodes, labels=labels, k=k)
    pf, cs, ns = loops(f, op, cl, nodes, n_nodes, labels, k)
    np.testing.assert_array_equal(got["per_file"], pf)
    np.testing.assert_array_equal(got["cluster_sums"], cs)
    np.testing.assert_array_equal(got["node_sums"], ns)
    assert got["unserved_reads"] == cs[:, 2].sum() - ns[:, 2].sum()
    for key in ("per_file", "cluster_sums", "node_sums"):
        assert got[key].dtype == np.int64
    # without labels: one cluster
    one = evaluate_host(f, op, cl, nodes, n_nodes)
    np.testing.assert_array_equal(one["cluster_sums"], cs.sum(axis=0, keepdims=True))


@pytest.mark.parametrize("n_nodes,nf,ne,R,k", SHAPES)
def test_identities_with_placement_host(n_nodes, nf, ne, R, k):
    rng = np.random.default_rng(nf)
    f, op, cl, _ = inputs(rng, n_nodes, nf, ne, R)
    prim = rng.integers(-2, n_nodes + 1, nf)          # -2: null, n_nodes: no node
    labels = rng.integers(0, k, nf)
    factor = rng.integers(0, R + 1, nf)
    exp = placement_host(f, cl, prim, n_nodes, factor, R, labels=labels, k=k)
    # I1: the placement's own nodes on the same events
    got = evaluate_host(f, op, cl, exp["nodes"], n_nodes, labels=labels, k=k)
    np.testing.assert_array_equal(got["per_file"][:, 0], exp["per_file"][:, 0])
    np.testing.assert_array_equal(got["per_file"][:, 1], exp["per_file"][:, 2])
    np.testing.assert_array_equal(got["cluster_sums"][:, 0:2], exp["cluster_sums"][:, [0, 2]])
    np.testing.assert_array_equal(got["node_sums"][:, 4], exp["node_replicas"])
    # I3
    assert got["node_sums"][:, 1].sum() == got["cluster_sums"][:, 1].sum()
    # I2: the primary alone
    only = np.where((prim >= 0) & (prim < n_nodes), prim, -1).reshape(nf, 1)
    got = evaluate_host(f, op, cl, only, n_nodes, labels=labels, k=k)
    np.testing.assert_array_equal(got["per_file"][:, 1], exp["per_file"][:, 1])
    assert got["node_sums"][:, 1].sum() == got["cluster_sums"][:, 1].sum()


def test_input_cases_by_hand():
    n_nodes = 4
    nodes = np.array([[2, 2, 0],      # a duplicate counts once: mask {0, 2}, first 2
                      [-1, 3, 1],     # a -1 in front: first is 3
                      [-1, -1, -1],   # no replica: its reads are unserved
                      [1, -1, 1]])
    ev = [(0, 2, 2), (0, 2, 0), (0, 2, 1), (0, 1, 3), (0, 0, 2),
          (1, 2, 0), (1, 2, 1), (1, 1, 1), (1, 2, -1), (1, 2, -3), (1, 2, 4), (1, 2, 200),
          (2, 2, 0), (2, 2, 1), (2, 1, 2), (2, 0, 3),
          (3, 1, 1), (3, 1, 0),
          (-1, 2, 0), (4, 2, 0), (7, 1, 1)]
    f, op, cl = (np.array(v) for v in zip(*ev))
    got = evaluate_host(f, op, cl, nodes, n_nodes, labels=[0, 1, 1, 0], k=2)
    assert got["per_file"].tolist() == [[5, 3], [7, 2], [4, 0], [2, 1]]
    # events, local, reads, reads_local, writes, write_copies
    assert got["cluster_sums"].tolist() == [[7, 4, 3, 2, 3, 2 + 1 + 1], [11, 2, 8, 1, 2, 2 + 0]]
    # issued, local, reads_served, writes_received, replicas
    #   reads served: file 0 by 2, 0 and (client 1, not local) by first = 2;
    #   file 1 by client 1 once, the five others by first = 3; file 2 by nobody
    assert got["node_sums"].tolist() == [[4, 1, 1, 1, 1],
                                         [5, 3, 1, 1 + 2, 2],
                                         [3, 2, 2, 1, 1],
                                         [2, 0, 5, 1, 1]]
    assert got["unserved_reads"] == 2
    pf, cs, ns = loops(f, op, cl, nodes, n_nodes, [0, 1, 1, 0], 2)
    assert pf.tolist() == got["per_file"].tolist() and ns.tolist() == got["node_sums"].tolist()


def test_errors():
    e = np.zeros(0, dtype=np.int64)
    with pytest.raises(ValueError):
        evaluate_host(e, e, e, [[3]], 3)
    with pytest.raises(ValueError):
        evaluate_host(e, e, e, [[-2]], 3)
    with pytest.raises(ValueError):
        evaluate_host(e, e, e, np.zeros((2, 9), dtype=int), 3)
    with pytest.raises(ValueError):
        evaluate_host(e, e, e, [[0], [1]], 3, labels=[0, 2], k=2)
    with pytest.raises(ValueError):
        evaluate_host(e, e, e, [[0], [1]], 3, labels=[0], k=2)
    with pytest.raises(NotImplementedError):
        evaluate_host(e, e, e, [[0]], 65)
    with pytest.raises(NotImplementedError):
        evaluate_host(e, e, e, [[0]], 3, labels=[0], k=1025)
    got = evaluate_host(e, e, e, [[0], [1]], 3, labels=[0, 1], k=2)
    assert not got["per_file"].any() and got["node_sums"][:, 4].tolist() == [1, 1, 0]


def test_placement_csv_round_trip(tmp_path):
    names = ["dn1", "dn2", "dn_3", "dn4"]
    paths = ["/a/b", "/a,c", '/q"uote', "/none", "/last"]
    nodes = np.array([[0, 2, -1], [3, -1, -1], [1, 0, 3], [-1, -1, -1], [2, -1, -1]],
                     dtype=np.int32)
    out = str(tmp_path / "p.csv")
    assert write_placement_csv(out, paths, [2, 1, 3, 0, 1], nodes, names) == 5
    back = read_placement_csv(out, paths, names)
    assert back.dtype == np.int32
    np.testing.assert_array_equal(back, nodes)
    # aligned by path; a path the file does not list gets an all -1 row
    other = ["/last", "/missing", "/a/b"]
    np.testing.assert_array_equal(read_placement_csv(out, other, names),
                                  [[2, -1, -1], [-1, -1, -1], [0, 2, -1]])
    # R is the widest row, at least 1
    write_placement_csv(out, paths[:2], [0, 0], np.full((2, 3), -1), names)
    assert read_placement_csv(out, paths[:2], names).tolist() == [[-1], [-1]]

    def write(rows):
        with open(out, "w") as fh:
            fh.write("path,replication,nodes\n" + "".join(r + "\n" for r in rows))

    write(["/a/b,1,dn9"])
    with pytest.raises(ValueError, match="unknown node"):
        read_placement_csv(out, paths, names)
    write(["/a/b,1,dn1", "/a/b,1,dn2"])
    with pytest.raises(ValueError, match="twice"):
        read_placement_csv(out, paths, names)
    write(["/a/b,9," + ";".join(["dn1"] * 9)])
    with pytest.raises(ValueError, match="above 8"):
        read_placement_csv(out, paths, names)
    write(["/a/b,8," + ";".join(["dn1", "dn2"] * 4)])
    assert read_placement_csv(out, ["/a/b"], names).tolist() == [[0, 1] * 4]


def test_summary_arithmetic():
    cs = np.array([[10, 4, 6, 3, 2, 6],
                   [5, 5, 0, 0, 5, 5],
                   [0, 0, 0, 0, 0, 0],
                   [8, 2, 8, 2, 0, 0]])
    ns = np.array([[12, 6, 9, 4, 3], [11, 5, 3, 3, 2]])
    s = _eval_summary(cs, ns, ["Hot", "Shared", "Cold", "Hot"], [3, 2, 1, 3])
    assert s["events"] == 23 and s["local"] == 11 and s["locality"] == Fraction(11, 23)
    assert s["reads"] == 14 and s["reads_local"] == 5 and s["read_locality"] == Fraction(5, 14)
    assert s["writes"] == 7 and s["write_copies"] == 11
    assert s["write_amplification"] == Fraction(11, 7)
    assert s["write_amplification_float"] == 11 / 7 and s["locality_float"] == 11 / 23
    hot = s["categories"]["Hot"]
    assert hot["clusters"] == [0, 3] and hot["factor"] == 3 and hot["events"] == 18
    assert hot["read_locality"] == Fraction(5, 14) and hot["write_amplification"] == 3
    sh = s["categories"]["Shared"]
    assert sh["read_locality"] is None and sh["read_locality_float"] is None
    assert sh["locality"] == 1 and sh["write_amplification"] == 1
    cold = s["categories"]["Cold"]
    assert cold["locality"] is None and cold["write_amplification"] is None
    assert cold["write_amplification_float"] is None and cold["events"] == 0
    assert s["nodes"] == [{"issued": 12, "local": 6, "reads_served": 9, "writes_received": 4,
                           "replicas": 3},
                          {"issued": 11, "local": 5, "reads_served": 3, "writes_received": 3,
                           "replicas": 2}]
    assert s["unserved_reads"] == 2
    assert s["read_load_imbalance"] == Fraction(9 * 2, 12) and s["read_load_imbalance_float"] == 1.5
    assert all(isinstance(s[key], int) for key in ("events", "local", "reads", "write_copies"))
    j = summary_json(s)
    assert j["locality"] == "11/23" and j["categories"]["Cold"]["locality"] is None
    assert j["read_load_imbalance"] == "3/2" and j["nodes"][0]["reads_served"] == 9
    import json
    json.dumps(j)
    # no events at all, and no read served
    z = _eval_summary(np.zeros((1, 6), dtype=np.int64), np.zeros((3, 5), dtype=np.int64), ["Hot"],
                      [3])
    assert z["locality"] is None and z["read_locality"] is None
    assert z["write_amplification"] is None and z["read_load_imbalance"] is None
    assert z["read_load_imbalance_float"] is None and z["unserved_reads"] == 0

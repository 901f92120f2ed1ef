"""Where each file's replicas go: on the nodes that read the file.

An extension with no counterpart in the reference, which stops at a replication
factor per category (src/main.py:92).  A plan that raises a hot file from 1 to
3 copies gains nothing when the new copies land on nodes that never read it.
Every event of the access log carries its client node, the manifest gives each
file's primary node; from them, per file f::

    cnt[f][j]  = events of f whose client is node j       (0 <= j < n_nodes)
    total[f]   = all events of f
    order(f)   = primary[f] first (when 0 <= primary[f] < n_nodes), then the
                 other nodes by descending cnt[f][j], ties to the lower id
                 (nodes nobody read from follow in id order)
    nodes[f]   = the first min(factor[f], n_nodes) of order(f), then -1 up to R
    local_before[f] = cnt[f][primary[f]]                  (0 without a primary)
    local_after[f]  = sum of cnt[f][j] over nodes[f]

Events of a path that is not in the manifest (file_idx < 0) are ignored; a
client that is no node (negative, or >= n_nodes) counts in total[f] only.  The
placement is greedy per file: the node balance is reported, not enforced.

``placement_host`` is the definition (NumPy, no GPU).  ``place`` gives the same
integers from libcdr.so (csrc/place.hip) over the events resident in the
context, with the labels of the last assignment never leaving the device.  All
of it is integer sums, so the two agree with ``==``.

``place`` reports the locality "after" on the log the placement was fitted to.
``evaluate_host`` / ``evaluate`` (csrc/place_eval.hip) judge a GIVEN placement,
yesterday's or one the project did not compute, on the resident events: the
local share of all accesses and of the reads, the write copies every replica
costs, and per node the reads it would serve and the writes it would receive.
``read_placement_csv`` reads back what ``write_placement_csv`` wrote.
"""
from __future__ import annotations

import csv
from fractions import Fraction

import numpy as np

from _cdr import Context, default_context

__all__ = ["placement_host", "place", "place_from_log", "write_placement_csv", "MAX_R",
           "MAX_NODES", "evaluate_host", "evaluate", "evaluate_from_log", "read_placement_csv",
           "summary_json"]

MAX_R = 8        # cdr_place_replicas' R
MAX_NODES = 64   # and its n_nodes


def _exact(lo, hi):
    return [int(a) + (int(b) << 32) for a, b in zip(lo, hi)]


def placement_host(file_idx, client, primary, n_nodes, factor, R, sizes=None, labels=None,
                   k=None) -> dict:
    """The definition (module docstring).  ``factor``: int (n_files,) with 0 <=
    factor <= R <= 8.  Returns ``nodes`` int32 (n_files, R), ``per_file`` int64
    (n_files, 3) = total, local_before, local_after, ``counts`` int64 (n_files,
    n_nodes), ``node_replicas`` int64 (n_nodes,), ``node_bytes`` (exact Python
    ints: ``lo + (hi << 32)`` of two uint64 sums of the placed sizes' low 32 and
    high 31 bits; zeros without ``sizes``) and, with ``labels`` in [0, k),
    ``cluster_sums`` int64 (k, 3): the per_file columns summed per cluster."""
    n_nodes, R = int(n_nodes), int(R)
    if not 1 <= n_nodes <= MAX_NODES:
        raise NotImplementedError(f"n_nodes = {n_nodes} outside [1, {MAX_NODES}]")
    if not 1 <= R <= MAX_R:
        raise ValueError(f"R = {R} outside [1, {MAX_R}]")
    f = np.asarray(file_idx).astype(np.int64, copy=False).ravel()
    c = np.asarray(client).astype(np.int64, copy=False).ravel()
    if f.size != c.size:
        raise ValueError(f"{f.size} files against {c.size} clients")
    prim = np.asarray(primary).astype(np.int64, copy=False).ravel()
    nf = prim.size
    fac = np.asarray(factor).astype(np.int64, copy=False).ravel()
    if fac.size != nf:
        raise ValueError(f"{fac.size} factors for {nf} files")
    if nf and (fac.min() < 0 or fac.max() > R):
        raise ValueError(f"a factor outside [0, {R}]")
    ok = (f >= 0) & (f < nf)
    f, c = f[ok], c[ok]
    total = np.bincount(f, minlength=nf).astype(np.int64)
    node = (c >= 0) & (c < n_nodes)
    cnt = np.bincount(f[node] * n_nodes + c[node], minlength=nf * n_nodes).astype(
        np.int64).reshape(nf, n_nodes)
    rows = np.arange(nf)
    pv = (prim >= 0) & (prim < n_nodes)
    # descending count, ties to the lower id (stable), the primary before all
    key = cnt.copy()
    key[rows[pv], prim[pv]] = np.int64(1) << 62
    order = np.argsort(-key, axis=1, kind="stable")
    m = np.minimum(fac, n_nodes)
    nodes = np.full((nf, R), -1, dtype=np.int32)
    w = min(R, n_nodes)
    take = np.arange(w)[None, :] < m[:, None]
    nodes[:, :w] = np.where(take, order[:, :w], -1)
    before = np.zeros(nf, dtype=np.int64)
    before[pv] = cnt[rows[pv], prim[pv]]
    after = np.where(take, np.take_along_axis(cnt, order[:, :w], axis=1), 0).sum(axis=1)
    per_file = np.stack([total, before, after.astype(np.int64)], axis=1) if nf else \
        np.zeros((0, 3), dtype=np.int64)
    placed_f, placed_s = np.nonzero(take)
    placed_n = order[placed_f, placed_s]
    out = {"nodes": nodes, "per_file": per_file, "counts": cnt,
           "node_replicas": np.bincount(placed_n, minlength=n_nodes).astype(np.int64),
           "node_bytes": [0] * n_nodes}
    if sizes is not None:
        s = np.asarray(sizes).astype(np.int64, copy=False).ravel()
        if s.size != nf:
            raise ValueError(f"{s.size} sizes for {nf} files")
        if s.size and s.min() < 0:
            raise ValueError("negative size")
        u = s.astype(np.uint64)[placed_f]
        lo = np.zeros(n_nodes, dtype=np.uint64)
        hi = np.zeros(n_nodes, dtype=np.uint64)
        np.add.at(lo, placed_n, u & np.uint64(0xFFFFFFFF))
        np.add.at(hi, placed_n, u >> np.uint64(32))
        out["node_bytes"] = _exact(lo, hi)
    if labels is not None:
        k = int(k)
        lab = np.asarray(labels).astype(np.int64, copy=False).ravel()
        if lab.size != nf:
            raise ValueError(f"{lab.size} labels for {nf} files")
        if lab.size and (lab.min() < 0 or lab.max() >= k):
            raise ValueError(f"a label outside [0, {k})")
        cs = np.zeros((k, 3), dtype=np.int64)
        np.add.at(cs, lab, per_file)
        out["cluster_sums"] = cs
    return out


def _share(num, den):
    """(Fraction, float) of num / den; (None, None) without events."""
    if den == 0:
        return None, None
    fr = Fraction(int(num), int(den))
    return fr, float(fr)


def _summary(cluster_sums, cats, facs, node_replicas, node_bytes) -> dict:
    """Locality before and after, overall and per category, and the node loads,
    from the (k, 3) cluster sums: arithmetic on Python ints."""
    per = {}
    for j, cat in enumerate(cats):
        row = per.setdefault(cat, {"factor": facs[j], "clusters": [], "events": 0,
                                   "local_before": 0, "local_after": 0})
        row["clusters"].append(j)
        for key, v in zip(("events", "local_before", "local_after"), cluster_sums[j]):
            row[key] += int(v)
    tot = {key: sum(r[key] for r in per.values()) for key in ("events", "local_before",
                                                              "local_after")}
    for row in list(per.values()) + [tot]:
        for key in ("before", "after"):
            fr, fl = _share(row[f"local_{key}"], row["events"])
            row[f"locality_{key}"] = fr
            row[f"locality_{key}_float"] = fl
    return dict(tot, categories=per,
                nodes=[{"replicas": int(r), "bytes": int(b)}
                       for r, b in zip(node_replicas, node_bytes)])


def _factors(categories, replication_factors, k, prefix="C"):
    from replication_plan import _tables

    cats, facs = _tables(categories, replication_factors, prefix, k)
    R = max(1, max(facs))
    if R > MAX_R:
        raise ValueError(f"a replication factor above {MAX_R}")
    return cats, facs, R


def place(categories, replication_factors, k, *, n_nodes=None, labels=None, sizes=None,
          context: Context | None = None, prefix="C"):
    """``placement_host`` on the device over the events resident in ``context``
    (one cdr_place_replicas call), with ``factor[f] = factors[labels[f]]`` from
    the category and factor tables ``replication_plan`` takes.  ``n_nodes``
    defaults to the node count of the manifest the context ingested;
    ``labels=None``: the labels of the last assignment resident in ``context``.
    Returns ``(nodes, per_file, summary)``: ``summary`` holds ``events``,
    ``local_before``, ``local_after`` and ``locality_before`` /
    ``locality_after`` (Fractions, with ``*_float`` beside them; None without
    events), the same per category under ``categories``, and per node
    ``replicas`` and exact ``bytes`` (Python ints) under ``nodes``."""
    ctx = context if context is not None else default_context()
    k = int(k)
    cats, facs, R = _factors(categories, replication_factors, k, prefix)
    if n_nodes is None:
        n_nodes = getattr(ctx, "_ing_nodes", None)
        if n_nodes is None:
            raise ValueError("n_nodes: the context has ingested no manifest")
    res = ctx.place_replicas(n_nodes, k, facs, R, labels=labels, sizes=sizes)
    summary = _summary(res["cluster_sums"], cats, facs, res["node_replicas"], res["node_bytes"])
    return res["nodes"], res["per_file"], summary


def place_from_log(manifest, access_log, features_csv, categories, replication_factors, k, *,
                   labels=None, context: Context | None = None, prefix="C") -> dict:
    """The placement of the files of ``manifest`` from ``access_log``, for the
    clustering of ``features_csv`` (``labels=None``: the labels resident in
    ``context`` after ``kmeans_csv`` of that file, else one label per row of
    it).  The log goes through the device tokeniser (``compute_features.
    ingest_events``), or through the host encoder when it holds syntax the
    tokeniser leaves to the host.  The labels are aligned with the manifest
    rows by path: resident labels are used as they are when the features CSV
    lists the manifest's paths in order.  With a ``size_bytes`` column in the
    manifest the node loads carry bytes.  A path listed twice in the manifest
    is a ValueError (its events sit on its first row; a placement per duplicate
    row has no meaning).  Returns ``paths``, ``node_names``, ``factors`` (per
    file), ``nodes``, ``per_file``, ``summary``."""
    ctx = context if context is not None else default_context()
    k = int(k)
    cats, facs, R = _factors(categories, replication_factors, k, prefix)
    paths, node_names, sizes, host_labels = _ingest_log(ctx, manifest, access_log, features_csv,
                                                        labels)
    nodes, per_file, summary = place(categories, replication_factors, k,
                                     n_nodes=len(node_names), labels=host_labels, sizes=sizes,
                                     context=ctx, prefix=prefix)
    lab = host_labels if host_labels is not None else ctx.labels()
    return {"paths": paths, "node_names": node_names,
            "factors": np.asarray(facs, dtype=np.int64)[np.asarray(lab, dtype=np.int64)],
            "nodes": nodes, "per_file": per_file, "summary": summary}


def _ingest_log(ctx, manifest, access_log, features_csv, labels):
    """What ``place_from_log`` and ``evaluate_from_log`` share: the manifest's
    paths, node names and sizes (None without a ``size_bytes`` column), the
    labels aligned with the manifest rows by path (None: the resident labels
    are already in that order) and the log's events made resident in ``ctx``."""
    import pandas as pd

    import compute_features as cf

    paths, _, primary = cf.load_manifest(manifest)
    if len(set(paths)) != len(paths):
        raise ValueError("the manifest lists a path twice")
    if not paths:
        raise ValueError("the manifest has no rows")
    man = pd.read_csv(cf._strip_scheme(manifest), dtype=str, keep_default_na=False,
                      na_filter=False)
    sizes = pd.to_numeric(man["size_bytes"]).to_numpy(dtype=np.int64) \
        if "size_bytes" in man.columns else None
    fpaths = pd.read_csv(features_csv, usecols=["path"], dtype=str, keep_default_na=False,
                         na_filter=False)["path"].tolist()
    in_order = fpaths == [p if p is not None else "" for p in paths]
    host_labels = None if labels is None else np.asarray(labels, dtype=np.int64).ravel()
    if not in_order or host_labels is not None:
        lab = host_labels if host_labels is not None else ctx.labels().astype(np.int64)
        if lab.size != len(fpaths):
            raise ValueError(f"{lab.size} labels, the features CSV has {len(fpaths)} rows")
        if not in_order:
            row_of = {}
            for i, p in enumerate(fpaths):
                row_of.setdefault(p, i)
            missing = [p for p in paths if p not in row_of]
            if missing:
                raise ValueError(f"{len(missing)} manifest paths are not in the features CSV")
            lab = lab[np.array([row_of[p] for p in paths], dtype=np.int64)]
        host_labels = lab
    prim, node_names = cf.encode_primary(primary)
    if not node_names:
        raise ValueError("the manifest names no primary node")
    if cf.ingest_events(ctx, paths, primary, access_log) < 0:
        lt, lp, lo, lc = cf.load_access_log(access_log)
        ctx.features_load_events(*cf.encode(paths, primary, lt, lp, lo, lc))
    return paths, node_names, sizes, host_labels


def write_placement_csv(out, paths, factors, nodes, node_names) -> int:
    """``path,replication,nodes`` with the file's node names joined by ``;``,
    written by ``csv.writer``; returns the row count."""
    with open(out, "w", newline="", encoding="utf-8") as fh:
        w = csv.writer(fh, lineterminator="\n")
        w.writerow(["path", "replication", "nodes"])
        for p, fac, row in zip(paths, factors, nodes):
            w.writerow([p, int(fac), ";".join(node_names[int(j)] for j in row if j >= 0)])
    return len(paths)


def read_placement_csv(path, paths, node_names) -> np.ndarray:
    """The inverse of ``write_placement_csv``: int32 (len(paths), R) node ids,
    aligned with ``paths`` by path, -1 past a row's nodes; R is the widest row
    (at least 1).  A path of ``paths`` that the file does not list gets an all
    -1 row.  ValueError for an unknown node name, a path listed twice in the
    file, or more than 8 nodes on a row."""
    node_of = {name: j for j, name in enumerate(node_names)}
    rows = {}
    with open(path, newline="", encoding="utf-8") as fh:
        rd = csv.reader(fh)
        header = next(rd, None)
        if header is None or header[0] != "path" or "nodes" not in header:
            raise ValueError(f"{path}: no path,replication,nodes header")
        col = header.index("nodes")
        for rec in rd:
            if not rec:
                continue
            if rec[0] in rows:
                raise ValueError(f"{path}: the path {rec[0]!r} is listed twice")
            names = rec[col].split(";") if len(rec) > col and rec[col] else []
            if len(names) > MAX_R:
                raise ValueError(f"{path}: {len(names)} nodes for {rec[0]!r}, above {MAX_R}")
            for name in names:
                if name not in node_of:
                    raise ValueError(f"{path}: unknown node {name!r}")
            rows[rec[0]] = [node_of[name] for name in names]
    R = max([1] + [len(v) for v in rows.values()])
    out = np.full((len(paths), R), -1, dtype=np.int32)
    for i, p in enumerate(paths):
        v = rows.get(p if p is not None else "")
        if v:
            out[i, :len(v)] = v
    return out


EVAL_CLUSTER_COLUMNS = ("events", "local", "reads", "reads_local", "writes", "write_copies")
EVAL_NODE_COLUMNS = ("issued", "local", "reads_served", "writes_received", "replicas")
OP_WRITE, OP_READ = 1, 2   # the event loaders' op codes


def evaluate_host(file_idx, op, client, nodes, n_nodes, labels=None, k=None) -> dict:
    """The definition of the evaluation of a given placement (NumPy, no GPU).
    ``nodes``: int (n_files, R), entries in [-1, n_nodes), 1 <= R <= 8.  Per
    file: ``mask[f]`` the set of its entries >= 0 (a node listed twice counts
    once), ``first[f]`` the first entry >= 0 in row order (-1 without one),
    ``copies[f]`` the size of the set.  Events with ``file_idx`` outside [0,
    n_files) are ignored; an event (f, o, c) is local (``in``) when 0 <= c <
    n_nodes and c is in mask[f].  Returns int64 arrays

    ``per_file`` (n_files, 2)   total, local
    ``cluster_sums`` (k, 6)     by labels[f] (all 0 with k = 1 when None):
                                events, local, reads (o == 2), reads_local,
                                writes (o == 1), write_copies (copies[f] summed
                                over the WRITE events)
    ``node_sums`` (n_nodes, 5)  issued (c == j), local (c == j and in),
                                reads_served (a local READ by its client, any
                                other READ by first[f], by nobody when that is
                                -1), writes_received (WRITE events of files
                                with j in mask[f]), replicas (files with j in
                                mask[f])

    and ``unserved_reads`` = all reads - all reads_served (a Python int)."""
    n_nodes = int(n_nodes)
    if not 1 <= n_nodes <= MAX_NODES:
        raise NotImplementedError(f"n_nodes = {n_nodes} outside [1, {MAX_NODES}]")
    nd = np.asarray(nodes).astype(np.int64, copy=False)
    if nd.ndim != 2:
        raise ValueError("nodes is not (n_files, R)")
    nf, R = nd.shape
    if not 1 <= R <= MAX_R:
        raise ValueError(f"R = {R} outside [1, {MAX_R}]")
    if nd.size and (nd.min() < -1 or nd.max() >= n_nodes):
        raise ValueError(f"a node entry outside [-1, {n_nodes})")
    if labels is None:
        k = 1 if k is None else int(k)
        lab = np.zeros(nf, dtype=np.int64)
    else:
        k = int(k)
        lab = np.asarray(labels).astype(np.int64, copy=False).ravel()
        if lab.size != nf:
            raise ValueError(f"{lab.size} labels for {nf} files")
    if not 1 <= k <= 1024:
        raise NotImplementedError(f"k = {k} outside [1, 1024]")
    if lab.size and (lab.min() < 0 or lab.max() >= k):
        raise ValueError(f"a label outside [0, {k})")
    f = np.asarray(file_idx).astype(np.int64, copy=False).ravel()
    o = np.asarray(op).astype(np.int64, copy=False).ravel()
    c = np.asarray(client).astype(np.int64, copy=False).ravel()
    if not f.size == o.size == c.size:
        raise ValueError(f"{f.size} files, {o.size} ops, {c.size} clients")
    has = np.zeros((nf, n_nodes), dtype=bool)     # has[f][j]: bit j of mask[f]
    valid = nd >= 0
    ff, ss = np.nonzero(valid)
    has[ff, nd[ff, ss]] = True
    first = np.where(valid.any(axis=1), nd[np.arange(nf), valid.argmax(axis=1)], -1) if nf else \
        np.zeros(0, dtype=np.int64)
    copies = has.sum(axis=1).astype(np.int64)
    ok = (f >= 0) & (f < nf)
    f, o, c = f[ok], o[ok], c[ok]
    node = (c >= 0) & (c < n_nodes)
    inn = node.copy()
    inn[node] = has[f[node], c[node]]
    rd, wr = o == OP_READ, o == OP_WRITE

    def count(idx, n):
        return np.bincount(idx, minlength=n).astype(np.int64)

    per_file = np.stack([count(f, nf), count(f[inn], nf)], axis=1)
    le = lab[f]
    wc = np.zeros(k, dtype=np.int64)
    np.add.at(wc, le[wr], copies[f[wr]])
    cluster_sums = np.stack([count(le, k), count(le[inn], k), count(le[rd], k),
                             count(le[rd & inn], k), count(le[wr], k), wc], axis=1)
    srv = np.where(inn[rd], c[rd], first[f[rd]])
    node_sums = np.stack([count(c[node], n_nodes), count(c[inn], n_nodes),
                          count(srv[srv >= 0], n_nodes),
                          has.astype(np.int64).T @ count(f[wr], nf),
                          has.sum(axis=0).astype(np.int64)], axis=1)
    return {"per_file": per_file, "cluster_sums": cluster_sums, "node_sums": node_sums,
            "unserved_reads": int(cluster_sums[:, 2].sum()) - int(node_sums[:, 2].sum())}


def _eval_summary(cluster_sums, node_sums, cats, facs) -> dict:
    """Locality, read locality and write amplification overall and per
    category, the node loads and the read-load imbalance, from the (k, 6)
    cluster sums and the (n_nodes, 5) node sums: arithmetic on Python ints."""
    per = {}
    for j, cat in enumerate(cats):
        row = per.setdefault(cat, dict({"factor": facs[j], "clusters": []},
                                       **{key: 0 for key in EVAL_CLUSTER_COLUMNS}))
        row["clusters"].append(j)
        for key, v in zip(EVAL_CLUSTER_COLUMNS, cluster_sums[j]):
            row[key] += int(v)
    tot = {key: sum(r[key] for r in per.values()) for key in EVAL_CLUSTER_COLUMNS}
    for row in list(per.values()) + [tot]:
        for key, num, den in (("locality", "local", "events"),
                              ("read_locality", "reads_local", "reads"),
                              ("write_amplification", "write_copies", "writes")):
            row[key], row[f"{key}_float"] = _share(row[num], row[den])
    nodes = [{key: int(v) for key, v in zip(EVAL_NODE_COLUMNS, r)} for r in node_sums]
    served = [n["reads_served"] for n in nodes]
    imb, imb_f = _share(max(served) * len(served), sum(served))
    return dict(tot, categories=per, nodes=nodes, unserved_reads=tot["reads"] - sum(served),
                read_load_imbalance=imb, read_load_imbalance_float=imb_f)


def evaluate(nodes, categories, replication_factors, k, *, n_nodes=None, labels=None,
             per_file=False, context: Context | None = None, prefix="C"):
    """``evaluate_host`` on the device over the events resident in ``context``
    (one cdr_place_evaluate call, csrc/place_eval.hip) for the given placement
    ``nodes`` (int (n_files, R), entries in [-1, n_nodes)): one computed
    earlier, or one the project did not compute.  ``n_nodes`` defaults to the
    node count of the manifest the context ingested; ``labels=None``: the
    labels of the last assignment resident in ``context``.  Returns
    ``(per_file, summary)``, ``per_file`` int64 (n_files, 2) = total, local or
    None unless asked.  ``summary`` holds, overall and per category under
    ``categories``: ``events``, ``local``, ``locality``, ``reads``,
    ``reads_local``, ``read_locality``, ``writes``, ``write_copies`` and
    ``write_amplification`` (write_copies / writes); per node under ``nodes``
    ``issued``, ``local``, ``reads_served``, ``writes_received`` and
    ``replicas``; ``unserved_reads`` and ``read_load_imbalance`` (the largest
    reads_served over their mean).  Counts are Python ints, ratios Fractions
    with ``*_float`` beside them (None where the denominator is 0)."""
    ctx = context if context is not None else default_context()
    k = int(k)
    cats, facs, _ = _factors(categories, replication_factors, k, prefix)
    if n_nodes is None:
        n_nodes = getattr(ctx, "_ing_nodes", None)
        if n_nodes is None:
            raise ValueError("n_nodes: the context has ingested no manifest")
    res = ctx.place_evaluate(n_nodes, nodes, k, labels=labels, per_file=per_file)
    return res["per_file"], _eval_summary(res["cluster_sums"], res["node_sums"], cats, facs)


def evaluate_from_log(manifest, access_log, features_csv, placement_csv, categories,
                      replication_factors, k, *, labels=None, context: Context | None = None,
                      prefix="C") -> dict:
    """``evaluate`` of the placement in ``placement_csv`` (a file
    ``write_placement_csv`` wrote, or one of that form) under ``access_log``:
    how local yesterday's placement is today.  The manifest, the log and the
    labels are taken exactly as ``place_from_log`` takes them.  Returns
    ``paths``, ``node_names``, ``nodes`` (the placement read), ``per_file``
    and ``summary``."""
    ctx = context if context is not None else default_context()
    k = int(k)
    _factors(categories, replication_factors, k, prefix)
    paths, node_names, _, host_labels = _ingest_log(ctx, manifest, access_log, features_csv,
                                                    labels)
    nodes = read_placement_csv(placement_csv, paths, node_names)
    per_file, summary = evaluate(nodes, categories, replication_factors, k,
                                 n_nodes=len(node_names), labels=host_labels, per_file=True,
                                 context=ctx, prefix=prefix)
    return {"paths": paths, "node_names": node_names, "nodes": nodes, "per_file": per_file,
            "summary": summary}


def summary_json(summary) -> dict:
    """``summary`` with the Fractions as ``"num/den"`` strings (for json.dumps)."""
    def conv(v):
        if isinstance(v, Fraction):
            return f"{v.numerator}/{v.denominator}"
        if isinstance(v, dict):
            return {a: conv(b) for a, b in v.items()}
        if isinstance(v, list):
            return [conv(b) for b in v]
        return v

    return conv(summary)

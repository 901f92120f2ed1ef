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
"""
from __future__ import annotations

import csv
from fractions import Fraction

import numpy as np

from _cdr import Context, default_context

__all__ = ["placement_host", "place", "place_from_log", "write_placement_csv", "MAX_R",
           "MAX_NODES"]

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
    import pandas as pd

    import compute_features as cf

    ctx = context if context is not None else default_context()
    k = int(k)
    cats, facs, R = _factors(categories, replication_factors, k, prefix)
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
    nodes, per_file, summary = place(categories, replication_factors, k,
                                     n_nodes=len(node_names), labels=host_labels, sizes=sizes,
                                     context=ctx, prefix=prefix)
    lab = host_labels if host_labels is not None else ctx.labels()
    return {"paths": paths, "node_names": node_names,
            "factors": np.asarray(facs, dtype=np.int64)[np.asarray(lab, dtype=np.int64)],
            "nodes": nodes, "per_file": per_file, "summary": summary}


def write_placement_csv(out, paths, factors, nodes, node_names) -> int:
    """``path,replication,nodes`` with the file's node names joined by ``;``,
    written by ``csv.writer``; returns the row count."""
    with open(out, "w", newline="", encoding="utf-8") as fh:
        w = csv.writer(fh, lineterminator="\n")
        w.writerow(["path", "replication", "nodes"])
        for p, fac, row in zip(paths, factors, nodes):
            w.writerow([p, int(fac), ";".join(node_names[int(j)] for j in row if j >= 0)])
    return len(paths)


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

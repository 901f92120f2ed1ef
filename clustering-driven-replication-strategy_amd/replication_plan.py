"""The per-file replication plan: path, cluster, category, replication factor.

``src/main.py:92`` forms ``feature_file['cluster'] = labels`` and drops it; the
reference writes one row per centroid.  The plan is the row per file, what one
hands to ``hdfs dfs -setrep``, and ``summarize`` says what it costs in bytes.

The plan is defined by ``write_plan_csv_host`` and by nothing else::

    frame = pd.read_csv(src, usecols=[path_column], dtype=str, keep_default_na=False,
                        na_filter=False)
    w = csv.writer(out, lineterminator="\\n")
    w.writerow(["path", "cluster", "category", "replication"])
    for p, l in zip(frame[path_column], labels):
        w.writerow([p, int(l), category_of_cluster[l], replication_factors[category_of_cluster[l]]])

``write_plan_csv`` gives the same bytes with the rows formatted in libcdr.so
(csrc/plan.hip): the paths are copied as bytes from the features CSV that
``kmeans_csv`` read, and the labels of the last assignment never leave the
device.  What the device does not decide itself goes to the definition, never
to a guess: a deferred row (a quote, a NUL, a lone CR, a field count other than
the header's, a path longer than 65535 bytes) is formatted by the host and
spliced in; the whole file goes to the host writer in the cases where
``read_features`` takes the whole file to pandas.  The file must be UTF-8, as
pandas requires.

CLI (the join of ``size_bytes`` on ``path`` for ``--manifest`` is host work, pandas)::

    python replication_plan.py --input_path F --k K --tables T.json --out plan.csv
                               [--manifest M.csv] [--current_factor R]
                               [--previous_plan PREV.csv]
                               [--access_log LOG --placement PLACEMENT.csv]
                               [--access_log LOG --evaluate_placement EARLIER.csv]

From the second plan on each file already carries the previous plan's factor,
so what a new plan costs is summed per file against that: ``transition`` (the
moves between the categories of two plans) from the contingency table of the
two clusterings (csrc/agree.hip, cluster_agreement.py), weighted by the sizes.
``--previous_plan`` (a file this module wrote; joined on ``path`` by pandas)
prints it as one more JSON line after ``summarize``'s.

``--access_log`` with ``--manifest`` and ``--placement`` also writes where the
replicas go (``path,replication,nodes``; replica_placement.py, csrc/place.hip)
and prints one more JSON line: the share of node-local accesses before and
after, overall and per category, and the replicas and bytes per node.  Without
them every output is what it was.

``--access_log`` with ``--manifest`` and ``--evaluate_placement`` judges a
placement CSV written earlier (yesterday's, or a cluster's real block
locations) on this log (replica_placement.evaluate, csrc/place_eval.hip) and
prints one more JSON line: locality, read locality and write amplification
overall and per category, and per node the events issued, the reads served,
the write copies received and the replicas.
"""
from __future__ import annotations

import argparse
import csv
import glob
import io
import json
import mmap
import os
import time

import numpy as np

from _cdr import PLAN_MAX_TAIL, Context, default_context

__all__ = ["HEADER", "write_plan_csv", "write_plan_csv_host", "summarize", "transition",
           "transition_from_table", "main"]

HEADER = ["path", "cluster", "category", "replication"]
MAX_K = 1024                  # cdr_plan_format's k
DEFERRED_CAP = 1 << 20        # deferred rows taken back from the device per call
# Rows per cdr_plan_format call.  Beyond the file and its record index (8 B per
# row), a call keeps 8 + 4 + 8 B per row of field offsets, lengths and output
# offsets and the chunk's text (about 50 B per row for paths of 30 bytes) on
# the device, pinned on the host, and once more in the buffer the context keeps
# for the text (96 B per row, grown to what a chunk needs): 2^18 rows bound each
# at about 25 MiB whatever the file's size, and still give every CU several
# workgroups.
PLAN_CHUNK_ROWS = 1 << 18


class _Bytes:
    """csv.writer target that collects UTF-8 bytes (newline="" semantics)."""

    def __init__(self):
        self.parts = []

    def write(self, text):
        self.parts.append(text.encode("utf-8"))


def _tables(categories, replication_factors, prefix="C", k=None):
    """(category of cluster j, factor of cluster j) for j < k (default: the
    number of entries of `categories`)."""
    k = len(categories) if k is None else int(k)
    cats, facs = [], []
    for j in range(k):
        name = f"{prefix}{j}"
        if name not in categories:
            raise ValueError(f"cluster {name} has no category")
        cat = categories[name]
        if cat not in replication_factors:
            raise ValueError(f"category {cat!r} has no replication factor")
        fac = replication_factors[cat]
        if isinstance(fac, bool) or not isinstance(fac, (int, np.integer)) or fac < 0:
            raise ValueError(f"the replication factor of {cat!r} is not an int >= 0: {fac!r}")
        cats.append(cat)
        facs.append(int(fac))
    return cats, facs


def _label(l, k):
    l = int(l)
    if not 0 <= l < k:
        raise ValueError(f"cluster {l} has no category")
    return l


def write_plan_csv_host(src, out, categories, replication_factors, *, labels=None,
                        path_column="path", prefix="C", chunk_rows=None, info=None) -> int:
    """The definition of the plan (module docstring); returns the row count.
    ``labels``: one cluster per row of ``src`` (there are no resident labels on
    the host); ``chunk_rows`` is accepted for the common signature and unused."""
    import pandas as pd

    cats, facs = _tables(categories, replication_factors, prefix)
    if labels is None:
        raise ValueError("the host writer needs the labels")
    frame = pd.read_csv(src, usecols=[path_column], dtype=str, keep_default_na=False,
                        na_filter=False)
    labels = np.asarray(labels).ravel()
    if len(labels) != len(frame):
        raise ValueError(f"{len(labels)} labels, the file has {len(frame)} rows")
    with open(out, "w", newline="", encoding="utf-8") as fh:
        w = csv.writer(fh, lineterminator="\n")
        w.writerow(HEADER)
        for p, l in zip(frame[path_column], labels):
            l = _label(l, len(cats))
            w.writerow([p, l, cats[l], facs[l]])
    if info is not None:
        info.clear()
        info.update(rows=len(frame), deferred_rows=0, whole_file_fallback=True)
    return len(frame)


def _tail(cat, fac) -> bytes:
    """``,<category>,<factor>\\n`` as csv.writer writes it after two fields."""
    sink = _Bytes()
    csv.writer(sink, lineterminator="\n").writerow(["", cat, fac])
    return b"".join(sink.parts)


def _splice(text, deferred, data, body, names, path_column, labels, cats, facs):
    """The chunk's text with the definition's rows at the deferred rows'
    offsets, or None when pandas' view of those rows does not line up with the
    device's (the whole file goes to the host writer then)."""
    import pandas as pd

    parts = [bytes(data[:body])]
    if not parts[0].endswith(b"\n"):
        parts.append(b"\n")
    # pandas infers an index from a first data row with more fields than the
    # header; a plain first row (dropped below) keeps the header's meaning
    parts.append(b",".join([b"0"] * len(names)) + b"\n")
    for _, _, b0, b1 in deferred:
        parts.append(bytes(data[int(b0):int(b1)]))
        parts.append(b"\n")
    try:
        frame = pd.read_csv(io.BytesIO(b"".join(parts)), usecols=[path_column], dtype=str,
                            keep_default_na=False, na_filter=False)
    except Exception:
        return None
    if len(frame) != len(deferred) + 1:  # (a lone CR ends a record for pandas)
        return None
    sink = _Bytes()
    w = csv.writer(sink, lineterminator="\n")
    text = memoryview(text)
    pos = 0
    for (row, off, _, _), p in zip(deferred, frame[path_column][1:]):
        sink.parts.append(bytes(text[pos:off]))
        pos = int(off)
        l = int(labels[int(row)])
        w.writerow([p, l, cats[l], facs[l]])
    sink.parts.append(bytes(text[pos:]))
    return b"".join(sink.parts)


def write_plan_csv(src, out, categories, replication_factors, *, labels=None, path_column="path",
                   prefix="C", context: Context | None = None, chunk_rows=None,
                   info: dict | None = None) -> int:
    """``write_plan_csv_host`` with the rows formatted on the device, byte for
    byte the same file; returns the row count.  ``categories`` is what
    ``ClusterClassifier.classify_labels`` returns; ``labels=None`` takes the
    labels of the last assignment resident in ``context`` (after ``kmeans_csv``
    of the same file, row i is point i).  One library call and one binary write
    per ``chunk_rows`` rows (default ``PLAN_CHUNK_ROWS``); the text does not
    depend on the chunking.

    ``info`` (a dict, filled in place) receives ``rows``, ``deferred_rows``,
    ``whole_file_fallback`` and the times ``upload_ms``, ``index_ms``,
    ``length_ms``, ``emit_ms``, ``copy_ms`` (cdr_plan_timing: device events) and,
    on the host clock, ``call_ms`` (inside the library calls) and ``write_ms``
    (writing the text to the file)."""
    from features_csv import _first_row_fields, _header

    ctx = context if context is not None else default_context()
    info = info if info is not None else {}
    info.clear()
    cats, facs = _tables(categories, replication_factors, prefix)
    k = len(cats)
    chunk = PLAN_CHUNK_ROWS if chunk_rows is None else int(chunk_rows)
    if chunk < 1:
        raise ValueError("chunk_rows must be at least 1")
    if labels is not None:
        labels = np.ascontiguousarray(labels, dtype=np.int64).ravel()
    tails = [_tail(c, f) for c, f in zip(cats, facs)]

    def whole_file():
        lab = labels if labels is not None else ctx.labels()
        return write_plan_csv_host(src, out, categories, replication_factors, labels=lab,
                                   path_column=path_column, prefix=prefix, info=info)

    size = os.path.getsize(src)
    if size == 0 or not 1 <= k <= MAX_K or max(len(t) for t in tails) > PLAN_MAX_TAIL:
        return whole_file()  # (an empty file: pandas' EmptyDataError)
    ok = True
    with open(src, "rb") as fh, mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) as data:
        head = _header(data)
        if head is None:
            return whole_file()
        names, body = head
        plain = (len(set(names)) == len(names) and all(names) and len(names) <= 32767
                 and path_column in names and body < size
                 and _first_row_fields(data, body) in (-1, len(names)))
        if not plain:
            # names pandas would mangle, a first row that makes pandas infer an
            # index, no such column (pandas' own error), no data rows
            return whole_file()
        col = names.index(path_column)
        n_deferred, call_s, write_s = 0, 0.0, 0.0
        # the text goes to a name of its own until it is whole: an error (a label
        # out of range, ...) leaves no plan file, a fallback no half-written one
        part = f"{out}.part"
        try:
            with open(part, "wb") as fo:
                fo.write((",".join(HEADER) + "\n").encode("utf-8"))
                lo = 0
                while ok:
                    t0 = time.perf_counter()
                    try:
                        res = ctx.plan_format(data, body, len(names), col, labels, k, tails, lo,
                                              chunk, deferred_cap=DEFERRED_CAP)
                    except ValueError as e:
                        if "the file has" not in str(e):
                            raise
                        # the label count is not the device's row count: pandas' rows
                        # decide (a lone CR ends a record for pandas alone)
                        ok = False
                        break
                    t1 = time.perf_counter()
                    call_s += t1 - t0
                    n, text = res["rows"], res["text"]
                    if res["guard"] >= 0 or res["deferred_rows"] > len(res["deferred"]):
                        ok = False
                        break
                    if res["deferred_rows"]:
                        lab = labels if labels is not None else ctx.labels()
                        text = _splice(text, res["deferred"], data, body, names, path_column, lab,
                                       cats, facs)
                        if text is None:
                            ok = False
                            break
                        n_deferred += res["deferred_rows"]
                    t1 = time.perf_counter()
                    fo.write(memoryview(text))
                    write_s += time.perf_counter() - t1
                    lo += chunk
                    if lo >= n:
                        break
            if ok:
                os.replace(part, out)
        finally:
            if os.path.exists(part):
                os.remove(part)
    if not ok:
        return whole_file()
    t = ctx.plan_timing()
    info.update(rows=n, deferred_rows=n_deferred, whole_file_fallback=False,
                upload_ms=float(t[0]), index_ms=float(t[1]), length_ms=float(t[2]),
                emit_ms=float(t[3]), copy_ms=float(t[4]), call_ms=1e3 * call_s,
                write_ms=1e3 * write_s)
    return n


def summarize(categories, replication_factors, k, *, sizes=None, current_factor=None, labels=None,
              context: Context | None = None, prefix="C") -> dict:
    """What the plan holds and costs: ``{"categories": {category: {...}},
    "total": {...}}`` with, per category, ``factor``, ``clusters`` (their
    numbers), ``files``; with ``sizes`` (int64 >= 0, one per file) also ``bytes``
    and ``replica_bytes = factor * bytes``; with ``current_factor`` (HDFS's one
    ``dfs.replication`` of all files) also ``bytes_to_copy = max(factor -
    current, 0) * bytes`` and ``bytes_to_free = max(current - factor, 0) *
    bytes``.  ``total`` sums them over the categories.  ``labels=None``: the
    labels resident in ``context``.  The per-cluster counts and size sums come
    from the device (cdr_plan_size_sums); the rest is arithmetic on k Python
    ints."""
    ctx = context if context is not None else default_context()
    k = int(k)
    cats, facs = _tables(categories, replication_factors, prefix, k)
    if current_factor is not None and (isinstance(current_factor, bool)
                                       or not isinstance(current_factor, (int, np.integer))
                                       or current_factor < 0):
        raise ValueError(f"current_factor is not an int >= 0: {current_factor!r}")
    if labels is not None:
        labels = np.ascontiguousarray(labels, dtype=np.int64).ravel()
        n = labels.size
    else:
        n = ctx.info()["n"]
    if sizes is not None:
        sizes = np.ascontiguousarray(sizes, dtype=np.int64).ravel()
        if sizes.size != n:
            raise ValueError(f"{sizes.size} sizes for {n} files")
    files = ctx.plan_size_sums(None, k, labels)  # no sizes: the rows are counted
    nbytes = ctx.plan_size_sums(sizes, k, labels) if sizes is not None else None
    keys = ["files"] + (["bytes", "replica_bytes"] if sizes is not None else []) + (
        ["bytes_to_copy", "bytes_to_free"] if sizes is not None and current_factor is not None
        else [])
    out = {}
    for j in range(k):
        row = out.setdefault(cats[j], dict({"factor": facs[j], "clusters": []},
                                           **{key: 0 for key in keys}))
        row["clusters"].append(j)
        row["files"] += files[j]
        if nbytes is not None:
            row["bytes"] += nbytes[j]
            row["replica_bytes"] += facs[j] * nbytes[j]
            if current_factor is not None:
                row["bytes_to_copy"] += max(facs[j] - int(current_factor), 0) * nbytes[j]
                row["bytes_to_free"] += max(int(current_factor) - facs[j], 0) * nbytes[j]
    total = {key: sum(row[key] for row in out.values()) for key in keys}
    return {"categories": out, "total": total}


def transition_from_table(counts, nbytes, prev_cats, prev_facs, cats, facs) -> dict:
    """What a new plan changes against the previous one, from the contingency
    table of the two clusterings: ``counts[i][j]`` files (and ``nbytes[i][j]``
    bytes, or None) that were in previous cluster i and are in new cluster j;
    ``prev_cats`` / ``prev_facs`` the category and factor of previous cluster i,
    ``cats`` / ``facs`` of new cluster j.  Returns ``{"moves": {old_category:
    {new_category: {...}}}, "total": {...}}``: per pair of categories that holds
    files ``old_factor``, ``new_factor``, ``files`` and with bytes also
    ``bytes``, ``bytes_to_copy = max(new - old, 0) * bytes`` and
    ``bytes_to_free = max(old - new, 0) * bytes``; ``total`` sums them and adds
    ``files_changed``, the files whose factor differs.  Arithmetic on Python
    ints; a category with two factors on one side is a ValueError."""
    ka, kb = len(prev_cats), len(cats)
    if len(prev_facs) != ka or len(facs) != kb:
        raise ValueError("one factor per cluster")
    counts = np.asarray(counts)
    if counts.shape != (ka, kb):
        raise ValueError(f"the table is {counts.shape}, the clusterings have {ka} and {kb} clusters")
    if nbytes is not None:
        nbytes = np.asarray(nbytes, dtype=object)
        if nbytes.shape != (ka, kb):
            raise ValueError(f"the byte table is {nbytes.shape}, not {(ka, kb)}")
    keys = ["files"] + (["bytes", "bytes_to_copy", "bytes_to_free"] if nbytes is not None else [])
    moves = {}
    total = dict({key: 0 for key in keys}, files_changed=0)
    for i in range(ka):
        for j in range(kb):
            files = int(counts[i, j])
            if files == 0:
                continue
            old, new = int(prev_facs[i]), int(facs[j])
            row = moves.setdefault(prev_cats[i], {}).setdefault(
                cats[j], dict({"old_factor": old, "new_factor": new}, **{key: 0 for key in keys}))
            if (row["old_factor"], row["new_factor"]) != (old, new):
                raise ValueError(f"the move {prev_cats[i]!r} -> {cats[j]!r} has two pairs of factors")
            add = {"files": files}
            if nbytes is not None:
                b = int(nbytes[i, j])
                add.update(bytes=b, bytes_to_copy=max(new - old, 0) * b,
                           bytes_to_free=max(old - new, 0) * b)
            for key, v in add.items():
                row[key] += v
                total[key] += v
            if old != new:
                total["files_changed"] += files
    return {"moves": moves, "total": total}


def transition(prev_categories, prev_replication_factors, prev_k, categories, replication_factors,
               k, *, prev_labels=None, labels=None, sizes=None, context: Context | None = None,
               prefix="C") -> dict:
    """``transition_from_table`` of the previous plan (its category and factor
    tables and its k) and the new one.  ``prev_labels=None``: the labels kept on
    the device (``cluster_agreement.keep``); ``labels=None``: the labels
    resident in ``context``; ``sizes``: int64 >= 0, one per file.  Both pairs of
    tables are validated as ``summarize`` validates its own; the table comes
    from one cdr_agree_table call over all files."""
    ctx = context if context is not None else default_context()
    prev_k, k = int(prev_k), int(k)
    prev_cats, prev_facs = _tables(prev_categories, prev_replication_factors, prefix, prev_k)
    cats, facs = _tables(categories, replication_factors, prefix, k)
    res = ctx.agree_table(k, prev_k, labels, prev_labels, sizes)  # [new][previous]
    counts, nbytes = res if sizes is not None else (res, None)
    return transition_from_table(counts.T, None if nbytes is None else nbytes.T, prev_cats,
                                 prev_facs, cats, facs)


NEW_FILES = "(new)"  # the previous category of the paths a previous plan does not hold


def _previous_plan(path, paths, current_factor, prefix="C"):
    """(labels, categories, factors, k) of the plan file `path` (one this module
    wrote) for the files `paths`, joined on the path.  The previous clusters are
    numbered 0.. in the order of their numbers in the file; the paths the file
    does not hold form one more cluster of category ``NEW_FILES`` and factor
    current_factor (SystemExit without it)."""
    import pandas as pd

    prev = pd.read_csv(path, usecols=HEADER, dtype={"path": str, "category": str},
                       keep_default_na=False, na_filter=False)
    per = prev.groupby("cluster")[["category", "replication"]].nunique()
    if len(per) and int(per.to_numpy().max()) > 1:
        raise SystemExit(f"Error: {path}: a cluster with more than one category or factor")
    first = prev.drop_duplicates("cluster").sort_values("cluster")
    dense = {int(c): j for j, c in enumerate(first["cluster"])}
    cats = {f"{prefix}{j}": c for j, c in enumerate(first["category"])}
    factors = {}
    for c, f in zip(first["category"], first["replication"]):
        if factors.setdefault(c, int(f)) != int(f):
            raise SystemExit(f"Error: {path}: category {c!r} has more than one factor")
    k = len(dense)
    labels = paths.map(prev.drop_duplicates("path").set_index("path")["cluster"])
    missing = labels.isna()
    if missing.any():
        if current_factor is None:
            raise SystemExit(f"Error: {int(missing.sum())} paths are not in the previous plan "
                             "(pass --current_factor for new files)")
        if factors.setdefault(NEW_FILES, int(current_factor)) != int(current_factor):
            raise SystemExit(f"Error: {path}: category {NEW_FILES!r} has another factor")
        cats[f"{prefix}{k}"] = NEW_FILES
        k += 1
    lab = np.array([k - 1 if m else dense[int(c)] for c, m in zip(labels.fillna(0), missing)],
                   dtype=np.int64)
    return lab, cats, factors, k


def _resolve(input_path):
    """src/main.py:154-168: a directory holds part-00000*.csv; the first match."""
    pattern = os.path.join(input_path, "part-00000*.csv") if os.path.isdir(input_path) \
        else input_path
    found = glob.glob(pattern)
    if not found:
        raise SystemExit(f"Error: No features CSV file found matching pattern: {pattern}")
    return found[0]


def main(argv=None, context: Context | None = None):
    from features_csv import CLUSTERING_FEATURES, kmeans_csv
    from scoring import ClusterClassifier

    ap = argparse.ArgumentParser(description="Cluster the features CSV and write the per-file "
                                             "replication plan.")
    ap.add_argument("--input_path", required=True)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--tables", required=True,
                    help="JSON with WEIGHTS, DIRECTIONS, REPLICATION_FACTORS and optionally "
                         "GLOBAL_MEDIANS")
    ap.add_argument("--out", default="plan.csv")
    ap.add_argument("--manifest", default=None, help="CSV with path and size_bytes columns")
    ap.add_argument("--current_factor", type=int, default=None)
    ap.add_argument("--previous_plan", default=None,
                    help="a plan CSV this program wrote earlier: the moves from it to the new "
                         "plan are printed as one more JSON line")
    ap.add_argument("--access_log", default=None,
                    help="the access log the features were built from (with --manifest and "
                         "--placement): the nodes of each file's replicas")
    ap.add_argument("--placement", default=None,
                    help="where to write path,replication,nodes (replica_placement.py)")
    ap.add_argument("--evaluate_placement", default=None,
                    help="a placement CSV written earlier (with --manifest and --access_log): "
                         "how local it is under this log and what it costs, as one more JSON "
                         "line")
    args = ap.parse_args(argv)
    uses_log = args.placement is not None or args.evaluate_placement is not None
    if (args.access_log is None) != (not uses_log) or (uses_log and args.manifest is None):
        raise SystemExit("Error: --access_log goes with --manifest and --placement or "
                         "--evaluate_placement")
    src = _resolve(args.input_path)
    with open(args.tables) as fh:
        t = json.load(fh)
    ctx = context if context is not None else default_context()
    kmeans_csv(src, args.k, random_state=42, context=ctx)
    if "GLOBAL_MEDIANS" in t:
        clf = ClusterClassifier(t["GLOBAL_MEDIANS"], t["WEIGHTS"], t["DIRECTIONS"],
                                t["REPLICATION_FACTORS"], context=ctx)
    else:
        clf = ClusterClassifier.from_points(t["WEIGHTS"], t["DIRECTIONS"],
                                            t["REPLICATION_FACTORS"], CLUSTERING_FEATURES,
                                            context=ctx)
    categories = clf.classify_labels(args.k, CLUSTERING_FEATURES, context=ctx)
    rows = write_plan_csv(src, args.out, categories, t["REPLICATION_FACTORS"], context=ctx)
    print(f"Wrote the plan of {rows} files to {args.out}")
    sizes = None
    if args.manifest or args.previous_plan:
        import pandas as pd

        paths = pd.read_csv(src, usecols=["path"], dtype=str, keep_default_na=False,
                            na_filter=False)["path"]
    if args.manifest:
        man = pd.read_csv(args.manifest, usecols=["path", "size_bytes"],
                          dtype={"path": str}, keep_default_na=False, na_filter=False)
        sizes = paths.map(man.drop_duplicates("path").set_index("path")["size_bytes"])
        if sizes.isna().any():
            raise SystemExit(f"Error: {int(sizes.isna().sum())} paths are not in the manifest")
        sizes = sizes.to_numpy(dtype=np.int64)
        print(json.dumps(summarize(categories, t["REPLICATION_FACTORS"], args.k, sizes=sizes,
                                   current_factor=args.current_factor, context=ctx)))
    if args.previous_plan:
        prev_labels, prev_cats, prev_factors, prev_k = _previous_plan(
            args.previous_plan, paths, args.current_factor)
        print(json.dumps(transition(prev_cats, prev_factors, prev_k, categories,
                                    t["REPLICATION_FACTORS"], args.k, prev_labels=prev_labels,
                                    sizes=sizes, context=ctx)))
    if args.placement:
        import replica_placement as rp

        res = rp.place_from_log(args.manifest, args.access_log, src, categories,
                                t["REPLICATION_FACTORS"], args.k, context=ctx)
        rp.write_placement_csv(args.placement, res["paths"], res["factors"], res["nodes"],
                               res["node_names"])
        print(json.dumps(dict(rp.summary_json(res["summary"]), node_names=res["node_names"])))
    if args.evaluate_placement:
        import replica_placement as rp

        res = rp.evaluate_from_log(args.manifest, args.access_log, src, args.evaluate_placement,
                                   categories, t["REPLICATION_FACTORS"], args.k, context=ctx)
        print(json.dumps(dict(rp.summary_json(res["summary"]), node_names=res["node_names"])))


if __name__ == "__main__":
    main()

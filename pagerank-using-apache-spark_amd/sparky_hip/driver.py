"""Process-level drop-in for the Spark job (Python host; the C++ CLI ``pagerank`` is the same).

CLI: ``python -m sparky_hip <input-path> [iterations=10] [--format edges|ccjson]
[--out DIR] [--save-every-iter] [--dangling=local|none|seeds] [--device N] [--quiet]
[--resume DIR/PageRank<i>] [--devices D0,D1,...] [--top K] [--seeds FILE] [--seed-set FILE]...
[--exclude-seeds] [--tol X] [--seed-queue LISTFILE [--slots W]] [--dangling-to-seeds]
[--mix W0,W1,...]...``

* input: text edge list, ``src dst`` per line; a single-token line ``src`` is a record without
  ``a`` links (Sparky.java:114-118).  Tokens (URLs) are taken verbatim and interned to dense
  int32 IDs in first-appearance order, src before dst.
* stdout: ``Starting iter<i>`` before every iteration (Sparky.java:188), then
  ``<url> has rank: <r>.`` for every URL after the last iteration (north_star contract).
* ``--out DIR``: ``DIR/PageRank<i>/part-00000`` with ``(url,rank)`` lines -- Scala
  ``Tuple2.toString`` of ``(String, Double)`` with Java ``Double.toString`` -- plus an empty
  ``_SUCCESS`` (Sparky.java:237 ``saveAsTextFile``); only the last iteration unless
  ``--save-every-iter``.
* ``--resume DIR/PageRank<i>``: start from the ranks saved there (instead of 1.0,
  Sparky.java:165-170) and continue the same loop with iterations i+1 .. N-1 (a directory not
  named ``PageRank<i>`` starts the loop at 0).  Same rules as the C++ CLI.
* ``--top K``: the final listing is only the K highest-ranked URLs -- rank descending, ties by
  first appearance (ID ascending) -- selected on the GPU (``PageRankGraph.topk`` /
  ``PartGroup.topk``); without ``--out`` the rank vector never crosses to the host.
* ``--seeds FILE``: personalised PageRank.  One ``url`` or ``url weight`` per line (weight > 0,
  default 1; blank and ``#`` lines skipped): the teleport mass 0.15 N goes to the seeds in
  proportion to their weights, every other URL's teleport term is 0 (``prh_seed_teleport``, then
  ``set_teleport_sparse``); the dangling term stays uniform unless ``--dangling=seeds`` is given.
  The file is read and checked before the graph is created: a bad one exits with status 2 without
  touching a GPU.  Same outputs as the C++ CLI: ``pagerank edges.txt 20 --seeds seeds.txt --top 100``.
* ``--dangling=seeds`` (needs ``--seeds``, else a usage error before any GPU work): the run's dangling
  mass returns to the ``--seeds`` set in proportion to the weights instead of being spread over all
  URLs (``PageRankGraph.set_teleport_dangling("teleport")``): textbook personalised PageRank, in
  which a URL the seeds cannot reach drains to 0.  The graph counts its dangling mass as with
  ``--dangling=local``.  Works with ``--devices``, ``--top``, ``--out`` and ``--resume``; same bytes as
  the C++ CLI.  For ``--seed-set`` and ``--seed-queue`` the same choice is ``--dangling-to-seeds``.
* ``--seed-set FILE`` (1 to 16 times): batched personalised PageRank.  Every FILE is a seed file as
  for ``--seeds`` and gives one personalised ranking; all of them run as one batch
  (``PageRankBatch``), one pass over the graph per iteration for all sets.  Per set, in
  command-line order, the listing is a line ``# seed set <j>: <FILE>`` followed by that set's
  ``<url> has rank: <r>.`` lines (with ``--top K`` its K best); ``--out DIR`` writes
  ``DIR/seedset<j>/PageRank<last>/part-00000`` + ``_SUCCESS``.  Not with ``--seeds``,
  ``--devices``, ``--resume`` or ``--save-every-iter`` (usage errors, before any GPU work).  Same
  bytes as the C++ CLI.  With ``--top K`` the listings of all sets come from one select
  (``PageRankBatch.topk_all``).
* ``--exclude-seeds`` (needs ``--seed-set`` and ``--top``, else a usage error before any GPU work):
  every set's own seed URLs are left out of that set's ``--top`` listing
  (``PageRankBatch.set_exclude``); part files from ``--out`` stay complete.
* ``--tol X`` (needs ``--seed-set``, else a usage error before any GPU work; X a finite number >= 0):
  every set stops at its own convergence, decided on the GPU (``PageRankBatch.step_until``): a set is
  done after the first iteration whose L1 delta, on the unnormalised ranks, is at most X, and the
  iterations argument becomes the cap.  ``Starting iter<i>`` is printed for every i below the largest
  count; after each ``# seed set <j>: <FILE>`` line comes ``# iterations: <n_j> (converged)`` or
  ``(not converged)``; ``--out`` writes set j to ``DIR/seedset<j>/PageRank<n_j - 1>``.  Same bytes as
  the C++ CLI.
* ``--seed-queue LISTFILE`` (needs ``--tol`` and ``--top``; not with ``--seeds``, ``--seed-set``,
  ``--devices``, ``--resume`` or ``--save-every-iter``; usage errors before any GPU work): LISTFILE
  names one seed file per line (blank lines and ``#`` comments skipped), any number of them.  The
  sets are served by ``--slots W`` (1..16, default min(16, sets)) batch columns through
  ``PageRankBatch.run_queue``: a column whose set has converged (or has had ``iterations`` iterations
  of its own) takes the next set at once.  No ``Starting iter`` lines; per set, in queue order:
  ``# seed set <q>: <FILE>``, ``# iterations: <n> (converged)`` or ``(not converged)``, then its
  ``--top`` listing (with ``--exclude-seeds`` without its own seeds) -- the lines ``--seed-set FILE
  --tol X --top K`` prints for that file alone.  ``--out DIR`` writes set q to
  ``DIR/seedset<q>/PageRank<n - 1>``.  Same bytes as the C++ CLI.
* ``--dangling-to-seeds`` (needs ``--seed-set`` or ``--seed-queue``, else a usage error before any GPU
  work): every set's dangling mass returns to that set's own seeds, in proportion to their weights
  (``PageRankBatch.set_dangling("teleport")``), instead of being spread over all URLs: a URL the
  seeds cannot reach keeps rank 0.  A set whose teleport terms sum to 0 or overflow keeps the uniform term; with
  ``--dangling=none`` there is no dangling mass and the option changes nothing.  The mode is the
  whole run's, not a set's; for ``--seeds`` (the engine's own iteration) the same choice is
  ``--dangling=seeds``.  Output format unchanged, same bytes as the C++ CLI.
* ``--mix W0,W1,...`` (1 to 16 times; needs ``--seed-set`` and ``--top``, not with ``--seed-queue``; exactly
  one finite number per ``--seed-set`` file; anything else is a usage error before any GPU work): after
  the per-set listings, mix i prints ``# mix <i>: <the weights as given>`` and the ``--top`` listing of
  the blend ``sum_j W_j * ranks_j`` of the sets' rankings, all mixes from one
  ``PageRankBatch.mix_topk`` call and no further iteration.  Negative weights are allowed (``1,-0.25``:
  what set 0 ranks highly and set 1 does not).  With ``--exclude-seeds`` a mix leaves out the seeds of
  every set it gives a non-zero weight.  The per-set output is that of the run without ``--mix``.  Same
  bytes as the C++ CLI.
"""
from __future__ import annotations

import argparse
import math
import os
import sys
from typing import Dict, Iterable, List, Sequence, TextIO, Tuple

import numpy as np

from .graph import PageRankGraph, PartGroup


def java_double_to_string(x: float) -> str:
    """``Double.toString`` (shortest-uniquely-distinguishing digits, JDK 19+ algorithm).

    Layout per the JDK spec: decimal notation for 1e-3 <= |x| < 1e7 with at least one digit
    after the point; otherwise ``d.dddE<exp>``.  JDK <= 18 (Spark 1.x era) emits a longer,
    non-shortest digit string for a few values (JDK-4511638); parity tests therefore compare
    parsed numbers, never strings.
    """
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"
    if x == 0.0:
        return "-0.0" if math.copysign(1.0, x) < 0 else "0.0"
    sign = "-" if x < 0 else ""
    ax = abs(x)
    r = repr(ax)  # shortest round-trip digits
    if "e" in r or "E" in r:
        mant, exp = r.lower().split("e")
        e10 = int(exp)
    else:
        mant, e10 = r, 0
    if "." in mant:
        ip, fp = mant.split(".")
    else:
        ip, fp = mant, ""
    digits = (ip + fp).lstrip("0")
    # position of the decimal point relative to the first significant digit
    lead_zeros = len(ip + fp) - len((ip + fp).lstrip("0"))
    point = len(ip) - lead_zeros + e10  # value = 0.digits * 10^point
    digits = digits.rstrip("0") or "0"
    if len(digits) == 1:
        # JDK 19+ renders at least two significant digits and picks the 2-digit decimal
        # closest to the value when the 1-digit shortest is not (e.g. 4.9E-324, not 5.0E-324).
        m2, e2 = f"{ax:.1e}".split("e")
        d2 = m2.replace(".", "").rstrip("0") or "0"
        digits, point = d2, int(e2) + 1
    if 1e-3 <= ax < 1e7:
        if point <= 0:
            s = "0." + "0" * (-point) + digits
        elif point >= len(digits):
            s = digits + "0" * (point - len(digits)) + ".0"
        else:
            s = digits[:point] + "." + digits[point:]
        return sign + s
    frac = digits[1:] or "0"
    return f"{sign}{digits[0]}.{frac}E{point - 1}"


def read_edge_list(lines: Iterable[str]) -> Tuple[List[str], np.ndarray, np.ndarray]:
    """Tokenise and intern (first appearance, src before dst).  Returns (urls, src, dst)."""
    ids: Dict[str, int] = {}
    urls: List[str] = []
    src: List[int] = []
    dst: List[int] = []
    for ln, line in enumerate(lines):
        toks = line.split()
        if not toks:
            continue
        if len(toks) > 2:
            raise ValueError(f"line {ln + 1}: expected 'src [dst]', got {len(toks)} tokens")
        u = toks[0]
        iu = ids.get(u)
        if iu is None:
            iu = ids[u] = len(urls)
            urls.append(u)
        src.append(iu)
        if len(toks) == 1:
            dst.append(-1)
        else:
            v = toks[1]
            iv = ids.get(v)
            if iv is None:
                iv = ids[v] = len(urls)
                urls.append(v)
            dst.append(iv)
    return urls, np.asarray(src, np.int32), np.asarray(dst, np.int32)


def write_part_file(out_dir: str, iteration: int, urls: Sequence[str], ranks: np.ndarray) -> str:
    """``ranks.saveAsTextFile(out_dir + "/PageRank" + iter + "/")`` (Sparky.java:237)."""
    d = os.path.join(out_dir, f"PageRank{iteration}")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "part-00000"), "w") as f:
        for u, r in zip(urls, ranks.tolist()):
            f.write(f"({u},{java_double_to_string(r)})\n")
    open(os.path.join(d, "_SUCCESS"), "w").close()
    return d


def write_has_rank(stream: TextIO, urls: Sequence[str], ranks: np.ndarray) -> None:
    for u, r in zip(urls, ranks.tolist()):
        stream.write(f"{u} has rank: {java_double_to_string(r)}.\n")


def saved_iteration(path: str) -> int:
    """i of a ``.../PageRank<i>`` directory, or -1."""
    base = os.path.basename(os.path.normpath(path))
    if base.startswith("PageRank") and base[8:].isdigit():
        return int(base[8:])
    return -1


def _run_group(edges, devices, dangling, n_run, init, cb, want_ranks, top=0, seeds=None, dangling_seeds=False):
    """--devices: one part per listed device, one process (pr_group_*); the callback gets the
    merged ranks of every part after each iteration, as with PageRankGraph.run.  Returns the
    final ranks, or with top > 0 the (ids, ranks) of PartGroup.topk(top)."""
    P = len(devices)
    parts = []
    try:
        for p, d in enumerate(devices):
            parts.append(PageRankGraph(edges.n_vertices, edges.src, edges.dst, device=d, dangling=dangling,
                                       keep_canonical=False, part=p, n_parts=P))
        grp = PartGroup(parts)
        if seeds is not None:
            grp.set_teleport_sparse(*seeds)
        if dangling_seeds:  # --dangling=seeds: every part alike
            grp.set_teleport_dangling("teleport")
        grp.reset(init_ranks=init)
        for it in range(n_run):
            grp.step(1)
            grp.sync()
            cb(it, grp.ranks() if want_ranks else None, None)
        return grp.topk(top) if top > 0 else grp.ranks()
    finally:
        for g in parts:
            g.close()


def _run_seed_sets(edges, a, sets, top, out) -> None:
    """--seed-set: every set is one column of a batch over one graph (which keeps its canonical
    CSR: the batch runs over it).  The iteration lines, then per set its header and listing."""
    from .batch import PageRankBatch

    with PageRankGraph(edges.n_vertices, edges.src, edges.dst, device=a.device, dangling=a.dangling) as g:
        with PageRankBatch(g, len(sets)) as b:
            if a.dangling_to_seeds:
                b.set_dangling("teleport")
            for j, (ids, values) in enumerate(sets):
                b.set_teleport_sparse(j, ids, values)
            b.reset()
            # iterations applied to every set: the argument, or with --tol each set's own count
            n_it = [a.iterations] * len(sets)
            if a.tol is not None:
                n_it = [int(n) for n in b.step_until(a.iterations, a.tol)]
                _, l1 = b.norms()
                converged = [n > 0 and x <= a.tol for n, x in zip(n_it, l1.tolist())]
                for it in range(max(n_it)):
                    out.write(f"Starting iter{it}\n")
            else:
                for it in range(a.iterations):
                    out.write(f"Starting iter{it}\n")
                    b.step(1)
            if a.exclude_seeds:  # a set's own seeds never appear in its listing
                for j, (ids, _) in enumerate(sets):
                    b.set_exclude(j, ids)
            # the listings of all sets from one select (PageRankBatch.topk_all)
            tops = b.topk_all(min(top, edges.n_vertices)) if top and not a.quiet else None
            for j in range(len(sets)):
                ranks = b.ranks(j) if a.out or (not top and not a.quiet) else None
                if a.out and n_it[j] > 0:
                    edges.write_part(os.path.join(a.out, f"seedset{j}"), n_it[j] - 1, ranks)
                if a.quiet:
                    continue
                out.write(f"# seed set {j}: {a.seed_set[j]}\n")
                if a.tol is not None:
                    out.write(f"# iterations: {n_it[j]} ({'converged' if converged[j] else 'not converged'})\n")
                out.flush()
                if top:
                    edges.write_has_rank_ids(None, *tops[j])
                else:
                    edges.write_has_rank(None, ranks)
            if a.mix and not a.quiet:  # the listings of all mixes from one call (PageRankBatch.mix_topk)
                weights = np.array(a.mix_weights, np.float64)
                excl = None
                if a.exclude_seeds:  # a mix leaves out the seeds of every set it gives a non-zero weight
                    excl = [np.unique(np.concatenate([np.zeros(0, np.int32)] +
                                                     [sets[j][0] for j in range(len(sets)) if w[j] != 0.0]))
                            for w in weights]
                lists = b.mix_topk(weights, min(top, edges.n_vertices), excl)
                for i, given in enumerate(a.mix):
                    out.write(f"# mix {i}: {given}\n")
                    out.flush()
                    edges.write_has_rank_ids(None, *lists[i])


def read_seed_queue(path: str) -> List[str]:
    """--seed-queue: the list file's seed-file paths; blank lines and ``#`` comments are skipped."""
    with open(path, "r") as f:
        lines = [ln.strip(" \t\r\n") for ln in f]
    return [ln for ln in lines if ln and not ln.startswith("#")]


def _run_seed_queue(edges, a, files, sets, top, out) -> None:
    """--seed-queue: the sets go through the columns of one batch (PageRankBatch.run_queue).  Per
    set, in queue order, its header, its iteration count and its --top listing."""
    from .batch import PageRankBatch

    if not sets:
        return
    width = a.slots or min(16, len(sets))
    queries = [(ids, values, 0.0, ids if a.exclude_seeds else None) for ids, values in sets]
    with PageRankGraph(edges.n_vertices, edges.src, edges.dst, device=a.device, dangling=a.dangling) as g:
        with PageRankBatch(g, width) as b:
            if a.dangling_to_seeds:
                b.set_dangling("teleport")
            b.reset()

            def on_done(q, column, rec):
                if a.out:
                    edges.write_part(os.path.join(a.out, f"seedset{q}"), rec["iterations"] - 1, b.ranks(column))

            recs = b.run_queue(queries, a.iterations, a.tol, k=None if a.quiet else min(top, edges.n_vertices),
                               on_done=on_done)
    if a.quiet:
        return
    for q, rec in enumerate(recs):
        out.write(f"# seed set {q}: {files[q]}\n")
        out.write(f"# iterations: {rec['iterations']} ({'converged' if rec['converged'] else 'not converged'})\n")
        out.flush()
        edges.write_has_rank_ids(None, *rec["topk"])


def parse_mix(text: str, n: int):
    """--mix: ``n`` comma-separated finite numbers in plain decimal or exponent form; None if not."""
    toks = text.split(",")
    if len(toks) != n or any(not t or set(t) - set("0123456789+-.eE") for t in toks):
        return None
    try:
        w = [float(t) for t in toks]
    except ValueError:
        return None
    return w if all(math.isfinite(x) for x in w) else None


def main(argv=None) -> int:
    from ._host import HostEdges, HostError, seed_teleport

    # "--mix -1,0.5": the value starts with '-', which argparse would read as an option
    argv = list(sys.argv[1:] if argv is None else argv)
    for i in range(len(argv) - 1, 0, -1):
        if argv[i - 1] == "--mix":
            argv[i - 1: i + 1] = ["--mix=" + argv[i]]

    ap = argparse.ArgumentParser(prog="sparky_hip", description=__doc__.splitlines()[0])
    ap.add_argument("edge_list")
    ap.add_argument("iterations", nargs="?", type=int, default=10)  # Sparky.java:187
    ap.add_argument("--format", choices=["edges", "ccjson"], default="edges")
    ap.add_argument("--out", default=None)
    ap.add_argument("--save-every-iter", action="store_true")
    ap.add_argument("--dangling", choices=["local", "none", "seeds"], default="local",
                    help="seeds (with --seeds): the run's dangling mass returns to the seeds instead of all URLs")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--quiet", action="store_true", help="omit the '<url> has rank' lines")
    ap.add_argument("--resume", default=None, metavar="DIR", help="start from saved (url,rank) part files")
    ap.add_argument("--devices", default=None, metavar="D0,D1,...",
                    help="one row part per listed GPU (a device may repeat), one process (pr_group_*)")
    ap.add_argument("--top", type=int, default=None, metavar="K",
                    help="list only the K highest-ranked URLs (selected on the GPU)")
    ap.add_argument("--seeds", default=None, metavar="FILE",
                    help="personalised PageRank: seed URLs, one 'url' or 'url weight' per line")
    ap.add_argument("--seed-set", action="append", default=None, metavar="FILE",
                    help="batched personalised PageRank: 1 to 16 seed files, run as one batch; not with --seeds, "
                         "--devices, --resume or --save-every-iter")
    ap.add_argument("--exclude-seeds", action="store_true",
                    help="with --seed-set and --top: a set's own seed URLs are left out of its listing")
    ap.add_argument("--tol", default=None, metavar="X",
                    help="with --seed-set: every set stops once its L1 delta is <= X; iterations is the cap")
    ap.add_argument("--seed-queue", default=None, metavar="LISTFILE",
                    help="a queue of seed sets (one seed-file path per line) served by --slots batch columns that are "
                         "refilled as sets converge; needs --tol and --top")
    ap.add_argument("--slots", default=None, metavar="W", help="with --seed-queue: the batch width, 1..16")
    ap.add_argument("--dangling-to-seeds", action="store_true",
                    help="with --seed-set or --seed-queue: a set's dangling mass returns to its own seeds instead of "
                         "all URLs; a set whose teleport terms sum to 0 or overflow keeps the uniform term; the whole run's "
                         "mode, not a set's; for --seeds: --dangling=seeds")
    ap.add_argument("--mix", action="append", default=None, metavar="W0,W1,...",
                    help="with --seed-set and --top, 1 to 16 times: also list the K best URLs of the weighted blend of "
                         "the sets' rankings, one finite weight per --seed-set; not with --seed-queue")
    a = ap.parse_args(argv)
    if a.mix:
        if a.seed_queue is not None:
            ap.error("--mix does not combine with --seed-queue")
        if not a.seed_set or a.top is None:
            ap.error("--mix needs --seed-set and --top")
        if len(a.mix) > 16:
            ap.error("--mix: at most 16 mixes")
        a.mix_weights = [parse_mix(m, len(a.seed_set)) for m in a.mix]
        if any(w is None for w in a.mix_weights):
            ap.error("--mix takes one finite weight per --seed-set, separated by commas")
    if a.slots is not None:
        if not (a.slots.isdigit() and len(a.slots) <= 2 and 1 <= int(a.slots) <= 16):
            ap.error("--slots takes a count W in 1..16")
        a.slots = int(a.slots)
    if a.tol is not None:
        try:
            a.tol = float(a.tol)
        except ValueError:
            a.tol = math.nan
        if not (math.isfinite(a.tol) and a.tol >= 0.0):
            ap.error("--tol: not a finite number >= 0")
        if not a.seed_set and a.seed_queue is None:
            ap.error("--tol needs --seed-set")
    if a.dangling_to_seeds and not (a.seed_set or a.seed_queue is not None):
        ap.error("--dangling-to-seeds needs --seed-set or --seed-queue")
    dangling_seeds = a.dangling == "seeds"
    if dangling_seeds:
        if a.seeds is None:
            ap.error("--dangling=seeds needs --seeds" if not (a.seed_set or a.seed_queue is not None) else
                     "--dangling=seeds needs --seeds; with --seed-set or --seed-queue use --dangling-to-seeds")
        a.dangling = "local"  # the graph counts its dangling mass; the handle's mode returns it to the seeds
    if a.seed_queue is not None:
        if a.seeds is not None or a.seed_set or a.devices is not None or a.resume or a.save_every_iter:
            ap.error("--seed-queue does not combine with --seeds, --seed-set, --devices, --resume or --save-every-iter")
        if a.tol is None or a.top is None:
            ap.error("--seed-queue needs --tol and --top")
        if a.top >= 1 and a.iterations < 1:
            ap.error("--seed-queue: iterations (the cap of every set) must be >= 1")
    elif a.slots is not None:
        ap.error("--slots needs --seed-queue")
    if a.exclude_seeds and not ((a.seed_set or a.seed_queue is not None) and a.top is not None):
        ap.error("--exclude-seeds needs --seed-set and --top")
    if a.top is not None and a.top < 1:
        ap.error("--top takes a count K >= 1")
    top = a.top or 0
    if a.seed_set:
        if a.seeds is not None:
            ap.error("--seeds and --seed-set are exclusive")
        if len(a.seed_set) > 16:
            ap.error("--seed-set: at most 16 seed sets")
        if a.devices is not None or a.resume or a.save_every_iter:
            ap.error("--seed-set does not combine with --devices, --resume or --save-every-iter")
    devices = [a.device]
    if a.devices is not None:
        try:
            devices = [int(t) for t in a.devices.split(",")]
        except ValueError:
            ap.error("--devices takes a comma-separated list of device numbers")
    edges = HostEdges.read(a.edge_list, a.format)  # native front-end + first-appearance interning
    seeds = None
    if a.seeds is not None:  # read and checked before any graph exists
        try:
            ids, weights = edges.read_seeds(a.seeds)
        except HostError as e:
            sys.stderr.write(f"sparky_hip: --seeds: {e}\n")
            edges.close()
            return 2
        seeds = (ids, seed_teleport(weights, edges.n_vertices))  # the native expression: the C++ CLI's bits
    out = sys.stdout
    if a.seed_queue is not None:  # the list and every file read and checked before any graph exists
        try:
            files = read_seed_queue(a.seed_queue)
        except OSError:
            sys.stderr.write(f"sparky_hip: --seed-queue {a.seed_queue}: cannot open the list file\n")
            edges.close()
            return 2
        sets = []
        for path in files:
            try:
                ids, weights = edges.read_seeds(path)
            except HostError as e:
                sys.stderr.write(f"sparky_hip: --seed-queue {path}: {e}\n")
                edges.close()
                return 2
            sets.append((ids, seed_teleport(weights, edges.n_vertices)))
        _run_seed_queue(edges, a, files, sets, top, out)
        out.flush()
        edges.close()
        return 0
    if a.seed_set:  # every file read and checked before any graph exists
        sets = []
        for path in a.seed_set:
            try:
                ids, weights = edges.read_seeds(path)
            except HostError as e:
                sys.stderr.write(f"sparky_hip: --seed-set {path}: {e}\n")
                edges.close()
                return 2
            sets.append((ids, seed_teleport(weights, edges.n_vertices)))
        _run_seed_sets(edges, a, sets, top, out)
        out.flush()
        edges.close()
        return 0
    init, start = None, 0
    if a.resume:
        init = edges.read_ranks(a.resume)
        start = saved_iteration(a.resume) + 1
    n_run = max(a.iterations - start, 0)
    # Sparky prints "Starting iter<i>" before each iteration (Sparky.java:188); the library
    # calls back after iteration i, so the host prints the next line there.
    def cb(it_run, ranks, _st):
        it = start + it_run
        if a.out and (a.save_every_iter or it == a.iterations - 1):
            edges.write_part(a.out, it, ranks)
        if it + 1 < a.iterations:
            out.write(f"Starting iter{it + 1}\n")

    if n_run > 0:
        out.write(f"Starting iter{start}\n")
    if len(devices) == 1:
        with PageRankGraph(edges.n_vertices, edges.src, edges.dst, device=devices[0], dangling=a.dangling,
                           keep_canonical=False) as g:
            if seeds is not None:
                g.set_teleport_sparse(*seeds)
            if dangling_seeds:
                g.set_teleport_dangling("teleport")
            if top and not a.out:  # no part file: the ranks stay on the device
                g.reset(init_ranks=init)
                for it in range(n_run):
                    g.step(1)
                    cb(it, None, None)
            else:
                ranks, _ = g.run(n_run, callback=cb, want_ranks_in_callback=bool(a.out), init_ranks=init)
            if top:
                ranks = g.topk(top)
    else:
        ranks = _run_group(edges, devices, a.dangling, n_run, init, cb, bool(a.out), top, seeds, dangling_seeds)
    out.flush()
    if not a.quiet and top:
        edges.write_has_rank_ids(None, *ranks)
    elif not a.quiet:
        edges.write_has_rank(None, ranks)
    edges.close()
    return 0

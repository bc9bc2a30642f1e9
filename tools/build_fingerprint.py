#!/usr/bin/env python3
"""Fingerprint of what the graph build produces, for comparing two builds of libpagerank_hip.

    PR_LIB_PATH=/path/to/parent/libpagerank_hip.so tools/build_fingerprint.py --out parent.json
    tools/build_fingerprint.py --out this.json
    cmp parent.json this.json

For a fixed list of small shapes -- every layout, class count, entry code, hot-set size, epilogue
variant and exchange form the build decides between, one part and parts of a row partition -- the
graph is built, given per-vertex random initial ranks from a fixed seed and stepped three
iterations (parts as a PartGroup).  Per handle the output holds every field of info() (device_bytes
included), the bit patterns of last_dc and last_l1 and a SHA-256 of the rank bytes: one JSON line
per shape, nothing that depends on time or place, so two libraries that build the same graph write
byte-identical files.  The whole list takes a few seconds on one GPU.
"""
import argparse
import hashlib
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pagerank-using-apache-spark_amd"))


def random_edges(V, E, seed, hub=0, nolink=0.05):
    """E random edges, `hub` more into vertex 0, some records without links, every ID present."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, V, E).astype(np.int32)
    dst = rng.integers(0, V, E).astype(np.int32)
    dst[rng.random(E) < nolink] = -1
    if hub:
        src = np.concatenate([src, rng.permutation(V)[:hub].astype(np.int32)])
        dst = np.concatenate([dst, np.zeros(hub, np.int32)])
    src = np.concatenate([src, np.arange(V, dtype=np.int32)])
    dst = np.concatenate([dst, np.full(V, -1, np.int32)])
    return src, dst


def skewed_edges(V, E, seed):
    """Sources drawn with a heavy head, so out-degrees (the hot order) and class loads differ."""
    rng = np.random.default_rng(seed)
    src = np.minimum((V * rng.random(E) ** 3).astype(np.int64), V - 1).astype(np.int32)
    dst = rng.integers(0, V, E).astype(np.int32)
    src = np.concatenate([src, np.arange(V, dtype=np.int32)])
    dst = np.concatenate([dst, np.full(V, -1, np.int32)])
    return src, dst


V40K = 40_000
SPLIT40K = dict(edges=("skewed", V40K, 400_000, 11), layout="split")
# name -> edges (kind, V, E, seed[, hub]), parts, layout and the other PageRankGraph arguments
SHAPES = [
    dict(name="fused_by_size", edges=("random", 5000, 60_000, 1)),
    dict(name="fused_hub_row", edges=("random", 6000, 40_000, 2, 3000)),
    dict(name="fused_tiny", edges=("random", 3, 7, 3)),
    *[dict(name=f"split_c{c}", options={"classes": c}, **SPLIT40K) for c in (8, 16, 64, 128)],
    *[dict(name=f"split_hot_slots_{k}", options={"classes": 8, "hot_slots": k}, **SPLIT40K) for k in (-1, 0, 40)],
    *[dict(name=f"split_codes_{k}", options={"classes": 8, "codes": k}, **SPLIT40K) for k in (-1, 0)],
    dict(name="split_epi_walk_0", options={"classes": 16, "epi_walk": 0}, **SPLIT40K),
    *[dict(name=f"split_epi_narrow_{k}", options={"classes": 16, "epi_narrow": k}, **SPLIT40K) for k in (0, 1)],
    *[dict(name=f"split_epi_order_{k}", options={"classes": 16, "epi_order": k}, **SPLIT40K) for k in (0, 1, 2)],
    dict(name="split_hub_row", edges=("random", V40K, 300_000, 12, 9000), layout="split", options={"classes": 8}),
    dict(name="split_dangling_none", dangling="none", options={"classes": 8}, **SPLIT40K),
    dict(name="fused_dangling_none", edges=("random", 5000, 60_000, 1), dangling="none"),
    dict(name="split_no_canonical", keep_canonical=False, options={"classes": 8}, **SPLIT40K),
    dict(name="fused_no_canonical", edges=("random", 5000, 60_000, 1), keep_canonical=False),
    dict(name="split_device_input", device_input=True, options={"classes": 8}, **SPLIT40K),
    dict(name="fused_device_input", edges=("random", 5000, 60_000, 1), device_input=True),
    *[dict(name=f"parts{P}_{lay}", parts=P, edges=("skewed", V40K, 400_000, 20 + P), layout=lay,
           options={"classes": 8} if lay == "split" else None) for P in (2, 3, 8, 9) for lay in ("split", "fused")],
    dict(name="parts4_allgather", parts=4, options={"classes": 8, "exchange_allgather": 1}, **SPLIT40K),
    dict(name="parts4_pack_fused_0", parts=4, options={"classes": 8, "pack_fused": 0}, **SPLIT40K),
    dict(name="parts8_codes_0", parts=8, options={"classes": 16, "codes": 0}, **SPLIT40K),
    dict(name="parts8_hot_slots_40", parts=8, options={"classes": 8, "hot_slots": 40}, **SPLIT40K),
    dict(name="parts8_V_lt_P", parts=8, edges=("random", 3, 7, 3)),
    dict(name="parts8_V_lt_P_split", parts=8, edges=("random", 5, 12, 4), layout="split", options={"classes": 8}),
    # class regions past 2^19 rows: the 24-bit codes, of one part and of parts
    dict(name="split_c24", edges=("random", 6_000_000, 12_000_000, 30), layout="split", options={"classes": 8}),
    dict(name="parts2_c24p", parts=2, edges=("random", 6_000_000, 12_000_000, 30), layout="split", options={"classes": 8}),
    dict(name="rmat_s20", edges=("rmat", 20)),
    dict(name="rmat_s20_parts2", parts=2, edges=("rmat", 20)),
]


def bits(x):
    return struct.pack("<d", float(x)).hex()


def fingerprint(shape, hip, torch):
    kind, *a = shape["edges"]
    keep = []  # device tensors the handles read during the build
    if kind == "rmat":
        scale = a[0]
        E = 16 << scale
        s = torch.empty(E, dtype=torch.int32, device="cuda")
        d = torch.empty(E, dtype=torch.int32, device="cuda")
        hip.gen_rmat(0, scale, E, s.data_ptr(), d.data_ptr(), seed=1)
        V = hip.intern_device(0, E, 1 << scale, s.data_ptr(), d.data_ptr())
        torch.cuda.synchronize()
        device_input = True
    else:
        V = a[0]
        src, dst = random_edges(*a) if kind == "random" else skewed_edges(*a)
        E = len(src)
        device_input = bool(shape.get("device_input"))
        if device_input:
            s, d = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
            torch.cuda.synchronize()
    if device_input:
        keep = [s, d]
        src, dst = s.data_ptr(), d.data_ptr()
    P = shape.get("parts", 1)
    kw = dict(dangling=shape.get("dangling", "local"), keep_canonical=shape.get("keep_canonical", True),
              layout=shape.get("layout", "auto"), options=shape.get("options"))
    if device_input:
        kw.update(device_input=True, n_edges=E)
    parts = [hip.PageRankGraph(V, src, dst, part=p, n_parts=P, **kw) for p in range(P)]
    init = np.random.default_rng(99).random(V) + 0.5
    init /= init.sum()
    drv = parts[0] if P == 1 else hip.PartGroup(parts)
    drv.reset(init_ranks=init)
    drv.step(3)
    drv.sync()
    handles = []
    for g in parts:
        st = g.stats()
        out = np.full(max(V, 1), np.nan)
        g.ranks(out)
        handles.append(dict(info=g.info(), iters=int(st["iters"]), last_dc=bits(st["last_dc"]), last_l1=bits(st["last_l1"]),
                            ranks_sha256=hashlib.sha256(out[:V].tobytes()).hexdigest()))
    for g in parts:
        g.close()
    del keep
    return dict(name=shape["name"], n_vertices=int(V), n_raw_edges=int(E), parts=handles)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True, help="file to write, one JSON line per shape")
    ap.add_argument("--only", default=None, help="comma-separated shape names (default: all)")
    a = ap.parse_args()
    import torch

    import sparky_hip as hip

    only = set(a.only.split(",")) if a.only else None
    with open(a.out, "w") as f:
        for shape in SHAPES:
            if only and shape["name"] not in only:
                continue
            f.write(json.dumps(fingerprint(shape, hip, torch), sort_keys=True) + "\n")
            f.flush()
            print(f"{shape['name']}: done", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

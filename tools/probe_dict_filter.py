#!/usr/bin/env python3
"""What predicates over kept dictionaries cost and save on the SF1 table.

Row group 0 (1,048,576 rows, 16 columns) of the lineitem-shaped SF1 table, written by the GPU writer as
tools/probe_row_filter.py writes it, is uploaded once (device-resident input) and decoded three ways, all 16 columns
returned:
  (i)   filtered, no keep flags      pf_decode_row_group_filter: every chunk expanded, the predicate row by row
  (ii)  filtered, every chunk asked  pf_decode_row_group_dict_filter: eligible chunks stay indices + dictionary, a
                                     RANGE on one is matched once per dictionary entry (k_sel_dict) and looked up per row
  (iii) the full kept decode         pf_decode_row_group_dict, for reference
under three predicates: Eq on l_shipmode (a 7-entry string dictionary), Range("l_quantity", hi=1) (about 2 % of the rows)
and Range("l_quantity", hi=25) (about half). Per route: the wall time of decode + wait (median and range), the filter
stage's kernels (HIP events, pf_debug_filter), the bytes fetch() brings back. (i) is checked against (ii) row for row
after materialize().

    python tools/probe_dict_filter.py [--out profiles/dict_filter_sf1.json] [--reps 20] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_filter_sf1.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "parquet-floor_amd"))
    from probe_write_hybrid import RG_ROWS, columns
    from pfloor import _native
    from pfloor import writer as W
    from pfloor.decoder import GpuDecoder, ParquetFile, materialize
    from pfloor.predicate import Eq, Range, bind
    cols = columns()
    names = list(cols)
    dec = GpuDecoder(0)
    dec.set_timing(True)
    has_kept = hasattr(dec, "decode_kept")   # (the parent of this feature: route (i) only)
    out = {"rows": RG_ROWS, "columns": len(names), "reps": args.reps, "warmup": args.warmup, "kept_route": has_kept}
    L = _native.lib()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "sf1_rg0.parquet")
        w = W.ParquetWriter(W.MessageType("lineitem", *[cols[n][0] for n in names]), path, None, decoder=dec, page_index=True)
        w.write_columns({n: cols[n][1] for n in names}, RG_ROWS)
        w.close()
        with ParquetFile(path) as f:
            idx = list(range(f.num_columns))
            types = [(f.columns[c].physical_type, f.columns[c].max_def, f.columns[c].max_rep) for c in idx]
            items, total = f.plan([0], idx)
            host = dec.staging(total)
            descs = []
            for _rg, c, s, n, off in items:
                f.read_into(s, n, host.ptr.value + off)
                descs.append(f.chunk_desc(0, c, off))
            arr = (_native.ChunkDesc * len(descs))(*descs)
            dptr = C.c_void_p()
            _native.check(L.pf_device_alloc(dec.h, total, C.byref(dptr)), dec.h, "pf_device_alloc")
            _native.check(L.pf_memcpy_h2d(dec.h, dptr, host.ptr, total), dec.h, "pf_memcpy_h2d")
            _native.check(L.pf_sync(dec.h), dec.h, "pf_sync")
            # a ship mode that occurs: the first row's
            sm = cols["l_shipmode"][1]
            offs, chars = np.asarray(sm[0]), np.asarray(sm[1], np.uint8)
            mode = chars[offs[0]:offs[1]].tobytes()
            qty = np.asarray(cols["l_quantity"][1] if not isinstance(cols["l_quantity"][1], tuple) else cols["l_quantity"][1][0])
            one, half = (1.0, 25.0) if qty.dtype.kind == "f" else (1, 25)
            cases = {"eq_shipmode": [Eq("l_shipmode", mode)], "quantity_le_1": [Range("l_quantity", None, one)],
                     "quantity_le_25": [Range("l_quantity", None, half)]}
            keep = [True] * len(descs)

            def run(route, native):
                t0 = time.perf_counter()
                if route == "expanded":
                    dec.decode(arr, dptr.value, total, on_device=True, predicates=native)
                elif route == "kept":
                    dec.decode_kept(arr, dptr.value, total, on_device=True, keep=keep, predicates=native)
                else:
                    dec.decode(arr, dptr.value, total, on_device=True, keep=keep)
                dec.n_chunks = len(descs)
                assert dec.wait() == 0, dec.error()
                return (time.perf_counter() - t0) * 1e3, (dec.filter_ms() if native else 0.0)

            def fetch_all():
                t0 = time.perf_counter()
                arrs = [dec.fetch(i, *types[i]) for i in range(len(idx))]
                ms = (time.perf_counter() - t0) * 1e3
                nbytes = 0
                for a in arrs:
                    nbytes += sum(v.nbytes for v in a.values() if isinstance(v, np.ndarray))
                    if "dictionary" in a:
                        nbytes += sum(v.nbytes for v in a["dictionary"].values() if isinstance(v, np.ndarray))
                return arrs, nbytes, ms

            for name, preds in cases.items():
                native = bind(preds, f.columns, {c: i for i, c in enumerate(idx)})
                res = {}
                for route in (("expanded", "kept") if has_kept else ("expanded",)):
                    wall, stage, fetch_ms = [], [], []
                    for r in range(args.warmup + args.reps):
                        a, b = run(route, native)
                        arrs, nbytes, fms = fetch_all()
                        if r >= args.warmup:
                            wall.append(a)
                            stage.append(b)
                            fetch_ms.append(fms)
                    rows_in, sel = dec.selection()
                    res[route] = (arrs, sel)
                    out.setdefault(name, {})[route] = {
                        "decode_wait_ms": stats(wall), "filter_stage_ms": stats(stage), "fetch_ms": stats(fetch_ms), "d2h_bytes": int(nbytes),
                        "rows_in": int(rows_in), "rows_selected": int(len(sel)), "chunks_kept": sum("indices" in x for x in arrs)}
                if has_kept:   # both routes return the same rows and, materialized, the same bytes
                    (ea, es), (ka, ks) = res["expanded"], res["kept"]
                    assert np.array_equal(es, ks), name
                    for i in range(len(idx)):
                        m = materialize(ka[i], types[i][0])
                        for k, v in ea[i].items():
                            if isinstance(v, np.ndarray):
                                assert np.array_equal(v.view(np.uint8), np.asarray(m[k]).view(np.uint8)), (name, names[i], k)
                    e, k = out[name]["expanded"], out[name]["kept"]
                    out[name]["expanded_over_kept"] = {
                        "d2h_bytes": round(e["d2h_bytes"] / max(k["d2h_bytes"], 1), 3),
                        "filter_stage_ms": round(e["filter_stage_ms"]["median"] / max(k["filter_stage_ms"]["median"], 1e-9), 3),
                        "decode_wait_ms": round(e["decode_wait_ms"]["median"] / max(k["decode_wait_ms"]["median"], 1e-9), 3)}
            if has_kept:   # (iii) the full kept decode
                wall, fetch_ms = [], []
                for r in range(args.warmup + args.reps):
                    a, _b = run("full", None)
                    arrs, nbytes, fms = fetch_all()
                    if r >= args.warmup:
                        wall.append(a)
                        fetch_ms.append(fms)
                out["full_kept_decode"] = {"decode_wait_ms": stats(wall), "fetch_ms": stats(fetch_ms), "d2h_bytes": int(nbytes),
                                           "chunks_kept": sum("indices" in x for x in arrs)}
            L.pf_device_free(dec.h, dptr)
    dec.close()
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What a filtered read costs and saves on the SF1 table.

Row group 0 (1,048,576 rows, 16 columns) of the lineitem-shaped SF1 table is written by the GPU writer with
page_index=True (default pages of 20,000 rows). Two conjunctions are read with prune_row_group / plan_rows /
decode(windows=, predicates=) / fetch / selection across all 16 columns:
  (a) Eq("l_orderkey", k): the page index narrows the row group to one page, the GPU filter to the key's rows;
  (b) Range("l_quantity", hi=1): an unsorted column the index cannot narrow, so the whole row group is decoded and
      the GPU filter keeps about 2 % of it.
Each is compared with a full decode plus fetch of the same row group and the same filter in numpy on the host, on the
same context: file bytes read, H2D bytes, D2H bytes, the wall time of decode + wait + fetch (+ the host filter; the file
reads are timed apart) and the filter kernels' time (HIP events, pf_debug_filter).

    python tools/probe_row_filter.py [--out profiles/row_filter_sf1.json] [--reps 200] [--full-reps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {0: np.uint8, 1: np.int32, 2: np.int64, 4: np.float32, 5: np.float64}


def med(xs):
    return round(float(np.median(xs)), 4)


def host_take(a, ptype, idx):
    """The host side of the comparison: one fetched chunk compacted to rows idx with numpy."""
    out = {}
    if ptype == 6:
        off = a["offsets"].astype(np.int64)
        lens = off[idx + 1] - off[idx]
        noff = np.zeros(len(idx) + 1, np.int64)
        np.cumsum(lens, out=noff[1:])
        src = np.repeat(off[idx] - noff[:-1], lens) + np.arange(noff[-1])
        out["offsets"], out["chars"] = noff.astype(np.int32), a["chars"][src]
    else:
        w = int(a["width"])
        out["values"] = a["values"].reshape(-1, w)[idx].ravel()
    if "validity" in a:
        out["validity"] = np.packbits(np.unpackbits(a["validity"], bitorder="little")[idx], bitorder="little")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "row_filter_sf1.json"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--full-reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "parquet-floor_amd"))
    from probe_write_hybrid import RG_ROWS, columns
    from pfloor import writer as W
    from pfloor.decoder import GpuDecoder, ParquetFile
    from pfloor.predicate import Eq, Range, bind
    cols = columns()
    names = list(cols)
    dec = GpuDecoder(0)
    dec.set_timing(True)
    out = {"rows": RG_ROWS, "columns": len(names), "reps": args.reps, "full_reps": args.full_reps, "warmup": args.warmup}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "sf1_rg0.parquet")
        w = W.ParquetWriter(W.MessageType("lineitem", *[cols[n][0] for n in names]), path, None, decoder=dec, page_index=True)
        w.write_columns({n: cols[n][1] for n in names}, RG_ROWS)
        w.close()
        out["file_bytes"] = os.path.getsize(path)
        with ParquetFile(path) as f:
            idx = list(range(f.num_columns))
            types = [(f.columns[c].physical_type, f.columns[c].max_def, f.columns[c].max_rep) for c in idx]
            key_col, qty_col = names.index("l_orderkey"), names.index("l_quantity")
            keys = np.asarray(cols["l_orderkey"][1])
            qty = np.asarray(cols["l_quantity"][1] if not isinstance(cols["l_quantity"][1], tuple) else cols["l_quantity"][1][0])
            key = int(keys[RG_ROWS // 2 + 12345])
            one = 1.0 if qty.dtype.kind == "f" else 1
            cases = {"a_eq_orderkey": ([Eq("l_orderkey", key)], key_col, lambda v: v == key),
                     "b_quantity_le_1": ([Range("l_quantity", None, one)], qty_col, lambda v: v <= one)}

            def d2h(arrs):
                return int(sum(v.nbytes for a in arrs for v in a.values() if isinstance(v, np.ndarray)))

            def full(col, test):
                t0 = time.perf_counter()
                items, total = f.plan([0], idx)
                buf = dec.staging(total)
                descs = []
                for _rg, c, s, n, off in items:
                    f.read_into(s, n, buf.ptr.value + off)
                    descs.append(f.chunk_desc(0, c, off))
                t1 = time.perf_counter()
                dec.decode(descs, buf.ptr.value, total)
                assert dec.wait() == 0, dec.error()
                arrs = [dec.fetch(i, *types[i]) for i in range(len(idx))]
                down = d2h(arrs)
                v = arrs[col]["values"].view(DTYPES[types[col][0]])
                rows = np.flatnonzero(test(v))
                kept = [host_take(a, types[i][0], rows) for i, a in enumerate(arrs)]
                t2 = time.perf_counter()
                return kept, rows, sum(n for _rg, _c, _s, n, _o in items), total, down, (t1 - t0) * 1e3, (t2 - t1) * 1e3, 0.0

            def filtered(preds):
                t0 = time.perf_counter()
                span = f.prune_row_group(0, preds)
                items, total, wins = f.plan_rows(0, idx, span[0], span[1])
                buf = dec.staging(total)
                nread = f.read_rows(items, buf.ptr.value)
                t1 = time.perf_counter()
                native = bind(preds, f.columns, {c: i for i, c in enumerate(idx)})
                dec.decode([d for _c, d, _r, _o in items], buf.ptr.value, max(total, 1), windows=wins, predicates=native)
                assert dec.wait() == 0, dec.error()
                arrs = [dec.fetch(i, *types[i]) for i in range(len(idx))]
                rows_in, rows = dec.selection()
                t2 = time.perf_counter()
                return arrs, rows.astype(np.int64) + span[0], nread, total, d2h(arrs) + rows.nbytes, (t1 - t0) * 1e3, (t2 - t1) * 1e3, \
                    dec.filter_ms(), rows_in

            for name, (preds, col, test) in cases.items():
                res = {}
                for label, fn, reps in (("host_filter", lambda: full(col, test), args.full_reps), ("gpu_filter", lambda: filtered(preds), args.reps)):
                    rec = []
                    for r in range(args.warmup + reps):
                        got = fn()
                        if r >= args.warmup:
                            rec.append(got[5:8])
                    res[label] = got
                    line = {"file_bytes_read": int(got[2]), "h2d_bytes": int(got[3]), "d2h_bytes": int(got[4]), "rows_returned": int(len(got[1])),
                            "reps": reps, "read_ms": med([x[0] for x in rec]), "decode_fetch_ms": med([x[1] for x in rec]),
                            "decode_fetch_ms_min_max": [round(min(x[1] for x in rec), 4), round(max(x[1] for x in rec), 4)]}
                    if label == "gpu_filter":
                        line["filter_stage_ms"] = med([x[2] for x in rec])
                        line["rows_in"] = int(got[8])
                    out.setdefault(name, {})[label] = line
                # both routes return the same rows and the same bytes
                h, g = res["host_filter"], res["gpu_filter"]
                assert np.array_equal(h[1], g[1]), name
                for i in range(len(idx)):
                    for k, v in h[0][i].items():
                        assert np.array_equal(v.view(np.uint8), np.asarray(g[0][i][k]).view(np.uint8)), (name, names[i], k)
                hf, gf = out[name]["host_filter"], out[name]["gpu_filter"]
                out[name]["ratios_host_over_gpu"] = {k: round(hf[k] / max(gf[k], 1e-9), 1)
                                                     for k in ("file_bytes_read", "h2d_bytes", "d2h_bytes", "decode_fetch_ms")}
            out["key"] = key
    dec.close()
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()

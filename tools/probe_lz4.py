"""LZ4_RAW against ZSTD and Snappy on the same pages: two tables -- the 50,000-row table of
tests/test_gpu_lz4_pages.py, and the first 1 Mi rows of the lineitem table (seed 42, all 16 columns) --
each written by pyarrow as LZ4, ZSTD (level 3) and Snappy, chunk bytes resident on the device, decoded
REPS times after 5 warm-up decodes with HIP-event stage times. Prints, per table and codec, the
compressed chunk bytes and the median of stage snappy_exec (k_lz4 / k_zstd / the Snappy executor; for
Snappy the index pass, stage snappy_parse, is given beside it) and of the whole decode.

  python tools/probe_lz4.py [REPS]"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "parquet-floor_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import pyarrow.parquet as pq  # noqa: E402
from pfloor import _native, datagen  # noqa: E402
from pfloor.decoder import GpuDecoder, ParquetFile  # noqa: E402

WARMUP = 5
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_dir = os.environ.get("PF_BENCH_DIR", "/tmp/pfloor_bench")
os.makedirs(out_dir, exist_ok=True)


def test_table():
    import test_gpu_lz4_pages as T
    return T._table(), dict(use_dictionary=T.DICT_COLS, data_page_size=1 << 20, max_rows_per_page=T.ROWS, row_group_size=T.ROWS)


def lineitem():
    rows = 1 << 20
    return datagen.lineitem_table(rows, seed=42), dict(row_group_size=rows)


result = {}
L = _native.lib()
for tname, make in (("test_table", test_table), ("lineitem_1Mi", lineitem)):
    table, kw = make()
    result[tname] = {}
    for codec, ckw in (("lz4", dict(compression="LZ4")), ("zstd", dict(compression="zstd", compression_level=3)),
                       ("snappy", dict(compression="snappy"))):
        path = os.path.join(out_dir, f"probe_lz4_{tname}_{codec}.parquet")
        pq.write_table(table, path, **kw, **ckw)
        with ParquetFile(path) as pf, GpuDecoder(0) as dec:
            items, total = pf.plan([0], list(range(pf.num_columns)))
            host = np.zeros(max(total, 1), np.uint8)
            descs = []
            for rg, col, s, n, off in items:
                pf.read_into(s, n, host.ctypes.data + off)
                descs.append(pf.chunk_desc(rg, col, off))
            dptr = C.c_void_p()
            _native.check(L.pf_device_alloc(dec.h, total, C.byref(dptr)), dec.h, "pf_device_alloc")
            _native.check(L.pf_memcpy_h2d(dec.h, dptr, host.ctypes.data, total), dec.h, "pf_memcpy_h2d")
            dec.set_timing(True)
            runs = []
            for _ in range(WARMUP + reps):
                dec.decode(descs, dptr.value, total, on_device=True)
                rc = dec.wait()
                assert rc == 0, dec.error()
                runs.append(dec.timing())
            runs = runs[WARMUP:]
            med = lambda k: round(statistics.median(r[k] for r in runs), 4)   # noqa: E731
            result[tname][codec] = dict(chunk_bytes=int(sum(n for _rg, _c, _s, n, _o in items)), pages=sum(d.n_pages for d in descs),
                                        snappy_exec_ms=med("snappy_exec"), snappy_exec_min_ms=round(min(r["snappy_exec"] for r in runs), 4),
                                        snappy_parse_ms=med("snappy_parse"),
                                        total_ms=round(statistics.median(sum(r.values()) for r in runs), 4))
            L.pf_device_free(dec.h, dptr)
print(json.dumps(result))
